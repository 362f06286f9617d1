"""The order of the checks of the K/V-cache host layer, without a GPU: every rule of the argument builders broken on its own, and every
pair of rules that are neighbours in the check order broken together, over a handful of valid argument blocks - for the decode and the
prefill entry points alike. tests/golden/kvhost_matrix.txt holds, per case, the return values of the three *_plan entry points, the two
*_workspace_bytes entry points and *_rope_append_plan (an accepted plan as a short hash of its text), so a change of WHICH code wins
when two rules are broken at once shows as a changed line.

Nothing is ever launched: the pointers are fake. Valid blocks go through the *_plan and *_workspace_bytes entry points only; the
forwards and the appends are called only with blocks the plan call has just refused, so they return before any HIP call.

    python tests/test_kvhost_matrix_cpu.py --record     rewrites the fixture from the library of this tree
"""
import ctypes
import functools
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "kvhost_matrix.txt")
DUMMY = 1 << 20
INT_MAX = 2 ** 31 - 1
BIG = ctypes.c_size_t(-1).value

# valid blocks: fields of fasn_kvcache_args (`qlens`: the prefill block also carries q_seqlens). Every block has seqlen_add = Sq and is
# called with k_new / v_new, so the rotary plan is the one with the append.
BASES = {
    "dec_paged": dict(B=4, H=64, Hkv=8, Sq=1, D=64, page=256, max_pages=32, dtype=1, paged=True, qlens=False),
    "dec_dense": dict(B=3, H=8, Hkv=2, Sq=3, D=128, page=1000, max_pages=1, dtype=0, paged=False, qlens=False),
    "pre_paged_qlens": dict(B=2, H=12, Hkv=4, Sq=300, D=64, page=128, max_pages=40, dtype=1, paged=True, qlens=True),
    "pre_dense_oddpage": dict(B=2, H=16, Hkv=16, Sq=150, D=32, page=1001, max_pages=1, dtype=0, paged=False, qlens=False),
    "d256": dict(B=4, H=64, Hkv=8, Sq=1, D=256, page=256, max_pages=32, dtype=1, paged=True, qlens=False),
    "g128": dict(B=2, H=128, Hkv=1, Sq=1, D=64, page=64, max_pages=64, dtype=0, paged=True, qlens=False),
}
PAIR_BASES = ("dec_paged", "pre_paged_qlens")   # the paged blocks: every rule applies to them


class Case:
    """One call's operands: the argument block (`kv`; `null`: a NULL block), q_seqlens, and the operands of the ALiBi, window and rotary
    entry points. A rule is a function that breaks one check on it."""

    def __init__(self, L, c):
        B, H, Hkv, Sq, D = c["B"], c["H"], c["Hkv"], c["Sq"], c["D"]
        self.L, self.null = L, False
        self.pa = L.KvPrefillArgs()
        a = self.kv = self.pa.kv
        for v in (a.q, a.o):
            self._view(v, H, Sq, D)
        a.lse = DUMMY
        a.k_cache = a.v_cache = DUMMY
        for i, s in enumerate((c["page"] * Hkv * D, Hkv * D, D)):
            a.k_stride[i] = a.v_stride[i] = s
        a.block_table = DUMMY if c["paged"] else None
        a.block_table_stride, a.max_pages = c["max_pages"], c["max_pages"]
        a.seqlens, a.seqlen_add, a.page_size = DUMMY, Sq, c["page"]
        a.B, a.H, a.kv_group, a.Sq, a.D, a.dtype = B, H, H // Hkv, Sq, D, c["dtype"]
        a.scale, a.softmax_n, a.causal = D ** -0.5, 1.0, 1
        self.qlens = DUMMY + 4096 if c["qlens"] else None
        self.alibi = L.AlibiSlopes(slopes=DUMMY + 512, stride_b=0, stride_h=1)
        self.win = L.KvWindow(window=100, reserved=0)
        self.rope = L.KvRope(cos=DUMMY, sin=DUMMY, row_stride=16, rows=c["page"] * c["max_pages"], rotary_dim=32, table_dtype=2, interleaved=0)
        self.qo, self.kn, self.vn = (self._view(L.View4(), h, Sq, D) for h in (H, Hkv, Hkv))
        self.has_alibi = self.has_win = self.has_rope = True

    @staticmethod
    def _view(v, heads, Sq, D):
        v.ptr = DUMMY
        for i, s in enumerate((heads * Sq * D, Sq * D, D, 1)):
            v.stride[i] = s
        return v


def _set(**fields):
    def rule(c):
        for k, v in fields.items():
            setattr(c.kv, k, v)
    return rule


def _on(what, **fields):
    def rule(c):
        for k, v in fields.items():
            setattr(getattr(c, what), k, v)
    return rule


def _stride(what, i, value):
    def rule(c):
        getattr(c.kv, what).stride[i] = value
    return rule


def _cache_stride(what, i, value):
    def rule(c):
        getattr(c.kv, what)[i] = value(c.kv) if callable(value) else value
    return rule


def _attr(name, value):
    def rule(c):
        setattr(c, name, value)
    return rule


def _rows_over(c):   # decode: one row more than a workgroup has
    c.kv.Sq = 128 // c.kv.kv_group + 1
    c.kv.seqlen_add = c.kv.Sq


def _capacity(c, cap_paged, cap_dense):
    if c.kv.block_table:
        c.kv.page_size, c.kv.max_pages, c.kv.block_table_stride = 64, cap_paged // 64, cap_paged // 64
    else:
        c.kv.page_size = cap_dense


def _cap_over(c):
    _capacity(c, 2 ** 31, INT_MAX - 100)


def _cap_edge_add(c):   # the largest capacity, and 200 rows more: the decode bound looks at seqlen_add
    _capacity(c, 2 ** 31 - 192, INT_MAX - 128)
    c.kv.seqlen_add = 200


def _cap_edge_sq(c):   # ... the prefill bound looks at Sq
    _capacity(c, 2 ** 31 - 192, INT_MAX - 128)
    c.kv.Sq, c.kv.seqlen_add = 200, 0


def _grid_over(c):
    c.kv.B, c.kv.H = 1 << 16, c.kv.kv_group << 16


def _kn_only(c):
    c.vn = None


def _no_new_rows(c):
    c.kn = c.vn = None
    c.kv.seqlen_add = 0


# the rules of the builders in the order of their checks; the operand rules follow the base rules
BASE_RULES = [
    ("args_null", _attr("null", True)),
    ("B_0", _set(B=0)), ("H_0", _set(H=0)), ("Sq_0", _set(Sq=0)), ("D_0", _set(D=0)), ("page_0", _set(page_size=0)),
    ("dtype_f32", _set(dtype=2)),
    ("D_96", _set(D=96)),
    ("group_7", _set(kv_group=7)),
    ("n_negative", _set(softmax_n=-1.0)), ("scale_inf", _set(scale=float("inf"))),
    ("seqlens_null", _set(seqlens=None)), ("k_cache_null", _set(k_cache=None)), ("v_cache_null", _set(v_cache=None)),
    ("seqlens_odd", _set(seqlens=DUMMY + 2)), ("block_table_odd", _set(block_table=DUMMY + 2)), ("q_seqlens_odd", _attr("qlens", DUMMY + 2)),
    ("seqlen_add_other", lambda c: setattr(c.kv, "seqlen_add", c.kv.Sq + 1)),
    ("q_null", lambda c: setattr(c.kv.q, "ptr", None)),
    ("q_stride3", _stride("q", 3, 2)), ("q_odd", lambda c: setattr(c.kv.q, "ptr", DUMMY + 2)), ("q_stride_mod8", _stride("q", 1, 68)),
    ("o_null", lambda c: setattr(c.kv.o, "ptr", None)),
    ("o_stride3", _stride("o", 3, 2)), ("o_odd", lambda c: setattr(c.kv.o, "ptr", DUMMY + 2)), ("o_stride_mod8", _stride("o", 2, 68)),
    ("k_cache_odd", _set(k_cache=DUMMY + 8)), ("v_cache_odd", _set(v_cache=DUMMY + 8)),
    ("k_stride_mod8", _cache_stride("k_stride", 2, lambda a: a.D + 4)), ("v_stride_negative", _cache_stride("v_stride", 0, -8)),
    ("max_pages_0", _set(max_pages=0)), ("table_stride_short", lambda c: setattr(c.kv, "block_table_stride", c.kv.max_pages - 1)),
    ("page_48", _set(page_size=48)),
    ("rows_over", _rows_over), ("group_256", _set(kv_group=256, H=256)),
    ("capacity_over", _cap_over), ("capacity_plus_add", _cap_edge_add), ("capacity_plus_Sq", _cap_edge_sq),
    ("k_row_huge", _cache_stride("k_stride", 1, 1 << 24)), ("v_row_huge", _cache_stride("v_stride", 1, 1 << 24)),
    ("k_row_short", _cache_stride("k_stride", 1, lambda a: a.D - 8)), ("v_row_short", _cache_stride("v_stride", 1, lambda a: a.D - 8)),
    ("n_odd", _set(n=DUMMY + 2)), ("n_stride_negative", _set(n=DUMMY, n_stride_b=-1)), ("n_stride_over", _set(n=DUMMY, n_stride_b=1 << 31)),
    ("grid_over", _grid_over),
]
ALIBI_RULES = [
    ("alibi_null", _attr("has_alibi", False)), ("slopes_null", _on("alibi", slopes=None)), ("slopes_odd", _on("alibi", slopes=DUMMY + 2)),
    ("slope_stride_negative", _on("alibi", stride_h=-1)), ("slope_stride_over", _on("alibi", stride_b=1 << 31)),
]
WINDOW_RULES = [
    ("window_null", _attr("has_win", False)), ("window_0", _on("win", window=0)), ("window_reserved", _on("win", reserved=1)),
    ("not_causal", _set(causal=0)),
]
ROPE_RULES = [
    ("rope_null", _attr("has_rope", False)), ("cos_null", _on("rope", cos=None)), ("sin_null", _on("rope", sin=None)),
    ("q_out_null", _attr("qo", None)),
    ("k_new_alone", _kn_only),
    ("seqlen_add_0", _set(seqlen_add=0)),
    ("rotary_dim_8", _on("rope", rotary_dim=8)), ("rotary_dim_over", lambda c: setattr(c.rope, "rotary_dim", c.kv.D + 16)),
    ("rotary_dim_24", _on("rope", rotary_dim=24)),
    ("table_rows_short", lambda c: setattr(c.rope, "rows", c.rope.rows - 1)),
    ("interleaved_2", _on("rope", interleaved=2)),
    ("table_dtype_other", lambda c: setattr(c.rope, "table_dtype", 1 - c.kv.dtype)),
    ("table_rows_overlap", _on("rope", row_stride=8)),
    ("cos_odd", _on("rope", cos=DUMMY + 4)), ("sin_odd", _on("rope", sin=DUMMY + 8)), ("table_stride_odd", _on("rope", row_stride=18)),
    ("q_out_stride3", lambda c: c.qo.stride.__setitem__(3, 2)), ("q_out_odd", lambda c: setattr(c.qo, "ptr", DUMMY + 2)),
    ("k_new_stride3", lambda c: c.kn.stride.__setitem__(3, 2)), ("v_new_odd", lambda c: setattr(c.vn, "ptr", DUMMY + 2)),
    ("no_new_rows", _no_new_rows),   # (valid: the queries alone are rotated)
]
CHAINS = [BASE_RULES] + [[BASE_RULES[-1]] + tail for tail in (ALIBI_RULES, WINDOW_RULES, ROPE_RULES)]


def cases():
    """(name, base block, rules to apply) in the order of the fixture's lines"""
    out = [(name, name, ()) for name in BASES]
    singles = BASE_RULES + ALIBI_RULES + WINDOW_RULES + ROPE_RULES
    for base in BASES:
        out += [(f"{base}+{n}", base, (fn,)) for n, fn in singles]
    for base in PAIR_BASES:
        for chain in CHAINS:
            out += [(f"{base}+{n1}+{n2}", base, (f1, f2)) for (n1, f1), (n2, f2) in zip(chain, chain[1:])]
    return out


def _plan(fn, *operands):
    buf = ctypes.create_string_buffer(4096)
    rc = fn(*operands, buf, len(buf))
    if rc < 0:
        return str(rc)
    assert rc == len(buf.value) > 0
    return "#" + hashlib.sha1(buf.value).hexdigest()[:8]


def _record(lib, c, stem):
    args = None if c.null else (c.kv if stem == "kvcache" else c.pa)
    alibi, win, rope = c.alibi if c.has_alibi else None, c.win if c.has_win else None, c.rope if c.has_rope else None
    c.pa.q_seqlens = c.qlens
    f = lambda name: getattr(lib, name.replace("KV", stem))   # noqa: E731
    base = _plan(f("fasn_KV_plan"), args)
    got = [base, _plan(f("fasn_KV_alibi_plan"), args, alibi), _plan(f("fasn_KV_window_plan"), args, win),
           str(f("fasn_fwd_KV_workspace_bytes")(args)), str(f("fasn_fwd_KV_window_workspace_bytes")(args, win)),
           _plan(f("fasn_KV_rope_append_plan"), args, rope, c.qo, c.kn, c.vn)]
    if base.startswith("-"):   # the block itself is refused: the calls that would launch return the same way, before any HIP call
        got.append("fwd=" + ",".join(str(rc) for rc in (
            f("fasn_fwd_KV")(args, 256, BIG, None), f("fasn_fwd_KV_alibi")(args, alibi, 256, BIG, None),
            f("fasn_fwd_KV_window")(args, win, 256, BIG, None), f("fasn_KV_append")(args, c.kn, c.vn, None))))
    return " ".join(got)


@functools.lru_cache(maxsize=None)
def matrix(pkg):
    L, lib = pkg._lib, pkg._lib.load()
    lines = []
    for name, base, rules in cases():
        sides = []
        for stem in ("kvcache", "kvprefill"):
            c = Case(L, BASES[base])
            for rule in rules:
                rule(c)
            sides.append(_record(lib, c, stem))
        lines.append(f"{name} | decode {sides[0]} | prefill {sides[1]}")
    return lines


def test_return_codes_and_plans_equal_the_recorded_matrix(pkg):
    want = open(FIXTURE).read().splitlines()
    got = matrix(pkg)
    assert len(got) == len(want) == len(cases()) and len(set(line.split(" | ")[0] for line in got)) == len(got)
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, f"{len(diff)} of {len(got)} cases moved; the first (got, recorded): {diff[:3]}"


def test_every_base_block_is_valid_where_it_is_meant_to_be(pkg):
    """the fixture is only worth something if the blocks the rules are broken on are accepted to begin with"""
    rows = dict(line.split(" | ", 1) for line in matrix(pkg)[:len(BASES)])
    for name in BASES:
        dec, pre = rows[name].split(" | ")
        assert "-" not in pre, (name, pre)                       # every block is a valid prefill
        assert ("-" not in dec) == (not name.startswith("pre_")), (name, dec)   # the prefill blocks exceed the decode row limit


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path.insert(0, ROOT)
    import flash_attention_softmax_n_amd
    text = matrix(flash_attention_softmax_n_amd)
    with open(FIXTURE, "w") as fh:
        fh.write("\n".join(text) + "\n")
    print(f"recorded {len(text)} cases in {FIXTURE}")
