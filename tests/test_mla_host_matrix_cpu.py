"""The order of the checks of the MLA host layer, without a GPU, for the five entry-point families mla, mla_fp8, mla_sparse,
mla_sparse_fp8 and mla_index: every rule of mla_build, of the FP8 and the index-list operands (both row formats) and of index_build
broken on its own, and every pair of rules that are neighbours in the check order broken together, over a handful of valid argument
blocks. tests/golden/mla_host_matrix.txt holds, per case, the return of the *_plan entry point (an accepted plan as a short hash of its
text), the *_workspace_bytes value, the returns of the forward with a NULL workspace and with one off 16 bytes, and the returns of the
append with a NULL view and with a view that breaks the stride rule - so a change of WHICH code wins when two rules are broken at once
shows as a changed line. tests/golden/mla_python_refusals.txt holds the exception type and the full message of a table of refusing calls
of the five public functions on CPU tensors, which reaches every `raise` of mla.py's call paths.

Nothing is ever launched: the pointers are fake. A forward is only called with a workspace it refuses (NULL, or off 16 bytes: both
checks come behind the block's and in front of any HIP call) and an append only with new rows it refuses (NULL, or a feature stride
of 2), so whatever the block, they return before any HIP call. The indexer with a caller's logits buffer needs no workspace: its
forward is called only where the plan call has just refused the block.

    python tests/test_mla_host_matrix_cpu.py --record     rewrites both fixtures from the library and the package of this tree
"""
import ctypes
import functools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mla_host_matrix.txt")
PY_FIXTURE = os.path.join(ROOT, "tests", "golden", "mla_python_refusals.txt")
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]   # (ROOT: mla_support's helpers import the package when this file is run as a script)
from kv_args import BIG, INT_MAX, _plan   # noqa: E402
from mla_support import BASE, _args, _fp8, _index_args, _sparse   # noqa: E402

NAN, INF = float("nan"), float("inf")
FAMILIES = ("mla", "mla_fp8", "mla_sparse", "mla_sparse_fp8")

# valid blocks: paged and dense, bf16 and fp16, Sq = 1 and 2, with and without a per-head n; kv_stride follows the family's row
MLA_BASES = {
    "paged_bf16_sq2": dict(B=2, H=16, Sq=2, dtype=1, page=64, pages=4, paged=True, n=False),
    "dense_f16_sq1": dict(B=3, H=5, Sq=1, dtype=0, page=200, pages=1, paged=False, n=False),
    "paged_f16_sq1_n": dict(B=2, H=128, Sq=1, dtype=0, page=128, pages=8, paged=True, n=True),
}
MLA_PAIR_BASES = ("paged_bf16_sq2", "paged_f16_sq1_n")
INDEX_BASES = {
    "paged_bf16_hi64_sq2": dict(B=3, Hi=64, Sq=2, dtype=1, page=64, pages=96, paged=True, logits=False, topk=2048),
    "dense_f16_hi32_sq1_logits": dict(B=2, Hi=32, Sq=1, dtype=0, page=1000, pages=1, paged=False, logits=True, topk=64),
    "paged_bf16_hi32_sq2_logits": dict(B=3, Hi=32, Sq=2, dtype=1, page=64, pages=96, paged=True, logits=True, topk=2048),
}
INDEX_PAIR_BASES = ("paged_bf16_hi64_sq2", "paged_bf16_hi32_sq2_logits")


class Case:
    """One call's operands: the block `a` (`null`: a NULL block), the FP8 operand `f` and the index list `x` (`has_op`: False passes
    NULL in their place), the new rows' view. A rule is a function that breaks one check on it."""

    def __init__(self, pkg, family, base):
        self.family, self.null, self.has_op = family, False, True
        self.view = pkg._lib.View4()
        self.view.ptr = BASE
        if family == "mla_index":
            c = INDEX_BASES[base]
            B, Hi, Sq, cap = c["B"], c["Hi"], c["Sq"], c["page"] * c["pages"]
            self.a = a = _index_args(pkg, B=B, Hi=Hi, Sq=Sq, dtype=c["dtype"], page_size=c["page"], max_pages=c["pages"], topk=c["topk"],
                                     block_table=BASE if c["paged"] else None, block_table_stride=c["pages"] if c["paged"] else 0,
                                     logits=BASE if c["logits"] else None)
            for i, s in enumerate((Hi * Sq * 128, Sq * 128, 128, 1)):
                a.q.stride[i] = s
            a.w_stride[0], a.w_stride[1], a.w_stride[2] = Hi * Sq, Sq, 1
            a.k_stride[0], a.k_stride[1] = c["page"] * 128, 128
            a.indices_stride[0], a.indices_stride[1] = Sq * c["topk"], c["topk"]
            a.logits_stride[0], a.logits_stride[1] = Sq * cap, cap
            self.row = 128
        else:
            c = MLA_BASES[base]
            B, H, Sq = c["B"], c["H"], c["Sq"]
            self.row = 656 if family == "mla_sparse_fp8" else 576   # elements of a cache row: bytes under the 656-byte rows
            self.eb = 1 if family in ("mla_fp8", "mla_sparse_fp8") else 2
            self.a = a = _args(pkg, B=B, H=H, Sq=Sq, dtype=c["dtype"], page_size=c["page"], max_pages=c["pages"],
                               block_table=BASE if c["paged"] else None, block_table_stride=c["pages"] if c["paged"] else 0)
            for v, d in ((a.q, 576), (a.o, 512)):
                for i, s in enumerate((H * Sq * d, Sq * d, d, 1)):
                    v.stride[i] = s
            a.kv_stride[0], a.kv_stride[1] = c["page"] * self.row, self.row
            if c["n"]:
                a.n, a.n_stride_b, a.n_stride_h = BASE, H, 1
            self.f = _fp8(pkg)
            self.x = _sparse(pkg)
        for i, s in enumerate((Sq * self.row, self.row, self.row, 1)):
            self.view.stride[i] = s


def _set(**fields):
    def rule(c):
        for k, v in fields.items():
            setattr(c.a, k, v(c) if callable(v) else v)
    return rule


def _on(what, **fields):
    def rule(c):
        for k, v in fields.items():
            setattr(getattr(c, what), k, v(c) if callable(v) else v)
    return rule


def _attr(name, value):
    def rule(c):
        setattr(c, name, value)
    return rule


def _arr(what, i, value):
    """member `what` of the block is an array (or `view.stride`): element i"""
    def rule(c):
        tgt = c.a
        for part in what.split("."):
            tgt = getattr(tgt, part)
        tgt[i] = value(c, tgt[i]) if callable(value) else value
    return rule


def _ptr(view, value):
    def rule(c):
        getattr(c.a, view).ptr = value
    return rule


def _capacity(paged_cap, dense_cap, **more):
    def rule(c):
        if c.a.block_table:
            c.a.page_size, c.a.max_pages, c.a.block_table_stride = 64, paged_cap // 64, paged_cap // 64
        else:
            c.a.page_size = dense_cap
        for k, v in more.items():
            setattr(c.a, k, v)
    return rule


def _view_rules(v):
    return [(f"{v}_null", _ptr(v, None)), (f"{v}_stride3", _arr(f"{v}.stride", 3, 2)), (f"{v}_odd", _ptr(v, BASE + 2)),
            (f"{v}_stride_mod8", _arr(f"{v}.stride", 1, lambda c, s: s + 4))]


# the rules of mla_build in the order of its checks ...
MLA_RULES = [
    ("args_null", _attr("null", True)),
    ("B_0", _set(B=0)), ("H_0", _set(H=0)), ("Sq_0", _set(Sq=0)), ("D_0", _set(D=0)), ("Dv_0", _set(Dv=0)), ("page_0", _set(page_size=0)),
    ("reserved_1", _set(reserved=1)),
    ("dtype_f32", _set(dtype=2)),
    ("D_640", _set(D=640)), ("Dv_576", _set(Dv=576)),
    ("n_negative", _set(softmax_n=-1.0)), ("n_nan", _set(softmax_n=NAN)), ("scale_inf", _set(scale=INF)),
    ("seqlens_null", _set(seqlens=None)), ("kv_cache_null", _set(kv_cache=None)),
    ("max_pages_0", _set(max_pages=0)), ("table_stride_short", _set(block_table_stride=lambda c: c.a.max_pages - 1)),
    ("capacity_over", _capacity(2 ** 31, INT_MAX - 100)), ("capacity_plus_add", _capacity(2 ** 31 - 192, INT_MAX - 128, seqlen_add=200)),
    ("seqlen_add_negative", _set(seqlen_add=-1)),
    ("kv_page_stride_negative", _arr("kv_stride", 0, -16)), ("kv_row_short", _arr("kv_stride", 1, lambda c, s: c.row - 16)),
    ("kv_row_576", _arr("kv_stride", 1, 576)),   # (valid over 576-element rows; too short under the 656-byte rows)
    ("n_stride_negative", _set(n=BASE, n_stride_b=-1)), ("n_stride_over", _set(n=BASE, n_stride_b=1 << 31)),
    ("rows_over", _set(H=129, Sq=2)),
    ("page_48", _set(page_size=48)),
    ("kv_row_huge", _arr("kv_stride", 1, 1 << 25)),
    ("f16_scale_6", _set(dtype=0, scale=6.0)),
    *_view_rules("q"), *_view_rules("o"),
    ("kv_cache_odd", _set(kv_cache=BASE + 8)),
    ("kv_page_stride_plus8", _arr("kv_stride", 0, lambda c, s: s + 8)), ("kv_page_stride_plus4", _arr("kv_stride", 0, lambda c, s: s + 4)),
    ("kv_row_plus8", _arr("kv_stride", 1, lambda c, s: s + 8)),   # (16 bytes at element size 2, off 16 bytes at element size 1)
    ("kv_row_plus4", _arr("kv_stride", 1, lambda c, s: s + 4)),
    ("seqlens_odd", _set(seqlens=BASE + 2)), ("block_table_odd", _set(block_table=BASE + 2)), ("n_odd", _set(n=BASE + 2)),
    ("grid_over", _set(B=1 << 24)),
]
# ... then the operand's
FP8_RULES = [
    ("fp8_null", _attr("has_op", False)), ("scale_null", _on("f", kv_scale=None)), ("fp8_reserved", _on("f", reserved=1)),
    ("sb_negative", _on("f", sb=-1)), ("sb_over", _on("f", sb=1 << 31)), ("sb_span_over", _on("f", sb=lambda c: -(-(1 << 31) // (c.a.B - 1)))),
    ("scale_odd", _on("f", kv_scale=BASE + 2)),
]
SPARSE_RULES = [
    ("sparse_null", _attr("has_op", False)), ("indices_null", _on("x", indices=None)), ("sparse_reserved", _on("x", reserved=1)),
    ("topk_0", _on("x", topk=0)), ("topk_negative", _on("x", topk=-64)),
    ("stride_b_negative", _on("x", stride_b=-1)), ("stride_q_negative", _on("x", stride_q=-1)),
    ("stride_b_over", _on("x", stride_b=1 << 31)), ("stride_q_over", _on("x", stride_q=1 << 31)), ("span_over", _on("x", stride_b=(1 << 31) - 64)),
    ("topk_96", _on("x", topk=96)), ("topk_2080", _on("x", topk=2080)),
    ("indices_odd", _on("x", indices=BASE + 2)),
    ("sparse_grid_over", _set(B=1 << 16, H=1, Sq=256)),   # (B * Sq * head blocks: the dense grid of the same block fits)
]
OPERAND_RULES = {"mla": [], "mla_fp8": FP8_RULES, "mla_sparse": SPARSE_RULES, "mla_sparse_fp8": SPARSE_RULES}

# the rules of index_build in the order of its checks
INDEX_RULES = [
    ("args_null", _attr("null", True)),
    ("B_0", _set(B=0)), ("Hi_0", _set(Hi=0)), ("Sq_0", _set(Sq=0)), ("D_0", _set(D=0)), ("page_0", _set(page_size=0)), ("topk_0", _set(topk=0)),
    ("reserved_1", _set(reserved=1)),
    ("dtype_f32", _set(dtype=2)),
    ("D_64", _set(D=64)),
    ("seqlens_null", _set(seqlens=None)), ("k_cache_null", _set(k_cache=None)), ("w_null", _set(w=None)), ("indices_null", _set(indices=None)),
    ("max_pages_0", _set(max_pages=0)), ("table_stride_short", _set(block_table_stride=lambda c: c.a.max_pages - 1)),
    ("capacity_over", _capacity((1 << 30) + 64, (1 << 30) + 1)), ("capacity_edge", _capacity(1 << 30, 1 << 30)),   # (the edge is served)
    ("seqlen_add_negative", _set(seqlen_add=-1)),
    ("k_page_stride_negative", _arr("k_stride", 0, -8)), ("k_row_short", _arr("k_stride", 1, 120)),
    ("w_stride0_negative", _arr("w_stride", 0, -1)), ("w_stride1_negative", _arr("w_stride", 1, -1)), ("w_stride2_negative", _arr("w_stride", 2, -1)),
    ("indices_stride0_negative", _arr("indices_stride", 0, -1)), ("indices_stride1_negative", _arr("indices_stride", 1, -1)),
    ("indices_row_short", _arr("indices_stride", 1, lambda c, s: c.a.topk - 1)),
    ("logits_stride0_negative", _arr("logits_stride", 0, -1)), ("logits_stride1_negative", _arr("logits_stride", 1, -1)),
    ("logits_row_short", _arr("logits_stride", 1, lambda c, s: s - 1)),
    ("Hi_48", _set(Hi=48)), ("topk_96", _set(topk=96)), ("page_48", _set(page_size=48)),
    *_view_rules("q"),
    ("k_cache_odd", _set(k_cache=BASE + 8)), ("k_page_stride_mod8", _arr("k_stride", 0, lambda c, s: s + 4)),
    ("k_row_mod8", _arr("k_stride", 1, 132)),
    ("seqlens_odd", _set(seqlens=BASE + 2)), ("block_table_odd", _set(block_table=BASE + 2)), ("w_odd", _set(w=BASE + 2)),
    ("indices_odd", _set(indices=BASE + 2)), ("logits_odd", _set(logits=BASE + 2)),
    ("grid_over", _set(B=INT_MAX)),
]


def cases():
    """(name, family, base block, rules to apply) in the order of the fixture's lines"""
    out = []
    for fam in FAMILIES + ("mla_index",):
        index = fam == "mla_index"
        bases, pair_bases = (INDEX_BASES, INDEX_PAIR_BASES) if index else (MLA_BASES, MLA_PAIR_BASES)
        chain = INDEX_RULES if index else MLA_RULES + OPERAND_RULES[fam]
        out += [(f"{fam}/{b}", fam, b, ()) for b in bases]
        for b in bases:
            out += [(f"{fam}/{b}+{n}", fam, b, (fn,)) for n, fn in chain]
        for b in pair_bases:
            out += [(f"{fam}/{b}+{n1}+{n2}", fam, b, (f1, f2)) for (n1, f1), (n2, f2) in zip(chain, chain[1:])]
    return out


def _record(lib, c):
    fam = c.family
    a = None if c.null else c.a
    op = () if fam in ("mla", "mla_index") else (None,) if not c.has_op else (c.f,) if fam == "mla_fp8" else (c.x,)
    plan = _plan(getattr(lib, f"fasn_{fam}_plan"), a, *op)
    got = [plan, str(getattr(lib, f"fasn_{fam}_workspace_bytes")(a, *op))]
    fwd = lib.fasn_mla_index if fam == "mla_index" else getattr(lib, f"fasn_fwd_{fam}")
    if fam != "mla_index" or plan.startswith("-") or not c.a.logits:   # (the indexer with a logits buffer takes no workspace to refuse)
        got.append(f"fwd={fwd(a, *op, None, 0, None)},{fwd(a, *op, BASE + 8, BIG, None)}")
    if fam != "mla_sparse":   # (no append of its own: the 16-bit cache's serves it)
        append = getattr(lib, f"fasn_{fam}_append")
        app_op = op if fam == "mla_fp8" else ()   # (the 656-byte rows' append takes no list)
        bad = type(c.view).from_buffer_copy(c.view)
        bad.stride[3] = 2
        got.append(f"append={append(a, *app_op, None, None)},{append(a, *app_op, bad, None)}")
    return " ".join(got)


@functools.lru_cache(maxsize=None)
def matrix(pkg):
    lib, lines = pkg._lib.load(), []
    for name, fam, base, rules in cases():
        c = Case(pkg, fam, base)
        for rule in rules:
            rule(c)
        lines.append(f"{name} | {_record(lib, c)}")
    return lines


def test_return_codes_and_plans_equal_the_recorded_matrix(pkg):
    want = open(FIXTURE).read().splitlines()
    got = matrix(pkg)
    assert len(got) == len(want) == len(cases()) and len(set(line.split(" | ")[0] for line in got)) == len(got)
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, f"{len(diff)} of {len(got)} cases moved; the first (got, recorded): {diff[:3]}"


def test_every_base_block_is_valid_and_every_rule_breaks_one(pkg):
    """the fixture is only worth something if the blocks the rules are broken on are accepted to begin with, a forward of an accepted
    block stops at the workspace (FASN_EWORKSPACE, then FASN_EALIGN) and its append at the new rows (FASN_EINVAL, then FASN_ESTRIDE),
    and each rule is refused on at least one block"""
    rows = dict(line.split(" | ", 1) for line in matrix(pkg))
    for name, fam, base, rules in cases():
        if not rules:
            takes_ws = not (fam == "mla_index" and INDEX_BASES[base]["logits"])
            fields = rows[name].split()
            assert fields[0].startswith("#") and [f for f in fields if f.startswith("fwd=")] == ["fwd=-8,-4"] * takes_ws, (name, rows[name])
            assert fam == "mla_sparse" or fields[-1] == "append=-1,-5", (name, rows[name])
    singles = {}
    for name, fam, base, rules in cases():
        if len(rules) == 1:
            singles.setdefault((fam, name.split("+")[1]), []).append(rows[name].startswith("-"))
    valid_on_purpose = {"kv_row_576", "kv_page_stride_plus8", "kv_row_plus8", "capacity_edge", "sparse_grid_over"}   # refused by some families only
    never = sorted(k for k, v in singles.items() if not any(v) and k[1] not in valid_on_purpose)
    assert not never, never
    for rule, fams in (("kv_row_576", ("mla_sparse_fp8",)), ("kv_row_plus8", ("mla_fp8", "mla_sparse_fp8")),
                       ("kv_page_stride_plus8", ("mla_fp8", "mla_sparse_fp8")), ("sparse_grid_over", ("mla_sparse", "mla_sparse_fp8"))):
        assert sorted(f for f in FAMILIES if any(singles.get((f, rule), []))) == sorted(fams), rule


# ---------------------------------------------------------------- the Python refusals
F16, BF16, F32, I32 = torch.float16, torch.bfloat16, torch.float32, torch.int32
F8, U8 = torch.float8_e4m3fn, torch.uint8
SKIP = object()   # what a callable operand returns where the function has no such operand
PY_FAMILIES = ("flash_attention_n_mla", "flash_attention_n_mla_fp8", "flash_attention_n_mla_sparse", "flash_attention_n_mla_sparse_fp8")


def _z(*shape, dtype=F16):
    return torch.zeros(*shape, dtype=dtype)


def _mla_operands(fn):
    """keyword operands every check of `fn` accepts, up to the CPU refusal: B = 1, H = 4, Sq = 2, two pages of 64 rows, one named"""
    fp8, sparse, rows8 = fn.endswith("mla_fp8"), "sparse" in fn, fn.endswith("sparse_fp8")
    row = 656 if rows8 else 576
    d = dict(query=_z(1, 4, 2, 576), kv_cache=_z(2, 64, 1, row, dtype=U8 if rows8 else F8 if fp8 else F16), cache_seqlens=_z(1, dtype=I32),
             scale=0.1, block_table=_z(1, 1, dtype=I32))
    if fp8:
        d["kv_scale"] = 1.0
    if sparse:
        d["indices"] = _z(1, 2, 64, dtype=I32)
    return d


def _index_operands(fn):
    return dict(q_index=_z(1, 32, 2, 128), weights=_z(1, 32, 2, dtype=F32), k_cache=_z(2, 64, 1, 128), cache_seqlens=_z(1, dtype=I32), topk=64,
                block_table=_z(1, 1, dtype=I32))


def _cache_as(dtype):
    return lambda d: _z(*d["kv_cache"].shape, dtype=dtype)


def _padded(key, pad_bytes=8):
    """the tensor's last axis cut out of a wider buffer: rows off 16 bytes"""
    def make(d):
        t = d[key]
        return _z(*t.shape[:-1], t.shape[-1] + pad_bytes // t.element_size(), dtype=t.dtype)[..., :t.shape[-1]]
    return make


def _grad(key):
    return lambda d: d[key].clone().requires_grad_()


def _indices_too(d):
    return d["indices"].to("meta") if "indices" in d else SKIP


def _meta(*keys):
    return {k: (lambda d, k=k: d[k].to("meta")) for k in keys}


ALL, SPARSE_FNS = PY_FAMILIES, PY_FAMILIES[2:]
# (case, the functions it is run on, operands replaced - a callable gets the valid operands)
MLA_PY_CASES = [
    ("valid", ALL, {}),
    ("valid_3d_cache", ALL, dict(kv_cache=lambda d: d["kv_cache"][:, :, 0])),
    ("valid_kv_new_n_none", ALL, dict(kv_new=_z(1, 2, 1, 576), softmax_n_param=None)),
    ("valid_n_tensor_not_causal", ALL, dict(softmax_n_param=torch.ones(1, 4), is_causal=False, return_lse=True)),
    ("query_none", ALL, dict(query=None)), ("query_3d", ALL, dict(query=_z(4, 2, 576))),
    ("cache_none", ALL, dict(kv_cache=None)), ("cache_2d", ALL, dict(kv_cache=_z(64, 576))),
    ("cache_f16", ALL, dict(kv_cache=_cache_as(F16))), ("cache_bf16", ALL, dict(kv_cache=_cache_as(BF16))),
    ("cache_f32", ALL, dict(kv_cache=_cache_as(F32))), ("cache_u8", ALL, dict(kv_cache=_cache_as(U8))),
    ("cache_e4m3fn", ALL, dict(kv_cache=_cache_as(F8))), ("cache_e5m2", ALL, dict(kv_cache=_cache_as(torch.float8_e5m2))),
    ("cache_e4m3fnuz", ALL, dict(kv_cache=_cache_as(torch.float8_e4m3fnuz))),
    ("head_dim_128", ALL, dict(query=_z(1, 4, 2, 128), kv_cache=lambda d: _z(2, 64, 1, 128, dtype=d["kv_cache"].dtype))),
    ("row_of_the_other_format", ALL, dict(kv_cache=lambda d: _z(2, 64, 1, 576 + 656 - d["kv_cache"].shape[3], dtype=d["kv_cache"].dtype))),
    ("cache_two_heads", ALL, dict(kv_cache=lambda d: _z(2, 64, 2, d["kv_cache"].shape[3], dtype=d["kv_cache"].dtype))),
    ("query_f32", ALL, dict(query=_z(1, 4, 2, 576, dtype=F32))),
    ("query_f32_cache_f32", ALL, dict(query=_z(1, 4, 2, 576, dtype=F32), kv_cache=_cache_as(F32))),
    ("query_bf16", ALL, dict(query=_z(1, 4, 2, 576, dtype=BF16))),
    ("rows_over", ALL, dict(query=_z(1, 129, 2, 576))),
    ("scale_none", ALL, dict(scale=None)), ("scale_bool", ALL, dict(scale=True)), ("scale_tensor", ALL, dict(scale=torch.tensor(0.1))),
    ("scale_int", ALL, dict(scale=1)),
    ("f16_scale_6", ALL, dict(scale=6.0)), ("f16_scale_nan", ALL, dict(scale=NAN)),
    ("bf16_scale_6", ALL, dict(query=_z(1, 4, 2, 576, dtype=BF16), scale=6.0, kv_cache=lambda d: d["kv_cache"] if d["kv_cache"].dtype != F16 else _cache_as(BF16)(d))),
    ("indices_none", SPARSE_FNS, dict(indices=None)), ("indices_int64", SPARSE_FNS, dict(indices=_z(1, 2, 64, dtype=torch.int64))),
    ("indices_one_position", SPARSE_FNS, dict(indices=_z(1, 1, 64, dtype=I32))), ("indices_2d", SPARSE_FNS, dict(indices=_z(2, 64, dtype=I32))),
    ("indices_4d", SPARSE_FNS, dict(indices=_z(1, 2, 64, 1, dtype=I32))), ("indices_strided", SPARSE_FNS, dict(indices=_z(1, 2, 128, dtype=I32)[..., ::2])),
    ("topk_96", SPARSE_FNS, dict(indices=_z(1, 2, 96, dtype=I32))), ("topk_32", SPARSE_FNS, dict(indices=_z(1, 2, 32, dtype=I32))),
    ("topk_0", SPARSE_FNS, dict(indices=_z(1, 2, 0, dtype=I32))),
    ("query_elsewhere", ALL, _meta("query")),
    ("indices_left_behind", SPARSE_FNS, _meta("query", "kv_cache", "cache_seqlens", "block_table")),
    ("lens_left_behind", ALL, {**_meta("query", "kv_cache", "block_table"), "indices": _indices_too}),
    ("table_left_behind", ALL, {**_meta("query", "kv_cache", "cache_seqlens"), "indices": _indices_too}),
    ("kv_new_left_behind", ALL, {**_meta("query", "kv_cache", "cache_seqlens", "block_table"), "kv_new": _z(1, 2, 1, 576),
                                 "indices": _indices_too}),
    ("query_grad", ALL, dict(query=_grad("query"))), ("kv_new_grad", ALL, dict(kv_new=_z(1, 2, 1, 576).requires_grad_())),
    ("cache_grad", ("flash_attention_n_mla", "flash_attention_n_mla_sparse"), dict(kv_cache=_grad("kv_cache"))),
    ("n_grad", ALL, dict(softmax_n_param=torch.ones(1, 4).requires_grad_())),
    ("lens_int64", ALL, dict(cache_seqlens=_z(1, dtype=torch.int64))), ("lens_two", ALL, dict(cache_seqlens=_z(2, dtype=I32))),
    ("lens_2d", ALL, dict(cache_seqlens=_z(1, 1, dtype=I32))), ("lens_strided", ALL, dict(cache_seqlens=_z(2, dtype=I32)[::2])),
    ("table_int64", ALL, dict(block_table=_z(1, 1, dtype=torch.int64))), ("table_1d", ALL, dict(block_table=_z(1, dtype=I32))),
    ("table_two_rows", ALL, dict(block_table=_z(2, 1, dtype=I32))), ("table_no_column", ALL, dict(block_table=_z(1, 0, dtype=I32))),
    ("table_strided", ALL, dict(block_table=_z(1, 2, dtype=I32)[:, ::2])),
    ("page_48", ALL, dict(kv_cache=lambda d: _z(2, 48, 1, d["kv_cache"].shape[3], dtype=d["kv_cache"].dtype))),
    ("dense_two_for_one", ALL, dict(block_table=None)),
    ("dense_valid", ALL, dict(block_table=None, kv_cache=lambda d: d["kv_cache"][:1])),
    ("cache_rows_off_16_bytes", ALL, dict(kv_cache=_padded("kv_cache"))),
    ("cache_feature_stride_2", ALL, dict(kv_cache=lambda d: _z(2, 64, 1, 2 * d["kv_cache"].shape[3], dtype=d["kv_cache"].dtype)[..., ::2])),
    ("cache_rows_overlap", ALL, dict(kv_cache=lambda d: d["kv_cache"][:, :1].expand(2, 64, 1, d["kv_cache"].shape[3]))),
    ("kv_new_bf16", ALL, dict(kv_new=_z(1, 2, 1, 576, dtype=BF16))), ("kv_new_512", ALL, dict(kv_new=_z(1, 2, 1, 512))),
    ("kv_new_one_position", ALL, dict(kv_new=_z(1, 1, 1, 576))), ("kv_new_3d", ALL, dict(kv_new=_z(1, 2, 576))),
    ("kv_new_656", ("flash_attention_n_mla_sparse_fp8",), dict(kv_new=_z(1, 2, 1, 656, dtype=U8))),
    ("kv_scale_none", PY_FAMILIES[1:2], dict(kv_scale=None)), ("kv_scale_int_tensor", PY_FAMILIES[1:2], dict(kv_scale=torch.ones(1, dtype=I32))),
    ("kv_scale_three", PY_FAMILIES[1:2], dict(kv_scale=torch.ones(3))), ("kv_scale_3d", PY_FAMILIES[1:2], dict(kv_scale=torch.ones(1, 1, 1))),
    ("kv_scale_grad", PY_FAMILIES[1:2], dict(kv_scale=torch.ones(1).requires_grad_())),
    ("kv_scale_1d_valid", PY_FAMILIES[1:2], dict(kv_scale=torch.ones(1))), ("kv_scale_bool", PY_FAMILIES[1:2], dict(kv_scale=True)),
    ("n_negative", ALL, dict(softmax_n_param=-1.0)), ("n_tensor_int", ALL, dict(softmax_n_param=torch.ones(1, 4, dtype=I32))),
    ("n_tensor_three_heads", ALL, dict(softmax_n_param=torch.ones(1, 3))),
]
INDEX_FN = "flash_attention_n_mla_index"
INDEX_PY_CASES = [
    ("valid", {}), ("valid_3d_cache", dict(k_cache=lambda d: d["k_cache"][:, :, 0])),
    ("valid_k_new_logits", dict(k_new=_z(1, 2, 1, 128), return_logits=True, is_causal=False)),
    ("q_none", dict(q_index=None)), ("q_3d", dict(q_index=_z(32, 2, 128))), ("cache_none", dict(k_cache=None)), ("cache_2d", dict(k_cache=_z(64, 128))),
    ("q_e4m3fn", dict(q_index=_z(1, 32, 2, 128, dtype=F8))), ("cache_e5m2", dict(k_cache=_z(2, 64, 1, 128, dtype=torch.float8_e5m2))),
    ("cache_u8", dict(k_cache=_z(2, 64, 1, 128, dtype=U8))),
    ("q_f32", dict(q_index=_z(1, 32, 2, 128, dtype=F32), k_cache=_z(2, 64, 1, 128, dtype=F32))), ("cache_bf16", dict(k_cache=_z(2, 64, 1, 128, dtype=BF16))),
    ("feature_size_64", dict(q_index=_z(1, 32, 2, 64), k_cache=_z(2, 64, 1, 64))), ("cache_576", dict(k_cache=_z(2, 64, 1, 576))),
    ("cache_two_heads", dict(k_cache=_z(2, 64, 2, 128))),
    ("Hi_48", dict(q_index=_z(1, 48, 2, 128), weights=_z(1, 48, 2, dtype=F32))),
    ("topk_100", dict(topk=100)), ("topk_0", dict(topk=0)), ("topk_bool", dict(topk=True)), ("topk_float", dict(topk=64.0)), ("topk_none", dict(topk=None)),
    ("weights_none", dict(weights=None)), ("weights_f16", dict(weights=_z(1, 32, 2))), ("weights_transposed_shape", dict(weights=_z(1, 2, 32, dtype=F32))),
    ("weights_negative_stride_free_view", dict(weights=_z(1, 2, 32, dtype=F32).transpose(1, 2))),   # (valid: the model's layout)
    ("q_feature_stride_2", dict(q_index=_z(1, 32, 2, 256)[..., ::2])), ("q_rows_off_16_bytes", dict(q_index=_padded("q_index"))),
    ("q_elsewhere", _meta("q_index")), ("weights_left_behind", _meta("q_index", "k_cache", "cache_seqlens", "block_table")),
    ("lens_left_behind", _meta("q_index", "weights", "k_cache", "block_table")), ("table_left_behind", _meta("q_index", "weights", "k_cache", "cache_seqlens")),
    ("k_new_left_behind", {**_meta("q_index", "weights", "k_cache", "cache_seqlens", "block_table"), "k_new": _z(1, 2, 1, 128)}),
    ("q_grad", dict(q_index=_grad("q_index"))), ("weights_grad", dict(weights=_grad("weights"))), ("cache_grad", dict(k_cache=_grad("k_cache"))),
    ("k_new_grad", dict(k_new=_z(1, 2, 1, 128).requires_grad_())),
    ("lens_int64", dict(cache_seqlens=_z(1, dtype=torch.int64))), ("lens_two", dict(cache_seqlens=_z(2, dtype=I32))),
    ("lens_strided", dict(cache_seqlens=_z(2, dtype=I32)[::2])),
    ("table_int64", dict(block_table=_z(1, 1, dtype=torch.int64))), ("table_1d", dict(block_table=_z(1, dtype=I32))),
    ("table_two_rows", dict(block_table=_z(2, 1, dtype=I32))), ("table_no_column", dict(block_table=_z(1, 0, dtype=I32))),
    ("table_strided", dict(block_table=_z(1, 2, dtype=I32)[:, ::2])),
    ("page_32", dict(k_cache=_z(2, 32, 1, 128))), ("dense_two_for_one", dict(block_table=None)), ("dense_valid", dict(block_table=None, k_cache=_z(1, 64, 1, 128))),
    ("cache_rows_off_16_bytes", dict(k_cache=_padded("k_cache"))), ("cache_feature_stride_2", dict(k_cache=_z(2, 64, 1, 256)[..., ::2])),
    ("cache_rows_overlap", dict(k_cache=_z(2, 1, 1, 128).expand(2, 64, 1, 128))),
    ("k_new_bf16", dict(k_new=_z(1, 2, 1, 128, dtype=BF16))), ("k_new_576", dict(k_new=_z(1, 2, 1, 576))), ("k_new_3d", dict(k_new=_z(1, 2, 128))),
]


def py_cases():
    """(name, function, operands replaced) in the order of the fixture's lines"""
    out = [(f"{fn}/{name}", fn, over) for name, fns, over in MLA_PY_CASES for fn in fns]
    return out + [(f"{INDEX_FN}/{name}", INDEX_FN, over) for name, over in INDEX_PY_CASES]


def _refusal(pkg, fn, over):
    d = (_index_operands if fn == INDEX_FN else _mla_operands)(fn)
    new = {k: v(d) if callable(v) else v for k, v in over.items()}
    d.update({k: v for k, v in new.items() if v is not SKIP})
    try:
        getattr(pkg, fn)(**d)
    except Exception as e:   # noqa: BLE001  (whatever is raised is what is recorded)
        return f"{type(e).__name__} | " + str(e).replace("\\", "\\\\").replace("\n", "\\n")
    return "returned"   # (never on CPU tensors: the last check refuses them)


@functools.lru_cache(maxsize=None)
def refusals(pkg):
    return [f"{name} | {_refusal(pkg, fn, over)}" for name, fn, over in py_cases()]


def test_python_refusals_equal_the_recorded_messages(pkg):
    want = open(PY_FIXTURE).read().splitlines()
    got = refusals(pkg)
    assert len(got) == len(want) == len(py_cases()) and len(set(line.split(" | ")[0] for line in got)) == len(got)
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, f"{len(diff)} of {len(got)} refusals moved; the first (got, recorded): {diff[:3]}"


def test_every_valid_call_ends_at_the_cpu_refusal(pkg):
    """the calls named valid_* pass every argument check: what refuses them is the last one, and no call of the table returns"""
    for line in refusals(pkg):
        name, rest = line.split(" | ", 1)
        assert rest != "returned", name
        if "valid" in name.split("/")[1]:
            assert rest.startswith("RuntimeError | ") and "no CPU fallback" in rest, line


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    import flash_attention_softmax_n_amd
    for path, text in ((FIXTURE, matrix(flash_attention_softmax_n_amd)), (PY_FIXTURE, refusals(flash_attention_softmax_n_amd))):
        with open(path, "w") as fh:
            fh.write("\n".join(text) + "\n")
        print(f"recorded {len(text)} cases in {path}")
