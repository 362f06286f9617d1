"""The order of the checks of the K/V-cache host layer, without a GPU: every rule of the argument builders broken on its own, and every
pair of rules that are neighbours in the check order broken together, over a handful of valid argument blocks - for the decode and the
prefill entry points alike. tests/golden/kvhost_matrix.txt holds, per case, the return values of the three *_plan entry points, the two
*_workspace_bytes entry points and *_rope_append_plan (an accepted plan as a short hash of its text), so a change of WHICH code wins
when two rules are broken at once shows as a changed line.

Nothing is ever launched: the pointers are fake. Valid blocks go through the *_plan and *_workspace_bytes entry points only; the
forwards and the appends are called only with blocks the plan call has just refused, so they return before any HIP call.

    python tests/test_kvhost_matrix_cpu.py --record     rewrites the fixture from the library of this tree
"""
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "kvhost_matrix.txt")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kv_args import BASES, BASE_RULES, BIG, DUMMY, Case, _attr, _kn_only, _no_new_rows, _on, _plan, _set   # noqa: E402

# the valid blocks and the base rules are kv_args's: the packed matrix of tests/test_kvvarlen_cpu.py is built on them too
PAIR_BASES = ("dec_paged", "pre_paged_qlens")   # the paged blocks: every rule applies to them


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
