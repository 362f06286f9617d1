"""The three witnesses of tests/kv_witness.py on the GPU, through every K/V-cache call: flash_attention_n_kvcache, _prefill (with and
without query_seqlens and k_new / v_new), _window (decode and prefill kernels), _varlen, and the base calls with alibi_slopes (C only).

Every expectation comes from the fp64 CPU reference of kv_witness.py and is compared per row and per element:
  A  |exp(lse) - Z_ref| <= 1e-5 Z_ref and |out Z_ref - c_ref| <= 0.25: Z_ref - n is the number of visible keys, c_ref the number of them
     in class d. The condition that the output's own rounding stays under 0.2 is asserted from the reference; the shapes with thousands
     of keys run in fp16 for that reason.
  B  |out - V[w]| <= 2 u |V[w]| + 1e-30 where key w decides the row (the last visible key, the first one, or under the sink the first one
     of the heads with n = 0), |out| <= 1e-12 where the sink does, exactly 0 where nothing is visible; lse under _check_lse.
  C  |out - ref| <= 3 u A + 1e-6 with A = sum_j p_ij |v_jd|, at logit standard deviations of 4 and 8; lse under _check_lse.
u = 2^-8 in bf16, 2^-11 in fp16. Each test prints the largest ratio to its gate before it asserts. The shapes are the smallest at which
each seam exists: a tile and a page edge, a second row block (heads (12, 4): 42 positions), ragged and empty sequences, split plans with
full, partly empty and wholly hidden splits, windows below, at and above a tile, the packed call's per-sequence alignment.
tests/test_kvwitness_cpu.py shows what each gate catches."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_witness as kw   # noqa: E402
import kv_args   # noqa: E402
import kv_support as ks   # noqa: E402

pytestmark = pytest.mark.gpu

Case = kw.Case
LENS = [65, 199, 50, 0]
QLENS = [40, 1, 0, 20]
VQ = lambda PB: [1, 0, PB, PB + 1, 2 * PB + 3, 1]   # noqa: E731  a decode token, an empty sequence, a block, a block edge, blocks, a token
VL = lambda page: [300, 5, 0, page + 1, 2 * page, 64]   # noqa: E731
DSPLIT = dict(H=64, Hkv=8, D=64, Sq=1, lens=[5000], page=256, max_pages=20, long=True)
PSPLIT = dict(H=16, Hkv=2, D=64, Sq=64, page=256, max_pages=40, long=True)

SHAPES = {
    # decode: a key past a tile / page edge, three pages and a part, fewer than a tile, nothing
    "decode D64 Sq1": Case("decode", 16, 4, 64, 1, LENS),
    "decode D64 Sq3": Case("decode", 16, 4, 64, 3, LENS),
    "decode D128 Sq1": Case("decode", 16, 4, 128, 1, LENS),
    "decode D128 Sq3": Case("decode", 16, 4, 128, 3, LENS),
    "decode D32 Sq3": Case("decode", 16, 4, 32, 3, LENS),
    "decode D256 Sq3": Case("decode", 16, 4, 256, 3, LENS),
    "decode D64 Sq3 full": Case("decode", 16, 4, 64, 3, LENS, causal=False),
    "decode D64 Sq3 append": Case("decode", 16, 4, 64, 3, LENS, append=True),
    "decode split": Case("decode", **DSPLIT),
    # prefill: heads (12, 4) make a row block 42 positions, so 40 positions of 3 heads fill one and Sq = 200 five
    "prefill D64 Sq40": Case("prefill", 12, 4, 64, 40, LENS),
    "prefill D64 Sq40 qlens": Case("prefill", 12, 4, 64, 40, LENS, qlens=QLENS),
    "prefill D64 Sq40 qlens append": Case("prefill", 12, 4, 64, 40, LENS, qlens=QLENS, append=True),
    "prefill D128 Sq40 qlens append": Case("prefill", 12, 4, 128, 40, LENS, qlens=QLENS, append=True),
    "prefill D64 Sq40 qlens full": Case("prefill", 12, 4, 64, 40, LENS, qlens=QLENS, causal=False),
    "prefill D64 Sq200 qlens": Case("prefill", 12, 4, 64, 200, LENS, qlens=[200, 1, 0, 107]),
    "prefill D64 Sq200 append": Case("prefill", 12, 4, 64, 200, LENS, append=True),
    "prefill split 9000": Case("prefill", lens=[9000], **PSPLIT),
    "prefill split 20": Case("prefill", lens=[20], **PSPLIT),
    # window: inside a tile, one tile, more than three; both dispatch branches; the split plans with whole pages below the window
    **{f"window {br} W{W}": Case(f"window_{br}", 12, 4, 64, 3 if br == "decode" else 40, LENS, qlens=None if br == "decode" else QLENS,
                                 window=W, append=(W == 64)) for br in ("decode", "prefill") for W in (5, 64, 200)},
    "window decode split W3000": Case("window_decode", window=3000, **DSPLIT),
    "window prefill split W3000": Case("window_prefill", 64, 8, 64, 64, [5000], page=256, max_pages=20, qlens=[37], window=3000, long=True),
    # token-packed queries: PB = 16 and 42
    "varlen H8/1": Case("varlen", 8, 1, 64, 35, VL(64), qlens=VQ(16)),
    "varlen H12/4": Case("varlen", 12, 4, 64, 87, VL(64), qlens=VQ(42)),
    "varlen H12/4 full": Case("varlen", 12, 4, 64, 87, VL(64), qlens=VQ(42), causal=False),
    "varlen H12/4 D128 append": Case("varlen", 12, 4, 128, 87, VL(64), qlens=VQ(42), append=True),
    "varlen split": Case("varlen", ks.VARLEN_SPLIT["H"], ks.VARLEN_SPLIT["Hkv"], ks.VARLEN_SPLIT["D"], 40, [4000, 2100], page=ks.VARLEN_SPLIT["page"],
                         max_pages=ks.VARLEN_SPLIT["max_pages"], qlens=ks.VARLEN_SPLIT["qlens"], long=True),
}
ALIBI = {
    "alibi decode D64 Sq3": Case("decode", 16, 4, 64, 3, LENS, alibi=True),
    "alibi prefill D64 Sq40 qlens append": Case("prefill", 16, 4, 64, 40, LENS, qlens=QLENS, append=True, alibi=True),
    "alibi decode split": Case("decode", alibi=True, **DSPLIT),
    "alibi prefill split 9000": Case("prefill", lens=[9000], alibi=True, **PSPLIT),
}
DESCENDING = [s for s in SHAPES if s.startswith("window") or "split" in s]


def _assert_split(pkg, name, case):
    """the plans of the split shapes really split the keys (as test_split_k and test_plan_with_a_combine_kernel assert it)"""
    if "split" not in name:
        return
    shape = dict(B=case.B, H=case.H, Hkv=case.Hkv, Sq=case.Sq, D=case.D, page=case.page, max_pages=case.max_pages)
    operand = None if case.window is None else pkg._lib.KvWindow(window=case.window, reserved=0)
    if case.route == "decode":
        plan = pkg._lib.kvcache_plan(kv_args._args_decode(pkg, **shape))
        assert plan[0][0].startswith("fasn_kvcache_fwd_kernel<") and plan[0][1] > case.B * case.Hkv, plan
    elif case.route == "window_decode":
        plan = pkg._lib.kvcache_window_plan(kv_args._args_decode(pkg, **shape), operand)
        assert plan[0][0].startswith("fasn_kvcache_fwd_window_kernel<") and plan[0][1] > case.B * case.Hkv, plan
    elif case.route == "prefill":
        assert ks._plan_names(pkg, **shape) == ["fasn_kvprefill_fwd_kernel", "fasn_kvprefill_combine_kernel"]
    elif case.route == "window_prefill":
        plan = pkg._lib.kvprefill_window_plan(kv_args._args_prefill(pkg, **shape), operand)
        assert [k[0].split("<")[0] for k in plan] == ["fasn_kvprefill_fwd_window_kernel", "fasn_kvprefill_combine_kernel"]
        assert ks._first(case.total[0], case.qlens[0], case.window) >= 7 * case.page   # whole pages lie below the window: poisoned
    else:
        assert case.tail == 7
        ks._varlen_split_plan(pkg)


def _seed(name):
    return 1000 + sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 9000


# ---------------------------------------------------------------- A: every visible key exactly once
def _dtypes(case):
    return ["fp16"] if case.long else ["fp16", "bf16"]


@pytest.mark.parametrize("name,dtype", [(s, d) for s in SHAPES for d in _dtypes(SHAPES[s])])
def test_a_every_visible_key_exactly_once(pkg, dev, name, dtype):
    case, dt = SHAPES[name], kw.DTYPES[dtype]
    _assert_split(pkg, name, case)
    inp = kw.inputs_a(case, dt, dev, _seed(name))
    refs = kw.reference(case, inp)
    cmax = kw.condition_a(refs, dt)
    got = kw.run(pkg, case, inp, _seed(name))
    ratios = [kw.gate_a(o, lse, r) for (o, lse), r in zip(got, refs)]
    rz, ro = max(r[0] for r in ratios), max(r[1] for r in ratios)
    print(f"A {name} {dtype}: largest class count {cmax:g}; exp(lse) at {rz:.3g} of 1e-5 Z, out Z at {ro:.3g} of 0.25")
    assert rz <= 1, f"exp(lse) is {rz:.3g}x (1e-5 Z_ref) from n + the number of visible keys, per sequence {[r[0] for r in ratios]}"
    assert ro <= 1, f"out Z_ref is {ro:.3g}x 0.25 from the class counts, per sequence {[r[1] for r in ratios]}"


# ---------------------------------------------------------------- B: one key decides, far from the others
B_CASES = ([(s, "ascending", d) for s in SHAPES for d in ("fp16", "bf16")] + [(s, "descending", "bf16") for s in DESCENDING]
           + [(s, "sink", "bf16") for s in SHAPES] + [(s, "sink", "fp16") for s in SHAPES if "split" in s])


@pytest.mark.parametrize("name,form,dtype", B_CASES)
def test_b_one_key_decides(pkg, dev, name, form, dtype):
    case, dt = SHAPES[name], kw.DTYPES[dtype]
    inp = kw.inputs_b(case, form, dt, dev, _seed(name))
    refs = kw.reference(case, inp)
    got = kw.run(pkg, case, inp, _seed(name))
    ratios, kinds, lses = [], set(), []
    for b, ((o, lse), r) in enumerate(zip(got, refs)):
        kind, want = kw.expect_b(r, kw.sequence(case, inp, b)[2][:, :case.total[b]], case.H // case.Hkv)
        kinds |= set(kind.unique().tolist())
        ratios.append(kw.gate_b(o, kind, want, dt))
        lses.append((lse.detach().cpu(), r["lse"], kind))
    print(f"B {name} {form} {dtype}: out at {max(ratios):.3g} of its gate; row kinds {sorted(kinds)}")
    assert max(ratios) <= 1, f"out is {max(ratios):.3g}x the gate from the deciding key's V row, per sequence {ratios}"
    for b, (lse, want, kind) in enumerate(lses):
        for k in (0, 1, 2):   # rows of one kind together: log n is not measured against a key's thousands of nats
            if (kind == k).any():
                ks._check_lse(lse[kind == k], want[kind == k], f"B {name} {form} {dtype} sequence {b} lse (rows of kind {k})")
    assert 1 in kinds and (form != "sink" or 2 in kinds)


# ---------------------------------------------------------------- C: a realistic dynamic range
@pytest.mark.parametrize("std", [4, 8])
@pytest.mark.parametrize("name,dtype", [(s, d) for s in list(SHAPES) + list(ALIBI) for d in ("fp16", "bf16")])
def test_c_realistic_dynamic_range(pkg, dev, name, dtype, std):
    """A CPU emulation of the kernels' arithmetic stays below 0.45 of this gate (tests/test_kvwitness_cpu.py)."""
    case, dt = (SHAPES.get(name) or ALIBI[name]), kw.DTYPES[dtype]
    inp = kw.inputs_c(case, std, dt, dev, _seed(name) + std)
    refs = kw.reference(case, inp)
    got = kw.run(pkg, case, inp, _seed(name))
    ratios = [kw.gate_c(o, r, dt) for (o, _), r in zip(got, refs)]
    print(f"C {name} std {std} {dtype}: out at {max(ratios):.3g} of 3 u A + 1e-6")
    assert max(ratios) <= 1, f"out is {max(ratios):.3g}x (3 u A + 1e-6) from the fp64 reference, per sequence {ratios}"
    for b, ((_, lse), r) in enumerate(zip(got, refs)):
        ks._check_lse(lse, r["lse"], f"C {name} std {std} {dtype} sequence {b} lse")
