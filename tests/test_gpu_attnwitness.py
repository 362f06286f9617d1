"""The three witnesses of tests/attn_witness.py on the GPU, through flash_attention_n and its backward, over every kernel family of
DESIGN 4.2 (attn_witness.SHAPES; tests/test_attnwitness_cpu.py pins each case's launch plan without a GPU).

Every expectation comes from the fp64 CPU reference of attn_witness.py and is compared per row and per element, in EVERY (batch, head):
  A  |exp(lse) - Z_ref| <= 1e-5 Z_ref and |out Z_ref (1 - p_eff) - c_ref| <= 0.25; dK exactly 0; |dV Z (1 - p_eff) - rows| <= 0.25 where Z
     is a power of two; dQ, dV, dn, dbias under witness C's per-element gates. The condition cmax u <= 0.2 is asserted from the reference;
     it decides which shapes run in fp16 only.
  B  |out - f V[t]| <= 2 u |V[t]| + 1e-30 where key t decides the row, |out| <= 1e-12 where the sink does, exactly 0 where nothing is
     visible; the bounded code also dV[t] = dO within 2 u |dO| and dQ, dK, dn = 0 up to the derived fp32 summation error.
  C  every result within its first-order bound (attn_witness docstring), at logit standard deviations of 4 and 8; the fp32 cases at
     u = unit(case, fp32).
attn_witness.NEW adds the instantiations of each family that the first cases leave out (8-wave forwards, key padding and dropout at every
head dim, grouped K/V at D = 32 / 128, split-K under key padding, the fp32 kernels' other head dims and modes).
Each test prints its largest ratios before it asserts <= 1. tests/test_attnwitness_cpu.py shows what each gate catches and that an
emulation of the kernels' arithmetic stays at or below 0.5 of witness C's gates."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_witness as aw   # noqa: E402
from flash_attention_softmax_n_amd import flash_attn   # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = aw.SHAPES

def _reference(case, inp, res, backward):
    keep, p_eff = aw.keep_of(case, res["state"])
    only = None if (backward or case.ub * case.uh <= 64) else ("l", "acc", "m", "out", "lse")   # (512 dropout problems: what witness A reads)
    return aw.reference(case, inp, keep=keep, p_eff=p_eff, backward=backward, only=only), p_eff


# ---------------------------------------------------------------- A: every visible key and every kept weight exactly once
@pytest.mark.parametrize("name,dtype", [(s, d) for s, c in SHAPES.items() if "A" in c.wit for d in c.a_dtypes])
def test_a_every_visible_key_exactly_once(pkg, dev, name, dtype):
    case, dt = SHAPES[name], aw.DTYPES[dtype]
    inp = aw.inputs_a(case, dt, dev, aw.seed_of(name))
    res = aw.run(pkg, case, inp, aw.seed_of(name))
    r, p_eff = _reference(case, inp, res, case.bwd)
    cmax = aw.condition_a(case, r, dt, p_eff)
    g = aw.with_bounds(case, inp, r, aw.unit(case, dt), aw.unit_abs(dt)) if case.bwd else None
    rat = aw.judge_a(case, dt, res, r, g, p_eff)
    print(f"A {name} {dtype}: largest class count {cmax:g}; ratios to the gates: {rat}")
    assert rat.worst() <= 1, f"witness A {name} {dtype}: {rat}"
    if case.bwd and aw.pow2_n(case) is not None and dtype in ("fp16", "fp32"):
        assert "dV Z" in rat, "the integer gate on dV Z must run where Z is a power of two (fp16: every such case)"
    # the launch plan pinned without a GPU is that of this very call
    path = flash_attn.kernel_path(inp["q"], inp["k"], inp["v"], attn_mask=inp["mask"], attn_bias=inp["bias"], is_causal=case.causal, dropout_p=case.p,
                           scale=inp["scale"], softmax_n_param=inp["n"])
    assert path == pkg._lib.FASN_PATH_NAMES[pkg._lib.load().fasn_fwd_path(aw.plan_args(pkg, case, dtype, backward=False).fwd)], (name, path)


# ---------------------------------------------------------------- B: one key decides
def _b_cases():
    for s, c in SHAPES.items():
        if "B" not in c.wit:
            continue
        for d in c.dtypes:
            yield s, "ascending", d
            if c.bwd and d != "fp32":   # (fp32: the bounded code's backward is not run - its gate wants the fp32 resolution of x - lse derived first)
                yield s, "code", d
        yield s, "sink", c.dtypes[-1]
        if c.bwd and c.dtypes[-1] != "fp32":
            yield s, "code_sink", c.dtypes[-1]
        if "split" in s:
            yield s, "descending", c.dtypes[-1]


@pytest.mark.parametrize("name,form,dtype", list(_b_cases()))
def test_b_one_key_decides(pkg, dev, name, form, dtype):
    case, dt = SHAPES[name], aw.DTYPES[dtype]
    backward = case.bwd and form.startswith("code")
    inp = aw.inputs_b(case, form, dt, dev, aw.seed_of(name))
    res = aw.run(pkg, case, inp, aw.seed_of(name), backward=backward)
    r, p_eff = _reference(case, inp, res, backward)
    g = aw.with_bounds(case, inp, r, aw.unit(case, dt), aw.unit_abs(dt))
    rat, kinds = aw.judge_b(case, form, dt, res, r, g, inp)
    print(f"B {name} {form} {dtype}: row kinds {sorted(kinds)}; ratios to the gates: {rat}")
    assert rat.worst() <= 1, f"witness B {name} {form} {dtype}: {rat}"
    assert 1 in kinds or form == "code_sink" or (case.nshape == "float" and form == "sink")   # (a float n: every head has the sink)
    assert 2 in kinds or "sink" not in form


# ---------------------------------------------------------------- C: a realistic dynamic range
@pytest.mark.parametrize("name,dtype,std", [(s, d, std) for s, c in SHAPES.items() if "C" in c.wit for d in c.dtypes for std in (4, 8)])
def test_c_realistic_dynamic_range(pkg, dev, name, dtype, std):
    case, dt = SHAPES[name], aw.DTYPES[dtype]
    inp = aw.inputs_c(case, std, dt, dev, aw.seed_of(name) + std)
    res = aw.run(pkg, case, inp, aw.seed_of(name))
    r, p_eff = _reference(case, inp, res, case.bwd)
    g = aw.with_bounds(case, inp, r, aw.unit(case, dt), aw.unit_abs(dt))
    rat = aw.judge_c(case, dt, res, r, g)
    print(f"C {name} std {std} {dtype}: ratios to the gates: {rat}")
    assert rat.worst() <= 1, f"witness C {name} std {std} {dtype}: {rat}"
