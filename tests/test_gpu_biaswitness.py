"""attn_bias as an additive mask on the GPU (tests/bias_witness.py): flash_attention_n and its backward where the bias hides keys with
-1e4, -65504, -1e9, finfo.min or -inf - a hidden prefix of one tile and of two tiles and a part, the causal-LM mask of a left-padded batch,
a split-K launch whose every split meets hidden tiles first, and a bias that forces one key per row - over every kernel family that reads a
bias: the seeded vector modes at D = 32, 64, 128 with a 16-bit and an fp32 bias, key padding, a dense mask, causal, dropout, split-K, the
decode regroup, and as controls the kernels that do not seed from a running maximum (D = 256, element loads, fp32).

Every expectation comes from the fp64 CPU reference of attn_witness.py and is compared per element in EVERY (batch, head): witness C's
gates with rounding point (9), the seed, added; the rows the sink alone takes, the rows with nothing and the weak-gated rows as the
docstring of bias_witness.py says. Each test prints its largest ratios before it asserts <= 1. tests/test_biaswitness_cpu.py shows that
these gates break by 10x and more on the arithmetic of the kernels before the seed floor, and that the arithmetic with it stays at or
below 0.5 of them."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_witness as aw   # noqa: E402
import bias_witness as bw   # noqa: E402
from flash_attention_softmax_n_amd import flash_attn   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,dtype,bdtype,label", list(bw.params()))
def test_bias_as_additive_mask(pkg, dev, name, dtype, bdtype, label):
    case = bw.SHAPES[name]
    text = bw.plan_text(pkg, case, dtype, bdtype)
    for prop in case.want:   # the launch pinned without a GPU (split-K: SPLIT=1 and a combine kernel)
        assert prop in text, (name, prop, text)
    inp = bw.inputs(case, dtype, bdtype, label, dev, aw.seed_of(name))
    path = flash_attn.kernel_path(inp["q"], inp["k"], inp["v"], attn_mask=inp["mask"], attn_bias=inp["bias"], is_causal=case.causal,
                                  dropout_p=case.p, scale=inp["scale"], softmax_n_param=inp["n"])
    assert path == pkg._lib.FASN_PATH_NAMES[pkg._lib.load().fasn_fwd_path(bw.plan_args(pkg, case, dtype, bdtype, backward=False).fwd)], (name, path)
    res = aw.run(pkg, case, inp, aw.seed_of(name))
    keep, p_eff = aw.keep_of(case, res["state"])
    r, g = bw.reference(case, inp, dtype, keep=keep, p_eff=p_eff)
    try:
        rat = bw.judge(case, dtype, res, r, g, inp)
    except aw.GateRefused as e:
        print(f"bias {name} {dtype} bias {bw.bias_dtype_name(dtype, bdtype)} -V {label}: refused outright: {e}")
        raise
    print(f"bias {name} {dtype} bias {bw.bias_dtype_name(dtype, bdtype)} -V {label}: ratios to the gates: {rat}")
    assert rat.worst() <= 1, f"bias witness {name} {dtype} bias {bdtype} -V {label}: {rat}"
