"""MLA decode over an FP8 latent cache without a GPU: the four entry points give the base call's refusals first and unchanged, then their
own operand's, before any HIP call; a served block has the 16-bit call's plan under the FP8 kernels' names; the Python call names the
right function for a cache it does not take."""
import ctypes

import pytest
import torch

from mla_support import BASE, EALIGN, EDTYPE, EHEADDIM, EINVAL, EUNSUPPORTED, _args, _fp8


def _codes(pkg, a, f):
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    view = pkg._lib.View4()
    view.ptr, view.stride[0], view.stride[1], view.stride[2], view.stride[3] = BASE, 2 * 576, 576, 576, 1
    f = None if f is None else ctypes.byref(f)
    return (lib.fasn_fwd_mla_fp8(a, f, BASE, 0, None), lib.fasn_mla_fp8_append(a, f, ctypes.byref(view), None),
            lib.fasn_mla_fp8_plan(a, f, buf, len(buf)), lib.fasn_mla_fp8_workspace_bytes(a, f))


REFUSALS = [
    # the base call's, unchanged and first (the operand beside them is one the second group refuses)
    ("fp32", dict(dtype=2), dict(reserved=1), EDTYPE),
    ("head dim 640", dict(D=640), dict(kv_scale=None), EHEADDIM),
    ("page 48", dict(page_size=48), dict(kv_scale=BASE + 2), EUNSUPPORTED),
    ("row stride 584: 16 bytes, not 8 elements", {"kv_stride": (64 * 592, 584)}, dict(), EALIGN),
    ("page stride off 16 bytes", {"kv_stride": (64 * 576 + 8, 576)}, dict(reserved=1), EALIGN),
    # the operand's
    ("NULL operand", dict(), None, EINVAL),
    ("NULL scale", dict(), dict(kv_scale=None), EINVAL),
    ("reserved = 1", dict(), dict(reserved=1), EINVAL),
    ("negative stride", dict(), dict(sb=-1), EINVAL),
    ("stride beyond 32 bits", dict(), dict(sb=1 << 31), EINVAL),
    ("scale off 4 bytes", dict(), dict(kv_scale=BASE + 2), EALIGN),
    ("reserved before the scale's alignment", dict(), dict(kv_scale=BASE + 2, reserved=1), EINVAL),
]


@pytest.mark.parametrize("what,over,fover,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_points_refuse_with_the_headers_codes(pkg, what, over, fover, code):
    a = _args(pkg, **{k: v for k, v in over.items() if k != "kv_stride"})
    if "kv_stride" in over:
        a.kv_stride[0], a.kv_stride[1] = over["kv_stride"]
    assert _codes(pkg, a, None if fover is None else _fp8(pkg, **fover)) == (code, code, code, 0), what


def test_a_served_block_has_the_16_bit_plan_under_the_fp8_names(pkg):
    a, f = _args(pkg, max_pages=40, block_table_stride=40), _fp8(pkg, sb=0)
    plan, base = pkg._lib.mla_fp8_plan(a, f), pkg._lib.mla_plan(a)
    assert [k[0].split("<")[0] for k in plan] == ["fasn_mla_fwd_fp8_kernel", "fasn_mla_fp8_combine_kernel"]
    assert [k[1:] for k in plan] == [k[1:] for k in base] and plan[0][3] == 144 * 1024   # grid, block, LDS
    lib = pkg._lib.load()
    assert lib.fasn_mla_fp8_workspace_bytes(a, f) == lib.fasn_mla_workspace_bytes(a) > 0
    assert _codes(pkg, a, f)[0] == -8   # the workspace comes behind every check


def test_python_call_names_the_right_function(pkg):
    fn = pkg.flash_attention_n_mla_fp8
    assert "flash_attention_n_mla_fp8" in pkg.__all__
    q, lens, table = torch.zeros(1, 4, 1, 576, dtype=torch.float16), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32)
    codes = torch.zeros(2, 64, 1, 576, dtype=torch.float8_e4m3fn)
    with pytest.raises(TypeError, match="float16 cache is flash_attention_n_mla's"):
        fn(q, torch.zeros(2, 64, 1, 576, dtype=torch.float16), lens, 0.1, 1.0, block_table=table)
    with pytest.raises(TypeError, match="float8_e4m3fn codes.*float8_e5m2 has no kernel"):
        fn(q, codes.view(torch.float8_e5m2), lens, 0.1, 1.0, block_table=table)
    with pytest.raises(TypeError, match="kv_scale"):
        fn(q, codes, lens, 0.1, block_table=table)
    with pytest.raises(TypeError, match="kv_scale must be a Python float or a floating-point tensor"):
        fn(q, codes, lens, 0.1, None, block_table=table)
    with pytest.raises(ValueError, match="16-byte aligned"):
        fn(q, torch.zeros(2, 64, 1, 584, dtype=torch.float8_e4m3fn)[..., :576], lens, 0.1, 1.0, block_table=table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(q, codes, lens, 0.1, 1.0, block_table=table)
