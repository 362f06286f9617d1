"""MLA decode without a GPU: the four entry points refuse what the header says they refuse, with its codes and in its order, before any
HIP call; the Python call names what is served."""
import ctypes

import pytest
import torch

from mla_support import EALIGN, EDTYPE, EHEADDIM, EINVAL, ESTRIDE, EUNSUPPORTED, _args


def _codes(pkg, a):
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    view = pkg._lib.View4()
    view.ptr, view.stride[0], view.stride[1], view.stride[2], view.stride[3] = 1 << 20, 2 * 576, 576, 576, 1
    p = None if a is None else ctypes.byref(a)
    return (lib.fasn_fwd_mla(p, 1 << 20, 1 << 40, None), lib.fasn_mla_append(p, ctypes.byref(view), None), lib.fasn_mla_plan(p, buf, len(buf)),
            lib.fasn_mla_workspace_bytes(p))


REFUSALS = [
    ("NULL block", None, EINVAL),
    ("head dim 512 + 128", dict(D=640), EHEADDIM),
    ("value dim 576", dict(Dv=576), EHEADDIM),
    ("fp32", dict(dtype=2), EDTYPE),
    ("H * Sq = 258", dict(H=129), EUNSUPPORTED),
    ("page 48", dict(page_size=48), EUNSUPPORTED),
    ("fp16 scale 6", dict(dtype=0, scale=6.0), EUNSUPPORTED),
    ("misaligned q row", {"q.stride2": 577}, EALIGN),
    ("misaligned cache row", dict(kv_cache=(1 << 20) + 8), EALIGN),
    ("feature stride 2", {"q.stride3": 2}, ESTRIDE),
    # the order: sizes and enums, what is not served, the views (their stride rule first), the remaining alignment
    ("fp32 before the head dims", dict(dtype=2, D=640), EDTYPE),
    ("head dims before the row limit", dict(D=640, H=129), EHEADDIM),
    ("page 48 before a misaligned row", {"page_size": 48, "q.stride2": 577}, EUNSUPPORTED),
    ("feature stride before alignment", {"q.stride3": 2, "o.stride2": 513}, ESTRIDE),
    ("a view before the cache's alignment", {"o.stride3": 2, "kv_cache": (1 << 20) + 8}, ESTRIDE),
]


@pytest.mark.parametrize("what,over,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_points_refuse_with_the_headers_codes(pkg, what, over, code):
    fwd, append, plan, ws = _codes(pkg, None if over is None else _args(pkg, **over))
    assert (fwd, append, plan, ws) == (code, code, code, 0), what


def test_a_served_block_has_a_plan_and_a_workspace(pkg):
    a = _args(pkg)
    names = [k[0].split("<")[0] for k in pkg._lib.mla_plan(a)]
    assert names == ["fasn_mla_fwd_kernel", "fasn_mla_combine_kernel"]
    nsplit = pkg._lib.mla_plan(a)[0][1] // 2          # B * ceil(32 / 64) blocks; 4 tiles of capacity, 4 per split
    assert nsplit == 1 and pkg._lib.load().fasn_mla_workspace_bytes(a) == 2 * nsplit * 32 * 514 * 4
    assert pkg._lib.load().fasn_fwd_mla(a, None, 0, None) == -8   # the workspace comes behind every check


def test_python_call_names_what_is_served(pkg):
    fn = pkg.flash_attention_n_mla
    assert "flash_attention_n_mla" in pkg.__all__
    q = torch.zeros(1, 4, 1, 576, dtype=torch.float16)
    lens = torch.zeros(1, dtype=torch.int32)
    table = torch.zeros(1, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="512 \\+ 64 = 576"):
        fn(torch.zeros(1, 4, 1, 128, dtype=torch.float16), torch.zeros(2, 64, 1, 128, dtype=torch.float16), lens, 0.1, block_table=table)
    with pytest.raises(TypeError, match="FP8.*512 \\+ 64 = 576"):
        fn(q, torch.zeros(2, 64, 1, 576, dtype=torch.float8_e4m3fn), lens, 0.1, block_table=table)
    with pytest.raises(TypeError, match="scale"):
        fn(q, torch.zeros(2, 64, 1, 576, dtype=torch.float16), lens, block_table=table)
    with pytest.raises(ValueError, match="log2\\(e\\) <= 8"):
        fn(q, torch.zeros(2, 64, 1, 576, dtype=torch.float16), lens, 6.0, block_table=table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(q, torch.zeros(2, 64, 1, 576, dtype=torch.float16), lens, 0.1, block_table=table)
