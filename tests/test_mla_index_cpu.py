"""The lightning indexer without a GPU: the four entry points refuse what the header says they refuse, with its codes and in its order,
before any HIP call; a served block's plan and workspace; the Python call names what is served."""
import ctypes

import pytest
import torch

from mla_support import BASE, EALIGN, EDTYPE, EHEADDIM, EINVAL, ESTRIDE, EUNSUPPORTED
from mla_support import _index_args as _args


def _codes(pkg, a):
    lib, buf, view = pkg._lib.load(), ctypes.create_string_buffer(4096), pkg._lib.View4()
    view.ptr, view.stride[0], view.stride[1], view.stride[2], view.stride[3] = BASE, 2 * 128, 128, 128, 1
    p = None if a is None else ctypes.byref(a)
    return (lib.fasn_mla_index(p, BASE, 1 << 40, None), lib.fasn_mla_index_append(p, ctypes.byref(view), None),
            lib.fasn_mla_index_plan(p, buf, len(buf)), lib.fasn_mla_index_workspace_bytes(p))


REFUSALS = [
    ("NULL block", None, EINVAL),
    ("topk 0", dict(topk=0), EINVAL),
    ("reserved = 1", dict(reserved=1), EINVAL),
    ("fp32", dict(dtype=2), EDTYPE),
    ("feature size 64", dict(D=64), EHEADDIM),
    ("NULL weights", dict(w=None), EINVAL),
    ("NULL list", dict(indices=None), EINVAL),
    ("negative weight stride", {"w_stride#1": -2}, EINVAL),
    ("key rows overlap", {"k_stride#1": 64}, EINVAL),
    ("Hi = 48", dict(Hi=48), EUNSUPPORTED),
    ("topk 100", dict(topk=100), EUNSUPPORTED),
    ("page 32", dict(page_size=32), EUNSUPPORTED),
    ("feature stride 2", {"q.stride#3": 2}, ESTRIDE),
    ("misaligned q row", {"q.stride#2": 129}, EALIGN),
    ("misaligned cache", dict(k_cache=BASE + 8), EALIGN),
    ("logits off 4 bytes", dict(logits=BASE + 2), EALIGN),
    # the order: sizes and enums, dtype, feature size, NULL members, what is not served, the view, the remaining alignment
    ("fp32 before the feature size", dict(dtype=2, D=64), EDTYPE),
    ("feature size before Hi", dict(D=64, Hi=48), EHEADDIM),
    ("a NULL member before topk 100", dict(w=None, topk=100), EINVAL),
    ("Hi = 48 before a misaligned row", {"Hi": 48, "q.stride#2": 129}, EUNSUPPORTED),
    ("the view before the cache's alignment", {"q.stride#3": 2, "k_cache": BASE + 8}, ESTRIDE),
]


@pytest.mark.parametrize("what,over,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_points_refuse_with_the_headers_codes(pkg, what, over, code):
    assert _codes(pkg, None if over is None else _args(pkg, **over)) == (code, code, code, 0), what


@pytest.mark.parametrize("B,Sq,pages,page,tpw", [(3, 2, 96, 64, 2), (64, 1, 128, 256, 16), (1, 2, 128, 256, 2), (3, 1, 1, 64, 2)])
def test_a_served_block_has_a_plan_and_a_workspace(pkg, B, Sq, pages, page, tpw):
    """tpw, the 64-key tiles of a workgroup: the even number >= 2 that brings the grid to ~2048 workgroups"""
    a = _args(pkg, B=B, Sq=Sq, max_pages=pages, block_table_stride=pages, page_size=page)
    tiles = pages * page // 64
    assert tpw == max(2, -(-min(tiles, -(-B * Sq * tiles // 2048)) // 2) * 2)
    assert pkg._lib.mla_index_plan(a) == [("fasn_mla_index_logits_kernel<fasn::bf16_tag, 64>", B * Sq * -(-tiles // tpw), 256, 0),
                                          ("fasn_mla_index_select_kernel<1024>", B * Sq, 1024, 0)]
    lib = pkg._lib.load()
    assert lib.fasn_mla_index_workspace_bytes(a) == B * Sq * tiles * 64 * 4
    assert lib.fasn_mla_index(a, None, 0, None) == -8   # the workspace comes behind every check
    a.logits = BASE
    assert lib.fasn_mla_index_workspace_bytes(a) == 0   # the caller's logits buffer: nothing else is needed


def test_python_call_names_what_is_served(pkg):
    fn = pkg.flash_attention_n_mla_index
    assert "flash_attention_n_mla_index" in pkg.__all__
    f16 = torch.float16
    q, w, cache = torch.zeros(1, 32, 2, 128, dtype=f16), torch.zeros(1, 32, 2), torch.zeros(2, 64, 1, 128, dtype=f16)
    lens, table = torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="dtype torch.float32.*served: "):
        fn(q.float(), w, cache.float(), lens, 64, block_table=table)
    with pytest.raises(TypeError, match="FP8 index keys.*served: "):
        fn(q, w, cache.to(torch.float8_e4m3fn), lens, 64, block_table=table)
    with pytest.raises(ValueError, match="Hi = 48.*served: "):
        fn(torch.zeros(1, 48, 2, 128, dtype=f16), torch.zeros(1, 48, 2), cache, lens, 64, block_table=table)
    with pytest.raises(ValueError, match="feature size 128.*served: "):
        fn(torch.zeros(1, 32, 2, 64, dtype=f16), w, torch.zeros(2, 64, 1, 64, dtype=f16), lens, 64, block_table=table)
    with pytest.raises(ValueError, match="topk = 100.*topk % 64 == 0.*served: "):
        fn(q, w, cache, lens, 100, block_table=table)
    with pytest.raises(ValueError, match="page_size 32"):
        fn(q, w, torch.zeros(2, 32, 1, 128, dtype=f16), lens, 64, block_table=table)
    with pytest.raises(RuntimeError, match="forward only"):
        fn(q, w.clone().requires_grad_(), cache, lens, 64, block_table=table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(q, w, cache, lens, 64, block_table=table)
