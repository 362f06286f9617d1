"""Sparse MLA decode without a GPU: the three entry points give mla_build's refusals first, then the index list's, with the header's codes
and order, before any HIP call; a served block's plan and workspace; the Python call names what is served."""
import ctypes

import pytest
import torch

from mla_support import BASE, EALIGN, EINVAL, EUNSUPPORTED, _args, _sparse


def _codes(pkg, a, s):
    lib, buf = pkg._lib.load(), ctypes.create_string_buffer(4096)
    s = None if s is None else ctypes.byref(s)
    return lib.fasn_fwd_mla_sparse(a, s, BASE, 0, None), lib.fasn_mla_sparse_plan(a, s, buf, len(buf)), lib.fasn_mla_sparse_workspace_bytes(a, s)


REFUSALS = [   # (what, block, operand, code): mla_build's first, beside an operand the second group refuses
    ("page 48 before topk 96", dict(page_size=48), dict(topk=96), EUNSUPPORTED),
    ("misaligned cache before a NULL list", dict(kv_cache=BASE + 8), dict(indices=None), EALIGN),
    ("NULL operand", dict(), None, EINVAL),
    ("NULL list", dict(), dict(indices=None), EINVAL),
    ("reserved = 1", dict(), dict(reserved=1), EINVAL),
    ("topk 0", dict(), dict(topk=0), EINVAL),
    ("negative stride", dict(), dict(stride_q=-1), EINVAL),
    ("stride beyond 32 bits", dict(), dict(stride_b=1 << 31), EINVAL),
    ("topk 96", dict(), dict(topk=96), EUNSUPPORTED),
    ("topk 2048 + 32", dict(), dict(topk=2080), EUNSUPPORTED),
    ("list off 4 bytes", dict(), dict(indices=BASE + 2), EALIGN),
    ("reserved before topk 96", dict(), dict(topk=96, reserved=1), EINVAL),
    ("topk 96 before the list's alignment", dict(), dict(topk=96, indices=BASE + 2), EUNSUPPORTED),
]


@pytest.mark.parametrize("what,over,sover,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_points_refuse_with_the_headers_codes(pkg, what, over, sover, code):
    assert _codes(pkg, _args(pkg, **over), None if sover is None else _sparse(pkg, **sover)) == (code, code, 0), what


@pytest.mark.parametrize("B,H,Sq,topk", [(2, 16, 2, 2048), (1, 128, 2, 2048), (3, 65, 1, 64)])
def test_a_served_block_has_a_plan_and_a_workspace(pkg, B, H, Sq, topk):
    a, s = _args(pkg, B=B, H=H, Sq=Sq), _sparse(pkg, topk=topk, stride_b=Sq * topk, stride_q=topk)
    plan = pkg._lib.mla_sparse_plan(a, s)
    assert [k[0].split("<")[0] for k in plan] == ["fasn_mla_sparse_fwd_kernel", "fasn_mla_combine_kernel"]
    base = B * Sq * ((H + 63) // 64)
    nsplit = plan[0][1] // base   # the split rule: ~512 workgroups, at least 8 index tiles per split of a full head block, 4 below that
    assert nsplit == max(1, min(-(-512 // base), (topk // 64) // (8 if H >= 64 else 4))) and plan[0][1] == base * nsplit
    assert plan[0][3] == 144 * 1024 and plan[1][1:] == pkg._lib.mla_plan(a)[1][1:]
    assert pkg._lib.load().fasn_mla_sparse_workspace_bytes(a, s) == B * nsplit * H * Sq * 514 * 4
    assert _codes(pkg, a, s)[0] == -8   # the workspace comes behind every check


def test_python_call_names_what_is_served(pkg):
    fn = pkg.flash_attention_n_mla_sparse
    assert "flash_attention_n_mla_sparse" in pkg.__all__
    q, cache = torch.zeros(1, 4, 2, 576, dtype=torch.float16), torch.zeros(2, 64, 1, 576, dtype=torch.float16)
    lens, table, idx = torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, 2, 64, dtype=torch.int32)
    for bad in (idx.long(), idx[:, :1], idx[0], None):
        with pytest.raises(ValueError, match="int32 tensor \\[B, Sq, topk\\].*served: .*top-k list"):
            fn(q, cache, bad, lens, 0.1, block_table=table)
    with pytest.raises(ValueError, match="topk = 96.*topk % 64 == 0.*served: "):
        fn(q, cache, torch.zeros(1, 2, 96, dtype=torch.int32), lens, 0.1, block_table=table)
    with pytest.raises(RuntimeError, match="indices is on cpu, query on meta.*served: "):
        fn(q.to("meta"), cache.to("meta"), idx, lens.to("meta"), 0.1, block_table=table.to("meta"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(q, cache, idx, lens, 0.1, block_table=table)
