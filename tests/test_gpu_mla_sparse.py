"""flash_attention_n_mla_sparse on the GPU against plain fp32 torch: per (b, i) the entries' visibility bits, the rows gathered by the
clamped entries from the table-gathered cache, x = scale q row^T with hidden entries at -inf, the explicit sink column of weight n,
out = p row[:, :512] - under the K/V-cache suites' own gates (tests/kv_support.py)."""
import pytest
import torch

import kv_layout as kl
from kv_support import _bits, _capture, _check, _check_lse, _gather, _Paged, _rand
from mla_support import E, LENS, SCALE, _cache, _entry_vis, _lists, _n
from mla_support import _nsplit as _dense_nsplit
from mla_support import _nsplit_sparse as _nsplit
from mla_support import _ref_sparse as _ref

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
SHAPES = [(5, 1), (16, 2), (64, 1), (128, 2)]   # a partial wave, one 32-row half, one full head block, two head blocks x two positions


def _check_case(pkg, q, pool, table, idx, lens, rows, n, causal, dtype, what):
    seqlens = torch.tensor(lens, dtype=torch.int32, device=q.device)
    out, lse = pkg.flash_attention_n_mla_sparse(q, pool, idx, seqlens, SCALE, block_table=table, softmax_n_param=n, is_causal=causal, return_lse=True)
    o_ref, lse_ref, vis = _ref(q, rows, idx, lens, n, causal)
    _check(out, o_ref, dtype, f"{what} out")
    _check_lse(lse, lse_ref, f"{what} lse")
    blind = ~vis.any(-1)[:, None].expand_as(lse)   # rows without a key: exactly 0, and log n exactly (0 for n = 1, -inf for n = 0)
    assert (out[blind] == 0).all(), f"{what}: rows without a key are not exactly 0"
    if not isinstance(n, torch.Tensor):
        assert (lse[blind] == (0.0 if n == 1 else float("-inf"))).all(), f"{what}: lse of rows without a key"
    return out, lse


@pytest.mark.parametrize("causal", [True, False], ids=["c", "nc"])
@pytest.mark.parametrize("topk", [64, 2048])
@pytest.mark.parametrize("H,Sq", SHAPES, ids=[f"{h}x{s}" for h, s in SHAPES])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_parity(pkg, dtype, H, Sq, topk, causal):
    """n = 0, 1 and a per-head tensor in one item: they share the lists, the queries and the conditions asserted on the lists"""
    pc, rows = _cache(dtype, 64)
    B = len(LENS)
    idx = _lists(B, Sq, topk, 64 * pc.max_pages, 41, longest=(B - 1, LENS[-1]))
    if topk == 2048:   # the longest element has a fully visible tile, a mixed one and a dead one between live ones; real partials are merged
        per_tile = _entry_vis(idx, LENS, Sq, causal)[B - 1, 0].view(-1, 64).sum(-1)
        live = (per_tile > 0).nonzero().flatten()
        assert (per_tile == 64).any() and ((per_tile > 0) & (per_tile < 64)).any() and (per_tile[live[0]:live[-1]] == 0).any()
        assert _nsplit(pkg, B, H, Sq, topk, pc.max_pages) >= 2
    q = _rand((B, H, Sq, E), dtype, rows.device, 5)
    for n in (0, 1, "tensor"):
        _check_case(pkg, q, pc.k, pc.table, idx.to(rows.device), LENS, rows, _n(n, B, H, rows.device), causal, dtype, f"sparse {dtype} H={H} Sq={Sq} topk={topk} n={n}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_identity_list_is_the_dense_call(pkg, dtype):
    dev, seqlens = torch.device("cuda"), torch.tensor([0, 1, 65, 192], dtype=torch.int32, device="cuda")
    dense, q = _rand((4, 192, 1, E), dtype, dev, 7), _rand((4, 33, 2, E), dtype, dev, 8)
    idx = torch.arange(192, dtype=torch.int32, device=dev).expand(4, 2, 192).contiguous()
    assert _nsplit(pkg, 4, 33, 2, 192, 1, page=192) == 1 and _dense_nsplit(pkg, 4, 33, 2, 192, 1, paged=False) == 1
    n = _n("tensor", 4, 33, dev)
    want = pkg.flash_attention_n_mla(q, dense, seqlens, SCALE, softmax_n_param=n, return_lse=True)
    got = pkg.flash_attention_n_mla_sparse(q, dense, idx, seqlens, SCALE, softmax_n_param=n, return_lse=True)
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[1], want[1])


def test_unnamed_not_read(pkg):
    """every pool row no visible entry names is NaN - in range or not - and every table slot none touches points at the NaN poison page"""
    dtype, Sq = torch.float16, 2
    pc, rows = _cache(dtype, 64)
    dev, B = rows.device, len(LENS)
    idx = _lists(B, Sq, 64, 64 * pc.max_pages, 43).to(dev)
    vis = _entry_vis(idx, LENS, Sq, True)
    named = torch.zeros(B, 64 * pc.max_pages, dtype=torch.bool, device=dev)
    for b in range(B):
        named[b, idx[b][vis[b]].long()] = True
    table = torch.where(named.view(B, pc.max_pages, 64).any(-1), pc.table, torch.full_like(pc.table, pc.poison))
    pool = torch.full_like(pc.k, float("nan"))
    b_of, j_of = named.nonzero(as_tuple=True)
    at = (pc.table[b_of, j_of // 64].long(), j_of % 64)
    pool[at] = pc.k[at]
    assert torch.isnan(pool[pc.table[B - 1, 0].long()]).any() and (table == pc.poison).sum() > (pc.table == pc.poison).sum()   # in-range rows and slots
    q = _rand((B, 33, Sq, E), dtype, dev, 10)
    got = _check_case(pkg, q, pool, table, idx, LENS, rows, 1, True, dtype, "sparse poisoned")
    clean = _check_case(pkg, q, torch.nan_to_num(pc.k), pc.table, idx, LENS, rows, 1, True, dtype, "sparse clean")
    assert torch.equal(_bits(got[0]), _bits(clean[0])) and torch.equal(got[1], clean[1])


def test_kv_new(pkg):
    dev, dtype, Sq, lens = torch.device("cuda"), torch.bfloat16, 2, (0, 5, 63, 191, 127)   # capacity 192: the last row of element 3 is dropped
    B = len(lens)
    rows0 = _rand((B, 1, 192, E), dtype, dev, 21)
    before = _Paged(rows0, rows0, list(lens), 64, 3, 21, alloc_all=True)
    kv_new, table = _rand((B, Sq, 1, E), dtype, dev, 22), before.table
    pool, want = before.k.clone(), before.k.clone()
    for b, ln in enumerate(lens):
        for i in range(min(Sq, 192 - ln)):
            want[int(table[b, (ln + i) // 64]), (ln + i) % 64] = kv_new[b, i]
    q = _rand((B, 16, Sq, E), dtype, dev, 23)
    seqlens = torch.tensor(lens, dtype=torch.int32, device=dev)
    idx = torch.arange(192, dtype=torch.int32, device=dev).flip(0).expand(B, Sq, 192).contiguous()   # every position, the new ones among them
    got = pkg.flash_attention_n_mla_sparse(q, pool, idx, seqlens, SCALE, block_table=table, kv_new=kv_new, return_lse=True)
    assert torch.equal(_bits(pool), _bits(want))                   # the dense append's pool: the rows are in the pages, one is dropped
    ref = pkg.flash_attention_n_mla_sparse(q, want, idx, seqlens + Sq, SCALE, block_table=table, return_lse=True)
    assert torch.equal(_bits(got[0]), _bits(ref[0])) and torch.equal(got[1], ref[1])
    after = [min(ln + Sq, 192) for ln in lens]
    _check(got[0], _ref(q, _gather(want, table, after, 64)[:, 0], idx, after, 1, True)[0], dtype, "sparse kv_new out")


def test_one_graph(pkg):
    dtype, B, Sq, topk = torch.bfloat16, 3, 2, 2048
    pc, _ = _cache(dtype, 64, (1100,) * 3, True, 31)
    dev, lists = pc.k.device, lambda seed: _lists(B, Sq, topk, 64 * pc.max_pages, seed, longest=(0, 1100))   # noqa: E731
    q = _rand((B, 33, Sq, E), dtype, dev, 32)
    seqlens, idx = torch.tensor([64, 65, 1100], dtype=torch.int32, device=dev), lists(44).to(dev)
    call = lambda: pkg.flash_attention_n_mla_sparse(q, pc.k, idx, seqlens, SCALE, block_table=pc.table, return_lse=True)   # noqa: E731
    graph, res = _capture(call)
    dead = torch.full((B, Sq, topk), -1, dtype=torch.int32)
    one = dead.clone()
    one[:, :, topk - 7] = 3   # a single live entry, in the last tile of the last split
    for new_idx, lens in ((lists(45), [65, 64, 300]), (dead, [1100, 257, 1024]), (one, [1100, 4, 2]), (lists(46), [1100, 1, 319])):
        idx.copy_(new_idx)
        seqlens.copy_(torch.tensor(lens, dtype=torch.int32))
        graph.replay()
        eager = call()
        assert torch.equal(_bits(res[0]), _bits(eager[0])) and torch.equal(res[1], eager[1]), lens


def test_far_rows(pkg):
    """three pages of one 4.5 GiB allocation: row byte offsets below 2^31, in [2^31, 2^32) and beyond 2^32"""
    dev, dtype = torch.device("cuda"), torch.bfloat16
    _, kf, _, info = kl.far_pool(torch.empty((1, 64, 1, E), dtype=dtype), dev)
    rows = _rand((1, 192, E), dtype, dev, 51)
    for s, pid in enumerate(info["ids"]):
        kf[pid, :, 0] = rows[0, s * 64:(s + 1) * 64]
    table = torch.tensor([list(info["ids"])], dtype=torch.int32, device=dev)
    idx = _lists(1, 2, 64, 192, 52).to(dev)
    assert info["k_off"][2] >= 1 << 32 and (idx[0, 1] >= 128).sum() > 4   # entries that live in the far page
    _check_case(pkg, _rand((1, 16, 2, E), dtype, dev, 53), kf, table, idx, [190], rows, 1, True, dtype, "sparse far rows")
