"""flash_attention_n_mla on the GPU: decode over a compressed latent K/V cache (576-feature rows, the first 512 the value) against plain
fp32 torch - the visible rows gathered through the table, x = scale q row^T, the mask, the explicit sink column of weight n,
out = p row[:, :512] - under the K/V-cache suites' own gates (tests/kv_support.py)."""
import functools

import pytest
import torch

from kv_support import _bh, _bits, _capture, _check, _check_lse, _gather, _n_values, _Paged, _rand, _visibility

pytestmark = pytest.mark.gpu

E, EV = 576, 512
SCALE = (128 + 64) ** -0.5
LENS = [0, 1, 63, 64, 65, 129, 1100]   # empty, shorter than Sq, a tile edge from both sides, a page edge, a length that is split
SHAPES = [(5, 1), (16, 2), (33, 2), (128, 2)]   # a partial wave, one 32-row half, a 64-row block + 2 rows, the 256-row limit


def _ref(q, rows, lens, n, causal, scale=SCALE):
    """rows: [B, S, 576] with the rows at or beyond len_b zeroed. Returns (out [B, H, Sq, 512], lse [B, H, Sq]) in fp32."""
    B, H, Sq, _ = q.shape
    x = scale * torch.einsum("bhqd,bsd->bhqs", q.float(), rows.float())
    x = x.masked_fill(~_visibility(lens, Sq, rows.shape[1], causal, q.device), float("-inf"))
    sink = _bh(torch.as_tensor(n, dtype=torch.float32, device=q.device), B, H).log()[..., None, None].expand(B, H, Sq, 1)   # (log 0 = -inf)
    xs = torch.cat([sink, x], -1)
    lse = torch.logsumexp(xs, -1)
    p = torch.exp(xs - torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))[..., None])[..., 1:]
    return torch.einsum("bhqs,bsd->bhqd", p, rows[..., :EV].float()), lse


@functools.lru_cache(maxsize=None)
def _cache(dtype, page, lens=tuple(LENS), alloc_all=False, seed=3):
    """one paged latent cache per (dtype, page): stale rows and unnamed pages are NaN (_Paged). Returns (pool, its gathered rows)."""
    dev = torch.device("cuda")
    max_pages = max(1, max((ln + page - 1) // page for ln in lens)) + 1
    rows = _rand((len(lens), 1, page * max_pages, E), dtype, dev, seed)
    pc = _Paged(rows, rows, list(lens), page, max_pages, seed, alloc_all=alloc_all)
    return pc, _gather(pc.k, pc.table, list(lens), page)[:, 0]


def _nsplit(pkg, B, H, Sq, page, max_pages, paged=True):
    a = pkg._lib.MlaArgs()
    a.q.ptr = a.o.ptr = a.kv_cache = a.seqlens = 1 << 20
    a.block_table = (1 << 20) if paged else None
    for v, d in ((a.q, E), (a.o, EV)):
        v.stride[0], v.stride[1], v.stride[2], v.stride[3] = H * Sq * d, Sq * d, d, 1
    a.kv_stride[0], a.kv_stride[1], a.block_table_stride, a.max_pages, a.page_size = page * E, E, max_pages, max_pages, page
    a.B, a.H, a.Sq, a.D, a.Dv, a.dtype, a.scale = B, H, Sq, E, EV, 1, SCALE
    fwd = pkg._lib.mla_plan(a)[0]
    return fwd[1] // (B * ((H * Sq + 63) // 64))


def _check_case(pkg, q, pool, table, lens, rows, n, causal, dtype, what):
    seqlens = torch.tensor(lens, dtype=torch.int32, device=q.device)
    out, lse = pkg.flash_attention_n_mla(q, pool, seqlens, SCALE, block_table=table, softmax_n_param=n, is_causal=causal, return_lse=True)
    o_ref, lse_ref = _ref(q, rows, lens, n, causal)
    _check(out, o_ref, dtype, f"{what} out")
    _check_lse(lse, lse_ref, f"{what} lse")
    blind = ~_visibility(lens, q.shape[2], rows.shape[1], causal, q.device).any(-1).expand_as(lse)   # rows without a visible key
    assert (out[blind] == 0).all(), f"{what}: rows without a visible key are not exactly 0"
    if not isinstance(n, torch.Tensor):   # log n exactly: 0 for n = 1, -inf for n = 0
        assert (lse[blind] == (0.0 if n == 1 else float("-inf"))).all(), f"{what}: lse of rows without a visible key"
    return out, lse


def _n(kind, B, H, dev):
    return _n_values((B, H), dev, 11) if kind == "tensor" else kind


@pytest.mark.parametrize("n", [0, 1, "tensor"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Sq", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_parity_ragged_batch_page_64(pkg, dtype, H, Sq, causal, n):
    pc, rows = _cache(dtype, 64)
    q = _rand((len(LENS), H, Sq, E), dtype, rows.device, 5)
    assert _nsplit(pkg, len(LENS), H, Sq, 64, pc.max_pages) >= 2   # the long element is split: the combine merges real partials
    _check_case(pkg, q, pc.k, pc.table, LENS, rows, _n(n, len(LENS), H, rows.device), causal, dtype, f"mla {dtype} H={H} Sq={Sq}")


def test_parity_page_256(pkg):
    pc, rows = _cache(torch.bfloat16, 256)
    q = _rand((len(LENS), 16, 2, E), torch.bfloat16, rows.device, 6)
    _check_case(pkg, q, pc.k, pc.table, LENS, rows, 1, True, torch.bfloat16, "mla page 256")
    _check_case(pkg, q, pc.k[:, :, 0], pc.table, LENS, rows, 1, True, torch.bfloat16, "mla page 256, 3-D cache")


def test_parity_dense_cache_one_split(pkg):
    dev, dtype, lens = torch.device("cuda"), torch.float16, [0, 1, 65, 192]
    dense = _rand((4, 192, 1, E), dtype, dev, 7)
    for b, ln in enumerate(lens):
        dense[b, ln:] = float("nan")
    q = _rand((4, 33, 2, E), dtype, dev, 8)
    assert _nsplit(pkg, 4, 33, 2, 192, 1, paged=False) == 1   # one partial per row: the combine's pass-through
    _check_case(pkg, q, dense, None, lens, torch.nan_to_num(dense[:, :, 0]), _n("tensor", 4, 33, dev), True, dtype, "mla dense")


def test_the_two_feature_seams(pkg):
    """the rope features reach the logits; they never reach the values"""
    dtype = torch.bfloat16
    pc, rows = _cache(dtype, 64)
    q = _rand((len(LENS), 16, 2, E), dtype, rows.device, 9)
    q_rope = q.clone()
    q_rope[..., :EV] = 0
    _check_case(pkg, q_rope, pc.k, pc.table, LENS, rows, 1, True, dtype, "mla rope-only query")
    q_lat = q.clone()
    q_lat[..., EV:] = 0
    loud = pc.k.clone()
    loud[..., EV:] = 1e4
    _check_case(pkg, q_lat, loud, pc.table, LENS, rows, 1, True, dtype, "mla loud rope features")


def test_stale_memory_never_surfaces(pkg):
    dtype = torch.float16
    pc, rows = _cache(dtype, 64)
    assert torch.isnan(pc.k[pc.poison]).all() and torch.isnan(pc.k[int(pc.table[2, 0]), 63:]).all()   # unnamed pages, rows at or beyond len_b
    q = _rand((len(LENS), 33, 2, E), dtype, rows.device, 10)
    got = _check_case(pkg, q, pc.k, pc.table, LENS, rows, 1, True, dtype, "mla stale")
    clean = _check_case(pkg, q, torch.nan_to_num(pc.k), pc.table, LENS, rows, 1, True, dtype, "mla clean")
    assert torch.equal(_bits(got[0]), _bits(clean[0])) and torch.equal(got[1], clean[1])


def test_kv_new_is_appended_then_seen(pkg):
    dev, dtype, Sq, lens = torch.device("cuda"), torch.bfloat16, 2, (0, 5, 63, 191, 127)   # capacity 192: the last row of element 3 is dropped
    B = len(lens)
    rows0 = _rand((B, 1, 192, E), dtype, dev, 21)
    before = _Paged(rows0, rows0, list(lens), 64, 3, 21, alloc_all=True)
    kv_new = _rand((B, Sq, 1, E), dtype, dev, 22)
    table = before.table
    pool, want = before.k.clone(), before.k.clone()
    for b, ln in enumerate(lens):
        for i in range(Sq):
            if ln + i < 192:
                want[int(table[b, (ln + i) // 64]), (ln + i) % 64] = kv_new[b, i]
    q = _rand((B, 16, Sq, E), dtype, dev, 23)
    seqlens = torch.tensor(lens, dtype=torch.int32, device=dev)
    got = pkg.flash_attention_n_mla(q, pool, seqlens, SCALE, block_table=table, kv_new=kv_new, return_lse=True)
    assert torch.equal(_bits(pool), _bits(want))                   # the rows are in the pages, one is dropped, nothing else changed
    ref = pkg.flash_attention_n_mla(q, want, seqlens + Sq, SCALE, block_table=table, return_lse=True)
    assert torch.equal(_bits(got[0]), _bits(ref[0])) and torch.equal(got[1], ref[1])
    rows = _gather(want, table, [min(ln + Sq, 192) for ln in lens], 64)[:, 0]
    _check(got[0], _ref(q, rows, [min(ln + Sq, 192) for ln in lens], 1, True)[0], dtype, "mla kv_new out")


def test_one_graph_many_lengths(pkg):
    dtype = torch.bfloat16
    pc, _ = _cache(dtype, 64, (1100,) * 3, True, 31)
    q = _rand((3, 33, 2, E), dtype, pc.k.device, 32)
    seqlens = torch.tensor([64, 65, 1100], dtype=torch.int32, device=q.device)
    call = lambda: pkg.flash_attention_n_mla(q, pc.k, seqlens, SCALE, block_table=pc.table, return_lse=True)
    graph, res = _capture(call)
    for lens in ([64, 65, 1100], [65, 64, 300], [0, 257, 1024], [1100, 1, 319]):   # tile edges; one and both of the two splits with tiles
        seqlens.copy_(torch.tensor(lens, dtype=torch.int32))
        graph.replay()
        eager = call()
        assert torch.equal(_bits(res[0]), _bits(eager[0])) and torch.equal(res[1], eager[1]), lens
