"""flash_attention_n_mla on the GPU: decode over a compressed latent K/V cache (576-feature rows, the first 512 the value) against plain
fp32 torch - the visible rows gathered through the table, x = scale q row^T, the mask, the explicit sink column of weight n,
out = p row[:, :512] - under the K/V-cache suites' own gates (tests/kv_support.py)."""
import pytest
import torch

from kv_support import _bits, _capture, _check, _check_lse, _gather, _Paged, _rand, _visibility
from mla_support import E, EV, LENS, SCALE, _cache, _n, _nsplit, _ref

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1), (16, 2), (33, 2), (128, 2)]   # a partial wave, one 32-row half, a 64-row block + 2 rows, the 256-row limit


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
