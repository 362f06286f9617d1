"""flash_attention_n_mla_sparse_fp8 on the GPU: the 656-byte rows against flash_attention_n_mla_sparse on their unpacked 16-bit rows (bit
for bit) and against plain fp32 torch on those rows (mla_support._ref_sparse under the family's gates, tests/kv_support.py)."""
import pytest
import torch

import kv_layout as kl
from kv_support import _bits, _capture, _check, _check_lse, _gather, _Paged, _rand
from mla_support import E, EV, LENS, SCALE, _args, _block, _entry_vis, _lists, _n, _sparse
from mla_support import _ref_sparse as _ref

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
QSTD = 2.0 ** -10   # random bytes are rows of rms ~ 250: queries this small keep the logits at the O(0.5) the family's gates are made for


def _rows8(lead, dtype, seed, pow2=True):
    """uint8 [*lead, 656] of seeded random bytes: finite codes, four different scales per row in [2^-6, 2^3], the rope part from _rand"""
    gen = torch.Generator().manual_seed(seed)
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)[torch.randint(0, 254, (*lead, EV), generator=gen)]
    e = torch.rand((*lead, 10 if pow2 else 9), generator=gen).argsort(-1)[..., :4] - 6   # four different exponents: four binades
    s = torch.exp2(e.float()) * (1 if pow2 else 1 + torch.rand((*lead, 4), generator=gen))
    rope = _rand((*lead, E - EV), dtype, "cpu", seed + 1000)
    return torch.cat([codes, s.contiguous().view(torch.uint8), rope.contiguous().view(torch.uint8)], -1).cuda()


def _paged8(rows8, lens, seed, alloc_all=False):
    """_Paged over byte rows [B, S, 656] through a bf16 view (its NaN fill is a NaN scale and a NaN rope part in either dtype)"""
    v = rows8.view(torch.bfloat16)[:, None]
    pc = _Paged(v, v, list(lens), 64, rows8.shape[1] // 64, seed, alloc_all=alloc_all)
    return pc, pc.k.view(torch.uint8)


def _both(pkg, q, pool8, table, idx, lens, n, causal):
    """the call, asserted bit for bit flash_attention_n_mla_sparse on the unpacked pool"""
    seqlens = torch.as_tensor(lens, dtype=torch.int32).to(q.device)
    args = dict(block_table=table, softmax_n_param=n, is_causal=causal, return_lse=True)
    got = pkg.flash_attention_n_mla_sparse_fp8(q, pool8, idx, seqlens, SCALE, **args)
    want = pkg.flash_attention_n_mla_sparse(q, pkg.mla_fp8_rows_unpack(pool8, q.dtype), idx, seqlens, SCALE, **args)
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    return got


@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "general"])
@pytest.mark.parametrize("topk", [64, 2048])
@pytest.mark.parametrize("H,Sq", [(5, 1), (128, 2)], ids=["5x1", "128x2"])
@DTYPES
def test_parity(pkg, dtype, H, Sq, topk, pow2):
    B, S = len(LENS), 64 * 19
    rows8 = _rows8((B, S), dtype, 3, pow2)
    assert len(rows8[..., :EV].unique()) == 254 and (rows8[..., EV:EV + 16].contiguous().view(torch.float32).sort(-1).values.diff() > 0).all()
    pc, pool8 = _paged8(rows8, LENS, 3)
    rows = _gather(pkg.mla_fp8_rows_unpack(pool8, dtype), pc.table, LENS, 64)[:, 0]
    shape, s = dict(B=B, H=H, Sq=Sq, max_pages=S // 64, block_table_stride=S // 64), _sparse(pkg, topk=topk, stride_b=Sq * topk, stride_q=topk)
    grid = pkg._lib.mla_sparse_fp8_plan(_block(pkg, **shape), s)[0][1]   # the 16-bit call's nsplit, >= 2 splits at topk 2048
    assert grid == pkg._lib.mla_sparse_plan(_args(pkg, **shape), s)[0][1] and (topk == 64 or grid >= 2 * B * Sq * ((H + 63) // 64))
    idx, q = _lists(B, Sq, topk, S, 41, longest=(B - 1, LENS[-1])).cuda(), _rand((B, H, Sq, E), dtype, "cuda", 5, std=QSTD)
    for causal in (True, False):
        vis = _entry_vis(idx, LENS, Sq, causal)
        live = vis[B - 1, 0].view(-1, 64).any(-1).nonzero().flatten()
        assert topk == 64 or live[-1] - live[0] >= len(live)   # a dead tile between live ones
        blind = ~vis.any(-1)[:, None].expand(B, H, Sq)
        for n in (0, 1, "tensor"):
            what, nv = f"sparse fp8 {dtype} H={H} Sq={Sq} topk={topk} causal={causal} n={n}", _n(n, B, H, torch.device("cuda"))
            out, lse = _both(pkg, q, pool8, pc.table, idx, LENS, nv, causal)
            o_ref, lse_ref, _ = _ref(q, rows, idx, LENS, nv, causal)
            _check(out, o_ref, dtype, f"{what} out")
            _check_lse(lse, lse_ref, f"{what} lse")
            assert (out[blind] == 0).all(), f"{what}: rows without a key are not exactly 0"
            assert n == "tensor" or (lse[blind] == (0.0 if n == 1 else float("-inf"))).all(), f"{what}: lse of rows without a key is not log n"


@DTYPES
def test_feature_seams(pkg, dtype):
    """element i: one row, zero except feature seams[i] = 1.0, scales (0.5, 1, 2, 3); head 0 asks for it, head 1 for its neighbour; n = 0"""
    seams, beside, value = (127, 128, 511, 512, 575), (128, 127, 512, 511, 574), torch.tensor([0.5, 1.0, 3.0, 1.0, 1.0])
    cache, q, want = torch.zeros(5, 64, 1, 656, dtype=torch.uint8), torch.zeros(5, 2, 1, E, dtype=dtype), torch.zeros(5, 2, 1, EV)
    cache[:, 0, 0, EV:EV + 16] = torch.tensor([0.5, 1.0, 2.0, 3.0]).view(torch.uint8)
    for i, f in enumerate(seams):
        if f < EV:
            cache[i, 0, 0, f], want[i, :, 0, f] = 0x38, value[i]   # (a rope feature never reaches a value)
        else:
            cache[i, 0, 0, 16 + 2 * f - EV:18 + 2 * f - EV] = torch.ones(1, dtype=dtype).view(torch.uint8)
        q[i, 0, 0, f], q[i, 1, 0, beside[i]] = 0.25, 0.25
    idx = torch.cat([torch.zeros(5, 1, 1), -torch.ones(5, 1, 63)], -1).int()   # the one key, then padding
    out, lse = pkg.flash_attention_n_mla_sparse_fp8(q.cuda(), cache.cuda(), idx.cuda(), torch.ones(5, dtype=torch.int32, device="cuda"), 0.125,
                                                    softmax_n_param=0, return_lse=True)
    assert torch.equal(out.float().cpu(), want)
    _check_lse(lse, torch.stack([0.125 * 0.25 * value, torch.zeros(5)], -1)[..., None], f"seams {dtype} lse")


def test_unnamed_not_read(pkg):
    """every row no visible entry names is NaN codes, NaN scales and NaN rope, every table slot none touches points at the poison page"""
    dtype, Sq, B, S = torch.float16, 2, len(LENS), 64 * 19
    pc, pool8 = _paged8(_rows8((B, S), dtype, 3), LENS, 3)
    idx = _lists(B, Sq, 64, S, 43).cuda()
    vis, named = _entry_vis(idx, LENS, Sq, True), torch.zeros(B, S, dtype=torch.bool, device="cuda")
    for b in range(B):
        named[b, idx[b][vis[b]].long()] = True
    table = torch.where(named.view(B, pc.max_pages, 64).any(-1), pc.table, torch.full_like(pc.table, pc.poison))
    b_of, j_of = named.nonzero(as_tuple=True)
    at = (pc.table[b_of, j_of // 64].long(), j_of % 64)
    poisoned, clean = torch.full_like(pool8, 0xFF), torch.zeros_like(pool8)
    poisoned[at], clean[at] = pool8[at], pool8[at]
    assert (poisoned[pc.table[B - 1, 0].long()] == 0xFF).all(-1).any() and (table == pc.poison).sum() > (pc.table == pc.poison).sum()
    q = _rand((B, 33, Sq, E), dtype, "cuda", 10)
    got = pkg.flash_attention_n_mla_sparse_fp8(q, poisoned, idx, pc.lens, SCALE, block_table=table, return_lse=True)
    want = _both(pkg, q, clean, pc.table, idx, LENS, 1, True)
    assert torch.isfinite(want[0]).all() and torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[1], want[1])


@DTYPES
def test_kv_new(pkg, dtype):
    B, Sq, lens = 5, 2, (0, 5, 63, 191, 127)   # capacity 192: a page edge, and the last row of element 3 is dropped
    pc, pool = _paged8(_rows8((B, 192), dtype, 21), (192,) * B, 21, alloc_all=True)
    kv_new, top = _rand((B, Sq, 1, E), dtype, "cuda", 22), torch.tensor(448.0 * 2.0 ** -3, dtype=dtype)
    kv_new[0, 0, 0, 128:256] = 0                                                 # an all-zero group
    kv_new[1, 0, 0, 7] = top                                                     # amax exactly 448 * 2^k
    kv_new[1, 1, 0, 300] = (top.view(torch.int16) + 1).view(dtype)               # ... and the next number above it
    kv_new[2, 1, 0, 3], kv_new[2, 1, 0, 4] = float("nan"), float("-inf")        # row 64 of element 2: named by nobody below
    want = pool.clone()
    for b, ln in enumerate(lens):
        for i in range(min(Sq, 192 - ln)):
            want[int(pc.table[b, (ln + i) // 64]), (ln + i) % 64] = pkg.mla_fp8_rows_pack(kv_new[b, i])
    q, seqlens = _rand((B, 16, Sq, E), dtype, "cuda", 23), torch.tensor(lens, dtype=torch.int32, device="cuda")
    idx = torch.arange(192, dtype=torch.int32, device="cuda").flip(0).expand(B, Sq, 192).contiguous()
    idx[2][idx[2] == 64] = -1
    got = pkg.flash_attention_n_mla_sparse_fp8(q, pool, idx, seqlens, SCALE, block_table=pc.table, kv_new=kv_new, return_lse=True)
    assert torch.equal(pool, want)                     # byte for byte the torch pack, one row dropped
    ref = pkg.flash_attention_n_mla_sparse_fp8(q, want, idx, seqlens + Sq, SCALE, block_table=pc.table, return_lse=True)
    assert torch.isfinite(got[0]).all() and torch.equal(_bits(got[0]), _bits(ref[0])) and torch.equal(got[1], ref[1])


def test_one_graph(pkg):
    dtype, B, Sq, topk, S = torch.bfloat16, 3, 2, 2048, 64 * 19
    pc, base = _paged8(_rows8((B, S), dtype, 60, False), (S,) * B, 31, alloc_all=True)
    pool, lists = base.clone(), lambda seed: _lists(B, Sq, topk, S, seed, longest=(0, 1100))   # noqa: E731
    q, seqlens, idx = _rand((B, 33, Sq, E), dtype, "cuda", 32), torch.tensor([64, 65, 1100], dtype=torch.int32, device="cuda"), lists(44).cuda()
    call = lambda: pkg.flash_attention_n_mla_sparse_fp8(q, pool, idx, seqlens, SCALE, block_table=pc.table, return_lse=True)   # noqa: E731
    graph, res = _capture(call)
    dead, one = torch.full((B, Sq, topk), -1, dtype=torch.int32), torch.full((B, Sq, topk), -1, dtype=torch.int32)
    one[:, :, topk - 7] = 3   # a single live entry, in the last tile of the last split
    for k, (new_idx, lens) in enumerate(((lists(45), [65, 64, 300]), (dead, [1100, 257, 1024]), (one, [1100, 4, 2]), (lists(46), [1100, 1, 319]))):
        idx.copy_(new_idx)
        seqlens.copy_(torch.tensor(lens, dtype=torch.int32))
        pool.copy_(base.roll(k + 1, 1))   # other cache bytes: every page's rows rotated
        graph.replay()
        eager = call()
        assert torch.equal(_bits(res[0]), _bits(eager[0])) and torch.equal(res[1], eager[1]), lens


def test_far_rows(pkg):
    """three pages of one 4.5 GiB allocation: row byte offsets below 2^31, in [2^31, 2^32) and beyond 2^32"""
    dtype, (_, kf, _, info) = torch.bfloat16, kl.far_pool(torch.empty((1, 64, 1, 328), dtype=torch.bfloat16), "cuda")   # (a byte template: 328 bf16 = 656 bytes)
    rows8 = _rows8((1, 192), dtype, 51)
    for s, pid in enumerate(info["ids"]):
        kf.view(torch.uint8)[pid, :, 0] = rows8[0, s * 64:(s + 1) * 64]
    table, idx = torch.tensor([list(info["ids"])], dtype=torch.int32, device="cuda"), _lists(1, 2, 64, 192, 52).cuda()
    assert info["k_off"][2] >= 1 << 32 and (idx[0, 1] >= 128).sum() > 4   # entries that live in the far page
    q, seqlens = _rand((1, 16, 2, E), dtype, "cuda", 53, std=QSTD), torch.tensor([190], dtype=torch.int32, device="cuda")
    out, lse = pkg.flash_attention_n_mla_sparse_fp8(q, kf.view(torch.uint8), idx, seqlens, SCALE, block_table=table, return_lse=True)
    o_ref, lse_ref, _ = _ref(q, pkg.mla_fp8_rows_unpack(rows8, dtype), idx, [190], 1, True)
    _check(out, o_ref, dtype, "sparse fp8 far rows out")
    _check_lse(lse, lse_ref, "sparse fp8 far rows lse")
