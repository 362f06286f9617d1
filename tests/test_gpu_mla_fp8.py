"""flash_attention_n_mla_fp8 on the GPU: MLA decode over a latent cache of e4m3fn codes. With kv_scale = 1 the call must equal
flash_attention_n_mla on the exactly upcast cache bit for bit - that pins the widening, the swizzle and the masks to the kernel that has
its own reference tests (tests/test_gpu_mla.py); with general scales it is held against that file's fp32 reference on
codes * kv_scale[b] under the K/V-cache suites' gates (tests/kv_support.py). Page 64, the lengths of tests/test_gpu_mla.py."""
import functools

import pytest
import torch

from kv_fp8 import F8, NAN_CODE, PagedCodes, finite_codes, is_nan_code, quantise, rand_codes, up, visible
from kv_support import _bits, _capture, _check, _check_lse, _n_values, _rand
from mla_support import E, EV, LENS, SCALE, _nsplit, _ref

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def _cache(lens=tuple(LENS), seed=3, top=0x7E):
    """a paged cache of random finite codes (top = 0x7e: every magnitude), stale rows and unnamed pages NaN codes (PagedCodes).
    Returns (the cache, its rows [B, S, 576] as uint8 with the rows at or beyond len_b at code 0)."""
    max_pages = max(1, max((ln + 63) // 64 for ln in lens)) + 1
    codes = rand_codes((len(lens), 1, 64 * max_pages, E), seed, torch.device("cuda"), top)
    return PagedCodes(codes, codes, list(lens), 64, max_pages, seed), visible(codes, lens)[:, 0]


def _twin(pkg, q, pool, table, seqlens, dtype, **kw):
    """the FP8 call at kv_scale = 1 against the 16-bit call on the upcast pool: bit for bit"""
    got = pkg.flash_attention_n_mla_fp8(q, pool, seqlens, SCALE, 1.0, block_table=table, return_lse=True, **kw)
    want = pkg.flash_attention_n_mla(q, pool.to(dtype), seqlens, SCALE, block_table=table, return_lse=True, **kw)
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[1], want[1])
    return got


@pytest.mark.parametrize("n", [0, "tensor"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Sq", [(5, 1), (33, 2), (128, 2)])   # a partial wave, one block plus two rows, the 256-row limit
@pytest.mark.parametrize("dtype", DTYPES)
def test_twin_ragged_batch(pkg, dtype, H, Sq, causal, n):
    pc, _ = _cache()
    q = _rand((len(LENS), H, Sq, E), dtype, pc.k.device, 5)
    assert _nsplit(pkg, len(LENS), H, Sq, 64, pc.max_pages) >= 2   # (tests/test_mla_fp8_cpu.py: the FP8 plan is the 16-bit plan)
    n = _n_values((len(LENS), H), q.device, 11) if n == "tensor" else n
    _twin(pkg, q, pc.k, pc.table, pc.lens, dtype, softmax_n_param=n, is_causal=causal)


def test_twin_dense_cache_one_split(pkg):
    dev, dtype, lens = torch.device("cuda"), torch.float16, [0, 1, 65, 192]
    dense = rand_codes((4, 192, 1, E), 7, dev, 0x7E)
    for b, ln in enumerate(lens):
        dense[b, ln:] = NAN_CODE
    assert _nsplit(pkg, 4, 33, 2, 192, 1, paged=False) == 1
    _twin(pkg, _rand((4, 33, 2, E), dtype, dev, 8), dense.view(F8), None, torch.tensor(lens, dtype=torch.int32, device=dev), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_code_at_every_chunk_position(pkg, dtype):
    """code index 7 (row * 576 + feature) mod 254: 7 is odd, so the 8 positions of every chunk - 63, 64 (the seam between the latent and the
    rotated part) and 71 (the last) among them - meet codes of both parities, and 130 rows bring all 254 to the cache"""
    dev, S = torch.device("cuda"), 192
    codes = finite_codes()[0][(7 * torch.arange(S * E)) % 254].view(1, 1, S, E).to(dev)
    pc = PagedCodes(codes, codes, [130], 64, 3, 41)
    assert torch.unique(visible(codes, [130])[0, 0, :130, 63 * 8:]).numel() == 254
    _twin(pkg, _rand((1, 33, 2, E), dtype, dev, 42), pc.k, pc.table, pc.lens, dtype, softmax_n_param=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_general_scales_against_the_reference(pkg, dtype):
    pc, rows = _cache(top=0x48)
    B, H, Sq = len(LENS), 33, 2
    ks = 2.0 ** torch.linspace(-6, 2, B, device=rows.device)   # 1/64 .. 4, one per batch element
    q = _rand((B, H, Sq, E), dtype, rows.device, 12)
    n = _n_values((B, H), rows.device, 13)
    assert _nsplit(pkg, B, H, Sq, 64, pc.max_pages) >= 2
    out, lse = pkg.flash_attention_n_mla_fp8(q, pc.k, pc.lens, SCALE, ks, block_table=pc.table, softmax_n_param=n, return_lse=True)
    o_ref, lse_ref = _ref(q, up(rows) * ks[:, None, None], LENS, n, True)
    _check(out, o_ref, dtype, f"mla fp8 {dtype} out")
    _check_lse(lse, lse_ref, f"mla fp8 {dtype} lse")


def test_the_two_feature_seams(pkg):
    """the rope features reach the logits; they never reach the values"""
    dtype, ks = torch.bfloat16, 0.5
    pc, rows = _cache(top=0x48)
    q = _rand((len(LENS), 16, 2, E), dtype, rows.device, 9)
    q_rope, q_lat = q.clone(), q.clone()
    q_rope[..., :EV], q_lat[..., EV:] = 0, 0
    loud = pc.ku.clone()
    loud[..., EV:] = 0x7E   # 448
    for what, qq, pool in (("rope-only query", q_rope, pc.k), ("loud rope codes", q_lat, loud.view(F8))):
        out, lse = pkg.flash_attention_n_mla_fp8(qq, pool, pc.lens, SCALE, ks, block_table=pc.table, return_lse=True)
        o_ref, lse_ref = _ref(qq, up(rows) * ks, LENS, 1, True)
        _check(out, o_ref, dtype, f"mla fp8 {what} out")
        _check_lse(lse, lse_ref, f"mla fp8 {what} lse")


def test_stale_memory_never_surfaces(pkg):
    pc, _ = _cache()
    assert is_nan_code(pc.ku[pc.poison]).all() and is_nan_code(pc.ku[int(pc.table[2, 0]), 63:]).all()   # unnamed pages, rows at or beyond len_b
    clean = torch.where(is_nan_code(pc.ku), torch.zeros_like(pc.ku), pc.ku).view(F8)
    q = _rand((len(LENS), 33, 2, E), torch.float16, pc.k.device, 10)
    got, want = (pkg.flash_attention_n_mla_fp8(q, pool, pc.lens, SCALE, 0.25, block_table=pc.table, return_lse=True) for pool in (pc.k, clean))
    assert torch.isfinite(got[0]).all() and torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_kv_new_is_quantised_appended_then_seen(pkg, dtype):
    dev, Sq, lens = torch.device("cuda"), 2, (0, 5, 63, 191, 127)   # capacity 192: the last row of element 3 is dropped
    B = len(lens)
    pc = PagedCodes(*[rand_codes((B, 1, 192, E), 21, dev)] * 2, [192] * B, 64, 3, 21)   # every page named: rows behind the lengths are codes
    ks = torch.tensor([1.0, 1 / 64, 4.0, 0.3, 1 / 7], device=dev)   # 1 / 64: |x / s| beyond 448 is clamped
    kv_new = _rand((B, Sq, 1, E), dtype, dev, 22, std=2.0)
    pool, want = pc.ku.clone(), pc.ku.clone()
    for b, ln in enumerate(lens):
        for i in range(Sq):
            if ln + i < 192:
                want[int(pc.table[b, (ln + i) // 64]), (ln + i) % 64] = quantise(kv_new[b, i], float(ks[b])).to(dev)
    q = _rand((B, 16, Sq, E), dtype, dev, 23)
    seqlens = torch.tensor(lens, dtype=torch.int32, device=dev)
    got = pkg.flash_attention_n_mla_fp8(q, pool.view(F8), seqlens, SCALE, ks, block_table=pc.table, kv_new=kv_new, return_lse=True)
    assert torch.equal(pool, want) and not torch.equal(pool, pc.ku)   # the codes are in the pages, one row is dropped, nothing else changed
    ref = pkg.flash_attention_n_mla_fp8(q, want.view(F8), seqlens + Sq, SCALE, ks, block_table=pc.table, return_lse=True)
    assert torch.equal(_bits(got[0]), _bits(ref[0])) and torch.equal(got[1], ref[1])


def test_one_graph_many_lengths_and_scales(pkg):
    dtype = torch.bfloat16
    pc, _ = _cache((1100,) * 3, 31, 0x48)
    q = _rand((3, 33, 2, E), dtype, pc.k.device, 32)
    seqlens = torch.tensor([64, 65, 1100], dtype=torch.int32, device=q.device)
    ks = torch.tensor([1.0, 0.5, 0.25], device=q.device)
    call = lambda: pkg.flash_attention_n_mla_fp8(q, pc.k, seqlens, SCALE, ks, block_table=pc.table, return_lse=True)
    graph, res = _capture(call)
    for lens, s in (([64, 65, 1100], [1.0, 0.5, 0.25]), ([65, 64, 300], [0.125, 3.0, 1.0]), ([0, 257, 1024], [2.0, 2.0, 0.7]), ([1100, 1, 319], [0.3, 1.0, 1.5])):
        seqlens.copy_(torch.tensor(lens, dtype=torch.int32))
        ks.copy_(torch.tensor(s))
        graph.replay()
        eager = call()
        assert torch.equal(_bits(res[0]), _bits(eager[0])) and torch.equal(res[1], eager[1]), lens
