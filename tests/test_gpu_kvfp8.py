"""FP8 (e4m3fn) K/V cache on the GPU: flash_attention_n_kvcache_fp8 bit for bit against the 16-bit cache calls on the exactly upcast cache
under power-of-two scales (random codes and all 254 finite codes), against the fp32 reference of tests/kv_support.py on the dequantised
cache under general scales, with NaN codes in every stale row and page, the quantising append byte for byte against tests/kv_fp8.py's
reference formula, and under graph replay with the lengths and the scales changed in place."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_args as ka   # noqa: E402
import kv_fp8 as k8    # noqa: E402
import kv_support as ks   # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
DIMS = [64, 128]
_ids = lambda d: str(d).split(".")[-1]   # noqa: E731


def _dt(dtype):
    return 1 if dtype == torch.bfloat16 else 0


def _cache(dev, kd, vd, lens, page, max_pages, seed, dense):
    """(k, v as float8, k, v as uint8 views of the same memory, block table or None, lengths): paged through PagedCodes; dense
    [B, capacity, Hkv, D] with the NaN code in every row at or beyond len_b"""
    if not dense:
        pc = k8.PagedCodes(kd, vd, lens, page, max_pages, seed)
        return pc.k, pc.v, pc.ku, pc.vu, pc.table, pc.lens
    keep = torch.arange(kd.shape[2], device=dev).view(1, 1, -1, 1) < torch.as_tensor(lens, device=dev).view(-1, 1, 1, 1)
    ku = torch.where(keep, kd, torch.full_like(kd, k8.NAN_CODE)).transpose(1, 2).contiguous()
    vu = torch.where(keep, vd, torch.full_like(vd, k8.NAN_CODE)).transpose(1, 2).contiguous()
    return ku.view(k8.F8), vu.view(k8.F8), ku, vu, None, torch.tensor(lens, dtype=torch.int32, device=dev)


def _split_counts_agree(pkg, route, dtype, dense, **shape):
    """the FP8 plan and the 16-bit plan of the same shape: the same grids, launch for launch. Returns the split count."""
    make = ka._args_decode if route == "decode" else ka._args_prefill
    a = make(pkg, dtype=_dt(dtype), paged=not dense, **shape)
    base = pkg._lib.kvcache_plan(a) if route == "decode" else pkg._lib.kvprefill_plan(a)
    plan = k8.fp8_plan(pkg, a)
    assert [k[1:3] for k in plan] == [k[1:3] for k in base], (plan, base)
    assert plan[0][0].startswith("fasn_kvcache_fwd_fp8_kernel<" if route == "decode" else "fasn_kvprefill_fwd_fp8_kernel<")
    G = shape["H"] // shape["Hkv"]
    blocks = shape["B"] * shape["Hkv"] * (1 if route == "decode" else -(-shape["Sq"] // (128 // G)))
    return plan[0][1] // blocks


def _twin_case(pkg, dev, route, B, H, Hkv, Sq, D, dtype, page, max_pages, lens, n, causal, seed, qlens=None, dense=False, codes="random",
               q_std=0.5, what=""):
    """one exactness case: the FP8 call under power-of-two per-(batch, head) scales against the 16-bit call of the same route"""
    Smax = page * max_pages
    if dense:
        page, max_pages = Smax, 1
    nsplit = _split_counts_agree(pkg, route, dtype, dense, B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages)
    q = ks._rand((B, H, Sq, D), dtype, dev, seed, std=q_std)
    if codes == "random":
        kd, vd = k8.rand_codes((B, Hkv, Smax, D), seed + 1, dev), k8.rand_codes((B, Hkv, Smax, D), seed + 2, dev)
    else:   # all 254 finite codes, both zeros and the subnormals among them, walked with two strides coprime to 254
        fin = k8.finite_codes()[0].to(dev)
        idx = torch.arange(B * Hkv * Smax * D, device=dev)
        kd, vd = fin[(idx * 5 + 3) % 254].view(B, Hkv, Smax, D), fin[(idx * 11 + 1) % 254].view(B, Hkv, Smax, D)
        for t in (kd, vd):   # every code is in the rows the shortest non-empty batch element sees
            shortest = min(ln for ln in lens if ln > 0)
            assert torch.unique(t[0, 0, :shortest]).numel() == 254
    k, v, _ku, _vu, table, lens_t = _cache(dev, kd, vd, lens, page, max_pages, seed, dense)
    k_scale, v_scale = k8.scales_bh(k8.POW2_SCALES, B, Hkv, dev, seed + 3), k8.scales_bh(k8.POW2_SCALES, B, Hkv, dev, seed + 4)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    assert (route == "decode") == (qs is None and (H // Hkv) * Sq <= 128)
    out, lse = pkg.flash_attention_n_kvcache_fp8(q, k, v, lens_t, k_scale, v_scale, block_table=table, query_seqlens=qs, softmax_n_param=n,
                                                 is_causal=causal, return_lse=True)
    k16, v16 = k.to(dtype), v.to(dtype)   # exact; the stale rows become NaN, which the 16-bit calls never read either
    if route == "decode":
        call16 = lambda q_, k_, v_, **kw: pkg.flash_attention_n_kvcache(q_, k_, v_, lens_t, block_table=table, softmax_n_param=n, is_causal=causal, **kw)   # noqa: E731
    else:
        call16 = lambda q_, k_, v_, **kw: pkg.flash_attention_n_kvcache_prefill(q_, k_, v_, lens_t, block_table=table, query_seqlens=qs,   # noqa: E731
                                                                                softmax_n_param=n, is_causal=causal, **kw)
    out16, vs_h, want_lse = k8.sixteen_bit_twin(call16, q, k16, v16, k_scale, v_scale, None)
    k8.assert_bitwise(out, out16, vs_h, lse, want_lse, dtype, f"{what} ({nsplit} splits)")
    live = [ln > 0 and (qlens is None or qlens[b] > 0) for b, ln in enumerate(lens)]
    assert torch.isfinite(out).all() and any(live) and (out[live.index(True)] != 0).any()
    return nsplit


# ---------------------------------------------------------------- 1. exactness against the 16-bit path
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
def test_decode_equals_the_16_bit_call_paged(pkg, dev, D, dtype):
    """page 64 behind a shuffled table, lengths that are no multiple of 64 and an empty batch element, 8/2 heads, three positions, a tensor
    n with zeros, causal"""
    B, H, Hkv = 3, 8, 2
    n = ks._n_values((B, H), dev, 5)
    assert (n == 0).any() and (n > 0).any()
    _twin_case(pkg, dev, "decode", B, H, Hkv, 3, D, dtype, 64, 4, [0, 70, 200], n, True, 21, what="decode paged")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
def test_decode_equals_the_16_bit_call_dense(pkg, dev, D, dtype):
    """a dense cache of 200 rows (no multiple of 64), 2/2 heads, one position, not causal, a float n"""
    _twin_case(pkg, dev, "decode", 2, 2, 2, 1, D, dtype, 200, 1, [200, 37], 0.75, False, 22, dense=True, what="decode dense")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
def test_decode_equals_the_16_bit_call_over_several_splits(pkg, dev, D, dtype):
    """B = 1, one K/V head, capacity 2048: eight splits, the sink on split 0, the last split's range ragged"""
    nsplit = _twin_case(pkg, dev, "decode", 1, 2, 1, 1, D, dtype, 64, 32, [1999], 1.0, True, 23, what="decode splits")
    assert nsplit == 8


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
def test_prefill_equals_the_16_bit_call_ragged(pkg, dev, D, dtype):
    """the prefill kernels' one-split direct store: 8/2 heads, 40 positions in two row blocks, ragged query lengths with an empty one, a
    tensor n with zeros, causal, page 64 shuffled"""
    B, H, Hkv = 3, 8, 2
    n = ks._n_values((B, H), dev, 6)
    nsplit = _twin_case(pkg, dev, "prefill", B, H, Hkv, 40, D, dtype, 64, 4, [130, 64, 200], n, True, 24, qlens=[40, 7, 0], what="prefill ragged")
    assert nsplit == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
def test_prefill_equals_the_16_bit_call_over_several_splits(pkg, dev, D, dtype):
    """B = 1, one K/V head, 130 positions in three row blocks behind a cache of 2048: two splits and the FP8 combine kernel; not causal"""
    nsplit = _twin_case(pkg, dev, "prefill", 1, 2, 1, 130, D, dtype, 64, 32, [1999], 0.5, False, 25, what="prefill splits")
    assert nsplit == 2


# ---------------------------------------------------------------- 2. every code
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_every_code_equals_the_16_bit_call(pkg, dev, route, D, dtype):
    """K and V rows hold all 254 finite codes - both zeros, the subnormals, +-448 - and the widening must give the upcast's values for each:
    the same comparison (small queries keep the softmax from collapsing onto one key)"""
    if route == "decode":
        _twin_case(pkg, dev, route, 2, 8, 2, 2, D, dtype, 64, 3, [130, 70], 1.0, True, 31, codes="all", q_std=2.0 ** -7, what="every code decode")
    else:
        _twin_case(pkg, dev, route, 2, 8, 2, 33, D, dtype, 64, 3, [130, 70], 1.0, True, 32, qlens=[33, 9], codes="all", q_std=2.0 ** -7,
                   what="every code prefill")


# ---------------------------------------------------------------- 3. general scales against the fp32 reference
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_general_scales_against_the_reference(pkg, dev, route, D, dtype):
    """per-(batch, K/V head) scales that are no powers of two: kv_support.reference_rows on the dequantised cache, kv_support's gates. The
    operands are the 16-bit calls' (exact codes, 16-bit queries and weights), so are the gates"""
    B, H, Hkv, page, max_pages = 3, 8, 2, 64, 4
    Sq, qlens = (3, None) if route == "decode" else (40, [40, 7, 0])
    lens = [130, 64, 200]
    Smax = page * max_pages
    q = ks._rand((B, H, Sq, D), dtype, dev, 41)
    kd, vd = k8.rand_codes((B, Hkv, Smax, D), 42, dev), k8.rand_codes((B, Hkv, Smax, D), 43, dev)
    pc = k8.PagedCodes(kd, vd, lens, page, max_pages, 44)
    gen = torch.Generator().manual_seed(45)
    k_scale = (0.3 + 2.7 * torch.rand(B, Hkv, generator=gen)).to(dev)
    v_scale = (0.05 + 1.5 * torch.rand(B, Hkv, generator=gen)).to(dev)
    n = ks._n_values((B, H), dev, 7)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache_fp8(q, pc.k, pc.v, pc.lens, k_scale, v_scale, block_table=pc.table, query_seqlens=qs,
                                                 softmax_n_param=n, return_lse=True)
    kg = k8.up(k8.visible(kd, lens)) * k_scale[:, :, None, None]
    vg = k8.up(k8.visible(vd, lens)) * v_scale[:, :, None, None]
    o_ref, lse_ref = ks.reference_rows(q, kg, vg, lens, qlens or [Sq] * B, n, True)
    ks._check(out, o_ref, dtype, f"general scales {route} out")
    ks._check_lse(lse, lse_ref, f"general scales {route} lse")
    # one Python float for every head is the same call
    out1, lse1 = pkg.flash_attention_n_kvcache_fp8(q, pc.k, pc.v, pc.lens, 0.7, torch.tensor(1.3, device=dev), block_table=pc.table, query_seqlens=qs,
                                                   softmax_n_param=n, return_lse=True)
    o_ref, lse_ref = ks.reference_rows(q, k8.up(k8.visible(kd, lens)) * 0.7, k8.up(k8.visible(vd, lens)) * 1.3, lens, qlens or [Sq] * B, n, True)
    ks._check(out1, o_ref, dtype, f"float scales {route} out")
    ks._check_lse(lse1, lse_ref, f"float scales {route} lse")


# ---------------------------------------------------------------- 4. stale memory
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_stale_rows_and_pages_hold_nan_codes(pkg, dev, route, dtype):
    """rows at or beyond len_b and pages no table entry needs are 0x7f: the result is that of a cache with zeros there, bit for bit, and
    finite. A NaN code in a visible K row makes exactly the rows that see it NaN."""
    B, H, Hkv, D, page, max_pages = 2, 8, 2, 64, 64, 4
    Sq = 4 if route == "decode" else 40
    lens = [150, 77]
    Smax = page * max_pages
    q = ks._rand((B, H, Sq, D), dtype, dev, 51)
    kd, vd = k8.rand_codes((B, Hkv, Smax, D), 52, dev), k8.rand_codes((B, Hkv, Smax, D), 53, dev)
    pc = k8.PagedCodes(kd, vd, lens, page, max_pages, 54)
    scales = (torch.tensor([[0.5, 1.25], [2.0, 0.75]], device=dev), torch.tensor([[1.5, 0.25], [1.0, 3.0]], device=dev))
    assert (pc.ku[pc.poison] == k8.NAN_CODE).all() and int(k8.is_nan_code(pc.ku).sum()) > Hkv * D * page   # the poison is there
    out, lse = pkg.flash_attention_n_kvcache_fp8(q, pc.k, pc.v, pc.lens, *scales, block_table=pc.table, return_lse=True)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    clean_k, clean_v = pc.ku.clone(), pc.vu.clone()
    clean_k[k8.is_nan_code(clean_k)] = 0
    clean_v[k8.is_nan_code(clean_v)] = 0
    out0, lse0 = pkg.flash_attention_n_kvcache_fp8(q, clean_k.view(k8.F8), clean_v.view(k8.F8), pc.lens, *scales, block_table=pc.table, return_lse=True)
    assert torch.equal(ks._bits(out), ks._bits(out0)) and torch.equal(lse, lse0)
    # a NaN code in K row j of (b, hkv) = (0, 1): position i sees it iff j <= i + len_b - Sq
    b, hkv, j = 0, 1, lens[0] - 2
    pid = int(pc.table[b, j // page])
    pc.ku[pid, j % page, hkv, 5] = 0xFF
    out2, lse2 = pkg.flash_attention_n_kvcache_fp8(q, pc.k, pc.v, pc.lens, *scales, block_table=pc.table, return_lse=True)
    G = H // Hkv
    hit = torch.zeros(B, H, Sq, dtype=torch.bool, device=dev)
    hit[b, hkv * G:(hkv + 1) * G] = (torch.arange(Sq, device=dev) + lens[0] - Sq >= j)
    assert hit.any() and not hit[b, hkv * G].all()
    assert torch.isnan(out2[hit]).all()   # (every feature of those rows; their lse is whatever a NaN sum gives)
    assert torch.equal(ks._bits(out2[~hit]), ks._bits(out[~hit])) and torch.equal(lse2[~hit], lse[~hit])


# ---------------------------------------------------------------- 5. the quantising append
def _new_rows(shape, dtype, scale_bh, dev, seed):
    """k_new / v_new [B, Hkv, Sq, D]: the append's witnesses times the head's scale (so that they land on the ties, the subnormals, the
    saturation of every head), then random values of a few magnitudes"""
    B, Hkv, Sq, D = shape
    w = k8.append_witnesses(torch.float32)
    flat = torch.randn(B * Hkv, Sq * D, generator=torch.Generator().manual_seed(seed)) * torch.tensor([0.01, 1.0, 50.0, 400.0]).repeat(Sq * D // 4)
    flat[:, :w.numel()] = w
    x = flat.view(B, Hkv, Sq, D) * scale_bh.cpu()[:, :, None, None]
    return x.to(dtype).to(dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_append_bytes_equal_the_reference_formula(pkg, dev, route, D, dtype):
    """cache bytes after k_new / v_new: code = rne_e4m3(clamp(float(x) / s, -448, 448)) byte for byte (a NaN: any NaN code), rows that are not
    appended untouched bytewise, positions at or beyond the capacity dropped, a ragged qlen (prefill route), cache_seqlens unchanged.
    Decode route: a dense cache; prefill route: page 64 behind a shuffled table."""
    B, H, Hkv = 2, 8, 2
    dense = route == "decode"
    Sq, qlens = (4, None) if dense else (70, [70, 9])
    page, max_pages = (200, 1) if dense else (64, 4)
    capacity = page * max_pages
    lens = [capacity - 2, 61] if dense else [capacity - 30, 3]   # batch element 0 runs into the capacity
    assert D * Sq >= k8.append_witnesses(dtype).numel()
    gen = torch.Generator().manual_seed(61)
    n_pages = B if dense else B * max_pages + 1
    ku = torch.randint(0, 256, (n_pages, page, Hkv, D), generator=gen, dtype=torch.int32).to(torch.uint8).to(dev)
    vu = torch.randint(0, 256, (n_pages, page, Hkv, D), generator=gen, dtype=torch.int32).to(torch.uint8).to(dev)
    table = None if dense else torch.randperm(n_pages, generator=gen)[:B * max_pages].view(B, max_pages).to(torch.int32).to(dev)
    k_scale = torch.tensor([[1.0, 0.3], [2.0 ** -3, 3.0]], device=dev)
    v_scale = torch.tensor([[16.0, 1.7e-3], [0.7, 1.0]], device=dev)
    k_new, v_new = _new_rows((B, Hkv, Sq, D), dtype, k_scale, dev, 62), _new_rows((B, Hkv, Sq, D), dtype, v_scale, dev, 63)
    assert torch.isnan(k_new).any() and torch.isinf(k_new).any() and (k_new == 0).any()
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    want_k, want_v = ku.cpu().clone(), vu.cpu().clone()
    codes_k = k8.quantise(k_new, k_scale.cpu()[:, :, None, None])
    codes_v = k8.quantise(v_new, v_scale.cpu()[:, :, None, None])
    written = dropped = 0
    for b in range(B):
        for i in range(Sq if qlens is None else qlens[b]):
            pos = lens[b] + i
            if pos >= capacity:
                dropped += 1
                continue
            pid = b if dense else int(table[b, pos // page])
            want_k[pid, pos % page] = codes_k[b, :, i]
            want_v[pid, pos % page] = codes_v[b, :, i]
            written += 1
    assert dropped > 0 and written > 0
    q = ks._rand((B, H, Sq, D), dtype, dev, 64)
    pkg.flash_attention_n_kvcache_fp8(q, ku.view(k8.F8), vu.view(k8.F8), lens_t, k_scale, v_scale, block_table=table, k_new=k_new, v_new=v_new,
                                      query_seqlens=qs)
    assert lens_t.tolist() == lens
    for name, got, want in (("k", ku.cpu(), want_k), ("v", vu.cpu(), want_v)):
        nan = k8.is_nan_code(want)
        assert k8.is_nan_code(got[nan]).all(), f"{name}: a NaN code of the reference is no NaN code in the cache"
        diff = (got != want) & ~nan
        assert not diff.any(), (f"{name}: {int(diff.sum())} bytes differ, first at {diff.nonzero()[0].tolist()}: "
                                f"got {int(got[diff][0]):#x}, want {int(want[diff][0]):#x}")
    # the witnesses did their work: saturation codes, subnormal codes and both zeros were written
    fresh = codes_k[0, 0, 0]
    assert (fresh == 0x7E).any() and (fresh == 0xFE).any() and (fresh == 0x00).any() and (fresh == 0x80).any() and ((fresh > 0) & (fresh < 8)).any()


# ---------------------------------------------------------------- 6. graph
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_graph_replay_follows_lengths_and_scales(pkg, dev, route):
    """captured once; cache_seqlens, query_seqlens and both scales change in place; the replay equals the eager call bit for bit"""
    dtype, B, H, Hkv, D, page, max_pages = torch.bfloat16, 2, 8, 2, 64, 64, 4
    Sq = 2 if route == "decode" else 40
    Smax = page * max_pages
    q = ks._rand((B, H, Sq, D), dtype, dev, 71)
    kd, vd = k8.rand_codes((B, Hkv, Smax, D), 72, dev), k8.rand_codes((B, Hkv, Smax, D), 73, dev)
    pc = k8.PagedCodes(kd, vd, [Smax, Smax], page, max_pages, 74)
    lens_t = torch.tensor([100, 31], dtype=torch.int32, device=dev)
    qs = None if route == "decode" else torch.tensor([40, 5], dtype=torch.int32, device=dev)
    k_scale = torch.tensor([[1.0, 0.5], [0.3, 2.0]], device=dev)
    v_scale = torch.full((Hkv,), 0.7, device=dev)
    call = lambda: pkg.flash_attention_n_kvcache_fp8(q, pc.k, pc.v, lens_t, k_scale, v_scale, block_table=pc.table, query_seqlens=qs,   # noqa: E731
                                                     return_lse=True)
    g, (out, lse) = ks._capture(call)
    g.replay()
    first = (out.clone(), lse.clone())
    eager = call()
    assert torch.equal(ks._bits(first[0]), ks._bits(eager[0])) and torch.equal(first[1], eager[1])
    lens_t.copy_(torch.tensor([255, 64], dtype=torch.int32))
    if qs is not None:
        qs.copy_(torch.tensor([13, 40], dtype=torch.int32))
    k_scale.mul_(1.7)
    v_scale.copy_(torch.tensor([0.1, 4.0]))
    g.replay()
    eager = call()
    assert torch.equal(ks._bits(out), ks._bits(eager[0])) and torch.equal(lse, eager[1])
    assert not torch.equal(ks._bits(out), ks._bits(first[0]))
