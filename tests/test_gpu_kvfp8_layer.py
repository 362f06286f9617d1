"""The FP8 K/V cache's layer calls on the GPU. flash_attention_n_kvcache_fp8_window bit for bit against flash_attention_n_kvcache_window on
the exactly upcast cache under power-of-two scales, with the pages below the window gone, and against the fp32 reference of
tests/kv_support.py under general scales; the rotate-quantise-append of flash_attention_n_kvcache_fp8_rope byte for byte against the
quantised eager rotation (tests/kv_fp8.py's formula on tests/kv_support.py's rotation); the rope call bit for bit against the composed
route - eager rotation, then flash_attention_n_kvcache_fp8 / _fp8_window - under any scales; graph replay with the lengths and the scales
changed in place; and one layer end to end on a paged FP8 cache: prompt, chunk, three decode steps."""
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
GENERAL = (0.3, 3.0, 1.7e-3)
_ids = lambda d: str(d).split(".")[-1]   # noqa: E731


def _dt(dtype):
    return 1 if dtype == torch.bfloat16 else 0


def _route(H, Hkv, Sq, qlens):
    return "decode" if qlens is None and (H // Hkv) * Sq <= 128 else "prefill"


def _window_nsplit(pkg, dtype, W, B, H, Hkv, Sq, D, page, max_pages, qlens=None):
    """the split count of the FP8 window plan, which has the grids of the 16-bit window plan of the same shape and window"""
    route = _route(H, Hkv, Sq, qlens)
    make = ka._args_decode if route == "decode" else ka._args_prefill
    a = make(pkg, dtype=_dt(dtype), B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages)
    win = ka._win(pkg, window=W)
    base = pkg._lib.kvcache_window_plan(a, win) if route == "decode" else pkg._lib.kvprefill_window_plan(a, win)
    plan = pkg._lib.kvfp8_window_plan(a, k8._fp8(pkg), win)
    assert [k[1:3] for k in plan] == [k[1:3] for k in base], (plan, base)
    assert plan[0][0].startswith("fasn_kvcache_fwd_fp8_window_kernel<" if route == "decode" else "fasn_kvprefill_fwd_fp8_window_kernel<")
    G = H // Hkv
    blocks = B * Hkv * (1 if route == "decode" else -(-Sq // (128 // G)))
    nsplit = plan[0][1] // blocks
    assert (len(plan) == 2) == (route == "decode" or nsplit > 1)
    return nsplit


def _poison_below(pc, lens, qlens, W):
    """every cache row below first_b = 64 * floor(max(0, len_b - qlen_b - W + 1) / 64) becomes the NaN code, and the table entry of every
    page wholly below first_b names the poison page. Returns the rows poisoned."""
    tbl = pc.table.cpu()
    rows = 0
    for b, (ln, ql) in enumerate(zip(lens, qlens)):
        first = ks._first(ln, ql, W)
        rows += first
        for s in range(-(-first // pc.page)):
            pid, cnt = int(tbl[b, s]), min(pc.page, first - s * pc.page)
            pc.ku[pid, :cnt] = k8.NAN_CODE
            pc.vu[pid, :cnt] = k8.NAN_CODE
        pc.table[b, :first // pc.page] = pc.poison
    return rows


def _same(a, b):
    out_a, lse_a = a
    out_b, lse_b = b
    return torch.equal(ks._bits(out_a), ks._bits(out_b)) and torch.equal(lse_a, lse_b)


# ---------------------------------------------------------------- 1. the window call = the 16-bit window call, bit for bit
def _window_twin(pkg, dev, B, H, Hkv, Sq, D, dtype, page, max_pages, lens, n, W, seed, qlens=None, what=""):
    Smax = page * max_pages
    nsplit = _window_nsplit(pkg, dtype, W, B, H, Hkv, Sq, D, page, max_pages, qlens)
    q = ks._rand((B, H, Sq, D), dtype, dev, seed)
    kd, vd = k8.rand_codes((B, Hkv, Smax, D), seed + 1, dev), k8.rand_codes((B, Hkv, Smax, D), seed + 2, dev)
    pc = k8.PagedCodes(kd, vd, lens, page, max_pages, seed)
    k_scale, v_scale = k8.scales_bh(k8.POW2_SCALES, B, Hkv, dev, seed + 3), k8.scales_bh(k8.POW2_SCALES, B, Hkv, dev, seed + 4)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    call8 = lambda: pkg.flash_attention_n_kvcache_fp8_window(q, pc.k, pc.v, pc.lens, k_scale, v_scale, W, block_table=pc.table,   # noqa: E731
                                                             query_seqlens=qs, softmax_n_param=n, return_lse=True)
    out, lse = call8()
    k16, v16 = pc.k.to(dtype), pc.v.to(dtype)   # exact; the stale rows become NaN, which the 16-bit call never reads either
    call16 = lambda q_, k_, v_, **kw: pkg.flash_attention_n_kvcache_window(q_, k_, v_, pc.lens, W, block_table=pc.table, query_seqlens=qs,   # noqa: E731
                                                                           softmax_n_param=n, **kw)
    out16, vs_h, want_lse = k8.sixteen_bit_twin(call16, q, k16, v16, k_scale, v_scale, None)
    k8.assert_bitwise(out, out16, vs_h, lse, want_lse, dtype, f"{what} W={W} ({nsplit} splits)")
    ql = qlens or [Sq] * B
    live = [ln > 0 and ql[b] > 0 for b, ln in enumerate(lens)]
    assert torch.isfinite(out).all() and any(live) and (out[live.index(True)] != 0).any()
    if W >= Smax:   # a window at or beyond the capacity: the causal FP8 call
        full = pkg.flash_attention_n_kvcache_fp8(q, pc.k, pc.v, pc.lens, k_scale, v_scale, block_table=pc.table, query_seqlens=qs, softmax_n_param=n,
                                                 is_causal=True, return_lse=True)
        assert _same((out, lse), full), f"{what}: W={W} differs from the causal FP8 call"
    # the pages below the window are gone: NaN codes in every row below first_b, the poison page in their table entries
    rows = _poison_below(pc, lens, ql, W)
    assert _same(call8(), (out, lse)), f"{what} W={W}: the result changed when {rows} rows below the window were poisoned"
    return nsplit, rows


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("W", [1, 70, 4096])
def test_window_decode_equals_the_16_bit_window_call(pkg, dev, W, D, dtype):
    """(3, 8/2, Sq 3), page 64 x 4 behind a shuffled table, lengths [0, 70, 200], a tensor n with zeros. W = 4096 is beyond the capacity
    and must also equal flash_attention_n_kvcache_fp8(is_causal=True). W = 1 leaves one V row times a weight below 1 per output, so where
    v_scale is 2^-3 far more fp16 results are subnormal than under a wider window: the fp32 reference of tests/kv_support.py, run on the
    CPU on these generators, puts 0 % to 5.6 % of the elements there depending on which heads the seed hands that scale to, and 1.5 % at
    this seed for both head dims (W = 70 / 4096: at most 0.2 %) - inside the 5 % the exact comparison may leave out."""
    B, H, Hkv = 3, 8, 2
    n = ks._n_values((B, H), dev, 5)
    assert (n == 0).any() and (n > 0).any()
    _nsplit, rows = _window_twin(pkg, dev, B, H, Hkv, 3, D, dtype, 64, 4, [0, 70, 200], n, W, 111, what="window decode")
    assert (rows > 0) == (W < 4096)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
def test_window_decode_equals_the_16_bit_window_call_over_several_splits(pkg, dev, D, dtype):
    """(1, 2/1, Sq 1), page 64 x 32, length 1999, W = 1000: the splits share [tlo, tiles_b), the sink sits on split 0"""
    nsplit, rows = _window_twin(pkg, dev, 1, 2, 1, 1, D, dtype, 64, 32, [1999], 1.0, 1000, 102, what="window decode splits")
    assert nsplit > 1 and rows > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
def test_window_prefill_equals_the_16_bit_window_call_ragged(pkg, dev, D, dtype):
    """(3, 8/2, Sq 40), query_seqlens [40, 0, 17], W = 50: two row blocks, one split, the direct store with v_scale"""
    B, H, Hkv = 3, 8, 2
    n = ks._n_values((B, H), dev, 6)
    nsplit, rows = _window_twin(pkg, dev, B, H, Hkv, 40, D, dtype, 64, 4, [200, 64, 130], n, 50, 103, qlens=[40, 0, 17], what="window prefill ragged")
    assert nsplit == 1 and rows > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
def test_window_prefill_equals_the_16_bit_window_call_behind_a_long_cache(pkg, dev, D, dtype):
    """(1, 2/1, Sq 130) behind a cache of 1999 keys, capacity 2048, W = 700: three row blocks whose walks start far above tile 0.
    The split count is read from the plan: it is the 16-bit window plan's, and under the family's split rule (at least 16 tiles per
    split of a 128-row workgroup) the 13 tiles a window of 700 can touch are ONE split - the several-split route is the next test's."""
    nsplit, rows = _window_twin(pkg, dev, 1, 2, 1, 130, D, dtype, 64, 32, [1999], 0.5, 700, 104, what="window prefill long cache")
    assert nsplit == 1 and rows > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
def test_window_prefill_equals_the_16_bit_window_call_over_several_splits(pkg, dev, D, dtype):
    """(1, 2/1, Sq 130) behind a cache of 3999 keys, capacity 4096, W = 1900: the smallest window whose 32 tiles give the prefill plan two
    splits (asserted from the plan) - partials, the FP8 combine kernel with v_scale - with 30 tiles below the window gone"""
    nsplit, rows = _window_twin(pkg, dev, 1, 2, 1, 130, D, dtype, 64, 64, [3999], 0.5, 1900, 105, what="window prefill splits")
    assert nsplit > 1 and rows > 0


# ---------------------------------------------------------------- 2. general scales against the fp32 reference
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_window_general_scales_against_the_reference(pkg, dev, route, D, dtype):
    """scales 0.3, 3.0, 1.7e-3 per (b, hkv), W = 70: kv_support.reference on the dequantised visible cache under _win_mask, the gates the
    FP8 general-scale cases already stand under"""
    B, H, Hkv, page, max_pages, W = 3, 8, 2, 64, 4, 70
    Sq, qlens = (3, None) if route == "decode" else (40, [40, 7, 0])
    lens = [130, 64, 200]
    Smax = page * max_pages
    assert _route(H, Hkv, Sq, qlens) == route
    q = ks._rand((B, H, Sq, D), dtype, dev, 41)
    kd, vd = k8.rand_codes((B, Hkv, Smax, D), 42, dev), k8.rand_codes((B, Hkv, Smax, D), 43, dev)
    pc = k8.PagedCodes(kd, vd, lens, page, max_pages, 44)
    k_scale, v_scale = k8.scales_bh(GENERAL, B, Hkv, dev, 45), k8.scales_bh(GENERAL, B, Hkv, dev, 46)
    n = ks._n_values((B, H), dev, 7)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    ql = qlens or [Sq] * B
    _poison_below(pc, lens, ql, W)
    out, lse = pkg.flash_attention_n_kvcache_fp8_window(q, pc.k, pc.v, pc.lens, k_scale, v_scale, W, block_table=pc.table, query_seqlens=qs,
                                                        softmax_n_param=n, return_lse=True)
    kg = k8.up(k8.visible(kd, lens)) * k_scale[:, :, None, None]
    vg = k8.up(k8.visible(vd, lens)) * v_scale[:, :, None, None]
    vis = ks._win_mask(lens, ql, Sq, Smax, W, dev)
    o_ref, lse_ref = ks.reference(q, kg, vg, vis, n)
    pad = (torch.arange(Sq, device=dev).view(1, 1, Sq) >= torch.tensor(ql, device=dev).view(B, 1, 1)).expand(B, H, Sq)
    lse_ref = torch.where(pad, torch.full_like(lse_ref, float("-inf")), lse_ref)   # padding positions: 0 / -inf whatever n is
    o_ref = torch.where(pad[..., None], torch.zeros_like(o_ref), o_ref)
    ks._check(out, o_ref, dtype, f"window general scales {route} out")
    ks._check_lse(lse, lse_ref, f"window general scales {route} lse")


# ---------------------------------------------------------------- 3. rotate-quantise-append, byte for byte
def _rope_tables(rows, rd, dev, dtype, fp32):
    return ks._tables(rows, rd, dev, torch.float32 if fp32 else dtype)


def _witness_rows(k_new, scales_b0, dtype):
    """row 0 of batch element 0 carries the append's witnesses, spread over the K/V heads and times the head's scale, padded with 1.5"""
    Hkv, D = k_new.shape[1], k_new.shape[3]
    w = k8.append_witnesses(torch.float32)
    assert Hkv * D >= w.numel()
    flat = torch.full((Hkv * D,), 1.5)
    flat[:w.numel()] = w
    k_new[0, :, 0] = (flat.view(Hkv, D) * scales_b0.cpu().view(Hkv, 1)).to(dtype).to(k_new.device)


ROPE_CASES = {"decode_1": (1, None, True), "decode_3": (3, None, False), "prefill_40": (40, [40, 40, 9], False)}   # Sq, qlens, dense


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", sorted(ROPE_CASES))
def test_rope_append_bytes_equal_the_quantised_eager_rotation(pkg, dev, case, D, dtype):
    """K bytes of the rows cache_seqlens[b] + i, i < qlen_b = quantise(rotate(k_new).to(dtype), k_scale); V bytes = quantise(v_new, v_scale);
    every other byte of both caches untouched - rows i >= qlen_b, the rows of batch element 1 that fall off the end of the cache, other
    pages. Batch element 0 is empty and its row 0 (position 0: cos 1, sin 0) carries the append's witnesses. Half-split and interleaved,
    rotary_dim D and D / 2, fp32 and 16-bit tables, scales that are no powers of two."""
    Sq, qlens, dense = ROPE_CASES[case]
    B, H, Hkv = 3, 8, 2
    page, max_pages = (192, 1) if dense else (64, 3)
    capacity = page * max_pages
    ql = qlens or [Sq] * B
    lens = [0, capacity - ql[1] + 1, 61]   # batch element 1: its last new row is at the capacity, and dropped
    assert _route(H, Hkv, Sq, qlens) == case.split("_")[0]
    k_scale = torch.tensor([[1.0, 0.3], [1.7e-3, 3.0], [0.3, 2.0 ** -3]], device=dev)
    v_scale = torch.tensor([[0.3, 1.0], [3.0, 0.7], [16.0, 1.7e-3]], device=dev)
    gen = torch.Generator().manual_seed(61)
    n_pages = B if dense else B * max_pages + 1
    table = None if dense else torch.randperm(n_pages, generator=gen)[:B * max_pages].view(B, max_pages).to(torch.int32).to(dev)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    q = ks._rand((B, H, Sq, D), dtype, dev, 64)
    pos = torch.tensor(lens).view(B, 1) + torch.arange(Sq).view(1, Sq)
    for interleaved, rd, fp32 in ((False, D, True), (True, D // 2, False), (False, D // 2, False), (True, D, True)):
        what = f"{case} interleaved={interleaved} rotary_dim={rd} fp32 tables={fp32}"
        ku = torch.randint(0, 256, (n_pages, page, Hkv, D), generator=gen, dtype=torch.int32).to(torch.uint8).to(dev)
        vu = torch.randint(0, 256, (n_pages, page, Hkv, D), generator=gen, dtype=torch.int32).to(torch.uint8).to(dev)
        k_new = (ks._rand((B, Hkv, Sq, D), torch.float32, dev, 62, std=1.0) * k_scale[:, :, None, None] * 40.0).to(dtype)
        v_new = (ks._rand((B, Hkv, Sq, D), torch.float32, dev, 63, std=1.0) * v_scale[:, :, None, None] * 40.0).to(dtype)
        _witness_rows(k_new, k_scale[0], dtype)
        _witness_rows(v_new, v_scale[0], dtype)
        assert torch.isnan(k_new[0, :, 0]).any() and torch.isinf(k_new[0, :, 0]).any()
        cos, sin = _rope_tables(capacity, rd, dev, dtype, fp32)
        assert (cos[0] == 1).all() and (sin[0] == 0).all()
        want_k, want_v = ku.cpu().clone(), vu.cpu().clone()
        codes_k = k8.quantise(ks._rotate(k_new, pos, cos, sin, interleaved).to(dtype), k_scale.cpu()[:, :, None, None])
        codes_v = k8.quantise(v_new, v_scale.cpu()[:, :, None, None])
        written = dropped = 0
        for b in range(B):
            for i in range(ql[b]):
                p = lens[b] + i
                if p >= capacity:
                    dropped += 1
                    continue
                pid = b if dense else int(table[b, p // page])
                want_k[pid, p % page] = codes_k[b, :, i]
                want_v[pid, p % page] = codes_v[b, :, i]
                written += 1
        assert dropped == 1 and written == sum(ql) - 1
        pkg.flash_attention_n_kvcache_fp8_rope(q, ku.view(k8.F8), vu.view(k8.F8), lens_t, k_scale, v_scale, cos, sin, block_table=table, k_new=k_new,
                                               v_new=v_new, query_seqlens=qs, rotary_interleaved=interleaved)
        assert lens_t.tolist() == lens
        for name, got, want in (("k", ku.cpu(), want_k), ("v", vu.cpu(), want_v)):
            nan = k8.is_nan_code(want)
            assert k8.is_nan_code(got[nan]).all(), f"{what} {name}: a NaN code of the reference is no NaN code in the cache"
            diff = (got != want) & ~nan
            assert not diff.any(), (f"{what} {name}: {int(diff.sum())} bytes differ, first at {diff.nonzero()[0].tolist()}: "
                                    f"got {int(got[diff][0]):#x}, want {int(want[diff][0]):#x}")
        # the witnesses did their work: saturation codes, subnormal codes and both zeros among the codes of position 0
        fresh = torch.cat([codes_v[0, :, 0].flatten(), codes_k[0, :, 0].flatten()])
        assert (fresh == 0x7E).any() and (fresh == 0xFE).any() and (fresh == 0x00).any() and (fresh == 0x80).any() and ((fresh > 0) & (fresh < 8)).any()
        if rd < D:   # the unrotated features are quantised, not copied: the key's witnesses beyond rotary_dim kept their codes
            assert torch.equal(codes_k[0, :, 0, rd:], k8.quantise(k_new[0, :, 0, rd:], k_scale.cpu()[0, :, None]))


# ---------------------------------------------------------------- 4. the rope call = the composed route, bit for bit
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("W", [None, 96])
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_rope_call_equals_eager_rotation_then_the_fp8_call(pkg, dev, route, W, D, dtype):
    """out, lse and both caches of flash_attention_n_kvcache_fp8_rope(window=W) = those of flash_attention_n_kvcache_fp8 / _fp8_window on a
    clone of the cache with query and k_new rotated by eager torch (rounded to dtype), under scales that are no powers of two; likewise the
    queries-only call"""
    B, H, Hkv, page, max_pages = 3, 8, 2, 64, 4
    Sq, qlens = (3, None) if route == "decode" else (40, [40, 0, 17])
    assert _route(H, Hkv, Sq, qlens) == route
    ql = qlens or [Sq] * B
    lens = [150, 64, 201]
    Smax = page * max_pages
    kd, vd = k8.rand_codes((B, Hkv, Smax, D), 82, dev), k8.rand_codes((B, Hkv, Smax, D), 83, dev)
    pc = k8.PagedCodes(kd, vd, [ln + Sq for ln in lens], page, max_pages, 84)   # (the pages the appended rows land in are there)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    k_scale, v_scale = k8.scales_bh(GENERAL, B, Hkv, dev, 85), k8.scales_bh(GENERAL, B, Hkv, dev, 86)
    n = ks._n_values((B, H), dev, 8)
    q = ks._rand((B, H, Sq, D), dtype, dev, 87)
    k_new, v_new = ks._rand((B, Hkv, Sq, D), dtype, dev, 88, std=1.0), ks._rand((B, Hkv, Sq, D), dtype, dev, 89, std=1.0)
    interleaved, rd = (D == 128), (D if dtype == torch.float16 else D // 2)
    cos, sin = _rope_tables(Smax, rd, dev, dtype, fp32=(route == "decode"))
    i = torch.arange(Sq).view(1, Sq)

    def composed(kc, vc, q_, kn, vn):
        kw = dict(block_table=pc.table, k_new=kn, v_new=vn, query_seqlens=qs, softmax_n_param=n, return_lse=True)
        if W is None:
            return pkg.flash_attention_n_kvcache_fp8(q_, kc.view(k8.F8), vc.view(k8.F8), lens_t, k_scale, v_scale, is_causal=True, **kw)
        return pkg.flash_attention_n_kvcache_fp8_window(q_, kc.view(k8.F8), vc.view(k8.F8), lens_t, k_scale, v_scale, W, **kw)

    for append in (True, False):
        what = f"{route} W={W} append={append}"
        ka_, va_ = pc.ku.clone(), pc.vu.clone()
        kb_, vb_ = pc.ku.clone(), pc.vu.clone()
        got = pkg.flash_attention_n_kvcache_fp8_rope(q, ka_.view(k8.F8), va_.view(k8.F8), lens_t, k_scale, v_scale, cos, sin, block_table=pc.table,
                                                     k_new=k_new if append else None, v_new=v_new if append else None, query_seqlens=qs,
                                                     softmax_n_param=n, return_lse=True, window=W, rotary_interleaved=interleaved)
        # p_i = i + len_b - qlen_b, len_b = cache_seqlens[b] + (qlen_b if appended else 0); the key rows sit at cache_seqlens[b] + i
        p_q = i + torch.tensor([ln + (0 if append else -ql[b]) for b, ln in enumerate(lens)]).view(B, 1)
        q_rot = ks._rotate(q, p_q, cos, sin, interleaved)
        k_rot = ks._rotate(k_new, i + torch.tensor(lens).view(B, 1), cos, sin, interleaved) if append else None
        want = composed(kb_, vb_, q_rot, k_rot, v_new if append else None)
        live = torch.tensor([x > 0 for x in ql], device=dev)
        assert torch.isfinite(got[0]).all() and (got[0][live] != 0).any()
        assert torch.equal(ks._bits(got[0]), ks._bits(want[0])), f"{what}: out differs at {int((ks._bits(got[0]) != ks._bits(want[0])).sum())} elements"
        assert torch.equal(got[1], want[1]), f"{what}: lse differs"
        assert torch.equal(ka_, kb_) and torch.equal(va_, vb_), f"{what}: the caches differ"
        assert torch.equal(ka_, pc.ku) != append, what   # the append wrote, the queries-only call did not


# ---------------------------------------------------------------- 5. graph replay
def test_graph_replay_follows_lengths_and_scales(pkg, dev):
    """one flash_attention_n_kvcache_fp8_rope(window=128) decode step, captured once; cache_seqlens, k_scale and v_scale change in place; the
    replay equals the eager call on the same state bit for bit, the cache bytes included"""
    dtype, B, H, Hkv, D, page, max_pages, W = torch.bfloat16, 2, 8, 2, 64, 64, 8, 128
    Smax = page * max_pages
    q = ks._rand((B, H, 1, D), dtype, dev, 71)
    k_new, v_new = ks._rand((B, Hkv, 1, D), dtype, dev, 75, std=1.0), ks._rand((B, Hkv, 1, D), dtype, dev, 76, std=1.0)
    kd, vd = k8.rand_codes((B, Hkv, Smax, D), 72, dev), k8.rand_codes((B, Hkv, Smax, D), 73, dev)
    pc = k8.PagedCodes(kd, vd, [Smax, Smax], page, max_pages, 74)
    lens_t = torch.tensor([100, 31], dtype=torch.int32, device=dev)
    k_scale = torch.tensor([[1.0, 0.5], [0.3, 2.0]], device=dev)
    v_scale = torch.full((Hkv,), 0.7, device=dev)
    cos, sin = ks._tables(Smax, D, dev, torch.float32)
    step = lambda kc, vc: pkg.flash_attention_n_kvcache_fp8_rope(q, kc.view(k8.F8), vc.view(k8.F8), lens_t, k_scale, v_scale, cos, sin,   # noqa: E731
                                                                 block_table=pc.table, k_new=k_new, v_new=v_new, return_lse=True, window=W)
    g, (out, lse) = ks._capture(lambda: step(pc.ku, pc.vu))
    g.replay()
    first = (out.clone(), lse.clone())
    k2, v2 = pc.ku.clone(), pc.vu.clone()
    assert _same(first, step(k2, v2)) and torch.equal(k2, pc.ku) and torch.equal(v2, pc.vu)
    before_k = pc.ku.clone()
    lens_t.copy_(torch.tensor([400, 201], dtype=torch.int32))
    k_scale.mul_(1.7)
    v_scale.copy_(torch.tensor([0.1, 4.0]))
    k2, v2 = pc.ku.clone(), pc.vu.clone()
    g.replay()
    eager = step(k2, v2)
    assert _same((out, lse), eager) and not _same((out, lse), first)
    assert torch.equal(k2, pc.ku) and torch.equal(v2, pc.vu) and not torch.equal(pc.ku, before_k)


# ---------------------------------------------------------------- 6. one layer end to end
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_layer_end_to_end_on_a_paged_fp8_cache(pkg, dev, dtype):
    """(2, 8/2, D 64, page 64): a ragged prompt through the prefill kernels, a chunk, three decode steps, each with rotary embedding and
    W = 96, cache_seqlens advanced here. Every step against kv_support.reference on the dequantised cache as it then stands (gathered
    through the table) with eagerly rotated queries; the final cache bytes against the quantised eager rotation of everything appended."""
    B, H, Hkv, D, page, max_pages, W = 2, 8, 2, 64, 64, 4, 96
    capacity = page * max_pages
    gen = torch.Generator().manual_seed(91)
    n_pages = B * max_pages + 2
    ku = torch.full((n_pages, page, Hkv, D), k8.NAN_CODE, dtype=torch.uint8, device=dev)
    vu = torch.full((n_pages, page, Hkv, D), k8.NAN_CODE, dtype=torch.uint8, device=dev)
    table = torch.randperm(n_pages, generator=gen)[:B * max_pages].view(B, max_pages).to(torch.int32).to(dev)
    k_scale = torch.tensor([[0.3, 3.0], [0.02, 0.7]], device=dev)
    v_scale = torch.tensor([[1.7e-2, 0.3], [3.0, 1.0]], device=dev)
    n = ks._n_values((B, H), dev, 9)
    cos, sin = ks._tables(capacity, D, dev, torch.float32)
    lens = [0, 0]
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    want_k, want_v = ku.cpu().clone(), vu.cpu().clone()
    steps = [(70, [70, 33]), (40, [40, 40]), (1, None), (1, None), (1, None)]
    routes = []
    for t, (Sq, qlens) in enumerate(steps):
        ql = qlens or [Sq] * B
        routes.append(_route(H, Hkv, Sq, qlens))
        q = ks._rand((B, H, Sq, D), dtype, dev, 200 + 3 * t)
        k_new, v_new = ks._rand((B, Hkv, Sq, D), dtype, dev, 201 + 3 * t, std=1.0), ks._rand((B, Hkv, Sq, D), dtype, dev, 202 + 3 * t, std=1.0)
        qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
        out, lse = pkg.flash_attention_n_kvcache_fp8_rope(q, ku.view(k8.F8), vu.view(k8.F8), lens_t, k_scale, v_scale, cos, sin, block_table=table,
                                                          k_new=k_new, v_new=v_new, query_seqlens=qs, softmax_n_param=n, return_lse=True, window=W)
        pos = torch.tensor(lens).view(B, 1) + torch.arange(Sq).view(1, Sq)
        codes_k = k8.quantise(ks._rotate(k_new, pos, cos, sin, False), k_scale.cpu()[:, :, None, None])
        codes_v = k8.quantise(v_new, v_scale.cpu()[:, :, None, None])
        for b in range(B):
            for i in range(ql[b]):
                p = lens[b] + i
                want_k[int(table[b, p // page]), p % page] = codes_k[b, :, i]
                want_v[int(table[b, p // page]), p % page] = codes_v[b, :, i]
        total = [lens[b] + ql[b] for b in range(B)]
        kg = k8.up(ks._gather(ku, table, total, page)) * k_scale[:, :, None, None]
        vg = k8.up(ks._gather(vu, table, total, page)) * v_scale[:, :, None, None]
        o_ref, lse_ref = ks.reference_rows(ks._rotate(q, pos, cos, sin, False), kg, vg, total, ql, n, W)
        ks._check(out, o_ref, dtype, f"step {t} out")
        ks._check_lse(lse, lse_ref, f"step {t} lse")
        lens = total
        lens_t.copy_(torch.tensor(lens, dtype=torch.int32))
    assert routes == ["prefill", "prefill", "decode", "decode", "decode"] and lens == [113, 76] and max(lens) > W
    assert torch.equal(ku.cpu(), want_k) and torch.equal(vu.cpu(), want_v)
