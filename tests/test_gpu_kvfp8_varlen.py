"""flash_attention_n_kvcache_fp8_varlen, _fp8_varlen_window and _fp8_varlen_rope on the GPU: token-packed queries - one [T, H, D] buffer,
cu_seqlens_q in device memory - over a paged cache of e4m3fn codes with one scale per (sequence, K/V head).

1. Exactness: under power-of-two scales (kv_fp8.POW2_SCALES, per (b, hkv) and as Python floats) out and lse are the bits of
   flash_attention_n_kvcache_varlen on `k_cache.to(dtype)` (kv_fp8.assert_bitwise states where a product with a power of two is exact), and
   the bits of the padded flash_attention_n_kvcache_fp8(query_seqlens=) where the two plans have one split count - the gates otherwise.
2. Values: scales that are no powers of two, as an fp32 device tensor, against kv_support.reference_rows on the dequantised cache under the
   cache tests' own gates (REF_ATOL / REL_TRUE on out, the lse gate; kv_support._check / _check_lse, imported).
3. Append: the bytes written are kv_fp8.quantise(k_new, scale) with kv_fp8.append_witnesses among the tokens; every other byte of both
   pools - other sequences' rows, rows at or beyond the capacity, what the tokens at or beyond cu[B] would have written - keeps its value.
4. Window: against the reference, then the same bits with the rows below first_b and the table entries of pages wholly below it poisoned.
5. Rope: byte for byte the route "kv_support._rotate in torch, then flash_attention_n_kvcache_fp8_varlen[_window]" on a clone of the pools.
6. The three witnesses of tests/kv_witness.py through a runner for the new call.
7. One captured graph replayed after cu_seqlens_q, cache_seqlens and the scales changed in place.

Token rows at or beyond cu[B] hold NaN on the way in and are not looked at on the way out; stale cache rows and pages hold the NaN code.
Shapes: heads (8, 2) - PB = 32 - and (4, 4) - PB = 128 -, qlens = [1, 0, PB, PB + 1, 2 PB + 3, 1], lens = [300, 5, 0, page + 1, 2 page, 64]:
a decode token, an empty sequence, a block, a block edge, several blocks; a cache that ends inside a tile, at a page edge, an empty one.
SPLIT is the shape whose plan has several splits (asserted from the plan), so that fasn_kvvarlen_fp8_combine_kernel runs."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_args as ka      # noqa: E402
import kv_fp8 as k8       # noqa: E402
import kv_support as ks   # noqa: E402
import kv_witness as kw   # noqa: E402

pytestmark = pytest.mark.gpu

NAN = ks.NAN
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
HEADS = [(8, 2), (4, 4)]
GENERAL = (0.3, 3.0, 1.7e-3)
VQ = lambda PB: [1, 0, PB, PB + 1, 2 * PB + 3, 1]   # noqa: E731
VL = lambda page: [300, 5, 0, page + 1, 2 * page, 64]   # noqa: E731
# few items behind a long cache: items_max = min(3 * 3, 51 // 16 + 3) = 6 blocks, 64 tiles of capacity -> several splits
SPLIT = dict(H=8, Hkv=1, D=64, page=256, max_pages=16, qlens=[1, 40, 3], lens=[4000, 2100, 20])


def _dt(dtype):
    return 1 if dtype == torch.bfloat16 else 0


def _pad(t, qlens):
    """[T, heads, D] -> [B, heads, Sq, D], Sq = the longest sequence (at least 1), padding rows zero"""
    Sq = max(max(qlens), 1)
    out = torch.zeros(len(qlens), t.shape[1], Sq, t.shape[2], dtype=t.dtype, device=t.device)
    t0 = 0
    for b, ql in enumerate(qlens):
        out[b, :, :ql] = t[t0:t0 + ql].transpose(0, 1)
        t0 += ql
    return out


def _unpad(o, lse, qlens):
    """[B, H, Sq, D], [B, H, Sq] -> [sum qlens, H, D], [H, sum qlens]"""
    return (torch.cat([o[b, :, :ql].transpose(0, 1) for b, ql in enumerate(qlens)], 0), torch.cat([lse[b, :, :ql] for b, ql in enumerate(qlens)], 1))


def _reference(q, qlens, kg, vg, lens, n, rule):
    """kv_support.reference_rows per sequence on its own tokens: (o [sum qlens, H, D], lse [H, sum qlens])"""
    return _unpad(*ks.reference_rows(_pad(q[:sum(qlens)], qlens), kg, vg, lens, qlens, n, rule), qlens)


def _seq_of(qlens, dev):
    """the sequence of every used token"""
    return torch.cat([torch.full((ql,), b, dtype=torch.long) for b, ql in enumerate(qlens)]).to(dev)


def _plans(pkg, B, H, Hkv, Sq, D, T, page, max_pages, dtype, W=None):
    """(the packed FP8 plan, the 16-bit packed plan of the same shape, the padded FP8 prefill plan): the first two must agree on grids and
    launch count - one split rule -, the first names the FP8 kernels and carries their LDS"""
    shape = dict(B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages, dtype=_dt(dtype))
    win = None if W is None else ka._win(pkg, window=min(W, 2 ** 31 - 1))
    va, pa, f8 = ka._args_varlen(pkg, T=T, **shape), ka._args_prefill(pkg, **shape), k8._fp8(pkg)
    packed = pkg._lib.kvfp8_varlen_plan(va, f8, win)
    base = pkg._lib.kvvarlen_plan(va) if W is None else pkg._lib.kvvarlen_window_plan(va, win)
    padded = pkg._lib.kvfp8_plan(pa, f8) if W is None else pkg._lib.kvfp8_window_plan(pa, f8, win)
    assert [k[1:3] for k in packed] == [k[1:3] for k in base], (packed, base)
    names = [k[0].split("<")[0] for k in packed]
    fwd = "fasn_kvvarlen_fwd_fp8_kernel" if W is None else "fasn_kvvarlen_fwd_window_fp8_kernel"
    PB = 128 // (H // Hkv)
    ns = packed[1][1] // (ka.items_max(B, Sq, T, PB) * Hkv)
    assert names == ["fasn_kvvarlen_schedule_kernel", fwd] + (["fasn_kvvarlen_fp8_combine_kernel"] if ns > 1 else []), names
    assert packed[1][3] == 2 * (3 if D == 64 else 2) * 64 * D + 4 * 64 * D   # kv_fp8_smem(D)
    return ns, padded[0][1] // (B * Hkv * -(-Sq // PB))


class _Step:
    """One packed step over a paged cache of codes: T = used + tail tokens (the tail NaN), lengths `lens`, NaN codes in every stale row"""

    def __init__(self, dev, H, Hkv, D, dtype, page, qlens, lens, seed, max_pages=None, tail=7):
        self.B, self.used = len(qlens), sum(qlens)
        self.H, self.Hkv, self.D, self.dtype, self.page, self.qlens, self.lens = H, Hkv, D, dtype, page, list(qlens), list(lens)
        self.max_pages = max_pages or max(1, max((ln + page - 1) // page for ln in lens)) + 1
        self.T, self.Sq = self.used + tail, max(max(qlens), 1)
        self.q = ks._rand((self.T, H, D), dtype, dev, seed)
        self.q[self.used:] = NAN
        cap = page * self.max_pages
        self.kd, self.vd = k8.rand_codes((self.B, Hkv, cap, D), seed + 1, dev), k8.rand_codes((self.B, Hkv, cap, D), seed + 2, dev)
        self.pc = k8.PagedCodes(self.kd, self.vd, lens, page, self.max_pages, seed)
        self.cu = ks._cu(qlens, dev)
        self.seq = _seq_of(qlens, dev)

    def dequantised(self, k_scale, v_scale):
        return (k8.up(k8.visible(self.kd, self.lens)) * k_scale[:, :, None, None], k8.up(k8.visible(self.vd, self.lens)) * v_scale[:, :, None, None])

    def call(self, pkg, k_scale, v_scale, n, W=None, causal=True):
        kw_ = dict(block_table=self.pc.table, softmax_n_param=n, return_lse=True)
        if W is None:
            return pkg.flash_attention_n_kvcache_fp8_varlen(self.q, self.pc.k, self.pc.v, self.pc.lens, k_scale, v_scale, self.cu, self.Sq,
                                                            is_causal=causal, **kw_)
        return pkg.flash_attention_n_kvcache_fp8_varlen_window(self.q, self.pc.k, self.pc.v, self.pc.lens, k_scale, v_scale, self.cu, self.Sq, W, **kw_)

    def plans(self, pkg, W=None):
        return _plans(pkg, self.B, self.H, self.Hkv, self.Sq, self.D, self.T, self.page, self.max_pages, self.dtype, W)


def _twin(pkg, st, k_scale, v_scale, n, W, got, what):
    """kv_fp8.sixteen_bit_twin for packed rows: the 16-bit packed call on the exactly upcast cache, once per distinct k_scale with
    scale * k_scale, every (token, head) taking its row from the run of its sequence's scale; then kv_fp8.assert_bitwise with a token
    standing for a batch element of one position"""
    out, lse = got
    G, used = st.H // st.Hkv, st.used
    k16, v16 = st.pc.k.to(st.dtype), st.pc.v.to(st.dtype)   # exact; the stale rows become NaN, which the 16-bit call never reads either
    ks_tok = k_scale.expand(st.B, st.Hkv).repeat_interleave(G, dim=1)[st.seq]   # [used, H]
    vs_tok = v_scale.expand(st.B, st.Hkv).repeat_interleave(G, dim=1)[st.seq]
    out16 = torch.zeros(used, st.H, st.D, dtype=torch.float32, device=out.device)
    lse16 = torch.zeros(used, st.H, dtype=torch.float32, device=out.device)
    for u in sorted(set(k_scale.flatten().tolist())):
        kw_ = dict(block_table=st.pc.table, softmax_n_param=n, scale=st.D ** -0.5 * u, return_lse=True)
        if W is None:
            o_u, l_u = pkg.flash_attention_n_kvcache_varlen(st.q, k16, v16, st.pc.lens, st.cu, st.Sq, **kw_)
        else:
            o_u, l_u = pkg.flash_attention_n_kvcache_varlen_window(st.q, k16, v16, st.pc.lens, st.cu, st.Sq, W, **kw_)
        pick = ks_tok == u
        out16 = torch.where(pick[:, :, None], o_u[:used].float(), out16)
        lse16 = torch.where(pick, l_u[:, :used].t(), lse16)
    k8.assert_bitwise(out[:used].unsqueeze(2), out16.unsqueeze(2), vs_tok, lse[:, :used].t().unsqueeze(2), lse16.unsqueeze(2), st.dtype, what)


def _padded(pkg, st, k_scale, v_scale, n, W, got, what):
    """the padded FP8 prefill on the same cache: the same kernel text on the same row blocks and tiles - the same bits where the plans have
    one split count, the gates otherwise"""
    out, lse = got
    qs = torch.tensor(st.qlens, dtype=torch.int32, device=out.device)
    kw_ = dict(block_table=st.pc.table, query_seqlens=qs, softmax_n_param=n, return_lse=True)
    qp = _pad(st.q[:st.used], st.qlens)
    if W is None:
        wo, wl = pkg.flash_attention_n_kvcache_fp8(qp, st.pc.k, st.pc.v, st.pc.lens, k_scale, v_scale, **kw_)
    else:
        wo, wl = pkg.flash_attention_n_kvcache_fp8_window(qp, st.pc.k, st.pc.v, st.pc.lens, k_scale, v_scale, W, **kw_)
    wo, wl = _unpad(wo, wl, st.qlens)
    ns_packed, ns_padded = st.plans(pkg, W)
    if ns_packed == ns_padded:
        assert torch.equal(ks._bits(out[:st.used]), ks._bits(wo)) and torch.equal(lse[:, :st.used], wl), f"{what}: not the bits of the padded call"
    else:
        ks._check(out[:st.used], wo, st.dtype, f"{what} out vs the padded call ({ns_packed} / {ns_padded} splits)")
        ks._check_lse(lse[:, :st.used], wl, f"{what} lse vs the padded call")
    return ns_packed


# ---------------------------------------------------------------- 1. exactness under power-of-two scales
@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", HEADS)
def test_power_of_two_scales_give_the_bits_of_the_16_bit_packed_call(pkg, dev, heads, D, dtype, page):
    H, Hkv = heads
    PB = 128 // (H // Hkv)
    st = _Step(dev, H, Hkv, D, DTYPES[dtype], page, VQ(PB), VL(page), 100 + D + page + H)
    n = ks._n_values((st.B, H), dev, 7)
    k_scale, v_scale = k8.scales_bh(k8.POW2_SCALES, st.B, Hkv, dev, 11), k8.scales_bh(k8.POW2_SCALES, st.B, Hkv, dev, 12)
    what = f"H={H}/{Hkv} D={D} {dtype} page={page}"
    got = st.call(pkg, k_scale, v_scale, n)
    assert got[0].shape == st.q.shape and got[1].shape == (H, st.T)
    assert torch.isfinite(got[0][:st.used]).all() and (got[0][:st.used] != 0).any()
    _twin(pkg, st, k_scale, v_scale, n, None, got, what)
    _padded(pkg, st, k_scale, v_scale, n, None, got, what)


@pytest.mark.parametrize("s", k8.POW2_SCALES)
def test_a_python_float_scale_is_the_one_element_tensor(pkg, dev, s):
    st = _Step(dev, 8, 2, 64, torch.bfloat16, 64, VQ(32), VL(64), 140)
    got = st.call(pkg, s, s, 1.0, causal=False)
    ten = torch.full((1, 1), s, device=dev)
    want = st.call(pkg, ten, ten, 1.0, causal=False)
    assert torch.equal(ks._bits(got[0][:st.used]), ks._bits(want[0][:st.used])) and torch.equal(got[1][:, :st.used], want[1][:, :st.used])
    _twin(pkg, st, ten, ten, 1.0, None, st.call(pkg, s, s, 1.0), f"float scale {s}")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("W", [None, 3000])
def test_several_splits_run_the_fp8_packed_combine(pkg, dev, W, dtype):
    c = SPLIT
    st = _Step(dev, c["H"], c["Hkv"], c["D"], DTYPES[dtype], c["page"], c["qlens"], c["lens"], 300, max_pages=c["max_pages"])
    ns, _ = st.plans(pkg, W)
    assert ns >= 2, f"the plan has {ns} split(s): the shape was chosen to have several"
    n = ks._n_values((c["H"],), dev, 301)
    k_scale, v_scale = k8.scales_bh(k8.POW2_SCALES, st.B, c["Hkv"], dev, 302), k8.scales_bh(k8.POW2_SCALES, st.B, c["Hkv"], dev, 303)
    got = st.call(pkg, k_scale, v_scale, n, W)
    _twin(pkg, st, k_scale, v_scale, n, W, got, f"several splits W={W} {dtype}")
    _padded(pkg, st, k_scale, v_scale, n, W, got, f"several splits W={W} {dtype}")
    # ... and scales that are no powers of two through the same combine
    k_scale, v_scale = k8.scales_bh(GENERAL, st.B, c["Hkv"], dev, 304), k8.scales_bh(GENERAL, st.B, c["Hkv"], dev, 305)
    out, lse = st.call(pkg, k_scale, v_scale, n, W)
    kg, vg = st.dequantised(k_scale, v_scale)
    o_ref, l_ref = _reference(st.q, st.qlens, kg, vg, st.lens, n, True if W is None else W)
    ks._check(out[:st.used], o_ref, st.dtype, f"several splits W={W} {dtype} general scales out")
    ks._check_lse(lse[:, :st.used], l_ref, f"several splits W={W} {dtype} general scales lse")


# ---------------------------------------------------------------- 2. values under general scales
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", HEADS)
def test_general_scales_against_the_reference(pkg, dev, heads, D, dtype, causal):
    H, Hkv = heads
    PB, page = 128 // (H // Hkv), 64 if D == 64 else 128
    st = _Step(dev, H, Hkv, D, DTYPES[dtype], page, VQ(PB), VL(page), 200 + D + H)
    n = ks._n_values((st.B, H), dev, 8)
    k_scale, v_scale = k8.scales_bh(GENERAL, st.B, Hkv, dev, 21), k8.scales_bh(GENERAL, st.B, Hkv, dev, 22)
    assert k_scale.dtype == torch.float32 and k_scale.is_cuda
    out, lse = st.call(pkg, k_scale, v_scale, n, causal=causal)
    kg, vg = st.dequantised(k_scale, v_scale)
    o_ref, l_ref = _reference(st.q, st.qlens, kg, vg, st.lens, n, causal)
    what = f"general scales H={H}/{Hkv} D={D} {dtype} causal={causal}"
    ks._check(out[:st.used], o_ref, st.dtype, f"{what} out")
    ks._check_lse(lse[:, :st.used], l_ref, f"{what} lse")
    _padded(pkg, st, k_scale, v_scale, n, None, (out, lse), what) if causal else None


# ---------------------------------------------------------------- 3. the quantising append
class _Pools:
    """pools of random bytes behind a shuffled table that names every page of every sequence, one spare page no table names"""

    def __init__(self, dev, B, Hkv, D, page, max_pages, seed):
        gen = torch.Generator().manual_seed(seed)
        n_pages = B * max_pages + 1
        self.table = torch.randperm(n_pages, generator=gen)[:B * max_pages].view(B, max_pages).to(torch.int32).to(dev)
        self.ku = torch.randint(0, 256, (n_pages, page, Hkv, D), generator=gen, dtype=torch.int32).to(torch.uint8).to(dev)
        self.vu = torch.randint(0, 256, (n_pages, page, Hkv, D), generator=gen, dtype=torch.int32).to(torch.uint8).to(dev)
        self.page, self.cap = page, page * max_pages


def _expect_append(pools, qlens, lens, codes_k, codes_v):
    """the pools after the append, on the CPU: token cu[b] + i -> row lens[b] + i through the table, dropped at or beyond the capacity"""
    want_k, want_v = pools.ku.cpu().clone(), pools.vu.cpu().clone()
    table = pools.table.cpu()
    t, written, dropped = 0, 0, 0
    for b, ql in enumerate(qlens):
        for i in range(ql):
            p = lens[b] + i
            if p >= pools.cap:
                dropped += 1
            else:
                pid = int(table[b, p // pools.page])
                want_k[pid, p % pools.page], want_v[pid, p % pools.page] = codes_k[t + i], codes_v[t + i]
                written += 1
        t += ql
    return want_k, want_v, written, dropped


def _assert_bytes(got, want, what):
    got = got.cpu()
    nan = k8.is_nan_code(want)
    assert k8.is_nan_code(got[nan]).all(), f"{what}: a NaN code of the reference is no NaN code in the cache"
    diff = (got != want) & ~nan
    assert not diff.any(), f"{what}: {int(diff.sum())} bytes differ, first at {diff.nonzero()[0].tolist()}: got {int(got[diff][0]):#x}, want {int(want[diff][0]):#x}"


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", HEADS)
def test_append_bytes_equal_the_quantised_rows(pkg, dev, heads, D, dtype):
    """sequence 4 has 2 PB rows left for 2 PB + 3 tokens: three rows are dropped. The first token of sequence 3 carries the witnesses."""
    H, Hkv = heads
    PB, page, max_pages, dt = 128 // (H // Hkv), 64, 6, DTYPES[dtype]
    qlens = VQ(PB)
    cap = page * max_pages
    lens = [300, 5, 0, page + 1, cap - 2 * PB, 64]
    B, used = len(qlens), sum(qlens)
    T = used + 7
    k_scale, v_scale = k8.scales_bh(GENERAL + (1.0, 2.0 ** -3, 16.0), B, Hkv, dev, 31), k8.scales_bh(GENERAL + (0.7, 1.0), B, Hkv, dev, 32)
    seq = _seq_of(qlens, dev)
    k_new = (ks._rand((T, Hkv, D), torch.float32, dev, 33, std=1.0) * 40.0)
    v_new = (ks._rand((T, Hkv, D), torch.float32, dev, 34, std=1.0) * 40.0)
    k_new[:used] *= k_scale[seq][:, :, None]
    v_new[:used] *= v_scale[seq][:, :, None]
    k_new, v_new = k_new.to(dt), v_new.to(dt)
    w = k8.append_witnesses(torch.float32)
    t_w = 1 + PB   # the first token of sequence 3
    assert Hkv * D >= w.numel() and seq[t_w] == 3
    flat = torch.full((Hkv * D,), 1.5)
    flat[:w.numel()] = w
    k_new[t_w] = (flat.view(Hkv, D) * k_scale[3].cpu().view(Hkv, 1)).to(dt).to(dev)
    v_new[t_w] = (flat.view(Hkv, D) * v_scale[3].cpu().view(Hkv, 1)).to(dt).to(dev)
    k_new[used:], v_new[used:] = NAN, NAN
    assert torch.isnan(k_new[t_w]).any() and torch.isinf(k_new[t_w]).any()
    codes_k = k8.quantise(k_new[:used], k_scale[seq].cpu()[:, :, None])
    codes_v = k8.quantise(v_new[:used], v_scale[seq].cpu()[:, :, None])
    pools = _Pools(dev, B, Hkv, D, page, max_pages, 35)
    want_k, want_v, written, dropped = _expect_append(pools, qlens, lens, codes_k, codes_v)
    assert dropped == 3 and written == used - 3
    q = ks._rand((T, H, D), dt, dev, 36)
    q[used:] = NAN
    lens_t, cu = torch.tensor(lens, dtype=torch.int32, device=dev), ks._cu(qlens, dev)
    kn0, vn0 = k_new.clone(), v_new.clone()
    out = pkg.flash_attention_n_kvcache_fp8_varlen(q, pools.ku.view(k8.F8), pools.vu.view(k8.F8), lens_t, k_scale, v_scale, cu, max(qlens),
                                                   block_table=pools.table, k_new=k_new, v_new=v_new)
    assert out.shape == q.shape and lens_t.tolist() == lens
    assert torch.equal(ks._bits(k_new), ks._bits(kn0)) and torch.equal(ks._bits(v_new), ks._bits(vn0)), "k_new / v_new was modified"
    _assert_bytes(pools.ku, want_k, f"append k H={H}/{Hkv} D={D} {dtype}")
    _assert_bytes(pools.vu, want_v, f"append v H={H}/{Hkv} D={D} {dtype}")
    fresh = torch.cat([codes_k[t_w].flatten(), codes_v[t_w].flatten()])
    assert (fresh == 0x7E).any() and (fresh == 0xFE).any() and (fresh == 0x00).any() and (fresh == 0x80).any() and ((fresh > 0) & (fresh < 8)).any()


# ---------------------------------------------------------------- 4. the window: reference, then the pages below it gone
def _poison_below(pc, lens, qlens, W):
    """kv_support._poison on a cache of codes: it writes NaN, which the float8 views of the pools take as the NaN code"""
    return ks._poison(pc.k, pc.v, pc.table, pc.page, pc.poison, lens, qlens, W)


@pytest.mark.parametrize("W", [1, 70, "capacity + 5"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", HEADS)
def test_window_against_the_reference_and_with_the_pages_below_it_gone(pkg, dev, heads, D, dtype, W):
    H, Hkv = heads
    PB, page = 128 // (H // Hkv), 64 if D == 64 else 128
    st = _Step(dev, H, Hkv, D, DTYPES[dtype], page, VQ(PB), VL(page), 400 + D + H)
    W = page * st.max_pages + 5 if isinstance(W, str) else W
    n = ks._n_values((st.B, H), dev, 9)
    k_scale, v_scale = k8.scales_bh(GENERAL, st.B, Hkv, dev, 41), k8.scales_bh(GENERAL, st.B, Hkv, dev, 42)
    what = f"window W={W} H={H}/{Hkv} D={D} {dtype}"
    out, lse = st.call(pkg, k_scale, v_scale, n, W)
    kg, vg = st.dequantised(k_scale, v_scale)
    o_ref, l_ref = _reference(st.q, st.qlens, kg, vg, st.lens, n, W)
    ks._check(out[:st.used], o_ref, st.dtype, f"{what} out")
    ks._check_lse(lse[:, :st.used], l_ref, f"{what} lse")
    _padded(pkg, st, k_scale, v_scale, n, W, (out, lse), what)
    if W > page * st.max_pages:   # a window beyond the capacity: the causal call
        o0, l0 = st.call(pkg, k_scale, v_scale, n)
        assert torch.equal(ks._bits(out[:st.used]), ks._bits(o0[:st.used])) and torch.equal(lse[:, :st.used], l0[:, :st.used]), f"{what}: not the causal call"
    rows = _poison_below(st.pc, st.lens, st.qlens, W)
    assert (rows > 0) == (W <= 70), rows
    o2, l2 = st.call(pkg, k_scale, v_scale, n, W)
    assert torch.isfinite(o2[:st.used]).all() and not torch.isnan(l2[:, :st.used]).any(), f"{what}: the poison below the window reached the result"
    assert torch.equal(ks._bits(out[:st.used]), ks._bits(o2[:st.used])) and torch.equal(lse[:, :st.used], l2[:, :st.used]), f"{what}: the rows below the window changed the result"


# ---------------------------------------------------------------- 5. rope: byte for byte the torch-rotated route
def _rotate_packed(x, pos, cos, sin, interleaved):
    """kv_support._rotate on [n, heads, D] rows at positions pos [n]"""
    return ks._rotate(x.transpose(0, 1).unsqueeze(0), pos[None], cos, sin, interleaved)[0].transpose(0, 1).contiguous()


def _run_rope(pkg, dev, H, Hkv, D, dtype, qlens, lens, seed, rd, interleaved, fp32_tables, window=None, append=True, what=""):
    page, max_pages = 64, 6
    B, used = len(qlens), sum(qlens)
    T, Sq = used + 7, max(max(qlens), 1)
    pools = _Pools(dev, B, Hkv, D, page, max_pages, seed)
    # the cache as it stands: finite random codes in the rows below the lengths, NaN codes in the stale rows (the append overwrites some)
    table = pools.table.cpu()
    codes = k8.rand_codes((2, B, pools.cap, Hkv, D), seed + 1, dev)
    pools.ku[:], pools.vu[:] = k8.NAN_CODE, k8.NAN_CODE
    for b, ln in enumerate(lens):
        for s in range(-(-ln // page)):
            cnt = min(page, ln - s * page)
            pools.ku[int(table[b, s]), :cnt], pools.vu[int(table[b, s]), :cnt] = codes[0, b, s * page:s * page + cnt], codes[1, b, s * page:s * page + cnt]
    q = ks._rand((T, H, D), dtype, dev, seed + 2)
    kn, vn = ks._rand((T, Hkv, D), dtype, dev, seed + 3, std=1.0), ks._rand((T, Hkv, D), dtype, dev, seed + 4, std=1.0)
    for t in (q, kn, vn):
        t[used:] = NAN
    cos, sin = ks._tables(pools.cap, rd, dev, torch.float32 if fp32_tables else dtype)
    total = [min(pools.cap, ln + ql) if append else ln for ln, ql in zip(lens, qlens)]
    kpos = torch.cat([lens[b] + torch.arange(ql) for b, ql in enumerate(qlens)])
    qpos = torch.cat([torch.arange(ql) + total[b] - ql for b, ql in enumerate(qlens)])
    q_rot, k_rot = q.clone(), kn.clone()
    q_rot[:used], k_rot[:used] = _rotate_packed(q[:used], qpos, cos, sin, interleaved), _rotate_packed(kn[:used], kpos, cos, sin, interleaved)
    k_scale, v_scale = k8.scales_bh(GENERAL, B, Hkv, dev, seed + 5), k8.scales_bh(GENERAL, B, Hkv, dev, seed + 6)
    n = ks._n_values((B, H), dev, seed + 7)
    lens_t, cu = torch.tensor(lens, dtype=torch.int32, device=dev), ks._cu(qlens, dev)
    kw_ = dict(block_table=pools.table, softmax_n_param=n, return_lse=True)
    kR, vR = pools.ku.clone(), pools.vu.clone()
    q0, kn0 = q.clone(), kn.clone()
    out, lse = pkg.flash_attention_n_kvcache_fp8_varlen_rope(q, kR.view(k8.F8), vR.view(k8.F8), lens_t, k_scale, v_scale, cu, Sq, cos, sin, window=window,
                                                             rotary_interleaved=interleaved, **(dict(k_new=kn, v_new=vn) if append else {}), **kw_)
    assert out.shape == q.shape and lse.shape == (H, T) and lens_t.tolist() == lens
    assert torch.equal(ks._bits(q), ks._bits(q0)) and torch.equal(ks._bits(kn), ks._bits(kn0)), f"{what}: query / k_new was modified"
    kT, vT = pools.ku.clone(), pools.vu.clone()
    new_t = dict(k_new=k_rot, v_new=vn) if append else {}
    if window is None:
        o_t, l_t = pkg.flash_attention_n_kvcache_fp8_varlen(q_rot, kT.view(k8.F8), vT.view(k8.F8), lens_t, k_scale, v_scale, cu, Sq, **new_t, **kw_)
    else:
        o_t, l_t = pkg.flash_attention_n_kvcache_fp8_varlen_window(q_rot, kT.view(k8.F8), vT.view(k8.F8), lens_t, k_scale, v_scale, cu, Sq, window, **new_t, **kw_)
    dk, dv = (kR != kT).sum().item(), (vR != vT).sum().item()
    do = (ks._bits(out[:used]) != ks._bits(o_t[:used])).sum().item()
    dl = (lse[:, :used].view(torch.int32) != l_t[:, :used].view(torch.int32)).sum().item()
    print(f"{what}: elements that differ between the routes: k pool {dk}, v pool {dv}, out {do}, lse {dl}")
    assert dk == 0 and dv == 0, f"{what}: the pools differ in {dk} / {dv} bytes"
    assert do == 0 and dl == 0, f"{what}: out / lse differ from the torch-rotated route in {do} / {dl} elements"
    assert torch.isfinite(out[:used]).all() and (out[:used] != 0).any() and not torch.isnan(lse[:, :used]).any()
    assert torch.equal(kR, pools.ku) != append and torch.equal(vR, pools.vu) != append, f"{what}: the append wrote, a queries-only call does not"


@pytest.mark.parametrize("window", [None, 70])
@pytest.mark.parametrize("layout", ["half", "interleaved"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_rope_equals_eager_rotation_then_the_packed_fp8_call(pkg, dev, D, dtype, layout, window):
    """heads (8, 2); rotary_dim = D with fp32 tables (half-split) and D / 2 with 16-bit tables (interleaved); appends across a tile and a
    page edge, an empty sequence, an empty cache"""
    inter = layout == "interleaved"
    _run_rope(pkg, dev, 8, 2, D, DTYPES[dtype], VQ(32), [130, 5, 0, 61, 100, 64], 500 + D, D // 2 if inter else D, inter, not inter, window=window,
              what=f"rope D={D} {dtype} {layout} window={window}")


@pytest.mark.parametrize("heads", HEADS)
def test_rope_without_new_rows_rotates_the_queries_only(pkg, dev, heads):
    H, Hkv = heads
    _run_rope(pkg, dev, H, Hkv, 64, torch.bfloat16, [1, 0, 42, 43, 5], [130, 5, 7, 100, 1], 540 + H, 32, False, True, append=False,
              what=f"rope queries only H={H}/{Hkv}")


# ---------------------------------------------------------------- 6. the witnesses of kv_witness.py
Case = kw.Case
SHAPES = {
    "H8/2": Case("fp8_varlen", 8, 2, 64, 67, VL(64), qlens=VQ(32)),
    "H4/4 D128 append": Case("fp8_varlen", 4, 4, 128, 259, VL(64), qlens=VQ(128), append=True),
    "H8/2 W70": Case("fp8_varlen", 8, 2, 64, 67, VL(64), qlens=VQ(32), window=70),
    "split": Case("fp8_varlen", SPLIT["H"], SPLIT["Hkv"], SPLIT["D"], 40, SPLIT["lens"], page=SPLIT["page"], max_pages=SPLIT["max_pages"],
                  qlens=SPLIT["qlens"], long=True),
}


def _quantise_inputs(case, inp, dtype, dev, seed, unit_k=False, v_scales=k8.POW2_SCALES):
    """the witness's K and V as codes under power-of-two scales per (b, hkv) - `unit_k`: k_scale = 1 - and, in `inp`, the values of those
    codes (exact in `dtype`): what the kernels see is what the fp64 reference sees. Returns (inp, K codes, V codes, k_scale, v_scale)."""
    k_scale = torch.ones(case.B, case.Hkv, device=dev) if unit_k else k8.scales_bh(k8.POW2_SCALES, case.B, case.Hkv, dev, seed)
    v_scale = k8.scales_bh(v_scales, case.B, case.Hkv, dev, seed + 1)
    kc = k8.quantise(inp["kd"], k_scale.cpu()[:, :, None, None]).to(dev)
    vc = k8.quantise(inp["vd"], v_scale.cpu()[:, :, None, None]).to(dev)
    inp = dict(inp)
    inp["kd"] = (k8.up(kc) * k_scale[:, :, None, None]).to(dtype)
    inp["vd"] = (k8.up(vc) * v_scale[:, :, None, None]).to(dtype)
    assert torch.equal(inp["kd"].float(), k8.up(kc) * k_scale[:, :, None, None]) and torch.equal(inp["vd"].float(), k8.up(vc) * v_scale[:, :, None, None])
    return inp, kc, vc, k_scale, v_scale


def _run_witness(pkg, case, inp, kc, vc, k_scale, v_scale, seed):
    """kv_witness.run_varlen for the new call: a paged cache of codes whose pages reach len_b, the rows old length .. len_b - 1 NaN codes
    until the append writes them (k_new / v_new: the values of the codes, which quantise back to them), the rows and table entries wholly
    below a window poisoned. Per sequence (out [H, qlen_b, D], lse [H, qlen_b])."""
    dev = kc.device
    pc = k8.PagedCodes(kc, vc, case.total, case.page, case.max_pages, seed)
    if case.append:
        tbl = pc.table.cpu()
        for b, (ln, tot) in enumerate(zip(case.lens, case.total)):
            for p in range(ln, tot):
                pc.ku[int(tbl[b, p // case.page]), p % case.page] = k8.NAN_CODE
                pc.vu[int(tbl[b, p // case.page]), p % case.page] = k8.NAN_CODE
    if case.window is not None:
        _poison_below(pc, case.total, case.qlens, case.window)
    kn, vn = kw._new_rows(case, inp)
    used = sum(case.qlens)

    def pack(t):   # [B, heads, Sq, D] -> [T, heads, D]
        rows = [t[b, :, :ql].transpose(0, 1) for b, ql in enumerate(case.qlens)]
        return torch.cat(rows + [torch.full((case.tail, t.shape[1], t.shape[3]), NAN, dtype=t.dtype, device=dev)], 0).contiguous()

    lens_t = torch.tensor(case.lens, dtype=torch.int32, device=dev)
    kw_ = dict(block_table=pc.table, k_new=None if kn is None else pack(kn), v_new=None if vn is None else pack(vn), softmax_n_param=inp["n"],
               scale=inp["scale"], return_lse=True)
    args = (pack(inp["q"]), pc.k, pc.v, lens_t, k_scale, v_scale, ks._cu(case.qlens, dev), max(max(case.qlens), 1))
    if case.window is None:
        out, lse = pkg.flash_attention_n_kvcache_fp8_varlen(*args, is_causal=case.causal, **kw_)
    else:
        out, lse = pkg.flash_attention_n_kvcache_fp8_varlen_window(*args, case.window, **kw_)
    assert out.shape == (used + case.tail, case.H, case.D) and lse.shape == (case.H, used + case.tail)
    res, t0 = [], 0
    for ql in case.qlens:
        res.append((out[t0:t0 + ql].transpose(0, 1), lse[:, t0:t0 + ql]))
        t0 += ql
    return res


def _seed(name):
    return 2000 + sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 9000


def _dtypes(case):
    return ["fp16"] if case.long else ["fp16", "bf16"]


@pytest.mark.parametrize("name,dtype", [(s, d) for s in SHAPES for d in _dtypes(SHAPES[s])])
def test_witness_a_every_visible_key_exactly_once(pkg, dev, name, dtype):
    case, dt = SHAPES[name], DTYPES[dtype]
    inp, kc, vc, k_scale, v_scale = _quantise_inputs(case, kw.inputs_a(case, dt, dev, _seed(name)), dt, dev, _seed(name) + 5)
    refs = kw.reference(case, inp)
    cmax = kw.condition_a(refs, dt)
    got = _run_witness(pkg, case, inp, kc, vc, k_scale, v_scale, _seed(name))
    ratios = [kw.gate_a(o, lse, r) for (o, lse), r in zip(got, refs)]
    rz, ro = max(r[0] for r in ratios), max(r[1] for r in ratios)
    print(f"A {name} {dtype}: largest class count {cmax:g}; exp(lse) at {rz:.3g} of 1e-5 Z, out Z at {ro:.3g} of 0.25")
    assert rz <= 1, f"exp(lse) is {rz:.3g}x (1e-5 Z_ref) from n + the number of visible keys, per sequence {[r[0] for r in ratios]}"
    assert ro <= 1, f"out Z_ref is {ro:.3g}x 0.25 from the class counts, per sequence {[r[1] for r in ratios]}"


B_CASES = [(s, form, d) for s in SHAPES for form, ds in (("ascending", ("fp16", "bf16")), ("descending", ("bf16",)), ("sink", ("bf16",)))
           for d in (("fp16",) if SHAPES[s].long else ds)]


@pytest.mark.parametrize("name,form,dtype", B_CASES)
def test_witness_b_one_key_decides(pkg, dev, name, form, dtype):
    """the keys of kv_witness.inputs_b - base-16 digits and ones - are e4m3fn numbers: quantised at k_scale = 1 without loss"""
    case, dt = SHAPES[name], DTYPES[dtype]
    raw = kw.inputs_b(case, form, dt, dev, _seed(name))
    # v_scale <= 2: where the sink decides, a key 32 nats down weighs e^-32 |V| / n <= 1.3e-14 * 4 / 0.25 - inside expect_b's 1e-12
    inp, kc, vc, k_scale, v_scale = _quantise_inputs(case, raw, dt, dev, _seed(name) + 5, unit_k=True, v_scales=(1.0, 2.0 ** -3, 2.0))
    assert torch.equal(inp["kd"], raw["kd"])
    vc = (vc & 0x8F) | 0x30   # 0.5 <= |code| < 2: no exact zeros (gate_b bounds them at 1e-30) and, times the smallest v_scale, no fp16 subnormals
    inp["vd"] = (k8.up(vc) * v_scale[:, :, None, None]).to(dt)
    refs = kw.reference(case, inp)
    got = _run_witness(pkg, case, inp, kc, vc, k_scale, v_scale, _seed(name))
    ratios, kinds, lses = [], set(), []
    for b, ((o, lse), r) in enumerate(zip(got, refs)):
        kind, want = kw.expect_b(r, kw.sequence(case, inp, b)[2][:, :case.total[b]], case.H // case.Hkv)
        kinds |= set(kind.unique().tolist())
        ratios.append(kw.gate_b(o, kind, want, dt))
        lses.append((lse.detach().cpu(), r["lse"], kind))
    print(f"B {name} {form} {dtype}: out at {max(ratios):.3g} of its gate; row kinds {sorted(kinds)}")
    assert max(ratios) <= 1, f"out is {max(ratios):.3g}x the gate from the deciding key's V row, per sequence {ratios}"
    for b, (lse, want, kind) in enumerate(lses):
        for k in (0, 1, 2):
            if (kind == k).any():
                ks._check_lse(lse[kind == k], want[kind == k], f"B {name} {form} {dtype} sequence {b} lse (rows of kind {k})")
    assert 1 in kinds and (form != "sink" or 2 in kinds)


@pytest.mark.parametrize("std", [4, 8])
@pytest.mark.parametrize("name,dtype", [(s, d) for s in SHAPES for d in _dtypes(SHAPES[s])])
def test_witness_c_realistic_dynamic_range(pkg, dev, name, dtype, std):
    case, dt = SHAPES[name], DTYPES[dtype]
    inp, kc, vc, k_scale, v_scale = _quantise_inputs(case, kw.inputs_c(case, std, dt, dev, _seed(name) + std), dt, dev, _seed(name) + 5)
    refs = kw.reference(case, inp)
    got = _run_witness(pkg, case, inp, kc, vc, k_scale, v_scale, _seed(name))
    ratios = [kw.gate_c(o, r, dt) for (o, _), r in zip(got, refs)]
    print(f"C {name} std {std} {dtype}: out at {max(ratios):.3g} of 3 u A + 1e-6")
    assert max(ratios) <= 1, f"out is {max(ratios):.3g}x (3 u A + 1e-6) from the fp64 reference, per sequence {ratios}"
    for b, ((_, lse), r) in enumerate(zip(got, refs)):
        ks._check_lse(lse, r["lse"], f"C {name} std {std} {dtype} sequence {b} lse")


# ---------------------------------------------------------------- 7. a captured graph follows the device memory
def test_graph_replay_follows_offsets_lengths_and_scales(pkg, dev):
    """one flash_attention_n_kvcache_fp8_varlen_rope(window=64) step with an append, T = 64, B = 4, max_seqlen_q = 48, captured on one stream;
    replays after cu_seqlens_q, cache_seqlens and both scale tensors changed in place: the bits - and the cache bytes - of an eager call"""
    dtype, H, Hkv, D, page, max_pages, T, B, Sq, W = torch.bfloat16, 8, 2, 64, 64, 8, 64, 4, 48, 64
    cap = page * max_pages
    q, kn, vn = ks._rand((T, H, D), dtype, dev, 600), ks._rand((T, Hkv, D), dtype, dev, 601, std=1.0), ks._rand((T, Hkv, D), dtype, dev, 602, std=1.0)
    kd, vd = k8.rand_codes((B, Hkv, cap, D), 603, dev), k8.rand_codes((B, Hkv, cap, D), 604, dev)
    pc = k8.PagedCodes(kd, vd, [cap] * B, page, max_pages, 605)   # every row finite: the lengths move
    cos, sin = ks._tables(cap, D, dev, torch.float32)
    n = ks._n_values((H,), dev, 606)
    cu = ks._cu([1, 1, 1, 1], dev)
    sl = torch.tensor([62, 100, 5, 300], dtype=torch.int32, device=dev)
    k_scale, v_scale = torch.full((B, Hkv), 0.5, device=dev), torch.full((Hkv,), 0.7, device=dev)
    k_e, v_e = pc.ku.clone(), pc.vu.clone()   # the eager route's pools: they see the same appends

    def call(kc, vc, sl_, cu_, ks_, vs_):
        return pkg.flash_attention_n_kvcache_fp8_varlen_rope(q, kc.view(k8.F8), vc.view(k8.F8), sl_, ks_, vs_, cu_, Sq, cos, sin, block_table=pc.table,
                                                             k_new=kn, v_new=vn, softmax_n_param=n, return_lse=True, window=W)

    g, (go, glse) = ks._capture(lambda: call(pc.ku, pc.vu, sl, cu, k_scale, v_scale))
    with torch.no_grad():   # the warm-up runs appended: the eager pools follow
        k_e.copy_(pc.ku)
        v_e.copy_(pc.vu)
    seen = []
    for step, qlens in enumerate(([1, 1, 1, 1], [48, 1, 10, 5], [0, 16, 30, 18])):
        lens = [62 + 37 * step, 100 + step, 5, 300 - 64 * step]
        used = sum(qlens)
        with torch.no_grad():
            cu.copy_(ks._cu(qlens, dev))
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
            k_scale.copy_(k8.scales_bh(GENERAL, B, Hkv, dev, 610 + step))
            v_scale.copy_(torch.tensor([0.1 + step, 4.0 / (1 + step)]))
        g.replay()
        torch.cuda.synchronize()
        eo, el = call(k_e, v_e, sl.clone(), cu.clone(), k_scale.clone(), v_scale.clone())
        assert torch.equal(ks._bits(go[:used]), ks._bits(eo[:used])) and torch.equal(glse[:, :used], el[:, :used]), f"replay {step}: differs from the eager call"
        assert torch.equal(pc.ku, k_e) and torch.equal(pc.vu, v_e), f"replay {step}: the pools differ from the eager call's"
        assert torch.isfinite(go[:used]).all()
        seen.append(go[:1].clone())
    assert not torch.equal(seen[0], seen[1]), "the replays returned one result: the graph does not follow the device memory"
