"""alibi_slopes on flash_attention_n_kvcache and flash_attention_n_kvcache_prefill, on the GPU: the logit of query position i and key j
is scale * q_i.k_j - slope[b, h] * |p_i - j| with p_i = i + len_b - qlen_b, computed in the kernels from the lengths in device memory.

Reference: kv_support.reference_rows with slopes (fp32 torch, the explicit sink column, -slope * |p_i - j| added to the scaled scores in
fp32 before the masking, per batch element on q[b, :, :qlen_b]); padding positions 0 / -inf.
Second witness: flash_attention_n on the gathered dense K/V with attn_bias = the same bias as an fp32 [B, H, Sq, S] tensor plus the
visibility mask, fed by kv_support._check_all. Gates: the project's own, unchanged - REF_ATOL and REL_TRUE on `out`,
1e-4 * max(1, |lse|) on `lse` (the imported _check / _check_lse). Caches are _Paged: every row at or beyond len_b and every unneeded
table entry is NaN, and _check asserts finite outputs."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_args   # noqa: E402
import kv_support as ks   # noqa: E402

pytestmark = pytest.mark.gpu

NAN = ks.NAN
_rand, _check, _check_lse, _Paged, _gather, _n_values, _check_all, _case, _capture = (
    ks._rand, ks._check, ks._check_lse, ks._Paged, ks._gather, ks._n_values, ks._check_all, ks._case, ks._capture)
_slopes, _steep, _alibi_operand, _run_decode, _run_prefill = ks._slopes, ks._steep, ks._alibi_operand, ks._run_alibi_decode, ks._run_alibi_prefill
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


# ---------------------------------------------------------------- 1. decode grid: empty cache, one key, a key past a tile / page edge, several tiles
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq", [1, 3])
@pytest.mark.parametrize("heads", [(16, 16), (64, 8), (8, 1)])
@pytest.mark.parametrize("page", [64, 256])
def test_decode_grid(pkg, dev, page, heads, Sq, D, dtype, causal):
    H, Hkv = heads
    lens = [0, 1, page + 1, 3 * page + 7]
    _run_decode(pkg, dev, 4, H, Hkv, Sq, D, DTYPES[dtype], page, lens, 1.0, _slopes(H, dev), causal=causal, seed=100 + D + page + H + Sq,
                what=f"decode D={D} {dtype} page={page} H={H}/{Hkv} Sq={Sq} causal={causal}")


# ---------------------------------------------------------------- 2. split-K: the key index is absolute in every split
@pytest.mark.parametrize("D", [64, 128])
def test_decode_split_k(pkg, dev, D):
    B, H, Hkv, Sq, page, max_pages, lens = 1, 64, 8, 1, 256, 20, [5000]
    plan = pkg._lib.kvcache_plan(kv_args._args_decode(pkg, B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages), _alibi_operand(pkg))
    assert plan[0][0].startswith("fasn_kvcache_fwd_alibi_kernel<") and plan[0][1] > B * Hkv, plan   # more than one split
    for slopes, tag in ((_steep(H, dev), "steep"), (_slopes(H, dev), "alibi")):
        _run_decode(pkg, dev, B, H, Hkv, Sq, D, torch.bfloat16, page, lens, _n_values((H,), dev, 200), slopes, seed=201, max_pages=max_pages,
                    what=f"decode split-K D={D} {tag} slopes")


@pytest.mark.parametrize("D", [64, 128])
def test_prefill_split_k(pkg, dev, D):
    B, H, Hkv, Sq, page, max_pages, lens = 1, 64, 8, 64, 256, 20, [5000]
    plan = pkg._lib.kvprefill_plan(kv_args._args_prefill(pkg, B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages), _alibi_operand(pkg))
    assert [k[0].split("<")[0] for k in plan] == ["fasn_kvprefill_fwd_alibi_kernel", "fasn_kvprefill_combine_kernel"]
    assert plan[0][1] > B * Hkv * -(-Sq // (128 // (H // Hkv))), plan                                # more than one split
    for slopes, tag in ((_steep(H, dev), "steep"), (_slopes(H, dev), "alibi")):
        _run_prefill(pkg, dev, B, H, Hkv, Sq, D, torch.bfloat16, page, lens, _n_values((H,), dev, 210), slopes, seed=211, max_pages=max_pages,
                     what=f"prefill split-K D={D} {tag} slopes", qlens=[37] if tag == "alibi" else None)


@pytest.mark.parametrize("call", ["decode", "prefill"])
def test_bias_decides_and_zero_slopes_are_no_slopes(pkg, dev, call):
    dtype, B, H, Hkv, D, page = torch.bfloat16, 3, 16, 4, 64, 64
    Sq = 3 if call == "decode" else 40
    lens = [page + 1, 3 * page + 7, 50]
    slopes = _slopes(H, dev)
    q, pc = _case(dev, B, H, Hkv, Sq, D, dtype, page, lens, 300)
    fa = pkg.flash_attention_n_kvcache if call == "decode" else pkg.flash_attention_n_kvcache_prefill
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)
    with_ref, _ = ks.reference_rows(q, kg, vg, lens, [Sq] * B, 1.0, True, slopes=slopes)
    plain = fa(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=1.0)
    err = (plain.float() - with_ref).abs().max().item()
    gate = ks.REL_TRUE[dtype] * max(with_ref.abs().max().item(), 1e-2)
    print(f"{call}: the call without slopes is {err:.3e} from the ALiBi reference, gate {gate:.3e}")
    assert err >= 10 * gate, "the slopes are a no-op at this shape: the tests above would show nothing"
    out, lse = fa(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=1.0, return_lse=True, alibi_slopes=slopes)
    _check(out, with_ref, dtype, f"{call} with slopes out")
    # zero slopes: the no-slope reference (the imported one), through the ALiBi kernels
    zout, zlse = fa(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=1.0, return_lse=True, alibi_slopes=torch.zeros(H, device=dev))
    o0, l0 = ks.reference_rows(q, kg, vg, lens, [Sq] * B, 1.0, True)
    _check(zout, o0, dtype, f"{call} zero slopes out")
    _check_lse(zlse, l0, f"{call} zero slopes lse")


# ---------------------------------------------------------------- 4. slope tensors: per batch element, strided, bf16
@pytest.mark.parametrize("call", ["decode", "prefill"])
@pytest.mark.parametrize("form", ["BH", "B1", "strided H", "bf16 H", "0-d", "fp64 1H"])
def test_slope_tensor_forms(pkg, dev, form, call):
    dtype, B, H, Hkv, D, page = torch.float16, 3, 16, 4, 128, 64
    Sq = 2 if call == "decode" else 50
    lens = [200, 3, 65]
    base = _slopes(H, dev)
    if form == "BH":
        slopes = (base.view(1, H) * torch.tensor([1.0, 0.5, 3.0], device=dev).view(B, 1)).contiguous()
        assert slopes.shape == (B, H) and len(set(slopes.view(-1).tolist())) > H
    elif form == "B1":
        slopes = torch.tensor([0.5, 0.03125, 0.0], device=dev).view(B, 1)
    elif form == "strided H":
        slopes = torch.stack((base, torch.full_like(base, NAN)), dim=1)[:, 0]      # every other element of a buffer whose rest is NaN
        assert slopes.shape == (H,) and not slopes.is_contiguous()
    elif form == "bf16 H":
        slopes = base.bfloat16()                                                      # converted to fp32 by the call: the reference reads the bf16 values
        assert not torch.equal(slopes.float(), base)
    elif form == "0-d":
        slopes = torch.tensor(0.0625, device=dev)
    else:
        slopes = base.double().view(1, H)
    run = _run_decode if call == "decode" else _run_prefill
    run(pkg, dev, B, H, Hkv, Sq, D, dtype, page, lens, 0.5, slopes, seed=400, what=f"{call} slopes[{form}]")


# ---------------------------------------------------------------- 5. next to the sink: tensor n with zeros, an empty batch element
@pytest.mark.parametrize("call", ["decode", "prefill"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_with_the_sink(pkg, dev, dtype, call):
    B, H, Hkv, D, page = 3, 32, 8, 64, 64
    Sq = 4 if call == "decode" else 70
    lens = [130, 0, 2]
    n = _n_values((H,), dev, 500)
    assert (n == 0).any() and (n > 0).any()
    run = _run_decode if call == "decode" else _run_prefill
    res = run(pkg, dev, B, H, Hkv, Sq, D, DTYPES[dtype], page, lens, n, _slopes(H, dev), seed=501, what=f"{call} sink {dtype}")
    out, lse = res[0], res[1]
    logn = torch.where(n > 0, torch.log(n), torch.full_like(n, float("-inf")))
    assert (out[1] == 0).all() and torch.allclose(lse[1], logn.view(H, 1).expand(H, Sq), atol=1e-6, rtol=0)   # len 0: nothing to see
    # causal, len 2 < Sq: the first Sq - 2 positions see no key either
    assert (out[2, :, :Sq - 2] == 0).all() and torch.allclose(lse[2, :, :Sq - 2], logn.view(H, 1).expand(H, Sq - 2), atol=1e-6, rtol=0)
    assert (out[2, :, Sq - 2:].float().abs().amax(-1) > 0).all()


# ---------------------------------------------------------------- 6. prefill grid
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Dd", [(64, "bf16"), (128, "fp16")])
@pytest.mark.parametrize("heads", [(64, 8), (16, 16), (12, 4)])
@pytest.mark.parametrize("Sq", [17, 200])
def test_prefill_grid(pkg, dev, Sq, heads, Dd, causal):
    H, Hkv = heads
    D, dtype = Dd
    page = 64
    lens = [0, Sq - 5, page + 1, 2 * page]
    _run_prefill(pkg, dev, 4, H, Hkv, Sq, D, DTYPES[dtype], page, lens, 1.0, _slopes(H, dev), causal=causal, seed=600 + D + H + Sq,
                 what=f"prefill D={D} {dtype} H={H}/{Hkv} Sq={Sq} causal={causal}")


@pytest.mark.parametrize("append", [False, True])
@pytest.mark.parametrize("causal", [True, False])
def test_prefill_ragged_queries(pkg, dev, causal, append):
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.bfloat16, 4, 64, 8, 200, 64, 64, 8
    qlens = [Sq, 1, 0, Sq // 2]
    lens = [10, page + 1, 70, 2 * page]                                                 # keys in the cache before the call
    n = _n_values((B, H), dev, 700)
    slopes = _slopes(H, dev)
    q = _rand((B, H, Sq, D), dtype, dev, 701)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 702)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 703, std=1.0)
    kn = _rand((B, Hkv, Sq, D), dtype, dev, 704)
    vn = _rand((B, Hkv, Sq, D), dtype, dev, 705, std=1.0)
    total = [ln + (ql if append else 0) for ln, ql in zip(lens, qlens)]
    if append:   # the dense picture of the cache after the append
        for b in range(B):
            kd[b, :, lens[b]:total[b]] = kn[b, :, :qlens[b]]
            vd[b, :, lens[b]:total[b]] = vn[b, :, :qlens[b]]
    pc = _Paged(kd, vd, lens, page, max_pages, 706, alloc_all=True)   # rows at or beyond the OLD length: NaN until the append writes them
    qs = torch.tensor(qlens, dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, k_new=kn if append else None,
                                                     v_new=vn if append else None, query_seqlens=qs, softmax_n_param=n, is_causal=causal,
                                                     return_lse=True, alibi_slopes=slopes)
    assert torch.equal(pc.lens.cpu(), torch.tensor(lens, dtype=torch.int32)), "cache_seqlens was modified"
    _check_all(pkg, out, lse, q, ks._visible_dense(kd, total), ks._visible_dense(vd, total), total, qlens, n, causal, dtype,
               f"prefill ragged causal={causal} append={append}", slopes=slopes)


def test_prefill_dense_cache(pkg, dev):
    dtype, B, H, Hkv, Sq, D, cap = torch.float16, 3, 16, 4, 150, 128, 200   # (a dense capacity need not be a multiple of 64)
    lens = [200, 77, 0]
    q = _rand((B, H, Sq, D), dtype, dev, 710)
    kc = _rand((B, cap, Hkv, D), dtype, dev, 711)
    vc = _rand((B, cap, Hkv, D), dtype, dev, 712, std=1.0)
    for b, ln in enumerate(lens):
        kc[b, ln:] = NAN
        vc[b, ln:] = NAN
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    slopes = _slopes(H, dev)
    out, lse = pkg.flash_attention_n_kvcache_prefill(q, kc, vc, sl, softmax_n_param=0.5, return_lse=True, alibi_slopes=slopes)
    keep = torch.arange(cap, device=dev).view(1, -1, 1, 1) < sl.view(-1, 1, 1, 1)
    kg, vg = (torch.where(keep, t, torch.zeros_like(t)).permute(0, 2, 1, 3).contiguous() for t in (kc, vc))
    _check_all(pkg, out, lse, q, kg, vg, lens, [Sq] * B, 0.5, True, dtype, "prefill dense", slopes=slopes)
    d_out, d_lse = pkg.flash_attention_n_kvcache(q[:, :, :8].contiguous(), kc, vc, sl, softmax_n_param=0.5, return_lse=True, alibi_slopes=slopes)
    _check_all(pkg, d_out, d_lse, q[:, :, :8].contiguous(), kg, vg, lens, [8] * B, 0.5, True, dtype, "decode dense", slopes=slopes)


@pytest.mark.parametrize("call", ["decode", "prefill"])
@pytest.mark.parametrize("scale", [-0.2, 0.2])
def test_scale_of_any_sign(pkg, dev, scale, call):
    """scale <= 0 is the prefill kernel's c <= 0 path without slopes; with slopes every sign takes the one biased path"""
    dtype, B, H, Hkv, D, page = torch.bfloat16, 3, 32, 8, 128, 64
    Sq = 4 if call == "decode" else 90
    run = _run_decode if call == "decode" else _run_prefill
    run(pkg, dev, B, H, Hkv, Sq, D, dtype, page, [70, 200, 9], _n_values((H,), dev, 720), _slopes(H, dev), seed=721, scale=scale,
        what=f"{call} scale={scale}")


# ---------------------------------------------------------------- 7. agreement of the two calls where both apply
@pytest.mark.parametrize("causal", [True, False])
def test_prefill_agrees_with_decode(pkg, dev, causal):
    dtype, B, H, Hkv, Sq, D, page = torch.bfloat16, 3, 32, 8, 16, 64, 64
    lens = [300, 7, 64]
    q, pc = _case(dev, B, H, Hkv, Sq, D, dtype, page, lens, 800, max_pages=6)
    n, slopes = _n_values((H,), dev, 801), _slopes(H, dev)
    a, la = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, is_causal=causal, return_lse=True, alibi_slopes=slopes)
    d, ld = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, is_causal=causal, return_lse=True, alibi_slopes=slopes)
    _check(a, d, dtype, "prefill vs decode out")
    _check_lse(la, ld, "prefill vs decode lse")


# ---------------------------------------------------------------- 8. HIP graph: the position offset follows the lengths in device memory
def test_graph_replay_decode_follows_the_lengths(pkg, dev):
    """One capture (linear, one stream); cache_seqlens changes in place between replays: the reference at the NEW lengths"""
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.bfloat16, 2, 16, 4, 2, 64, 64, 4
    q = _rand((B, H, Sq, D), dtype, dev, 900)
    pool_k = _rand((B * max_pages, page, Hkv, D), dtype, dev, 901)
    pool_v = _rand((B * max_pages, page, Hkv, D), dtype, dev, 902, std=1.0)
    table = torch.arange(B * max_pages, dtype=torch.int32, device=dev).view(B, max_pages).flip(1).contiguous()
    sl = torch.tensor([62, 100], dtype=torch.int32, device=dev)
    n, slopes = _n_values((H,), dev, 903), _slopes(H, dev)
    g, (go, glse) = _capture(lambda: pkg.flash_attention_n_kvcache(q, pool_k, pool_v, sl, block_table=table, softmax_n_param=n, return_lse=True,
                                                                   alibi_slopes=slopes))
    seen = []
    for lens in ([62, 100], [63, 129], [200, 1]):
        with torch.no_grad():
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        kg, vg = _gather(pool_k, table, lens, page), _gather(pool_v, table, lens, page)
        _check_all(pkg, go, glse, q, kg, vg, lens, [Sq] * B, n, True, dtype, f"decode replay at {lens}", witness=False, slopes=slopes)
        eo, el = pkg.flash_attention_n_kvcache(q, pool_k, pool_v, sl.clone(), block_table=table, softmax_n_param=n, return_lse=True, alibi_slopes=slopes)
        assert torch.equal(go, eo) and torch.equal(glse, el), f"replay at {lens}: differs from the eager call"
        seen.append(go.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


@pytest.mark.parametrize("shape", [dict(B=2, Sq=150, max_pages=8), dict(B=1, Sq=32, max_pages=40)])
def test_graph_replay_prefill_follows_the_lengths(pkg, dev, shape):
    """cache_seqlens and query_seqlens change in place between replays; both plans (one split / several)"""
    dtype, H, Hkv, D, page = torch.bfloat16, 16, 4, 64, 64
    B, Sq, max_pages = shape["B"], shape["Sq"], shape["max_pages"]
    q = _rand((B, H, Sq, D), dtype, dev, 910)
    pool_k = _rand((B * max_pages, page, Hkv, D), dtype, dev, 911)
    pool_v = _rand((B * max_pages, page, Hkv, D), dtype, dev, 912, std=1.0)
    table = torch.arange(B * max_pages, dtype=torch.int32, device=dev).view(B, max_pages).flip(1).contiguous()
    sl = torch.tensor([62, 100][:B], dtype=torch.int32, device=dev)
    ql = torch.tensor([Sq, Sq // 3][:B], dtype=torch.int32, device=dev)
    n, slopes = _n_values((H,), dev, 913), _slopes(H, dev)
    g, (go, glse) = _capture(lambda: pkg.flash_attention_n_kvcache_prefill(q, pool_k, pool_v, sl, block_table=table, query_seqlens=ql, softmax_n_param=n,
                                                                           return_lse=True, alibi_slopes=slopes))
    for lens, qlens in (([62, 100], [Sq, Sq // 3]), ([page * 3 + 1, 5], [Sq - 7, 1]), ([300, 129], [9, Sq])):
        lens, qlens = lens[:B], qlens[:B]
        with torch.no_grad():
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
            ql.copy_(torch.tensor(qlens, dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        kg, vg = _gather(pool_k, table, lens, page), _gather(pool_v, table, lens, page)
        _check_all(pkg, go, glse, q, kg, vg, lens, qlens, n, True, dtype, f"prefill replay at {lens} / {qlens}", witness=False, slopes=slopes)
        eo, el = pkg.flash_attention_n_kvcache_prefill(q, pool_k, pool_v, sl.clone(), block_table=table, query_seqlens=ql.clone(), softmax_n_param=n,
                                                       return_lse=True, alibi_slopes=slopes)
        assert torch.equal(go, eo) and torch.equal(glse, el), f"replay at {lens} / {qlens}: differs from the eager call"


# ---------------------------------------------------------------- 9. determinism
@pytest.mark.parametrize("call", ["decode", "prefill one split", "prefill several splits"])
def test_deterministic(pkg, dev, call):
    dtype, H, Hkv, D, page = torch.bfloat16, 64, 8, 64, 256
    if call == "decode":
        B, Sq, max_pages, lens = 4, 1, 20, [5000, 1, 4096, 2049]
    elif call == "prefill one split":
        B, Sq, max_pages, lens = 4, 300, 9, [2000, 1, 1024, 2049]
    else:
        B, Sq, max_pages, lens = 1, 64, 20, [5000]
    q, pc = _case(dev, B, H, Hkv, Sq, D, dtype, page, lens, 1000, max_pages=max_pages)
    n, slopes = _n_values((H,), dev, 1001), _slopes(H, dev)
    fa = pkg.flash_attention_n_kvcache if call == "decode" else pkg.flash_attention_n_kvcache_prefill
    a = fa(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, return_lse=True, alibi_slopes=slopes)
    b = fa(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, return_lse=True, alibi_slopes=slopes)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert math.isfinite(a[0].float().abs().max().item())
