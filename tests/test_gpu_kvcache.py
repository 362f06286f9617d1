"""flash_attention_n_kvcache on the GPU: paged / dense K/V cache, lengths in device memory, grouped-query heads as rows of one problem,
a softmax_n per query head, append, graph replay.

Reference, gates and second witness are those of tests/kv_support.py: the visible pages gathered into dense [B, Hkv, Smax, D] tensors on
the device, the per-batch visibility as a boolean mask, fp32 torch with the explicit sink column; REF_ATOL / REL_TRUE on `out`, the
1e-4-scaled gate on `lse`; flash_attention_n on the gathered dense K/V with the same mask and n as the witness."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_support as ks   # noqa: E402
from flash_attention_softmax_n_amd import synth   # noqa: E402

pytestmark = pytest.mark.gpu

NAN = ks.NAN
_rand, _check, _check_lse, _visibility, _reference, _Paged, _gather, _run_case, _n_values = (
    ks._rand, ks._check, ks._check_lse, ks._visibility, ks.reference, ks._Paged, ks._gather, ks._run_case_decode, ks._n_values)


# ---------------------------------------------------------------- 1. shapes x pages x ragged lengths
@pytest.mark.parametrize("Sq", [1, 4])
@pytest.mark.parametrize("heads", [(16, 16), (32, 8), (64, 8), (8, 1)])
@pytest.mark.parametrize("page", [64, 256])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("D", [64, 128])
def test_paged_ragged(pkg, dev, D, dtype, page, heads, Sq):
    H, Hkv = heads
    # a multiple of the page, one row into a page, fewer than 64 keys, none at all: both sets under every (D, dtype, page, heads)
    lens = [2 * page, page + 1, 37] if Sq == 1 else [0, 3 * page, 2 * page + 1]
    _run_case(pkg, dev, 3, H, Hkv, Sq, D, dtype, page, lens, 1.0, seed=100 + D + page + H + Sq, what=f"D={D} {dtype} page={page} H={H}/{Hkv} Sq={Sq}")


# ---------------------------------------------------------------- 2. softmax_n: scalars and tensors
@pytest.mark.parametrize("n", [0, 1, 0.5])
def test_scalar_n(pkg, dev, n):
    _run_case(pkg, dev, 3, 32, 8, 2, 64, torch.bfloat16, 64, [130, 64, 5], n, seed=210, what=f"n={n}")


@pytest.mark.parametrize("shape", ["H", "BH", "B1"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_tensor_n_per_row(pkg, dev, shape, dtype):
    B, H, Hkv = 3, 32, 8
    n = _n_values({"H": (H,), "BH": (B, H), "B1": (B, 1)}[shape], dev, 220)
    assert (n == 0).any() and (n > 0).any()
    _run_case(pkg, dev, B, H, Hkv, 4, 128, dtype, 64, [200, 3, 65], n, seed=221, what=f"n[{shape}] {dtype}")


# ---------------------------------------------------------------- 3. shuffled table, shared prefix pages, poison page
def test_shared_prefix_and_poison(pkg, dev):
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.bfloat16, 3, 32, 8, 1, 64, 64, 6
    lens = [150, 100, 64]
    q = _rand((B, H, Sq, D), dtype, dev, 300)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 301)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 302, std=1.0)
    kd[1, :, :page] = kd[0, :, :page]   # batch elements 0 and 1 share their first page (a common prefix)
    vd[1, :, :page] = vd[0, :, :page]
    pc = _Paged(kd, vd, lens, page, max_pages, 303)
    pc.table[1, 0] = pc.table[0, 0]
    assert (pc.table[:, 3:] == pc.poison).all() and torch.isnan(pc.k[pc.poison]).all()   # max_pages larger than needed: poison entries
    n = _n_values((H,), dev, 304)
    out, lse = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, return_lse=True)
    assert torch.isfinite(out).all()
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)
    vis = _visibility(lens, Sq, kg.shape[2], True, dev)
    o_ref, lse_ref = _reference(q, kg, vg, vis, n)
    _check(out, o_ref, dtype, "shared prefix out")
    _check_lse(lse, lse_ref, "shared prefix lse")
    _check(out, pkg.flash_attention_n(q, kg, vg, softmax_n_param=n, attn_mask=vis), dtype, "shared prefix vs flash_attention_n")


# ---------------------------------------------------------------- 4. dense cache, strided views
@pytest.mark.parametrize("D", [64, 128])
def test_dense_cache(pkg, dev, D):
    dtype, B, H, Hkv, Sq, cap = torch.float16, 3, 16, 4, 2, 200   # (a dense capacity need not be a multiple of 64)
    lens = [200, 77, 0]
    q = _rand((B, H, Sq, D), dtype, dev, 400)
    kc = _rand((B, cap, Hkv, D), dtype, dev, 401)
    vc = _rand((B, cap, Hkv, D), dtype, dev, 402, std=1.0)
    for b, ln in enumerate(lens):
        kc[b, ln:] = NAN
        vc[b, ln:] = NAN
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache(q, kc, vc, sl, softmax_n_param=0.5, return_lse=True)
    keep = torch.arange(cap, device=dev).view(1, -1, 1, 1) < sl.view(-1, 1, 1, 1)
    kg, vg = (torch.where(keep, t, torch.zeros_like(t)).permute(0, 2, 1, 3).contiguous() for t in (kc, vc))
    vis = _visibility(lens, Sq, cap, True, dev)
    o_ref, lse_ref = _reference(q, kg, vg, vis, 0.5)
    _check(out, o_ref, dtype, "dense out")
    _check_lse(lse, lse_ref, "dense lse")
    _check(out, pkg.flash_attention_n(q, kg, vg, softmax_n_param=0.5, attn_mask=vis), dtype, "dense vs flash_attention_n")


def test_strided_view_of_a_fused_buffer(pkg, dev):
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.bfloat16, 2, 16, 4, 1, 64, 64, 3
    lens = [129, 64]
    q = _rand((B, H, Sq, D), dtype, dev, 410)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 411)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 412, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, 413)
    fused = torch.stack((pc.k, pc.v), dim=2)           # [num_pages, page, 2, Hkv, D]
    kv, vv = fused[:, :, 0], fused[:, :, 1]
    assert not kv.is_contiguous() and kv.stride(1) == 2 * Hkv * D
    out = pkg.flash_attention_n_kvcache(q, kv, vv, pc.lens, block_table=pc.table, softmax_n_param=1.0)
    want = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=1.0)
    assert torch.equal(out, want)
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)
    _check(out, _reference(q, kg, vg, _visibility(lens, Sq, kg.shape[2], True, dev), 1.0)[0], dtype, "strided view out")


# ---------------------------------------------------------------- 5. per-batch causal limit, rows that see nothing
@pytest.mark.parametrize("causal", [True, False])
def test_causal_per_batch_and_empty_rows(pkg, dev, causal):
    dtype, B, H, Hkv, Sq, D, page = torch.bfloat16, 3, 16, 4, 4, 64, 64
    lens = [2, 0, 130]
    n = _n_values((H,), dev, 500)
    out, lse, o_ref, lse_ref = _run_case(pkg, dev, B, H, Hkv, Sq, D, dtype, page, lens, n, causal=causal, seed=501, what=f"causal={causal}")
    logn = torch.where(n > 0, torch.log(n), torch.full_like(n, float("-inf")))
    assert (out[1] == 0).all() and torch.allclose(lse[1], logn.view(H, 1).expand(H, Sq), atol=1e-6, rtol=0)   # len 0: nothing to see
    if causal:   # len 2 < Sq: positions 0 and 1 see no key, position 2 sees key 0, position 3 keys 0 and 1
        assert (out[0, :, :2] == 0).all() and torch.allclose(lse[0, :, :2], logn.view(H, 1).expand(H, 2), atol=1e-6, rtol=0)
        assert (out[0, :, 2:].float().abs().amax(-1) > 0).all()


# ---------------------------------------------------------------- 6. append
def test_append_writes_exactly_the_new_rows(pkg, dev):
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.bfloat16, 3, 16, 4, 4, 64, 64, 3
    cap = page * max_pages
    lens = [10, page - 2, cap - 1]   # inside a page; across a page boundary; one row of room: three rows dropped
    q = _rand((B, H, Sq, D), dtype, dev, 600)
    kd = _rand((B, Hkv, cap, D), dtype, dev, 601)
    vd = _rand((B, Hkv, cap, D), dtype, dev, 602, std=1.0)
    kn = _rand((B, Hkv, Sq, D), dtype, dev, 603)
    vn = _rand((B, Hkv, Sq, D), dtype, dev, 604, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, 605, alloc_all=True, guard=7.0)
    k0, v0, lens0 = pc.k.clone(), pc.v.clone(), pc.lens.clone()
    out = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, k_new=kn, v_new=vn, softmax_n_param=1.0)
    assert torch.equal(pc.lens, lens0), "cache_seqlens was modified"
    assert torch.isfinite(out).all()
    ke, ve = k0.clone(), v0.clone()   # expected cache: the old one with the new rows at len_b .. len_b + Sq - 1, below the capacity
    for b in range(B):
        for i in range(Sq):
            pos = lens[b] + i
            if pos < cap:
                pid = int(pc.table[b, pos // page])
                ke[pid, pos % page] = kn[b, :, i]
                ve[pid, pos % page] = vn[b, :, i]
    assert torch.equal(pc.k.view(torch.int16), ke.view(torch.int16)), "k_cache: not exactly the new rows"
    assert torch.equal(pc.v.view(torch.int16), ve.view(torch.int16)), "v_cache: not exactly the new rows"
    assert (pc.k[-1] == 7.0).all() and (pc.v[-1] == 7.0).all(), "guard page behind the cache was written"
    # the output is the one of the pre-appended cache with lengths + Sq (the element at capacity - 1: contents only, its newest keys were dropped)
    lens_after = torch.tensor([ln + Sq for ln in lens], dtype=torch.int32, device=dev)
    want = pkg.flash_attention_n_kvcache(q, ke, ve, lens_after, block_table=pc.table, softmax_n_param=1.0)
    assert torch.equal(out[:2], want[:2])
    la = [ln + Sq for ln in lens[:2]]
    kg, vg = _gather(ke, pc.table[:2], la, page), _gather(ve, pc.table[:2], la, page)
    _check(out[:2], _reference(q[:2], kg, vg, _visibility(la, Sq, kg.shape[2], True, dev), 1.0)[0], dtype, "append out")


# ---------------------------------------------------------------- 7. many splits, more than one round of workgroups
def test_long_many_splits(pkg, dev):
    _run_case(pkg, dev, 2, 64, 8, 1, 64, torch.bfloat16, 256, [30000, 777], _n_values((64,), dev, 700), seed=701, max_pages=118, what="long (2,64/8,30000)")


def test_many_batch_elements(pkg, dev):
    B = 64
    lens = [1 + (b * 8191) // (B - 1) for b in range(B)]   # spread over 1 .. 8192
    assert lens[0] == 1 and lens[-1] == 8192
    _run_case(pkg, dev, B, 16, 16, 1, 128, torch.float16, 256, lens, 1.0, seed=710, max_pages=32, what="(64,16,1..8192,128)")


# ---------------------------------------------------------------- 8. determinism
def test_deterministic(pkg, dev):
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.bfloat16, 4, 64, 8, 1, 64, 256, 20
    lens = [5000, 1, 4096, 2049]
    q = _rand((B, H, Sq, D), dtype, dev, 800)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 801)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 802, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, 803)
    n = _n_values((H,), dev, 804)
    a = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, return_lse=True)
    b = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, return_lse=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------- 9. HIP graph
def test_graph_replay_follows_lengths_table_and_cache(pkg, dev):
    """One capture (append + forward), three replays after query, k_new, v_new, cache_seqlens (+1) and one block-table row changed in
    place: the bits of an eager call on cloned inputs."""
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.bfloat16, 2, 16, 4, 1, 64, 64, 4
    cap = page * max_pages
    lens = [62, 100]
    q = _rand((B, H, Sq, D), dtype, dev, 900)
    kn = _rand((B, Hkv, Sq, D), dtype, dev, 901)
    vn = _rand((B, Hkv, Sq, D), dtype, dev, 902, std=1.0)
    num_pages = 2 * B * max_pages
    pool_k = _rand((num_pages, page, Hkv, D), dtype, dev, 903)
    pool_v = _rand((num_pages, page, Hkv, D), dtype, dev, 904, std=1.0)
    table = torch.arange(B * max_pages, dtype=torch.int32, device=dev).view(B, max_pages).flip(1).contiguous()
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    n = _n_values((H,), dev, 905)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            pkg.flash_attention_n_kvcache(q, pool_k, pool_v, sl, block_table=table, k_new=kn, v_new=vn, softmax_n_param=n, return_lse=True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        go, glse = pkg.flash_attention_n_kvcache(q, pool_k, pool_v, sl, block_table=table, k_new=kn, v_new=vn, softmax_n_param=n, return_lse=True)
    for step in range(3):
        with torch.no_grad():
            q.copy_(_rand((B, H, Sq, D), dtype, dev, 910 + step))
            kn.copy_(_rand((B, Hkv, Sq, D), dtype, dev, 920 + step))
            vn.copy_(_rand((B, Hkv, Sq, D), dtype, dev, 930 + step, std=1.0))
            sl += 1
            table[0] = torch.arange(B * max_pages + step * max_pages // 2, B * max_pages + step * max_pages // 2 + max_pages, dtype=torch.int32, device=dev)
        ck, cv, csl, ctab = pool_k.clone(), pool_v.clone(), sl.clone(), table.clone()
        g.replay()
        torch.cuda.synchronize()
        eo, else_ = pkg.flash_attention_n_kvcache(q.clone(), ck, cv, csl, block_table=ctab, k_new=kn.clone(), v_new=vn.clone(), softmax_n_param=n.clone(), return_lse=True)
        assert torch.equal(go, eo) and torch.equal(glse, else_), f"replay {step}: output differs from the eager call"
        assert torch.equal(pool_k, ck) and torch.equal(pool_v, cv), f"replay {step}: cache differs from the eager call's"
        assert torch.isfinite(go).all()
    assert int(sl[0]) == lens[0] + 3 and cap > int(sl.max())


# ---------------------------------------------------------------- 10. GPT-OSS-shaped decode
def test_gpt_oss_decode(pkg, dev):
    dtype, B, H, Hkv, Sq, D, page = torch.bfloat16, 4, 64, 8, 1, 64, 256
    lens = [3117, 2048, 1, 4000]
    max_pages = 17
    sinks = synth.counter_normal((H,), 1000, std=1.0, dtype=torch.float32, device=dev)
    n = torch.exp(sinks)
    q = _rand((B, H, Sq, D), dtype, dev, 1001)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 1002)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 1003, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, 1004)
    out, lse = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, return_lse=True)
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)
    S = kg.shape[2]
    o_ref, lse_ref = _reference(q, kg, vg, _visibility(lens, Sq, S, True, dev), n)
    _check(out, o_ref, dtype, "GPT-OSS decode out")
    _check_lse(lse, lse_ref, "GPT-OSS decode lse")
    keypad = (torch.arange(S, device=dev).view(1, 1, 1, S) < pc.lens.view(B, 1, 1, 1))   # [B,1,1,S]
    _check(out, pkg.flash_attention_n(q, kg, vg, softmax_n_param=n, attn_mask=keypad), dtype, "GPT-OSS decode vs flash_attention_n")
    assert math.isfinite(out.float().abs().max().item())


# ---------------------------------------------------------------- lengths beyond the capacity, scale, [B, Sq, H, D] queries
def test_length_beyond_capacity_is_clamped(pkg, dev):
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.float16, 2, 16, 4, 1, 64, 64, 2
    cap = page * max_pages
    q = _rand((B, H, Sq, D), dtype, dev, 1100)
    kd = _rand((B, Hkv, cap, D), dtype, dev, 1101)
    vd = _rand((B, Hkv, cap, D), dtype, dev, 1102, std=1.0)
    pc = _Paged(kd, vd, [cap, cap], page, max_pages, 1103)
    over = torch.tensor([cap + 1000, cap], dtype=torch.int32, device=dev)
    out = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, over, block_table=pc.table, softmax_n_param=1.0)
    want = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=1.0)
    assert torch.equal(out, want)
    _check(out, _reference(q, kd, vd, _visibility([cap, cap], Sq, cap, True, dev), 1.0)[0], dtype, "clamped length out")


def test_scale_and_strided_query(pkg, dev):
    """a [B, Sq, H, D] query seen as [B, H, Sq, D] (the layout serving stacks keep) goes in without a copy; scale is the caller's"""
    dtype, B, H, Hkv, Sq, D, page = torch.bfloat16, 3, 32, 8, 4, 128, 64
    lens = [70, 200, 9]
    qb = _rand((B, Sq, H, D), dtype, dev, 1110)
    q = qb.transpose(1, 2)
    assert not q.is_contiguous()
    max_pages = 4
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 1111)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 1112, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, 1113)
    n = _n_values((H,), dev, 1114)
    out, lse = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, scale=0.2, return_lse=True)
    assert torch.equal(out, pkg.flash_attention_n_kvcache(q.contiguous(), pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, scale=0.2))
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)
    o_ref, lse_ref = _reference(q.contiguous(), kg, vg, _visibility(lens, Sq, kg.shape[2], True, dev), n, scale=0.2)
    _check(out, o_ref, dtype, "scale 0.2 out")
    _check_lse(lse, lse_ref, "scale 0.2 lse")
