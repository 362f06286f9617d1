"""flash_attention_n_kvcache_window on the GPU: a sliding window of W keys over the paged / dense K/V cache, decode and prefill kernels.

Reference of every case: kv_support.reference_rows (fp32 torch, explicit sink column, per batch element on q[b, :, :qlen_b]) under the
rule W: the visibility  j < len_b and p_i - W < j <= p_i,  p_i = i + len_b - qlen_b.
Gates: those of the cache tests, imported unchanged (REF_ATOL / REL_TRUE on `out`, 1e-4 on `lse`). Second witness: flash_attention_n
on the gathered dense K/V with the same visibility as a boolean attn_mask.

Poison. The reference inputs are gathered first. Then every cache row below first_b = 64 * floor(max(0, len_b - qlen_b - W + 1) / 64)
becomes NaN and every block-table entry of a page wholly below first_b points at the poison page (a valid id whose page is NaN): a
kernel that still walks from tile 0 fails every case whose window starts beyond the first tile."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_args   # noqa: E402
import kv_support as ks   # noqa: E402
from flash_attention_softmax_n_amd import synth   # noqa: E402

pytestmark = pytest.mark.gpu

NAN = ks.NAN
_rand, _check, _check_lse, _Paged, _gather, _n_values, _check_all, _case, _capture, _poison, _first = (
    ks._rand, ks._check, ks._check_lse, ks._Paged, ks._gather, ks._n_values, ks._check_all, ks._case, ks._capture, ks._poison, ks._first)
REL_TRUE = ks.REL_TRUE
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _run(pkg, dev, B, H, Hkv, Sq, D, dtype, page, lens, n, windows, seed=1, max_pages=None, what="", witness=True, qlens=None, prefill=False):
    """One cache, the windows from the widest to the narrowest (the poison only grows), no append. prefill=True passes full query
    lengths, which takes the prefill kernels whatever the shape."""
    q, pc = _case(dev, B, H, Hkv, Sq, D, dtype, page, lens, seed, max_pages)
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)
    ql = qlens or [Sq] * B
    qs = torch.tensor(ql, dtype=torch.int32, device=dev) if (qlens is not None or prefill) else None
    res = None
    for W in sorted(windows, reverse=True):
        _poison(pc.k, pc.v, pc.table, page, pc.poison, lens, ql, W)
        out, lse = pkg.flash_attention_n_kvcache_window(q, pc.k, pc.v, pc.lens, W, block_table=pc.table, query_seqlens=qs, softmax_n_param=n,
                                                        return_lse=True)
        o_ref, lse_ref = _check_all(pkg, out, lse, q, kg, vg, lens, ql, n, W, dtype, f"{what} W={W}", witness)
        res = (out, lse, o_ref, lse_ref)
    return res


# ---------------------------------------------------------------- 1. decode grid
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq", [1, 3])
@pytest.mark.parametrize("heads", [(16, 16), (64, 8), (8, 1)])
@pytest.mark.parametrize("page", [64, 256])
def test_decode_grid(pkg, dev, page, heads, Sq, D, dtype):
    """an empty cache, one key, a key past a page edge, several pages; windows of one key, a few, one tile, one tile and a key, several tiles"""
    H, Hkv = heads
    lens = [0, 1, page + 1, 3 * page + 7]
    _run(pkg, dev, 4, H, Hkv, Sq, D, DTYPES[dtype], page, lens, 1.0, [1, 5, 64, 65, 200], seed=100 + D + page + H + Sq,
         what=f"decode D={D} {dtype} page={page} H={H}/{Hkv} Sq={Sq}")


@pytest.mark.parametrize("D", [32, 256])
def test_decode_and_prefill_at_the_outer_head_dims(pkg, dev, D):
    lens = [0, 1, 65, 199]
    _run(pkg, dev, 4, 16, 4, 3, D, torch.bfloat16, 64, lens, 0.5, [5, 65], seed=150 + D, what=f"decode D={D}")
    _run(pkg, dev, 4, 16, 4, 40, D, torch.float16, 64, lens, 0.5, [5, 65], seed=160 + D, what=f"prefill D={D}", qlens=[40, 1, 0, 20])


# ---------------------------------------------------------------- 2. the window decides: a test of these tests
@pytest.mark.parametrize("call", ["decode", "prefill"])
def test_window_decides_and_a_wide_window_is_no_window(pkg, dev, call):
    dtype, B, H, Hkv, D, page, W = torch.bfloat16, 3, 16, 4, 64, 64, 16
    Sq = 3 if call == "decode" else 40
    lens = [page + 1, 3 * page + 7, 50]
    q, pc = _case(dev, B, H, Hkv, Sq, D, dtype, page, lens, 300)
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)
    fa = pkg.flash_attention_n_kvcache if call == "decode" else pkg.flash_attention_n_kvcache_prefill
    qs = None if call == "decode" else torch.full((B,), Sq, dtype=torch.int32, device=dev)
    with_ref, _ = ks.reference_rows(q, kg, vg, lens, [Sq] * B, 1.0, W)
    plain, plain_lse = fa(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=1.0, return_lse=True)
    err = (plain.float() - with_ref).abs().max().item()
    gate = REL_TRUE[dtype] * max(with_ref.abs().max().item(), 1e-2)
    print(f"{call}: the call without a window is {err:.3e} from the window reference, gate {gate:.3e}")
    assert err >= 10 * gate, "the window is a no-op at this shape: the tests of this file would show nothing"
    # a window at or beyond the capacity: the no-window reference (the imported one), through the window kernels
    capacity = page * pc.max_pages
    o0, l0 = ks.reference_rows(q, kg, vg, lens, [Sq] * B, 1.0, True)
    for wide in (capacity, capacity + 1, 10 ** 12):
        out, lse = pkg.flash_attention_n_kvcache_window(q, pc.k, pc.v, pc.lens, wide, block_table=pc.table, query_seqlens=qs,
                                                        softmax_n_param=1.0, return_lse=True)
        _check(out, o0, dtype, f"{call} W={wide} out")
        _check_lse(lse, l0, f"{call} W={wide} lse")
        print(f"{call} W={wide}: bit-equal to the call without a window: out {torch.equal(out, plain)}, lse {torch.equal(lse, plain_lse)}")
    # and the narrow window itself, poisoned
    _poison(pc.k, pc.v, pc.table, page, pc.poison, lens, [Sq] * B, W)
    out, lse = pkg.flash_attention_n_kvcache_window(q, pc.k, pc.v, pc.lens, W, block_table=pc.table, query_seqlens=qs, softmax_n_param=1.0,
                                                    return_lse=True)
    _check_all(pkg, out, lse, q, kg, vg, lens, [Sq] * B, 1.0, W, dtype, f"{call} W={W}")


# ---------------------------------------------------------------- 3. split-K: the shares start at the window's first tile, the sink sits on split 0
def _window_operand(pkg, W):
    return pkg._lib.KvWindow(window=W, reserved=0)


@pytest.mark.parametrize("call", ["decode", "prefill"])
def test_split_k(pkg, dev, call):
    B, H, Hkv, D, page, max_pages, lens, W = 1, 64, 8, 64, 256, 20, [5000], 3000
    Sq, qlens = (1, None) if call == "decode" else (64, [37])
    if call == "decode":
        plan = pkg._lib.kvcache_window_plan(kv_args._args_decode(pkg, B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages), _window_operand(pkg, W))
        assert plan[0][0].startswith("fasn_kvcache_fwd_window_kernel<") and plan[0][1] > B * Hkv, plan
    else:
        plan = pkg._lib.kvprefill_window_plan(kv_args._args_prefill(pkg, B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages), _window_operand(pkg, W))
        assert [k[0].split("<")[0] for k in plan] == ["fasn_kvprefill_fwd_window_kernel", "fasn_kvprefill_combine_kernel"]
        assert plan[0][1] > B * Hkv * -(-Sq // (128 // (H // Hkv))), plan
    assert _first(lens[0], (qlens or [Sq])[0], W) >= 7 * page                            # whole pages lie below the window: poisoned
    n = _n_values((H,), dev, 200)
    assert (n == 0).any() and (n > 0).any()
    _run(pkg, dev, B, H, Hkv, Sq, D, torch.bfloat16, page, lens, n, [W], seed=201, max_pages=max_pages, what=f"{call} split-K", qlens=qlens)


# ---------------------------------------------------------------- 4. next to the sink: tensor n with zeros, rows that see nothing
@pytest.mark.parametrize("call", ["decode", "prefill"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_with_the_sink(pkg, dev, dtype, call):
    B, H, Hkv, D, page, W = 3, 32, 8, 64, 64, 3
    Sq = 4 if call == "decode" else 70
    lens = [130, 0, 2]
    n = _n_values((H,), dev, 500)
    assert (n == 0).any() and (n > 0).any()
    out, lse, _o, _l = _run(pkg, dev, B, H, Hkv, Sq, D, DTYPES[dtype], page, lens, n, [W], seed=501, what=f"{call} sink {dtype}")
    logn = torch.where(n > 0, torch.log(n), torch.full_like(n, float("-inf")))
    assert (out[1] == 0).all() and torch.allclose(lse[1], logn.view(H, 1).expand(H, Sq), atol=1e-6, rtol=0)   # len 0: nothing to see
    # len 2 < Sq: the first Sq - 2 positions (p_i < 0) see no key either
    assert (out[2, :, :Sq - 2] == 0).all() and torch.allclose(lse[2, :, :Sq - 2], logn.view(H, 1).expand(H, Sq - 2), atol=1e-6, rtol=0)
    assert (out[2, :, Sq - 2:].float().abs().amax(-1) > 0).all()
    keep = min(Sq, lens[0])                                                               # batch element 0: p_i = i + 130 - Sq
    assert (out[0, :, Sq - keep:].float().abs().amax(-1) > 0).all()


# ---------------------------------------------------------------- 5. prefill grid
@pytest.mark.parametrize("Dd", [(64, "bf16"), (128, "fp16")])
@pytest.mark.parametrize("heads", [(64, 8), (16, 16), (12, 4)])
@pytest.mark.parametrize("Sq", [17, 200])
def test_prefill_grid(pkg, dev, Sq, heads, Dd):
    H, Hkv = heads
    D, dtype = Dd
    page = 64
    lens = [0, Sq - 5, page + 1, 2 * page]
    _run(pkg, dev, 4, H, Hkv, Sq, D, DTYPES[dtype], page, lens, 1.0, [1, 16, 64, 100, 300], seed=600 + D + H + Sq, prefill=True,
         what=f"prefill D={D} {dtype} H={H}/{Hkv} Sq={Sq}")


@pytest.mark.parametrize("append", [False, True])
@pytest.mark.parametrize("W", [16, 100])
def test_prefill_ragged_queries(pkg, dev, W, append):
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.bfloat16, 4, 64, 8, 200, 64, 64, 8
    qlens = [Sq, 1, 0, Sq // 2]
    lens = [10, page + 1, 70, 2 * page]                                                 # keys in the cache before the call
    n = _n_values((B, H), dev, 700)
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
    _poison(pc.k, pc.v, pc.table, page, pc.poison, total, qlens, W)
    qs = torch.tensor(qlens, dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache_window(q, pc.k, pc.v, pc.lens, W, block_table=pc.table, k_new=kn if append else None,
                                                    v_new=vn if append else None, query_seqlens=qs, softmax_n_param=n, return_lse=True)
    assert torch.equal(pc.lens.cpu(), torch.tensor(lens, dtype=torch.int32)), "cache_seqlens was modified"
    _check_all(pkg, out, lse, q, ks._visible_dense(kd, total), ks._visible_dense(vd, total), total, qlens, n, W, dtype,
               f"prefill ragged W={W} append={append}")


def test_dense_cache(pkg, dev):
    dtype, B, H, Hkv, Sq, D, cap, W = torch.float16, 3, 16, 4, 150, 128, 200, 20   # (a dense capacity need not be a multiple of 64)
    lens = [200, 77, 0]
    q = _rand((B, H, Sq, D), dtype, dev, 710)
    kc = _rand((B, cap, Hkv, D), dtype, dev, 711)
    vc = _rand((B, cap, Hkv, D), dtype, dev, 712, std=1.0)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    keep = torch.arange(cap, device=dev).view(1, -1, 1, 1) < sl.view(-1, 1, 1, 1)
    kg, vg = (torch.where(keep, t, torch.zeros_like(t)).permute(0, 2, 1, 3).contiguous() for t in (kc, vc))
    q8 = q[:, :, :8].contiguous()
    for b, ln in enumerate(lens):   # rows at or beyond len_b: NaN
        kc[b, ln:] = NAN
        vc[b, ln:] = NAN
    out, lse = pkg.flash_attention_n_kvcache_window(q, kc, vc, sl, W, softmax_n_param=0.5, return_lse=True)
    _check_all(pkg, out, lse, q, kg, vg, lens, [Sq] * B, 0.5, W, dtype, "prefill dense")
    for b, ln in enumerate(lens):   # 8 positions: the window starts later, and the rows below its first tile go too
        first = _first(ln, 8, W)
        kc[b, :first] = NAN
        vc[b, :first] = NAN
    assert _first(lens[0], 8, W) == 128
    d_out, d_lse = pkg.flash_attention_n_kvcache_window(q8, kc, vc, sl, W, softmax_n_param=0.5, return_lse=True)
    _check_all(pkg, d_out, d_lse, q8, kg, vg, lens, [8] * B, 0.5, W, dtype, "decode dense")


# ---------------------------------------------------------------- 6. both dispatch branches give one function
@pytest.mark.parametrize("W", [5, 64, 200])
def test_both_branches_agree(pkg, dev, W):
    dtype, B, H, Hkv, Sq, D, page = torch.bfloat16, 3, 32, 8, 16, 64, 64
    lens = [300, 7, 64]
    q, pc = _case(dev, B, H, Hkv, Sq, D, dtype, page, lens, 800, max_pages=6)
    n = _n_values((H,), dev, 801)
    _poison(pc.k, pc.v, pc.table, page, pc.poison, lens, [Sq] * B, W)
    full = torch.full((B,), Sq, dtype=torch.int32, device=dev)
    d, ld = pkg.flash_attention_n_kvcache_window(q, pc.k, pc.v, pc.lens, W, block_table=pc.table, softmax_n_param=n, return_lse=True)
    a, la = pkg.flash_attention_n_kvcache_window(q, pc.k, pc.v, pc.lens, W, block_table=pc.table, query_seqlens=full, softmax_n_param=n,
                                                 return_lse=True)
    _check(a, d, dtype, "prefill kernels vs decode kernels out")
    _check_lse(la, ld, "prefill kernels vs decode kernels lse")


# ---------------------------------------------------------------- 7. HIP graph: the window's first tile follows the lengths in device memory
# W = 64 on 64-key pages: one split, and the window start crosses a tile and page edge between the replays. The plan has several splits
# only where a window spans 8 tiles (decode) / 32 tiles (prefill) and more, so those two shapes carry the same walk at longer lengths.
REPLAYS = {
    "decode one split": dict(Sq=2, W=64, max_pages=4, prefill=False, steps=([62, 100], [63, 129], [200, 1]), splits=False),
    "decode several splits": dict(Sq=2, W=500, max_pages=40, prefill=False, steps=([700, 1000], [701, 1029], [2000, 1]), splits=True),
    "prefill one split": dict(Sq=150, W=64, max_pages=8, prefill=True, steps=([62, 100], [63, 129], [200, 1]), splits=False),
    "prefill several splits": dict(Sq=32, W=2000, max_pages=64, prefill=True, steps=([2100, 3000], [2101, 3029], [4000, 1]), splits=True),
}


@pytest.mark.parametrize("shape", sorted(REPLAYS))
def test_graph_replay_follows_the_lengths(pkg, dev, shape):
    """One capture; cache_seqlens (and query_seqlens) change in place between replays, the poison is applied again at every step"""
    s = REPLAYS[shape]
    dtype, B, H, Hkv, D, page = torch.bfloat16, 2, 16, 4, 64, 64
    Sq, W, max_pages = s["Sq"], s["W"], s["max_pages"]
    operand = _window_operand(pkg, W)
    if s["prefill"]:
        plan = pkg._lib.kvprefill_window_plan(kv_args._args_prefill(pkg, B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages), operand)
        assert (len(plan) == 2) == s["splits"], plan
    else:
        plan = pkg._lib.kvcache_window_plan(kv_args._args_decode(pkg, B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages), operand)
        assert (plan[0][1] > B * Hkv) == s["splits"], plan
    q = _rand((B, H, Sq, D), dtype, dev, 900)
    n_pages = B * max_pages
    k0 = _rand((n_pages + 1, page, Hkv, D), dtype, dev, 901)
    v0 = _rand((n_pages + 1, page, Hkv, D), dtype, dev, 902, std=1.0)
    k0[n_pages] = NAN   # the poison page
    v0[n_pages] = NAN
    table0 = torch.arange(n_pages, dtype=torch.int32, device=dev).view(B, max_pages).flip(1).contiguous()
    pool_k, pool_v, table = k0.clone(), v0.clone(), table0.clone()
    sl = torch.tensor(s["steps"][0], dtype=torch.int32, device=dev)
    ql = torch.tensor([Sq, Sq // 3], dtype=torch.int32, device=dev) if s["prefill"] else None
    n = _n_values((H,), dev, 903)

    def call(lens_t, qlens_t):
        return pkg.flash_attention_n_kvcache_window(q, pool_k, pool_v, lens_t, W, block_table=table, query_seqlens=qlens_t, softmax_n_param=n,
                                                    return_lse=True)

    g, (go, glse) = _capture(lambda: call(sl, ql))
    seen, firsts = [], []
    for step, lens in enumerate(s["steps"]):
        qlens = ([Sq, Sq // 3], [Sq - 7, 1], [9, Sq])[step] if s["prefill"] else [Sq] * B
        with torch.no_grad():
            pool_k.copy_(k0)
            pool_v.copy_(v0)
            table.copy_(table0)
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
            if ql is not None:
                ql.copy_(torch.tensor(qlens, dtype=torch.int32))
        kg, vg = _gather(pool_k, table, lens, page), _gather(pool_v, table, lens, page)
        _poison(pool_k, pool_v, table, page, n_pages, lens, qlens, W)
        firsts.append([_first(ln, qn, W) for ln, qn in zip(lens, qlens)])
        g.replay()
        torch.cuda.synchronize()
        _check_all(pkg, go, glse, q, kg, vg, lens, qlens, n, W, dtype, f"{shape} replay at {lens} / {qlens}", witness=False)
        eo, el = call(sl.clone(), None if ql is None else ql.clone())
        assert torch.equal(go, eo) and torch.equal(glse, el), f"replay at {lens}: differs from the eager call"
        seen.append(go.clone())
    assert len({tuple(f) for f in firsts}) == 3, firsts                                  # the window start moved between the replays
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---------------------------------------------------------------- 8. a GPT-OSS-shaped step: a sliding layer's decode, then a chunk, both appending
def test_gpt_oss_sliding_layer(pkg, dev):
    dtype, B, H, Hkv, D, page, max_pages, W = torch.bfloat16, 3, 64, 8, 64, 64, 13, 128
    lens = [300, 517, 700]
    sinks = synth.counter_normal((H,), 1100, std=1.0, dtype=torch.float32, device=dev)
    n = torch.exp(sinks)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 1101)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 1102, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, 1103, alloc_all=True)   # rows at or beyond the length: NaN until an append writes them
    for Sq, seed in ((1, 1104), (40, 1105)):                            # one token, then a chunk of 40 positions
        q = _rand((B, H, Sq, D), dtype, dev, seed)
        kn = torch.stack([kd[b, :, lens[b]:lens[b] + Sq] for b in range(B)])
        vn = torch.stack([vd[b, :, lens[b]:lens[b] + Sq] for b in range(B)])
        total = [ln + Sq for ln in lens]
        assert _poison(pc.k, pc.v, pc.table, page, pc.poison, total, [Sq] * B, W) > 0
        sl = torch.tensor(lens, dtype=torch.int32, device=dev)
        out, lse = pkg.flash_attention_n_kvcache_window(q, pc.k, pc.v, sl, W, block_table=pc.table, k_new=kn, v_new=vn, softmax_n_param=n,
                                                        return_lse=True)
        _check_all(pkg, out, lse, q, ks._visible_dense(kd, total), ks._visible_dense(vd, total), total, [Sq] * B, n, W, dtype,
                   f"GPT-OSS sliding layer Sq={Sq}")
        lens = total


# ---------------------------------------------------------------- 9. determinism
@pytest.mark.parametrize("call", ["decode", "prefill one split", "prefill several splits"])
def test_deterministic(pkg, dev, call):
    dtype, H, Hkv, D, page = torch.bfloat16, 64, 8, 64, 256
    if call == "decode":
        B, Sq, max_pages, lens, W = 4, 1, 20, [5000, 1, 4096, 2049], 1000
    elif call == "prefill one split":
        B, Sq, max_pages, lens, W = 4, 300, 9, [2000, 1, 1024, 2049], 128
    else:
        B, Sq, max_pages, lens, W = 1, 64, 20, [5000], 3000
    if call != "decode":
        plan = pkg._lib.kvprefill_window_plan(kv_args._args_prefill(pkg, B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages), _window_operand(pkg, W))
        assert len(plan) == (2 if call == "prefill several splits" else 1)
    q, pc = _case(dev, B, H, Hkv, Sq, D, dtype, page, lens, 1000, max_pages=max_pages)
    n = _n_values((H,), dev, 1001)
    qs = None if call == "decode" else torch.full((B,), Sq, dtype=torch.int32, device=dev)
    a = pkg.flash_attention_n_kvcache_window(q, pc.k, pc.v, pc.lens, W, block_table=pc.table, query_seqlens=qs, softmax_n_param=n, return_lse=True)
    b = pkg.flash_attention_n_kvcache_window(q, pc.k, pc.v, pc.lens, W, block_table=pc.table, query_seqlens=qs, softmax_n_param=n, return_lse=True)
    assert torch.isfinite(a[0]).all() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
