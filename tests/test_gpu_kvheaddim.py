"""flash_attention_n_kvcache and flash_attention_n_kvcache_prefill at head dims 32 and 256, on the GPU.

References, second witness (flash_attention_n on the gathered dense K/V) and gates are those of tests/kv_support.py,
whose helpers and runners the decode, prefill and ALiBi suites use too: REF_ATOL and REL_TRUE on
`out`, 1e-4 x max(1, |lse|) on `lse`. Caches are _Paged: every row at or beyond len_b and every unneeded table entry is NaN, and _check
asserts finite outputs. Shapes are the smallest at which the named thing can go wrong at these head dims: three LDS buffers per operand at
D = 32, two of 32 KiB at D = 256 (the second V buffer ends at 128 KiB), one workgroup per CU at D = 256."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_args   # noqa: E402
import kv_support as ks   # noqa: E402

pytestmark = pytest.mark.gpu

NAN = ks.NAN
_run_case, _Paged, _gather, _visibility, _reference, _n_values, _check, _check_lse, _rand = (
    ks._run_case_decode, ks._Paged, ks._gather, ks._visibility, ks.reference, ks._n_values, ks._check, ks._check_lse, ks._rand)
DIMS = [32, 256]
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _dec_splits(pkg, alibi=False, **shape):
    plan = pkg._lib.kvcache_plan(kv_args._args_decode(pkg, **shape), ks._alibi_operand(pkg) if alibi else None)
    G = shape["H"] // shape["Hkv"]
    assert plan[0][0].startswith("fasn_kvcache_fwd_alibi_kernel<" if alibi else "fasn_kvcache_fwd_kernel<") and f", {shape['D']}>" in plan[0][0]
    assert G * shape["Sq"] <= 128
    return plan[0][1] // (shape["B"] * shape["Hkv"])


def _pre_splits(pkg, alibi=False, **shape):
    plan = pkg._lib.kvprefill_plan(kv_args._args_prefill(pkg, **shape), ks._alibi_operand(pkg) if alibi else None)
    assert plan[0][0].startswith("fasn_kvprefill_fwd_alibi_kernel<" if alibi else "fasn_kvprefill_fwd_kernel<") and f", {shape['D']}>" in plan[0][0]
    PB = 128 // (shape["H"] // shape["Hkv"])
    nsplit = plan[0][1] // (shape["B"] * shape["Hkv"] * -(-shape["Sq"] // PB))
    assert (len(plan) == 2) == (nsplit > 1)
    return nsplit


# ---------------------------------------------------------------- 1. decode grid: the masked and the all-visible tile paths
@pytest.mark.parametrize("Sq", [1, 4])
@pytest.mark.parametrize("heads", [(16, 16), (32, 8), (8, 1)])
@pytest.mark.parametrize("page", [64, 256])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", DIMS)
def test_decode_grid(pkg, dev, D, dtype, page, heads, Sq):
    H, Hkv = heads
    # test_paged_ragged's sets: a multiple of the page, one row into a page, fewer than 64 keys, none at all
    lens = [2 * page, page + 1, 37] if Sq == 1 else [0, 3 * page, 2 * page + 1]
    _run_case(pkg, dev, 3, H, Hkv, Sq, D, DTYPES[dtype], page, lens, 1.0, seed=100 + D + page + H + Sq,
              what=f"D={D} {dtype} page={page} H={H}/{Hkv} Sq={Sq}")


# ---------------------------------------------------------------- 2. every LDS buffer inside one split
@pytest.mark.parametrize("call", ["decode", "prefill"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", DIMS)
def test_all_lds_buffers_within_one_split(pkg, dev, D, dtype, call):
    """5 and 7 tiles walked by ONE workgroup: at D = 32 the three buffers cycle (twice), at D = 256 both 32 KiB buffers of K and of V
    (V's second one at 96 .. 128 KiB) are filled and read more than once"""
    B, H, Hkv, page, max_pages = 2, 8, 2, 64, 7
    lens = [4 * 64 + 1, 7 * 64]
    Sq = 2 if call == "decode" else 40
    shape = dict(B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages)
    if call == "decode":
        assert _dec_splits(pkg, **shape) == 1
        _run_case(pkg, dev, B, H, Hkv, Sq, D, DTYPES[dtype], page, lens, 1.0, seed=200 + D, max_pages=max_pages, what=f"one split D={D} {dtype}")
    else:
        assert _pre_splits(pkg, **shape) == 1
        ks._run_case_prefill(pkg, dev, B, H, Hkv, Sq, D, DTYPES[dtype], page, lens, 1.0, seed=210 + D, max_pages=max_pages, what=f"prefill one split D={D} {dtype}")


# ---------------------------------------------------------------- 3. full and minimal row occupancy
@pytest.mark.parametrize("rows", ["128 rows", "one row"])
@pytest.mark.parametrize("D", DIMS)
def test_row_occupancy(pkg, dev, D, rows):
    H, Hkv, Sq = (8, 1, 16) if rows == "128 rows" else (1, 1, 1)
    _run_case(pkg, dev, 2, H, Hkv, Sq, D, torch.bfloat16, 64, [200, 65], 1.0, seed=300 + D, what=f"{rows} D={D}")


# ---------------------------------------------------------------- 4. softmax_n
@pytest.mark.parametrize("n", [0, 0.5])
@pytest.mark.parametrize("D", DIMS)
def test_scalar_n(pkg, dev, D, n):
    _run_case(pkg, dev, 3, 32, 8, 2, D, torch.bfloat16, 64, [130, 64, 5], n, seed=400 + D, what=f"D={D} n={n}")


@pytest.mark.parametrize("shape", ["H", "BH"])
@pytest.mark.parametrize("D", DIMS)
def test_tensor_n_per_row(pkg, dev, D, shape):
    B, H, Hkv = 3, 32, 8
    n = _n_values({"H": (H,), "BH": (B, H)}[shape], dev, 420)
    assert (n == 0).any() and (n > 0).any()
    out, lse, _, _ = _run_case(pkg, dev, B, H, Hkv, 4, D, torch.float16, 64, [200, 0, 65], n, seed=421 + D, what=f"D={D} n[{shape}]")
    nb = n.reshape((1,) * (2 - n.dim()) + tuple(n.shape)).expand(B, H)
    logn = torch.where(nb[1] > 0, torch.log(nb[1]), torch.full_like(nb[1], float("-inf")))
    assert (out[1] == 0).all() and torch.allclose(lse[1], logn.view(H, 1).expand(H, 4), atol=1e-6, rtol=0)   # len 0: 0 and log n


# ---------------------------------------------------------------- 5. several splits
@pytest.mark.parametrize("D", DIMS)
def test_several_splits(pkg, dev, D):
    B, H, Hkv, Sq, page, max_pages = 2, 16, 2, 1, 256, 40
    nsplit = _dec_splits(pkg, B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages)
    assert nsplit > 1
    cap = page * max_pages
    tiles = cap // 64
    assert -(-tiles // nsplit) * (nsplit - 1) < tiles - 1          # a full cache keeps every split busy, one tile less still does
    _run_case(pkg, dev, B, H, Hkv, Sq, D, torch.bfloat16, page, [cap, cap - 64 - 5], _n_values((H,), dev, 500), seed=501 + D, max_pages=max_pages,
              what=f"D={D} {nsplit} splits, all busy")
    _run_case(pkg, dev, B, H, Hkv, Sq, D, torch.float16, page, [20, 0], 1.0, seed=502 + D, max_pages=max_pages,
              what=f"D={D} {nsplit} splits, most empty")


# ---------------------------------------------------------------- 6. append
@pytest.mark.parametrize("D", DIMS)
def test_append_writes_exactly_the_new_rows(pkg, dev, D):
    dtype, B, H, Hkv, Sq, page, max_pages = torch.bfloat16, 3, 16, 4, 4, 64, 3
    cap = page * max_pages
    lens = [10, page - 2, cap - 1]   # inside a page; across a page boundary; one row of room: three rows dropped
    q = _rand((B, H, Sq, D), dtype, dev, 600)
    kd = _rand((B, Hkv, cap, D), dtype, dev, 601)
    vd = _rand((B, Hkv, cap, D), dtype, dev, 602, std=1.0)
    kn = _rand((B, Hkv, Sq, D), dtype, dev, 603)
    vn = _rand((B, Hkv, Sq, D), dtype, dev, 604, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, 605, alloc_all=True, guard=7.0)
    k0, v0, lens0 = pc.k.clone(), pc.v.clone(), pc.lens.clone()
    out, lse = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, k_new=kn, v_new=vn, softmax_n_param=1.0, return_lse=True)
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
    la = [ln + Sq for ln in lens[:2]]
    kg, vg = _gather(ke, pc.table[:2], la, page), _gather(ve, pc.table[:2], la, page)
    o_ref, lse_ref = _reference(q[:2], kg, vg, _visibility(la, Sq, kg.shape[2], True, dev), 1.0)
    _check(out[:2], o_ref, dtype, f"append D={D} out")
    _check_lse(lse[:2], lse_ref, f"append D={D} lse")


@pytest.mark.parametrize("D", DIMS)
def test_prefill_append_from_nothing(pkg, dev, D):
    """the prefill append (rows i < qlen_b only) through the shuffled table, then attention equal to flash_attention_n(is_causal)"""
    dtype, B, H, Hkv, Sq, page, max_pages = torch.float16, 2, 8, 2, 150, 64, 3
    qlens = [150, 70]
    q = _rand((B, H, Sq, D), dtype, dev, 650)
    kn = _rand((B, Hkv, Sq, D), dtype, dev, 651)
    vn = _rand((B, Hkv, Sq, D), dtype, dev, 652, std=1.0)
    zeros = torch.zeros(B, Hkv, page * max_pages, D, dtype=dtype, device=dev)
    pc = _Paged(zeros, zeros, [0] * B, page, max_pages, 653, alloc_all=True, guard=7.0)
    k0, v0 = pc.k.clone(), pc.v.clone()
    qs = torch.tensor(qlens, dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, k_new=kn, v_new=vn, query_seqlens=qs,
                                                     softmax_n_param=1.0, return_lse=True)
    assert (pc.lens == 0).all(), "cache_seqlens was modified"
    ke, ve = k0.clone(), v0.clone()
    for b in range(B):
        for i in range(qlens[b]):
            pid = int(pc.table[b, i // page])
            ke[pid, i % page] = kn[b, :, i]
            ve[pid, i % page] = vn[b, :, i]
    assert torch.equal(pc.k.view(torch.int16), ke.view(torch.int16)), "k_cache: not exactly the new rows"
    assert torch.equal(pc.v.view(torch.int16), ve.view(torch.int16)), "v_cache: not exactly the new rows"
    assert (pc.k[-1] == 7.0).all() and (pc.v[-1] == 7.0).all(), "guard page behind the cache was written"
    kg, vg = ks._visible_dense(kn, qlens), ks._visible_dense(vn, qlens)
    ks._check_all(pkg, out, lse, q, kg, vg, qlens, qlens, 1.0, True, dtype, f"prefill append D={D}")
    _check(out[:1], pkg.flash_attention_n(q[:1], kn[:1], vn[:1], softmax_n_param=1.0, is_causal=True), dtype, f"prefill append D={D} vs flash_attention_n(is_causal)")


# ---------------------------------------------------------------- 7. dense cache, sliced out of a fused K/V buffer
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("call", ["decode", "prefill"])
@pytest.mark.parametrize("D", DIMS)
def test_dense_cache_in_a_fused_buffer(pkg, dev, D, call, causal):
    dtype, B, H, Hkv, cap = torch.float16, 3, 16, 4, 200   # (a dense capacity need not be a multiple of 64)
    Sq = 2 if call == "decode" else 150
    lens = [200, 77, 0]
    q = _rand((B, H, Sq, D), dtype, dev, 700)
    fused = torch.stack((_rand((B, cap, Hkv, D), dtype, dev, 701), _rand((B, cap, Hkv, D), dtype, dev, 702, std=1.0)), dim=2)   # [B, cap, 2, Hkv, D]
    for b, ln in enumerate(lens):
        fused[b, ln:] = NAN
    kc, vc = fused[:, :, 0], fused[:, :, 1]
    assert not kc.is_contiguous() and kc.stride(1) == 2 * Hkv * D
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    fa = pkg.flash_attention_n_kvcache if call == "decode" else pkg.flash_attention_n_kvcache_prefill
    out, lse = fa(q, kc, vc, sl, softmax_n_param=0.5, is_causal=causal, return_lse=True)
    keep = torch.arange(cap, device=dev).view(1, -1, 1, 1) < sl.view(-1, 1, 1, 1)
    kg, vg = (torch.where(keep, t, torch.zeros_like(t)).permute(0, 2, 1, 3).contiguous() for t in (kc, vc))
    ks._check_all(pkg, out, lse, q, kg, vg, lens, [Sq] * B, 0.5, causal, dtype, f"dense {call} D={D} causal={causal}")


# ---------------------------------------------------------------- 8. ALiBi slopes on both calls
@pytest.mark.parametrize("form", ["H", "BH"])
@pytest.mark.parametrize("call", ["decode", "prefill"])
@pytest.mark.parametrize("D", DIMS)
def test_alibi(pkg, dev, D, call, form):
    B, H, Hkv, page = 3, 16, 4, 64
    Sq = 3 if call == "decode" else 70
    lens = [0, page + 1, 3 * page + 7]
    slopes = ks._slopes(H, dev)
    if form == "BH":
        slopes = (slopes.view(1, H) * torch.tensor([1.0, 0.5, 3.0], device=dev).view(B, 1)).contiguous()
    run = ks._run_alibi_decode if call == "decode" else ks._run_alibi_prefill
    run(pkg, dev, B, H, Hkv, Sq, D, torch.bfloat16, page, lens, _n_values((H,), dev, 800), slopes, seed=801 + D, what=f"alibi {call} D={D} slopes[{form}]")


@pytest.mark.parametrize("call", ["decode", "prefill"])
@pytest.mark.parametrize("D", DIMS)
def test_alibi_weight_in_the_last_split(pkg, dev, D, call):
    """steep slopes: a key 256 positions back is 64 .. 128 nats down, so the result is the last split's - the key index is absolute there"""
    B, H, Hkv, page, max_pages, lens = 1, 16, 2, 256, 20, [5000]
    Sq = 1 if call == "decode" else 64
    shape = dict(B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages)
    nsplit = _dec_splits(pkg, alibi=True, **shape) if call == "decode" else _pre_splits(pkg, alibi=True, **shape)
    assert nsplit > 1
    run = ks._run_alibi_decode if call == "decode" else ks._run_alibi_prefill
    run(pkg, dev, B, H, Hkv, Sq, D, torch.float16, page, lens, 1.0, ks._steep(H, dev), seed=850 + D, max_pages=max_pages, what=f"alibi {call} D={D} steep, {nsplit} splits")


# ---------------------------------------------------------------- 9. prefill
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("heads", [(16, 2), (12, 4)])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", DIMS)
def test_prefill_one_split(pkg, dev, D, dtype, heads, causal):
    """Sq = 300 with G = 8 (16 positions per row block, 19 blocks, the last one partly filled) and G = 3 (126 of 128 slots); ragged query
    lengths with an empty and a full element; padding rows exactly 0 / -inf (asserted by _check_all)"""
    H, Hkv = heads
    B, Sq, page, max_pages = 4, 300, 64, 8
    shape = dict(B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages)
    assert _pre_splits(pkg, **shape) == 1
    assert pkg._lib.load().fasn_fwd_kvprefill_workspace_bytes(kv_args._args_prefill(pkg, **shape)) == 0
    ks._run_case_prefill(pkg, dev, B, H, Hkv, Sq, D, DTYPES[dtype], page, [0, Sq - 5, page + 1, 6 * page], _n_values((B, H), dev, 900), causal=causal,
                  seed=901 + D + H, max_pages=max_pages, qlens=[Sq, 1, 0, 129], what=f"prefill D={D} {dtype} H={H}/{Hkv} causal={causal}")


@pytest.mark.parametrize("D", DIMS)
def test_prefill_several_splits(pkg, dev, D):
    shape = dict(B=1, H=16, Hkv=2, Sq=64, D=D, page=256, max_pages=40)
    assert _pre_splits(pkg, **shape) > 1
    ks._run_case_prefill(pkg, dev, 1, 16, 2, 64, D, torch.bfloat16, 256, [9000], _n_values((16,), dev, 950), seed=951 + D, max_pages=40, what=f"prefill split plan D={D}")
    ks._run_case_prefill(pkg, dev, 1, 16, 2, 64, D, torch.float16, 256, [9000], 0.0, causal=False, seed=952 + D, max_pages=40, what=f"prefill split plan D={D} non-causal", qlens=[33])
    ks._run_case_prefill(pkg, dev, 1, 16, 2, 64, D, torch.float16, 256, [20], 1.0, seed=953 + D, max_pages=40, what=f"prefill split plan D={D}, most splits empty")


# ---------------------------------------------------------------- 10. prompt -> chunked prefill -> two decode steps at D = 256
def test_chain_d256(pkg, dev):
    """on the paged cache alone, with k_new / v_new; every piece against flash_attention_n(is_causal=True) on the whole sequence (the
    D = 64 chain of test_gpu_kvprefill.py at D = 256)"""
    dtype, B, H, Hkv, D, page, max_pages, S, C = torch.bfloat16, 2, 8, 2, 256, 64, 11, 600, 256
    T = S + 2
    q = _rand((B, H, T, D), dtype, dev, 1000)
    k = _rand((B, Hkv, T, D), dtype, dev, 1001)
    v = _rand((B, Hkv, T, D), dtype, dev, 1002, std=1.0)
    n = _n_values((H,), dev, 1003)
    one = pkg.flash_attention_n(q, k, v, softmax_n_param=n, is_causal=True)
    o_ref, lse_ref = _reference(q, k, v, _visibility([T] * B, T, T, True, dev), n)
    _check(one, o_ref, dtype, "flash_attention_n on the whole sequence")
    num_pages = B * max_pages + 1
    pool_k = torch.full((num_pages, page, Hkv, D), NAN, dtype=dtype, device=dev)
    pool_v = torch.full((num_pages, page, Hkv, D), NAN, dtype=dtype, device=dev)
    table = torch.randperm(B * max_pages, generator=torch.Generator().manual_seed(1004)).to(torch.int32).view(B, max_pages).to(dev)
    sl = torch.zeros(B, dtype=torch.int32, device=dev)
    for c0 in range(0, S, C):
        cl = min(C, S - c0)   # the last chunk is padded to C positions and carries its length in query_seqlens
        qc, kc, vc = (torch.full((B, t.shape[1], C, D), NAN, dtype=dtype, device=dev) for t in (q, k, v))
        qc[:, :, :cl], kc[:, :, :cl], vc[:, :, :cl] = q[:, :, c0:c0 + cl], k[:, :, c0:c0 + cl], v[:, :, c0:c0 + cl]
        ql = torch.full((B,), cl, dtype=torch.int32, device=dev)
        out, lse = pkg.flash_attention_n_kvcache_prefill(qc, pool_k, pool_v, sl, block_table=table, k_new=kc, v_new=vc, query_seqlens=ql,
                                                         softmax_n_param=n, return_lse=True)
        sl += ql   # advanced on the device
        _check(out[:, :, :cl], one[:, :, c0:c0 + cl], dtype, f"chunk at {c0} vs flash_attention_n")
        _check(out[:, :, :cl], o_ref[:, :, c0:c0 + cl], dtype, f"chunk at {c0} out")
        _check_lse(lse[:, :, :cl], lse_ref[:, :, c0:c0 + cl], f"chunk at {c0} lse")
        assert (out[:, :, cl:] == 0).all() and (lse[:, :, cl:] == float("-inf")).all()
    assert sl.tolist() == [S] * B
    for t in (S, S + 1):
        out1, lse1 = pkg.flash_attention_n_kvcache(q[:, :, t:t + 1].contiguous(), pool_k, pool_v, sl, block_table=table, k_new=k[:, :, t:t + 1].contiguous(),
                                                   v_new=v[:, :, t:t + 1].contiguous(), softmax_n_param=n, return_lse=True)
        sl += 1
        _check(out1, one[:, :, t:t + 1], dtype, f"decode step at {t} vs flash_attention_n")
        _check(out1, o_ref[:, :, t:t + 1], dtype, f"decode step at {t} out")
        _check_lse(lse1, lse_ref[:, :, t:t + 1], f"decode step at {t} lse")
    assert sl.tolist() == [T] * B


# ---------------------------------------------------------------- 11. one graph replay per call at D = 256
@pytest.mark.parametrize("call", ["decode", "prefill"])
def test_graph_replay_d256(pkg, dev, call):
    """captured once; cache_seqlens and query change in place; the replay gives the bits of the eager call at the new lengths"""
    dtype, B, H, Hkv, D, page, max_pages = torch.bfloat16, 2, 8, 2, 256, 64, 6
    Sq = 1 if call == "decode" else 70
    fa = pkg.flash_attention_n_kvcache if call == "decode" else pkg.flash_attention_n_kvcache_prefill
    lens = [62, 100]
    q = _rand((B, H, Sq, D), dtype, dev, 1100)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 1101)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 1102, std=1.0)
    pc = _Paged(kd, vd, [page * max_pages] * B, page, max_pages, 1103)   # every row holds data: the lengths decide what is seen
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    n = _n_values((H,), dev, 1104)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fa(q, pc.k, pc.v, sl, block_table=pc.table, softmax_n_param=n, return_lse=True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        go, glse = fa(q, pc.k, pc.v, sl, block_table=pc.table, softmax_n_param=n, return_lse=True)
    with torch.no_grad():
        q.copy_(_rand((B, H, Sq, D), dtype, dev, 1110))
        sl.copy_(torch.tensor([257, 0], dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    eo, else_ = fa(q.clone(), pc.k, pc.v, sl.clone(), block_table=pc.table, softmax_n_param=n, return_lse=True)
    assert torch.equal(go, eo) and torch.equal(glse, else_), "replay differs from the eager call at the new lengths"
    new = [257, 0]
    kg, vg = _gather(pc.k, pc.table, new, page), _gather(pc.v, pc.table, new, page)
    o_ref, lse_ref = _reference(q, kg, vg, _visibility(new, Sq, kg.shape[2], True, dev), n)
    _check(go, o_ref, dtype, f"graph replay {call} out")
    _check_lse(glse, lse_ref, f"graph replay {call} lse")
