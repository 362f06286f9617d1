"""flash_attention_n_kvcache_prefill on the GPU: any number of query positions over a paged / dense K/V cache, cache lengths and query
lengths in device memory, row blocks of (query heads of a K/V head) x positions, append, both launch plans, graph replay.

Reference, gates and second witness are those of tests/kv_support.py: the visible rows gathered through
the table, visibility as a boolean mask, fp32 torch with the explicit sink column; REF_ATOL / REL_TRUE on `out`, the 1e-4-scaled gate on
`lse`; flash_attention_n with that mask as the witness. With `query_seqlens` the reference is computed per batch element on
q[b, :, :qlen_b]; padding positions must be exactly 0 / -inf."""
import math
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
_rand, _check, _check_lse, _visibility, _reference, _Paged, _gather, _n_values = (
    ks._rand, ks._check, ks._check_lse, ks._visibility, ks.reference, ks._Paged, ks._gather, ks._n_values)
_visible_dense, _check_all, _run_case, _plan_names, _poke_rows = ks._visible_dense, ks._check_all, ks._run_case_prefill, ks._plan_names, ks._poke_rows


# ---------------------------------------------------------------- 1. parity grid
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Sq", [17, 200, 1024])
@pytest.mark.parametrize("heads", [(16, 16), (32, 8), (64, 8), (8, 1), (12, 4)])
@pytest.mark.parametrize("page", [64, 256])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("D", [64, 128])
def test_parity_grid(pkg, dev, D, dtype, page, heads, Sq, causal):
    H, Hkv = heads
    # none at all; fewer than Sq (causal: the first positions see nothing); one row into a page; an exact multiple of the page
    lens = [0, Sq - 5, page + 1, 2 * page]
    _run_case(pkg, dev, 4, H, Hkv, Sq, D, dtype, page, lens, 1.0, causal=causal, seed=100 + D + page + H + Sq,
              what=f"D={D} {dtype} page={page} H={H}/{Hkv} Sq={Sq} causal={causal}")


def test_first_shape_the_decode_call_refuses(pkg, dev):
    with pytest.raises(ValueError, match="rows exceed"):
        pkg.flash_attention_n_kvcache(torch.zeros(1, 64, 17, 64, dtype=torch.bfloat16, device=dev), torch.zeros(2, 64, 8, 64, dtype=torch.bfloat16, device=dev),
                                      torch.zeros(2, 64, 8, 64, dtype=torch.bfloat16, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                                      block_table=torch.zeros(1, 2, dtype=torch.int32, device=dev))
    _run_case(pkg, dev, 2, 64, 8, 17, 64, torch.bfloat16, 64, [100, 17], _n_values((64,), dev, 150), seed=151, what="G=8 Sq=17")


def test_dense_cache(pkg, dev):
    dtype, B, H, Hkv, Sq, D, cap = torch.float16, 3, 16, 4, 150, 128, 200   # (a dense capacity need not be a multiple of 64)
    lens = [200, 77, 0]
    q = _rand((B, H, Sq, D), dtype, dev, 160)
    kc = _rand((B, cap, Hkv, D), dtype, dev, 161)
    vc = _rand((B, cap, Hkv, D), dtype, dev, 162, std=1.0)
    for b, ln in enumerate(lens):
        kc[b, ln:] = NAN
        vc[b, ln:] = NAN
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache_prefill(q, kc, vc, sl, softmax_n_param=0.5, return_lse=True)
    keep = torch.arange(cap, device=dev).view(1, -1, 1, 1) < sl.view(-1, 1, 1, 1)
    kg, vg = (torch.where(keep, t, torch.zeros_like(t)).permute(0, 2, 1, 3).contiguous() for t in (kc, vc))
    _check_all(pkg, out, lse, q, kg, vg, lens, [Sq] * B, 0.5, True, dtype, "dense")


# ---------------------------------------------------------------- 2. ragged queries, with and without an append
@pytest.mark.parametrize("append", [False, True])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("heads", [(64, 8), (16, 16)])
def test_ragged_queries(pkg, dev, heads, causal, append):
    H, Hkv = heads
    dtype, B, Sq, D, page, max_pages = torch.bfloat16, 4, 200, 64, 64, 8
    PB = 128 // (H // Hkv)
    qlens = [Sq, 1, 0, 6 * PB + PB // 2 if 6 * PB + PB // 2 < Sq else PB + PB // 2]   # all, one, none, one that ends inside a row block
    assert qlens[3] % PB != 0 and 0 < qlens[3] < Sq
    lens = [10, page + 1, 70, 2 * page]                                                 # keys in the cache before the call
    n = _n_values((B, H), dev, 200)
    q = _rand((B, H, Sq, D), dtype, dev, 201)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 202)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 203, std=1.0)
    kn = _rand((B, Hkv, Sq, D), dtype, dev, 204)
    vn = _rand((B, Hkv, Sq, D), dtype, dev, 205, std=1.0)
    total = [ln + (ql if append else 0) for ln, ql in zip(lens, qlens)]
    if append:   # the dense picture of the cache after the append
        for b in range(B):
            kd[b, :, lens[b]:total[b]] = kn[b, :, :qlens[b]]
            vd[b, :, lens[b]:total[b]] = vn[b, :, :qlens[b]]
    pc = _Paged(kd, vd, lens, page, max_pages, 206, alloc_all=True)   # rows at or beyond the OLD length: NaN until the append writes them
    qs = torch.tensor(qlens, dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, k_new=kn if append else None,
                                                     v_new=vn if append else None, query_seqlens=qs, softmax_n_param=n, is_causal=causal, return_lse=True)
    assert torch.equal(pc.lens.cpu(), torch.tensor(lens, dtype=torch.int32)), "cache_seqlens was modified"
    _check_all(pkg, out, lse, q, _visible_dense(kd, total), _visible_dense(vd, total), total, qlens, n, causal, dtype,
               f"ragged H={H}/{Hkv} causal={causal} append={append}")


# ---------------------------------------------------------------- 3. prefill from nothing; the append writes exactly the new rows
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_from_nothing(pkg, dev, D):
    dtype, B, H, Hkv, Sq, page, max_pages = torch.bfloat16, 3, 32, 8, 300, 64, 5
    q = _rand((B, H, Sq, D), dtype, dev, 300)
    kn = _rand((B, Hkv, Sq, D), dtype, dev, 301)
    vn = _rand((B, Hkv, Sq, D), dtype, dev, 302, std=1.0)
    zeros = torch.zeros(B, Hkv, page * max_pages, D, dtype=dtype, device=dev)
    pc = _Paged(zeros, zeros, [0] * B, page, max_pages, 303, alloc_all=True, guard=7.0)
    k0, v0 = pc.k.clone(), pc.v.clone()
    n = _n_values((H,), dev, 304)
    out, lse = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, k_new=kn, v_new=vn, softmax_n_param=n, return_lse=True)
    _check(out, pkg.flash_attention_n(q, kn, vn, softmax_n_param=n, is_causal=True), dtype, "from nothing vs flash_attention_n(is_causal)")
    _check_all(pkg, out, lse, q, kn, vn, [Sq] * B, [Sq] * B, n, True, dtype, "from nothing")
    ke, ve = k0.clone(), v0.clone()
    for b in range(B):
        for s in range(max_pages):
            rows = max(0, min(page, Sq - s * page))
            pid = int(pc.table[b, s])
            ke[pid, :rows] = kn[b, :, s * page:s * page + rows].transpose(0, 1)
            ve[pid, :rows] = vn[b, :, s * page:s * page + rows].transpose(0, 1)
    assert torch.equal(pc.k.view(torch.int16), ke.view(torch.int16)), "k_cache: not exactly the new rows"
    assert torch.equal(pc.v.view(torch.int16), ve.view(torch.int16)), "v_cache: not exactly the new rows"
    assert (pc.k[-1] == 7.0).all() and (pc.v[-1] == 7.0).all(), "guard page behind the cache was written"


def test_append_drops_rows_at_the_capacity_and_beyond_qlen(pkg, dev):
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.float16, 3, 16, 4, 50, 64, 64, 3
    cap = page * max_pages
    lens = [cap - 10, page - 2, 0]      # ten rows of room: forty dropped; across a page boundary; an empty element
    qlens = [50, 20, 0]                 # rows 20 .. 49 of element 1 and every row of element 2 are padding
    q = _rand((B, H, Sq, D), dtype, dev, 310)
    kd = _rand((B, Hkv, cap, D), dtype, dev, 311)
    vd = _rand((B, Hkv, cap, D), dtype, dev, 312, std=1.0)
    kn = _rand((B, Hkv, Sq, D), dtype, dev, 313)
    vn = _rand((B, Hkv, Sq, D), dtype, dev, 314, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, 315, alloc_all=True, guard=7.0)
    k0, v0, lens0 = pc.k.clone(), pc.v.clone(), pc.lens.clone()
    qs = torch.tensor(qlens, dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, k_new=kn, v_new=vn, query_seqlens=qs,
                                                     softmax_n_param=1.0, return_lse=True)
    assert torch.equal(pc.lens, lens0), "cache_seqlens was modified"
    ke, ve = k0.clone(), v0.clone()
    for b in range(B):
        for i in range(qlens[b]):
            pos = lens[b] + i
            if pos < cap:
                pid = int(pc.table[b, pos // page])
                ke[pid, pos % page] = kn[b, :, i]
                ve[pid, pos % page] = vn[b, :, i]
    assert torch.equal(pc.k.view(torch.int16), ke.view(torch.int16)), "k_cache: not exactly the new rows"
    assert torch.equal(pc.v.view(torch.int16), ve.view(torch.int16)), "v_cache: not exactly the new rows"
    assert (pc.k[-1] == 7.0).all() and (pc.v[-1] == 7.0).all(), "guard page behind the cache was written"
    # elements 1 and 2 against the reference (element 0 lost its newest keys: its length is clamped, only finiteness is checked)
    assert torch.isfinite(out).all()
    total = [lens[1] + qlens[1], 0]
    kg, vg = _gather(ke, pc.table[1:], total, page), _gather(ve, pc.table[1:], total, page)
    _check_all(pkg, out[1:], lse[1:], q[1:], kg, vg, total, qlens[1:], 1.0, True, dtype, "append with query lengths")


# ---------------------------------------------------------------- 4. chunked prefill equals one shot, then a decode step
def test_chunked_equals_one_shot_then_decode(pkg, dev):
    dtype, B, H, Hkv, D, page, max_pages, S, C = torch.bfloat16, 2, 32, 8, 64, 64, 17, 1000, 256
    q = _rand((B, H, S + 1, D), dtype, dev, 400)
    k = _rand((B, Hkv, S + 1, D), dtype, dev, 401)
    v = _rand((B, Hkv, S + 1, D), dtype, dev, 402, std=1.0)
    n = _n_values((H,), dev, 403)
    one = pkg.flash_attention_n(q[:, :, :S].contiguous(), k[:, :, :S].contiguous(), v[:, :, :S].contiguous(), softmax_n_param=n, is_causal=True)
    o_ref, lse_ref = _reference(q[:, :, :S], k[:, :, :S], v[:, :, :S], _visibility([S] * B, S, S, True, dev), n)
    num_pages = B * max_pages + 1
    pool_k = torch.full((num_pages, page, Hkv, D), NAN, dtype=dtype, device=dev)
    pool_v = torch.full((num_pages, page, Hkv, D), NAN, dtype=dtype, device=dev)
    table = torch.randperm(B * max_pages, generator=torch.Generator().manual_seed(404)).to(torch.int32).view(B, max_pages).to(dev)
    sl = torch.zeros(B, dtype=torch.int32, device=dev)
    for c0 in range(0, S, C):
        cl = min(C, S - c0)   # the last chunk is padded to C positions and carries its length in query_seqlens
        qc, kc, vc = (torch.full((B, t.shape[1], C, D), NAN, dtype=dtype, device=dev) for t in (q, k, v))
        qc[:, :, :cl], kc[:, :, :cl], vc[:, :, :cl] = q[:, :, c0:c0 + cl], k[:, :, c0:c0 + cl], v[:, :, c0:c0 + cl]
        ql = torch.full((B,), cl, dtype=torch.int32, device=dev)
        out, lse = pkg.flash_attention_n_kvcache_prefill(qc, pool_k, pool_v, sl, block_table=table, k_new=kc, v_new=vc, query_seqlens=ql,
                                                         softmax_n_param=n, return_lse=True)
        sl += ql   # advanced on the device
        _check(out[:, :, :cl], one[:, :, c0:c0 + cl], dtype, f"chunk at {c0} vs one-shot flash_attention_n")
        _check(out[:, :, :cl], o_ref[:, :, c0:c0 + cl], dtype, f"chunk at {c0} out")
        _check_lse(lse[:, :, :cl], lse_ref[:, :, c0:c0 + cl], f"chunk at {c0} lse")
        assert (out[:, :, cl:] == 0).all() and (lse[:, :, cl:] == float("-inf")).all()
    assert sl.tolist() == [S] * B
    # one decode step over the cache the chunks built
    out1, lse1 = pkg.flash_attention_n_kvcache(q[:, :, S:].contiguous(), pool_k, pool_v, sl, block_table=table, k_new=k[:, :, S:].contiguous(),
                                               v_new=v[:, :, S:].contiguous(), softmax_n_param=n, return_lse=True)
    o1, l1 = _reference(q[:, :, S:], k, v, _visibility([S + 1] * B, 1, S + 1, True, dev), n)
    _check(out1, o1, dtype, "decode after chunked prefill out")
    _check_lse(lse1, l1, "decode after chunked prefill lse")


# ---------------------------------------------------------------- 5. softmax_n
@pytest.mark.parametrize("n", [0, 0.5, 1])
def test_scalar_n(pkg, dev, n):
    _run_case(pkg, dev, 3, 32, 8, 150, 64, torch.bfloat16, 64, [130, 64, 5], n, seed=500, what=f"n={n}", qlens=[150, 70, 150])


@pytest.mark.parametrize("shape", ["H", "BH"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_tensor_n_per_row(pkg, dev, shape, dtype):
    B, H, Hkv = 3, 32, 8
    n = _n_values({"H": (H,), "BH": (B, H)}[shape], dev, 510)
    assert (n == 0).any() and (n > 0).any()
    _run_case(pkg, dev, B, H, Hkv, 100, 128, dtype, 64, [200, 3, 65], n, seed=511, what=f"n[{shape}] {dtype}")


def test_gpt_oss_prefill(pkg, dev):
    dtype, B, H, Hkv, Sq, D, page = torch.bfloat16, 4, 64, 8, 300, 64, 256
    n = torch.exp(synth.counter_normal((H,), 520, std=1.0, dtype=torch.float32, device=dev))
    out, _ = _run_case(pkg, dev, B, H, Hkv, Sq, D, dtype, page, [3117, 2048, 300, 4000], n, seed=521, max_pages=17, what="GPT-OSS prefill",
                       qlens=[300, 128, 300, 77])
    assert math.isfinite(out.float().abs().max().item())


# ---------------------------------------------------------------- 6. agreement with the decode call where both apply
@pytest.mark.parametrize("causal", [True, False])
def test_agrees_with_decode(pkg, dev, causal):
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.bfloat16, 3, 32, 8, 16, 64, 64, 6
    lens = [300, 7, 64]
    q = _rand((B, H, Sq, D), dtype, dev, 600)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 601)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 602, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, 603)
    n = _n_values((H,), dev, 604)
    a, la = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, is_causal=causal, return_lse=True)
    d, ld = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, is_causal=causal, return_lse=True)
    _check(a, d, dtype, "prefill vs decode out")
    _check_lse(la, ld, "prefill vs decode lse")


# ---------------------------------------------------------------- 7. poison
@pytest.mark.parametrize("shape", ["one split", "several splits"])
def test_poison_never_reaches_the_result(pkg, dev, shape):
    """NaN in every cache row at or beyond len_b, in the poison page behind every unneeded table entry, and in the q / k_new / v_new rows
    >= qlen_b: finite output, the bits of the clean run."""
    dtype, H, Hkv, D, page = torch.bfloat16, 16, 2, 64, 256
    if shape == "one split":
        B, Sq, max_pages, lens, qlens = 3, 600, 6, [700, 3, 256], [600, 250, 0]
    else:
        B, Sq, max_pages, lens, qlens = 1, 64, 40, [5000], [37]
    assert ("fasn_kvprefill_combine_kernel" in _plan_names(pkg, B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages)) == (shape == "several splits")
    total = [ln + ql for ln, ql in zip(lens, qlens)]
    q = _rand((B, H, Sq, D), dtype, dev, 700)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 701)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 702, std=1.0)
    kn = _rand((B, Hkv, Sq, D), dtype, dev, 703)
    vn = _rand((B, Hkv, Sq, D), dtype, dev, 704, std=1.0)
    pc = _Paged(kd, vd, total, page, max_pages, 705)          # pages for the keys after the append; behind them the poison page
    assert (pc.table == pc.poison).any() and torch.isnan(pc.k[pc.poison]).all()
    for b in range(B):
        _poke_rows(pc, b, lens[b], total[b], NAN)             # the rows the append is to write: NaN until then
        q[b, :, qlens[b]:] = NAN
        kn[b, :, qlens[b]:] = NAN
        vn[b, :, qlens[b]:] = NAN
    qs = torch.tensor(qlens, dtype=torch.int32, device=dev)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    n = _n_values((H,), dev, 706)
    clean = [torch.nan_to_num(t, nan=0.37) for t in (q, pc.k, pc.v, kn, vn)]
    out, lse = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, sl, block_table=pc.table, k_new=kn, v_new=vn, query_seqlens=qs, softmax_n_param=n, return_lse=True)
    assert torch.isfinite(out).all() and not torch.isnan(lse).any()
    co, cl = pkg.flash_attention_n_kvcache_prefill(clean[0], clean[1], clean[2], sl, block_table=pc.table, k_new=clean[3], v_new=clean[4], query_seqlens=qs,
                                                   softmax_n_param=n, return_lse=True)
    assert torch.equal(out, co) and torch.equal(lse, cl), "poison changed the result"
    for b in range(B):   # against the reference too
        kd[b, :, lens[b]:total[b]] = torch.nan_to_num(kn[b, :, :qlens[b]])
        vd[b, :, lens[b]:total[b]] = torch.nan_to_num(vn[b, :, :qlens[b]])
    _check_all(pkg, out, lse, torch.nan_to_num(q), _visible_dense(kd, total), _visible_dense(vd, total), total, qlens, n, True, dtype, f"poison, {shape}")


# ---------------------------------------------------------------- 8. both plans
@pytest.mark.parametrize("D", [64, 128])
def test_plan_with_a_combine_kernel(pkg, dev, D):
    """small batch, long cache: the row blocks do not fill the chip, the keys are split and merged"""
    shape = dict(B=1, H=16, Hkv=2, Sq=64, D=D, page=256, max_pages=40)
    assert _plan_names(pkg, **shape) == ["fasn_kvprefill_fwd_kernel", "fasn_kvprefill_combine_kernel"]
    _run_case(pkg, dev, 1, 16, 2, 64, D, torch.bfloat16, 256, [9000], _n_values((16,), dev, 800), seed=801, max_pages=40, what=f"split plan D={D}")
    _run_case(pkg, dev, 1, 16, 2, 64, D, torch.float16, 256, [9000], 0.0, causal=False, seed=802, max_pages=40, what=f"split plan D={D} non-causal", qlens=[33])
    _run_case(pkg, dev, 1, 16, 2, 64, D, torch.float16, 256, [20], 1.0, seed=803, max_pages=40, what=f"split plan D={D}, most splits empty")


@pytest.mark.parametrize("D", [64, 128])
def test_plan_without_a_combine_kernel(pkg, dev, D):
    """many row blocks: one split, the forward kernel stores o / lse itself, no workspace"""
    shape = dict(B=2, H=64, Hkv=8, Sq=1024, D=D, page=256, max_pages=9)
    assert _plan_names(pkg, **shape) == ["fasn_kvprefill_fwd_kernel"]
    assert pkg._lib.load().fasn_fwd_kvprefill_workspace_bytes(kv_args._args_prefill(pkg, **shape)) == 0
    _run_case(pkg, dev, 2, 64, 8, 1024, D, torch.bfloat16, 256, [2048, 1025], _n_values((64,), dev, 810), seed=811, max_pages=9, what=f"one-split plan D={D}")


# ---------------------------------------------------------------- 9. determinism
@pytest.mark.parametrize("shape", [dict(B=1, Sq=64, max_pages=40, lens=[9000]), dict(B=4, Sq=700, max_pages=20, lens=[5000, 1, 4096, 2049])])
def test_deterministic(pkg, dev, shape):
    dtype, H, Hkv, D, page = torch.bfloat16, 64, 8, 64, 256
    B, Sq, max_pages, lens = shape["B"], shape["Sq"], shape["max_pages"], shape["lens"]
    q = _rand((B, H, Sq, D), dtype, dev, 900)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 901)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 902, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, 903)
    n = _n_values((H,), dev, 904)
    a = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, return_lse=True)
    b = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, return_lse=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------- 10. clamping
def test_lengths_beyond_their_limits_are_clamped(pkg, dev):
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.float16, 2, 16, 4, 40, 64, 64, 2
    cap = page * max_pages
    q = _rand((B, H, Sq, D), dtype, dev, 1000)
    kd = _rand((B, Hkv, cap, D), dtype, dev, 1001)
    vd = _rand((B, Hkv, cap, D), dtype, dev, 1002, std=1.0)
    pc = _Paged(kd, vd, [cap, cap], page, max_pages, 1003)
    over = torch.tensor([cap + 1000, cap], dtype=torch.int32, device=dev)
    qover = torch.tensor([Sq + 9, -3], dtype=torch.int32, device=dev)     # clamp(., 0, Sq): all positions / none
    qexact = torch.tensor([Sq, 0], dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, over, block_table=pc.table, query_seqlens=qover, softmax_n_param=1.0, return_lse=True)
    want, wlse = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, query_seqlens=qexact, softmax_n_param=1.0, return_lse=True)
    assert torch.equal(out, want) and torch.equal(lse, wlse)
    _check_all(pkg, out, lse, q, kd, vd, [cap, cap], [Sq, 0], 1.0, True, dtype, "clamped lengths")


# ---------------------------------------------------------------- 11. strided inputs
def test_strided_views(pkg, dev):
    """the cache as views of a fused K/V buffer, the query as a [B, Sq, H, D] tensor seen as [B, H, Sq, D]: no copies, the same bits"""
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.bfloat16, 2, 16, 4, 90, 64, 64, 3
    lens = [129, 64]
    qb = _rand((B, Sq, H, D), dtype, dev, 1100)
    q = qb.transpose(1, 2)
    assert not q.is_contiguous()
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 1101)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 1102, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, 1103)
    fused = torch.stack((pc.k, pc.v), dim=2)           # [num_pages, page, 2, Hkv, D]
    kv, vv = fused[:, :, 0], fused[:, :, 1]
    assert not kv.is_contiguous() and kv.stride(1) == 2 * Hkv * D
    out, lse = pkg.flash_attention_n_kvcache_prefill(q, kv, vv, pc.lens, block_table=pc.table, softmax_n_param=1.0, scale=0.2, return_lse=True)
    want = pkg.flash_attention_n_kvcache_prefill(q.contiguous(), pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=1.0, scale=0.2)
    assert torch.equal(out, want)
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)
    _check_all(pkg, out, lse, q.contiguous(), kg, vg, lens, [Sq] * B, 1.0, True, dtype, "strided views", scale=0.2)


# ---------------------------------------------------------------- 12. HIP graph
@pytest.mark.parametrize("shape", [dict(B=2, Sq=150, max_pages=8), dict(B=1, Sq=32, max_pages=40)])
def test_graph_replay_follows_lengths_table_cache_and_query(pkg, dev, shape):
    """One capture (append + forward; linear, one stream), three replays after query, k_new, v_new, cache_seqlens, query_seqlens and one
    block-table row changed in place: the bits of an eager call on cloned inputs. Both plans."""
    dtype, H, Hkv, D, page = torch.bfloat16, 16, 4, 64, 64
    B, Sq, max_pages = shape["B"], shape["Sq"], shape["max_pages"]
    cap = page * max_pages
    q = _rand((B, H, Sq, D), dtype, dev, 1200)
    kn = _rand((B, Hkv, Sq, D), dtype, dev, 1201)
    vn = _rand((B, Hkv, Sq, D), dtype, dev, 1202, std=1.0)
    num_pages = (B + 2) * max_pages
    pool_k = _rand((num_pages, page, Hkv, D), dtype, dev, 1203)
    pool_v = _rand((num_pages, page, Hkv, D), dtype, dev, 1204, std=1.0)
    table = torch.arange(B * max_pages, dtype=torch.int32, device=dev).view(B, max_pages).flip(1).contiguous()
    sl = torch.tensor([62, 100][:B], dtype=torch.int32, device=dev)
    ql = torch.tensor([Sq, Sq // 3][:B], dtype=torch.int32, device=dev)
    n = _n_values((H,), dev, 1205)

    def call(q_, pk, pv, sl_, tab, kn_, vn_, ql_, n_):
        return pkg.flash_attention_n_kvcache_prefill(q_, pk, pv, sl_, block_table=tab, k_new=kn_, v_new=vn_, query_seqlens=ql_, softmax_n_param=n_, return_lse=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            call(q, pool_k, pool_v, sl, table, kn, vn, ql, n)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        go, glse = call(q, pool_k, pool_v, sl, table, kn, vn, ql, n)
    for step in range(3):
        with torch.no_grad():
            q.copy_(_rand((B, H, Sq, D), dtype, dev, 1210 + step))
            kn.copy_(_rand((B, Hkv, Sq, D), dtype, dev, 1220 + step))
            vn.copy_(_rand((B, Hkv, Sq, D), dtype, dev, 1230 + step, std=1.0))
            sl += 37
            ql.copy_(torch.tensor([Sq - 7 * step, 1 + 5 * step][:B], dtype=torch.int32))
            table[0] = torch.arange(B * max_pages + step * max_pages // 2, B * max_pages + step * max_pages // 2 + max_pages, dtype=torch.int32, device=dev)
        ck, cv, csl, ctab = pool_k.clone(), pool_v.clone(), sl.clone(), table.clone()
        g.replay()
        torch.cuda.synchronize()
        eo, else_ = call(q.clone(), ck, cv, csl, ctab, kn.clone(), vn.clone(), ql.clone(), n.clone())
        assert torch.equal(go, eo) and torch.equal(glse, else_), f"replay {step}: output differs from the eager call"
        assert torch.equal(pool_k, ck) and torch.equal(pool_v, cv), f"replay {step}: cache differs from the eager call's"
        assert torch.isfinite(go).all()
    assert cap > int(sl.max()) + Sq
