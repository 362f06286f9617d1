"""flash_attention_n_kvcache_varlen on the GPU: the prefill call on token-packed queries - one [T, H, D] buffer, cu_seqlens_q in device
memory, an item table built on the device so that the grid follows the tokens.

Reference and gates are those of tests/kv_support.py: per sequence, fp32
torch on the rows gathered through the table with the explicit sink column; REF_ATOL / REL_TRUE on `out`, the 1e-4-scaled gate on `lse`.
Second witness: flash_attention_n_kvcache_prefill on the same cache with the queries padded and query_seqlens = qlens, under the same
gates. The rows of the buffer at or beyond cu[B] hold NaN on the way in and are not looked at on the way out."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_support as ks   # noqa: E402

pytestmark = pytest.mark.gpu

NAN = ks.NAN
_rand, _check, _check_lse, _visibility, _reference, _Paged, _gather, _n_values = (
    ks._rand, ks._check, ks._check_lse, ks._visibility, ks.reference, ks._Paged, ks._gather, ks._n_values)
_cu, _plan, _nsplit, SPLIT, _split_plan = ks._cu, ks._varlen_plan, ks._varlen_nsplit, ks.VARLEN_SPLIT, ks._varlen_split_plan


def _packed_reference(q, qlens, kg, vg, lens, n, causal):
    """per sequence on its own tokens: (o [sum qlens, H, D], lse [H, sum qlens]) in fp32"""
    H = q.shape[1]
    dev = q.device
    nt = torch.as_tensor(n, dtype=torch.float32, device=dev)
    nb = nt.reshape((1,) * (2 - nt.dim()) + tuple(nt.shape)).expand(len(qlens), H)
    os_, ls, t0 = [], [], 0
    for b, ql in enumerate(qlens):
        if ql:
            qb = q[t0:t0 + ql].transpose(0, 1).unsqueeze(0)                     # [1, H, ql, D]
            ob, lb = _reference(qb, kg[b:b + 1], vg[b:b + 1], _visibility([lens[b]], ql, kg.shape[2], causal, dev), nb[b:b + 1])
            os_.append(ob[0].transpose(0, 1))
            ls.append(lb[0])
        t0 += ql
    return torch.cat(os_, 0), torch.cat(ls, 1)


def _padded_witness(pkg, q, qlens, k, v, sl, table, n, causal):
    """the route the packed call replaces: pad, flash_attention_n_kvcache_prefill with query_seqlens, gather"""
    B, Sq = len(qlens), max(max(qlens), 1)
    qp = torch.zeros(B, q.shape[1], Sq, q.shape[2], dtype=q.dtype, device=q.device)
    t0 = 0
    for b, ql in enumerate(qlens):
        qp[b, :, :ql] = q[t0:t0 + ql].transpose(0, 1)
        t0 += ql
    qs = torch.tensor(qlens, dtype=torch.int32, device=q.device)
    o, lse = pkg.flash_attention_n_kvcache_prefill(qp, k, v, sl, block_table=table, query_seqlens=qs, softmax_n_param=n, is_causal=causal, return_lse=True)
    return (torch.cat([o[b, :, :ql].transpose(0, 1) for b, ql in enumerate(qlens)], 0), torch.cat([lse[b, :, :ql] for b, ql in enumerate(qlens)], 1))


def _check_packed(pkg, out, lse, q, qlens, k, v, table, page, lens, n, causal, dtype, what):
    used = sum(qlens)
    assert out.shape == q.shape and lse.shape == (q.shape[1], q.shape[0])
    kg, vg = _gather(k, table, lens, page), _gather(v, table, lens, page)
    o_ref, lse_ref = _packed_reference(q, qlens, kg, vg, lens, n, causal)
    _check(out[:used], o_ref, dtype, f"{what} out")
    _check_lse(lse[:, :used], lse_ref, f"{what} lse")
    sl = torch.tensor(lens, dtype=torch.int32, device=q.device)
    wo, wl = _padded_witness(pkg, q, qlens, k, v, sl, table, n, causal)
    _check(out[:used], wo, dtype, f"{what} out vs the padded call")
    _check_lse(lse[:, :used], wl, f"{what} lse vs the padded call")


def _run_packed(pkg, dev, H, Hkv, D, dtype, page, qlens, lens, n, causal=True, seed=1, max_pages=None, tail=7, what=""):
    """no append: `lens` are the keys in the cache. Returns (out, lse, q, pc)"""
    B = len(qlens)
    max_pages = max_pages or max(1, max((ln + page - 1) // page for ln in lens)) + 1
    T = sum(qlens) + tail
    q = _rand((T, H, D), dtype, dev, seed)
    q[sum(qlens):] = NAN
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, seed + 1)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, seed + 2, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, seed)
    out, lse = pkg.flash_attention_n_kvcache_varlen(q, pc.k, pc.v, pc.lens, _cu(qlens, dev), max(max(qlens), 1), block_table=pc.table,
                                                    softmax_n_param=n, is_causal=causal, return_lse=True)
    _check_packed(pkg, out, lse, q, qlens, pc.k, pc.v, pc.table, page, lens, n, causal, dtype, what)
    return out, lse, q, pc


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("page", [64, 256])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", [(8, 1), (16, 16), (12, 4)])
def test_parity(pkg, dev, heads, D, dtype, page, causal):
    H, Hkv = heads
    PB = 128 // (H // Hkv)   # 16 / 128 / 42
    # a decode token, an empty sequence, an exact block, a block boundary, several blocks, a decode token last
    qlens = [1, 0, PB, PB + 1, 2 * PB + 3, 1]
    lens = [300, 5, 0, page + 1, 2 * page, 64]
    _run_packed(pkg, dev, H, Hkv, D, dtype, page, qlens, lens, 1.0, causal=causal, seed=100 + D + page + H,
                what=f"H={H}/{Hkv} D={D} {dtype} page={page} causal={causal}")


@pytest.mark.parametrize("D", [32, 256])
def test_parity_other_head_dims(pkg, dev, D):
    qlens = [1, 0, 16, 17, 35, 1]
    _run_packed(pkg, dev, 8, 1, D, torch.bfloat16, 64, qlens, [300, 5, 0, 65, 128, 64], 1.0, seed=150 + D, what=f"D={D}")


# ---------------------------------------------------------------- 2. neighbours inside one wave span
@pytest.mark.parametrize("cache", [(64, 4), (256, 16)])
def test_neighbouring_sequences_do_not_touch_each_other(pkg, dev, cache):
    """qlens = [5, 3] at G = 8 (PB = 16): both sequences' rows lie inside the first 32-row wave span of their items. Each sequence's result
    must be the result of calling it alone - bit for bit where both launches have the same split count."""
    page, max_pages = cache
    dtype, H, Hkv, D, qlens, lens = torch.bfloat16, 8, 1, 64, [5, 3], [70, 200]
    n = _n_values((H,), dev, 200)
    out, lse, q, pc = _run_packed(pkg, dev, H, Hkv, D, dtype, page, qlens, lens, n, seed=201, max_pages=max_pages, tail=0, what=f"neighbours {cache}")
    both = _nsplit(_plan(pkg, 2, H, Hkv, 5, D, 8, page, max_pages), 2, Hkv, 5, 8, 16)
    t0 = 0
    for b, ql in enumerate(qlens):
        alone = _nsplit(_plan(pkg, 1, H, Hkv, ql, D, ql, page, max_pages), 1, Hkv, ql, ql, 16)
        o1, l1 = pkg.flash_attention_n_kvcache_varlen(q[t0:t0 + ql].contiguous(), pc.k, pc.v, pc.lens[b:b + 1], _cu([ql], dev), ql,
                                                      block_table=pc.table[b:b + 1], softmax_n_param=n, return_lse=True)
        if alone == both:
            assert torch.equal(out[t0:t0 + ql], o1) and torch.equal(lse[:, t0:t0 + ql], l1), f"sequence {b}: not the bits of the call alone"
        else:
            _check(out[t0:t0 + ql], o1, dtype, f"sequence {b} vs alone out")
            _check_lse(lse[:, t0:t0 + ql], l1, f"sequence {b} vs alone lse")
        t0 += ql
    assert both == _nsplit(_plan(pkg, 1, H, Hkv, 5, D, 5, page, max_pages), 1, Hkv, 5, 5, 16), "the shapes were chosen so that the bits are compared"


# ---------------------------------------------------------------- 3. several splits
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_several_splits(pkg, dev, dtype):
    c = SPLIT
    _split_plan(pkg)
    _run_packed(pkg, dev, c["H"], c["Hkv"], c["D"], dtype, c["page"], c["qlens"], [4000, 2100], _n_values((c["H"],), dev, 300), seed=301,
                max_pages=c["max_pages"], what=f"several splits {dtype}")


@pytest.mark.parametrize("n", [1.0, 0.0, 0.5])
def test_several_splits_nothing_visible(pkg, dev, n):
    c = SPLIT
    _split_plan(pkg)
    out, lse, _, _ = _run_packed(pkg, dev, c["H"], c["Hkv"], c["D"], torch.bfloat16, c["page"], c["qlens"], [0, 0], n, seed=310,
                                 max_pages=c["max_pages"], what=f"nothing visible n={n}")
    assert (out[:41] == 0).all()
    want = math.log(n) if n > 0 else float("-inf")
    assert torch.equal(lse[:, :41], torch.full_like(lse[:, :41], want))


# ---------------------------------------------------------------- 4. append
def test_append_writes_exactly_the_new_rows(pkg, dev):
    dtype, H, Hkv, D, page, max_pages = torch.float16, 16, 4, 64, 64, 3
    cap = page * max_pages
    qlens = [50, 1, 0, 20, 1]
    lens = [cap - 48, page - 1, 7, page - 2, 0]      # sequence 0 crosses the capacity by 2; a page boundary; an empty one; from nothing
    B, used = len(qlens), sum(qlens)
    T = used + 7
    q = _rand((T, H, D), dtype, dev, 400)
    kn = _rand((T, Hkv, D), dtype, dev, 401)
    vn = _rand((T, Hkv, D), dtype, dev, 402, std=1.0)
    for t in (q, kn, vn):
        t[used:] = NAN
    kd = _rand((B, Hkv, cap, D), dtype, dev, 403)
    vd = _rand((B, Hkv, cap, D), dtype, dev, 404, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, 405, alloc_all=True, guard=7.0)
    k0, v0, lens0 = pc.k.clone(), pc.v.clone(), pc.lens.clone()
    cu = _cu(qlens, dev)
    out, lse = pkg.flash_attention_n_kvcache_varlen(q, pc.k, pc.v, pc.lens, cu, 50, block_table=pc.table, k_new=kn, v_new=vn, return_lse=True)
    assert torch.equal(pc.lens, lens0), "cache_seqlens was modified"
    ke, ve = k0.clone(), v0.clone()
    t0 = 0
    for b, ql in enumerate(qlens):
        for i in range(ql):
            pos = lens[b] + i
            if pos < cap:
                pid = int(pc.table[b, pos // page])
                ke[pid, pos % page], ve[pid, pos % page] = kn[t0 + i], vn[t0 + i]
        t0 += ql
    assert torch.equal(pc.k.view(torch.int16), ke.view(torch.int16)), "k_cache: not exactly the new rows"
    assert torch.equal(pc.v.view(torch.int16), ve.view(torch.int16)), "v_cache: not exactly the new rows"
    assert (pc.k[-1] == 7.0).all() and (pc.v[-1] == 7.0).all(), "guard page behind the cache was written"
    assert torch.isfinite(out[:used]).all()
    # the call without an append on a cache that already holds the rows: the same bits, sequence 0 (its length is clamped) included ...
    total = [min(ln + ql, cap) for ln, ql in zip(lens, qlens)]
    sl = torch.tensor([ln + ql for ln, ql in zip(lens, qlens)], dtype=torch.int32, device=dev)
    o2, l2 = pkg.flash_attention_n_kvcache_varlen(q, pc.k, pc.v, sl, cu, 50, block_table=pc.table, return_lse=True)
    assert torch.equal(out[:used], o2[:used]) and torch.equal(lse[:, :used], l2[:, :used])
    # ... and the sequences that lost no row against the reference (causal alignment counts the rows of sequence 0 that were dropped)
    kg, vg = _gather(pc.k, pc.table, total, page), _gather(pc.v, pc.table, total, page)
    o_ref, lse_ref = _packed_reference(q[50:], qlens[1:], kg[1:], vg[1:], total[1:], 1.0, True)
    _check(out[50:used], o_ref, dtype, "append out")
    _check_lse(lse[:, 50:used], lse_ref, "append lse")


# ---------------------------------------------------------------- 5. tensor n: per sequence and head
@pytest.mark.parametrize("shape", ["H", "BH"])
def test_tensor_n(pkg, dev, shape):
    H, Hkv, qlens = 12, 4, [1, 50, 0, 3]
    n = _n_values({"H": (H,), "BH": (len(qlens), H)}[shape], dev, 500)
    assert (n == 0).any() and (n > 0).any()
    _run_packed(pkg, dev, H, Hkv, 128, torch.bfloat16, 64, qlens, [200, 3, 9, 65], n, seed=501, what=f"n[{shape}]")


# ---------------------------------------------------------------- 6. HIP graph
def test_graph_replay_follows_offsets_lengths_table_and_query(pkg, dev):
    """One capture (forward alone; linear, one stream) at T = 64, B = 4, max_seqlen_q = 48; replays after cu_seqlens_q, cache_seqlens,
    query and one block-table row changed in place: three raggednesses, parity each time and the bits of an eager call."""
    dtype, H, Hkv, D, page, max_pages, T, B, Sq = torch.bfloat16, 16, 4, 64, 64, 8, 64, 4, 48
    q = _rand((T, H, D), dtype, dev, 600)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 601)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, 602, std=1.0)
    pc = _Paged(kd, vd, [page * max_pages] * B, page, max_pages, 603, alloc_all=True)   # every row finite: the lengths move
    n = _n_values((H,), dev, 604)
    cu = _cu([1, 1, 1, 1], dev)
    sl = torch.tensor([62, 100, 5, 300], dtype=torch.int32, device=dev)
    table = pc.table

    def call(q_, sl_, cu_, tab):
        return pkg.flash_attention_n_kvcache_varlen(q_, pc.k, pc.v, sl_, cu_, Sq, block_table=tab, softmax_n_param=n, return_lse=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            call(q, sl, cu, table)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        go, glse = call(q, sl, cu, table)
    for step, qlens in enumerate(([1, 1, 1, 1], [48, 1, 10, 5], [0, 16, 30, 18])):
        lens = [62 + 37 * step, 100 + step, 5, 300 - 64 * step]
        with torch.no_grad():
            q.copy_(_rand((T, H, D), dtype, dev, 610 + step))
            q[sum(qlens):] = NAN
            cu.copy_(_cu(qlens, dev))
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
            table[step] = table[step].flip(0)
        g.replay()
        torch.cuda.synchronize()
        eo, el = call(q.clone(), sl.clone(), cu.clone(), table.clone())
        used = sum(qlens)
        assert torch.equal(go[:used], eo[:used]) and torch.equal(glse[:, :used], el[:, :used]), f"replay {step}: differs from the eager call"
        _check_packed(pkg, go, glse, q, qlens, pc.k, pc.v, table, page, lens, n, True, dtype, f"replay {step} qlens={qlens}")


# ---------------------------------------------------------------- 7. refusals on the device
def test_refusals_on_the_device(pkg, dev):
    dtype = torch.bfloat16
    q = torch.zeros(10, 8, 64, dtype=dtype, device=dev)
    kc = torch.zeros(4, 64, 2, 64, dtype=dtype, device=dev)
    sl = torch.zeros(2, dtype=torch.int32, device=dev)
    cu = torch.tensor([0, 4, 9], dtype=torch.int32, device=dev)
    bt = torch.zeros(2, 2, dtype=torch.int32, device=dev)
    fa = pkg.flash_attention_n_kvcache_varlen
    assert fa(q, kc, kc, sl, cu, 8, block_table=bt).shape == (10, 8, 64)
    with pytest.raises(NotImplementedError, match="alibi_slopes is not supported on token-packed queries"):
        fa(q, kc, kc, sl, cu, 8, block_table=bt, alibi_slopes=torch.ones(8, device=dev))
    with pytest.raises(NotImplementedError, match="window is not supported on token-packed queries"):
        fa(q, kc, kc, sl, cu, 8, block_table=bt, window=64)
    with pytest.raises(NotImplementedError, match="rotary_cos is not supported on token-packed queries"):
        fa(q, kc, kc, sl, cu, 8, block_table=bt, rotary_cos=torch.ones(128, 16, device=dev), rotary_sin=torch.ones(128, 16, device=dev))
    with pytest.raises(ValueError, match=r"k_new must be \[T, Hkv, D\] = \[10, 2, 64\]"):
        kn = torch.zeros(2, 2, 5, 64, dtype=dtype, device=dev)
        fa(q, kc, kc, sl, cu, 8, block_table=bt, k_new=kn, v_new=kn)
    with pytest.raises(RuntimeError, match="cu_seqlens_q is on cpu"):
        fa(q, kc, kc, sl, cu.cpu(), 8, block_table=bt)
