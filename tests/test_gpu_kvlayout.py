"""The K/V cache's layout contract on the GPU: "any strided view whose rows are 16-byte aligned with feature stride 1; never copied".

Every route below - one per compiled forward text and per writing kernel - runs on caches re-housed under tests/kv_layout.py's L1 (K
nhd_pad, V hnd) and L2 (K hnd, V nhd_pad), where K and V differ in page, row and head stride, with strided query / k_new / v_new and
sliced block_table / tree_mask / accepted; then on contiguous clones of the same content. Asserted per case:
  (a) out and lse are bit-identical between the two calls;
  (b) after a call that writes, the views' logical content is bit-identical to the contiguous pools', and the rows the call wrote are
      those of the dense picture the test built on its own (eager rotation, CPU quantisation);
  (c) the gaps of the storage still hold the sentinel;
  (d) the launch plans of the two calls are equal and the argument blocks carried the views' strides;
  (e) the strided call meets the fp64 gate of tests/kv_witness.py directly: attend over the route's visible set (tree routes:
      kv_tree.tree_vis_brute), gate_c (3 u A + 1e-6) and _check_lse, inputs_c at logit std 4; FP8 routes on the upcast codes under
      power-of-two scales. No tolerance of its own.
Shapes: B = 3, heads 8 / 2, D = 64 (FP8 also 128), lens [0, 61, 130], Sq = 3 on the decode kernels, 40 with query_seqlens [40, 7, 0] on the
prefill kernels, 13-node trees, packed qlens [1, 0, 16, 17]; page 64, and 256 once per forward text; bf16, and fp16 once per forward text;
the base routes also at D = 32, 128, 256. The window is 40: the longest sequence's walk starts at tile 1, with the page below it freed.
The far-pool cases put the three pages of one sequence below 2^31, below 2^32 and beyond 2^32 bytes of one 4.5 GiB pool; the
largest-stride cases use the largest row stride fasn_kv_check admits. Both rest on the review of every address expression of the
K/V kernels (64-bit throughout; the forwards' 32-bit lane offsets and descriptor ranges stay below 64 * row_stride * 2 < 2^31)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_fp8 as k8         # noqa: E402
import kv_layout as kl      # noqa: E402
import kv_support as ks     # noqa: E402

from kv_layout import (BF16, FP16, HKV, ROUTES, _check_plans, _check_reference, _dense_bits, _invoke, _logical, _operands,   # noqa: E402
                       _per_sequence, _setup, _written)

pytestmark = pytest.mark.gpu


def _run_layout(pkg, s, layout, what):
    """the case under L1 / L2 against its contiguous twin: (a) - (e)"""
    ks_, vs_, kst, vst = kl.rehouse(s.k_pool, s.v_pool, layout)
    kc, vc = s.k_pool.clone(), s.v_pool.clone()
    with kl.recording(pkg) as rec_s:
        out_s, lse_s = _invoke(pkg, s, _operands(s, ks_, vs_, s.table, True))
    with kl.recording(pkg) as rec_c:
        out_c, lse_c = _invoke(pkg, s, _operands(s, kc, vc, s.table, False))
    torch.cuda.synchronize()
    (a_o, a_l), (b_o, b_l) = _written(s, out_s, lse_s), _written(s, out_c, lse_c)
    assert torch.equal(ks._bits(a_o), ks._bits(b_o)), f"{what}: out differs from the contiguous call in {(ks._bits(a_o) != ks._bits(b_o)).sum().item()} elements"
    assert torch.equal(a_l.view(torch.int32), b_l.view(torch.int32)), f"{what}: lse differs from the contiguous call"
    assert torch.equal(kl.ints(ks_), kl.ints(kc)) and torch.equal(kl.ints(vs_), kl.ints(vc)), f"{what}: the pools differ after the call"
    if s.case.append:
        for pool, exp, name in ((kc, s.k_exp, "k"), (vc, s.v_exp, "v")):
            have = _logical(s, pool, s.table, s.page)
            exp_bits = _dense_bits(s, exp)
            assert torch.equal(have, exp_bits[:, :, :have.shape[2]]), f"{what}: {name} rows of the cache are not the dense picture's"
    assert kl.gaps_intact(kst, ks_) and kl.gaps_intact(vst, vs_), f"{what}: a gap of the storage was written"
    _check_plans(s, rec_s, rec_c, ks_, vs_, what)
    _check_reference(s, _per_sequence(s, out_s, lse_s), what)


# ---------------------------------------------------------------- 1. every route under L1 and L2
@pytest.mark.parametrize("layout", ["L1", "L2"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_route_on_a_rehoused_cache(pkg, dev, route, layout):
    D = 64
    _run_layout(pkg, _setup(dev, route, BF16, D, 64, 900 + sorted(ROUTES).index(route)), layout, f"{route} {layout}")


@pytest.mark.parametrize("layout", ["L1", "L2"])
@pytest.mark.parametrize("route", ["fp8_decode", "fp8_prefill", "fp8_tree_rope"])
def test_fp8_route_at_head_dim_128(pkg, dev, route, layout):
    _run_layout(pkg, _setup(dev, route, BF16, 128, 64, 940), layout, f"{route} D=128 {layout}")


@pytest.mark.parametrize("layout", ["L1", "L2"])
@pytest.mark.parametrize("variant", ["page256", "fp16"])
@pytest.mark.parametrize("route", ["decode", "prefill", "decode_window", "prefill_window"])
def test_forward_text_variants(pkg, dev, route, variant, layout):
    """once per forward text: several tiles per page (the u_tip * KV_KT * row_stride term of the tile offset; under the window the walk
    STARTS at tile 1 of a page), and fp16"""
    dtype, page = (BF16, 256) if variant == "page256" else (FP16, 64)
    _run_layout(pkg, _setup(dev, route, dtype, 64, page, 950), layout, f"{route} {variant} {layout}")


@pytest.mark.parametrize("layout", ["L1", "L2"])
@pytest.mark.parametrize("D", [32, 128, 256])
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_other_head_dims(pkg, dev, route, D, layout):
    """the base forwards and appends at the other head dims the 16-bit cache kernels are built for"""
    _run_layout(pkg, _setup(dev, route, BF16, D, 64, 955), layout, f"{route} D={D} {layout}")


@pytest.mark.parametrize("layout", ["L1", "L2"])
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_dense_cache(pkg, dev, route, layout):
    """block_table=None, capacity 200: the page stride is the batch stride"""
    _run_layout(pkg, _setup(dev, route, BF16, 64, 200, 960, max_pages=1, dense=True), layout, f"dense {route} {layout}")


# ---------------------------------------------------------------- 2. the commits
def _commit_reference(k, v, table, page, base, accepted, alens):
    """through a temporary: every source is read before any destination is written"""
    k2, v2 = k.clone(), v.clone()
    for b, (bs, path, alen) in enumerate(zip(base, accepted, alens)):
        for kk in range(alen):
            src, dst = bs + path[kk], bs + kk
            ps, pd = (int(table[b, src // page]), int(table[b, dst // page])) if table is not None else (b, b)
            k2[pd, dst % page], v2[pd, dst % page] = k[ps, src % page], v[ps, src % page]
    return k2, v2


COMMIT = dict(base=[60, 5, 0, 128 - 3], accepted=[[0, 2, 3, 7], [0, 1, 2, 3], [0, 5, 9, 11], [0, 4, 9, 15]], alens=[4, 4, 0, 4])


@pytest.mark.parametrize("layout", ["L1", "L2"])
@pytest.mark.parametrize("paged", [True, False], ids=["paged", "dense"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_commit_on_a_rehoused_cache(pkg, dev, fp8, paged, layout):
    """tests/test_gpu_kvtree.py::test_commit's paths - the overlapping chain (row 2 is a source and a destination), the identity, an empty
    path, a path that ends at node 15 and crosses a page edge - on L1 / L2 with `accepted` and the table as slices: the whole pools bit for
    bit against the contiguous call and against a move on the host, the gaps untouched"""
    Sq, D, page, mp = 16, 64, 64, 3
    base, accepted, alens = COMMIT["base"], COMMIT["accepted"], COMMIT["alens"]
    B = len(base)
    if fp8:
        kd, vd = k8.rand_codes((B, HKV, page * mp, D), 71, dev), k8.rand_codes((B, HKV, page * mp, D), 72, dev)
    else:
        kd, vd = ks._rand((B, HKV, page * mp, D), BF16, dev, 71), ks._rand((B, HKV, page * mp, D), BF16, dev, 72, std=1.0)
    if paged:
        pc = k8.PagedCodes(kd, vd, [b + Sq for b in base], page, mp, 73) if fp8 else ks._Paged(kd, vd, [b + Sq for b in base], page, mp, 73, alloc_all=True)
        k, v, table = pc.k, pc.v, pc.table
    else:
        k, v, table = kd.permute(0, 2, 1, 3).contiguous(), vd.permute(0, 2, 1, 3).contiguous(), None
        k, v = (k.view(kl.F8), v.view(kl.F8)) if fp8 else (k, v)
    tbl = None if table is None else table.cpu()
    k_ref, v_ref = _commit_reference(kl.ints(k), kl.ints(v), tbl, page if paged else page * mp, base, accepted, alens)
    assert not torch.equal(k_ref, kl.ints(k))
    commit = pkg.flash_attention_n_kvcache_fp8_tree_commit if fp8 else pkg.flash_attention_n_kvcache_tree_commit
    sl = torch.tensor(base, dtype=torch.int32, device=dev)
    acc, al = torch.tensor(accepted, dtype=torch.int32, device=dev), torch.tensor(alens, dtype=torch.int32, device=dev)
    ks_, vs_, kst, vst = kl.rehouse(k, v, layout)
    kc, vc = k.clone(), v.clone()
    commit(ks_, vs_, sl, kl.column_slice(acc, 99), al, block_table=None if table is None else kl.column_slice(table, pc.poison))
    commit(kc, vc, sl, acc, al, block_table=table)
    torch.cuda.synchronize()
    assert torch.equal(kl.ints(ks_), kl.ints(kc)) and torch.equal(kl.ints(vs_), kl.ints(vc)), "the pools differ after the commit"
    assert torch.equal(kl.ints(kc), k_ref) and torch.equal(kl.ints(vc), v_ref), "the contiguous commit is not the move on the host"
    assert kl.gaps_intact(kst, ks_) and kl.gaps_intact(vst, vs_), "a gap of the storage was written"
    assert sl.tolist() == base


# ---------------------------------------------------------------- 3. pages beyond 4 GiB
FAR = {
    "decode": ("decode", [126], 3), "prefill": ("prefill", [100], 3), "packed": ("packed", [120], 3), "rope": ("rope_decode", [126], 3),
    "tree_commit": ("decode_tree", [120], 3), "fp8_decode": ("fp8_decode", [126], 3), "fp8_prefill": ("fp8_prefill", [100], 3),
    "fp8_tree_commit": ("fp8_tree_decode", [120], 3),
}
FAR_PATH = [0, 8, 9, 12]   # nodes 8, 9, 12 lie in the page beyond 2^32 (rows 128, 129, 132), their destinations 121 .. 123 in the one below


@pytest.mark.parametrize("name", sorted(FAR))
def test_far_pool(pkg, dev, name):
    """One sequence whose three pages are far_ids of a 4.5 GiB pool [P, 2, page, Hkv, D] serving K and V: byte offsets below 2^31, in
    [2^31, 2^32) and beyond 2^32 for both, the last beyond 2^31 16-bit elements. The appends cross from the middle page into the last; the
    commit moves rows back across that edge. (a), (b) on the used pages and (e); the alias pages (the offsets mod 2^31 and 2^32) and the
    neighbours of the used pages keep the sentinel."""
    route, lens, mp = FAR[name]
    s = _setup(dev, route, BF16, 64, 64, 970, lens=lens, max_pages=mp, qlens=[17] if route == "packed" else None)
    store = None
    torch.cuda.reset_peak_memory_stats()
    try:
        store, kf, vf, info = kl.far_pool(s.k_pool, dev)
        ids = info["ids"]
        near = [int(x) for x in s.table[0]]
        for pid, src in zip(ids, near):
            store[pid, 0], store[pid, 1] = kl.ints(s.k_pool)[src], kl.ints(s.v_pool)[src]
        far_table = torch.tensor([ids], dtype=torch.int32, device=dev)
        assert far_table.tolist() == [list(ids)] and s.table.shape == (1, 3)
        kc, vc = s.k_pool.clone(), s.v_pool.clone()
        with kl.recording(pkg) as rec_s:
            out_s, lse_s = _invoke(pkg, s, _operands(s, kf, vf, far_table, False))
        with kl.recording(pkg) as rec_c:
            out_c, lse_c = _invoke(pkg, s, _operands(s, kc, vc, s.table, False))
        if "commit" in name:
            commit = pkg.flash_attention_n_kvcache_fp8_tree_commit if s.fp8 else pkg.flash_attention_n_kvcache_tree_commit
            acc, al = torch.tensor([FAR_PATH], dtype=torch.int32, device=dev), torch.tensor([4], dtype=torch.int32, device=dev)
            before = kl.ints(kc).clone()
            commit(kf, vf, s.lens_t, acc, al, block_table=far_table)
            commit(kc, vc, s.lens_t, acc, al, block_table=s.table)
            assert not torch.equal(before, kl.ints(kc))
        torch.cuda.synchronize()
        (a_o, a_l), (b_o, b_l) = _written(s, out_s, lse_s), _written(s, out_c, lse_c)
        assert torch.equal(ks._bits(a_o), ks._bits(b_o)) and torch.equal(a_l.view(torch.int32), b_l.view(torch.int32)), f"far {name}: outputs differ"
        for pid, src in zip(ids, near):
            assert torch.equal(kl.ints(kf[pid]), kl.ints(kc[src])) and torch.equal(kl.ints(vf[pid]), kl.ints(vc[src])), f"far {name}: page {pid} differs"
        assert kl.far_guard_intact(store, info, s.k_pool.dtype), f"far {name}: an alias or a neighbour page was written"
        assert [(n, p) for n, p, _ in rec_s] == [(n, p) for n, p, _ in rec_c]
        _check_reference(s, _per_sequence(s, out_s, lse_s), f"far {name}")
        peak = torch.cuda.max_memory_allocated()
        print(f"far {name}: peak device memory {peak / 2 ** 30:.2f} GiB")
        assert peak <= 5 * 2 ** 30
    finally:
        del store
        kf = vf = None
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 4. the largest row stride the host admits
KV_KT = 64
MAX_ROW_STRIDE = (2 ** 31 - 1) // (KV_KT * 2) // 8 * 8   # fasn_kv_check: KV_KT * row_stride * 2 < 2^31, strides % 8 elements: 2^24 - 8


@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_largest_legal_row_stride(pkg, dev, route):
    """A dense cache of one sequence, 64 + 3 rows MAX_ROW_STRIDE elements apart in one uninitialised buffer (K at the head of a row's
    stretch, V in its middle): the forwards' 32-bit lane offsets and descriptor ranges at their limit. (a) against the contiguous call and
    (e); one alignment step more is refused as FASN_EUNSUPPORTED (-7)."""
    rows, D = KV_KT + 3, 64
    ln = rows - ROUTES[route]["Sq"]
    s = _setup(dev, route, BF16, D, rows, 980, lens=[ln], max_pages=1, dense=True)
    assert KV_KT * MAX_ROW_STRIDE * 2 < 2 ** 31 <= KV_KT * (MAX_ROW_STRIDE + 8) * 2
    buf = None
    try:
        buf = torch.empty(rows * MAX_ROW_STRIDE, dtype=BF16, device=dev)
        size, stride = (1, rows, HKV, D), (rows * MAX_ROW_STRIDE, MAX_ROW_STRIDE, D, 1)
        kbig, vbig = torch.as_strided(buf, size, stride), torch.as_strided(buf, size, stride, 1 << 23)
        kbig.copy_(s.k_pool)
        vbig.copy_(s.v_pool)
        kc, vc = s.k_pool.clone(), s.v_pool.clone()
        with kl.recording(pkg) as rec_s:
            out_s, lse_s = _invoke(pkg, s, _operands(s, kbig, vbig, None, False))
        with kl.recording(pkg) as rec_c:
            out_c, lse_c = _invoke(pkg, s, _operands(s, kc, vc, None, False))
        torch.cuda.synchronize()
        assert torch.equal(ks._bits(out_s), ks._bits(out_c)) and torch.equal(lse_s.view(torch.int32), lse_c.view(torch.int32))
        assert torch.equal(kl.ints(kbig), kl.ints(kc)) and torch.equal(kl.ints(vbig), kl.ints(vc))
        assert [(n, p) for n, p, _ in rec_s] == [(n, p) for n, p, _ in rec_c]
        assert all(st[0][1] == MAX_ROW_STRIDE and st[1][1] == MAX_ROW_STRIDE for _, _, st in rec_s)
        _check_reference(s, _per_sequence(s, out_s, lse_s), f"largest stride {route}")
        # one alignment step more: refused on the host, nothing is launched (the view stays inside the buffer)
        over = torch.as_strided(buf, size, (rows * MAX_ROW_STRIDE, MAX_ROW_STRIDE + 8, D, 1))
        with pytest.raises(pkg._lib.FasnError, match=r"code -7"):
            _invoke(pkg, s, _operands(s, over, vc, None, False))
        with pytest.raises(pkg._lib.FasnError, match=r"code -7"):
            _invoke(pkg, s, _operands(s, kc, over, None, False))
        del over
    finally:
        del buf
        kbig = vbig = None
        torch.cuda.empty_cache()
