"""The test of the layout tests (tests/kv_layout.py, tests/test_gpu_kvlayout.py), without a GPU: the re-housed views are what they claim to
be; a cache read and written through (strides, table) in plain integers reproduces the dense picture, and each way a kernel could get
that arithmetic wrong - V read with K's strides, the head stride taken as D, the page stride taken as page * Hkv * D, an offset truncated
to 32 bits, a write one row early - breaks check (b) or (c) of the GPU suite on that suite's own shapes; the argument blocks
kvcache.py fills from the views carry the views' strides and every route's plan names the kernels it is there to reach; far_ids'
arithmetic; the fp64 gate (e) accepts the rounded reference and refuses a cache whose heads are swapped."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_fp8 as k8        # noqa: E402
import kv_layout as kl     # noqa: E402
import kv_support as ks    # noqa: E402
import kv_tree as kt       # noqa: E402
import kv_witness as kw    # noqa: E402

CPU = torch.device("cpu")
BF16, FP16 = torch.bfloat16, torch.float16
P, PAGE, HKV, D = 5, 64, 2, 64


def _pools(kind):
    if kind == "codes":
        return k8.rand_codes((P, PAGE, HKV, D), 1, CPU).view(kl.F8), k8.rand_codes((P, PAGE, HKV, D), 2, CPU).view(kl.F8)
    dtype = BF16 if kind == "bf16" else FP16
    k, v = ks._rand((P, PAGE, HKV, D), dtype, CPU, 1), ks._rand((P, PAGE, HKV, D), dtype, CPU, 2)
    k[3, 40:], v[3, 40:] = kl.NAN, kl.NAN   # stale rows
    return k, v


# ---------------------------------------------------------------- 1. the views
@pytest.mark.parametrize("layout", ["L1", "L2"])
@pytest.mark.parametrize("kind", ["bf16", "fp16", "codes"])
def test_rehoused_views(pkg, kind, layout):
    k, v = _pools(kind)
    kv, vv, kst, vst = kl.rehouse(k, v, layout)
    for view, pool, lay, store in ((kv, k, kl.LAYOUTS[layout][0], kst), (vv, v, kl.LAYOUTS[layout][1], vst)):
        assert torch.equal(kl.ints(view), kl.ints(pool)) and view.dtype == pool.dtype and not view.is_contiguous()
        assert tuple(view.stride()) == kl.expected_strides(lay, PAGE, HKV, D) + (1,)
        pkg.kvcache._check_cache("cache", view, True, D)
        assert view.data_ptr() % 16 == 0 and all(view.stride(i) * view.element_size() % 16 == 0 for i in range(3))
        assert kl.gaps_intact(store, view)
        assert not (kl.ints(pool) == kl.SENTINEL[pool.dtype]).any()   # no test value and no stale row is the sentinel
    assert all(kv.stride(i) != vv.stride(i) for i in range(3))
    # one poked gap element shows; a write inside the view does not
    pad, pad_view = (kst, kv) if layout == "L1" else (vst, vv)
    for spot in ((2, PAGE, 0, 5), (2, 7, HKV, 0), (P - 1, PAGE, HKV, D - 1)):
        old = pad[spot].item()
        pad[spot] = 0
        assert not kl.gaps_intact(pad, pad_view), spot
        pad[spot] = old
    kl.ints(pad_view)[1, 2, 1, 3] = 0
    assert kl.gaps_intact(pad, pad_view)


def test_the_sentinels_are_nan_with_a_payload():
    for dtype, std in ((BF16, 0x7FC0), (FP16, 0x7E00)):
        s = torch.tensor([kl.SENTINEL[dtype]], dtype=torch.int16)
        assert torch.isnan(s.view(dtype)).all() and kl.SENTINEL[dtype] != std
        assert torch.tensor([kl.NAN], dtype=dtype).view(torch.int16).item() == std
    assert kl.SENTINEL[kl.F8] == 0xFF != k8.NAN_CODE


def test_operand_and_argument_views():
    q, kn, vn = (ks._rand((3, h, 5, D), BF16, CPU, 3 + h) for h in (8, HKV, HKV))
    qv, knv, vnv = kl.q_view(q), kl.k_new_view(kn), kl.v_new_view(vn)
    assert torch.equal(qv, q) and torch.equal(knv, kn) and torch.equal(vnv, vn)
    assert all(knv.stride(i) != vnv.stride(i) for i in range(3))
    tq, tk, tv = (ks._rand((11, h, D), BF16, CPU, 9 + h) for h in (8, HKV, HKV))
    pq, pk, pv = kl.packed_views(tq, tk, tv)
    assert torch.equal(pq, tq) and torch.equal(pk, tk) and torch.equal(pv, tv) and pq.stride(0) == (8 + 2 * HKV) * D and pk.stride() != pv.stride()
    table = torch.arange(12, dtype=torch.int32).view(3, 4)
    sl = kl.column_slice(table, 77)
    assert sl.stride(0) == 7 and sl.data_ptr() % 4 == 0
    words = kl.column_slice(torch.arange(39, dtype=torch.int64).view(3, 13), -1)
    assert words.stride(0) > 13 and words.data_ptr() % 8 == 0


# ---------------------------------------------------------------- 2. the address arithmetic and its mutants, on the GPU cases' shapes
def _flat(view, store):
    """(flat storage, the view's (page, row, head) strides, its base offset in the storage)"""
    return store.reshape(-1), tuple(view.stride()[:3]), view.storage_offset() - store.storage_offset()


def _read(s, view, store, strides=None, base=None):
    flat, st, b0 = _flat(view, store)
    need = s.table.shape[1]
    return kl.gather(flat, st if strides is None else strides, s.table, s.page, HKV, s.D, s.B, need * s.page, b0 if base is None else base)


def _same(a, b):
    return a is not None and b is not None and torch.equal(a, b)


@pytest.mark.parametrize("layout", ["L1", "L2"])
@pytest.mark.parametrize("route", ["prefill", "fp8_prefill", "decode_tree"])
def test_gather_through_strides_and_its_mutants(pkg, route, layout):
    s = kl._setup(CPU, route, BF16, 64, 64, 900)
    kv, vv, kst, vst = kl.rehouse(s.k_pool, s.v_pool, layout)
    need = s.table.shape[1]
    dense = lambda pool: kl.ints(pool)[s.table.long()].reshape(s.B, need * s.page, HKV, s.D).permute(0, 2, 1, 3)   # noqa: E731
    want_k, want_v = dense(s.k_pool), dense(s.v_pool)
    assert _same(_read(s, kv, kst), want_k) and _same(_read(s, vv, vst), want_v)
    (_, k_st, k_base), (_, v_st, _) = _flat(kv, kst), _flat(vv, vst)
    # V read with K's strides
    assert not _same(_read(s, vv, vst, k_st, k_base), want_v)
    # the head stride taken as D, the page stride taken as page * Hkv * D: each is right for one of the two layouts, so a pair of pools
    # under L1 / L2 always holds one it is wrong for
    for mutant in (lambda st: (st[0], st[1], s.D), lambda st: (s.page * HKV * s.D, st[1], st[2])):
        ok_k, ok_v = _same(_read(s, kv, kst, mutant(k_st)), want_k), _same(_read(s, vv, vst, mutant(v_st)), want_v)
        assert ok_k != ok_v, "the mutant must be wrong for exactly the pool whose layout differs from its assumption"
    # the append as the kernels address it lands on the dense picture and leaves the gaps alone; one row early breaks (b) or (c)
    new_k, new_v = (torch.stack([kl.ints(e)[b, :, s.case.lens[b]:s.case.lens[b] + s.case.Sq] for b in range(s.B)]) for e in (s.k_exp, s.v_exp))
    for shift in (0, -1):
        kv2, vv2, kst2, vst2 = kl.rehouse(s.k_pool, s.v_pool, layout)
        faulted = False
        try:
            for view, store, rows in ((kv2, kst2, new_k), (vv2, vst2, new_v)):
                flat, st, b0 = _flat(view, store)
                for b in range(s.B):
                    x = s.case.qlens[b]
                    if x:
                        kl.scatter(flat, rows[b:b + 1, :, :x], st, s.table[b:b + 1], s.page, [s.case.lens[b]], b0, shift)
        except IndexError:
            faulted = True
        have = [kl._logical(s, view, s.table, s.page) for view in (kv2, vv2)]
        b_ok = all(torch.equal(h, kl._dense_bits(s, exp)[:, :, :h.shape[2]]) for h, exp in zip(have, (s.k_exp, s.v_exp)))
        c_ok = kl.gaps_intact(kst2, kv2) and kl.gaps_intact(vst2, vv2)
        assert (b_ok and c_ok and not faulted) == (shift == 0), (shift, b_ok, c_ok, faulted)


@pytest.mark.parametrize("page_bytes", [64 * 2 * 64 * 2, 64 * 2 * 64, 256 * 2 * 128 * 2], ids=["16bit", "codes", "page256_D128"])
def test_far_ids_and_the_truncated_offset(page_bytes):
    """far_ids' arithmetic for the 16-bit and the code page sizes, and the mutant in pure integers: an offset truncated to 32 bits (or a
    16-bit element index to 31) lands in a page that carries the sentinel, so check (c) of the far-pool cases sees it"""
    info = kl.far_ids(page_bytes)
    lo, mid, hi = info["ids"]
    slot = info["slot"]
    assert slot == 2 * page_bytes and info["pages"] * slot <= 5 << 30 and info["pages"] * slot > 1 << 32
    for off in (info["k_off"], info["v_off"]):
        assert 0 < off[0] < off[0] + page_bytes <= 2 ** 31 <= off[1] < off[1] + page_bytes <= 2 ** 32 <= off[2] < off[2] + page_bytes <= info["pages"] * slot
        assert off[2] // 2 >= 2 ** 31   # the 16-bit element offset of the last page
    assert info["k_off"] == tuple(p * slot for p in info["ids"]) and info["v_off"] == tuple(o + page_bytes for o in info["k_off"])
    guard, used = set(info["guard"]), {lo, mid, hi}
    assert not guard & used and {p + d for p in used for d in (-1, 1)} <= guard and set(info["aliases"]) <= guard
    for off in info["k_off"][1:] + info["v_off"][1:]:
        for last in (0, page_bytes - 16):   # the first and the last 16-byte chunk of the page
            true = off + last
            for wrapped in (true % 2 ** 32, true % 2 ** 31, 2 * ((true // 2) % 2 ** 31)):   # bytes in 32 / 31 bits, 16-bit elements in 31
                if wrapped != true:
                    assert wrapped // slot in guard and wrapped // slot not in used, (off, wrapped)
    assert info["k_off"][2] % 2 ** 32 != info["k_off"][2] and info["k_off"][1] % 2 ** 31 != info["k_off"][1]


# ---------------------------------------------------------------- 3. the argument blocks and the plans
@pytest.mark.parametrize("layout", ["L1", "L2"])
@pytest.mark.parametrize("route", sorted(kl.ROUTES))
def test_blocks_carry_the_views_strides(pkg, route, layout):
    """every route of the GPU suite with the launches taken out (kv_layout.dry_run): the blocks kvcache.py fills from the L1 / L2 views carry
    the views' strides - in codes on an FP8 cache - the plan is the contiguous call's and names the route's forward text and writer"""
    s = kl._setup(CPU, route, BF16, 64, 64, 900)
    kv, vv, _, _ = kl.rehouse(s.k_pool, s.v_pool, layout)
    recs = []
    for k, v, strided in ((kv, vv, True), (s.k_pool, s.v_pool, False)):
        o = kl._operands(s, k, v, s.table, strided)
        o.q = kl.on_device(o.q)
        with kl.dry_run(pkg) as rec:
            kl._invoke(pkg, s, o)
        recs.append(rec)
    kl._check_plans(s, recs[0], recs[1], kv, vv, f"{route} {layout}")
    lay_k, lay_v = kl.LAYOUTS[layout]
    assert all(st == (kl.expected_strides(lay_k, 64, HKV, 64), kl.expected_strides(lay_v, 64, HKV, 64)) for _, _, st in recs[0])
    assert all(st == ((64 * HKV * 64, HKV * 64, 64),) * 2 for _, _, st in recs[1])


def test_size_one_rules(pkg):
    """kvcache._prepare's rules for dimensions of size 1: a pool of ONE page carries page stride 0, a dense cache of ONE row carries the row
    stride D - whatever stride the view itself reports there"""
    q = kl.on_device(ks._rand((2, 8, 1, D), BF16, CPU, 1))
    lens = torch.zeros(2, dtype=torch.int32)
    one_page_k, one_page_v, _, _ = kl.rehouse(ks._rand((1, PAGE, HKV, D), BF16, CPU, 2), ks._rand((1, PAGE, HKV, D), BF16, CPU, 3), "L1")
    with kl.dry_run(pkg) as rec:
        pkg.flash_attention_n_kvcache(q, one_page_k, one_page_v, lens, block_table=torch.zeros(2, 1, dtype=torch.int32))
    (_, _, (k_st, v_st)), = rec
    assert one_page_k.stride(0) != 0 and k_st == (0,) + kl.expected_strides("nhd_pad", PAGE, HKV, D)[1:] and v_st == (0,) + kl.expected_strides("hnd", PAGE, HKV, D)[1:]
    one_row = torch.zeros(2, 3, HKV + 1, D, dtype=BF16)[:, :1, :HKV]   # row stride (Hkv + 1) D in the view
    with kl.dry_run(pkg) as rec:
        pkg.flash_attention_n_kvcache(q, one_row, one_row.clone(memory_format=torch.preserve_format), lens)
    (_, _, (k_st, v_st)), = rec
    assert one_row.stride(1) == (HKV + 1) * D and k_st[1] == v_st[1] == D and k_st[0] == 3 * (HKV + 1) * D and k_st[2] == D


# ---------------------------------------------------------------- 4. gate (e) sees a wrong cache
@pytest.mark.parametrize("route", ["prefill", "fp8_decode", "decode_tree", "rope_prefill"])
def test_the_reference_gate(route):
    """the fp64 reference rounded to the output type passes kv_layout._check_reference; the same with the K/V heads swapped does not"""
    s = kl._setup(CPU, route, BF16, 64, 64, 900)

    f = lambda t: t.detach().to("cpu", torch.float64)   # noqa: E731
    def rounded(k_eff, v_eff):
        res = []
        for b in range(s.B):
            ln, x = s.case.total[b], s.case.qlens[b]
            w = (kt.tree_vis_brute(ln, x, ln, s.rows[b], s.case.window) if s.rows is not None else kw.visible(ln, x, ln, True, s.case.window)).double()
            ref = kw.attend(f(s.q_eff[b, :, :x]), f(k_eff[b, :, :ln]), f(v_eff[b, :, :ln]), w, f(s.n), s.scale, None)
            res.append((ref["out"].to(s.dtype), ref["lse"].float()))
        return res

    kl._check_reference(s, rounded(s.k_eff, s.v_eff), f"{route} reference")
    with pytest.raises(AssertionError):
        kl._check_reference(s, rounded(s.k_eff.flip(1), s.v_eff.flip(1)), f"{route} heads swapped")
