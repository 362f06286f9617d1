"""Token-tree attention over the FP8 K/V cache on the GPU, on a paged cache of codes with NaN codes in every stale row and page.
flash_attention_n_kvcache_fp8_tree bit for bit against flash_attention_n_kvcache_tree on the exactly upcast cache under power-of-two scales
(both routes, the full word, several splits, a window with the pages below it gone), bit for bit against the causal and the window FP8
calls under the chain mask, against the fp64 reference of tests/kv_witness.py where one key decides a row, against the fp32 reference of
tests/kv_tree.py under general scales; the rotate-quantise-append at depth positions byte for byte against the quantised eager rotation and
the whole call against the composed route; flash_attention_n_kvcache_fp8_tree_commit byte for byte against a move on the host; verify -
commit - advance - decode end to end; graph replay; determinism."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_args as ka        # noqa: E402
import kv_fp8 as k8         # noqa: E402
import kv_fp8_tree as k8t   # noqa: E402
import kv_support as ks     # noqa: E402
import kv_tree as kt        # noqa: E402
import kv_witness as kw     # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
DIMS = [64, 128]
GENERAL = (0.3, 3.0, 1.7e-3)
_ids = lambda d: str(d).split(".")[-1]   # noqa: E731


def _dt(dtype):
    return 1 if dtype == torch.bfloat16 else 0


def _same(a, b):
    return torch.equal(ks._bits(a[0]), ks._bits(b[0])) and torch.equal(a[1], b[1])


def _plan(pkg, dtype, window, B, H, Hkv, Sq, D, page, max_pages, qlens=None):
    """(route, split count) of the FP8 tree plan, which has the grids of the 16-bit tree plan of the same shape and window"""
    route = k8t.route_of(H, Hkv, Sq, qlens)
    make = ka._args_decode if route == "decode" else ka._args_prefill
    a = make(pkg, dtype=_dt(dtype), B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages)
    tree = kt._tree(pkg, window=window or 0)
    base, plan = pkg._lib.kvtree_plan(a, tree), pkg._lib.kvfp8_tree_plan(a, k8._fp8(pkg), tree)
    assert [k[1:3] for k in plan] == [k[1:3] for k in base], (plan, base)
    assert plan[0][0].startswith("fasn_kvcache_fwd_fp8_tree_kernel<" if route == "decode" else "fasn_kvprefill_fwd_fp8_tree_kernel<")
    blocks = B * Hkv * (1 if route == "decode" else -(-Sq // (128 // (H // Hkv))))
    nsplit = plan[0][1] // blocks
    assert (len(plan) == 2) == (route == "decode" or nsplit > 1)
    return route, nsplit


# ---------------------------------------------------------------- 1. equal to the 16-bit tree call, bit for bit
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", sorted(k8t.TWIN_CASES))
def test_equals_the_16_bit_tree_call(pkg, dev, case, D, dtype):
    """kv_fp8_tree.TWIN_CASES under power-of-two scales: out and lse of the FP8 call are those of flash_attention_n_kvcache_tree on the exactly
    upcast cache with scale * k_scale, times v_scale (kv_fp8.assert_bitwise; tests/test_kvfp8_tree_cpu.py shows from the fp32 reference
    alone that every case stays inside its 5 % cap on subnormal results). Under the window every row and table entry below first_b is then
    poisoned, and the result does not change."""
    o = k8t.twin_operands(case, D, dtype, dev)
    c = k8t.TWIN_CASES[case]
    W, qlens = o["window"], o["qlens"]
    route, nsplit = _plan(pkg, dtype, W, o["B"], o["H"], o["Hkv"], o["Sq"], D, o["page"], o["max_pages"], qlens)
    assert route == ("prefill" if "prefill" in case or case == "full_g4" else "decode") and (nsplit > 1) == bool(c.get("splits"))
    pc = k8.PagedCodes(o["kd"], o["vd"], o["lens"], o["page"], o["max_pages"], c["seed"])
    masks = kt.words_tensor(o["rows"], dev)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    call8 = lambda: pkg.flash_attention_n_kvcache_fp8_tree(o["q"], pc.k, pc.v, pc.lens, o["k_scale"], o["v_scale"], masks, block_table=pc.table,   # noqa: E731
                                                           query_seqlens=qs, softmax_n_param=o["n"], return_lse=True, window=W)
    out, lse = call8()
    k16, v16 = pc.k.to(dtype), pc.v.to(dtype)   # exact; the stale rows become NaN, which the 16-bit call never reads either
    call16 = lambda q_, k_, v_, **kw_: pkg.flash_attention_n_kvcache_tree(q_, k_, v_, pc.lens, masks, block_table=pc.table, query_seqlens=qs,   # noqa: E731
                                                                          softmax_n_param=o["n"], window=W, **kw_)
    out16, vs_h, want_lse = k8.sixteen_bit_twin(call16, o["q"], k16, v16, o["k_scale"], o["v_scale"], None)
    k8.assert_bitwise(out, out16, vs_h, lse, want_lse, dtype, f"{case} D={D} ({route}, {nsplit} splits)")
    live = [b for b in range(o["B"]) if o["ql"][b] > 0]
    assert torch.isfinite(out).all() and all((out[b, :, :o["ql"][b]] != 0).any() for b in live)
    for b in range(o["B"]):
        assert (out[b, :, o["ql"][b]:] == 0).all() and (lse[b, :, o["ql"][b]:] == float("-inf")).all(), f"{case}: padding rows of batch element {b}"
    if case.startswith("full"):   # bit 63 is a key of some node and node 63 sees something
        assert all(r[63] >> 63 and any(w >> 63 for w in r[:63]) for r in o["rows"])
    if W is not None:
        rows = k8t.poison_below(pc, o["lens"], o["ql"], W)
        assert rows >= 128
        assert _same(call8(), (out, lse)), f"{case}: the result changed when {rows} rows below the window were poisoned"


# ---------------------------------------------------------------- 2. the chain mask is causal attention
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
def test_chain_equals_the_causal_fp8_call_bit_for_bit(pkg, dev, D, dtype):
    """Hidden scores are exact zeros in the sums and the split of the tiles is the base call's: equality with
    flash_attention_n_kvcache_fp8(is_causal=True), and under a window with flash_attention_n_kvcache_fp8_window, is derived, not measured.
    General scales: both sides are FP8 kernels."""
    n = ks._n_values((8,), dev, 2)
    for route in ("decode", "prefill"):
        B, H, Hkv, Sq, page, mp, lens, qlens = (2, 8, 2, 13, 64, 16, [513, 143], None) if route == "decode" else (3, 8, 1, 40, 64, 8, [110, 40, 300], [40, 40, 23])
        r, nsplit = _plan(pkg, dtype, None, B, H, Hkv, Sq, D, page, mp, qlens)
        assert r == route and (nsplit >= 2) == (route == "decode")
        q = ks._rand((B, H, Sq, D), dtype, dev, 31)
        kd, vd = k8.rand_codes((B, Hkv, page * mp, D), 32, dev), k8.rand_codes((B, Hkv, page * mp, D), 33, dev)
        pc = k8.PagedCodes(kd, vd, lens, page, mp, 34)
        k_scale, v_scale = k8.scales_bh(GENERAL, B, Hkv, dev, 35), k8.scales_bh(GENERAL, B, Hkv, dev, 36)
        masks = kt.words_tensor(k8t.rows_of("chain", Sq, B, 0), dev)
        qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
        kw_ = dict(block_table=pc.table, query_seqlens=qs, softmax_n_param=n, return_lse=True)
        want = pkg.flash_attention_n_kvcache_fp8(q, pc.k, pc.v, pc.lens, k_scale, v_scale, is_causal=True, **kw_)
        got = pkg.flash_attention_n_kvcache_fp8_tree(q, pc.k, pc.v, pc.lens, k_scale, v_scale, masks, **kw_)
        assert torch.isfinite(got[0]).all() and (got[0] != 0).any() and _same(got, want), route
        for W in (128, 64):   # (both hold all Sq nodes of the decode case: a window never hides a node's ancestors there)
            if W < Sq:
                continue
            want = pkg.flash_attention_n_kvcache_fp8_window(q, pc.k, pc.v, pc.lens, k_scale, v_scale, W, **kw_)
            got = pkg.flash_attention_n_kvcache_fp8_tree(q, pc.k, pc.v, pc.lens, k_scale, v_scale, masks, window=W, **kw_)
            assert _same(got, want), (route, W)


# ---------------------------------------------------------------- 3. witnesses, where one key decides
def _attend_refs(case, q, kd, vd, k_scale, v_scale, n, scale, rows):
    """per sequence the fp64 reference (kv_witness.attend) on the dequantised cache under the tree rule, and the dequantised V"""
    inp = dict(q=q, kd=k8.up(kd.cpu()).double() * k_scale.cpu().double()[:, :, None, None], vd=k8.up(vd.cpu()).double() * v_scale.cpu().double()[:, :, None, None],
               n=n, scale=scale)
    refs = []
    for b in range(case.B):
        qb, k, v, nb, _ = kw.sequence(case, inp, b)
        ln, ql = case.total[b], case.qlens[b]
        w = kt.tree_vis_brute(ln, ql, ln, rows[b]).double()
        refs.append((kw.attend(qb, k[:, :ln], v[:, :ln], w, nb, scale), v[:, :ln]))
    return refs


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_witness_a_hidden_sibling_would_take_the_row(pkg, dev, route, D, dtype):
    """Node i's query is e_s for a node s it does NOT see (a sibling where it has one); the key of node t is the largest code, 448, in
    feature t; the prefix keys are code 0 in those features. Every visible logit is 0 and the hidden key of s lies 448 k_scale >= 134 nats
    above them: a leak of s replaces the row's output by V_s - a distinct random row - wholesale. The row must be what the visible keys
    alone give: kv_witness.attend in fp64 on the dequantised cache, under witness C's gate (3 u A + 1e-6 per element)."""
    H, Hkv, Sq = (8, 2, 13) if route == "decode" else (8, 1, 40)
    prefix = [0, 60, 128]
    case = kw.Case(route, H, Hkv, D, Sq, [p + Sq for p in prefix])
    assert k8t.route_of(H, Hkv, Sq, None) == route
    gen = torch.Generator().manual_seed(23)
    trees = [kt.random_tree(Sq, gen) for _ in prefix]
    rows = [t[0] for t in trees]
    q = torch.zeros(case.B, H, Sq, D, dtype=dtype, device=dev)
    kd, vd = k8.rand_codes((case.B, Hkv, case.cap, D), 41, dev), k8.rand_codes((case.B, Hkv, case.cap, D), 42, dev)
    kd[..., :Sq] = 0
    hidden = 0
    for b, (words, parents) in enumerate(trees):
        for i in range(Sq):
            sibs = [t for t in range(Sq) if t != i and parents[t] == parents[i]] or [t for t in range(Sq) if not (words[i] >> t) & 1]
            if sibs:
                s = sibs[int(torch.randint(0, len(sibs), (1,), generator=gen))]
                assert not (words[i] >> s) & 1
                q[b, :, i, s] = 1.0
                hidden += 1
            kd[b, :, prefix[b] + i, i] = 0x7E
    assert hidden >= 3 * Sq - 3 and float(k8.up(torch.tensor([0x7E], dtype=torch.uint8))) == 448.0
    k_scale, v_scale = k8.scales_bh((0.3, 3.0, 1.0), case.B, Hkv, dev, 43), k8.scales_bh(GENERAL, case.B, Hkv, dev, 44)
    n = ks._n_values((H,), dev, 45)
    pc = k8.PagedCodes(kd, vd, case.total, case.page, case.max_pages, 46)
    out, lse = pkg.flash_attention_n_kvcache_fp8_tree(q, pc.k, pc.v, pc.lens, k_scale, v_scale, kt.words_tensor(rows, dev), block_table=pc.table,
                                                      softmax_n_param=n, scale=1.0, return_lse=True)
    for b, (ref, _v) in enumerate(_attend_refs(case, q, kd, vd, k_scale, v_scale, n, 1.0, rows)):
        assert (ref["x"][torch.isfinite(ref["x"])] == 0).all()          # every visible logit is 0: the hidden one would be >= 134
        r = kw.gate_c(out[b], ref, dtype)
        print(f"witness A {route} sequence {b}: ratio {r:.3f}")
        assert r <= 1.0, (b, r)
        ks._check_lse(lse[b], ref["lse"].float(), f"witness A {route} lse {b}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_witness_b_only_the_own_key(pkg, dev, route, D, dtype):
    """An empty prefix, every node's word names the node alone, q.k_j = j + 1 exactly and scale = 32 (kv_witness.inputs_b, whose keys are
    e4m3fn numbers: quantised at k_scale = 1 without loss): the row is v_scale V_self / (1 + n e^-x) with x >= 32 nats - the own V row
    times v_scale, over the n term - to two roundings (kv_witness.gate_b)."""
    H, Hkv, Sq = (8, 2, 13) if route == "decode" else (8, 1, 40)
    case = kw.Case(route, H, Hkv, D, Sq, [Sq, Sq])
    inp = kw.inputs_b(case, "ascending", dtype, dev, 51)
    kd = k8.quantise(inp["kd"], 1.0).to(dev)
    assert torch.equal(k8.up(kd), inp["kd"].float())
    vd = k8.rand_codes((case.B, Hkv, case.cap, D), 52, dev)
    vd = (vd & 0x8F) | 0x30   # 0.5 <= |V| < 2: no exact zeros (gate_b bounds them at 1e-30) and, times the smallest v_scale, no fp16 subnormals
    k_scale, v_scale = torch.ones(case.B, Hkv, device=dev), k8.scales_bh(GENERAL, case.B, Hkv, dev, 53)
    rows = k8t.rows_of("self", Sq, case.B, 0)
    pc = k8.PagedCodes(kd, vd, case.total, case.page, case.max_pages, 54)
    out = pkg.flash_attention_n_kvcache_fp8_tree(inp["q"], pc.k, pc.v, pc.lens, k_scale, v_scale, kt.words_tensor(rows, dev), block_table=pc.table,
                                                 softmax_n_param=inp["n"], scale=inp["scale"])
    for b, (ref, v) in enumerate(_attend_refs(case, inp["q"], kd, vd, k_scale, v_scale, inp["n"], inp["scale"], rows)):
        kind, want = kw.expect_b(ref, v, H // Hkv)
        assert (kind == 1).all() and torch.equal(ref["x"].argmax(-1), torch.arange(Sq).expand(H, Sq))
        r = kw.gate_b(out[b], kind, want, dtype)
        print(f"witness B {route} sequence {b}: ratio {r:.3f}")
        assert r <= 1.0, (b, r)


# ---------------------------------------------------------------- 4. general scales against the fp32 reference
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("W", [None, 70])
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_general_scales_against_the_reference(pkg, dev, route, W, D, dtype):
    """scales 0.3, 3.0, 1.7e-3 per (b, hkv): kv_tree.reference_tree on the dequantised visible cache, under kv_support's gates - the ones the
    FP8 general-scale cases already stand under. Under the window the pages below first_b are gone."""
    B, H, Hkv, page, max_pages = 3, 8, 2, 64, 4
    Sq, qlens = (13, None) if route == "decode" else (40, [40, 7, 0])
    assert k8t.route_of(H, Hkv, Sq, qlens) == route
    ql = qlens or [Sq] * B
    lens = [p + x for p, x in zip([200, 135, 60], ql)]
    Smax = page * max_pages
    q = ks._rand((B, H, Sq, D), dtype, dev, 61)
    kd, vd = k8.rand_codes((B, Hkv, Smax, D), 62, dev), k8.rand_codes((B, Hkv, Smax, D), 63, dev)
    pc = k8.PagedCodes(kd, vd, lens, page, max_pages, 64)
    k_scale, v_scale = k8.scales_bh(GENERAL, B, Hkv, dev, 65), k8.scales_bh(GENERAL, B, Hkv, dev, 66)
    n = ks._n_values((B, H), dev, 67)
    rows = k8t.rows_of("tree", Sq, B, 68)
    rows[2] = k8t.rows_of("arbitrary", Sq, 1, 69)[0]
    masks = kt.words_tensor(rows, dev)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    if W is not None:
        assert k8t.poison_below(pc, lens, ql, W) >= 128
    out, lse = pkg.flash_attention_n_kvcache_fp8_tree(q, pc.k, pc.v, pc.lens, k_scale, v_scale, masks, block_table=pc.table, query_seqlens=qs,
                                                      softmax_n_param=n, return_lse=True, window=W)
    o_ref, lse_ref = k8t.reference_fp8_tree(q, kd, vd, lens, ql, n, masks, k_scale, v_scale, W)
    ks._check(out, o_ref, dtype, f"general scales {route} W={W} out")
    ks._check_lse(lse, lse_ref, f"general scales {route} W={W} lse")
    for b in range(B):
        assert (out[b, :, ql[b]:] == 0).all() and (lse[b, :, ql[b]:] == float("-inf")).all()


# ---------------------------------------------------------------- 5. rotary at depth
def _witness_rows(k_new, scales_b0, dtype):
    """row 0 of batch element 0 carries the append's witnesses, spread over the K/V heads and times the head's scale, padded with 1.5"""
    Hkv, D = k_new.shape[1], k_new.shape[3]
    w = k8.append_witnesses(torch.float32)
    assert Hkv * D >= w.numel()
    flat = torch.full((Hkv * D,), 1.5)
    flat[:w.numel()] = w
    k_new[0, :, 0] = (flat.view(Hkv, D) * scales_b0.cpu().view(Hkv, 1)).to(dtype).to(k_new.device)


ROPE_CASES = {"decode": (13, None), "prefill": (40, [40, 7, 40])}   # Sq, qlens


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("route", sorted(ROPE_CASES))
def test_rope_append_bytes_equal_the_quantised_eager_rotation_at_depth(pkg, dev, route, D, dtype):
    """K bytes of the rows cache_seqlens[b] + i, i < qlen_b = quantise(rotate(k_new at cache_seqlens[b] + depth_i).to(dtype), k_scale); V bytes =
    quantise(v_new, v_scale); every other byte of both pools untouched - padding rows, the rows of the last batch element that fall off the
    end of the cache (all but 5), other pages. Batch element 0 is empty and its root (depth 0, position 0: cos 1, sin 0) carries the
    append's witnesses. Half-split and interleaved pairs, rotary_dim D and D / 2, fp32 and 16-bit tables, scales that are no powers of two."""
    Sq, qlens = ROPE_CASES[route]
    B, H, Hkv, page, max_pages = 3, 8, 2, 64, 3
    capacity = page * max_pages
    ql = qlens or [Sq] * B
    lens = [0, 60, capacity - 5]
    assert k8t.route_of(H, Hkv, Sq, qlens) == route
    k_scale = torch.tensor([[1.0, 0.3], [1.7e-3, 3.0], [0.3, 2.0 ** -3]], device=dev)
    v_scale = torch.tensor([[0.3, 1.0], [3.0, 0.7], [16.0, 1.7e-3]], device=dev)
    gen = torch.Generator().manual_seed(71)
    n_pages = B * max_pages + 1
    table = torch.randperm(n_pages, generator=gen)[:B * max_pages].view(B, max_pages).to(torch.int32).to(dev)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    rows = k8t.rows_of("tree", Sq, B, 72)
    masks = kt.words_tensor(rows, dev)
    dep = kt.depths(masks, ql)
    assert dep[0, 0] == 0 and not torch.equal(dep, torch.arange(Sq).expand(B, Sq))   # depth != index
    pos = torch.tensor(lens).view(B, 1) + dep
    q = ks._rand((B, H, Sq, D), dtype, dev, 73)
    for interleaved, rd, fp32 in ((False, D, True), (True, D // 2, False), (False, D // 2, False), (True, D, True)):
        what = f"{route} interleaved={interleaved} rotary_dim={rd} fp32 tables={fp32}"
        ku = torch.randint(0, 256, (n_pages, page, Hkv, D), generator=gen, dtype=torch.int32).to(torch.uint8).to(dev)
        vu = torch.randint(0, 256, (n_pages, page, Hkv, D), generator=gen, dtype=torch.int32).to(torch.uint8).to(dev)
        k_new = (ks._rand((B, Hkv, Sq, D), torch.float32, dev, 74, std=1.0) * k_scale[:, :, None, None] * 40.0).to(dtype)
        v_new = (ks._rand((B, Hkv, Sq, D), torch.float32, dev, 75, std=1.0) * v_scale[:, :, None, None] * 40.0).to(dtype)
        _witness_rows(k_new, k_scale[0], dtype)
        _witness_rows(v_new, v_scale[0], dtype)
        assert torch.isnan(k_new[0, :, 0]).any() and torch.isinf(k_new[0, :, 0]).any()
        cos, sin = ks._tables(capacity, rd, dev, torch.float32 if fp32 else dtype)
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
                pid = int(table[b, p // page])
                want_k[pid, p % page] = codes_k[b, :, i]
                want_v[pid, p % page] = codes_v[b, :, i]
                written += 1
        assert dropped == ql[2] - 5 and written == sum(ql) - dropped
        pkg.flash_attention_n_kvcache_fp8_tree(q, ku.view(k8.F8), vu.view(k8.F8), lens_t, k_scale, v_scale, masks, block_table=table, k_new=k_new,
                                               v_new=v_new, query_seqlens=qs, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved)
        assert lens_t.tolist() == lens
        for name, got, want in (("k", ku.cpu(), want_k), ("v", vu.cpu(), want_v)):
            nan = k8.is_nan_code(want)
            assert k8.is_nan_code(got[nan]).all(), f"{what} {name}: a NaN code of the reference is no NaN code in the cache"
            diff = (got != want) & ~nan
            assert not diff.any(), (f"{what} {name}: {int(diff.sum())} bytes differ, first at {diff.nonzero()[0].tolist()}: "
                                    f"got {int(got[diff][0]):#x}, want {int(want[diff][0]):#x}")
        # the witnesses did their work: saturation codes, subnormal codes and both zeros among the codes of the root of batch element 0
        fresh = torch.cat([codes_v[0, :, 0].flatten(), codes_k[0, :, 0].flatten()])
        assert (fresh == 0x7E).any() and (fresh == 0xFE).any() and (fresh == 0x00).any() and (fresh == 0x80).any() and ((fresh > 0) & (fresh < 8)).any()
        if rd < D:   # the unrotated features are quantised, not copied
            assert torch.equal(codes_k[0, :, 0, rd:], k8.quantise(k_new[0, :, 0, rd:], k_scale.cpu()[0, :, None]))
        # ... and the rows were rotated at the depth, not at the index
        by_index = k8.quantise(ks._rotate(k_new, torch.tensor(lens).view(B, 1) + torch.arange(Sq).view(1, Sq), cos, sin, interleaved).to(dtype),
                               k_scale.cpu()[:, :, None, None])
        assert not torch.equal(by_index[1, :, :ql[1]], codes_k[1, :, :ql[1]])


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("W", [None, 96])
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_rope_call_equals_eager_rotation_at_depth_then_the_call_without_tables(pkg, dev, route, W, D, dtype):
    """out, lse and both pools of flash_attention_n_kvcache_fp8_tree(rotary tables) = those of the same call without tables on a clone of the
    cache, with query and k_new rotated at the depth positions by eager torch (rounded to dtype), under scales that are no powers of two;
    likewise without k_new / v_new (the queries only). A self-only batch element with n > 0 is among them: there q decides the row
    through the sink's share, so a query rotated elsewhere shows."""
    B, H, Hkv, page, max_pages = 3, 8, 2, 64, 4
    Sq, qlens = (13, None) if route == "decode" else (40, [40, 0, 17])
    assert k8t.route_of(H, Hkv, Sq, qlens) == route
    ql = qlens or [Sq] * B
    lens = [150, 64, 201]
    Smax = page * max_pages
    kd, vd = k8.rand_codes((B, Hkv, Smax, D), 82, dev), k8.rand_codes((B, Hkv, Smax, D), 83, dev)
    pc = k8.PagedCodes(kd, vd, [ln + Sq for ln in lens], page, max_pages, 84)   # (the pages the appended rows land in are there)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    k_scale, v_scale = k8.scales_bh(GENERAL, B, Hkv, dev, 85), k8.scales_bh(GENERAL, B, Hkv, dev, 86)
    n = ks._n_values((B, H), dev, 8, zeros=False)
    q = ks._rand((B, H, Sq, D), dtype, dev, 87)
    k_new, v_new = ks._rand((B, Hkv, Sq, D), dtype, dev, 88, std=1.0), ks._rand((B, Hkv, Sq, D), dtype, dev, 89, std=1.0)
    rows = k8t.rows_of("tree", Sq, B, 90)
    rows[2] = k8t.rows_of("self", Sq, 1, 0)[0]
    masks = kt.words_tensor(rows, dev)
    dep = kt.depths(masks, ql)
    interleaved, rd = (D == 128), (D if dtype == torch.float16 else D // 2)
    cos, sin = ks._tables(Smax, rd, dev, torch.float32 if route == "decode" else dtype)

    def call(kc, vc, q_, kn, vn, **kw_):
        return pkg.flash_attention_n_kvcache_fp8_tree(q_, kc.view(k8.F8), vc.view(k8.F8), lens_t, k_scale, v_scale, masks, block_table=pc.table, k_new=kn,
                                                      v_new=vn, query_seqlens=qs, softmax_n_param=n, return_lse=True, window=W, **kw_)

    for append in (True, False):
        what = f"{route} W={W} append={append}"
        ka_, va_ = pc.ku.clone(), pc.vu.clone()
        kb_, vb_ = pc.ku.clone(), pc.vu.clone()
        got = call(ka_, va_, q, k_new if append else None, v_new if append else None, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved)
        # p_i = base_b + depth_i, base_b = len_b - qlen_b, len_b = cache_seqlens[b] + (qlen_b if appended else 0); the keys: cache_seqlens[b] + depth_i
        p_q = dep + torch.tensor([ln + (0 if append else -ql[b]) for b, ln in enumerate(lens)]).view(B, 1)
        q_rot = ks._rotate(q, p_q, cos, sin, interleaved)
        k_rot = ks._rotate(k_new, dep + torch.tensor(lens).view(B, 1), cos, sin, interleaved) if append else None
        want = call(kb_, vb_, q_rot, k_rot, v_new if append else None)
        live = torch.tensor([x > 0 for x in ql], device=dev)
        assert torch.isfinite(got[0]).all() and (got[0][live] != 0).any()
        assert torch.equal(ks._bits(got[0]), ks._bits(want[0])), f"{what}: out differs at {int((ks._bits(got[0]) != ks._bits(want[0])).sum())} elements"
        assert torch.equal(got[1], want[1]), f"{what}: lse differs"
        assert torch.equal(ka_, kb_) and torch.equal(va_, vb_), f"{what}: the pools differ"
        assert torch.equal(ka_, pc.ku) != append, what   # the append wrote, the queries-only call did not
        if append:   # the self-only element: a query rotated one position further gives another row
            off = call(pc.ku.clone(), pc.vu.clone(), ks._rotate(q, p_q + 1, cos, sin, interleaved), k_rot, v_new)
            assert not torch.equal(ks._bits(off[0][2]), ks._bits(got[0][2]))


# ---------------------------------------------------------------- 6. commit
def _commit_reference(k, v, table, page, base, accepted, alens):
    """on the host, through a temporary: all the sources are read before any destination is written"""
    k2, v2 = k.clone(), v.clone()
    for b, (bs, path, alen) in enumerate(zip(base, accepted, alens)):
        for kk in range(alen):
            src, dst = bs + path[kk], bs + kk
            ps, pd = (int(table[b, src // page]), int(table[b, dst // page])) if table is not None else (b, b)
            k2[pd, dst % page], v2[pd, dst % page] = k[ps, src % page], v[ps, src % page]
    return k2, v2


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("paged", [True, False], ids=["paged", "dense"])
def test_commit(pkg, dev, paged, D):
    """the uint8 views of both pools byte for byte against the move on the host: the overlapping chain (row 2 is a source and a destination),
    the identity (accepted[b, k] == k moves nothing), an empty path, a path that crosses a page edge and ends at node Sq - 1; every byte
    outside the destination rows [base_b, base_b + alen_b) unchanged; then malformed paths (an index below k, beyond the nodes, decreasing,
    a length beyond A) leave memory outside those rows unchanged. cache_seqlens is not modified."""
    Sq, Hkv, page, mp = 16, 2, 64, 3
    base = [60, 5, 0, 128 - 3]
    accepted = [[0, 2, 3, 7], [0, 1, 2, 3], [0, 5, 9, 11], [0, 4, 9, 15]]
    alens = [4, 4, 0, 4]
    B = len(base)
    gen = torch.Generator().manual_seed(91)
    n_pages = B * mp + 2 if paged else B
    rows_per = page if paged else page * mp
    ku = torch.randint(0, 256, (n_pages, rows_per, Hkv, D), generator=gen, dtype=torch.int32).to(torch.uint8).to(dev)
    vu = torch.randint(0, 256, (n_pages, rows_per, Hkv, D), generator=gen, dtype=torch.int32).to(torch.uint8).to(dev)
    table = torch.randperm(n_pages, generator=gen)[:B * mp].view(B, mp).to(torch.int32).to(dev) if paged else None
    tbl = None if table is None else table.cpu()
    k_ref, v_ref = _commit_reference(ku.cpu(), vu.cpu(), tbl, rows_per, base, accepted, alens)
    before_k, before_v = ku.cpu().clone(), vu.cpu().clone()
    assert not torch.equal(k_ref, before_k)

    def row_of(b, pos):
        return (int(tbl[b, pos // page]) if paged else b), pos % rows_per

    for b in (1, 2):   # the identity and the empty path move nothing
        for kk in range(4):
            pid, r = row_of(b, base[b] + kk)
            assert torch.equal(k_ref[pid, r], before_k[pid, r]) and torch.equal(v_ref[pid, r], before_v[pid, r])
    sl = torch.tensor(base, dtype=torch.int32, device=dev)
    pkg.flash_attention_n_kvcache_fp8_tree_commit(ku.view(k8.F8), vu.view(k8.F8), sl, torch.tensor(accepted, dtype=torch.int32, device=dev),
                                                  torch.tensor(alens, dtype=torch.int32, device=dev), block_table=table)
    assert torch.equal(ku.cpu(), k_ref) and torch.equal(vu.cpu(), v_ref)
    assert sl.tolist() == base
    allowed = torch.zeros(n_pages, rows_per, dtype=torch.bool)
    for b, bs in enumerate(base):
        for kk in range(alens[b]):
            allowed[row_of(b, bs + kk)] = True
    changed = (ku.cpu() != before_k).any(-1).any(-1) | (vu.cpu() != before_v).any(-1).any(-1)   # [pages, rows]
    assert changed.any() and not (changed & ~allowed).any()
    # malformed paths
    before_k, before_v = ku.cpu().clone(), vu.cpu().clone()
    bad = torch.tensor([[3, 0, 99, -4], [0, 1, 2, 3], [70, 70, 70, 70], [5, 4, 3, 2]], dtype=torch.int32, device=dev)
    pkg.flash_attention_n_kvcache_fp8_tree_commit(ku.view(k8.F8), vu.view(k8.F8), sl, bad, torch.tensor([99, -3, 4, 4], dtype=torch.int32, device=dev),
                                                  block_table=table)
    changed = (ku.cpu() != before_k).any(-1).any(-1) | (vu.cpu() != before_v).any(-1).any(-1)
    allowed = torch.zeros_like(changed)
    for b, bs in enumerate(base):
        for kk in range(4):
            allowed[row_of(b, bs + kk)] = True
    assert not (changed & ~allowed).any() and sl.tolist() == base


# ---------------------------------------------------------------- 7. end to end
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("D", DIMS)
def test_end_to_end_verify_commit_advance_decode(pkg, dev, D, dtype):
    """verify a random tree with k_new and rotary, commit a root-to-leaf path, advance cache_seqlens, then one decode step with
    flash_attention_n_kvcache_fp8_rope: out and lse equal, bit for bit, the same step on a cache that was filled with the accepted tokens
    directly (one flash_attention_n_kvcache_fp8_rope chunk of the path's tokens at consecutive positions), and so do the visible code rows."""
    B, H, Hkv, Sq, page, mp = 2, 8, 2, 16, 64, 4
    prefix = [60, 131]
    gen = torch.Generator().manual_seed(101)
    trees = [kt.random_tree(Sq, gen) for _ in range(B)]
    masks = kt.words_tensor([t[0] for t in trees], dev)
    paths = []
    for words, parents in trees:
        leaf = max(range(Sq), key=lambda i: (kt.depth(words[i], Sq), i))
        path = [t for t in range(Sq) if (words[leaf] >> t) & 1]
        assert path[0] == 0 and path[-1] == leaf and all(parents[b_] == a_ for a_, b_ in zip(path, path[1:]))
        paths.append(path)
    A = max(len(p) for p in paths)
    assert A >= 3 and any(p != list(range(len(p))) for p in paths)
    acc = torch.tensor([p + [0] * (A - len(p)) for p in paths], dtype=torch.int32, device=dev)
    alens = torch.tensor([len(p) for p in paths], dtype=torch.int32, device=dev)
    n = ks._n_values((H,), dev, 102)
    k_scale, v_scale = k8.scales_bh(GENERAL, B, Hkv, dev, 103), k8.scales_bh(GENERAL, B, Hkv, dev, 104)
    q, kn, vn = ks._rand((B, H, Sq, D), dtype, dev, 105), ks._rand((B, Hkv, Sq, D), dtype, dev, 106, std=1.0), ks._rand((B, Hkv, Sq, D), dtype, dev, 107, std=1.0)
    cos, sin = ks._tables(page * mp, D, dev, torch.float32)
    kd, vd = k8.rand_codes((B, Hkv, page * mp, D), 108, dev), k8.rand_codes((B, Hkv, page * mp, D), 109, dev)
    pa, pb = (k8.PagedCodes(kd, vd, [p + Sq for p in prefix], page, mp, 110) for _ in range(2))
    for pc in (pa, pb):   # the rows behind the prefix are stale: NaN codes until something is appended
        for b in range(B):
            for pos in range(prefix[b], prefix[b] + Sq):
                pc.ku[int(pc.table[b, pos // page]), pos % page] = k8.NAN_CODE
                pc.vu[int(pc.table[b, pos // page]), pos % page] = k8.NAN_CODE
    sl_a = torch.tensor(prefix, dtype=torch.int32, device=dev)
    out = pkg.flash_attention_n_kvcache_fp8_tree(q, pa.k, pa.v, sl_a, k_scale, v_scale, masks, block_table=pa.table, k_new=kn, v_new=vn, softmax_n_param=n,
                                                 rotary_cos=cos, rotary_sin=sin)
    assert torch.isfinite(out).all()
    pkg.flash_attention_n_kvcache_fp8_tree_commit(pa.k, pa.v, sl_a, acc, alens, block_table=pa.table)
    assert sl_a.tolist() == prefix
    sl_a += alens
    # the direct route: the accepted tokens as one chunk at consecutive positions
    idx = acc.long()[:, None, :, None]
    kn_acc, vn_acc = kn.gather(2, idx.expand(B, Hkv, A, D)), vn.gather(2, idx.expand(B, Hkv, A, D))
    q_acc = q.gather(2, idx.expand(B, H, A, D))
    sl_b = torch.tensor(prefix, dtype=torch.int32, device=dev)
    direct = pkg.flash_attention_n_kvcache_fp8_rope(q_acc, pb.k, pb.v, sl_b, k_scale, v_scale, cos, sin, block_table=pb.table, k_new=kn_acc, v_new=vn_acc,
                                                    query_seqlens=alens, softmax_n_param=n)
    sl_b += alens
    final = sl_a.tolist()
    assert final == [p + len(path) for p, path in zip(prefix, paths)] == sl_b.tolist()
    for pool_a, pool_b in ((pa.ku, pb.ku), (pa.vu, pb.vu)):
        assert torch.equal(ks._gather(pool_a, pa.table, final, page), ks._gather(pool_b, pb.table, final, page))
    for b, path in enumerate(paths):   # the accepted nodes saw what the chunk's positions see: the same rows up to the gates
        ks._check(out[b, :, path], direct[b, :, :len(path)], dtype, f"end to end: sequence {b} accepted nodes")
    # one decode step on both caches
    q1, k1, v1 = ks._rand((B, H, 1, D), dtype, dev, 111), ks._rand((B, Hkv, 1, D), dtype, dev, 112, std=1.0), ks._rand((B, Hkv, 1, D), dtype, dev, 113, std=1.0)
    step = lambda pc, sl: pkg.flash_attention_n_kvcache_fp8_rope(q1, pc.k, pc.v, sl, k_scale, v_scale, cos, sin, block_table=pc.table, k_new=k1, v_new=v1,   # noqa: E731
                                                                 softmax_n_param=n, return_lse=True)
    got, want = step(pa, sl_a), step(pb, sl_b)
    assert torch.isfinite(got[0]).all() and (got[0] != 0).any() and _same(got, want)


# ---------------------------------------------------------------- 8. graph replay
@pytest.mark.parametrize("route", ["decode", "prefill"])
def test_graph_replay_follows_the_device_operands(pkg, dev, route):
    """one captured graph per route - the tree call with k_new, rotary and a window, then the commit; tree_mask, cache_seqlens, the scales, the
    accepted path and the cache change in place between replays; each replay equals the eager call on the same operands, pools included"""
    dtype, D = torch.bfloat16, 64
    B, H, Hkv, Sq, page, mp = (2, 8, 2, 13, 64, 4) if route == "decode" else (2, 8, 1, 40, 64, 4)
    assert _plan(pkg, dtype, 100, B, H, Hkv, Sq, D, page, mp)[0] == route
    q, kn, vn = ks._rand((B, H, Sq, D), dtype, dev, 121), ks._rand((B, Hkv, Sq, D), dtype, dev, 122, std=1.0), ks._rand((B, Hkv, Sq, D), dtype, dev, 123, std=1.0)
    kd, vd = k8.rand_codes((B, Hkv, page * mp, D), 124, dev), k8.rand_codes((B, Hkv, page * mp, D), 125, dev)
    cos, sin = ks._tables(page * mp, D, dev, torch.float32)
    pc = k8.PagedCodes(kd, vd, [page * mp] * B, page, mp, 126)     # every row finite: the lengths move freely
    pool_k, pool_v = pc.ku.clone(), pc.vu.clone()
    sl = torch.tensor([60, 131], dtype=torch.int32, device=dev)
    masks = kt.words_tensor(k8t.rows_of("tree", Sq, B, 127), dev)
    k_scale, v_scale = torch.tensor([[1.0] * Hkv, [0.3] * Hkv], device=dev), torch.full((Hkv,), 0.7, device=dev)
    acc = torch.tensor([[0, 2, 5], [0, 1, 4]], dtype=torch.int32, device=dev)
    alens = torch.tensor([3, 2], dtype=torch.int32, device=dev)

    def step():
        o = pkg.flash_attention_n_kvcache_fp8_tree(q, pc.k, pc.v, sl, k_scale, v_scale, masks, block_table=pc.table, k_new=kn, v_new=vn, softmax_n_param=0.5,
                                                   return_lse=True, rotary_cos=cos, rotary_sin=sin, window=100)
        pkg.flash_attention_n_kvcache_fp8_tree_commit(pc.k, pc.v, sl, acc, alens, block_table=pc.table)
        return o

    g, res = ks._capture(step)
    seen = []
    for new_sl, seed, new_acc, new_alens, ksc, vsc in (([60, 131], 127, [[0, 2, 5], [0, 1, 4]], [3, 2], 1.0, [0.7] * Hkv),
                                                       ([3, 190], 128, [[0, 1, 2], [0, 3, 9]], [1, 3], 1.7, [0.1, 4.0][:Hkv])):
        sl.copy_(torch.tensor(new_sl, dtype=torch.int32))
        masks.copy_(kt.words_tensor(k8t.rows_of("tree" if seed == 127 else "arbitrary", Sq, B, seed)))
        acc.copy_(torch.tensor(new_acc, dtype=torch.int32))
        alens.copy_(torch.tensor(new_alens, dtype=torch.int32))
        k_scale.copy_(torch.tensor([[1.0] * Hkv, [0.3] * Hkv]) * ksc)
        v_scale.copy_(torch.tensor(vsc))
        pc.ku.copy_(pool_k if seed == 127 else pool_v), pc.vu.copy_(pool_v if seed == 127 else pool_k)   # (the cache changes in place too)
        start_k, start_v = pc.ku.clone(), pc.vu.clone()
        g.replay()
        got, got_k, got_v = [t.clone() for t in res], pc.ku.clone(), pc.vu.clone()
        pc.ku.copy_(start_k), pc.vu.copy_(start_v)
        want = step()
        assert torch.isfinite(got[0]).all() and (got[0] != 0).any() and _same(got, want)
        assert torch.equal(got_k, pc.ku) and torch.equal(got_v, pc.vu) and not torch.equal(got_k, start_k)
        seen.append(got)
    assert not _same(seen[0], seen[1])


# ---------------------------------------------------------------- 9. determinism
@pytest.mark.parametrize("case", ["decode_arbitrary", "prefill_arbitrary", "split_decode", "split_prefill"])
def test_deterministic(pkg, dev, case):
    dtype, D = torch.bfloat16, 128
    o = k8t.twin_operands(case, D, dtype, dev)
    _route, nsplit = _plan(pkg, dtype, None, o["B"], o["H"], o["Hkv"], o["Sq"], D, o["page"], o["max_pages"], o["qlens"])
    assert (nsplit > 1) == case.startswith("split")
    pc = k8.PagedCodes(o["kd"], o["vd"], o["lens"], o["page"], o["max_pages"], 5)
    masks = kt.words_tensor(o["rows"], dev)
    qs = None if o["qlens"] is None else torch.tensor(o["qlens"], dtype=torch.int32, device=dev)
    runs = [pkg.flash_attention_n_kvcache_fp8_tree(o["q"], pc.k, pc.v, pc.lens, o["k_scale"], o["v_scale"], masks, block_table=pc.table, query_seqlens=qs,
                                                   softmax_n_param=0.25, return_lse=True) for _ in range(2)]
    assert _same(runs[0], runs[1])
    assert math.isfinite(runs[0][0].float().abs().sum().item()) and (runs[0][0] != 0).any()
