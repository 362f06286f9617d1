"""flash_attention_n_kvcache_rope on the GPU: rotary position embedding fused into the append of the K/V-cache calls.

The test's rotation is eager torch in fp32, rounded once to the dtype: (x1.float() * cos.float() - x2.float() * sin.float()).to(dtype) and
(x2.float() * cos.float() + x1.float() * sin.float()).to(dtype) - the arithmetic the kernel pins. Every case runs two routes on clones of one
cache pool: R, the new call, and T, the existing call fed the torch-rotated q and k_new. It asserts
  (a) the two pools are equal bit for bit as wholes (int16 views): the new rows are the rotated rows, v is copied, nothing else changed;
  (b) out and lse of R equal those of T bit for bit (the same forward kernels on the same bits);
  (c) R is within the cache tests' gates (REF_ATOL / REL_TRUE on out, 1e-4 on lse; imported) of their fp32 reference on the rotated inputs;
  (d) cache_seqlens is unchanged.
Positions: key row i of batch element b sits at lens[b] + i; query i at p_i = i + len_b - qlen_b with len_b = min(lens[b] + qlen_b, capacity)
after an append (lens[b] without one) - computed here on the host from the lists the device tensors were made of."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_support as ks   # noqa: E402

pytestmark = pytest.mark.gpu

NAN = ks.NAN
_rand, _check, _check_lse, _Paged, _n_values, _tables, _rotate, _bits = (
    ks._rand, ks._check, ks._check_lse, ks._Paged, ks._n_values, ks._tables, ks._rotate, ks._bits)
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
MAX_ROWS = 128   # rows of the decode kernels: the dispatch rule of the window function


def _both_routes(pkg, q, kn, vn, k0, v0, sl, cos, sin, q_rot, k_rot, table=None, qs=None, window=None, causal=True, n=1.0, interleaved=False,
                 what=""):
    """R and T on clones of (k0, v0); asserts (a), (b), (d); returns R's out, lse and pools"""
    B, H, Sq, D = q.shape
    G = H // k0.shape[2]
    sl0 = sl.clone()
    kR, vR = k0.clone(), v0.clone()
    out, lse = pkg.flash_attention_n_kvcache_rope(q, kR, vR, sl, cos, sin, block_table=table, k_new=kn, v_new=vn, query_seqlens=qs,
                                                  softmax_n_param=n, is_causal=causal, return_lse=True, window=window,
                                                  rotary_interleaved=interleaved)
    assert torch.equal(sl, sl0), f"{what}: cache_seqlens was modified"
    kT, vT = k0.clone(), v0.clone()
    if window is not None:
        o_t, l_t = pkg.flash_attention_n_kvcache_window(q_rot, kT, vT, sl, window, block_table=table, k_new=k_rot, v_new=vn, query_seqlens=qs,
                                                        softmax_n_param=n, return_lse=True)
    elif qs is None and G * Sq <= MAX_ROWS:
        o_t, l_t = pkg.flash_attention_n_kvcache(q_rot, kT, vT, sl, block_table=table, k_new=k_rot, v_new=vn, softmax_n_param=n,
                                                 is_causal=causal, return_lse=True)
    else:
        o_t, l_t = pkg.flash_attention_n_kvcache_prefill(q_rot, kT, vT, sl, block_table=table, k_new=k_rot, v_new=vn, query_seqlens=qs,
                                                         softmax_n_param=n, is_causal=causal, return_lse=True)
    torch.cuda.synchronize()
    dk = (_bits(kR) != _bits(kT)).sum().item()
    dv = (_bits(vR) != _bits(vT)).sum().item()
    do = (_bits(out) != _bits(o_t)).sum().item()
    dl = (lse.view(torch.int32) != l_t.view(torch.int32)).sum().item()
    print(f"{what}: elements that differ between the routes: k pool {dk}, v pool {dv}, out {do}, lse {dl}")
    assert torch.equal(_bits(kR), _bits(kT)), f"{what}: k pools differ in {dk} elements"
    assert torch.equal(_bits(vR), _bits(vT)), f"{what}: v pools differ in {dv} elements"
    assert torch.equal(_bits(out), _bits(o_t)), f"{what}: out differs from the torch-rotated route in {do} elements"
    assert torch.equal(lse.view(torch.int32), l_t.view(torch.int32)), f"{what}: lse differs from the torch-rotated route in {dl} elements"
    return out, lse, kR, vR


def _run(pkg, dev, B, H, Hkv, Sq, D, dtype, page, max_pages, lens, seed, qlens=None, rd=None, table_dtype=torch.float32, interleaved=False,
         window=None, causal=True, n=1.0, shared=False, nan_pad=False, extra_rows=0, nan_table_tail=False, guard=None, fused=False,
         prefill=False, what=""):
    """One paged case with an append: builds the inputs, runs both routes, checks R against the fp32 reference on the rotated inputs"""
    cap = page * max_pages
    rd = rd or D
    ql = qlens or [Sq] * B
    if fused:   # q, k_new, v_new as views of one [B, Sq, (H + 2 Hkv) D] buffer
        buf = _rand((B, Sq, (H + 2 * Hkv) * D), dtype, dev, seed)
        q = buf[..., :H * D].view(B, Sq, H, D).permute(0, 2, 1, 3)
        kn = buf[..., H * D:(H + Hkv) * D].view(B, Sq, Hkv, D).permute(0, 2, 1, 3)
        vn = buf[..., (H + Hkv) * D:].view(B, Sq, Hkv, D).permute(0, 2, 1, 3)
        assert not q.is_contiguous() and not kn.is_contiguous()
    else:
        nb = 1 if shared else B   # shared: every batch element carries the same rows - only the device length can make the results differ
        q = _rand((nb, H, Sq, D), dtype, dev, seed).expand(B, H, Sq, D).contiguous()
        kn = _rand((nb, Hkv, Sq, D), dtype, dev, seed + 1).expand(B, Hkv, Sq, D).contiguous()
        vn = _rand((nb, Hkv, Sq, D), dtype, dev, seed + 2, std=1.0).expand(B, Hkv, Sq, D).contiguous()
    if nan_pad:
        for b in range(B):
            q[b, :, ql[b]:] = NAN
            kn[b, :, ql[b]:] = NAN
            vn[b, :, ql[b]:] = NAN
    rows = cap + extra_rows
    if fused:   # the tables as a slice of a longer and wider table
        big_c, big_s = (torch.full((rows + 9, rd), NAN, dtype=table_dtype, device=dev) for _ in range(2))
        c0, s0 = _tables(rows, rd, dev, table_dtype)
        big_c[5:5 + rows, :rd // 2], big_s[5:5 + rows, :rd // 2] = c0, s0
        cos, sin = big_c[5:5 + rows, :rd // 2], big_s[5:5 + rows, :rd // 2]
        assert not cos.is_contiguous()
    else:
        cos, sin = _tables(rows, rd, dev, table_dtype)
    if nan_table_tail:
        cos[cap:], sin[cap:] = NAN, NAN
    kd = _rand((B, Hkv, cap, D), dtype, dev, seed + 3)
    vd = _rand((B, Hkv, cap, D), dtype, dev, seed + 4, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, seed, alloc_all=True, guard=guard)   # rows at or beyond the length: NaN until the append writes them
    total = [min(cap, ln + qn) for ln, qn in zip(lens, ql)]
    i = torch.arange(Sq)[None]
    kpos = torch.tensor(lens)[:, None] + i
    qpos = i + torch.tensor(total)[:, None] - torch.tensor(ql)[:, None]
    q_rot, k_rot = _rotate(q, qpos, cos, sin, interleaved), _rotate(kn, kpos, cos, sin, interleaved)
    for b in range(B):   # the dense picture of the cache after the append
        m = max(0, min(ql[b], cap - lens[b]))
        kd[b, :, lens[b]:lens[b] + m] = k_rot[b, :, :m]
        vd[b, :, lens[b]:lens[b] + m] = vn[b, :, :m]
    if window is not None:
        assert ks._poison(pc.k, pc.v, pc.table, page, pc.poison, total, ql, window) > 0
    qs = torch.tensor(ql, dtype=torch.int32, device=dev) if (qlens is not None or prefill) else None
    out, lse, kR, vR = _both_routes(pkg, q, kn, vn, pc.k, pc.v, pc.lens, cos, sin, q_rot, k_rot, table=pc.table, qs=qs, window=window,
                                    causal=causal, n=n, interleaved=interleaved, what=what)
    kg, vg = ks._visible_dense(kd, total), ks._visible_dense(vd, total)
    if window is not None:
        o_ref, l_ref = ks.reference_rows(q_rot, kg, vg, total, ql, n, window)
    else:
        o_ref, l_ref = ks.reference_rows(q_rot, kg, vg, total, ql, n, causal)
    _check(out, o_ref, dtype, f"{what} out")
    _check_lse(lse, l_ref, f"{what} lse")
    for b in range(B):   # padding: exactly 0 / -inf
        assert (out[b, :, ql[b]:] == 0).all() and (lse[b, :, ql[b]:] == float("-inf")).all(), f"{what}: padding rows of batch element {b}"
    return out, lse, kR, vR, pc


# ---------------------------------------------------------------- 1. decode, paged: 61 + 3 rows cross a tile and a page boundary
@pytest.mark.parametrize("rd", [64, 32])
@pytest.mark.parametrize("layout", ["half", "interleaved"])
@pytest.mark.parametrize("tables", ["fp32", "16bit"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_decode_paged(pkg, dev, dtype, tables, layout, rd):
    dt = DTYPES[dtype]
    out, _lse, _k, _v, _pc = _run(pkg, dev, 3, 8, 2, 3, 64, dt, 64, 4, [0, 61, 130], 100, rd=rd, table_dtype=torch.float32 if tables == "fp32" else dt,
                                  interleaved=layout == "interleaved", shared=True, what=f"decode {dtype} tables={tables} {layout} rd={rd}")
    assert torch.isfinite(out).all()


# ---------------------------------------------------------------- 2. all head dims, rotary_dim = D and 16
@pytest.mark.parametrize("part", ["full", "16"])
@pytest.mark.parametrize("D", [32, 128, 256])
def test_head_dims(pkg, dev, D, part):
    dt = {32: torch.float16, 128: torch.bfloat16, 256: torch.float16}[D]
    _run(pkg, dev, 3, 8, 2, 3, D, dt, 64, 4, [0, 61, 130], 200 + D, rd=D if part == "full" else 16, table_dtype=torch.float32 if D != 128 else dt,
         interleaved=(D == 256) != (part == "16"), shared=True, n=_n_values((8,), dev, 201), what=f"D={D} rotary_dim={part}")


# ---------------------------------------------------------------- 3. capacity: rows beyond it are dropped, the tables beyond it never read
def test_capacity(pkg, dev):
    page, max_pages = 64, 2
    cap = page * max_pages
    out, lse, kR, vR, pc = _run(pkg, dev, 2, 8, 2, 3, 64, torch.bfloat16, page, max_pages, [cap - 1, cap - 2], 300, extra_rows=8,
                                nan_table_tail=True, guard=7.0, what="capacity")
    assert (kR[-1] == 7.0).all() and (vR[-1] == 7.0).all(), "guard page behind the pool was written"
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    # one row of element 0 and two of element 1 landed: everything else is what it was
    changed = (_bits(kR) != _bits(pc.k)).flatten(2).any(-1)   # [page, row]
    assert changed.sum().item() == 3, changed.sum().item()


# ---------------------------------------------------------------- 4. prefill, ragged: three row blocks of 32 positions, padding rows NaN
@pytest.mark.parametrize("layout,tables", [("half", "fp32"), ("interleaved", "16bit")])
def test_prefill_ragged(pkg, dev, layout, tables):
    dt = torch.bfloat16
    _run(pkg, dev, 3, 8, 2, 70, 128, dt, 64, 3, [0, 100, 64], 400, qlens=[70, 33, 0], table_dtype=torch.float32 if tables == "fp32" else dt,
         interleaved=layout == "interleaved", nan_pad=True, what=f"prefill ragged {layout} tables={tables}")


# ---------------------------------------------------------------- 5. a sliding window: decode and prefill kernels, the rows below it poisoned
@pytest.mark.parametrize("call", ["decode", "prefill"])
def test_window(pkg, dev, call):
    Sq = 3 if call == "decode" else 70
    _run(pkg, dev, 2, 8, 2, Sq, 64, torch.bfloat16, 64, 6, [200, 70], 500, window=64, n=_n_values((8,), dev, 501), what=f"window {call}")


# ---------------------------------------------------------------- 6. queries only, on a dense cache
@pytest.mark.parametrize("kernels", ["decode", "prefill"])
@pytest.mark.parametrize("causal", [True, False])
def test_query_only_dense(pkg, dev, causal, kernels):
    dtype, B, H, Hkv, Sq, D, cap = torch.float16, 3, 8, 2, 3, 64, 150   # (a dense capacity need not be a multiple of 64)
    lens = [150, 61, 1]                                              # one key under three positions: p_i = -2, -1, 0 - the clamp at row 0
    q = _rand((B, H, Sq, D), dtype, dev, 600)
    kc = _rand((B, cap, Hkv, D), dtype, dev, 601)
    vc = _rand((B, cap, Hkv, D), dtype, dev, 602, std=1.0)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    keep = torch.arange(cap, device=dev).view(1, -1, 1, 1) < sl.view(-1, 1, 1, 1)
    kg, vg = (torch.where(keep, t, torch.zeros_like(t)).permute(0, 2, 1, 3).contiguous() for t in (kc, vc))
    for b, ln in enumerate(lens):   # rows at or beyond len_b: NaN
        kc[b, ln:] = NAN
        vc[b, ln:] = NAN
    cos, sin = _tables(cap, 32, dev, torch.float32)
    cos[0], sin[0] = 0.5, 0.25   # (row 0 of a real table is the identity: make the clamped rows count)
    qpos = torch.arange(Sq)[None] + torch.tensor(lens)[:, None] - Sq
    q_rot = _rotate(q, qpos, cos, sin, False)
    assert not torch.equal(q_rot[2, :, 0], q[2, :, 0])
    qs = torch.full((B,), Sq, dtype=torch.int32, device=dev) if kernels == "prefill" else None
    what = f"query only causal={causal} {kernels}"
    out, lse, kR, vR = _both_routes(pkg, q, None, None, kc, vc, sl, cos, sin, q_rot, None, qs=qs, causal=causal, n=0.5, what=what)
    assert torch.equal(_bits(kR), _bits(kc)) and torch.equal(_bits(vR), _bits(vc)), "the cache was written without k_new"
    o_ref, l_ref = ks.reference_rows(q_rot, kg, vg, lens, [Sq] * B, 0.5, causal)
    _check(out, o_ref, dtype, f"{what} out")
    _check_lse(lse, l_ref, f"{what} lse")


# ---------------------------------------------------------------- 7. strided operands: one fused buffer, tables sliced from longer ones
def test_strided_operands(pkg, dev):
    _run(pkg, dev, 3, 8, 2, 3, 64, torch.float16, 64, 4, [0, 61, 130], 700, rd=32, fused=True, extra_rows=3, what="fused q/k/v, sliced tables")
    _run(pkg, dev, 2, 8, 2, 40, 64, torch.bfloat16, 64, 3, [5, 100], 710, rd=64, fused=True, interleaved=True, table_dtype=torch.bfloat16,
         prefill=True, what="fused q/k/v, sliced tables, prefill kernels")


# ---------------------------------------------------------------- 8. HIP graph: the positions follow the lengths in device memory
def test_graph_replay_follows_the_lengths(pkg, dev):
    """One captured decode step with append and an in-graph cache_seqlens.add_(1); four replays from length 62 cross position 64"""
    dtype, B, H, Hkv, Sq, D, page, max_pages = torch.bfloat16, 2, 8, 2, 1, 64, 64, 3
    cap = page * max_pages
    start = [62, 126]
    kd = _rand((B, Hkv, cap, D), dtype, dev, 800)
    vd = _rand((B, Hkv, cap, D), dtype, dev, 801, std=1.0)
    pc = _Paged(kd, vd, start, page, max_pages, 802, alloc_all=True)
    cos, sin = _tables(cap, D, dev, torch.float32)
    n = _n_values((H,), dev, 803)
    q, kn, vn = (torch.zeros((B, h, Sq, D), dtype=dtype, device=dev) for h in (H, Hkv, Hkv))
    k_g, v_g, sl_g = pc.k.clone(), pc.v.clone(), pc.lens.clone()
    k_e, v_e, sl_e = pc.k.clone(), pc.v.clone(), pc.lens.clone()

    def step(kc, vc, sl):
        res = pkg.flash_attention_n_kvcache_rope(q, kc, vc, sl, cos, sin, block_table=pc.table, k_new=kn, v_new=vn, softmax_n_param=n,
                                                 return_lse=True)
        sl.add_(1)
        return res

    g, (go, gl) = ks._capture(lambda: step(k_g, v_g, sl_g))   # (a single stream: the captured graph is one chain, no parallel branches)
    with torch.no_grad():   # the warm-up runs appended and advanced: back to the start
        k_g.copy_(pc.k)
        v_g.copy_(pc.v)
        sl_g.copy_(pc.lens)
    seen = []
    for t in range(4):
        with torch.no_grad():
            q.copy_(_rand((B, H, Sq, D), dtype, dev, 810 + 3 * t))
            kn.copy_(_rand((B, Hkv, Sq, D), dtype, dev, 811 + 3 * t))
            vn.copy_(_rand((B, Hkv, Sq, D), dtype, dev, 812 + 3 * t, std=1.0))
        g.replay()
        torch.cuda.synchronize()
        eo, el = step(k_e, v_e, sl_e)
        torch.cuda.synchronize()
        assert sl_g.tolist() == sl_e.tolist() == [s + t + 1 for s in start]
        assert torch.equal(_bits(go), _bits(eo)) and torch.equal(gl.view(torch.int32), el.view(torch.int32)), f"replay {t}: differs from the eager call"
        assert torch.equal(_bits(k_g), _bits(k_e)) and torch.equal(_bits(v_g), _bits(v_e)), f"replay {t}: the pools differ from the eager call's"
        # the row this step appended is the row rotated at position start + t
        k_rot = _rotate(kn, torch.tensor(start)[:, None] + t, cos, sin, False)
        for b in range(B):
            pos = start[b] + t
            pid = int(pc.table[b, pos // page])
            assert torch.equal(_bits(k_g[pid, pos % page]), _bits(k_rot[b, :, 0])), f"replay {t}: cache row {pos} of element {b}"
        assert torch.isfinite(go).all()
        seen.append(go.clone())
    assert all(not torch.equal(seen[t], seen[t + 1]) for t in range(3))
