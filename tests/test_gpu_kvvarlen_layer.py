"""flash_attention_n_kvcache_varlen_window and flash_attention_n_kvcache_varlen_rope on the GPU: a sliding window and rotary position
embedding on token-packed queries - one [T, H, D] buffer, cu_seqlens_q in device memory.

Window. Reference: kv_support.reference_rows (fp32 torch, explicit sink column, the visibility j < len_b and
p_i - W < j <= p_i) per sequence on its own tokens, under the cache tests' gates (REF_ATOL / REL_TRUE on `out`, 1e-4 on `lse`; imported).
Second witness: flash_attention_n_kvcache_window on the same cache with the queries padded and query_seqlens = qlens - the same bits
where both launches have the same split count (the two plan calls say), the gates otherwise. Then the rows below
first_b = 64 * floor(max(0, len_b - qlen_b - W + 1) / 64) become NaN and the table entries of pages wholly below it the poison page
(kv_support._poison), and the call must return the bits it returned before. The three witnesses of tests/kv_witness.py (every
visible key exactly once; one key decides; a realistic dynamic range) run through a runner defined here.

Rope. Bit for bit against the torch-rotated route, as tests/test_gpu_kvrope.py has it for the padded call: flash_attention_n_kvcache_varlen
(or _varlen_window) fed kv_support._rotate'd query / k_new on a clone of the pools - K pool, V pool, out and lse equal as integers -
then the gates against the fp32 reference on the rotated inputs and against the padded flash_attention_n_kvcache_rope(query_seqlens=).

The rows of the token buffers at or beyond cu[B] hold NaN on the way in and are not looked at on the way out."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_witness as kw   # noqa: E402
import kv_args   # noqa: E402
import kv_support as ks   # noqa: E402

pytestmark = pytest.mark.gpu

NAN = ks.NAN
_rand, _Paged, _gather, _check, _check_lse, _poison, _n_values, _cu, _bits = (
    ks._rand, ks._Paged, ks._gather, ks._check, ks._check_lse, ks._poison, ks._n_values, ks._cu, ks._bits)
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
VQ = lambda PB: [1, 0, PB, PB + 1, 2 * PB + 3, 1]   # noqa: E731  a decode token, an empty sequence, a block, a block edge, blocks, a token
VL = lambda page: [300, 5, 0, page + 1, 2 * page, 64]   # noqa: E731


def _pad(t, qlens):
    """[T, heads, D] -> [B, heads, Sq, D], Sq = the longest sequence (at least 1), padding rows zero"""
    Sq = max(max(qlens), 1)
    out = torch.zeros(len(qlens), t.shape[1], Sq, t.shape[2], dtype=t.dtype, device=t.device)
    t0 = 0
    for b, ql in enumerate(qlens):
        out[b, :, :ql] = t[t0:t0 + ql].transpose(0, 1)
        t0 += ql
    return out


def _unpad(o, lse, qlens):
    """[B, H, Sq, D], [B, H, Sq] -> [sum qlens, H, D], [H, sum qlens]"""
    return (torch.cat([o[b, :, :ql].transpose(0, 1) for b, ql in enumerate(qlens)], 0), torch.cat([lse[b, :, :ql] for b, ql in enumerate(qlens)], 1))


def _reference(q, qlens, kg, vg, lens, n, window, causal=True):
    """fp32, per sequence on its own tokens: (o [sum qlens, H, D], lse [H, sum qlens])"""
    qp = _pad(q[:sum(qlens)], qlens)
    return _unpad(*ks.reference_rows(qp, kg, vg, lens, qlens, n, causal if window is None else window), qlens)


def _nsplits(pkg, B, H, Hkv, Sq, D, T, page, max_pages, dtype, W):
    """(the packed window call's split count, the padded window call's) from the two plan calls"""
    shape = dict(B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, page=page, max_pages=max_pages, dtype=1 if dtype == torch.bfloat16 else 0)
    PB = 128 // (H // Hkv)
    operand = pkg._lib.KvWindow(window=min(W, 2 ** 31 - 1), reserved=0)
    packed = pkg._lib.kvvarlen_window_plan(kv_args._args_varlen(pkg, T=T, **shape), operand)
    assert [k[0].split("<")[0] for k in packed[:2]] == ["fasn_kvvarlen_schedule_kernel", "fasn_kvvarlen_fwd_window_kernel"]
    padded = pkg._lib.kvprefill_window_plan(kv_args._args_prefill(pkg, **shape), operand)
    return packed[1][1] // (kv_args.items_max(B, Sq, T, PB) * Hkv), padded[0][1] // (B * Hkv * -(-Sq // PB))


def _run_window(pkg, dev, H, Hkv, D, dtype, page, qlens, lens, n, W, seed=1, max_pages=None, tail=7, what=""):
    """no append: `lens` are the keys in the cache. The call, its two witnesses, then the same call over the poisoned cache. Returns
    (out, lse, poisoned rows, the packed call's split count)"""
    B, used = len(qlens), sum(qlens)
    max_pages = max_pages or max(1, max((ln + page - 1) // page for ln in lens)) + 1
    T, Sq = used + tail, max(max(qlens), 1)
    q = _rand((T, H, D), dtype, dev, seed)
    q[used:] = NAN
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, seed + 1)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, seed + 2, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, seed)
    cu = _cu(qlens, dev)
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)

    def call():
        return pkg.flash_attention_n_kvcache_varlen_window(q, pc.k, pc.v, pc.lens, cu, Sq, W, block_table=pc.table, softmax_n_param=n, return_lse=True)

    out, lse = call()
    assert out.shape == q.shape and lse.shape == (H, T)
    o_ref, l_ref = _reference(q, qlens, kg, vg, lens, n, W)
    _check(out[:used], o_ref, dtype, f"{what} out")
    _check_lse(lse[:, :used], l_ref, f"{what} lse")
    # the padded call: the same kernel text on the same row blocks and tiles
    wo, wl = pkg.flash_attention_n_kvcache_window(_pad(q[:used], qlens), pc.k, pc.v, pc.lens, W, block_table=pc.table,
                                                  query_seqlens=torch.tensor(qlens, dtype=torch.int32, device=dev), softmax_n_param=n, return_lse=True)
    wo, wl = _unpad(wo, wl, qlens)
    ns_packed, ns_padded = _nsplits(pkg, B, H, Hkv, Sq, D, T, page, max_pages, dtype, W)
    if ns_packed == ns_padded:
        assert torch.equal(out[:used], wo) and torch.equal(lse[:, :used], wl), f"{what}: not the bits of the padded call ({ns_packed} splits both)"
    else:
        _check(out[:used], wo, dtype, f"{what} out vs the padded call")
        _check_lse(lse[:, :used], wl, f"{what} lse vs the padded call")
    # freed pages: NaN below first_b, the poison page behind every table entry wholly below it
    rows = _poison(pc.k, pc.v, pc.table, page, pc.poison, lens, qlens, W)
    o2, l2 = call()
    assert torch.isfinite(o2[:used]).all() and not torch.isnan(l2[:, :used]).any(), f"{what}: the poison below the window reached the result"
    assert torch.equal(out[:used], o2[:used]) and torch.equal(lse[:, :used], l2[:, :used]), f"{what}: the rows below the window changed the result"
    return out, lse, rows, ns_packed


# ---------------------------------------------------------------- 1. window parity, freed pages
@pytest.mark.parametrize("W", [5, 64, 200])
@pytest.mark.parametrize("page", [64, 256])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", [(8, 1), (16, 16), (12, 4)])
def test_window_parity(pkg, dev, heads, D, dtype, page, W):
    H, Hkv = heads
    PB = 128 // (H // Hkv)   # 16 / 128 / 42
    _o, _l, rows, _ns = _run_window(pkg, dev, H, Hkv, D, DTYPES[dtype], page, VQ(PB), VL(page), 1.0, W, seed=100 + D + page + H + W,
                                    what=f"H={H}/{Hkv} D={D} {dtype} page={page} W={W}")
    assert rows > 0, "no row was poisoned"


@pytest.mark.parametrize("D", [32, 256])
def test_window_parity_other_head_dims(pkg, dev, D):
    _o, _l, rows, _ns = _run_window(pkg, dev, 8, 1, D, torch.bfloat16, 64, VQ(16), VL(64), _n_values((8,), dev, 150), 64, seed=150 + D, what=f"D={D} W=64")
    assert rows > 0


def test_a_window_at_or_beyond_the_capacity_is_no_window(pkg, dev):
    H, Hkv, D, page, dtype = 12, 4, 64, 64, torch.bfloat16
    qlens, lens = VQ(42), VL(page)
    max_pages = max((ln + page - 1) // page for ln in lens) + 1
    for W in (page * max_pages, 1 << 40):
        out, lse, rows, _ns = _run_window(pkg, dev, H, Hkv, D, dtype, page, qlens, lens, 0.5, W, seed=170, max_pages=max_pages, what=f"W={W}")
        assert rows == 0
        used, T = sum(qlens), sum(qlens) + 7
        q = _rand((T, H, D), dtype, dev, 170)    # (the operands of _run_window, rebuilt)
        q[used:] = NAN
        kd = _rand((len(qlens), Hkv, page * max_pages, D), dtype, dev, 171)
        vd = _rand((len(qlens), Hkv, page * max_pages, D), dtype, dev, 172, std=1.0)
        pc = _Paged(kd, vd, lens, page, max_pages, 170)
        o0, l0 = pkg.flash_attention_n_kvcache_varlen(q, pc.k, pc.v, pc.lens, _cu(qlens, dev), max(qlens), block_table=pc.table, softmax_n_param=0.5,
                                                      return_lse=True)
        assert torch.equal(out[:used], o0[:used]) and torch.equal(lse[:, :used], l0[:, :used]), f"W={W}: not what the call without a window gives"


# ---------------------------------------------------------------- 2. several splits
SPLIT = dict(H=8, Hkv=1, D=64, page=256, max_pages=16, qlens=[1, 40, 3], lens=[4000, 2100, 20], W=3000)


def _run_split(pkg, dev, dtype, n, seed):
    c = SPLIT
    out, lse, rows, ns = _run_window(pkg, dev, c["H"], c["Hkv"], c["D"], dtype, c["page"], c["qlens"], c["lens"], n, c["W"], seed=seed,
                                     max_pages=c["max_pages"], what=f"several splits {dtype} n={n if not isinstance(n, torch.Tensor) else 'tensor'}")
    # items_max = min(3 * 3, 51 // 16 + 3) = 6; the window spans min(64, ceil((3000 + 15) / 64) + 1) = 49 tiles, 16 per split: 3 splits.
    # Sequence 0 has 960 rows below its window; sequence 2 (20 keys, one tile) leaves two of the three splits empty
    assert ns >= 2, f"the plan has {ns} split(s): the shape was chosen to have several"
    assert rows == 960
    return out, lse


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_several_splits(pkg, dev, dtype):
    _run_split(pkg, dev, DTYPES[dtype], _n_values((SPLIT["H"],), dev, 300), 301)


@pytest.mark.parametrize("n", [1.0, 0.0, 0.5])
def test_several_splits_scalar_n(pkg, dev, n):
    _run_split(pkg, dev, torch.bfloat16, n, 310)


# ---------------------------------------------------------------- 3. the witnesses of kv_witness.py
Case = kw.Case
SHAPES = {
    "H8/1 W5": Case("varlen_window", 8, 1, 64, 35, VL(64), qlens=VQ(16), window=5),
    "H12/4 W64 append": Case("varlen_window", 12, 4, 64, 87, VL(64), qlens=VQ(42), window=64, append=True),
    "H12/4 D128 W200": Case("varlen_window", 12, 4, 128, 87, VL(64), qlens=VQ(42), window=200),
    "split W3000": Case("varlen_window", SPLIT["H"], SPLIT["Hkv"], SPLIT["D"], 40, SPLIT["lens"], page=SPLIT["page"], max_pages=SPLIT["max_pages"],
                        qlens=SPLIT["qlens"], window=SPLIT["W"], long=True),
}


def _run_witness(pkg, case, inp, seed):
    """kv_witness.run_varlen for the window call: the queries (and k_new / v_new) token-packed, `tail` NaN rows behind cu[B]; the cache of
    kw._cache is poisoned below every sequence's window. Per sequence (out [H, qlen_b, D], lse [H, qlen_b])"""
    pc = kw._cache(case, inp, seed)
    dev = pc.k.device
    kn, vn = kw._new_rows(case, inp)
    used = sum(case.qlens)

    def pack(t):   # [B, heads, Sq, D] -> [T, heads, D]
        rows = [t[b, :, :ql].transpose(0, 1) for b, ql in enumerate(case.qlens)]
        return torch.cat(rows + [torch.full((case.tail, t.shape[1], t.shape[3]), NAN, dtype=t.dtype, device=dev)], 0).contiguous()

    out, lse = pkg.flash_attention_n_kvcache_varlen_window(pack(inp["q"]), pc.k, pc.v, pc.lens, _cu(case.qlens, dev), max(max(case.qlens), 1),
                                                           case.window, block_table=pc.table, k_new=None if kn is None else pack(kn),
                                                           v_new=None if vn is None else pack(vn), softmax_n_param=inp["n"], scale=inp["scale"],
                                                           return_lse=True)
    assert out.shape == (used + case.tail, case.H, case.D) and lse.shape == (case.H, used + case.tail)
    res, t0 = [], 0
    for ql in case.qlens:
        res.append((out[t0:t0 + ql].transpose(0, 1), lse[:, t0:t0 + ql]))
        t0 += ql
    return res


def _seed(name):
    return 2000 + sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 9000


def _dtypes(case):
    return ["fp16"] if case.long else ["fp16", "bf16"]


@pytest.mark.parametrize("name,dtype", [(s, d) for s in SHAPES for d in _dtypes(SHAPES[s])])
def test_witness_a_every_visible_key_exactly_once(pkg, dev, name, dtype):
    case, dt = SHAPES[name], DTYPES[dtype]
    inp = kw.inputs_a(case, dt, dev, _seed(name))
    refs = kw.reference(case, inp)
    cmax = kw.condition_a(refs, dt)
    got = _run_witness(pkg, case, inp, _seed(name))
    ratios = [kw.gate_a(o, lse, r) for (o, lse), r in zip(got, refs)]
    rz, ro = max(r[0] for r in ratios), max(r[1] for r in ratios)
    print(f"A {name} {dtype}: largest class count {cmax:g}; exp(lse) at {rz:.3g} of 1e-5 Z, out Z at {ro:.3g} of 0.25")
    assert rz <= 1, f"exp(lse) is {rz:.3g}x (1e-5 Z_ref) from n + the number of visible keys, per sequence {[r[0] for r in ratios]}"
    assert ro <= 1, f"out Z_ref is {ro:.3g}x 0.25 from the class counts, per sequence {[r[1] for r in ratios]}"


B_CASES = [(s, form, d) for s in SHAPES for form, ds in (("ascending", ("fp16", "bf16")), ("descending", ("bf16",)), ("sink", ("bf16",)))
           for d in (("fp16",) if SHAPES[s].long else ds)]


@pytest.mark.parametrize("name,form,dtype", B_CASES)
def test_witness_b_one_key_decides(pkg, dev, name, form, dtype):
    case, dt = SHAPES[name], DTYPES[dtype]
    inp = kw.inputs_b(case, form, dt, dev, _seed(name))
    refs = kw.reference(case, inp)
    got = _run_witness(pkg, case, inp, _seed(name))
    ratios, kinds, lses = [], set(), []
    for b, ((o, lse), r) in enumerate(zip(got, refs)):
        kind, want = kw.expect_b(r, kw.sequence(case, inp, b)[2][:, :case.total[b]], case.H // case.Hkv)
        kinds |= set(kind.unique().tolist())
        ratios.append(kw.gate_b(o, kind, want, dt))
        lses.append((lse.detach().cpu(), r["lse"], kind))
    print(f"B {name} {form} {dtype}: out at {max(ratios):.3g} of its gate; row kinds {sorted(kinds)}")
    assert max(ratios) <= 1, f"out is {max(ratios):.3g}x the gate from the deciding key's V row, per sequence {ratios}"
    for b, (lse, want, kind) in enumerate(lses):
        for k in (0, 1, 2):   # rows of one kind together: log n is not measured against a key's thousands of nats
            if (kind == k).any():
                _check_lse(lse[kind == k], want[kind == k], f"B {name} {form} {dtype} sequence {b} lse (rows of kind {k})")
    assert 1 in kinds and (form != "sink" or 2 in kinds)


@pytest.mark.parametrize("std", [4, 8])
@pytest.mark.parametrize("name,dtype", [(s, d) for s in SHAPES for d in _dtypes(SHAPES[s])])
def test_witness_c_realistic_dynamic_range(pkg, dev, name, dtype, std):
    case, dt = SHAPES[name], DTYPES[dtype]
    inp = kw.inputs_c(case, std, dt, dev, _seed(name) + std)
    refs = kw.reference(case, inp)
    got = _run_witness(pkg, case, inp, _seed(name))
    ratios = [kw.gate_c(o, r, dt) for (o, _), r in zip(got, refs)]
    print(f"C {name} std {std} {dtype}: out at {max(ratios):.3g} of 3 u A + 1e-6")
    assert max(ratios) <= 1, f"out is {max(ratios):.3g}x (3 u A + 1e-6) from the fp64 reference, per sequence {ratios}"
    for b, ((_, lse), r) in enumerate(zip(got, refs)):
        _check_lse(lse, r["lse"], f"C {name} std {std} {dtype} sequence {b} lse")


# ---------------------------------------------------------------- 4. rope: bit for bit against the torch-rotated route
def _rotate_packed(x, pos, cos, sin, interleaved):
    """kv_support._rotate on [n, heads, D] rows at positions pos [n]"""
    return ks._rotate(x.transpose(0, 1).unsqueeze(0), pos[None], cos, sin, interleaved)[0].transpose(0, 1).contiguous()


def _run_rope(pkg, dev, H, Hkv, D, dtype, page, max_pages, qlens, lens, seed, rd=None, table_dtype=torch.float32, interleaved=False, window=None,
              append=True, causal=True, n=1.0, tail=7, check_ref=True, what=""):
    """One paged case: the new call (R) and the existing packed call fed torch-rotated rows (T) on clones of one pool; R against the fp32
    reference on the rotated inputs and against the padded rope call. Returns (out, lse, R's pools, the pools before)."""
    B, used, cap, rd = len(qlens), sum(qlens), page * max_pages, rd or D
    T, Sq = used + tail, max(max(qlens), 1)
    q = _rand((T, H, D), dtype, dev, seed)
    kn = _rand((T, Hkv, D), dtype, dev, seed + 1)
    vn = _rand((T, Hkv, D), dtype, dev, seed + 2, std=1.0)
    for t in (q, kn, vn):
        t[used:] = NAN
    cos, sin = ks._tables(cap, rd, dev, table_dtype)
    kd = _rand((B, Hkv, cap, D), dtype, dev, seed + 3)
    vd = _rand((B, Hkv, cap, D), dtype, dev, seed + 4, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, seed, alloc_all=True, guard=7.0)   # rows at or beyond the length: NaN until the append writes them
    total = [min(cap, ln + ql) if append else ln for ln, ql in zip(lens, qlens)]
    kpos = torch.cat([lens[b] + torch.arange(ql) for b, ql in enumerate(qlens)])
    qpos = torch.cat([torch.arange(ql) + total[b] - ql for b, ql in enumerate(qlens)])
    q_rot, k_rot = q.clone(), kn.clone()
    q_rot[:used], k_rot[:used] = _rotate_packed(q[:used], qpos, cos, sin, interleaved), _rotate_packed(kn[:used], kpos, cos, sin, interleaved)
    if append:   # the dense picture of the cache after the append
        t0 = 0
        for b, ql in enumerate(qlens):
            m = max(0, min(ql, cap - lens[b]))
            kd[b, :, lens[b]:lens[b] + m] = k_rot[t0:t0 + m].transpose(0, 1)
            vd[b, :, lens[b]:lens[b] + m] = vn[t0:t0 + m].transpose(0, 1)
            t0 += ql
    if window is not None:
        assert _poison(pc.k, pc.v, pc.table, page, pc.poison, total, qlens, window) > 0
    cu, sl = _cu(qlens, dev), pc.lens
    cu0, sl0, q0, kn0 = cu.clone(), sl.clone(), q.clone(), kn.clone()
    new = dict(k_new=kn, v_new=vn) if append else {}
    kR, vR = pc.k.clone(), pc.v.clone()
    out, lse = pkg.flash_attention_n_kvcache_varlen_rope(q, kR, vR, sl, cu, Sq, cos, sin, block_table=pc.table, softmax_n_param=n, is_causal=causal,
                                                         return_lse=True, window=window, rotary_interleaved=interleaved, **new)
    assert out.shape == q.shape and lse.shape == (H, T)
    assert torch.equal(sl, sl0) and torch.equal(cu, cu0), f"{what}: cache_seqlens / cu_seqlens_q was modified"
    assert torch.equal(_bits(q), _bits(q0)) and torch.equal(_bits(kn), _bits(kn0)), f"{what}: query / k_new was modified"
    kT, vT = pc.k.clone(), pc.v.clone()
    new_t = dict(k_new=k_rot, v_new=vn) if append else {}
    if window is None:
        o_t, l_t = pkg.flash_attention_n_kvcache_varlen(q_rot, kT, vT, sl, cu, Sq, block_table=pc.table, softmax_n_param=n, is_causal=causal,
                                                        return_lse=True, **new_t)
    else:
        o_t, l_t = pkg.flash_attention_n_kvcache_varlen_window(q_rot, kT, vT, sl, cu, Sq, window, block_table=pc.table, softmax_n_param=n,
                                                               return_lse=True, **new_t)
    torch.cuda.synchronize()
    dk, dv = (_bits(kR) != _bits(kT)).sum().item(), (_bits(vR) != _bits(vT)).sum().item()
    do = (_bits(out[:used]) != _bits(o_t[:used])).sum().item()
    dl = (lse[:, :used].view(torch.int32) != l_t[:, :used].view(torch.int32)).sum().item()
    print(f"{what}: elements that differ between the routes: k pool {dk}, v pool {dv}, out {do}, lse {dl}")
    assert dk == 0, f"{what}: k pools differ in {dk} elements"
    assert dv == 0, f"{what}: v pools differ in {dv} elements"
    assert do == 0, f"{what}: out differs from the torch-rotated route in {do} elements"
    assert dl == 0, f"{what}: lse differs from the torch-rotated route in {dl} elements"
    assert (kR[-1] == 7.0).all() and (vR[-1] == 7.0).all(), f"{what}: guard page behind the pool was written"
    assert torch.isfinite(out[:used]).all() and not torch.isnan(lse[:, :used]).any(), f"{what}: the NaN rows behind cu[B] reached the used rows"
    if not append:
        assert torch.equal(_bits(kR), _bits(pc.k)) and torch.equal(_bits(vR), _bits(pc.v)), f"{what}: the cache was written without k_new"
    if check_ref:   # (a sequence that lost rows at the capacity is aligned by its clamped length: the dense picture above does not hold it)
        kg, vg = ks._visible_dense(kd, total), ks._visible_dense(vd, total)
        o_ref, l_ref = _reference(q_rot, qlens, kg, vg, total, n, window, causal)
        _check(out[:used], o_ref, dtype, f"{what} out")
        _check_lse(lse[:, :used], l_ref, f"{what} lse")
    # the padded call on its own clone of the pools
    kP, vP = pc.k.clone(), pc.v.clone()
    new_p = dict(k_new=_pad(kn[:used], qlens), v_new=_pad(vn[:used], qlens)) if append else {}
    po, pl = pkg.flash_attention_n_kvcache_rope(_pad(q[:used], qlens), kP, vP, sl, cos, sin, block_table=pc.table,
                                                query_seqlens=torch.tensor(qlens, dtype=torch.int32, device=dev), softmax_n_param=n, is_causal=causal,
                                                return_lse=True, window=window, rotary_interleaved=interleaved, **new_p)
    po, pl = _unpad(po, pl, qlens)
    _check(out[:used], po, dtype, f"{what} out vs the padded rope call")
    _check_lse(lse[:, :used], pl, f"{what} lse vs the padded rope call")
    assert torch.equal(_bits(kR), _bits(kP)) and torch.equal(_bits(vR), _bits(vP)), f"{what}: the pools differ from the padded rope call's"
    return out, lse, kR, vR, pc


@pytest.mark.parametrize("rd", [64, 32])
@pytest.mark.parametrize("layout", ["half", "interleaved"])
@pytest.mark.parametrize("tables", ["fp32", "16bit"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_rope(pkg, dev, dtype, tables, layout, rd):
    """heads (8, 2): PB = 32; a decode token, an empty sequence, a block, a block edge, blocks; appends across a tile and a page edge"""
    dt = DTYPES[dtype]
    _run_rope(pkg, dev, 8, 2, 64, dt, 64, 4, VQ(32), [130, 5, 0, 61, 100, 64], 400, rd=rd, table_dtype=torch.float32 if tables == "fp32" else dt,
              interleaved=layout == "interleaved", n=_n_values((8,), dev, 401), what=f"rope {dtype} tables={tables} {layout} rd={rd}")


@pytest.mark.parametrize("D", [32, 128, 256])
def test_rope_head_dims(pkg, dev, D):
    dt = {32: torch.float16, 128: torch.bfloat16, 256: torch.float16}[D]
    _run_rope(pkg, dev, 8, 2, D, dt, 64, 4, VQ(32), [130, 5, 0, 61, 100, 64], 420 + D, rd=D if D != 128 else 16,
              table_dtype=torch.float32 if D != 128 else dt, interleaved=D == 256, what=f"rope D={D}")


@pytest.mark.parametrize("causal", [True, False])
def test_rope_queries_only(pkg, dev, causal):
    """no k_new: the cache is not written, p_i = i + len_b - qlen_b over the cache as it is - negative where a sequence has more positions
    than keys (the table row is clamped to 0)"""
    _run_rope(pkg, dev, 12, 4, 64, torch.bfloat16, 64, 4, [1, 0, 42, 43, 5], [130, 5, 7, 100, 1], 440, append=False, causal=causal, n=0.5,
              what=f"rope queries only causal={causal}")


def test_rope_window(pkg, dev):
    _run_rope(pkg, dev, 8, 1, 64, torch.bfloat16, 64, 8, VQ(16), [300, 5, 0, 65, 128, 64], 460, window=128, n=_n_values((8,), dev, 461),
              what="rope window=128")


def test_rope_append_crosses_the_capacity(pkg, dev):
    """sequence 0 has 48 rows left for 50 tokens: two rows are dropped, by the new launch exactly as by fasn_kvvarlen_append"""
    page, max_pages = 64, 3
    cap = page * max_pages
    _o, _l, kR, _vR, pc = _run_rope(pkg, dev, 16, 4, 64, torch.float16, page, max_pages, [50, 1, 0, 20, 1], [cap - 48, page - 1, 7, page - 2, 0], 480,
                                    check_ref=False, what="rope capacity")
    changed = (_bits(kR) != _bits(pc.k)).flatten(2).any(-1).sum().item()   # rows of the pool that were NaN and hold a key now
    assert changed == 48 + 1 + 20 + 1, changed


# ---------------------------------------------------------------- 5. HIP graph
def test_graph_replay_follows_offsets_lengths_table_and_query(pkg, dev):
    """One captured step of flash_attention_n_kvcache_varlen_rope(window=64) with an append at T = 64, B = 4, max_seqlen_q = 48; replays
    after cu_seqlens_q, cache_seqlens, query, k_new / v_new and one block-table row changed in place: the bits of an eager call."""
    dtype, H, Hkv, D, page, max_pages, T, B, Sq, W = torch.bfloat16, 16, 4, 64, 64, 8, 64, 4, 48, 64
    cap = page * max_pages
    q, kn, vn = _rand((T, H, D), dtype, dev, 600), _rand((T, Hkv, D), dtype, dev, 601), _rand((T, Hkv, D), dtype, dev, 602, std=1.0)
    kd = _rand((B, Hkv, cap, D), dtype, dev, 603)
    vd = _rand((B, Hkv, cap, D), dtype, dev, 604, std=1.0)
    pc = _Paged(kd, vd, [cap] * B, page, max_pages, 605, alloc_all=True)   # every row finite: the lengths move
    cos, sin = ks._tables(cap, D, dev, torch.float32)
    n = _n_values((H,), dev, 606)
    cu = _cu([1, 1, 1, 1], dev)
    sl = torch.tensor([62, 100, 5, 300], dtype=torch.int32, device=dev)
    table = pc.table
    k_e, v_e = pc.k.clone(), pc.v.clone()   # the eager route's pools: they see the same appends

    def call(q_, kn_, vn_, kc, vc, sl_, cu_, tab):
        return pkg.flash_attention_n_kvcache_varlen_rope(q_, kc, vc, sl_, cu_, Sq, cos, sin, block_table=tab, k_new=kn_, v_new=vn_, softmax_n_param=n,
                                                         return_lse=True, window=W)

    g, (go, glse) = ks._capture(lambda: call(q, kn, vn, pc.k, pc.v, sl, cu, table))
    with torch.no_grad():   # the warm-up runs appended: the eager pools follow
        k_e.copy_(pc.k)
        v_e.copy_(pc.v)
    seen = []
    for step, qlens in enumerate(([1, 1, 1, 1], [48, 1, 10, 5], [0, 16, 30, 18])):
        lens = [62 + 37 * step, 100 + step, 5, 300 - 64 * step]
        used = sum(qlens)
        with torch.no_grad():
            for t, s in ((q, 610), (kn, 620), (vn, 630)):
                t.copy_(_rand(tuple(t.shape), dtype, dev, s + step, std=1.0 if t is vn else 0.5))
                t[used:] = NAN
            cu.copy_(_cu(qlens, dev))
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
            table[step] = table[step].flip(0)
        g.replay()
        torch.cuda.synchronize()
        eo, el = call(q.clone(), kn.clone(), vn.clone(), k_e, v_e, sl.clone(), cu.clone(), table.clone())
        assert torch.equal(_bits(go[:used]), _bits(eo[:used])) and torch.equal(glse[:, :used], el[:, :used]), f"replay {step}: differs from the eager call"
        assert torch.equal(_bits(pc.k), _bits(k_e)) and torch.equal(_bits(pc.v), _bits(v_e)), f"replay {step}: the pools differ from the eager call's"
        assert torch.isfinite(go[:used]).all()
        seen.append(go[:1].clone())
    assert not torch.equal(seen[0], seen[1]), "the replays returned one result: the graph does not follow the device memory"


# ---------------------------------------------------------------- 6. refusals on the device
def test_refusals_on_the_device(pkg, dev):
    dtype = torch.bfloat16
    q = torch.zeros(10, 8, 64, dtype=dtype, device=dev)
    kc = torch.zeros(4, 64, 2, 64, dtype=dtype, device=dev)
    sl = torch.zeros(2, dtype=torch.int32, device=dev)
    cu = torch.tensor([0, 4, 9], dtype=torch.int32, device=dev)
    bt = torch.zeros(2, 2, dtype=torch.int32, device=dev)
    cos, sin = ks._tables(128, 32, dev, torch.float32)
    fw, fr = pkg.flash_attention_n_kvcache_varlen_window, pkg.flash_attention_n_kvcache_varlen_rope
    assert fw(q, kc, kc, sl, cu, 8, 5, block_table=bt).shape == (10, 8, 64)
    assert fr(q, kc, kc, sl, cu, 8, cos, sin, block_table=bt, window=5).shape == (10, 8, 64)
    with pytest.raises(TypeError, match="flash_attention_n_kvcache_varlen_window: window must be a Python int"):
        fw(q, kc, kc, sl, cu, 8, torch.tensor(5, device=dev), block_table=bt)
    with pytest.raises(ValueError, match="flash_attention_n_kvcache_varlen_window: window must be >= 1"):
        fw(q, kc, kc, sl, cu, 8, 0, block_table=bt)
    with pytest.raises(ValueError, match=r"k_new must be \[T, Hkv, D\] = \[10, 2, 64\]"):
        kn = torch.zeros(2, 2, 5, 64, dtype=dtype, device=dev)
        fw(q, kc, kc, sl, cu, 8, 5, block_table=bt, k_new=kn, v_new=kn)
    with pytest.raises(RuntimeError, match="cu_seqlens_q is on cpu"):
        fw(q, kc, kc, sl, cu.cpu(), 8, 5, block_table=bt)
    with pytest.raises(ValueError, match="flash_attention_n_kvcache_varlen_rope: a sliding window is always causal"):
        fr(q, kc, kc, sl, cu, 8, cos, sin, block_table=bt, window=5, is_causal=False)
    with pytest.raises(RuntimeError, match="rotary_cos is on cpu"):
        fr(q, kc, kc, sl, cu, 8, cos.cpu(), sin.cpu(), block_table=bt)
    with pytest.raises(ValueError, match="flash_attention_n_kvcache_varlen_rope: the rotary tables cover 127 positions but the cache holds up to 128"):
        fr(q, kc, kc, sl, cu, 8, cos[:127], sin[:127], block_table=bt)
    with pytest.raises(ValueError, match=r"flash_attention_n_kvcache_varlen_rope: rotary_cos / rotary_sin must be float32 or the dtype of query"):
        fr(q, kc, kc, sl, cu, 8, cos.half(), sin.half(), block_table=bt)
    with pytest.raises(RuntimeError, match="cu_seqlens_q is on cpu"):
        fr(q, kc, kc, sl, cu.cpu(), 8, cos, sin, block_table=bt)
