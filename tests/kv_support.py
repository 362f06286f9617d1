"""What the K/V-cache GPU suites share: data (_rand, _n_values, _Paged and what reads and pokes it), the visibility masks and the ALiBi
bias, the fp32 reference and its per-batch-element wrapper, the gates, _check_all with its flash_attention_n witness, the runners of the
plain and the ALiBi calls, graph capture, the rotary tables and rotation, and the plan checks of the split shapes. A plain module: no
tests, importable without a GPU (tests/test_kvwitness_cpu.py runs the reference and the gates on the CPU).

Reference of every case: the visible rows gathered through the table into dense [B, Hkv, S, D] tensors, the visibility as a boolean
mask, fp32 torch with the explicit sink column, one n per (batch, head), an optional fp32 bias added to the scaled scores before the
masking. Gates: the project's own (REF_ATOL and REL_TRUE as tests/test_gpu_parity.py::_check applies them) on `out`, atol 1e-4 scaled
the same way on `lse`. Second, independent witness: flash_attention_n on the gathered dense K/V with the same mask, bias and n.

A visibility `rule` is False (every position sees the len_b keys), True (causal, bottom-right aligned per batch element) or an int W
(a sliding window of W keys, always causal): position i < qlen_b sees key j iff j < len_b and, with p_i = i + len_b - qlen_b,
(True) j <= p_i, (W) p_i - W < j <= p_i."""
import itertools

import torch

import kv_args
from flash_attention_softmax_n_amd import synth

REF_ATOL = {torch.float16: 1e-2, torch.bfloat16: 5e-2}
REL_TRUE = {torch.float16: 2.0 ** -9, torch.bfloat16: 2.0 ** -6}
NAN = float("nan")


def _rand(shape, dtype, dev, seed, std=0.5):
    return synth.counter_normal(shape, seed, std=std, dtype=dtype, device=dev)


def _check(got, want, dtype, what):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - want).abs().max().item() if got.numel() else 0.0
    scale = want.abs().max().item() if want.numel() else 0.0
    atol = REF_ATOL[dtype] * max(1.0, scale)
    print(f"{what}: max-abs {err:.3e} (atol {atol:.3e}, relative gate {REL_TRUE[dtype] * max(scale, 1e-2):.3e})")
    assert err <= atol, f"{what}: max-abs {err:.3e} > reference atol {atol:.3e}"
    lim = REL_TRUE[dtype] * max(scale, 1e-2)
    assert err <= lim, f"{what}: max-abs {err:.3e} > {lim:.3e} (relative gate)"


def _check_lse(got, want, what):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert not torch.isnan(got).any(), f"{what}: NaN"
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], want[inf]), f"{what}: -inf rows differ"
    if (~inf).any():
        err = (got[~inf] - want[~inf]).abs().max().item()
        atol = 1e-4 * max(1.0, want[~inf].abs().max().item())
        print(f"{what}: max-abs {err:.3e} (atol {atol:.3e})")
        assert err <= atol, f"{what}: max-abs {err:.3e} > {atol:.3e}"


def _visibility(lens, Sq, S, causal, dev):
    """[B, 1, Sq, S] bool: key j of batch element b is visible to position i"""
    ln = torch.as_tensor(lens, device=dev).view(-1, 1, 1, 1)
    i = torch.arange(Sq, device=dev).view(1, 1, Sq, 1)
    j = torch.arange(S, device=dev).view(1, 1, 1, S)
    vis = j < ln
    if causal:
        vis = vis & (j <= i + ln - Sq)
    return vis.expand(len(lens), 1, Sq, S)


def _mask(lens, qlens, Sq, S, causal, dev):
    """[B, 1, Sq, S] bool: position i < qlen_b sees key j iff j < len_b and (causal) j <= i + len_b - qlen_b; padding positions see nothing"""
    ln = torch.as_tensor(lens, device=dev).view(-1, 1, 1, 1)
    ql = torch.as_tensor(qlens, device=dev).view(-1, 1, 1, 1)
    i = torch.arange(Sq, device=dev).view(1, 1, Sq, 1)
    j = torch.arange(S, device=dev).view(1, 1, 1, S)
    vis = (j < ln) & (i < ql)
    if causal:
        vis = vis & (j <= i + ln - ql)
    return vis


def _win_mask(lens, qlens, Sq, S, W, dev):
    """[B, 1, Sq, S] bool: position i < qlen_b sees key j iff j < len_b and p_i - W < j <= p_i; padding positions see nothing"""
    ln = torch.as_tensor(lens, device=dev).view(-1, 1, 1, 1)
    ql = torch.as_tensor(qlens, device=dev).view(-1, 1, 1, 1)
    i = torch.arange(Sq, device=dev).view(1, 1, Sq, 1)
    j = torch.arange(S, device=dev).view(1, 1, 1, S)
    p = i + ln - ql
    return (j < ln) & (i < ql) & (j <= p) & (j > p - W)


def _rule_mask(lens, qlens, Sq, S, rule, dev):
    """the [B, 1, Sq, S] bool mask of a visibility rule (the module docstring); padding positions see nothing"""
    return _mask(lens, qlens, Sq, S, rule, dev) if isinstance(rule, bool) else _win_mask(lens, qlens, Sq, S, rule, dev)


def _slopes(H, dev):
    """synth.alibi_slopes (a power of two of heads; otherwise the first H of the next power of two), fp32 [H]"""
    P = 1 << (H - 1).bit_length()
    return synth.alibi_slopes(P)[:H].float().to(dev)


def _bh(t, B, H):
    """a tensor that broadcasts to [B, H] ([H], [1, H], [B, 1], [B, H] or 0-d) as fp32 [B, H]"""
    t = t.float()
    return t.reshape((1,) * (2 - t.dim()) + tuple(t.shape)).expand(B, H)


def _bias(slopes, lens, qlens, H, Sq, S, dev):
    """fp32 [B, H, Sq, S]: -slope[b, h] * |i + len_b - qlen_b - j| (synth.alibi_bias's convention with S = len_b, L = qlen_b)"""
    B = len(lens)
    off = (torch.as_tensor(lens, device=dev) - torch.as_tensor(qlens, device=dev)).view(B, 1, 1, 1)
    i = torch.arange(Sq, device=dev).view(1, 1, Sq, 1)
    j = torch.arange(S, device=dev).view(1, 1, 1, S)
    dist = (i + off - j).abs().float()
    return -(_bh(slopes.to(dev), B, H)[:, :, None, None] * dist)


def reference(q, kd, vd, vis, n, bias=None, scale=None):
    """fp32 torch on the device: Z_i = n + sum_j exp(x_ij) (the sink column: logit 0, weight n, value 0). kd / vd: [B, Hkv, S, D] with
    finite values everywhere; n: float or tensor broadcasting to [B, H]; `bias` (fp32, broadcasts to [B, H, Sq, S]) is added to the
    scaled scores before the masking. Returns (o [B,H,Sq,D], lse [B,H,Sq])."""
    B, H, Sq, D = q.shape
    Hkv, S = kd.shape[1], kd.shape[2]
    G = H // Hkv
    qf = q.float().view(B, Hkv, G, Sq, D)
    s = torch.einsum("bkgqd,bksd->bkgqs", qf, kd.float()).view(B, H, Sq, S) * (D ** -0.5 if scale is None else scale)
    if bias is not None:
        s = s + bias
    s = s.masked_fill(~vis, float("-inf"))
    nt = torch.as_tensor(n, dtype=torch.float32, device=q.device)
    nb = nt.reshape((1,) * (2 - nt.dim()) + tuple(nt.shape)).expand(B, H)[..., None, None]
    m = s.amax(-1, keepdim=True)
    m = torch.where(nb > 0, m.clamp_min(0.0), m)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    # (n = 0 rows carry no sink term: written as a select, because with a bias the maximum of such a row can lie below -88, where
    # exp(-m) overflows in fp32 and 0 * inf would be NaN; rows with n > 0 have m >= 0)
    z = torch.where(nb > 0, nb * torch.exp(-m), torch.zeros_like(m)) + e.sum(-1, keepdim=True)
    p = e / torch.where(z > 0, z, torch.ones_like(z))
    o = torch.einsum("bkgqs,bksd->bkgqd", p.view(B, Hkv, G, Sq, S), vd.float()).reshape(B, H, Sq, D)
    lse = (m + torch.log(z)).squeeze(-1)
    return o, lse


def reference_rows(q, kg, vg, lens, qlens, n, rule, scale=None, slopes=None):
    """`reference` per batch element on q[b, :, :qlen_b] under a visibility rule, with the ALiBi bias of `slopes`; padding positions: 0 / -inf"""
    B, H, Sq, D = q.shape
    dev = q.device
    S = kg.shape[2]
    o = torch.zeros(B, H, Sq, D, dtype=torch.float32, device=dev)
    lse = torch.full((B, H, Sq), float("-inf"), dtype=torch.float32, device=dev)
    nb = _bh(torch.as_tensor(n, dtype=torch.float32, device=dev), B, H)
    sb = None if slopes is None else _bh(slopes.to(dev), B, H)
    for b in range(B):
        ql = qlens[b]
        if ql == 0:
            continue
        vis = _rule_mask([lens[b]], [ql], ql, S, rule, dev)
        bias = None if sb is None else _bias(sb[b:b + 1], [lens[b]], [ql], H, ql, S, dev)
        ob, lb = reference(q[b:b + 1, :, :ql], kg[b:b + 1], vg[b:b + 1], vis, nb[b:b + 1], bias, scale)
        o[b, :, :ql] = ob[0]
        lse[b, :, :ql] = lb[0]
    return o, lse


def _check_all(pkg, out, lse, q, kg, vg, lens, qlens, n, rule, dtype, what, witness=True, scale=None, slopes=None):
    """the gates against reference_rows, padding rows exactly 0 / -inf, and the flash_attention_n witness. Returns the reference."""
    B, H, Sq, D = q.shape
    o_ref, lse_ref = reference_rows(q, kg, vg, lens, qlens, n, rule, scale, slopes)
    _check(out, o_ref, dtype, f"{what} out")
    _check_lse(lse, lse_ref, f"{what} lse")
    for b in range(B):   # padding: exactly 0 / -inf, whatever n is
        assert (out[b, :, qlens[b]:] == 0).all() and (lse[b, :, qlens[b]:] == float("-inf")).all(), f"{what}: padding rows of batch element {b}"
    if witness:
        qz = q.clone()
        for b in range(B):
            qz[b, :, qlens[b]:] = 0
        S = kg.shape[2]
        bias = None if slopes is None else _bias(slopes, lens, qlens, H, Sq, S, q.device)
        wit = pkg.flash_attention_n(qz, kg, vg, softmax_n_param=n, attn_mask=_rule_mask(lens, qlens, Sq, S, rule, q.device), attn_bias=bias, scale=scale)
        how = "(attn_bias)" if slopes is not None else "" if isinstance(rule, bool) else "(attn_mask)"
        _check(out, wit, dtype, f"{what} out vs flash_attention_n{how}")
    return o_ref, lse_ref


# ---------------------------------------------------------------- data
class _Paged:
    """A paged cache built from dense data: shuffled, non-contiguous page ids; every row at or beyond len_b inside a needed page is NaN,
    every table entry beyond the needed pages points at a poison page full of NaN."""

    def __init__(self, kd, vd, lens, page, max_pages, seed, alloc_all=False, spare=2, guard=None):
        B, Hkv, Smax, D = kd.shape
        dev, dtype = kd.device, kd.dtype
        assert Smax == page * max_pages
        need = [max_pages if alloc_all else (ln + page - 1) // page for ln in lens]
        n_ids = sum(need) + spare + 1
        gen = torch.Generator().manual_seed(seed)
        ids = torch.randperm(n_ids, generator=gen).tolist()
        self.poison = ids.pop()
        extra = 0 if guard is None else 1
        self.k = torch.full((n_ids + extra, page, Hkv, D), NAN, dtype=dtype, device=dev)
        self.v = torch.full((n_ids + extra, page, Hkv, D), NAN, dtype=dtype, device=dev)
        if guard is not None:   # trailing page no table names
            self.k[n_ids] = guard
            self.v[n_ids] = guard
        table = torch.full((B, max_pages), self.poison, dtype=torch.int32)
        for b in range(B):
            for s in range(need[b]):
                pid = ids.pop()
                table[b, s] = pid
                rows = max(0, min(page, lens[b] - s * page))
                if rows:
                    self.k[pid, :rows] = kd[b, :, s * page:s * page + rows].transpose(0, 1)
                    self.v[pid, :rows] = vd[b, :, s * page:s * page + rows].transpose(0, 1)
        self.table = table.to(dev)
        self.lens = torch.tensor(lens, dtype=torch.int32, device=dev)
        self.page, self.max_pages = page, max_pages


def _gather(pool, table, lens, page):
    """the visible rows of a paged cache as dense [B, Hkv, Smax, D] (rows at or beyond len_b: zeros) - read through the block table"""
    B, max_pages = table.shape
    need = max(1, max((ln + page - 1) // page for ln in lens))
    t = table[:, :need].long()
    d = pool[t]                                   # [B, need, page, Hkv, D]
    d = d.reshape(B, need * page, pool.shape[2], pool.shape[3]).permute(0, 2, 1, 3)
    keep = torch.arange(need * page, device=pool.device).view(1, 1, -1, 1) < torch.as_tensor(lens, device=pool.device).view(-1, 1, 1, 1)
    return torch.where(keep, d, torch.zeros_like(d)).contiguous()


def _visible_dense(kd, lens):
    """dense [B, Hkv, S, D] with the rows at or beyond len_b zeroed (what _gather gives for a paged cache)"""
    keep = torch.arange(kd.shape[2], device=kd.device).view(1, 1, -1, 1) < torch.as_tensor(lens, device=kd.device).view(-1, 1, 1, 1)
    return torch.where(keep, kd, torch.zeros_like(kd))


def _poke_rows(pc, b, lo, hi, value):
    """cache rows lo .. hi - 1 of batch element b, through the table"""
    for pos in range(lo, hi):
        pid = int(pc.table[b, pos // pc.page])
        pc.k[pid, pos % pc.page] = value
        pc.v[pid, pos % pc.page] = value


def _n_values(shape, dev, seed, zeros=True):
    n = synth.counter_normal(shape, seed, std=1.0, dtype=torch.float32, device=dev).abs() + 0.25
    if zeros:
        flat = n.view(-1)
        flat[::3] = 0.0   # exact zeros next to positive entries
    return n


def _case(dev, B, H, Hkv, Sq, D, dtype, page, lens, seed, max_pages=None):
    max_pages = max_pages or max(1, max((ln + page - 1) // page for ln in lens)) + 1
    q = _rand((B, H, Sq, D), dtype, dev, seed)
    kd = _rand((B, Hkv, page * max_pages, D), dtype, dev, seed + 1)
    vd = _rand((B, Hkv, page * max_pages, D), dtype, dev, seed + 2, std=1.0)
    return q, _Paged(kd, vd, lens, page, max_pages, seed)


def _first(ln, ql, W):
    return 64 * (max(0, ln - ql - W + 1) // 64)


def _poison(k, v, table, page, poison_id, lens, qlens, W):
    """rows below first_b: NaN; table entries of pages wholly below first_b: the poison page. `lens` are the lengths the forward sees
    (an append included). Returns the number of poisoned rows."""
    tbl = table.cpu()
    rows = 0
    for b, (ln, ql) in enumerate(zip(lens, qlens)):
        first = _first(ln, ql, W)
        rows += first
        for s in range(-(-first // page)):
            pid, cnt = int(tbl[b, s]), min(page, first - s * page)
            k[pid, :cnt] = NAN
            v[pid, :cnt] = NAN
        table[b, :first // page] = poison_id
    return rows


# ---------------------------------------------------------------- runners of the plain and the ALiBi calls
def _run_case_decode(pkg, dev, B, H, Hkv, Sq, D, dtype, page, lens, n, causal=True, seed=1, max_pages=None, what="", witness=True, scale=None):
    max_pages = max_pages or max(1, max((ln + page - 1) // page for ln in lens)) + 1
    Smax = page * max_pages
    q = _rand((B, H, Sq, D), dtype, dev, seed)
    kd = _rand((B, Hkv, Smax, D), dtype, dev, seed + 1)
    vd = _rand((B, Hkv, Smax, D), dtype, dev, seed + 2, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, seed)
    out, lse = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, is_causal=causal,
                                             return_lse=True, scale=scale)
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)
    vis = _visibility(lens, Sq, kg.shape[2], causal, dev)
    o_ref, lse_ref = reference(q, kg, vg, vis, n, None, scale)
    _check(out, o_ref, dtype, f"{what} out")
    _check_lse(lse, lse_ref, f"{what} lse")
    if witness:
        wit = pkg.flash_attention_n(q, kg, vg, softmax_n_param=n, attn_mask=vis, scale=scale)
        _check(out, wit, dtype, f"{what} out vs flash_attention_n")
    return out, lse, o_ref, lse_ref


def _run_case_prefill(pkg, dev, B, H, Hkv, Sq, D, dtype, page, lens, n, causal=True, seed=1, max_pages=None, what="", witness=True, scale=None, qlens=None):
    """no append: `lens` are the keys in the cache"""
    max_pages = max_pages or max(1, max((ln + page - 1) // page for ln in lens)) + 1
    Smax = page * max_pages
    q = _rand((B, H, Sq, D), dtype, dev, seed)
    kd = _rand((B, Hkv, Smax, D), dtype, dev, seed + 1)
    vd = _rand((B, Hkv, Smax, D), dtype, dev, seed + 2, std=1.0)
    pc = _Paged(kd, vd, lens, page, max_pages, seed)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, query_seqlens=qs, softmax_n_param=n,
                                                     is_causal=causal, return_lse=True, scale=scale)
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)
    _check_all(pkg, out, lse, q, kg, vg, lens, qlens or [Sq] * B, n, causal, dtype, what, witness, scale)
    return out, lse


def _run_alibi_decode(pkg, dev, B, H, Hkv, Sq, D, dtype, page, lens, n, slopes, causal=True, seed=1, max_pages=None, what="", witness=True, scale=None):
    q, pc = _case(dev, B, H, Hkv, Sq, D, dtype, page, lens, seed, max_pages)
    out, lse = pkg.flash_attention_n_kvcache(q, pc.k, pc.v, pc.lens, block_table=pc.table, softmax_n_param=n, is_causal=causal,
                                             return_lse=True, scale=scale, alibi_slopes=slopes)
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)
    o_ref, lse_ref = _check_all(pkg, out, lse, q, kg, vg, lens, [Sq] * B, n, causal, dtype, what, witness, scale, slopes)
    return out, lse, o_ref, lse_ref, q, pc


def _run_alibi_prefill(pkg, dev, B, H, Hkv, Sq, D, dtype, page, lens, n, slopes, causal=True, seed=1, max_pages=None, what="", witness=True, scale=None,
                       qlens=None):
    q, pc = _case(dev, B, H, Hkv, Sq, D, dtype, page, lens, seed, max_pages)
    qs = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache_prefill(q, pc.k, pc.v, pc.lens, block_table=pc.table, query_seqlens=qs, softmax_n_param=n,
                                                     is_causal=causal, return_lse=True, scale=scale, alibi_slopes=slopes)
    kg, vg = _gather(pc.k, pc.table, lens, page), _gather(pc.v, pc.table, lens, page)
    _check_all(pkg, out, lse, q, kg, vg, lens, qlens or [Sq] * B, n, causal, dtype, what, witness, scale, slopes)
    return out, lse, q, pc


def _steep(H, dev):
    """slopes between 0.25 and 0.5: a key 256 positions back is 64 .. 128 nats down, so the weight sits in the last split's keys"""
    return torch.linspace(0.25, 0.5, H, device=dev)


def _alibi_operand(pkg):
    s = pkg._lib.AlibiSlopes()
    s.slopes, s.stride_b, s.stride_h = 1 << 20, 0, 1   # (plans only: never dereferenced)
    return s


# ---------------------------------------------------------------- graph capture, packed offsets, bits
def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = fn()
    return g, res


def _cu(qlens, dev):
    return torch.tensor([0] + list(itertools.accumulate(qlens)), dtype=torch.int32, device=dev)


def _bits(t):
    return t.view(torch.int16)


# ---------------------------------------------------------------- rotary tables and the eager rotation
def _tables(rows, rd, dev, dtype, base=10000.0):
    inv = base ** (-torch.arange(0, rd, 2, dtype=torch.float64) / rd)
    ang = torch.arange(rows, dtype=torch.float64)[:, None] * inv[None]
    return ang.cos().to(dtype).to(dev), ang.sin().to(dtype).to(dev)


def _rotate(x, pos, cos, sin, interleaved):
    """x [B, heads, S, D] in a 16-bit type, pos [B, S] (any integers: clamped to the table's rows here, as the kernel clamps). Eager torch,
    fp32, every product and the sum an operation of its own, one rounding to x.dtype."""
    rd = 2 * cos.shape[1]
    p = pos.clamp(0, cos.shape[0] - 1).to(x.device)
    c, s = cos[p].float()[:, None], sin[p].float()[:, None]   # [B, 1, S, rd / 2]
    if interleaved:
        x1, x2 = x[..., 0:rd:2].float(), x[..., 1:rd:2].float()
    else:
        x1, x2 = x[..., :rd // 2].float(), x[..., rd // 2:rd].float()
    y1 = (x1 * c - x2 * s).to(x.dtype)
    y2 = (x2 * c + x1 * s).to(x.dtype)
    out = x.clone()
    if interleaved:
        out[..., 0:rd:2], out[..., 1:rd:2] = y1, y2
    else:
        out[..., :rd // 2], out[..., rd // 2:rd] = y1, y2
    return out


# ---------------------------------------------------------------- plans
def _plan_names(pkg, **shape):
    return [k[0].split("<")[0] for k in pkg._lib.kvprefill_plan(kv_args._args_prefill(pkg, **shape))]


def _varlen_plan(pkg, B, H, Hkv, Sq, D, T, page, max_pages, dtype=torch.bfloat16):
    return pkg._lib.kvvarlen_plan(kv_args._args_varlen(pkg, B=B, H=H, Hkv=Hkv, Sq=Sq, D=D, T=T, page=page, max_pages=max_pages, dtype=1 if dtype == torch.bfloat16 else 0))


def _varlen_nsplit(plan, B, Hkv, Sq, T, PB):
    return plan[1][1] // (kv_args.items_max(B, Sq, T, PB) * Hkv)


VARLEN_SPLIT = dict(H=8, Hkv=1, D=64, page=256, max_pages=16, qlens=[1, 40])


def _varlen_split_plan(pkg):
    c = VARLEN_SPLIT
    plan = _varlen_plan(pkg, 2, c["H"], c["Hkv"], 40, c["D"], 41 + 7, c["page"], c["max_pages"])
    assert [k[0].split("<")[0] for k in plan] == ["fasn_kvvarlen_schedule_kernel", "fasn_kvvarlen_fwd_kernel", "fasn_kvvarlen_combine_kernel"]
    assert _varlen_nsplit(plan, 2, c["Hkv"], 40, 48, 16) >= 2
