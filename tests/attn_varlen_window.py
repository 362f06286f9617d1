"""What the tests of flash_attention_n_varlen(..., window=) share (tests/test_attnvarlenwindow_cpu.py, tests/test_gpu_attnvarlenwindow.py;
DESIGN 4.26). A plain module: no tests, importable without a GPU. It builds on tests/attn_varlen.py (packs, operands, gates, the C ABI
blocks), tests/attn_witness.py and tests/attn_varlen_witness.py (the fp64 reference and the per-element gates) and adds no tolerance.

  band        the rule: row i of a sequence (sq, sk) sits at p_i = i + (sk - sq) and sees key j iff 0 <= j < sk and p_i - window < j <= p_i
  LONGW       a pack whose first sequence puts the rebased walk two tiles and more up (q0 = 512, window = 64: the walk starts at key 448)
  reference   av.reference's method under the band: oracle.ref_attention.ref_attention_n(attn_mask=band) in fp32, sequence by sequence,
              rows that see no key left out of its call; lse from its definition under the same mask. Cached and never modified.
  fwd_walk / dkdv_walk   the three walks of csrc in integers - the forward's and dQ's rebase, tile range and per-wave skips, the dK/dV
              kernel's query-tile range and per-wave skips - and contract_*: the bounds include/fasn.h states, written from its text
  run_abi     forward and backward through fasn_fwd_varlen_window / fasn_bwd_varlen_window on caller-allocated outputs
  WindowWorld one attn_witness.Case per sequence under the band (the band goes in as the case's boolean mask `um`), witness B's bounded code
              aimed at the window's first / middle / last visible key, witness C's operands; judged by avw.judge, unchanged"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_varlen as av            # noqa: E402
import attn_witness as aw           # noqa: E402
import attn_varlen_witness as avw   # noqa: E402
from oracle.ref_attention import ref_attention_n   # noqa: E402

D = 64
KT = QT = 64      # keys per K/V tile of the forward and dQ kernels, rows per Q/dO tile of the dK/dV kernel
BLOCK = 128       # rows / keys of a work item
WAVE = 32         # rows / keys of a wave inside it
WINDOWS = (1, 63, 64, 65, 128, 200)
LONGW = av.Pack([700, 1, 130], tail_q=20)
PACKS = {"seams": av.SEAMS, "unequal": av.UNEQUAL, "longw": LONGW}
POISON_K = (av.Pack([128], [1000]), 100, 768)     # (pack, window, K / V rows [0, 768) hold NaN)
POISON_Q = (av.Pack([600]), 64, 384, 256)         # (pack, window, q / dO rows [384, 600) hold NaN, dk / dv rows [0, 256) are judged)


def band(sq, sk, window):
    """bool [sq, sk]: band[i, j] = (j <= p_i) & (j > p_i - window), p_i = i + (sk - sq)"""
    p = torch.arange(sq).unsqueeze(-1) + (sk - sq)
    j = torch.arange(sk).unsqueeze(0)
    return (j <= p) & (j > p - window)


def count(sq, sk, window):
    """keys row i sees: clamp(min(window, p_i + 1), 0, ...) - an int64 [sq]"""
    return band(sq, sk, window).sum(1)


_REF = {}


def reference(key, pack, inp, n, window, log_n=None):
    """av.reference under the band, cached under `key`: out [Tq, H, D], lse [H, Tq], dq, dk, dv and - with log_n, an [H] tensor s whose
    n is exp(s) - ds. Rows that see no key: out 0, lse log n (-inf at n = 0), no gradient; rows beyond the last sequence: 0 / -inf."""
    if key in _REF:
        return _REF[key]
    q, k, v = (inp[x].float().requires_grad_() for x in ("q", "k", "v"))
    do = inp["do"].float()
    s = None if log_n is None else log_n.detach().float().cpu().requires_grad_()
    Hq, Hkv, Dh = q.shape[1], k.shape[1], q.shape[2]
    G = Hq // Hkv
    out = torch.zeros(pack.Tq, Hq, Dh)
    lse = torch.full((Hq, pack.Tq), -math.inf)
    pieces = []
    for b in range(pack.B):
        q0, q1, k0, k1 = pack.cu_q[b], pack.cu_q[b + 1], pack.cu_k[b], pack.cu_k[b + 1]
        sq, sk = q1 - q0, k1 - k0
        if sq == 0:
            continue
        m = band(sq, sk, window)
        live = m.any(1)
        for h in range(Hq):
            nh = float(n) if s is None else torch.exp(s[h])
            nv = float(nh.detach()) if torch.is_tensor(nh) else nh
            qb, kb, vb = q[q0:q1, h], k[k0:k1, h // G], v[k0:k1, h // G]
            if live.any():
                ob = ref_attention_n(qb[live], kb, vb, softmax_n_param=nh, attn_mask=m[live])
                pieces.append((ob * do[q0:q1, h][live]).sum())
                out[q0:q1, h][live] = ob.detach()
            with torch.no_grad():
                x = (qb @ kb.t() / math.sqrt(Dh)).masked_fill(~m, -math.inf) if sk else torch.empty(sq, 0)
                sink = torch.full((sq, 1), math.log(nv) if nv > 0 else -math.inf)
                lse[h, q0:q1] = torch.logsumexp(torch.cat([x, sink], dim=1), dim=1)
    if pieces:
        torch.stack(pieces).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad   # noqa: E731
    r = dict(out=out, lse=lse, dq=zero(q), dk=zero(k), dv=zero(v), ds=None if s is None else zero(s))
    _REF[key] = r
    return r


# ---------------------------------------------------------------- the walks, in integers
def _fdiv(a, b):
    """C's a / b for a >= 0 (the kernels divide non-negative values only)"""
    assert a >= 0
    return a // b


def fwd_walk(sq, sk, window, q0):
    """The forward's and the dQ kernel's walk of the 128-row block at q0 < sq (varlen_window_rebase, then the causal walk on the rebased
    keys): dict(klo, tiles=(first, last) absolute 64-key tile indices or None, waves=[per 32-row wave the list of absolute tiles it
    computes on]). A wave without rows computes on nothing."""
    assert 0 <= q0 < sq and q0 % BLOCK == 0
    coff = sk - sq
    klo = KT * _fdiv(max(0, q0 + coff - window + 1), KT)
    sk2, coff2 = sk - klo, coff - klo
    ntiles = -(-sk2 // KT)
    kmax = min(q0 + BLOCK, sq) - 1 + coff2
    ntiles = min(ntiles, 0 if kmax < 0 else kmax // KT + 1)
    waves = []
    for w in range(BLOCK // WAVE):
        qw0 = q0 + w * WAVE
        mine = []
        for t in range(ntiles):
            k0 = t * KT
            skip = k0 > qw0 + WAVE - 1 + coff2                # beyond the last row's own position
            skip = skip or (k0 + KT - 1 <= qw0 + coff2 - window)   # below the first row's window
            skip = skip or qw0 >= sq
            if not skip:
                mine.append(klo // KT + t)
        waves.append(mine)
    return dict(klo=klo, tiles=(klo // KT, klo // KT + ntiles - 1) if ntiles > 0 else None, waves=waves)


def dkdv_walk(sq, sk, window, k0):
    """The dK/dV kernel's walk of the 128-key block at k0 < sk: dict(tiles=(first, last) 64-row query tiles or None, waves=[per 32-key
    wave the list of query tiles it computes on])."""
    assert 0 <= k0 < sk and k0 % BLOCK == 0
    coff = sk - sq
    ntq = -(-sq // QT)
    first_row = k0 - coff
    tq0 = 0 if first_row <= 0 else first_row // QT
    last_row = min(k0 + BLOCK, sk) - 1 - coff + window - 1
    ntq = min(ntq, 0 if last_row < 0 else last_row // QT + 1)
    waves = []
    for w in range(BLOCK // WAVE):
        kw0 = k0 + w * WAVE
        mine = []
        for tq in range(tq0, ntq):
            r0 = tq * QT
            skip = (r0 + QT - 1 + coff) < kw0                       # even the last row's position lies below my keys
            skip = skip or (kw0 + WAVE - 1 <= r0 + coff - window)   # even the first row's window lies above them
            if not skip:
                mine.append(tq)
        waves.append(mine)
    return dict(tiles=(tq0, ntq - 1) if ntq > tq0 else None, waves=waves)


def contract_first_key(sq, sk, window, q0):
    """include/fasn.h: the forward and the dQ kernel read no K / V row of the sequence below this one"""
    return 64 * (max(0, q0 + (sk - sq) - window + 1) // 64)


def contract_last_qtile(sq, sk, window, k0):
    """include/fasn.h: the dK/dV kernel uses no row of a 64-row tile beyond this one (negative: no tile at all)"""
    last_key = min(k0 + BLOCK, sk) - 1
    return (last_key - (sk - sq) + window - 1) // 64   # (Python's floor: negative values stay negative)


def rows_read_fwd(sq, sk, window):
    """the smallest and largest K / V row of the sequence any block's walk of the forward / dQ kernel touches, or None"""
    lo = hi = None
    for q0 in range(0, sq, BLOCK):
        t = fwd_walk(sq, sk, window, q0)["tiles"]
        if t is not None:
            lo = t[0] * KT if lo is None else min(lo, t[0] * KT)
            hi = t[1] * KT + KT - 1 if hi is None else max(hi, t[1] * KT + KT - 1)
    return lo, hi


# ---------------------------------------------------------------- the call and the C ABI
def call(pkg, dev, pack, inp, n, window, cu=None, causal=True):
    """flash_attention_n_varlen(..., is_causal=causal, window=window) and its backward: out, lse, dq, dk, dv"""
    q, k, v = (inp[x].to(dev).requires_grad_() for x in ("q", "k", "v"))
    cu_q, cu_k = pack.cu(dev) if cu is None else cu
    out, lse = pkg.flash_attention_n_varlen(q, k, v, cu_q, pack.max_q, None if pack.self_attn else cu_k, pack.max_k, softmax_n_param=n,
                                            is_causal=causal, return_lse=True, window=window)
    out.backward(inp["do"].to(dev))
    torch.cuda.synchronize()
    return dict(out=out.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def window_block(pkg, window, reserved=0):
    w = pkg._lib.KvWindow()
    w.window, w.reserved = window, reserved
    return w


def run_abi(pkg, pack, t, n, window, cu_q, cu_k):
    """av.run_abi through fasn_fwd_varlen_window and fasn_bwd_varlen_window (causal): the two codes"""
    L = pkg._lib
    lib = L.load()
    q = t["q"]
    a = L.BwdArgs()
    f = a.fwd
    f.q, f.k, f.v, f.o = (av.view_packed(pkg, t[x]) for x in ("q", "k", "v", "o"))
    f.lse = t["lse"].data_ptr()
    f.mask.ptr = f.bias.ptr = None
    f.bias_dtype = 0
    f.dtype = L.FASN_DTYPE_F16 if q.dtype == torch.float16 else L.FASN_DTYPE_BF16
    f.B, f.H, f.Sq, f.Sk, f.D, f.Dv = 1, q.shape[1], q.shape[0], t["k"].shape[0], q.shape[2], q.shape[2]
    f.scale, f.softmax_n, f.causal, f.dropout_p = 1.0 / math.sqrt(q.shape[2]), n, 1, 0.0
    f.seed = f.offset = 0
    f.kv_group = q.shape[1] // t["k"].shape[1] if t["k"].shape[1] != q.shape[1] else 0
    f.rng_state = None
    vl = L.Varlen()
    vl.cu_seqlens_q, vl.cu_seqlens_k = cu_q.data_ptr(), cu_k.data_ptr()
    vl.num_seqs, vl.max_seqlen_q, vl.max_seqlen_k, vl.reserved = pack.B, pack.max_q, pack.max_k, 0
    win = window_block(pkg, window)
    stream = torch.cuda.current_stream(q.device).cuda_stream
    with torch.cuda.device(q.device):
        rc_f = lib.fasn_fwd_varlen_window(a.fwd, vl, win, None, 0, stream)
        rc_b = None
        if rc_f == 0:
            a.dout, a.dq, a.dk, a.dv = (av.view_packed(pkg, t[x]) for x in ("do", "dq", "dk", "dv"))
            a.delta = t["delta"].data_ptr()
            a.workspace, a.workspace_bytes, a.flags, a.dbias_dtype = None, 0, 0, 0
            a.dbias.ptr = None
            rc_b = lib.fasn_bwd_varlen_window(a, vl, win, stream)
    torch.cuda.synchronize(q.device)
    return rc_f, rc_b


# ---------------------------------------------------------------- named plan cases (tests/golden/attn_varlen_window_plans.txt)
def plan_cases():
    """name -> (keyword arguments of av.block, window, plan): forward and backward, grouped and not, window in {1, 64, 128} at max_q = 300"""
    out = {}
    for Hkv in (8, 2):
        for window in (1, 64, 128):
            for which in (0, 1):
                name = f"D64_w{window}_{'gqa4' if Hkv != 8 else 'mha'}_{'bwd' if which else 'fwd'}"
                out[name] = (dict(Tq=2100, Tk=2100, Hq=8, Hkv=Hkv, D=64, causal=True, num_seqs=14, max_q=300), window, which)
    out["D64_f16_w64_unequal_bwd"] = (dict(Tq=700, Tk=520, Hq=4, Hkv=4, D=64, dtype=torch.float16, causal=True, num_seqs=6, max_q=257, max_k=200), 64, 1)
    return out


# ---------------------------------------------------------------- the witnesses under the band
WHERE = ("first", "middle", "last")


def _target(m, where):
    """t [L]: the band's first / middle / last visible key of every row, -1 where the row sees none"""
    L, S = m.shape
    if S == 0:
        return torch.full((L,), -1, dtype=torch.long)
    jj = torch.arange(S).view(1, S)
    cnt = m.sum(1)
    last = torch.where(m, jj, torch.full_like(jj, -1)).amax(1)
    first = last - cnt + 1      # (a row's visible keys are contiguous)
    t = {"first": first, "last": last, "middle": first + (cnt - 1) // 2}[where]
    return torch.where(cnt > 0, t, torch.full_like(t, -1))


def inputs_b_band(case, m, where, dtype, dev, seed, n):
    """witness B's bounded code (aw.inputs_b, form "code") aimed inside a band: k_jd = +-1 by bit d of j over 12 bits, q_i = g k_t(i) with
    t(i) the band's first / middle / last visible key of row i, g = 4, scale = 4: the target's logit is 16 * 12 = 192 and every other
    key's at most 160 (one differing bit costs 32). Rows that see no key get q = 0. V, dO as aw.inputs_b draws them."""
    B, H, Hkv, L, S = case.B, case.H, case.Hkv, case.L, case.S
    assert B == 1 and case.ub == 1 and case.uh == H and S <= 4096
    scale, g = 4.0, 4.0
    j = torch.arange(S)
    k1 = torch.zeros(S, D)
    for d in range(12):
        k1[:, d] = 1.0 - 2.0 * ((j >> d) & 1).float()
    t = _target(m, where)
    uq = (g * k1[t.clamp_min(0)] * (t >= 0).unsqueeze(-1).float()).view(1, 1, L, D).expand(1, H, L, D)
    k = k1.view(1, 1, S, D).repeat(1, Hkv, 1, 1).to(dtype).to(dev)
    uv = aw._counter_normal((1, case.uhk, S, D), seed + 1, 1.0, dtype, dev)
    uv = torch.where(uv.abs() < 2.0 ** -12, torch.ones_like(uv), uv)
    udo = aw._counter_normal((1, H, L, D), seed + 2, 1.0, dtype, dev)
    udo = torch.where(udo.abs() < 2.0 ** -12, torch.ones_like(udo), udo)
    nt, un = aw.n_values(case, dev, given=n)
    return dict(q=uq.contiguous().to(dtype).to(dev), k=k, v=aw._tile(case, uv, "kv"), do=aw._tile(case, udo), n=nt, un=un, mask=None, um=None,
                bias=None, ubias=None, scale=scale)


class WindowWorld(avw.World):
    """avw.World under a window: per live sequence b the case Case(1, H, sq_b, sk_b, 64, Hkv, causal=True) with the band as its boolean
    mask - it enters as inp["um"], which aw.reference multiplies into the causal visible set -, witness B's code aimed at `form` (one of
    WHERE) or witness C's operands at `std`, the fp64 reference and the gates. Never modified."""

    def __init__(self, wp, wit, dtype, dev, window, form=None, std=None, seed=0):
        assert wit in ("B", "C")
        self.wp, self.wit, self.dt, self.dev, self.causal, self.std, self.backward = wp, wit, dtype, dev, True, std, True
        self.where, self.form, self.window = form, "code", window
        p = wp.pack
        self.n = avw.n_of(wp, wit)
        self.seq = {}
        g = torch.Generator().manual_seed(1900 + seed)
        junk = lambda T, heads: (2.0 * torch.randn(T, heads, D, generator=g)).to(dtype).to(dev)   # noqa: E731
        self.q, self.do = junk(p.Tq, wp.H), junk(p.Tq, wp.H)
        self.k, self.v = junk(p.Tk, wp.Hkv), junk(p.Tk, wp.Hkv)
        self.scale = None
        u, ua = aw.U[dtype], aw.unit_abs(dtype)
        for b in wp.live():
            case = wp.case(b, True).but(mask="dense")   # (a case with a boolean mask: the band below)
            m = band(case.L, case.S, window)
            sd = 7919 * seed + 31 * b + 5
            if wit == "B":
                inp = inputs_b_band(case, m, form, dtype, dev, sd, self.n)
            else:
                inp = aw.inputs_c(case.but(mask=None), std, dtype, dev, sd, n=self.n)
            inp["um"] = m.view(1, 1, case.L, case.S)
            assert self.scale in (None, inp["scale"]), "one scale per call"
            self.scale = inp["scale"]
            rq, rk = av.seq_rows(p, "q", b), av.seq_rows(p, "k", b)
            self.q[rq], self.do[rq] = inp["q"][0].transpose(0, 1), inp["do"][0].transpose(0, 1)
            self.k[rk], self.v[rk] = inp["k"][0].transpose(0, 1), inp["v"][0].transpose(0, 1)
            r = aw.reference(case, inp)
            gates = aw.with_bounds(case, inp, r, u, ua)
            inp = {key: (val.cpu() if torch.is_tensor(val) else val) for key, val in inp.items()}
            self.seq[b] = (case, inp, r, gates)
        assert self.scale is not None


def run_world(pkg, w):
    """flash_attention_n_varlen(..., is_causal=True, window=w.window) on the world's packed operands and its backward, as avw.run returns"""
    p = w.wp.pack
    cu_q, cu_k = p.cu(w.dev)
    q, k, v = (t.detach().clone().requires_grad_() for t in (w.q, w.k, w.v))
    n = w.n.to(w.dev).requires_grad_()
    out, lse = pkg.flash_attention_n_varlen(q, k, v, cu_q, p.max_q, None if p.self_attn else cu_k, p.max_k, softmax_n_param=n, scale=w.scale,
                                            is_causal=True, return_lse=True, window=w.window)
    out.backward(w.do)
    torch.cuda.synchronize(w.dev)
    return dict(out=out.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dn=n.grad)
