"""Three witnesses for the K/V-cache calls whose expected values are exact or carry a derived bound, compared per row and per element.

Why. The K/V tests draw q, k ~ N(0, 0.5^2): at D = 64 the logits have a standard deviation of 0.25, every softmax is close to a plain
average, the running maximum hardly moves and the split-K combine weights are all about 1. Their gate (kv_support._check) is one
number per tensor, REL_TRUE * max|want|, which the rows of short sequences set for the rows of long ones. A fault that depends on the
position - a causal limit one key off in the rows of one sequence, a 64-key tile dropped at a seam, a split merged with the wrong weight -
moves a long row by less than that and passes. The witnesses below make one key (or one count) decide every row:

  A  query = 0: every logit is 0, every p is 1. V is an indicator pattern, so Z_i = exp(lse_i) is n plus the number of visible keys and
     out_id * Z_i counts the visible keys of class d. Every visible key is seen exactly once, in every row.
  B  q.k_j = j + 1 (or 65536 - j) in exact integer arithmetic and scale = 32: neighbouring keys lie 32 nats apart, one key (the last or
     the first visible one, or the sink) takes the whole row, and out_i is that key's V row to two roundings.
  C  random operands at a logit standard deviation of 4 and 8, gated per element by 3 u A_id with A_id = sum_j p_ij |v_jd|.

The reference (visible / attend / reference) is written from the docstrings of kvcache.py alone, on the CPU in fp64: qlen_b,
len_b = clamp(cache_seqlens[b] + (qlen_b if appended), 0, capacity), p_i = i + len_b - qlen_b, key j visible to position i iff j < len_b
and (causal) j <= p_i and (window) j > p_i - W. It shares no code with _visibility, _win_mask or _reference of the other test files.

One adapter table (ROUTES) drives every witness through the calls: flash_attention_n_kvcache, flash_attention_n_kvcache_prefill (with and
without query_seqlens and k_new / v_new), flash_attention_n_kvcache_window (decode and prefill kernels), flash_attention_n_kvcache_varlen,
and the two base calls with alibi_slopes (witness C only). Rotary stays out: it is tested bit for bit against these forwards fed
torch-rotated inputs, and a rotation destroys the operand patterns of A and B.

This is a helper module (no test is collected from it). tests/test_kvwitness_cpu.py is the test of these tests: it mutates the visible
set of the reference and asserts that each witness's gate breaks by 10x; tests/test_gpu_kvwitness.py runs the kernels."""
import itertools
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_support as ks   # noqa: E402

_rand, _Paged, _n_values, _poison = ks._rand, ks._Paged, ks._n_values, ks._poison
NAN = float("nan")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # unit roundoff of the operand / output type
KT = 64   # keys per tile in every K/V kernel


class Case:
    """One shape of one route. `lens`: keys in the cache BEFORE the call; `qlens`: query positions per sequence (None: Sq each)."""

    def __init__(self, route, H, Hkv, D, Sq, lens, page=64, max_pages=None, qlens=None, causal=True, window=None, append=False,
                 alibi=False, long=False, tail=7):
        self.route, self.H, self.Hkv, self.D, self.Sq, self.page = route, H, Hkv, D, Sq, page
        self.lens, self.B = list(lens), len(lens)
        self.qlens = [Sq] * self.B if qlens is None else list(qlens)
        self.ragged = qlens is not None
        self.causal, self.window, self.append, self.alibi, self.long, self.tail = causal, window, append, alibi, long, tail
        self.total = [ln + (ql if append else 0) for ln, ql in zip(self.lens, self.qlens)]   # len_b, below the capacity by construction
        self.max_pages = max_pages or max(1, max((t + page - 1) // page for t in self.total)) + 1
        self.cap = page * self.max_pages
        assert max(self.total) <= self.cap and max(self.qlens) <= Sq and (window is None or causal)

    def but(self, **kw):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(kw)
        return c


# ---------------------------------------------------------------- the reference: fp64, from the docstrings of kvcache.py
def visible(len_b, qlen_b, S, causal, window):
    """[qlen_b, S] bool: position i sees key j iff j < len_b and (causal) j <= p_i and (window) j > p_i - W, p_i = i + len_b - qlen_b"""
    i = torch.arange(qlen_b).view(-1, 1)
    j = torch.arange(S).view(1, -1)
    p = i + len_b - qlen_b
    vis = (j < len_b).expand(qlen_b, S).clone()
    if causal:
        vis &= j <= p
    if window is not None:
        vis &= j > p - window
    return vis


def attend(q, k, v, w, n, scale, bias=None):
    """softmax_n attention of one sequence in fp64. q [H, L, D], k / v [Hkv, S, D], n [H], all fp64 on the CPU; w [L, S]: how often
    position i counts key j (0: hidden, 1: visible; the test of these tests also passes 2). bias [H, L, S] is added to the scaled
    logits. Returns out, A = sum_j p_ij |v_jd| [H, L, D], lse [H, L] and the un-normalised sums: the reference point m [H, L] (the largest
    visible logit; at least 0 where n > 0; 0 where nothing is visible), l = n e^-m + sum_j w_ij e^(x_ij - m), acc = sum_j w_ij e^(x_ij - m) v_j,
    and x, the logits ([H, L, S], -inf where hidden)."""
    H, L, D = q.shape
    Hkv, S, _ = k.shape
    G = H // Hkv
    x = scale * torch.einsum("kgld,ksd->kgls", q.view(Hkv, G, L, D), k).reshape(H, L, S)
    if bias is not None:
        x = x + bias
    x = torch.where(w > 0, x, torch.full_like(x, -math.inf))
    m = x.amax(-1) if S else torch.full((H, L), -math.inf, dtype=torch.float64)
    m = torch.where(n.view(H, 1) > 0, m.clamp_min(0.0), m)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = w * torch.exp(x - m.unsqueeze(-1))
    l = torch.where(n.view(H, 1) > 0, n.view(H, 1) * torch.exp(-m), torch.zeros_like(m)) + e.sum(-1)
    e5 = e.view(Hkv, G, L, S)
    acc = torch.einsum("kgls,ksd->kgld", e5, v).reshape(H, L, D)
    acc_abs = torch.einsum("kgls,ksd->kgld", e5, v.abs()).reshape(H, L, D)
    safe = torch.where(l > 0, l, torch.ones_like(l)).unsqueeze(-1)
    lse = torch.where(l > 0, m + torch.log(torch.where(l > 0, l, torch.ones_like(l))), torch.full_like(m, -math.inf))
    return dict(out=acc / safe, A=acc_abs / safe, lse=lse, m=m, l=l, acc=acc, x=x)


def alibi_bias(slopes_b, len_b, qlen_b, S):
    """[H, qlen_b, S] fp64: -slope_h * |p_i - j|"""
    p = torch.arange(qlen_b, dtype=torch.float64).view(1, -1, 1) + (len_b - qlen_b)
    j = torch.arange(S, dtype=torch.float64).view(1, 1, -1)
    return -(slopes_b.view(-1, 1, 1) * (p - j).abs())


def sequence(case, inp, b):
    """(q [H, qlen_b, D], k, v [Hkv, capacity, D], n [H], slopes [H] or None) of sequence b in fp64 on the CPU: the operands as the
    kernels get them, widened exactly. k / v hold every row of the dense picture; the caller slices to the rows it looks at."""
    f = lambda t: t.detach().to("cpu", torch.float64)   # noqa: E731
    n = f(inp["n"])
    n = n.reshape((1,) * (2 - n.dim()) + tuple(n.shape)).expand(case.B, case.H)[b]
    sl = None
    if inp.get("slopes") is not None:
        sl = f(inp["slopes"])
        sl = sl.reshape((1,) * (2 - sl.dim()) + tuple(sl.shape)).expand(case.B, case.H)[b]
    return f(inp["q"][b, :, :case.qlens[b]]), f(inp["kd"][b]), f(inp["vd"][b]), n, sl


def reference(case, inp):
    """per sequence b: attend() over the keys 0 .. len_b - 1 with the visible set of the docstrings; a list of B dicts"""
    res = []
    for b in range(case.B):
        q, k, v, n, sl = sequence(case, inp, b)
        ln, ql = case.total[b], case.qlens[b]
        w = visible(ln, ql, ln, case.causal, case.window).double()
        bias = None if sl is None else alibi_bias(sl, ln, ql, ln)
        res.append(attend(q, k[:, :ln], v[:, :ln], w, n, inp["scale"], bias))
    return res


# ---------------------------------------------------------------- the operands of the three witnesses
def head_shift(case, dtype):
    """Witness A's per-head constant is (hkv + 1) * 2^-k: k is the smallest shift at which the constant's class count, at most
    Hkv * 2^-k * max len_b, keeps the output's own rounding under 0.2 (the condition the test asserts from the reference)."""
    k = 0
    while case.Hkv * 2.0 ** -k * max(max(case.total), 1) * U[dtype] > 0.2:
        k += 1
    return k


GRANULE = {torch.float16: KT, torch.bfloat16: KT // 2}


def inputs_a(case, dtype, dev, seed):
    """query = 0; any finite K; V[j, d] = 1 for d = j mod (D/2) and for d = D/2 + (j // 64) mod (D/2 - 1), else 0: the key's place inside
    its half tile and its tile. The last feature is the spare class: it holds (hkv + 1) * 2^-k for every key of K/V head hkv, so that a
    query head that reads another K/V head's cache shows. Every value is exact in fp16 and bf16.

    In bf16 the second half counts half tiles, (j // 32): one rounding of the output is up to 2^-8 of its value, and against the gate of
    0.25 the 64 keys of one whole tile in one class would leave no room (64 * 2^-8 = 0.25), 32 do (0.125)."""
    B, H, Hkv, D, cap = case.B, case.H, case.Hkv, case.D, case.cap
    q = torch.zeros(B, H, case.Sq, D, dtype=dtype, device=dev)
    kd = _rand((B, Hkv, cap, D), dtype, dev, seed)
    j = torch.arange(cap, device=dev)
    v = torch.zeros(cap, D, dtype=torch.float32, device=dev)
    v[j, j % (D // 2)] = 1.0
    v[j, D // 2 + (j // GRANULE[dtype]) % (D // 2 - 1)] = 1.0
    vd = v.view(1, 1, cap, D).repeat(B, Hkv, 1, 1)
    vd[:, :, :, D - 1] = ((torch.arange(Hkv, device=dev) + 1).float() * 2.0 ** -head_shift(case, dtype)).view(1, Hkv, 1)
    return dict(q=q, kd=kd, vd=vd.to(dtype), n=_n_values((H,), dev, seed + 1), scale=1.0 / math.sqrt(D))


B_FORMS = ("ascending", "descending", "sink")


def inputs_b(case, form, dtype, dev, seed):
    """q_d = 16^d for d < 4, k_jd = base-16 digit d of j (descending: 15 - digit), feature 4 is 1 in both, the rest 0; scale = 32. The
    MFMA sum is the integer j + 1 (descending: 65536 - j), every operand is exact in fp16 and bf16, and the logit is 32 (j + 1) nats.
    sink: q negated, every logit <= -32. V is random normal without exact zeros. n per head has zeros and positives."""
    B, H, Hkv, D, cap = case.B, case.H, case.Hkv, case.D, case.cap
    assert form in B_FORMS and cap <= 16 ** 4
    q = torch.zeros(B, H, case.Sq, D, dtype=torch.float32, device=dev)
    for d in range(4):
        q[..., d] = 16.0 ** d
    q[..., 4] = 1.0
    if form == "sink":
        q = -q
    j = torch.arange(cap, device=dev)
    k = torch.zeros(cap, D, dtype=torch.float32, device=dev)
    for d in range(4):
        digit = (j // 16 ** d) % 16
        k[:, d] = (15 - digit if form == "descending" else digit).float()
    k[:, 4] = 1.0
    kd = k.view(1, 1, cap, D).repeat(B, Hkv, 1, 1).to(dtype)
    vd = _rand((B, Hkv, cap, D), dtype, dev, seed, std=1.0)
    vd = torch.where(vd == 0, torch.ones_like(vd), vd)   # (an exact 0 would be gated at 1e-30, below the runner-up's e^-32 |v|)
    n = _n_values((H,), dev, seed + 1)
    assert (n == 0).any() and (n > 0).any()
    return dict(q=q.to(dtype), kd=kd, vd=vd, n=n, scale=32.0)


def inputs_c(case, std, dtype, dev, seed):
    """random q, k ~ N(0, 0.5^2), v ~ N(0, 1) in the operand type; scale so that the logits have the standard deviation `std`:
    q.k has 0.25 sqrt(D). With case.alibi, one slope per query head (synth.alibi_slopes)."""
    B, H, Hkv, D, cap = case.B, case.H, case.Hkv, case.D, case.cap
    inp = dict(q=_rand((B, H, case.Sq, D), dtype, dev, seed), kd=_rand((B, Hkv, cap, D), dtype, dev, seed + 1),
               vd=_rand((B, Hkv, cap, D), dtype, dev, seed + 2, std=1.0), n=_n_values((H,), dev, seed + 3), scale=std / (0.25 * math.sqrt(D)))
    if case.alibi:
        from flash_attention_softmax_n_amd import synth
        P = 1 << (H - 1).bit_length()
        inp["slopes"] = synth.alibi_slopes(P)[:H].float().to(dev)
    return inp


# ---------------------------------------------------------------- the gates: per row and per element, ratios to the bound
def _ratio(err, bound):
    """largest err / bound; a bound of 0 is met by an error of 0 only"""
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return r.max().item() if r.numel() else 0.0


def _f64(t):
    return t.detach().to("cpu", torch.float64)


def condition_a(refs, dtype):
    """the sizes keep the output's own rounding under 0.2: max c_ref * u <= 0.2 with the unit roundoff u = 2^-8 in bf16 and 2^-11 in fp16
    (one rounding is at most u of the value: twice as strict as c_ref * 2^-9 / 2^-12, which holds in the mean only), and m = 0 in every row"""
    cmax = max((r["acc"].max().item() if r["acc"].numel() else 0.0) for r in refs)
    assert all((r["m"] == 0).all() for r in refs), "witness A: a logit is not 0"
    assert cmax * U[dtype] <= 0.2, f"witness A: class count {cmax} x {U[dtype]} > 0.2: the output's own rounding would show"
    return cmax


def gate_a(out, lse, ref):
    """|exp(lse) - Z_ref| <= 1e-5 Z_ref and |out Z_ref - c_ref| <= 0.25, as (ratio of lse, ratio of out) to those bounds"""
    z = ref["l"]
    assert not torch.isnan(_f64(lse)).any() and torch.isfinite(_f64(out)).all(), "non-finite values"
    rz = _ratio((torch.exp(_f64(lse)) - z).abs(), 1e-5 * z)
    ro = _ratio((_f64(out) * z.unsqueeze(-1) - ref["acc"]).abs(), torch.full_like(ref["acc"], 0.25))
    return rz, ro


def expect_b(ref, v, G):
    """Witness B's expectation of one sequence from the clean reference and V [Hkv, S, D]: (kind [H, L], want [H, L, D]). kind 0: the row
    sees nothing - out is exactly 0; 1: a key decides - out is its V row; 2: the sink decides - |out| <= 1e-12. Asserts that whatever
    decides does so by at least 32 nats."""
    x, m, l = ref["x"], ref["m"], ref["l"]
    H, L, S = x.shape
    if S == 0:
        return torch.zeros(H, L, dtype=torch.long), torch.zeros(H, L, v.shape[2], dtype=torch.float64)
    top, w = x.max(-1)
    any_key = torch.isfinite(top)
    key_wins = any_key & (top == m)
    kind = torch.where(key_wins, 1, torch.where(any_key, 2, 0))
    second = torch.where(torch.arange(S).view(1, 1, S) == w.unsqueeze(-1), torch.full_like(x, -math.inf), x).amax(-1)
    assert (second[key_wins] <= top[key_wins] - 32).all(), "witness B: the runner-up is closer than 32 nats"
    assert (top[kind == 2] <= -32).all(), "witness B: the sink does not decide by 32 nats"
    sink_in_row = key_wins & (ref["l"] > 1 + 1e-12)   # (a sink beside a winning key weighs n e^-x_w)
    assert not sink_in_row.any(), "witness B: the sink weighs in beside the winning key"
    hkv = (torch.arange(H) // G).view(H, 1).expand(H, L)
    want = torch.where((kind == 1).unsqueeze(-1), v[hkv, w], torch.zeros(H, L, v.shape[2], dtype=torch.float64))
    assert ((ref["out"] - want).abs() <= 1e-12).all(), "witness B: the reference itself is not the winner's V row"
    return kind, want


def gate_b(out, kind, want, dtype):
    """|out - V[w]| <= 2 u |V[w]| + 1e-30 where a key decides, |out| <= 1e-12 where the sink does, exactly 0 where nothing is visible;
    the largest ratio to those bounds"""
    out = _f64(out)
    assert torch.isfinite(out).all(), "non-finite values"
    bound = torch.where((kind == 1).unsqueeze(-1), 2 * U[dtype] * want.abs() + 1e-30,
                        torch.where((kind == 2).unsqueeze(-1), torch.full_like(want, 1e-12), torch.zeros_like(want)))
    return _ratio((out - want).abs(), bound)


def gate_c(out, ref, dtype):
    """|out - ref| <= 3 u A + 1e-6 per element; the largest ratio"""
    out = _f64(out)
    assert torch.isfinite(out).all(), "non-finite values"
    return _ratio((out - ref["out"]).abs(), 3 * U[dtype] * ref["A"] + 1e-6)


# ---------------------------------------------------------------- the adapters: one table, every route
def _cache(case, inp, seed):
    """the paged cache before the call: NaN in every row at or beyond the old length and behind every unneeded table entry; under a
    window also in every row (and behind every table entry) wholly below the window's first tile"""
    pc = _Paged(inp["kd"], inp["vd"], case.lens, case.page, case.max_pages, seed, alloc_all=case.append)
    if case.window is not None:
        _poison(pc.k, pc.v, pc.table, case.page, pc.poison, case.total, case.qlens, case.window)
    return pc


def _new_rows(case, inp):
    """k_new / v_new [B, Hkv, Sq, D]: the rows old length .. len_b - 1 of the dense picture; padding rows are zeros"""
    if not case.append:
        return None, None
    kn, vn = (torch.zeros(case.B, case.Hkv, case.Sq, case.D, dtype=t.dtype, device=t.device) for t in (inp["kd"], inp["vd"]))
    for b, (ln, ql) in enumerate(zip(case.lens, case.qlens)):
        kn[b, :, :ql], vn[b, :, :ql] = inp["kd"][b, :, ln:ln + ql], inp["vd"][b, :, ln:ln + ql]
    return kn, vn


def _rows_of(case, out, lse, padding):
    """[B, H, Sq, D] / [B, H, Sq] -> per sequence ([H, qlen_b, D], [H, qlen_b]); padding positions must be exactly 0 / -inf"""
    res = []
    for b, ql in enumerate(case.qlens):
        if padding:
            assert (out[b, :, ql:] == 0).all() and (lse[b, :, ql:] == -math.inf).all(), f"padding rows of sequence {b}"
        res.append((out[b, :, :ql], lse[b, :, :ql]))
    return res


def _qs(case, dev):
    return torch.tensor(case.qlens, dtype=torch.int32, device=dev)


def run_decode(pkg, case, inp, seed):
    assert not case.ragged and case.window is None and (case.H // case.Hkv) * case.Sq <= 128
    pc = _cache(case, inp, seed)
    kn, vn = _new_rows(case, inp)
    out, lse = pkg.flash_attention_n_kvcache(inp["q"], pc.k, pc.v, pc.lens, block_table=pc.table, k_new=kn, v_new=vn, softmax_n_param=inp["n"],
                                             scale=inp["scale"], is_causal=case.causal, return_lse=True, alibi_slopes=inp.get("slopes"))
    return _rows_of(case, out, lse, False)


def run_prefill(pkg, case, inp, seed):
    assert case.window is None
    pc = _cache(case, inp, seed)
    kn, vn = _new_rows(case, inp)
    qs = _qs(case, pc.k.device) if case.ragged else None
    out, lse = pkg.flash_attention_n_kvcache_prefill(inp["q"], pc.k, pc.v, pc.lens, block_table=pc.table, k_new=kn, v_new=vn, query_seqlens=qs,
                                                     softmax_n_param=inp["n"], scale=inp["scale"], is_causal=case.causal, return_lse=True,
                                                     alibi_slopes=inp.get("slopes"))
    return _rows_of(case, out, lse, True)


def run_window(pkg, case, inp, seed):
    """route "window_decode": query_seqlens=None and G * Sq <= 128 - the decode kernels; "window_prefill": query_seqlens given"""
    assert case.window is not None and inp.get("slopes") is None
    decode = case.route == "window_decode"
    assert not (decode and (case.ragged or (case.H // case.Hkv) * case.Sq > 128))
    pc = _cache(case, inp, seed)
    kn, vn = _new_rows(case, inp)
    qs = None if decode else _qs(case, pc.k.device)
    out, lse = pkg.flash_attention_n_kvcache_window(inp["q"], pc.k, pc.v, pc.lens, case.window, block_table=pc.table, k_new=kn, v_new=vn,
                                                    query_seqlens=qs, softmax_n_param=inp["n"], scale=inp["scale"], return_lse=True)
    return _rows_of(case, out, lse, not decode)


def run_varlen(pkg, case, inp, seed):
    """the queries (and k_new / v_new) token-packed; the `tail` rows of the buffer behind cu[B] hold NaN"""
    assert case.window is None and inp.get("slopes") is None
    pc = _cache(case, inp, seed)
    dev = pc.k.device
    kn, vn = _new_rows(case, inp)
    used = sum(case.qlens)

    def pack(t):   # [B, heads, Sq, D] -> [T, heads, D]
        rows = [t[b, :, :ql].transpose(0, 1) for b, ql in enumerate(case.qlens)]
        return torch.cat(rows + [torch.full((case.tail, t.shape[1], t.shape[3]), NAN, dtype=t.dtype, device=dev)], 0).contiguous()

    cu = torch.tensor([0] + list(itertools.accumulate(case.qlens)), dtype=torch.int32, device=dev)
    out, lse = pkg.flash_attention_n_kvcache_varlen(pack(inp["q"]), pc.k, pc.v, pc.lens, cu, max(max(case.qlens), 1), block_table=pc.table,
                                                    k_new=None if kn is None else pack(kn), v_new=None if vn is None else pack(vn),
                                                    softmax_n_param=inp["n"], scale=inp["scale"], is_causal=case.causal, return_lse=True)
    assert out.shape == (used + case.tail, case.H, case.D) and lse.shape == (case.H, used + case.tail)
    res, t0 = [], 0
    for ql in case.qlens:
        res.append((out[t0:t0 + ql].transpose(0, 1), lse[:, t0:t0 + ql]))
        t0 += ql
    return res


ROUTES = {"decode": run_decode, "prefill": run_prefill, "window_decode": run_window, "window_prefill": run_window, "varlen": run_varlen}


def run(pkg, case, inp, seed=1):
    """per sequence (out [H, qlen_b, D], lse [H, qlen_b]) of the route's call on a freshly built paged cache"""
    return ROUTES[case.route](pkg, case, inp, seed)
