"""Three witnesses for flash_attention_n, forward and backward, whose expected values are exact or carry a derived bound, compared per row
and per element. The pattern is that of tests/kv_witness.py; this module brings it to the training path and adds the gradients (dQ, dK,
dV, dbias, dn), dropout, masks and bias, split-K and the routes of DESIGN 4.2.

Why. tests/test_gpu_parity.py draws q, k ~ N(0, 0.5^2) at scale = 1 / sqrt(D): the logits have a standard deviation near 0.25, every
softmax is close to a plain average, the running maximum never moves, split-K combine weights are all about 1 and the sink weighs about
1 / S. Its gate is one number per tensor. In a row that averages 1000 keys a causal limit one key off, a 64-key tile dropped at a seam, a
wrong keep bit or a pair partner's block served for its own moves the row by less than that gate.

  A  query = 0: every logit is 0 and every p is 1. V (and K) is an indicator pattern, so Z_i = exp(lse_i) is n plus the number of visible
     keys and out_id Z_i (1 - p_eff) counts the kept visible keys of class d. dO is an indicator of the row's class: dK is exactly 0 and,
     where Z is a power of two, dV_jd Z (1 - p_eff) counts the rows of class d that kept key j.
  B  one key decides. The ladder (forward only): q.k_j = g (j + 1) in exact integers, neighbouring keys 32 nats apart, the last or the first
     visible key or the sink takes the row. The bounded code (forward and backward): k_jd = +-1 by bit d of j over 12 bits, q_i = g k_t(i),
     scale g = 16: the target wins by 32 nats at |logit| <= 192, out_i = V[t(i)], dV[t(i)] = dO_i, and dQ, dK, dn are 0 up to the fp32
     summation error derived below.
  C  random operands at logit standard deviations of 4 and 8, every result gated per element by the first-order bound derived below.

The reference (visible_set / attend) is written from the docstring of flash_attention_n alone, on the CPU in fp64: key j is visible to row
i iff the mask allows it and, when causal, j <= i + S - L; the logits are scale q.k + bias; the sink is a column of logit 0, value 0 and
weight n[b, h]; query head h reads K/V head h // (H / Hkv); a row that sees nothing with n = 0 returns 0. The gradients are closed forms
(no autograd): with P_ij = w_ij exp(x_ij - lse_i), the dropout factor f_ij = keep_ij / (1 - p_eff) and a given dO,
    dV = (P f)^T dO,  dP = f (dO V^T),  delta_i = dO_i . O_i,  dS = P (dP - delta),  dQ = scale dS K,  dK = scale dS^T Q,
    dbias = dS summed over the dimensions the bias broadcasts over,  dn = - sum_i delta_i exp(-lse_i),
and every sum comes with its absolute-value companion, the same sum over |terms|. It shares no code with oracle/ref_attention.py,
_torch_reference_on_device or kv_witness.visible; _ratio, U and _f64 are imported from kv_witness.

Witness C's gates: the derivation. u is the unit roundoff of the operand type (2^-8 bf16, 2^-11 fp16). The rounding points are those
DESIGN 4.1 and 4.4 and the kernel sources name:
  (1) the prescale: Q (K in the dK / dV kernels) is multiplied by scale log2e once and rounded to the operand type. Each product q_id k_jd
      of a logit moves by at most u of itself: eps_ij = u |scale| sum_d |q_id k_jd| nats.
  (2) P is rounded to the operand type before the P.V and P^T.dO MFMAs; the fast path sums l from the rounded weights.
  (3) O is rounded to the output type (and that O is what delta reads).
  (4) lse is fp32, and the backward recomputes P = exp2(x' - lse log2e) from it.
  (5) dS is rounded to the operand type before the dS.K and dS^T.Q MFMAs.
  (6) one rounding of each result.
  (7) the two-wave kernels (D = 128 / 256, fasn_bwd_dkdv_ws.h ds_pass, fasn_bwd_dbias_ws.h) hand P through LDS in the operand type and form
      dS = rd(P) (dP - delta) from it: dS carries P's rounding as well as its own.
  (8) fp16 underflows gradually: below 2^-14 a rounding is off by up to ua = 2^-25 absolutely, not by u relatively (bf16: ua = 0). That
      matters where a weight far below the row's maximum meets a large factor: rd(P) |dP - delta| in (7), rd(P f) |dO| in dV, rd(P) |v|.
  (9) the seed (DESIGN 4.1 "Seeded accumulators"; gated by tests/bias_witness.py, not by witness C's own cases, whose biases are N(0, 1)
      and whose row maxima stay near 0): the score accumulates in fp32 onto a start value of magnitude at most max(|m_i| log2e, F), and
      bias * log2e is formed in fp32. The vector bias modes of fasn_fwd_kernel start a tile's accumulator from fma(bias, log2e, -m_run)
      and add q'.k onto it in D / 16 MFMAs; each of these `steps` = D / 16 + 2 roundings (the fma, the MFMAs, the subtraction of the
      moved maximum) is off by at most 2^-24 of the running value, which is below |x_ij| log2e + max(|m_i| log2e, F) with m_i the row's
      true maximum. In nats: eps_ij += steps 2^-24 (|x_ij| log2e + max(|m_i| log2e, F)) ln 2. F is the seed floor, a design constant of
      the kernels (kSeedFloor in csrc/fasn_fwd_kernel.h, F_SEED in bias_witness.py): a row whose running maximum lies at or below -F
      counts as unseeded (start value bias log2e alone, exact path), so no start value exceeds max(|m_i| log2e, F). The F part is capped:
      (128 / 16 + 2) 2^-24 F ln 2 <= 2^-12 nats at D = 128, so F <= 590; F = 512. Without the floor a row that had seen only keys at
      -1e9 was seeded from +1.44e9, where fp32 is spaced 128 apart, and the next tile's q.k was rounded away.
To first order a logit perturbation eps moves out_id by sum_j Pf_ij eps_ij |v_jd - o_id|, bounded here by E1 + |o_id| E0 with
E1 = sum_j Pf_ij eps_ij |v_jd|, E0 = sum_j Pf_ij eps_ij (the same sums without the [L, S, D] tensor), and lse_i by lam0_i = sum_j P_ij eps_ij.
    out    3 u A + E1 + |o| E0 + ua sum_j w_ij |v_jd| / l_i + 1e-6      A = sum_j Pf_ij |v_jd|: (2) weights, (2) l, (3), (8); l_i relative to the row's maximum
    lse    lam = lam0 + u + 2^-22 (1 + |lse|)                (1), (2) l from rounded weights, (4)
    dV     2 u sum_i Pf_ij |dO_id| + sum_i Pf_ij (eps_ij + lam_i) |dO_id| + ua sum_i w_ij |dO_id| + 1e-6     (2), (6), (8); the recomputed P is off by eps + lam relatively
    delta  eta_i = sum_d |dO_id| gate(out)_id + 2^-20 sum_d |dO_id O_id|              (3) and the forward's own error, fp32 sum
    dS     bdS_ij = |dS_ij| (u [2 u where (7) applies: a *_ws_ / *_ws256_ kernel in the case's plan] + eps_ij + lam_i) + P_ij eta_i + 2^-20 P_ij sum_d f_ij |dO_id v_jd| + ua w_ij (1 + |dP_ij - delta_i|)      (5), (7), (1), (4), delta, fp32 dP, (8)
    dQ     |scale| sum_j bdS_ij |k_jd| + u |dQ_id| + 1e-6     (6)
    dK     |scale| sum_i bdS_ij |q_id| + u |dK_jd| + 1e-6     (6), summed over the query heads of the K/V head
    dbias  sum of bdS over the broadcast dimensions + u |dbias| + 1e-6
    dn     sum_i (eta_i + |delta_i| lam_i) exp(-lse_i) + 2^-20 sum_i |delta_i| exp(-lse_i) + 1e-6
No constant comes from a GPU run. tests/attn_emulate.py emulates exactly these roundings on the CPU - (1) to (8) with absolute fp32
scores, and with (9) the seeded start value and the step-wise fp32 accumulation - and tests/test_attnwitness_cpu.py and
tests/test_biaswitness_cpu.py assert that every result stays at or below 0.5 of its gate.

Witness B's bound on dQ, dK, dn (bounded code). The winner t has P_it = 1 in fp32, so O_i = f_it V_t: exact without dropout, one rounding
(u) with it. dS_it = P_it (dP_it - delta_i) is the difference of two fp32 evaluations of the same sum dO_i . O_i over D terms, in different
orders: each is off by at most (D + 2) 2^-24 sum_d |dO_id O_id|, so |dS_it| <= gamma sum_d |dO_id O_id| with gamma = 2 (D + 2) 2^-24
(+ u under dropout, from the rounded O). Every other key has P_ij <= e^-30: with |dP - delta| <= 2 sum |dO| max|v| / (1 - p) and S keys that
is below 1e-6 for the sizes used. So |dQ_id| <= |scale| gamma sum|dO_i O_i| |k_td| (1 + 2u) + 1e-6, |dK_td| likewise with |q_id| summed over
the rows t wins, and every dn term carries exp(-lse) <= e^-160 where a key wins and delta ~ 0 where the sink does.

Big grids. With q = 0 (A) and with operands that repeat over batch and heads (B, C) the expectation depends on (b, h) only through a few
distinct problems: a Case draws `ub` x `uh` distinct (batch, head) problems and tiles them over [B, H], n included, so that the fp64
reference is computed once per distinct problem while EVERY (batch, head, row) of the kernels' result is gated. What this cannot see: a
block served with the data of batch b + ub or head h + uh (a multiple of the period) is bit-identical to the right answer. The period is
1 x 2 at the forward-only large grids; the cases with ub = B and uh = H (the small grids, dropout) witness every such mix-up.

Witness C in fp32. The fp32 kernels (fasn_f32_kernels.h) keep P and dS in fp32 and round nothing to a 16-bit type: rounding points (2), (3),
(5), (6), (7) and (8) shrink to fp32's own 2^-24 and what is left is the error of their sums, at most S + D terms each. The gates are the
formulas above, unchanged, at u = unit(case, fp32) = (S + D) 2^-24 and ua = 0. tests/test_attnwitness_cpu.py shows on every fp32 case that
an independent evaluation in torch fp32 - the online softmax and every sum over keys in tile order - stays at or below 0.5 of every gate
(out, lse, dQ, dK, dV, dbias, dn: it is below 0.03), so no result's gate is left out in fp32.

The instantiations (NEW). SHAPES' first part reaches every kernel template once; its second part, NEW, the modes of each template that
the first leaves to tests/test_gpu_parity.py: the 8-wave forward kernels of large grids (D = 128 plain / causal, D = 64 bias / mask /
bias + mask / bias + key padding), key padding at D = 32, 128, 256 and under causal at D = 64, dropout away from D = 64 and the backward
of the 64-rows-per-wave dropout kernel, grouped K/V at D = 32 and 128, split-K under key padding, and the fp32 kernels at D = 64 and 128,
in their mask / bias / dropout mode and with grouped K/V. Three shapes differ from the obvious ones because the dispatch does:
  * at D = 128 the two-wave backward kernels have dropout instantiations and take every dropout call with one query head per K/V head;
    the one-wave fasn_bwd_dq_kernel / fasn_bwd_dkdv_kernel run under dropout with grouped K/V only (launch_bwd_one, fasn_bwd_launch.h).
    "d128 drop" and "d128 drop causal keypad" are therefore grouped (H = 8, Hkv = 2), and "... two-wave" are their ungrouped twins;
  * a key-padding row of S = 4090 bytes is no run of aligned 4-byte vectors, takes the element loads and is never split: the split-K
    key-padding cases have S = 4092. Their forward is the general (bias+mask) SPLIT=1 instantiation - split-K has no key-padding one;
  * "d64 drop 64 rows bwd" needs ceil(L / 256) B H >= 512 under ub = B, uh = H: 512 distinct problems, witness A only.

This is a helper module (no test is collected from it). tests/test_attnwitness_cpu.py is the test of these tests;
tests/test_gpu_attnwitness.py runs the kernels."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kv_witness import U as _U16, _f64, _ratio   # noqa: E402

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
DT_ENUM = {"fp16": 0, "bf16": 1, "fp32": 2}
U = dict(_U16)
U[torch.float32] = 2.0 ** -24
KT = 64        # keys per tile in every attention kernel
DUMMY = 1 << 20
LOG2E = math.log2(math.e)


def unit_abs(dtype):
    """fp16's gradual underflow: half the spacing of its subnormals (rounding point 8)"""
    return 2.0 ** -25 if dtype == torch.float16 else 0.0


def unit(case, dtype):
    """the unit roundoff the gates are built on: that of the 16-bit operand type; fp32 kernels sum up to S + D terms in fp32, each sum
    off by at most (S + D) 2^-24 of the sum of its |terms|"""
    return U[dtype] if dtype != torch.float32 else (case.S + case.D) * 2.0 ** -24


class Case:
    """One call shape. mask: None, "keypad" ([B,1,1,S] from `lens`), "dense" ([B,H,L,S]) or "misaligned" (a dense mask whose rows start at
    odd addresses: element loads). bias: None, "hls" ([H,L,S], its gradient reduced over the batch in the kernel) or "bhls" (dense gradient).
    nshape: "H", "BH", "B1" or "float" (the grouped-query decode regroup). ub x uh distinct (batch, head) problems are tiled over [B, H].
    want: properties of the launch plans this case is named for (tests/test_attnwitness_cpu.py asserts them)."""

    def __init__(self, B, H, L, S, D, Hkv=None, causal=False, mask=None, bias=None, p=0.0, lens=None, nshape="H", ub=None, uh=None,
                 dtypes=("fp16", "bf16"), bwd=True, want=(), wit="ABC", a_dtypes=None, hide_from=None, n_pos=None):
        self.B, self.H, self.L, self.S, self.D, self.Hkv = B, H, L, S, D, Hkv or H
        self.G = H // self.Hkv
        self.causal, self.mask, self.bias, self.p, self.nshape = causal, mask, bias, p, nshape
        self.lens = list(lens) if lens is not None else None
        self.ub = ub or B
        self.uh = uh or H
        self.dtypes, self.bwd, self.want, self.wit = tuple(dtypes), bwd, tuple(want), wit
        self.hide_from = hide_from   # a dense mask hides every key from this one on
        self.n_pos = n_pos           # the n > 0 of a caller that hands its own n to inputs_* (tests/attn_varlen_witness.py: one n for a whole pack); pow2_n answers from it
        self.a_dtypes = tuple(a_dtypes) if a_dtypes is not None else self.dtypes
        assert H % self.Hkv == 0 and self.uh % self.G == 0 and H % self.uh == 0 and B % self.ub == 0
        assert (mask == "keypad") == (lens is not None) and (lens is None or len(lens) == self.ub)
        assert p == 0.0 or (self.ub == B and self.uh == H), "dropout bits differ in every (batch, head)"

    @property
    def p_rounded(self):
        """rounding point 7: the case's backward runs two-wave kernels, which form dS from a P already rounded to the operand type. Keyed on
        the kernel names the case asserts of its plan. (d256 bias: dQ comes from fasn_bwd_dq_ws256_kernel, dK from the one-wave kernel, whose
        P stays fp32; the bound on dS is one per case, so its dK gate carries the u |dS| as well.)"""
        return any("_ws" in w for w in self.want)   # (fasn_bwd_*_ws_kernel, *_ws256_kernel, fasn_bwd_dbias_ws_kernel: the plan test asserts the names)

    def but(self, **kw):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(kw)
        return c

    @property
    def bidx(self):
        return torch.arange(self.B) % self.ub

    @property
    def hidx(self):
        return torch.arange(self.H) % self.uh

    @property
    def uhk(self):
        return self.uh // self.G


# ---------------------------------------------------------------- the reference: fp64, from the docstring of flash_attention_n
def visible_set(L, S, causal, mask=None):
    """[..., L, S] fp64 of 0 / 1: key j is visible to row i iff the mask (bool, broadcastable to [..., L, S]) allows it and, when causal,
    j <= i + S - L (bottom-right aligned)"""
    w = torch.ones(L, S, dtype=torch.float64)
    if causal:
        w = torch.tril(w, diagonal=S - L)
    if mask is not None:
        w = w * mask.to(torch.float64)
    return w


def attend(q, k, v, w, n, scale, bias=None, keep=None, p_eff=0.0, do=None, row_w=None, delta_mode=None):
    """softmax_n attention of N independent (batch, head) problems in fp64, with closed-form gradients. q [N, L, D]; k, v [N, S, D] (the
    K/V head of each problem); w [N or 1, L, S]: how often row i counts key j (0 hidden, 1 visible; the test of the tests passes 2 too);
    n [N]; bias [N or 1, L, S] or None; keep [N, L, S] of 0 / 1 or None with p_eff = dropout.effective_p; do [N, L, D] or None.
    Forward: x (logits, -inf where hidden), m (largest visible logit; at least 0 where n > 0; 0 where nothing is visible),
    l = n e^-m + sum_j w e^(x - m), acc = sum_j w f e^(x - m) v_j, acc_abs (over |v|), out, A = acc_abs / l, lse, P, f.
    Backward (given do): dV, dP, delta, dS, dQ, dK (per problem: the caller sums a K/V head's group), dn, and *_abs companions.
    For the test of the tests: row_w [N, L] counts row i that often in the sums over rows (dV, dK); delta_mode "zero" / "undropped" replaces
    delta by 0 / by dO . (the output without dropout)."""
    N, L, D = q.shape
    S = k.shape[1]
    n = n.reshape(N, 1)
    x = scale * (q @ k.transpose(1, 2))
    if bias is not None:
        x = x + bias
    x = torch.where(w > 0, x, torch.full_like(x, -math.inf))
    m = x.amax(-1) if S else torch.full((N, L), -math.inf, dtype=torch.float64)
    m = torch.where(n > 0, m.clamp_min(0.0), m)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = w * torch.exp(x - m.unsqueeze(-1))
    l = torch.where(n > 0, n * torch.exp(-m), torch.zeros_like(m)) + e.sum(-1)
    f = torch.ones_like(e) if keep is None else keep / (1.0 - p_eff)
    # the dropout factor is applied AFTER the sums over keys and rows: in witness A e keep, P keep (Z a power of two), v and dO are small
    # integers or dyadic fractions, so these sums are exact in whatever order the host's BLAS takes them, and the one division that follows
    # rounds the same everywhere. Summing e f v instead left host-dependent ulps in acc and dV - enough to turn "one count is exactly four
    # gates" into 3.999999999999998 on one machine and 4 on another.
    ek, live = (e, 1.0) if keep is None else (e * keep, 1.0 - p_eff)
    acc, acc_abs = (ek @ v) / live, (ek @ v.abs()) / live
    has = l > 0
    safe = torch.where(has, l, torch.ones_like(l))
    out, A = acc / safe.unsqueeze(-1), acc_abs / safe.unsqueeze(-1)
    lse = torch.where(has, m + torch.log(safe), torch.full_like(m, -math.inf))
    P = e / safe.unsqueeze(-1)
    r = dict(x=x, m=m, l=l, acc=acc, acc_abs=acc_abs, out=out, A=A, lse=lse, P=P, f=f)
    if do is None:
        return r
    Pf = P * f
    rows = torch.ones(N, L, 1, dtype=torch.float64) if row_w is None else row_w.unsqueeze(-1)
    Pk = P if keep is None else P * keep
    r["dV"], r["dV_abs"] = (Pk.transpose(1, 2) @ (rows * do)) / live, (Pk.transpose(1, 2) @ (rows * do.abs())) / live
    dP, dP_abs = f * (do @ v.transpose(1, 2)), f * (do.abs() @ v.abs().transpose(1, 2))
    delta, delta_abs = (do * out).sum(-1), (do * out).abs().sum(-1)
    if delta_mode == "zero":
        delta = torch.zeros_like(delta)
    elif delta_mode == "undropped":
        delta = (do * ((e @ v) / safe.unsqueeze(-1))).sum(-1)
    dS = P * (dP - delta.unsqueeze(-1))
    r.update(dP=dP, dP_abs=dP_abs, delta=delta, delta_abs=delta_abs, dS=dS, dS_abs=P * (dP_abs + delta_abs.unsqueeze(-1)))
    r["dQ"], r["dQ_abs"] = scale * (dS @ k), abs(scale) * (dS.abs() @ k.abs())
    r["dK"], r["dK_abs"] = scale * (dS.transpose(1, 2) @ (rows * q)), abs(scale) * (dS.abs().transpose(1, 2) @ (rows * q.abs()))
    einv = torch.where(has, torch.exp(-lse), torch.zeros_like(lse))
    einv = torch.where((do == 0).all(-1), torch.zeros_like(einv), einv)   # a row without dO adds 0 to dn, also where exp(-lse) overflows (bias_witness: pad rows at lse = -V)
    r["einv"] = einv
    r["dn"], r["dn_abs"] = -(delta * einv).sum(-1), (delta.abs() * einv).sum(-1)
    return r


def seed_eps(r, steps, F):
    """rounding point (9) in nats, [N, L, S]: steps 2^-24 (|x_ij| log2e + max(|m_i| log2e, F)) ln 2 with x, m of the attend() result r;
    0 where the key is hidden outright (x = -inf: its weight is exactly 0 whatever the score's rounding)"""
    x, m = r["x"], r["m"]
    fin = torch.isfinite(x)
    xa = torch.where(fin, x.abs(), torch.zeros_like(x))
    e = steps * 2.0 ** -24 * (xa * LOG2E + (m.abs() * LOG2E).clamp_min(F).unsqueeze(-1)) * math.log(2.0)
    return torch.where(fin, e, torch.zeros_like(e))


def bounds_c(r, q, k, v, do, scale, u, ua=0.0, p_rounded=False, eps_add=None):
    """Witness C's per-element gates of one attend() result (module docstring): a dict with out, lse and, when the result carries
    gradients, dV, dQ, dK, dS (the bound on dS, from which a bias gradient's gate is summed) and dn. eps_add [L, S]: further terms of
    eps_ij (seed_eps: rounding point 9)"""
    eps = u * abs(scale) * (q.abs() @ k.abs().transpose(1, 2))
    if eps_add is not None:
        eps = eps + eps_add
    P, f = r["P"], r["f"]
    Pf = P * f
    Pe = Pf * eps
    vis = torch.isfinite(r["x"]).double()
    wv = (vis @ v.abs()) / torch.where(r["l"] > 0, r["l"], torch.ones_like(r["l"])).unsqueeze(-1)
    g_out = 3 * u * r["A"] + Pe @ v.abs() + r["out"].abs() * Pe.sum(-1, keepdim=True) + ua * wv + 1e-6
    fin = torch.where(torch.isfinite(r["lse"]), r["lse"], torch.zeros_like(r["lse"]))
    lam = (P * eps).sum(-1) + u + 2.0 ** -22 * (1 + fin.abs())
    g = dict(out=g_out, lse=lam)
    if do is None or "dV" not in r:
        return g
    rel = eps + lam.unsqueeze(-1)
    g["dV"] = 2 * u * r["dV_abs"] + (Pf * rel).transpose(1, 2) @ do.abs() + ua * (vis.transpose(1, 2) @ do.abs()) + 1e-6
    eta = (do.abs() * g_out).sum(-1) + 2.0 ** -20 * r["delta_abs"]
    bdS = (r["dS"].abs() * ((2 if p_rounded else 1) * u + rel) + P * eta.unsqueeze(-1) + 2.0 ** -20 * P * r["dP_abs"]
           + ua * vis * (1 + (r["dP"] - r["delta"].unsqueeze(-1)).abs()))
    g["dS"] = bdS
    g["dQ"] = abs(scale) * (bdS @ k.abs()) + u * r["dQ"].abs() + 1e-6
    g["dK"] = abs(scale) * (bdS.transpose(1, 2) @ q.abs())   # (+ u |dK| + 1e-6 after the sum over the group)
    g["dn"] = ((eta + r["delta"].abs() * lam) * r["einv"]).sum(-1) + 2.0 ** -20 * r["dn_abs"]   # (+ 1e-6 after the sum over what n broadcasts over)
    return g


# ---------------------------------------------------------------- operands
def _counter_normal(shape, seed, std, dtype, dev):
    from flash_attention_softmax_n_amd import synth
    return synth.counter_normal(shape, seed, std=std, dtype=dtype, device=dev)


def _tile(case, t, heads="q"):
    """[ub, uh or uhk, ...] -> [B, H or Hkv, ...]"""
    hid = case.hidx if heads == "q" else torch.arange(case.Hkv) % case.uhk
    return t[case.bidx.to(t.device)][:, hid.to(t.device)].contiguous()


def n_values(case, dev, pos=None, given=None):
    """(n as the call gets it, un [ub, uh] fp64 on the CPU). Zeros next to positive entries; `pos` replaces the positive value.
    given: an [H] tensor handed in instead of drawn (a case with ub = 1, uh = H: the packed call's one n per head)"""
    ub, uh = case.ub, case.uh
    if given is not None:
        assert case.nshape == "H" and ub == 1 and uh == case.H and tuple(given.shape) == (case.H,)
        return given.float().to(dev), given.detach().double().cpu().view(1, uh)
    if case.nshape == "float":
        val = 1.5 if pos is None else pos
        return val, torch.full((ub, uh), val, dtype=torch.float64)
    b, h = torch.arange(ub).view(-1, 1), torch.arange(uh).view(1, -1) // case.G   # (one sign per K/V head's group: see judge_b)
    if case.nshape == "H":
        assert case.uhk >= 2
        un = torch.where(h % 2 == 0, 0.0, 0.5 + 0.75 * h.double()).expand(ub, uh)
    elif case.nshape == "B1":
        assert ub >= 2
        un = torch.where(b % 2 == 0, 0.0, 0.5 + 0.75 * b.double()).expand(ub, uh)
    else:
        un = torch.where((b + h) % 2 == 0, 0.0, 0.5 + 0.75 * (h + 2 * b).double())
    un = un.clone()
    if pos is not None:
        un = torch.where(un > 0, torch.full_like(un, float(pos)), un)
    assert (un == 0).any() and (un > 0).any()
    full = un[case.bidx][:, case.hidx].float()
    nt = {"H": full[0], "B1": full[:, :1], "BH": full}[case.nshape].contiguous().to(dev)
    return nt, un


def masks(case, dev, seed):
    """(mask as the call gets it or None, um: bool [ub, uh or 1, L or 1, S] on the CPU or None). keypad: lens per batch element; dense: random
    with 1/4 hidden, at least one visible key per row kept out of it so that every row has a last visible key below"""
    L, S = case.L, case.S
    if case.mask is None:
        return None, None
    if case.mask == "keypad":
        um = (torch.arange(S).view(1, -1) < torch.tensor(case.lens).view(-1, 1)).view(case.ub, 1, 1, S)
        return um[case.bidx].contiguous().to(dev), um
    g = torch.Generator().manual_seed(seed)
    um = torch.rand(case.ub, case.uh, L, S, generator=g) >= 0.25
    if case.hide_from is not None:
        um[..., case.hide_from:] = False
    full = um[case.bidx][:, case.hidx].contiguous()
    if case.mask == "misaligned":   # rows of S + 1 bytes starting at an odd address
        buf = torch.zeros(case.B * case.H * L * (S + 1) + 1, dtype=torch.bool, device=dev)
        view = buf[1:].view(case.B, case.H, L, S + 1)[..., :S]
        view.copy_(full.to(dev))
        return view, um
    return full.to(dev), um


def weights(case, um):
    """w [ub, uh or 1, L, S] fp64 of the clean reference"""
    w = visible_set(case.L, case.S, case.causal, um)
    return w.expand(case.ub, -1, -1, -1) if w.dim() == 4 else w.view(1, 1, case.L, case.S).expand(case.ub, 1, -1, -1)


def _bias(case, kind, dtype, dev, seed):
    """(bias as the call gets it or None, ubias [ub or 1, uh, L, S] fp64 or None). kind "zero" (A) or "random" (B: N(0, 0.25^2), C: N(0, 1))"""
    if case.bias is None:
        return None, None
    ub = 1 if case.bias == "hls" else case.ub
    if kind == "zero":
        t = torch.zeros(ub, case.uh, case.L, case.S, dtype=dtype, device=dev)
    else:
        t = _counter_normal((ub, case.uh, case.L, case.S), seed, 0.25 if kind == "small" else 1.0, dtype, dev)
    full = t[:, case.hidx.to(dev)]
    full = full[0].contiguous() if case.bias == "hls" else full[case.bidx.to(dev)].contiguous()
    return full, _f64(t)


GRANULE = {torch.float16: KT, torch.bfloat16: KT // 2, torch.float32: KT}


def _indicator(rows, D, gran, dev):
    j = torch.arange(rows, device=dev)
    t = torch.zeros(rows, D, dtype=torch.float32, device=dev)
    if rows:
        t[j, j % (D // 2)] = 1.0
        t[j, D // 2 + (j // gran) % (D // 2 - 1)] = 1.0
    return t


def pow2_n(case):
    """the n > 0 that makes Z = n + S a power of two (non-causal, no mask: every row sees S keys), or None"""
    if case.causal or case.mask is not None or case.nshape == "float":
        return None
    if case.n_pos is not None:   # a handed-in n: Z is a power of two only at the key lengths it was chosen for
        z = case.n_pos + case.S
        return float(case.n_pos) if z == 2.0 ** round(math.log2(z)) else None
    z = 1 << case.S.bit_length()
    return float(z - case.S)


def inputs_a(case, dtype, dev, seed, n=None):
    """query = 0. V[j, d] = 1 for d = j mod (D/2) and for d = D/2 + (j // granule) mod (D/2 - 1): the key's place within its half tile and
    its tile (bf16: half tile, as kv_witness.inputs_a). The last feature is the spare class: (hkv + 1) 2^-k for every key of K/V head hkv.
    K is the same indicator (the logits stay 0). dO[i] is the indicator of row i's class, the same in every head. A zero bias where the
    case has one. Every value is exact in fp16 and bf16."""
    B, H, Hkv, L, S, D = case.B, case.H, case.Hkv, case.L, case.S, case.D
    q = torch.zeros(B, H, L, D, dtype=dtype, device=dev)
    ind = _indicator(S, D, GRANULE[dtype], dev)
    k = ind.view(1, 1, S, D).repeat(B, Hkv, 1, 1)
    v = k.clone()
    shift = 0   # (the spare class repeats with the distinct problems, like every operand; under dropout the kept keys weigh 1 / (1 - p))
    while case.uhk * 2.0 ** -shift * max(S, 1) * unit(case, dtype) / (1.0 - case.p) > 0.2:
        shift += 1
    v[:, :, :, D - 1] = ((torch.arange(Hkv, device=dev) % case.uhk + 1).float() * 2.0 ** -shift).view(1, Hkv, 1)
    do = _indicator(L, D, KT // 2, dev).view(1, 1, L, D).repeat(B, H, 1, 1)
    n, un = n_values(case, dev, pos=pow2_n(case), given=n)
    mask, um = masks(case, dev, seed)
    bias, ubias = _bias(case, "zero", dtype, dev, seed)
    return dict(q=q, k=k.to(dtype), v=v.to(dtype), do=do.to(dtype), n=n, un=un, mask=mask, um=um, bias=bias, ubias=ubias, scale=1.0 / math.sqrt(D))


B_FORMS = ("ascending", "descending", "sink", "code", "code_sink")


def ladder_params(dtype, S):
    """(g, digits, scale): bf16 / fp32 the ladder of kv_witness.inputs_b (scale 32); fp16 within |scale log2e| <= 8 and a prescaled operand
    below 65504: three base-16 digits, g = 8, scale = 4 (S <= 4096)"""
    if dtype == torch.float16:
        assert S <= 4096
        return 8.0, 3, 4.0
    assert S <= 65536
    return 1.0, 4, 32.0


def inputs_b(case, form, dtype, dev, seed, n=None):
    """ascending / descending / sink: q_d = g 16^d for d < digits, k_jd = base-16 digit d of j (descending: 15 - digit), feature `digits`
    is g and 1; the MFMA sum is the integer g (j + 1), every operand exact, neighbouring logits scale g = 32 nats apart. sink: q negated.
    code / code_sink: k_jd = +-1 by bit d of j for 12 bits, q_i = g k_t(i) with t(i) the last visible key of row i (without causal: the last
    visible key at or below S - 1 - i mod S, so that t stays injective where the mask allows), scale g = 16,
    scale = 4. code_sink: q negated and shifted by 14 g through a constant feature, so that every logit is at most -32. V, dO ~ N(0, 1) with every |value| below 2^-12 replaced by 1 (fp16 rounds
    relatively down to 2^-14 only, the factor f is at most 4 / 3 and an operand may lose a bit to its own rounding: two binades of room); a bias ~ N(0, 0.25^2) where the case has one."""
    B, H, Hkv, L, S, D = case.B, case.H, case.Hkv, case.L, case.S, case.D
    assert form in B_FORMS
    mask, um = masks(case, dev, seed)
    j = torch.arange(S, device=dev)
    if form.startswith("code"):
        assert S <= 4096 and D >= 12
        scale, g = 4.0, 4.0
        k1 = torch.zeros(S, D, dtype=torch.float32, device=dev)
        for d in range(12):
            k1[:, d] = 1.0 - 2.0 * ((j >> d) & 1).float()
        w = weights(case, um)                                              # [ub, uh or 1, L, S]
        jj = torch.arange(S, dtype=torch.float64)
        if not case.causal:   # keep t injective where the visible set allows it: row i aims at key S - 1 - i mod S
            w = w * (jj.view(1, 1, 1, S) <= (S - 1 - torch.arange(L) % S).view(1, 1, L, 1))
        t = (torch.where(w > 0, jj + 1, torch.zeros_like(w)).amax(-1) - 1).long()   # last visible key at or below the aim, -1: none
        t = t.expand(case.ub, case.uh, L)
        uq = g * k1.cpu()[t.clamp_min(0)] * (t >= 0).unsqueeze(-1)
        if form == "code_sink":   # feature 12 shifts every logit to 16 (12 - 2 hamming) - 224 <= -32: the sink (logit 0) wins where n > 0
            assert D >= 13
            k1[:, 12] = 1.0
            uq = -uq
            uq[..., 12] = -14.0 * g
        q = _tile(case, uq).to(dev)
    else:
        g, nd, scale = ladder_params(dtype, S)
        q1 = torch.zeros(D, dtype=torch.float32, device=dev)
        k1 = torch.zeros(S, D, dtype=torch.float32, device=dev)
        for d in range(nd):
            q1[d] = g * 16.0 ** d
            digit = (j // 16 ** d) % 16
            k1[:, d] = (15 - digit if form == "descending" else digit).float()
        q1[nd], k1[:, nd] = g, 1.0
        q = (-q1 if form == "sink" else q1).view(1, 1, 1, D).repeat(B, H, L, 1)
    k = k1.view(1, 1, S, D).repeat(B, Hkv, 1, 1).to(dtype)
    uv = _counter_normal((case.ub, case.uhk, S, D), seed + 1, 1.0, dtype, dev)
    uv = torch.where(uv.abs() < 2.0 ** -12, torch.ones_like(uv), uv)   # (no zeros, and f V, f dO stay clear of fp16's gradual underflow, where 2 u |x| does not hold)
    udo = _counter_normal((case.ub, case.uh, L, D), seed + 2, 1.0, dtype, dev)
    udo = torch.where(udo.abs() < 2.0 ** -12, torch.ones_like(udo), udo)
    n, un = n_values(case, dev, given=n)
    bias, ubias = _bias(case, "small", dtype, dev, seed + 3)
    return dict(q=q.to(dtype), k=k, v=_tile(case, uv, "kv"), do=_tile(case, udo), n=n, un=un, mask=mask, um=um, bias=bias, ubias=ubias, scale=scale)


def inputs_c(case, std, dtype, dev, seed, n=None):
    """q, k ~ N(0, 0.5^2), v, dO ~ N(0, 1) in the operand type; scale so that the logits have the standard deviation `std` (q.k has
    0.25 sqrt(D)); a bias ~ N(0, 1) where the case has one"""
    L, S, D = case.L, case.S, case.D
    uq = _counter_normal((case.ub, case.uh, L, D), seed, 0.5, dtype, dev)
    uk = _counter_normal((case.ub, case.uhk, S, D), seed + 1, 0.5, dtype, dev)
    uv = _counter_normal((case.ub, case.uhk, S, D), seed + 2, 1.0, dtype, dev)
    udo = _counter_normal((case.ub, case.uh, L, D), seed + 3, 1.0, dtype, dev)
    n, un = n_values(case, dev, given=n)
    mask, um = masks(case, dev, seed)
    bias, ubias = _bias(case, "random", dtype, dev, seed + 4)
    return dict(q=_tile(case, uq), k=_tile(case, uk, "kv"), v=_tile(case, uv, "kv"), do=_tile(case, udo), n=n, un=un, mask=mask, um=um,
                bias=bias, ubias=ubias, scale=std / (0.25 * math.sqrt(D)))


# ---------------------------------------------------------------- the reference of a case: per distinct problem
def unique_operands(case, inp):
    """the ub x uh distinct problems of `inp`, widened exactly to fp64 on the CPU: q, do [ub, uh, L, D]; k, v [ub, uh, S, D] (each query
    head with its K/V head); n [ub, uh]; bias [ub or 1, uh, L, S] or None"""
    ub, uh, G = case.ub, case.uh, case.G
    q, do = _f64(inp["q"][:ub, :uh]), _f64(inp["do"][:ub, :uh])
    kv = torch.arange(uh) // G
    k, v = _f64(inp["k"][:ub, :case.uhk])[:, kv], _f64(inp["v"][:ub, :case.uhk])[:, kv]
    return q, k, v, do, inp["un"], inp["ubias"]


def keep_of(case, state):
    """keep [B, H, L, S] fp64 and p_eff from the host mirror of the kernels' dropout bits, or (None, 0)"""
    if not case.p:
        return None, 0.0
    from flash_attention_softmax_n_amd import dropout
    keep = dropout.keep_mask(state[0], state[1], case.B, case.H, case.L, case.S, case.p)
    return torch.from_numpy(keep.astype(np.float64)), dropout.effective_p(case.p)


def reference(case, inp, w=None, keep=None, p_eff=0.0, backward=True, swap_kv=False, un=None, ubias=None, only=None, **alt):
    """attend() of every distinct problem of the case: a dict of [ub, uh, ...] tensors, dK / dV summed over each K/V head's group
    ([ub, uhk, S, D]) and with_bounds() ready. w [ub, uh or 1, L, S] replaces the visible set (the test of the tests)."""
    ub, uh, L, S, D, G = case.ub, case.uh, case.L, case.S, case.D, case.G
    q, k, v, do, un0, ubias0 = unique_operands(case, inp)
    un, ubias = (un0 if un is None else un), (ubias0 if ubias is None else ubias)
    if swap_kv:
        k, v = k.roll(G, 1), v.roll(G, 1)
    if w is None:
        w = weights(case, inp["um"])
    res = []
    for b in range(ub):
        bias = None if ubias is None else ubias[b if ubias.shape[0] > 1 else 0]
        kp = None if keep is None else keep[b]
        one = attend(q[b], k[b], v[b], w[b], un[b], inp["scale"], bias, kp, p_eff, do[b] if backward else None,
                     **{key: (val[b] if torch.is_tensor(val) else val) for key, val in alt.items()})
        res.append(one if only is None else {key: one[key] for key in only})   # (big grids: keep what the gates read)
    r = {key: torch.stack([x[key] for x in res]) for key in res[0]}
    r["_bias"] = ubias
    r["_ops"] = (q, k, v, do if backward else None)
    r["_un"] = un
    return r


def group_sum(case, t):
    """[ub, uh, S, D] -> [ub, uhk, S, D]: the sum over the query heads of each K/V head"""
    return t.view(case.ub, case.uhk, case.G, *t.shape[2:]).sum(2)


def with_bounds(case, inp, r, u, ua=0.0, seed=None):
    """bounds_c of every distinct problem: dict of [ub, uh, ...]; dK already summed over the group with its result rounding.
    seed = (steps, F): add rounding point (9) to eps (tests/bias_witness.py)"""
    q, k, v, do = r["_ops"]
    gs = []
    for b in range(case.ub):
        rb = {key: val[b] for key, val in r.items() if not key.startswith("_")}
        gs.append(bounds_c(rb, q[b], k[b], v[b], None if do is None else do[b], inp["scale"], u, ua, case.p_rounded,
                           None if seed is None else seed_eps(rb, *seed)))
    g = {key: torch.stack([x[key] for x in gs]) for key in gs[0]}
    if "dK" in g:
        g["dK"] = group_sum(case, g["dK"]) + u * group_sum(case, r["dK"]).abs() + 1e-6
        g["dV"] = group_sum(case, g["dV"])
    return g


def tile_q(case, t, b):
    """rows of batch element b of a [ub, uh, ...] per-query-head tensor -> [H, ...]"""
    return t[b % case.ub][case.hidx]


def tile_kv(case, t, b):
    return t[b % case.ub][torch.arange(case.Hkv) % case.uhk]


def reduce_n(case, t):
    """[ub, uh] per-problem dn -> the shape of the call's n: summed over the dimensions n broadcasts over"""
    full = t[case.bidx][:, case.hidx]
    return {"H": full.sum(0), "B1": full.sum(1, keepdim=True), "BH": full}[case.nshape]


def reduce_bias(case, t):
    """[ub, uh, L, S] per-problem dS -> the shape of the call's bias"""
    if case.bias == "hls":
        return (t.sum(0) * (case.B // case.ub))[case.hidx]
    return None   # dense: compared per batch element with tile_q


# ---------------------------------------------------------------- gates
class GateRefused(AssertionError):
    """a result a gate refuses outright: non-finite values, an lse that is not -inf exactly in the empty rows"""


def finite(*ts):
    for t in ts:
        if not torch.isfinite(_f64(t)).all():
            raise GateRefused("non-finite values")


def condition_a(case, r, dtype, p_eff):
    """the sizes keep a result's own rounding under 0.2: the largest count times u <= 0.2, and every logit is 0"""
    cmax = r["acc"].max().item()
    assert (r["m"] == 0).all(), "witness A: a logit is not 0"
    if "x" in r:
        assert (torch.where(torch.isfinite(r["x"]), r["x"], torch.zeros_like(r["x"])) == 0).all(), "witness A: a logit is not 0"
    assert cmax * (1 - p_eff) * U[dtype] <= 0.2, f"witness A: class count {cmax * (1 - p_eff)} x {U[dtype]} > 0.2: the output's own rounding would show"
    return cmax


def gate_a_fwd(out, lse, r_out_l_acc, p_eff):
    """|exp(lse) - Z_ref| <= 1e-5 Z_ref and |out Z_ref (1 - p_eff) - c_ref| <= 0.25 with c_ref = acc (1 - p_eff) the kept visible keys of
    a class; (ratio of lse, ratio of out). Tensors of one batch element: out [H, L, D], lse [H, L]."""
    l, acc = r_out_l_acc
    finite(out)
    if torch.isnan(_f64(lse)).any():
        raise GateRefused("lse is NaN")
    rz = _ratio((torch.exp(_f64(lse)) - l).abs(), 1e-5 * l)
    ro = _ratio(((_f64(out) * l.unsqueeze(-1) - acc) * (1 - p_eff)).abs(), torch.full_like(acc, 0.25))
    return rz, ro


def gate_a_dv(case, dv, r, p_eff, b, dtype):
    """where Z is a power of two (the n > 0 heads of a non-causal, unmasked case): |dV Z (1 - p_eff) - rows| <= 0.25 with rows the number
    of rows of a class that kept the key, summed over the K/V head's group. Returns the ratio, or None when no head of the group qualifies."""
    if pow2_n(case) is None:
        return None
    z = pow2_n(case) + case.S
    un = tile_q(case, r["_un"], b)   # [H]
    if not (un > 0).view(case.Hkv, case.G).all(1).any():
        return None
    sel = (un > 0).view(case.Hkv, case.G).all(1)
    want = tile_kv(case, group_sum(case, r["dV"]), b) * z * (1 - p_eff)
    if want.max().item() * unit(case, dtype) * (2 if p_eff else 1) > 0.2:
        return None   # (the count's own rounding - and, under dropout, that of the weight P / (1 - p) before its MFMA - would show: fp16 only)
    assert ((want[sel] - want[sel].round()).abs() <= 1e-9).all(), "witness A: the row counts are integers"
    want = want.round()
    return _ratio((_f64(dv)[sel] * z * (1 - p_eff) - want[sel]).abs(), torch.full_like(want[sel], 0.25))


def expect_b(r, v, n, min_gap=30.0):
    """Witness B's expectation of N problems from the clean reference r (dict of [N, ...]), v [N, S, D], n [N]. kind [N, L]:
    0 the row sees nothing - everything exactly 0; 1 a key decides; 2 the sink decides; 3 undecided (nothing wins by min_gap: not gated;
    the caller asserts where that may happen). Asserts that whatever decides does so by min_gap nats and that the reference itself gives the
    winner's V row. Returns kind, winner [N, L], onehot f [N, L, S] (the winner's dropout factor)."""
    x, m = r["x"], r["m"]
    N, L, S = x.shape
    top, win = x.max(-1)
    any_key = torch.isfinite(top)
    second = torch.where(torch.arange(S).view(1, 1, S) == win.unsqueeze(-1), torch.full_like(x, -math.inf), x).amax(-1)
    sink = (n > 0).view(N, 1).expand(N, L)   # the row has a sink
    key_wins = any_key & (second <= top - min_gap) & (~sink | (top >= min_gap))
    sink_wins = sink & (~any_key | (top <= -min_gap))
    kind = torch.where(~any_key & ~sink, 0, torch.where(key_wins, 1, torch.where(sink_wins, 2, 3)))
    one = torch.zeros(N, L, S, dtype=torch.float64)
    one.scatter_(2, win.unsqueeze(-1), (kind == 1).double().unsqueeze(-1))
    onef = one * r["f"]
    want = onef @ v
    dec = (kind != 3).unsqueeze(-1)
    assert ((r["out"] - want).abs() * dec <= 1e-11 * (1 + want.abs())).all(), "witness B: the reference itself is not the winner's V row"
    return kind, win, onef


def gate_b_out(out, kind, want, u):
    """|out - f V[t]| <= 2 u |f V[t]| + 1e-30 where a key decides (|out| <= 1e-12 where dropout removed it: V holds no exact zero),
    |out| <= 1e-12 where the sink does, exactly 0 where nothing is visible"""
    out = _f64(out)
    finite(out)
    k1, k2, k3 = ((kind == c).unsqueeze(-1) for c in (1, 2, 3))
    bound = torch.where(k1, 2 * u * want.abs() + torch.where(want == 0, 1e-12, 1e-30), torch.where(k2, torch.full_like(want, 1e-12), torch.zeros_like(want)))
    err = torch.where(k3, torch.zeros_like(want), (out - want).abs())
    return _ratio(err, bound)


def b_grad_bounds(r, onef, kind, q, k, do, scale, u, D, dropout):
    """(want, bound) of dV, dQ, dK per problem (module docstring): dV = onef^T dO within 2 u onef^T |dO| + 1e-12 (a key that wins
    no row) + twice the reference's own sum_i P_ij f_ij |dO_id| over the rows the key does not win (the rounded prescale moves a gap of 32
    nats by u 32 + the bias's rounding, far less than ln 2);
    dQ, dK within |scale| gamma sum_d |dO O| |k_t| (resp. |q_i|, summed over the rows the key wins) (1 + 2u) + 1e-6. Undecided rows
    (kind 3) make the problem's dK / dV ungated: the caller keeps them out."""
    gamma = 2 * (D + 2) * 2.0 ** -24 + (u if dropout else 0.0)
    oneT = onef.transpose(1, 2)
    dv_want = oneT @ do
    rest = (r["P"] * r["f"] - onef).clamp_min(0.0)   # the reference's own weights of the rows a key does not win (e^-32 and below)
    dv_bound = 2 * u * (oneT @ do.abs()) + 1e-12 + 2 * (rest.transpose(1, 2) @ do.abs())
    ds = gamma * r["delta_abs"] * (kind == 1)                      # [N, L]: |dS_it| at most this
    sel = (onef > 0).double()
    dq_bound = abs(scale) * (1 + 2 * u) * ds.unsqueeze(-1) * (sel @ k.abs()) + 1e-6
    dk_bound = abs(scale) * (1 + 2 * u) * (sel.transpose(1, 2) @ (ds.unsqueeze(-1) * q.abs())) + 1e-6
    return dict(dV=(dv_want, dv_bound), dQ=(torch.zeros_like(q), dq_bound), dK=(torch.zeros_like(k), dk_bound))


def ratio(got, want, bound):
    got = _f64(got)
    finite(got)
    return _ratio((got - want).abs(), bound)


# ---------------------------------------------------------------- launch plans without a GPU
def _view(v, strides, ptr=DUMMY):
    v.ptr = ptr
    for i, s in enumerate(strides):
        v.stride[i] = s


def plan_args(pkg, case, dtype, backward=True):
    """the BwdArgs block of the case's call as run() makes it (contiguous operands, n as a tensor: softmax_n = 0 in the block), with dummy
    aligned addresses: enough for fasn_launch_plan, which launches nothing"""
    Lb = pkg._lib
    a = Lb.BwdArgs()
    f = a.fwd
    B, H, Hkv, L, S, D = case.B, case.H, case.Hkv, case.L, case.S, case.D
    if case.nshape == "float" and L == 1 and Hkv != H:   # the grouped-query decode regroup: G query rows per K/V head
        H, L = Hkv, case.G
    for v in (f.q, f.o, a.dout, a.dq):
        _view(v, (H * L * D, L * D, D, 1))
    Hk = Hkv if (case.nshape != "float" or case.L != 1) else H
    for v in (f.k, f.v, a.dk, a.dv):
        _view(v, (Hk * S * D, S * D, D, 1))
    f.lse = DUMMY
    a.delta = DUMMY
    f.dtype, f.B, f.H, f.Sq, f.Sk, f.D, f.Dv = DT_ENUM[dtype], B, H, L, S, D, D
    f.scale = 1.0 / math.sqrt(D)
    f.softmax_n = 1.5 if case.nshape == "float" else 0.0
    f.causal, f.dropout_p = int(case.causal and H == case.H), case.p
    f.kv_group = H // Hk if Hk != H else 0
    if case.mask == "keypad":
        _view(f.mask, (S, 0, 0, 1))
    elif case.mask == "dense":
        _view(f.mask, (H * L * S, L * S, S, 1))
    elif case.mask == "misaligned":
        _view(f.mask, (H * L * (S + 1), L * (S + 1), S + 1, 1), ptr=DUMMY + 1)
    if case.bias is not None:
        _view(f.bias, (0 if case.bias == "hls" else H * L * S, L * S, S, 1))
        f.bias_dtype = Lb.FASN_BIAS_SAME
        if backward:
            if case.bias == "hls" and B > 1 and case.p == 0.0 and dtype != "fp32":
                _view(a.dbias, (0, L * S, S, 1))
                a.dbias_dtype = Lb.FASN_BIAS_SAME
            else:
                _view(a.dbias, (H * L * S, L * S, S, 1))
    return a


def plan_text(pkg, case, dtype):
    """the fasn_launch_plan text of the case: forward (with its workspace) and, where the case runs one, backward"""
    import ctypes
    Lb = pkg._lib
    lib = Lb.load()
    buf = ctypes.create_string_buffer(1 << 14)
    out = []
    for name, which in (("fwd", Lb.FASN_PLAN_FWD_WS), ("bwd", Lb.FASN_PLAN_BWD)):
        if name == "bwd" and not case.bwd:
            continue
        a = plan_args(pkg, case, dtype, backward=(name == "bwd"))
        rc = lib.fasn_launch_plan(a, which, buf, len(buf))
        out.append(f"  [{name}] rc={rc} fwd_path={lib.fasn_fwd_path(a.fwd)}" + (f" bwd_path={lib.fasn_bwd_path(a)}" if name == "bwd" else ""))
        out += ["    " + line for line in buf.value.decode().splitlines()]
    return "\n".join(out)


# ---------------------------------------------------------------- the call on the GPU
def _leaf_like(t):
    """a leaf that requires grad with t's values AND strides (clone() makes a view with padded rows contiguous, which moves a bias
    whose rows are aligned only through their padding to the element loads)"""
    leaf = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device)
    leaf.copy_(t.detach())
    return leaf.requires_grad_()


def run(pkg, case, inp, seed=1, backward=None):
    """the case's call through flash_attention_n (and its backward with inp["do"]), and once more through flash_attn._launch_fwd, which
    returns lse and must give the same output bit for bit. Returns a dict: out, lse (None for the regrouped decode), dq, dk, dv, dn,
    dbias (None where not asked), state (the dropout state or None)."""
    from flash_attention_softmax_n_amd import flash_attn
    backward = case.bwd if backward is None else backward
    q, k, v, n = inp["q"], inp["k"], inp["v"], inp["n"]
    kwargs = dict(scale=inp["scale"], dropout_p=case.p, attn_mask=inp["mask"], is_causal=case.causal)
    res = dict(dq=None, dk=None, dv=None, dn=None, dbias=None, lse=None)
    torch.manual_seed(seed)
    if backward:
        qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
        nn = n.detach().clone().requires_grad_() if torch.is_tensor(n) else n
        bb = None if inp["bias"] is None else _leaf_like(inp["bias"])
        out = pkg.flash_attention_n(qq, kk, vv, softmax_n_param=nn, attn_bias=bb, **kwargs)
        state = flash_attn.last_dropout_state()
        out.backward(inp["do"])
        res.update(dq=qq.grad, dk=kk.grad, dv=vv.grad, dn=nn.grad if torch.is_tensor(nn) else None, dbias=None if bb is None else bb.grad)
    else:
        with torch.no_grad():
            out = pkg.flash_attention_n(q, k, v, softmax_n_param=n, attn_bias=inp["bias"], **kwargs)
        state = flash_attn.last_dropout_state()
    res.update(out=out.detach(), state=state)
    if case.nshape != "float":
        q_, k_, v_, m_, b_, n_, sc, dp, _, _, small = flash_attn._prepare(q, k, v, n, inp["scale"], case.p, inp["mask"], inp["bias"])
        if b_ is not None:
            b_ = b_.expand(case.B, case.H, case.L, case.S)
        o2, lse = flash_attn._launch_fwd(q_, k_, v_, m_, b_, n_, sc, case.causal, dp, state)
        assert torch.equal(o2, res["out"]), "flash_attention_n and _launch_fwd disagree"
        res["lse"] = lse
    return res


# ---------------------------------------------------------------- a result in the layout of run(), from a reference
def as_result(case, r, dtype, backward=True):
    """what a kernel that computed exactly `r` (a reference() result, mutated or not) would return: every tensor tiled over [B, H] and
    rounded once to its type (lse, dn fp32)"""
    res = dict(out=_tile(case, r["out"]).to(dtype), lse=_tile(case, r["lse"]).float(), dq=None, dk=None, dv=None, dn=None, dbias=None, state=None)
    if backward and "dV" in r:
        res.update(dq=_tile(case, r["dQ"]).to(dtype), dk=_tile(case, group_sum(case, r["dK"]), "kv").to(dtype),
                   dv=_tile(case, group_sum(case, r["dV"]), "kv").to(dtype))
        if case.nshape != "float":
            res["dn"] = reduce_n(case, r["dn"]).float()
        if case.bias is not None:
            res["dbias"] = (reduce_bias(case, r["dS"]) if case.bias == "hls" else _tile(case, r["dS"])).to(dtype)
    return res


def _lse_pair(got, want):
    """lse with -inf rows (nothing visible, n = 0) taken out: they must be -inf in both"""
    got, want = _f64(got), want.clone()
    empty = torch.isinf(want)
    if torch.isnan(got).any() or not torch.equal(torch.isinf(got) & (got < 0), empty):
        raise GateRefused("lse: the rows that see nothing with n = 0 must hold -inf, and only they; no NaN")
    return torch.where(empty, torch.zeros_like(got), got), torch.where(empty, torch.zeros_like(want), want)


class Ratios(dict):
    def up(self, key, val):
        if val is not None:
            self[key] = max(self.get(key, 0.0), val)

    def worst(self):
        return max(self.values()) if self else 0.0

    def __str__(self):
        return ", ".join(f"{k} {v:.3g}" for k, v in self.items())


def judge_c(case, dtype, res, r, g, rat=None, skip=()):
    """every result of the call against witness C's per-element gates: the largest ratio per tensor"""
    u = U[dtype]
    rat = Ratios() if rat is None else rat
    bwd = res.get("dq") is not None
    for b in range(case.B):
        rat.up("out", ratio(res["out"][b], tile_q(case, r["out"], b), tile_q(case, g["out"], b)))
        if res.get("lse") is not None:
            got, want = _lse_pair(res["lse"][b], tile_q(case, r["lse"], b))
            rat.up("lse", _ratio((got - want).abs(), tile_q(case, g["lse"], b)))
        if bwd:
            rat.up("dQ", ratio(res["dq"][b], tile_q(case, r["dQ"], b), tile_q(case, g["dQ"], b)))
            if "dK" not in skip:
                rat.up("dK", ratio(res["dk"][b], tile_kv(case, group_sum(case, r["dK"]), b), tile_kv(case, g["dK"], b)))
            rat.up("dV", ratio(res["dv"][b], tile_kv(case, group_sum(case, r["dV"]), b), tile_kv(case, g["dV"], b)))
            if res.get("dbias") is not None and case.bias == "bhls":
                want = tile_q(case, r["dS"], b)
                rat.up("dbias", ratio(res["dbias"][b], want, tile_q(case, g["dS"], b) + u * want.abs() + 1e-6))
    if bwd and res.get("dn") is not None:
        want = reduce_n(case, r["dn"])
        rat.up("dn", ratio(res["dn"], want, reduce_n(case, g["dn"]) + 1e-6))
    if bwd and res.get("dbias") is not None and case.bias == "hls":
        want = reduce_bias(case, r["dS"])
        rat.up("dbias", ratio(res["dbias"], want, reduce_bias(case, g["dS"]) + u * want.abs() + 1e-6))
    return rat


def judge_a(case, dtype, res, r, g, p_eff=0.0):
    """witness A: the integer gates on exp(lse) and out Z (1 - p_eff) of every (batch, head, row); dK exactly 0; dV Z (1 - p_eff) an integer
    count where Z is a power of two; dQ, dV, dn, dbias under witness C's per-element gates (with q = 0 they hold no prescale term)"""
    rat = Ratios()
    bwd = res.get("dq") is not None
    for b in range(case.B):
        l, acc = tile_q(case, r["l"], b), tile_q(case, r["acc"], b)
        if res.get("lse") is not None:
            rz, ro = gate_a_fwd(res["out"][b], res["lse"][b], (l, acc), p_eff)
            rat.up("exp(lse)", rz)
        else:
            finite(res["out"][b])
            ro = _ratio(((_f64(res["out"][b]) * l.unsqueeze(-1) - acc) * (1 - p_eff)).abs(), torch.full_like(acc, 0.25))
        rat.up("out Z", ro)
        if bwd:
            rat.up("dK = 0", _ratio(_f64(res["dk"][b]).abs(), torch.zeros_like(_f64(res["dk"][b]))))
            rat.up("dV Z", gate_a_dv(case, res["dv"][b], r, p_eff, b, dtype))
    if bwd:
        rc = judge_c(case, dtype, res, r, g, skip=("dK",))
        for key in ("dQ", "dV", "dn", "dbias"):
            if key in rc:
                rat.up(key, rc[key])
    return rat


def judge_b(case, form, dtype, res, r, g, inp, min_gap=30.0):
    """witness B: out against the deciding key's V row in every (batch, head, row), lse under the prescale bound, and (bounded code) dV, dQ,
    dK, dn. Returns (ratios, the set of row kinds met). code_sink: the heads with n = 0 hold rows that no key decides (ties); only there
    may rows be undecided, and those heads' results are not gated."""
    u = U[dtype]
    rat, kinds = Ratios(), set()
    q, k, v, do = r["_ops"]
    bwd = res.get("dq") is not None
    per = []
    for ib in range(case.ub):
        rb = {key: val[ib] for key, val in r.items() if not key.startswith("_")}
        kind, win, onef = expect_b(rb, v[ib], r["_un"][ib], min_gap)
        und = (kind == 3).any(1)
        if form == "code_sink":   # (and exp(-lse) of a head without a sink overflows there: lse is about -400)
            und = und | (r["_un"][ib] == 0)
        assert not und.any() or form == "code_sink", f"witness B {form}: rows that nothing decides by {min_gap} nats"
        assert not ((kind == 3).any(1) & (r["_un"][ib] > 0)).any(), "witness B: undecided rows in a head with a sink"
        kinds |= set(kind.unique().tolist())
        e = dict(kind=kind, want=onef @ v[ib], live=~und)
        if bwd:
            e["g"] = b_grad_bounds(rb, onef, kind, q[ib], k[ib], do[ib], inp["scale"], u, case.D, case.p > 0)
        per.append(e)
    live = torch.stack([e["live"] for e in per])                       # [ub, uh]
    live_kv = live.view(case.ub, case.uhk, case.G).all(2)
    stack = lambda f: torch.stack([f(e) for e in per])                # noqa: E731
    kind, want = stack(lambda e: e["kind"]), stack(lambda e: e["want"])
    if bwd:
        gb = {key: (stack(lambda e: e["g"][key][0]), stack(lambda e: e["g"][key][1])) for key in ("dV", "dQ", "dK")}
    for b in range(case.B):
        rat.up("out", gate_b_out(res["out"][b], tile_q(case, kind, b), tile_q(case, want, b), u))
        lv = tile_q(case, live, b)
        if res.get("lse") is not None:
            got, wl = _lse_pair(res["lse"][b][lv], tile_q(case, r["lse"], b)[lv])
            rat.up("lse", _ratio((got - wl).abs(), tile_q(case, g["lse"], b)[lv]))
        if bwd:
            rat.up("dQ", ratio(res["dq"][b][lv], tile_q(case, gb["dQ"][0], b)[lv], tile_q(case, gb["dQ"][1], b)[lv]))
            lk = tile_kv(case, live_kv, b)
            for key, got in (("dK", res["dk"]), ("dV", res["dv"])):
                w_, b_ = (tile_kv(case, group_sum(case, t), b)[lk] for t in gb[key])
                rat.up(key, ratio(got[b][lk], w_, b_))
    if bwd and res.get("dn") is not None:
        ln = reduce_n(case, live.double()) == reduce_n(case, torch.ones_like(live, dtype=torch.float64))
        want_n = reduce_n(case, torch.where(live, r["dn"], torch.zeros_like(r["dn"])))
        rat.up("dn", ratio(res["dn"][ln], want_n[ln], torch.full_like(want_n[ln], 1e-6)))
    return rat, kinds


# ---------------------------------------------------------------- the routes: every family of DESIGN 4.2 at its smallest shape
# (a_dtypes: witness A runs in fp16 only where S > 992 puts two half tiles of 32 keys into one class in bf16: 64 u = 0.25 > 0.2)
RAGGED = [300, 512, 512, 77, 448]
SHAPES = {
    # D = 64 small grids: 32 rows per wave, L != S both ways (rows without keys), S no multiple of 64; the pipelined backward
    "d64 small L<S": Case(2, 4, 300, 420, 64, want=("D=64,QB=1,plain", "fasn_bwd_dq_pipe_kernel", "fasn_bwd_dkdv_pipe_kernel")),
    "d64 small L>S causal": Case(2, 4, 420, 300, 64, causal=True, nshape="BH", want=("D=64,QB=1,causal", "_pipe_")),
    "d64 small L<S causal": Case(2, 4, 300, 420, 64, causal=True, nshape="B1", want=("D=64,QB=1,causal", "_pipe_")),
    # D = 64, 64 rows per wave
    "d64 64 rows": Case(8, 16, 1024, 1024, 64, a_dtypes=("fp16",), ub=2, uh=2, nshape="BH", want=("D=64,QB=2,plain", "_pipe_")),
    "d64 64 rows keypad": Case(8, 16, 1024, 1024, 64, a_dtypes=("fp16",), mask="keypad", lens=[1024, 700, 64, 5], ub=4, uh=2, want=("D=64,QB=2,keypad", "fasn_bwd_dq_kernel", "fasn_bwd_dkdv_kernel")),
    # folded causal rows with an odd block count (paired blocks: grid = 3 of 5 blocks per head), and L != S
    "d64 fold odd pairs": Case(13, 32, 1152, 1152, 64, a_dtypes=("fp16",), causal=True, ub=1, uh=2, bwd=False, want=("FOLD=1", "QB=2", "pair")),
    "d64 fold L!=S": Case(16, 32, 1100, 1300, 64, a_dtypes=("fp16",), causal=True, ub=1, uh=2, bwd=False, want=("FOLD=1",)),
    # long launches: the dynamic XCD deal
    "d64 xcd plain": Case(32, 32, 1000, 1000, 64, a_dtypes=("fp16",), ub=1, uh=2, bwd=False, want=("D=64,QB=2,plain",)),
    "d64 xcd causal": Case(32, 32, 2000, 2000, 64, causal=True, ub=1, uh=2, bwd=False, dtypes=("fp16",), want=("FOLD=1",)),
    # D = 128: plain, causal (paired), bias + key padding on a length-paired ragged batch; the two-wave backward and the reduced dbias
    "d128 plain": Case(5, 16, 512, 512, 128, ub=1, uh=2, nshape="BH", want=("D=128,QB=1,plain", "_ws_")),
    "d128 causal": Case(5, 16, 1024, 1024, 128, a_dtypes=("fp16",), causal=True, ub=1, uh=2, want=("D=128,QB=1,causal", "pair", "_ws_")),
    "d128 bias keypad ragged": Case(5, 16, 512, 512, 128, bias="hls", mask="keypad", lens=RAGGED, ub=5, uh=2, want=("bias+keypad", "_ws_", "fasn_bwd_dbias_ws_kernel")),
    # D = 256: the two-wave kernels, head groups, grouped K/V, a bias (fast reduced dbias)
    "d256 plain": Case(2, 16, 384, 320, 256, ub=1, uh=2, want=("_ws256_",)),
    "d256 causal gqa": Case(2, 32, 256, 256, 256, Hkv=8, causal=True, ub=1, uh=8, want=("_ws256_", "GQA=1")),
    "d256 bias": Case(2, 16, 200, 200, 256, bias="hls", ub=2, uh=2, wit="AC", want=("_ws256_", "bias+mask", "fasn_bwd_dbias_kernel", "FAST=true")),
    # D = 32
    "d32 plain": Case(2, 4, 300, 420, 32, nshape="BH", want=("D=32,QB=2,plain",)),
    "d32 causal bias dense": Case(2, 4, 300, 420, 32, causal=True, bias="hls", mask="dense", want=("D=32,QB=1,bias+mask", "fasn_bwd_dbias_kernel")),
    # vector bias and dense mask at D = 64; causal with a bias pairs its blocks; reduced (both kernels) and dense dbias
    "d64 bias": Case(2, 4, 300, 420, 64, bias="hls", want=("D=64,QB=1,bias,", "fasn_bwd_dbias_kernel", "FAST=false")),
    "d64 dense mask causal": Case(2, 4, 300, 420, 64, mask="dense", causal=True, nshape="BH", want=("D=64,QB=1,mask",)),
    "d64 bias causal paired": Case(4, 16, 1024, 1024, 64, a_dtypes=("fp16",), bias="hls", causal=True, ub=1, uh=2, wit="AC", want=("pair", "fasn_bwd_dbias_ws_kernel")),
    "d64 dense dbias": Case(2, 4, 300, 420, 64, bias="bhls", mask="dense", wit="AC", want=("D=64,QB=1,bias+mask",)),
    # split-K: a few rows over thousands of keys; under key padding the last splits' keys are all hidden
    "split 5x4000": Case(1, 16, 5, 4000, 64, uh=2, a_dtypes=("fp16",), want=("SPLIT=1", "fasn_fwd_combine_kernel")),
    "split 130x4090 causal": Case(1, 16, 130, 4090, 64, causal=True, uh=2, a_dtypes=("fp16",), want=("SPLIT=1", "fasn_fwd_combine_kernel")),
    "split hidden splits": Case(1, 16, 130, 4080, 64, mask="dense", hide_from=700, uh=2, bwd=False, want=("SPLIT=1", "fasn_fwd_combine_kernel")),
    # split-K at the other head dims, with a backward behind it: D = 128 plain (register staging), D = 128 causal at an ordinary small-batch
    # training shape (128 row blocks < 256, 16 key tiles: two splits), D = 32
    "split d128 plain": Case(1, 16, 130, 4090, 128, uh=2, a_dtypes=("fp16",), want=("D=128,QB=1,plain", "SPLIT=1", "SEED=2", "_ws_")),
    "split d128 causal training": Case(1, 16, 1024, 1024, 128, causal=True, uh=2, a_dtypes=("fp16",), want=("D=128,QB=1,causal", "SPLIT=1", "SEED=2", "_ws_")),
    "split d32": Case(1, 16, 130, 4090, 32, uh=2, a_dtypes=("fp16",), want=("D=32,QB=1,plain", "SPLIT=1", "SEED=2")),
    # grouped K/V heads: the forward's head map and the dK / dV sum over the group
    "gqa": Case(2, 8, 300, 420, 64, Hkv=2, want=("GQA=1",)),
    "gqa causal": Case(2, 8, 300, 420, 64, Hkv=2, causal=True, nshape="BH", want=("GQA=1",)),
    # dropout: plain (both tuning points), causal, key padding, grouped K/V
    "drop": Case(2, 4, 300, 420, 64, p=0.1, want=("DROP=1", "_pipe_")),
    "drop 64 rows": Case(32, 16, 256, 192, 64, p=0.1, wit="A", bwd=False, dtypes=("fp16",), want=("QB=2", "DROP=1")),
    "drop causal": Case(2, 4, 300, 420, 64, p=0.25, causal=True, nshape="BH", want=("DROP=1", "causal")),
    "drop keypad": Case(2, 4, 300, 420, 64, p=0.1, mask="keypad", lens=[420, 100], want=("DROP=1", "keypad")),
    "drop gqa": Case(2, 8, 300, 420, 64, Hkv=2, p=0.1, want=("DROP=1", "GQA=1")),
    # the grouped-query decode regroup (float n): G query rows per K/V head, forward only
    "gqa decode regroup": Case(2, 8, 1, 420, 64, Hkv=2, nshape="float", bwd=False, want=("D=64,QB=1,plain",)),
    # the element-load kernels: a dense mask whose rows are no aligned vectors
    "element loads": Case(2, 4, 130, 200, 64, mask="misaligned", want=("element-load",)),
    # fp32 kernels: A, B (the ladder) and C at u = unit(case, fp32)
    "fp32": Case(2, 2, 130, 96, 32, dtypes=("fp32",), want=("fasn_f32_",)),
    "fp32 causal": Case(2, 2, 130, 96, 32, causal=True, dtypes=("fp32",), nshape="BH", want=("fasn_f32_",)),
}

# ---------------------------------------------------------------- the instantiations: the modes of each family that the cases above leave out
# (NEW names them: tests/test_attnwitness_cpu.py runs the emulation bound on every 16-bit one of them)
RAGGED16 = [512, 300, 448, 77, 512, 5, 64, 511, 129, 512, 200, 333, 1, 450, 65, 512]
_NEW = {
    # D = 128, 8 waves: the kernel of every large D = 128 launch (512 row blocks of 256 rows and more)
    "d128 8-wave plain": Case(16, 32, 256, 320, 128, ub=1, uh=2, bwd=False, want=("D=128,QB=1,plain", "NW=8")),
    "d128 8-wave causal": Case(16, 32, 512, 512, 128, causal=True, ub=1, uh=2, bwd=False, want=("D=128,QB=1,causal", "NW=8")),
    # D = 128: key padding (two-wave backward), with causal and grouped K/V; dropout keeps the one-wave backward
    "d128 keypad": Case(4, 4, 300, 420, 128, mask="keypad", lens=[420, 300, 64, 5], want=("D=128", "keypad", "_ws_")),
    "d128 keypad causal gqa": Case(2, 8, 300, 420, 128, Hkv=2, mask="keypad", lens=[420, 100], causal=True, want=("keypad", "GQA=1", "_ws_")),
    # (the two-wave kernels have dropout instantiations of their own and take every dropout call with one query head per K/V head: only grouped
    # K/V under dropout is left to the one-wave dQ and dK / dV kernels at this head dim, launch_bwd_one of fasn_bwd_launch.h)
    "d128 drop": Case(2, 8, 300, 420, 128, Hkv=2, p=0.1, want=("D=128", "DROP=1", "GQA=1", "fasn_bwd_dq_kernel", "fasn_bwd_dkdv_kernel")),
    "d128 drop causal keypad": Case(2, 8, 300, 420, 128, Hkv=2, p=0.25, causal=True, mask="keypad", lens=[420, 100], nshape="BH", want=("DROP=1", "keypad", "GQA=1", "fasn_bwd_dq_kernel", "fasn_bwd_dkdv_kernel")),
    "d128 drop two-wave": Case(2, 4, 300, 420, 128, p=0.1, want=("D=128", "DROP=1", "fasn_bwd_dq_ws_kernel", "fasn_bwd_dkdv_ws_kernel")),
    "d128 drop causal keypad two-wave": Case(2, 4, 300, 420, 128, p=0.25, causal=True, mask="keypad", lens=[420, 100], nshape="BH", want=("DROP=1", "keypad", "fasn_bwd_dq_ws_kernel", "fasn_bwd_dkdv_ws_kernel")),
    # D = 256: key padding, the general instantiation (dense mask), dropout
    "d256 keypad": Case(2, 4, 200, 200, 256, mask="keypad", lens=[200, 70], want=("_ws256_", "keypad")),
    "d256 dense mask": Case(2, 4, 200, 200, 256, mask="dense", causal=True, nshape="BH", want=("_ws256_", "bias+mask")),
    "d256 drop": Case(2, 4, 200, 200, 256, p=0.1, want=("_ws256_", "DROP=1")),
    # D = 32
    "d32 keypad causal": Case(2, 4, 300, 420, 32, mask="keypad", lens=[420, 100], causal=True, want=("D=32", "keypad")),
    "d32 drop": Case(2, 4, 300, 420, 32, p=0.1, want=("D=32", "DROP=1")),
    "d32 gqa": Case(2, 8, 300, 420, 32, Hkv=2, nshape="BH", want=("D=32", "GQA=1")),
    # D = 64: key padding under causal; the 64-rows-per-wave dropout kernel with its backward
    "d64 keypad causal": Case(2, 4, 300, 420, 64, mask="keypad", lens=[420, 100], causal=True, nshape="B1", want=("D=64,QB=1,keypad",)),
    "d64 drop 64 rows bwd": Case(32, 16, 256, 192, 64, p=0.1, wit="A", want=("QB=2", "DROP=1", "_pipe_")),
    # D = 64, 8 waves: the general kernels of large grids
    "d64 8-wave bias": Case(8, 32, 512, 520, 64, bias="hls", ub=1, uh=2, bwd=False, wit="AC", want=("D=64,QB=2,bias,", "NW=8")),
    "d64 8-wave dense mask": Case(8, 32, 512, 520, 64, mask="dense", ub=1, uh=2, bwd=False, want=("QB=2,mask", "NW=8")),
    "d64 8-wave bias+mask": Case(8, 32, 512, 520, 64, bias="hls", mask="dense", ub=1, uh=2, bwd=False, wit="AC", want=("QB=2,bias+mask", "NW=8")),
    "d64 8-wave bias keypad": Case(16, 32, 512, 512, 64, bias="hls", mask="keypad", lens=RAGGED16, ub=16, uh=2, bwd=False, wit="AC", want=("bias+keypad", "NW=8")),
    "d64 8-wave bias causal": Case(16, 32, 512, 512, 64, bias="hls", causal=True, ub=1, uh=2, bwd=False, wit="AC", want=("QB=2", "NW=8")),
    # split-K under key padding: the last splits see no key (S = 4092: a key-padding row of 4090 bytes is no run of aligned 4-byte vectors, and
    # such a mask takes the element loads, which do not split)
    "split keypad": Case(1, 16, 130, 4092, 64, mask="keypad", lens=[700], uh=2, want=("D=64,QB=1,bias+mask", "SPLIT=1", "keypad", "fasn_fwd_combine_kernel")),
    "split keypad d128": Case(1, 16, 130, 4092, 128, mask="keypad", lens=[700], uh=2, want=("D=128", "SPLIT=1", "keypad", "fasn_fwd_combine_kernel", "_ws_")),
    "split keypad d32": Case(1, 16, 130, 4092, 32, mask="keypad", lens=[700], uh=2, a_dtypes=("fp16",), want=("D=32", "SPLIT=1", "keypad", "fasn_fwd_combine_kernel")),
    # fp32 kernels: the other head dims, the mask / bias / dropout mode, grouped K/V
    "fp32 d64": Case(2, 2, 130, 96, 64, dtypes=("fp32",), want=("fasn_f32_", "D=64")),
    "fp32 d128 causal": Case(1, 2, 130, 96, 128, causal=True, dtypes=("fp32",), want=("fasn_f32_", "D=128")),
    "fp32 mask bias": Case(2, 2, 130, 96, 32, mask="dense", bias="bhls", dtypes=("fp32",), want=("fasn_f32_",)),
    "fp32 drop": Case(2, 2, 130, 96, 32, p=0.1, dtypes=("fp32",), want=("fasn_f32_",)),
    "fp32 gqa": Case(2, 4, 130, 96, 32, Hkv=2, dtypes=("fp32",), want=("fasn_f32_",)),
}
NEW = tuple(_NEW)
SHAPES.update(_NEW)


def seed_of(name):
    return 1000 + sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 9000


def plans_file_text(pkg):
    out = []
    for name, case in SHAPES.items():
        for dt in case.dtypes:
            out.append(f"{name} [{dt}]")
            out.append(plan_text(pkg, case, dt))
    return "\n".join(out) + "\n"
