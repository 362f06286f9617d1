"""The attention kernels' arithmetic on the CPU, with exactly the rounding points of the derivation in the docstring of
tests/attn_witness.py. Shared by tests/test_attnwitness_cpu.py and tests/test_biaswitness_cpu.py (no test is collected from here).

emulate(w) takes a "world": an object with case, inp, dt (the operand type), keep (the dropout keep mask or None) and p_eff.

Two models of the forward's score:
  seeded=None   the score of a key is an ABSOLUTE fp32 value, scale log2e q.k + bias log2e, formed in one piece. That is the arithmetic
                of the kernels that do not seed their accumulators from a running maximum (fasn_fwd_ws256.h, fasn_f32_kernels.h, the
                element-load mode) and, for every row whose maximum stays within a few hundred log2 units of 0, also of the seeded ones.
  seeded="inf" / "floor"
                rounding point (9), DESIGN 4.1 "Seeded accumulators": the vector bias modes of fasn_fwd_kernel start a tile's score
                accumulator from fma(bias, log2e, -m_run) in fp32 and add q'.k onto it in D / 16 MFMA steps, each rounded to fp32; a
                row that is still UNSEEDED starts from bias log2e alone (mref = 0) and takes the exact path. What "unseeded" means is the
                parameter: "inf" is m_run == -inf (the kernels before the floor), "floor" is not (m_run > -F) (the kernels with it).
                `tiles_per_split` models split-K: every split starts its own online-softmax state - unseeded even under a sink, which
                only split 0 holds - and the partials are merged as fasn_fwd_combine_kernel does. The backward's score starts from
                fma(bias, log2e, -lse log2e), as the backward kernels' does.
In every model the backward gives a row whose lse lies below -LSE_FLOOR nats no weights (lse_no_weights, csrc/fasn_common.h)."""
import math

import torch

import attn_witness as aw

LOG2E_F32 = float(torch.tensor(aw.LOG2E, dtype=torch.float32))
LSE_FLOOR = 2.0 ** 22   # kLseFloor of csrc/fasn_common.h (nats): below it a row has no weights in the backward, as at lse = -inf


def _steps(start, a, bt):
    """start [.., L, T] fp32 + a [.., L, D] . bt [.., T, D]^T, 16 features per MFMA, every step rounded to fp32"""
    s = start
    for d0 in range(0, a.shape[-1], 16):
        s = (s.double() + a[..., d0:d0 + 16].double() @ bt[..., d0:d0 + 16].double().transpose(-1, -2)).float()
    return s


def _forward_seeded(qs, kf, vf, vis, f, bias, n, rd, D, mode, F, tiles):
    """one split-K forward ([uh, L] state per split) in the seeded arithmetic: m, l (log2 domain), acc of the merged result"""
    uh, L, S = vis.shape
    KT = aw.KT
    ntiles = -(-S // KT)
    tps = ntiles if tiles is None else tiles
    parts = []
    for t0 in range(0, max(ntiles, 1), tps):
        first = t0 == 0
        sink = (n > 0) & first
        m = torch.where(sink, 0.0, -math.inf).expand(uh, L).clone().float()
        l = torch.where(sink, n, torch.zeros_like(n)).expand(uh, L).clone().float()
        acc = torch.zeros(uh, L, D)
        for t in range(t0, min(t0 + tps, ntiles)):
            sl = slice(t * KT, min((t + 1) * KT, S))
            unseeded = torch.isinf(m) if mode == "inf" else ~(m > -F)
            mref = torch.where(unseeded, torch.zeros_like(m), m)
            if bias is None:
                start = (-mref).unsqueeze(-1).expand(uh, L, sl.stop - sl.start).contiguous()
            else:   # one fma: exact product and sum, one rounding
                start = (bias[..., sl].double() * LOG2E_F32 - mref.double().unsqueeze(-1)).float().expand(uh, L, -1).contiguous()
            s = _steps(start, qs, kf[:, sl])
            s = torch.where(vis[..., sl], s, torch.full_like(s, -math.inf))
            mx = s.amax(-1)
            m_new = torch.maximum(m, mx + mref)
            m_use = torch.where(torch.isinf(m_new) & (m_new < 0), torch.zeros_like(m_new), m_new)
            alpha = torch.exp2(m - m_use)
            p = rd(torch.exp2(s - (m_use - mref).unsqueeze(-1)))
            l = l * alpha + p.sum(-1)
            acc = acc * alpha.unsqueeze(-1) + rd(p * f[..., sl]) @ vf[:, sl]
            m = m_new
        parts.append((m, l, acc))
    if len(parts) == 1:
        return parts[0]
    mstar = torch.stack([p_[0] for p_ in parts]).amax(0)
    m_use = torch.where(torch.isinf(mstar) & (mstar < 0), torch.zeros_like(mstar), mstar)
    l = torch.zeros(uh, L)
    acc = torch.zeros(uh, L, D)
    for ms, ls, accs in parts:
        wgt = torch.where(torch.isinf(ms) & (ms < 0), torch.zeros_like(ms), torch.exp2(ms - m_use))
        l = l + ls * wgt
        acc = acc + accs * wgt.unsqueeze(-1)
    return mstar, l, acc


def emulate(w, seeded=None, F=None, tiles_per_split=None):
    """the kernels' arithmetic on the CPU with exactly the rounding points of the derivation: the prescaled Q (forward, dQ) or K (dK / dV)
    rounded to the operand type, fp32 scores in the log2 domain (absolute, or - `seeded` - accumulated step by step onto the start value
    fma(bias, log2e, -m_run): module docstring), an online softmax over 64-key tiles, P rounded for the P.V product and l summed from the
    rounded weights, fp32 accumulation, O rounded once; fp32 lse; the backward recomputes P = exp2(x' - lse log2e), rounds P for dV and (as
    the two-wave kernels do) before dS, rounds dS for dQ / dK, reads delta from the rounded O, and rounds each result once."""
    assert seeded in (None, "inf", "floor") and (seeded != "floor" or F is not None)
    case, inp, dt = w.case, w.inp, w.dt
    q, k, v, do, un, ubias = aw.unique_operands(case, inp)
    c = inp["scale"] * aw.LOG2E
    rd = lambda t: t.to(dt).float()   # noqa: E731
    wt = aw.weights(case, inp["um"])
    res = {key: [] for key in ("out", "lse", "dQ", "dK", "dV", "dS", "dn")}
    for b in range(case.ub):
        qf, kf, vf, dof = q[b].float(), k[b].float(), v[b].float(), do[b].float()
        vis = (wt[b] > 0).expand(case.uh, -1, -1)
        n = un[b].float().view(-1, 1)
        bias1 = None if ubias is None else ubias[b if ubias.shape[0] > 1 else 0].float()
        bias2 = None if bias1 is None else bias1 * aw.LOG2E
        f = torch.ones(case.uh, case.L, case.S) if w.keep is None else (w.keep[b] / (1 - w.p_eff)).float()
        qs, ks = rd(qf * c), rd(kf * c)
        if seeded is None:
            m = torch.where(n > 0, 0.0, -math.inf).expand(case.uh, case.L).clone()
            l = n.expand(case.uh, case.L).clone()
            acc = torch.zeros(case.uh, case.L, case.D)
            for k0 in range(0, case.S, aw.KT):
                sl = slice(k0, k0 + aw.KT)
                s = qs @ kf[:, sl].transpose(1, 2)
                if bias2 is not None:
                    s = s + bias2[..., sl]
                s = torch.where(vis[..., sl], s, torch.full_like(s, -math.inf))
                m_new = torch.maximum(m, s.amax(-1))
                m_use = torch.where(torch.isfinite(m_new), m_new, torch.zeros_like(m_new))
                alpha = torch.exp2(m - m_use)
                p = rd(torch.exp2(s - m_use.unsqueeze(-1)))
                l = l * alpha + p.sum(-1)
                acc = acc * alpha.unsqueeze(-1) + rd(p * f[..., sl]) @ vf[:, sl]
                m = m_new
        else:
            m, l, acc = _forward_seeded(qs, kf, vf, vis, f, bias1, n, rd, case.D, seeded, F, tiles_per_split)
        has = l > 0
        safe = torch.where(has, l, torch.ones_like(l))
        o = rd(acc / safe.unsqueeze(-1))
        m0 = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        lse2 = torch.where(has, m0 + torch.log2(safe), torch.full_like(m, math.inf))   # log2 domain; rows without anything: P = 0
        res["out"].append(o.double())
        res["lse"].append(torch.where(has, lse2 / aw.LOG2E, torch.full_like(m, -math.inf)).double())
        delta = (dof * o).sum(-1)
        has = has & ~(lse2 / aw.LOG2E < -LSE_FLOOR)   # the backward: a row below the lse floor has no weights (P = 0, nothing to dn)
        lse2 = torch.where(has, lse2, torch.full_like(lse2, math.inf))
        grads = {}
        for side in ("q", "k"):
            if seeded is None:
                s = qs @ kf.transpose(1, 2) if side == "q" else qf @ ks.transpose(1, 2)
                if bias2 is not None:
                    s = s + bias2
                s = torch.where(vis, s, torch.full_like(s, -math.inf))
                P = torch.exp2(s - lse2.unsqueeze(-1))
            else:
                if bias1 is None:
                    start = (-lse2).unsqueeze(-1).expand(case.uh, case.L, case.S).contiguous()
                else:
                    start = (bias1.double() * LOG2E_F32 - lse2.double().unsqueeze(-1)).float().expand(case.uh, case.L, -1).contiguous()
                s = _steps(start, qs, kf) if side == "q" else _steps(start, qf, ks)
                P = torch.exp2(torch.where(vis, s, torch.full_like(s, -math.inf)))
            dP = f * (dof @ vf.transpose(1, 2))
            dS = rd((rd(P) if case.p_rounded else P) * (dP - delta.unsqueeze(-1)))   # (rounding point 7: the two-wave kernels' P arrives rounded)
            if side == "q":
                grads["dQ"] = rd(inp["scale"] * (dS @ kf))
                grads["dS"] = dS
            else:
                grads["dK"] = inp["scale"] * (dS.transpose(1, 2) @ qf)
                grads["dV"] = rd(P * f).transpose(1, 2) @ dof
        for key in ("dQ", "dK", "dV", "dS"):
            res[key].append(grads[key].double())
        einv = torch.where(has & (delta != 0), torch.exp(-lse2 / aw.LOG2E), torch.zeros_like(l))   # (fasn_bwd_dn: a row with delta = 0 adds 0)
        res["dn"].append(-(delta * einv).sum(-1).double())
    r = {key: torch.stack(val) for key, val in res.items()}
    out = aw.as_result(case, r, dt)
    for key, full in (("dk", r["dK"]), ("dv", r["dV"])):   # (the group's sum is rounded once)
        out[key] = aw._tile(case, aw.group_sum(case, full), "kv").to(dt)
    out["dS_unique"] = r["dS"]   # [ub, uh, L, S]: for a caller whose bias has another shape than as_result knows
    return out
