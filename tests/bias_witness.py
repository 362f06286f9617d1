"""attn_bias as an additive mask: a witness for flash_attention_n, forward and backward, where the bias hides keys the way additive float
masks do in the wild - 0 where a key is visible and -1e4, -65504, -1e9, finfo.min or -inf where it is not.

Why. attn_witness draws its biases from N(0, 1); no score there leaves the neighbourhood of 0. A bias of -1e9 does: the vector bias modes
of fasn_fwd_kernel start each tile's score accumulator from fma(bias, log2e, -m_run) (DESIGN 4.1 "Seeded accumulators"), and a row
without a sink - n = 0, or any row of split s > 0 of a split-K launch - whose first tiles hold hidden keys only leaves them with a running
maximum of -1.44e9. Seeded from +1.44e9, where fp32 is spaced 128 apart, the next tile's q.k is rounded away and its keys all weigh 1:
nothing is NaN, nothing is refused, and the row is a plain average of that tile. The kernels therefore keep a row unseeded while its
maximum is at or below -F (kSeedFloor); this module is the test of that, and of every other place a hiding value may go wrong.

Operands are witness C's (attn_witness.inputs_c) at a logit standard deviation of 4 (8 as well in the first case); n has zeros next to
positive entries in every case. On top of the N(0, 1) bias one pattern is written (V is the hiding value, always written as -V):
  prefix   keys j < P get -V: P = 64, exactly one tile, or P = 134, two tiles and a part
  leftpad  the causal-LM form of a left-padded batch: bias [B, 1, L, S], L = S, is_causal = False, -V where j > i or j < pad_b. Rows
           i < pad_b see hidden keys only: the pad rows
  sparse   only keys with j mod 512 >= 472 are visible: whatever tile a split of a split-K launch starts at, it meets hidden tiles first
  forced   +V' on one key t(i) = (37 i + 11) mod S per row, V' = 1e4 (6e4 in fp16): that key decides the row, in a different tile from
           row to row, and the reference itself gives out_i = V[t(i)] within 1e-11
The fp64 reference (attn_witness.attend) reads the bias as the call gets it: rounded to its dtype, then widened exactly. One exception:
finfo.min of bf16 and fp32 overflows to -inf once multiplied by log2e in fp32; such a value is read as -inf (hidden outright).

Expectation. A key at -V (V >= 1e4) or -inf has weight exp(-V - m) = 0 in fp64 wherever the row has a real key or a sink, so the
expectation is the masked softmax_n, and the gates are witness C's per-element gates (attn_witness.judge_c) on out, lse, dQ, dK, dV, dn
and dbias with rounding point (9) of the attn_witness docstring added to eps_ij (attn_witness.seed_eps; steps = D / 16 + 2 MFMAs and
roundings in one score chain, D / 2 + 2 in the fp32 kernels, whose MFMA takes 2 features; F = F_SEED, 0 in the fp32 kernels, which do not seed).

Rows whose visible keys are all at -V (the pad rows of `leftpad`):
  n > 0             the sink takes the row: |out| <= 1e-12 and lse = log n within its gate; gradients under the C gates.
  -inf, n = 0       out, dQ and the row's dbias exactly 0, lse = -inf exactly; the row adds 0 to dK, dV, dn (their C gates hold that).
  finite V, n = 0   the weak-gated rows. (Where lse < -2^22 nats - V = 1e9 - the backward gives the row no weights at all, kLseFloor in
                    csrc/fasn_common.h: fp32 cannot hold such an lse to a nat, and the recomputed P overflowed fp16.) The scores are -V + scale q.k in fp32, where q.k is lost at |x| = 1e9: no relative claim can
                    be made. Gated: every result finite; min_j v_jd <= out_id <= max_j v_jd over the row's keys, up to 2u;
                    |lse + V| <= |scale| max_j |q.k_j| + ln S + 2^-21 V. Their dO is set to 0 (a loss never reads a pad row), so that
                    they add exactly 0 to dK, dV, dn and dbias whatever weights the kernel gave them and every gradient keeps its gate.
Condition (asserted from the reference): rows without a visible real key are at most 1/4 of a case's rows.
dbias at an entry hidden by -inf is exactly 0; at -V it is within its C gate.

What this cannot see: whatever attn_witness's big-grid note says of the period ub x uh; here only the split-K cases have uh < H.

This is a helper module (no test is collected from it). tests/test_biaswitness_cpu.py is the test of these tests;
tests/test_gpu_biaswitness.py runs the kernels."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_witness as aw   # noqa: E402
from attn_witness import _f64, _ratio   # noqa: E402

# the seed floor in log2 units: kSeedFloor of csrc/fasn_fwd_kernel.h (tests/test_biaswitness_cpu.py reads the header and compares).
# A design constant, not a measurement: the cap below bounds it, 512 is the largest power of two under the cap.
F_SEED = 512.0
assert (128 // 16 + 2) * 2.0 ** -24 * F_SEED * math.log(2.0) <= 2.0 ** -12, "the F part of rounding point (9) exceeds 2^-12 nats at D = 128"
HIDDEN_BELOW = -9000.0   # a bias at or below this hides its key (the N(0, 1) part never comes near it)
F32_MAX = torch.finfo(torch.float32).max
PADS = (0, 70, 130)

VALUES = {   # hiding values by bias dtype: label -> V
    "fp16": ("1e4", "65504", "inf"),
    "bf16": ("1e4", "1e9", "fmin", "inf"),
    "fp32": ("1e4", "1e9", "fmin", "inf"),
}


def hiding_value(label, bdt):
    """-V as a python float in the bias dtype's range"""
    if label == "fmin":
        return torch.finfo(bdt).min
    return -{"1e4": 1e4, "65504": 65504.0, "1e9": 1e9, "inf": math.inf}[label]


def values_of(bdtype, every, extra=()):
    """every hiding value of the bias dtype, or the largest finite one and -inf (and those of `extra` the dtype holds)"""
    v = VALUES[bdtype]
    return v if every else tuple(x for x in v if x in v[-2:] or x in extra)


def BCase(*args, pattern="prefix", P=134, bdtypes=("same",), std=4, every=False, rowpad=False, extra=("1e9",), **kw):
    """an attn_witness.Case with the bias pattern. bias kinds: "hls", "bhls" (attn_witness) and "b1ls" ([B, 1, L, S]), "bh1s" ([B, H, 1, S]).
    bdtypes: "same" (the operand type) and / or "fp32". every: run every hiding value of the bias dtype; extra: values run next to the
    largest finite one and -inf (bf16's largest finite value, finfo.min, reads as -inf: a split-K case run at it alone would not meet
    the stale seed it is there for). rowpad: the bias is a view whose
    rows start 16 bytes aligned (row stride S rounded up to 8 elements) - what the vector bias modes, the only ones with a split-K
    instantiation, ask of a bias whose S is no multiple of 8; a contiguous one takes the element loads."""
    c = aw.Case(*args, wit="C", **kw)
    c.pattern, c.P, c.bdtypes, c.std, c.every, c.rowpad, c.extra = pattern, P, tuple(bdtypes), std, every, rowpad, tuple(extra)
    return c


def row_stride(case):
    return -(-case.S // 8) * 8 if case.rowpad else case.S


def bias_dtype_name(dtype, bdtype):
    return dtype if bdtype == "same" else bdtype


def steps_of(case, dtype):
    """roundings in one score chain: the MFMAs (16 features each in v_mfma_f32_32x32x16_{f16,bf16}, 2 each in the fp32 kernels'
    v_mfma_f32_32x32x2_f32) plus two (bias * log2e, the moved maximum)"""
    return case.D // (2 if dtype == "fp32" else 16) + 2


def seed_of_case(case, dtype):
    """(steps, F) of rounding point (9). The fp32 kernels do not seed from a running maximum: F = 0 there, and the term is the fp32
    accumulation of a score of magnitude |x_ij| + |m_i| alone."""
    return steps_of(case, dtype), (0.0 if dtype == "fp32" else F_SEED)


# ---------------------------------------------------------------- inputs
def hidden_pattern(case):
    """bool [ub or 1, 1, L or 1, S] on the CPU: the entries the pattern hides"""
    L, S = case.L, case.S
    j = torch.arange(S).view(1, 1, 1, S)
    if case.pattern == "prefix":
        return j < case.P
    if case.pattern == "sparse":
        return (j % 512) < 472
    if case.pattern == "leftpad":
        assert L == S and case.ub == len(PADS) and not case.causal
        i = torch.arange(L).view(1, 1, L, 1)
        return (j > i) | (j < torch.tensor(PADS).view(-1, 1, 1, 1))
    assert case.pattern == "forced"
    return torch.zeros(1, 1, 1, S, dtype=torch.bool)


def inputs(case, dtype, bdtype, label, dev, seed):
    """witness C's operands with the case's pattern written into the bias. dtype / bdtype: names ("fp16", ...; bdtype also "same");
    label: a key of the hiding values, or "forced". Adds to the dict: hidden (the pattern), ubias_call (what the call's bias holds,
    fp64 [nb, uh, L, S]) next to ubias (what the reference reads: finfo.min that overflows in fp32 read as -inf), and weak / sinkonly /
    empty (bool [ub, uh, L]: the rows without a visible real key, by class; the weak rows' dO is 0)."""
    dt = aw.DTYPES[dtype]
    bdt = aw.DTYPES[bias_dtype_name(dtype, bdtype)]
    ub, uh, L, S = case.ub, case.uh, case.L, case.S
    inp = aw.inputs_c(case.but(bias=None), case.std, dt, dev, seed)
    if case.nshape == "float":   # the decode regroup takes a float n: 0.0, every row without a sink
        inp["n"], inp["un"] = 0.0, torch.zeros(ub, uh, dtype=torch.float64)
    nb = 1 if case.bias == "hls" else ub
    nh = 1 if case.bias == "b1ls" else uh
    t = aw._counter_normal((nb, nh, L, S), seed + 4, 1.0, bdt, dev)
    hid = hidden_pattern(case)
    if case.pattern == "forced":
        vp = 6e4 if bdt == torch.float16 else 1e4
        i = torch.arange(L, device=dev)
        t[:, :, i, (37 * i + 11) % S] = vp
    else:
        t = torch.where(hid.to(dev), torch.full_like(t, hiding_value(label, bdt)), t)
    full = t[:, case.hidx.to(dev)] if nh > 1 else t
    full = full[case.bidx.to(dev)] if nb > 1 else full
    full = (full[0] if case.bias == "hls" else full).contiguous()
    if case.rowpad:
        buf = torch.zeros(*full.shape[:-1], row_stride(case), dtype=bdt, device=dev)
        buf[..., :S] = full
        full = buf[..., :S]
    inp["bias"] = full
    call = _f64(t).expand(nb, uh, L, S)
    inp["ubias_call"] = call
    inp["ubias"] = torch.where(call * aw.LOG2E < -F32_MAX, torch.full_like(call, -math.inf), call)
    inp["hidden"] = hid
    # rows by class, from the visible set and the bias alone
    w = aw.weights(case, inp["um"]).expand(ub, uh, L, S) > 0
    real = (w & (inp["ubias"] > HIDDEN_BELOW)).any(-1)
    cut = (w & torch.isinf(inp["ubias"])).any(-1)   # (a pattern writes one value: a row's hidden keys are all finite or all -inf)
    sink = (inp["un"] > 0).view(ub, uh, 1)
    allhid = ~real & w.any(-1)
    inp["allhidden"] = allhid
    inp["sinkonly"] = allhid & sink
    inp["empty"] = allhid & ~sink & cut
    inp["weak"] = allhid & ~sink & ~cut
    inp["do"] = inp["do"] * (~aw._tile(case, inp["weak"])).to(dev).unsqueeze(-1).to(dt)
    return inp


def reference(case, inp, dtype, keep=None, p_eff=0.0, backward=None, **kw):
    """(r, g): attn_witness.reference and with_bounds with rounding point (9); asserts the conditions the reference decides"""
    backward = case.bwd if backward is None else backward
    r = aw.reference(case, inp, keep=keep, p_eff=p_eff, backward=backward, **kw)
    dt = aw.DTYPES[dtype]
    g = aw.with_bounds(case, inp, r, aw.unit(case, dt), aw.unit_abs(dt), seed=seed_of_case(case, dtype))
    share = inp["allhidden"].double().mean().item()
    assert share <= 0.25, f"rows without a visible real key: {share:.3f} of the case's rows > 1/4"
    if case.pattern == "forced":
        q, k, v, do = r["_ops"]
        tgt = (37 * torch.arange(case.L) + 11) % case.S
        assert (r["out"] - v[:, :, tgt]).abs().max() <= 1e-11, "forced: the reference itself is not the forced key's V row"
    return r, g


# ---------------------------------------------------------------- gates
def _full(case, t):
    return aw._tile(case, t)


def reduce_dbias(case, t, shape):
    """[B, H, L, S] -> the shape of the call's bias (4-dim): summed over the dimensions the bias broadcasts over"""
    for d in (0, 1):
        if shape[d] == 1 and t.shape[d] > 1:
            t = t.sum(d, keepdim=True)
    return t


def judge(case, dtype, res, r, g, inp):
    """every result of the call against the gates of the module docstring: the largest ratio per tensor and row class. A result that a gate
    refuses outright (non-finite values, an lse that is not -inf exactly in the empty rows) raises attn_witness.GateRefused."""
    dt = aw.DTYPES[dtype]
    u = aw.U[dt]
    rat = aw.Ratios()
    bwd = res.get("dq") is not None
    for key in ("out", "dq", "dk", "dv", "dn", "dbias"):
        if res.get(key) is not None:
            aw.finite(res[key])
    weak, sinkonly, empty = (_full(case, inp[key]) for key in ("weak", "sinkonly", "empty"))   # [B, H, L]
    out, lse = _f64(res["out"]), (None if res.get("lse") is None else _f64(res["lse"]))
    # ---- the C gates, with the weak rows' out / lse taken from the reference (they have gates of their own below)
    res_c = dict(res)
    res_c["dbias"] = None
    if weak.any():
        res_c["out"] = torch.where(weak.unsqueeze(-1), _full(case, r["out"]), out)
        if lse is not None:
            res_c["lse"] = torch.where(weak, _full(case, r["lse"]), lse)
    aw.judge_c(case, dt, res_c, r, g, rat)
    # ---- dbias: dS summed over what the bias broadcasts over
    if bwd and res.get("dbias") is not None:
        got = _f64(res["dbias"])
        got = got.unsqueeze(0) if got.dim() == 3 else got
        want = reduce_dbias(case, _full(case, r["dS"]), got.shape)
        gate = reduce_dbias(case, _full(case, g["dS"]), got.shape)
        rat.up("dbias", _ratio((got - want).abs(), gate + u * want.abs() + 1e-6))
        bias_ref = inp["ubias"]
        bias_ref = bias_ref[case.bidx] if bias_ref.shape[0] > 1 else bias_ref
        bias_ref = bias_ref[:, case.hidx]
        if inp["bias"].dim() == 4 and inp["bias"].shape[1] == 1:
            bias_ref = bias_ref[:, :1]
        cut = torch.isinf(bias_ref).expand(got.shape)
        rat.up("dbias at -inf = 0", _ratio(got[cut].abs(), torch.zeros_like(got[cut])))
        if empty.any() and got.shape[0] == case.B and got.shape[1] == case.H:
            rows = got[empty]
            rat.up("empty rows: dbias = 0", _ratio(rows.abs(), torch.zeros_like(rows)))
    # ---- rows the sink alone takes
    if sinkonly.any():
        rows = out[sinkonly]
        rat.up("sink rows: |out| <= 1e-12", _ratio(rows.abs(), torch.full_like(rows, 1e-12)))
    # ---- rows with nothing: exactly 0 (lse = -inf exactly: judge_c's _lse_pair refuses anything else)
    if empty.any():
        rows = out[empty]
        rat.up("empty rows: out = 0", _ratio(rows.abs(), torch.zeros_like(rows)))
        if bwd:
            rows = _f64(res["dq"])[empty]
            rat.up("empty rows: dQ = 0", _ratio(rows.abs(), torch.zeros_like(rows)))
    # ---- the weak-gated rows
    if weak.any():
        q, k, v, do = r["_ops"]
        wvis = (aw.weights(case, inp["um"]).expand(case.ub, case.uh, case.L, case.S) > 0)
        # (the row's keys: every visible key; without a mask or causal limit that is every key of the K/V head)
        assert bool(wvis.all()), "weak-gated rows: a case with a boolean mask or a causal limit needs the per-row key set here"
        lo, hi = _full(case, v.amin(2).unsqueeze(2).expand(-1, -1, case.L, -1)), _full(case, v.amax(2).unsqueeze(2).expand(-1, -1, case.L, -1))
        err = torch.maximum((lo - out).clamp_min(0.0), (out - hi).clamp_min(0.0))[weak]
        span = torch.maximum(lo.abs(), hi.abs())[weak]
        rat.up("weak rows: out within its keys' v", _ratio(err, 2 * u * span))
        if lse is not None:
            xb = r["x"] - inp["ubias"].expand(case.ub, case.uh, case.L, case.S)    # scale q.k of the reference
            V = -inp["ubias"].expand(case.ub, case.uh, case.L, case.S).amax(-1)     # the row's hiding value (all of its keys hold it)
            bound = xb.abs().amax(-1) + math.log(case.S) + 2.0 ** -21 * V
            rat.up("weak rows: lse + V", _ratio((lse - _full(case, -V)).abs()[weak], _full(case, bound)[weak]))
    return rat


# ---------------------------------------------------------------- launch plans without a GPU
def plan_args(pkg, case, dtype, bdtype, backward=True):
    """attn_witness.plan_args with the bias as this module's call hands it over: its shape (strides 0 where it broadcasts), its dtype and
    the reduced gradient flash_attn asks for where the bias broadcasts over batch or heads"""
    Lb = pkg._lib
    a = aw.plan_args(pkg, case.but(bias="hls" if case.bias == "hls" else "bhls"), dtype, backward)
    f = a.fwd
    if case.nshape == "float":
        f.softmax_n = 0.0
    L, S = f.Sq, f.Sk
    small = (backward and case.p == 0.0 and dtype != "fp32" and L > 1 and
             ((case.bias == "hls" and case.B > 1) or (case.bias == "b1ls" and case.H > 1)))
    if case.rowpad:
        assert case.bias == "hls"
        aw._view(f.bias, (0, L * row_stride(case), row_stride(case), 1))
    if case.bias == "b1ls":
        aw._view(f.bias, (L * S, 0, S, 1))
        if small:
            aw._view(a.dbias, (L * S, 0, S, 1))
            a.dbias_dtype = Lb.FASN_BIAS_SAME
    if bdtype == "fp32" and dtype != "fp32":
        f.bias_dtype = Lb.FASN_BIAS_F32
        if small:
            a.dbias_dtype = Lb.FASN_BIAS_F32
    return a


def plan_text(pkg, case, dtype, bdtype):
    """the fasn_launch_plan text of the case: forward (with its workspace) and, where the case runs one, backward"""
    import ctypes
    Lb = pkg._lib
    lib = Lb.load()
    buf = ctypes.create_string_buffer(1 << 14)
    out = []
    for name, which in (("fwd", Lb.FASN_PLAN_FWD_WS), ("bwd", Lb.FASN_PLAN_BWD)):
        if name == "bwd" and not case.bwd:
            continue
        a = plan_args(pkg, case, dtype, bdtype, backward=(name == "bwd"))
        rc = lib.fasn_launch_plan(a, which, buf, len(buf))
        out.append(f"  [{name}] rc={rc} fwd_path={lib.fasn_fwd_path(a.fwd)}" + (f" bwd_path={lib.fasn_bwd_path(a)}" if name == "bwd" else ""))
        out += ["    " + line for line in buf.value.decode().splitlines()]
    return "\n".join(out)


# ---------------------------------------------------------------- the cases: the smallest shapes with four key tiles and two row blocks
SHAPES = {
    "d64 prefix": BCase(2, 4, 70, 300, 64, bias="hls", every=True, want=("D=64,QB=1,bias,", "SEED=2")),
    "d64 prefix std 8": BCase(2, 4, 70, 300, 64, bias="hls", std=8, every=True, want=("D=64,QB=1,bias,", "SEED=2")),
    "d64 prefix one tile": BCase(2, 4, 70, 300, 64, bias="hls", P=64, every=True, want=("D=64,QB=1,bias,", "SEED=2")),
    "d64 prefix fp32 bias": BCase(2, 4, 70, 300, 64, bias="hls", bdtypes=("fp32",), every=True, want=("D=64,QB=1,bias,", "SEED=2", "BF32=1")),
    "d32 prefix": BCase(2, 4, 70, 300, 32, bias="hls", bdtypes=("same", "fp32"), every=True, want=("D=32,", "bias", "SEED=2")),
    "d128 prefix": BCase(2, 4, 70, 300, 128, bias="hls", every=True, want=("D=128,QB=1,bias", "NW=8", "_ws_")),
    "d128 prefix fp32 bias": BCase(2, 4, 70, 300, 128, bias="hls", bdtypes=("fp32",), every=True, want=("D=128,QB=1,bias", "NW=8", "RING=0", "BF32=1")),   # register staging
    "d256 prefix": BCase(2, 4, 70, 300, 256, bias="hls", want=("_ws256_",)),                                       # control: no seed from m_run
    "d128 prefix keypad ragged": BCase(3, 4, 70, 300, 128, bias="hls", mask="keypad", lens=(300, 200, 140), want=("bias+keypad", "_ws_")),
    "d64 prefix dense mask": BCase(2, 4, 70, 300, 64, bias="bhls", mask="dense", want=("D=64,QB=1,bias+mask",)),
    "d64 prefix causal": BCase(2, 4, 150, 300, 64, bias="hls", causal=True, want=("D=64,QB=1,bias",)),           # S - L >= P
    "d64 leftpad": BCase(3, 4, 300, 300, 64, bias="b1ls", pattern="leftpad", bdtypes=("same", "fp32"), every=True, want=("D=64,QB=1,bias",)),
    "d64 prefix dropout": BCase(2, 4, 70, 300, 64, bias="hls", p=0.1, want=("DROP=1",)),
    "split sparse": BCase(1, 16, 5, 4090, 64, bias="hls", uh=2, pattern="sparse", rowpad=True, want=("SPLIT=1", "fasn_fwd_combine_kernel", "bias")),
    "split sparse d128": BCase(1, 16, 130, 4090, 128, bias="hls", uh=2, pattern="sparse", rowpad=True, bwd=False, want=("D=128", "SPLIT=1", "fasn_fwd_combine_kernel", "bias")),
    "decode regroup": BCase(2, 8, 1, 420, 64, Hkv=2, bias="bh1s", nshape="float", bwd=False, want=("D=64,QB=1,bias",)),
    "element loads": BCase(2, 4, 70, 301, 64, bias="hls", want=("element-load",)),                                # control
    "fp32 operands": BCase(2, 2, 70, 200, 32, bias="hls", dtypes=("fp32",), want=("fasn_f32_",)),                # control
    "d64 forced": BCase(2, 4, 70, 300, 64, bias="hls", pattern="forced", want=("D=64,QB=1,bias,", "SEED=2")),
}
CONTROLS = ("d256 prefix", "element loads", "fp32 operands")   # kernels that do not seed from a running maximum


def params():
    """(name, dtype, bdtype, label) of every run"""
    for name, c in SHAPES.items():
        for dt in c.dtypes:
            for bd in c.bdtypes:
                if dt == "fp32" and bd == "fp32":
                    continue
                labels = ("forced",) if c.pattern == "forced" else values_of(bias_dtype_name(dt, bd), c.every, c.extra)
                for lab in labels:
                    yield name, dt, bd, lab


def plans_file_text(pkg):
    out = []
    for name, case in SHAPES.items():
        for dt in case.dtypes:
            for bd in case.bdtypes:
                if dt == "fp32" and bd == "fp32":
                    continue
                out.append(f"{name} [{dt}, bias {bias_dtype_name(dt, bd)}]")
                out.append(plan_text(pkg, case, dt, bd))
    return "\n".join(out) + "\n"
