"""The test of the witness of tests/bias_witness.py, without a GPU.

  (a) the kernels' arithmetic BEFORE the seed floor (attn_emulate.emulate, seeded="inf": a row is unseeded while m_run == -inf) breaks a
      gate by 10x and more: `prefix` at V = 1e9 in every head with n = 0 (the heads with a sink stay inside), `sparse` under split-K at
      V = 1e9 in every head. The witness catches the defect it is named for.
  (b) the arithmetic WITH the floor (seeded="floor", F = F_SEED) stays at or below 0.5 of every gate, in every pattern, bias dtype and
      hiding value; so does the absolute-score model of the kernels that do not seed from a running maximum.
  (c) the rows without a visible real key are at most 1/4 of every case's rows (bias_witness.reference asserts it; here for every case of
      bias_witness.SHAPES, from the patterns alone).
  (d) the reference on these inputs agrees with oracle.ref_attention and autograd to 1e-11 once -V is replaced by a boolean mask.
  (e) the launch plans of bias_witness.SHAPES match tests/golden/bias_witness_plans.txt and each case reaches the family it names.
  (f) a kernel that reads the neighbouring head's bias in the key tiles the hidden prefix touches is caught. (The fully hidden tiles hold
      the same -V in every head; the tile the prefix ends in holds 58 visible keys, and there the mix-up shows.)
F_SEED equals kSeedFloor of csrc/fasn_fwd_kernel.h and respects the cap of rounding point (9); the emulation's lse floor of the backward
equals kLseFloor of csrc/fasn_common.h; the emulated split-K launch has the tiles per split of the launch the GPU case makes.
One deviation from "at or below 0.5 of every gate" in (b): the weak rows' gate on lse bounds a value, not an error (test_b)."""
import math
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_witness as aw   # noqa: E402
import bias_witness as bw   # noqa: E402
from attn_emulate import emulate   # noqa: E402

CPU = torch.device("cpu")
STATE = (1234, 8)   # a dropout (seed, offset)
WEAK_LSE = "weak rows: lse + V"
TPS = 12            # tiles per split of the emulated split-K launch: test_emulated_split_is_the_launchs derives it from the launch plan
CASES = {
    "prefix": bw.BCase(2, 2, 70, 300, 64, bias="hls"),
    "prefix one tile": bw.BCase(2, 2, 70, 300, 64, bias="hls", P=64),
    "prefix std 8": bw.BCase(2, 2, 70, 300, 64, bias="hls", std=8),
    "prefix d128": bw.BCase(2, 2, 70, 300, 128, bias="hls", want=("_ws_",)),
    "prefix causal": bw.BCase(1, 2, 150, 300, 64, bias="hls", causal=True),
    "prefix keypad": bw.BCase(2, 2, 70, 300, 64, bias="hls", mask="keypad", lens=(300, 200)),
    "prefix dense": bw.BCase(2, 2, 70, 300, 64, bias="bhls", mask="dense"),
    "prefix drop": bw.BCase(2, 2, 70, 300, 64, bias="hls", p=0.1),
    "leftpad": bw.BCase(3, 2, 300, 300, 64, bias="b1ls", pattern="leftpad"),
    "sparse": bw.BCase(1, 2, 5, 4090, 64, bias="hls", pattern="sparse"),
    "forced": bw.BCase(2, 2, 70, 300, 64, bias="hls", pattern="forced"),
}


class World:
    """inputs, clean reference and gates of one (case, operand dtype, bias dtype, hiding value)"""

    def __init__(self, name, dtype, bdtype, label):
        self.case, self.dtype, self.dt = CASES[name], dtype, aw.DTYPES[dtype]
        self.inp = bw.inputs(self.case, dtype, bdtype, label, CPU, aw.seed_of(name))
        self.keep, self.p_eff = aw.keep_of(self.case, STATE)
        self.r, self.g = bw.reference(self.case, self.inp, dtype, keep=self.keep, p_eff=self.p_eff, backward=True)

    def result(self, r, dtype=None):
        """what a kernel that computed exactly r would return (attn_witness.as_result), dbias in the shape of the call's bias"""
        res = aw.as_result(self.case, r, dtype or self.dt)
        return self.shaped(res, r["dS"])

    def shaped(self, res, dS):
        shape = self.inp["bias"].shape if self.inp["bias"].dim() == 4 else (1,) + tuple(self.inp["bias"].shape)
        res["dbias"] = bw.reduce_dbias(self.case, aw._tile(self.case, dS), shape).reshape(self.inp["bias"].shape).to(self.inp["bias"].dtype)
        return res

    def emulated(self, **kw):
        res = emulate(self, **kw)
        return self.shaped(res, res.pop("dS_unique"))

    def judge(self, res):
        try:
            return bw.judge(self.case, self.dtype, res, self.r, self.g, self.inp)
        except aw.GateRefused:
            return aw.Ratios(refused=math.inf)


_WORLDS = {}


def world(*key):
    if key not in _WORLDS:
        _WORLDS[key] = World(*key)
    return _WORLDS[key]


def _head_spliced(w, clean, mut, h):
    """the clean result with head h's out, lse and dQ taken from `mut`"""
    res = {key: (val.clone() if torch.is_tensor(val) else val) for key, val in clean.items()}
    for key in ("out", "lse", "dq"):
        res[key][:, h] = mut[key][:, h]
    return res


def _runs(names):
    for name in names:
        case = CASES[name]
        for dt in ("fp16", "bf16"):
            for bd in ("same", "fp32"):
                if bd == "fp32" and (case.p or name not in ("prefix", "leftpad", "prefix d128")):
                    continue   # (an fp32 bias under dropout takes the element loads; elsewhere it changes the start value's fma only)
                labels = ("forced",) if case.pattern == "forced" else bw.VALUES[bw.bias_dtype_name(dt, bd)]
                for lab in labels:
                    yield name, dt, bd, lab


# ---------------------------------------------------------------- (a) the defect is caught
@pytest.mark.parametrize("dtype,bdtype", [("bf16", "same"), ("fp16", "fp32")])
def test_a_stale_seed_is_caught_prefix(dtype, bdtype):
    w = world("prefix", dtype, bdtype, "1e9")
    clean, mut = w.result(w.r), w.emulated(seeded="inf")
    assert w.judge(clean).worst() <= 0.5
    for h in range(w.case.H):
        rat = w.judge(_head_spliced(w, clean, mut, h))
        sink = bool(w.inp["un"][0, h] > 0)
        print(f"(a) prefix 1e9 {dtype} bias {bdtype} head {h} (n {'>' if sink else '='} 0): m_run == -inf as the predicate: {rat}")
        if sink:
            assert rat.worst() <= 0.5, (h, dict(rat))
        else:
            assert max(rat.get("out", 0), rat.get("lse", 0), rat.get("refused", 0)) >= 10, (h, dict(rat))


def test_a_stale_seed_is_caught_sparse_split():
    w = world("sparse", "bf16", "same", "1e9")
    clean, mut = w.result(w.r), w.emulated(seeded="inf", tiles_per_split=TPS)
    for h in range(w.case.H):
        rat = w.judge(_head_spliced(w, clean, mut, h))
        print(f"(a) sparse 1e9 bf16 head {h}, splits of {TPS} tiles: m_run == -inf as the predicate: {rat}")
        assert max(rat.get("out", 0), rat.get("lse", 0), rat.get("refused", 0)) >= 10, (h, dict(rat))


# ---------------------------------------------------------------- (b) the arithmetic with the floor stays inside
@pytest.mark.parametrize("name,dtype,bdtype,label", list(_runs(CASES)))
def test_b_gates_hold_for_the_kernels_arithmetic(name, dtype, bdtype, label):
    w = world(name, dtype, bdtype, label)
    tps = TPS if w.case.pattern == "sparse" else None
    clean = w.judge(w.result(w.r))   # (the reference rounded once)
    assert max([v for k, v in clean.items() if k != WEAK_LSE] + [0.0]) <= 0.5 and clean.get(WEAK_LSE, 0.0) <= 1
    for what, kw in (("seeded, floor", dict(seeded="floor", F=bw.F_SEED, tiles_per_split=tps)), ("absolute scores", dict())):
        rat = w.judge(w.emulated(**kw))
        print(f"(b) {name} {dtype} bias {bdtype} -V {label}: emulated kernel arithmetic ({what}) at {rat} of the gates")
        # the weak rows' gate on lse bounds a VALUE, |lse + V| = |log sum_j exp(scale q.k_j)|, not an error: the fp64 reference itself stands
        # at 0.75 of it in `leftpad`. It has to hold (<= 1); every other gate stays at or below 0.5.
        own = rat.pop(WEAK_LSE, None)
        assert rat.worst() <= 0.5, (what, dict(rat))
        assert own is None or own <= 1, (what, own, clean.get(WEAK_LSE))


# ---------------------------------------------------------------- (c) the weak-gated share
@pytest.mark.parametrize("name", list(bw.SHAPES))
def test_c_rows_without_a_real_key_are_at_most_a_quarter(name):
    case = bw.SHAPES[name]
    hid = bw.hidden_pattern(case).expand(case.ub if case.pattern == "leftpad" else 1, 1, case.L, case.S)
    um = None
    if case.mask == "keypad":
        um = (torch.arange(case.S).view(1, -1) < torch.tensor(case.lens).view(-1, 1)).view(case.ub, 1, 1, case.S)
    w = aw.weights(case, um)[:, :1] > 0
    real = (w & ~hid).any(-1)
    share = (~real).double().mean().item()
    print(f"(c) {name}: {share:.3f} of the rows see no real key")
    assert share <= 0.25
    assert (share > 0) == (case.pattern == "leftpad")
    if case.pattern == "leftpad":
        assert int((~real).sum()) == sum(bw.PADS) == 200 and real.numel() == 900


# ---------------------------------------------------------------- (d) the reference against the suite's oracle and autograd
@pytest.mark.parametrize("name,label", [("prefix", "1e9"), ("prefix", "inf"), ("leftpad", "1e9"), ("sparse", "inf")])
def test_d_reference_agrees_with_the_oracle_and_autograd(name, label):
    from oracle.ref_attention import ref_attention_n
    small = dict(L=40, S=150) if name == "prefix" else (dict(L=300, S=300) if name == "leftpad" else dict(L=5, S=1100))
    case = CASES[name].but(**small)
    inp = bw.inputs(case, "bf16", "same", label, CPU, 41)
    r = aw.reference(case, inp)
    q, k, v, do, un, ubias = aw.unique_operands(case, inp)
    hid = inp["hidden"].expand(-1, -1, case.L, case.S)
    for b in range(case.ub):
        for h in range(case.uh):
            rows = ~inp["allhidden"][b, h]   # (rows with a real key: the boolean mask says the same there)
            mask = ~hid[b if hid.shape[0] > 1 else 0, 0]
            n = un[b, h].clone().requires_grad_()
            ops = [t[b, h].clone().requires_grad_() for t in (q, k, v)]
            plain = torch.where(mask, ubias[b if ubias.shape[0] > 1 else 0, h], torch.zeros(()).double())
            bias = plain.clone().requires_grad_()
            out = ref_attention_n(*ops, softmax_n_param=n if n > 0 else 0.0, scale=inp["scale"], attn_mask=mask, attn_bias=bias)
            (out[rows] * do[b, h][rows]).sum().backward()
            pairs = [("out", out.detach()[rows], r["out"][b, h][rows]), ("dQ", ops[0].grad[rows], r["dQ"][b, h][rows]),
                     ("dbias", (bias.grad * mask)[rows], (r["dS"][b, h] * mask)[rows])]
            if bool(rows.all()) or label == "inf" or bool(n > 0):   # (finite V, n = 0: the pad rows reach dK, dV through their own softmax only in the reference)
                pairs += [("dK", ops[1].grad, r["dK"][b, h]), ("dV", ops[2].grad, r["dV"][b, h])]
            if n > 0 and bool(rows.all()):
                pairs.append(("dn", n.grad, r["dn"][b, h]))
            for what, got, want in pairs:
                assert torch.isfinite(got).all() and torch.isfinite(want).all(), (name, label, b, h, what)
                assert (got - want).abs().max() <= 1e-11 * (1 + want.abs().max()), (name, label, b, h, what)


# ---------------------------------------------------------------- (e) the routes, without a GPU
def test_e_plans_match_the_golden_file(pkg, golden_dir):
    with open(os.path.join(golden_dir, "bias_witness_plans.txt")) as fh:
        assert bw.plans_file_text(pkg) == fh.read(), "the launch plans of bias_witness.SHAPES changed: tests/golden/bias_witness_plans.txt"


@pytest.mark.parametrize("name", list(bw.SHAPES))
def test_e_each_case_reaches_the_family_it_is_named_for(pkg, name):
    case = bw.SHAPES[name]
    for dt in case.dtypes:
        for bd in case.bdtypes:
            if dt == "fp32" and bd == "fp32":
                continue
            text = bw.plan_text(pkg, case, dt, bd)
            fwd = [ln for ln in text.splitlines() if "fasn_fwd_kernel<" in ln or "fasn_fwd_ws256_kernel<" in ln or "fasn_f32_fwd" in ln]
            for prop in case.want:
                assert prop in text, (name, dt, bd, prop, text)
            assert " rc=-" not in text
            if name in bw.CONTROLS:   # the kernels that do not seed from a running maximum
                assert "fasn_fwd_kernel<" not in text or "SEED=0" in text, (name, text)
            elif dt != "fp32":
                assert fwd and "SEED=2" in fwd[0] and "bias" in fwd[0], (name, dt, bd, text)
            if bd == "fp32" and dt != "fp32":
                assert "BF32=1" in fwd[0], (name, dt, "an fp32 bias must reach the BF32 image", text)


# ---------------------------------------------------------------- (f) a mix-up of heads in the prefix's tiles
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_f_bias_of_the_neighbouring_head_in_the_prefix_tiles(dtype):
    w = world("prefix", dtype, "same", "1e4")
    upto = -(-w.case.P // aw.KT) * aw.KT
    ub = w.inp["ubias"].clone()
    ub[..., :upto] = w.inp["ubias"].roll(1, 1)[..., :upto]
    mut = w.result(aw.reference(w.case, w.inp, ubias=ub))
    clean = w.result(w.r)
    for h in range(w.case.H):
        rat = w.judge(_head_spliced(w, clean, mut, h))
        print(f"(f) {dtype} head {h}: the neighbouring head's bias in keys < {upto}: {rat}")
        assert rat["out"] >= 10, (h, dict(rat))


# ---------------------------------------------------------------- the floor
def test_seed_floor_is_the_kernels_and_under_the_cap():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "flash-attention-softmax-n_amd", "csrc", "fasn_fwd_kernel.h")) as fh:
        m = re.search(r"constexpr float kSeedFloor = ([0-9.]+)f;", fh.read())
    assert m and float(m.group(1)) == bw.F_SEED
    assert bw.steps_of(bw.SHAPES["d128 prefix"], "fp16") * 2.0 ** -24 * bw.F_SEED * math.log(2.0) <= 2.0 ** -12
    with open(os.path.join(root, "flash-attention-softmax-n_amd", "csrc", "fasn_common.h")) as fh:
        m = re.search(r"constexpr float kLseFloor = ([0-9.]+)f;", fh.read())
    from attn_emulate import LSE_FLOOR
    assert m and float(m.group(1)) == LSE_FLOOR == 2.0 ** 22


def test_emulated_split_is_the_launchs(pkg):
    """the split-K rule of fasn_api.hip (plan_splitk) applied to the `split sparse` shape gives TPS tiles per split, and the number of
    splits that follows from it is the one in the grid of the launch plan: the emulation of (a) and (b) models the launch the GPU case makes"""
    case = bw.SHAPES["split sparse"]
    base, ntiles = case.B * case.H * -(-case.L // 128), -(-case.S // aw.KT)
    n0 = min(-(-1024 // base), ntiles // 6)
    tps = -(-(-(-ntiles // n0)) // 6) * 6
    nsplit = -(-ntiles // tps)
    line = [ln for ln in bw.plan_text(pkg, case, "bf16", "same").splitlines() if "SPLIT=1" in ln][0]
    assert int(re.search(r"grid=(\d+)", line).group(1)) == base * nsplit, line
    assert tps == TPS
    assert CASES["sparse"].S == case.S and all((t * TPS * aw.KT) % 512 < 472 for t in range(nsplit)), "every split starts on a hidden tile"
