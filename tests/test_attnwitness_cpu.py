"""The test of the witnesses of tests/attn_witness.py, without a GPU: on the fp64 reference alone.

The reference is mutated the way attention kernels go wrong and the mutated result, rounded to the output type, is put through the
witness's gates as if a kernel had returned it - once per (batch, head) and row block of 128 rows the fault touches, with every other
slice left clean, so that the gate must break in EVERY slice and not in one lucky one. Threshold: 4x for witness A's integer gates (one
count is four gates of 0.25 by construction; the exp(lse) gate catches a count at 10x and more), 10x everywhere else.

Which witness is claimed to catch which mutant (dtype in brackets where only one is claimed):

  mutant                                                        caught by
  1  causal edge + 1 key (L < S and L > S)                      A: exp(lse);  B ladder ascending: out;  backward: A dV [fp16]
     causal edge - 1 key                                        A: exp(lse), out Z;  B ladder, B code: out, dV (the winner is hidden)
  2  a 64-key tile dropped / counted twice                      A: exp(lse), out Z;  backward (tile dropped in dK/dV only): A dV Z
     the partial last tile treated as full                      A: exp(lse)
  3  a row block served with its pair partner's / its           A: exp(lse);  B ladder ascending: out
     neighbour's keys (causal)
  4  a query head reading the neighbouring K/V head             A: out Z (the spare class carries the K/V head);  B code, C: out
     dK / dV missing one query head of the group                A: dV Z;  B code: dV [fp16]
  5  split-K merged with equal weights                          B ladder: out;  C: out, lse   (not A: with q = 0 the right weights are 1)
     the sink counted in every split / in none                  A: exp(lse)
  6  one keep bit flipped; the keep bits of the neighbouring    A: out Z (forward), dV Z (backward)
     row; of the neighbouring 16-key group
  7  lse without n read by the backward                         A: dV Z;  B code_sink: dV
     delta from the undropped output; delta = 0                 C: dQ [fp16];  delta = 0 also B code: dQ, dK
  8  dK / dV missing one row block / counting one twice         A: dV Z;  B code: dV
  9  dn summed without one row chunk                            A: dn
  10 key-padding word of the neighbouring tile / of the         A: exp(lse), out Z
     other (length-paired) batch element
  11 bias of the neighbouring head                              C: out [fp16]

Mutants 2, 4, 6 and 10 are shown caught again on cases of attn_witness.NEW, cut down to their distinct problems (distinct()): the
key-padding words on "d128 keypad", the keep bits on "d128 drop" (one-wave backward, grouped) and "d128 drop two-wave", the tiles on
"d64 8-wave dense mask", the K/V head map on "d32 gqa". Every 16-bit case of NEW passes the emulation bound below at both logit standard
deviations; every fp32 case passes it with an fp32 evaluation in tile order (witness C in fp32); witness A's class-count condition and
the rounded reference's pass through every gate are asserted for each case of NEW from the reference alone.

The unmutated reference, rounded to the output type, passes every gate; an emulation of the kernels' arithmetic with the rounding
points (1) to (8) of the derivation (attn_witness docstring; tests/attn_emulate.py in its absolute-score model - the seed, rounding point
(9), is the business of tests/test_biaswitness_cpu.py) stays at or below 0.5 of every gate of witness C; the fp64 reference and its closed-form
gradients agree with oracle.ref_attention.ref_attention_n and autograd on the suite's ordinary data; and the launch plans of every case of
attn_witness.SHAPES match tests/golden/attn_witness_plans.txt and have the property the case is named for."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_witness as aw   # noqa: E402

CPU = torch.device("cpu")
Case = aw.Case
RB = 128   # rows per slice the mutants are judged in
CASES = {
    "plain": Case(1, 2, 200, 420, 64),                                   # Z = 512 in the head with a sink
    "causal L<S": Case(1, 2, 200, 420, 64, causal=True),
    "causal L>S": Case(1, 2, 300, 200, 64, causal=True),
    "gqa": Case(1, 4, 200, 420, 64, Hkv=2),
    "keypad": Case(2, 2, 200, 420, 64, mask="keypad", lens=[420, 100], nshape="BH"),
    "drop": Case(1, 2, 200, 420, 64, p=0.1),
    "bias": Case(2, 2, 200, 420, 64, bias="hls"),
    "long": Case(1, 2, 5, 4000, 64),
}
STATE = (1234, 8)   # a dropout (seed, offset)


def unit(case, dtype):
    return aw.unit(case, aw.DTYPES[dtype])


class World:
    """inputs, keep mask, clean reference and gates of one (case, witness, dtype)"""

    def __init__(self, case, wit, dtype, form=None, std=None):
        self.case, self.wit, self.dtype, self.dt, self.form = case, wit, dtype, aw.DTYPES[dtype], form
        self.u = unit(case, dtype)
        seed = aw.seed_of(f"{wit}{form}{std}")
        if wit == "A":
            self.inp = aw.inputs_a(case, self.dt, CPU, seed)
        elif wit == "B":
            self.inp = aw.inputs_b(case, form, self.dt, CPU, seed)
        else:
            self.inp = aw.inputs_c(case, std, self.dt, CPU, seed)
        self.keep, self.p_eff = aw.keep_of(case, STATE)
        self.bwd = not (wit == "B" and not form.startswith("code"))
        self.r = self.ref()
        self.g = aw.with_bounds(case, self.inp, self.r, self.u, aw.unit_abs(self.dt))
        self.clean = aw.as_result(case, self.r, self.dt)
        self.clean64 = aw.as_result(case, self.r, torch.float64)

    def ref(self, **kw):
        kw.setdefault("keep", self.keep)
        return aw.reference(self.case, self.inp, p_eff=self.p_eff, backward=self.bwd, **kw)

    def judge(self, res):
        try:
            if self.wit == "A":
                return aw.judge_a(self.case, self.dt, res, self.r, self.g, self.p_eff)
            if self.wit == "B":
                return aw.judge_b(self.case, self.form, self.dt, res, self.r, self.g, self.inp)[0]
            return aw.judge_c(self.case, self.dt, res, self.r, self.g)
        except aw.GateRefused:   # (a gate that refuses outright: lse of an empty row, non-finite values)
            return aw.Ratios(refused=math.inf)


_WORLDS = {}


def distinct(case):
    """a case of attn_witness.SHAPES cut down to its ub x uh distinct problems (2 x 2 of them where it has more than 64): the reference, the
    gates and the kernels' arithmetic are those of one (batch, head) problem and know nothing of the grid the problems are tiled over"""
    if case.ub * case.uh > 64:
        assert case.G == 1 and case.lens is None
        return case.but(B=2, H=2, Hkv=2, ub=2, uh=2)
    return case.but(B=case.ub, H=case.uh, Hkv=case.uhk)


def world(case_name, wit, dtype, form=None, std=None):
    """case_name: one of CASES, or one of attn_witness.SHAPES (its distinct problems)"""
    key = (case_name, wit, dtype, form, std)
    if key not in _WORLDS:
        _WORLDS[key] = World(CASES[case_name] if case_name in CASES else distinct(aw.SHAPES[case_name]), wit, dtype, form, std)
    return _WORLDS[key]


def _spliced(w, clean, mut, b, h, rows, fwd=True, kv=True):
    """the clean result with the slice (b, h, rows) of out, lse, dQ and the K/V head of h in dK, dV taken from `mut`"""
    res = {key: (val.clone() if torch.is_tensor(val) else val) for key, val in clean.items()}
    keys = (("out", "lse") if fwd else ()) + (("dq",) if w.bwd else ())
    for key in keys:
        res[key][b, h, rows] = mut[key][b, h, rows]
    if w.bwd and kv:
        hk = h // w.case.G
        res["dk"][b, hk], res["dv"][b, hk] = mut["dk"][b, hk], mut["dv"][b, hk]
    return res


def assert_caught(w, mut_r, keys, thr, what, fwd=True, kv=True, whole=False, exact=False):
    """every slice in which the mutated result differs from the clean one breaks one of the gates `keys` by `thr`. exact: the mutated
    result is not rounded to the output type (witness A's integer gates: one count is four gates; rounded, up to 0.2 of a count less).

    "Four" holds to the last few ulps of fp64 only. The reference's sums are exact in any order (attend() applies the dropout factor after
    them), but the gate reads the count back as out * Z * (1 - p_eff) from out = (count / (1 - p_eff)) / Z: four correctly rounded
    operations with a factor 1 - p_eff that is no power of two, 3.999999999999998 where one count was flipped. These roundings are the same
    on every host; an allowance of 1e-12 relative on the threshold covers them, a thousand times their size and 1e-12 of one count."""
    if exact:
        thr = thr * (1 - 1e-12)
    case = w.case
    clean = w.clean64 if exact else w.clean
    mut = aw.as_result(case, mut_r, torch.float64 if exact else w.dt) if "_ops" in mut_r else mut_r   # (a reference() result, or one in run()'s layout)
    if whole:
        rat = w.judge(mut)
        best = max(rat.get(k, 0.0) for k in tuple(keys) + ("refused",))
        print(f"{what}: {rat}")
        assert best >= thr, (what, dict(rat))
        return
    touched, worst = 0, math.inf
    for b in range(case.B):
        for h in range(case.H):
            hk = h // case.G
            for r0 in range(0, case.L, RB):
                rows = slice(r0, min(r0 + RB, case.L))
                differs = any(not torch.equal(mut[k][b, h, rows], clean[k][b, h, rows]) for k in (("out", "lse") if fwd else ()) + (("dq",) if w.bwd else ()))
                if w.bwd and kv and r0 == 0:
                    differs |= not (torch.equal(mut["dk"][b, hk], clean["dk"][b, hk]) and torch.equal(mut["dv"][b, hk], clean["dv"][b, hk]))
                if not differs:
                    continue
                touched += 1
                rat = w.judge(_spliced(w, clean, mut, b, h, rows, fwd, kv))
                best = max(rat.get(k, 0.0) for k in tuple(keys) + ("refused",))
                worst = min(worst, best)
                assert best >= thr, (what, b, h, r0, dict(rat))
    assert touched, f"{what}: the mutant changes nothing"
    print(f"{what}: {touched} slices touched, the weakest breaks {' / '.join(keys)} by {worst:.3g}x")


# ---------------------------------------------------------------- the unmutated reference passes
UNMUTATED = [("plain", "A", None, None), ("causal L>S", "A", None, None), ("gqa", "A", None, None), ("keypad", "A", None, None),
             ("drop", "A", None, None), ("bias", "A", None, None),
             *[(c, "B", f, None) for c in ("plain", "causal L>S", "keypad", "drop", "bias", "gqa") for f in aw.B_FORMS],
             *[(c, "C", None, s) for c in ("plain", "causal L>S", "keypad", "drop", "bias", "gqa") for s in (4, 8)]]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case_name,wit,form,std", UNMUTATED)
def test_unmutated_reference_passes(case_name, wit, form, std, dtype):
    w = world(case_name, wit, dtype, form, std)
    if wit == "A":
        aw.condition_a(w.case, w.r, w.dt, w.p_eff)
        count = w.r["l"] - w.r["_un"].unsqueeze(-1)
        assert torch.equal(count, count.round()), "the visible keys are counted in integers"
        if not w.case.p:
            assert torch.equal(w.r["acc"][..., :w.case.D // 2].sum(-1), count), "every visible key is in exactly one class of the first half"
    if wit == "C":
        x = w.r["x"]
        got = x[torch.isfinite(x)].std().item()
        want = math.hypot(std, 1.0) if w.case.bias else std
        assert 0.85 * want <= got <= 1.15 * want, f"logit standard deviation {got}"
    rat = w.judge(w.clean)
    print(f"{case_name} {wit} {form or std or ''} {dtype}: rounded reference at {rat}")
    # the integer gate on dV Z runs wherever Z is a power of two: in fp16 always; in bf16 where a count's own rounding stays under 0.2
    # (not under dropout, 2 u per count, nor over a group of 4 heads) - there the mutants below are caught by the per-element gate on dV
    if wit == "A" and aw.pow2_n(w.case) is not None and (dtype == "fp16" or (w.case.G == 1 and not w.case.p)):
        assert "dV Z" in rat, (case_name, dtype)
    assert "refused" not in rat
    lim = {"A": 0.8 + 1e-9, "B": 1.0, "C": 0.5}[wit]   # A: the result's own rounding stays under 0.2 of 0.25 ... 0.8 of the gate
    assert rat.worst() <= lim, dict(rat)
    if wit == "B":
        kinds = aw.judge_b(w.case, form, w.dt, w.clean, w.r, w.g, w.inp)[1]
        assert 1 in kinds or form == "code_sink"
        assert 2 in kinds or "sink" not in form


def test_b_gap_and_prescale():
    """the bounded code wins every row by at least 30 nats at |logit| <= 193 after ONE rounding of the prescaled operand, in both operand
    types; the ladder's prescaled operand rounds with the same relative error in every feature, so its order and gaps survive"""
    case = CASES["causal L<S"]
    for dtype in ("fp16", "bf16"):
        dt = aw.DTYPES[dtype]
        inp = aw.inputs_b(case, "code", dt, CPU, 3)
        c = inp["scale"] * aw.LOG2E
        q, k = aw._f64(inp["q"][0, 0]), aw._f64(inp["k"][0, 0])
        x = ((q * c).to(dt).double() @ k.T) / aw.LOG2E          # the logits the kernels see, in nats
        vis = aw.visible_set(case.L, case.S, True) > 0
        x = torch.where(vis, x, torch.full_like(x, -math.inf))
        top, win = x.max(-1)
        second = x.scatter(1, win.unsqueeze(1), -math.inf).amax(-1)
        assert torch.equal(win, torch.arange(case.L) + case.S - case.L), "the last causally visible key wins"
        assert (top - second).min() >= 30 and x[vis].abs().max() <= 193, ((top - second).min(), x[vis].abs().max())
        assert len(set(win.tolist())) == case.L, "t is injective"
        for form in ("ascending", "descending"):
            inp = aw.inputs_b(case, form, dt, CPU, 3)
            q1 = aw._f64(inp["q"][0, 0, 0])
            pre = (q1 * inp["scale"] * aw.LOG2E).to(dt).double()
            nz = q1 != 0
            rel = pre[nz] / q1[nz]
            assert (rel == rel[0]).all(), "one relative rounding error in every feature"
            assert dt != torch.float16 or (pre.abs().max() < 65504 and inp["scale"] * aw.LOG2E <= 8)


# ---------------------------------------------------------------- the mutants
def _causal_w(case, delta):
    return aw.visible_set(case.L, case.S, False).tril(case.S - case.L + delta).view(1, 1, case.L, case.S).expand(case.ub, 1, -1, -1)


@pytest.mark.parametrize("delta", [1, -1])
@pytest.mark.parametrize("case_name", ["causal L<S", "causal L>S"])
def test_1_causal_edge(case_name, delta):
    for dtype in ("fp16", "bf16"):
        w = world(case_name, "A", dtype)
        mut = w.ref(w=_causal_w(w.case, delta))
        assert_caught(w, mut, ("exp(lse)",), 10, f"1 A {case_name} edge {delta:+d} {dtype} exp(lse)", kv=False)
        if delta < 0:   # (one key too many also raises Z: out Z_ref moves by (Z - c) / (Z + 1) of a count, just under four gates)
            assert_caught(w, mut, ("out Z",), 4, f"1 A {case_name} edge {delta:+d} {dtype} out Z", kv=False, exact=True)
        w = world(case_name, "B", dtype, "ascending")
        assert_caught(w, w.ref(w=_causal_w(w.case, delta)), ("out",), 10, f"1 B ladder {case_name} edge {delta:+d} {dtype}")
        if delta < 0:
            w = world(case_name, "B", dtype, "code")
            mut = w.ref(w=_causal_w(w.case, delta))
            assert_caught(w, mut, ("out",), 10, f"1 B code {case_name} edge {delta:+d} {dtype} out", kv=False)
            assert_caught(w, mut, ("dV",), 10, f"1 B code {case_name} edge {delta:+d} {dtype} dV (backward only)", fwd=False)
    w = world(case_name, "A", "fp16")
    assert_caught(w, w.ref(w=_causal_w(w.case, delta)), ("dV",), 10, f"1 A {case_name} edge {delta:+d} fp16 dV (backward only)", fwd=False)


def _tile_w(case, um, factor, t=3):
    w = aw.weights(case, um).clone()
    w[..., t * aw.KT:(t + 1) * aw.KT] *= factor
    return w


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_2_tiles(dtype):
    for case_name in ("plain", "causal L<S"):
        w = world(case_name, "A", dtype)
        for factor, what in ((0.0, "dropped"), (2.0, "counted twice")):
            mut = w.ref(w=_tile_w(w.case, w.inp["um"], factor))
            assert_caught(w, mut, ("exp(lse)",), 10, f"2 A {case_name} tile {what} {dtype} exp(lse)", kv=False)
            assert_caught(w, mut, ("out Z",), 4, f"2 A {case_name} tile {what} {dtype} out Z", kv=False, exact=True)
            if case_name == "plain":
                assert_caught(w, mut, ("dV Z", "dV"), 4, f"2 A tile {what} {dtype} in the backward only", fwd=False, exact=True)
        # the partial last tile treated as full: 64 - S % 64 phantom keys of logit 0 and value 0
        pad = aw.KT - w.case.S % aw.KT
        mut = w.ref(un=w.inp["un"] + pad)
        assert_caught(w, mut, ("exp(lse)",), 10, f"2 A {case_name} last tile full {dtype}", kv=False)


def _rowblock_w(case, um, partner):
    w = aw.weights(case, um).clone()
    src = w.clone()
    nblk = -(-case.L // RB)
    for r in range(nblk):
        o = nblk - 1 - r if partner else (r + 1) % nblk
        rows = min(RB, case.L - r * RB, case.L - o * RB)
        w[..., r * RB:r * RB + rows, :] = src[..., o * RB:o * RB + rows, :]
    return w


@pytest.mark.parametrize("partner", [True, False])
def test_3_row_block_with_another_blocks_keys(partner):
    for dtype in ("fp16", "bf16"):
        for wit, form, keys, thr in (("A", None, ("exp(lse)",), 10), ("B", "ascending", ("out",), 10)):
            w = world("causal L>S", wit, dtype, form)
            mut = w.ref(w=_rowblock_w(w.case, w.inp["um"], partner))
            assert_caught(w, mut, keys, thr, f"3 {wit} row block with its {'partner' if partner else 'neighbour'}'s keys {dtype}", kv=False)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_4_kv_heads(dtype):
    for wit, form, std, keys, thr in (("A", None, None, ("out Z",), 4), ("B", "code", None, ("out",), 10), ("C", None, 4, ("out",), 10)):
        w = world("gqa", wit, dtype, form, std)
        assert_caught(w, w.ref(swap_kv=True), keys, thr, f"4 {wit} neighbouring K/V head {dtype}", kv=False)
    for wit, form, keys, thr in (("A", None, ("dV Z", "dV"), 4), ("B", "code", ("dV",), 10)):
        if wit == "B" and dtype == "bf16":   # (2 u sum |dO| over the group's heads leaves one head's dO at 5x in bf16)
            continue
        w = world("gqa", wit, dtype, form)
        mut = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in w.clean.items()}
        for key, full in (("dk", w.r["dK"]), ("dv", w.r["dV"])):
            less = aw.group_sum(w.case, full) - full[:, ::w.case.G]        # without the first query head of each group
            mut[key] = aw._tile(w.case, less, "kv").to(w.dt)
        assert_caught(w, mut, keys, thr, f"4 {wit} dK / dV without one query head {dtype}", fwd=False)


def _merged(w, nsplit, equal):
    """the reference cut into tile-aligned key ranges (the sink on range 0) and merged with e^(m_s - m*) or, the fault, with 1"""
    case = w.case
    wt = aw.weights(case, w.inp["um"])
    tiles = -(-case.S // aw.KT)
    tps = -(-tiles // nsplit)
    parts = []
    for s in range(nsplit):
        ws = torch.zeros_like(wt).expand(case.ub, wt.shape[1], -1, -1).clone()
        lo, hi = min(s * tps * aw.KT, case.S), min((s + 1) * tps * aw.KT, case.S)
        ws[..., lo:hi] = wt[..., lo:hi]
        parts.append(w.ref(w=ws, un=w.inp["un"] if s == 0 else torch.zeros_like(w.inp["un"])))
    m = torch.stack([p["m"] for p in parts]).amax(0)
    cs = [torch.ones_like(m) if equal else torch.exp(p["m"] - m) for p in parts]
    l = sum(p["l"] * c for p, c in zip(parts, cs))
    acc = sum(p["acc"] * c.unsqueeze(-1) for p, c in zip(parts, cs))
    safe = torch.where(l > 0, l, torch.ones_like(l))
    r = dict(w.r)
    r.update(out=acc / safe.unsqueeze(-1), lse=torch.where(l > 0, m + torch.log(safe), torch.full_like(m, -math.inf)))
    return r


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_5_split_k(dtype):
    for wit, form, std, keys in (("B", "ascending", None, ("out",)), ("C", None, 4, ("out", "lse")), ("C", None, 8, ("out", "lse"))):
        w = world("long", wit, dtype, form, std)
        good = aw.as_result(w.case, _merged(w, 4, False), w.dt, backward=False)
        assert w.judge({**w.clean, "out": good["out"], "lse": good["lse"]}).worst() <= 1.0, "the right merge passes"
        bad = aw.as_result(w.case, _merged(w, 4, True), w.dt, backward=False)
        assert_caught(w, {**w.clean, "out": bad["out"], "lse": bad["lse"]}, keys, 10, f"5 {wit} {form or std} equal-weight merge {dtype}", kv=False)
    if dtype == "fp16":
        w = world("long", "A", dtype)
        for k, what in ((4.0, "in every split"), (0.0, "in none")):
            mut = aw.as_result(w.case, w.ref(un=w.inp["un"] * k), w.dt)
            assert (w.inp["un"][0] > 0).any()
            assert_caught(w, {**w.clean, "out": mut["out"], "lse": mut["lse"]}, ("exp(lse)",), 10, f"5 A the sink counted {what}", kv=False)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_6_keep_bits(dtype):
    w = world("drop", "A", dtype)
    flip = w.keep.clone()
    flip[:, :, 7::RB, 100] = 1 - flip[:, :, 7::RB, 100]      # one bit in every row block of every (batch, head)
    for keep, what in ((flip, "one keep bit flipped"), (w.keep.roll(1, 2), "keep bits of the neighbouring row"),
                       (w.keep.roll(16, 3), "keep bits of the neighbouring 16-key group")):
        mut = w.ref(keep=keep)
        assert_caught(w, mut, ("out Z",), 4, f"6 A {what} {dtype} in the forward", kv=False, exact=True)
        assert_caught(w, mut, ("dV Z", "dV"), 4, f"6 A {what} {dtype} in the backward only", fwd=False, exact=True)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_7_lse_and_delta(dtype):
    for case_name, wit, form, std, keys, thr in (("plain", "A", None, None, ("dV Z", "dV"), 4), ("plain", "B", "code_sink", None, ("dV",), 10)):
        w = world(case_name, wit, dtype, form, std)
        mut = w.ref(un=torch.zeros_like(w.inp["un"]))     # lse = log sum_j e^x_j: without n
        assert (w.inp["un"] > 0).any()
        assert_caught(w, mut, keys, thr, f"7 {wit} {form or std or ''} the backward reads an lse without n {dtype}", fwd=False, exact=(wit == "A"))
    w = world("plain", "B", dtype, "code")
    assert_caught(w, w.ref(delta_mode="zero"), ("dQ", "dK"), 10, f"7 B code delta = 0 {dtype}", fwd=False)
    if dtype == "fp16":
        w = world("drop", "C", dtype, None, 4)
        for mode in ("zero", "undropped"):
            assert_caught(w, w.ref(delta_mode=mode), ("dQ",), 10, f"7 C delta {mode} {dtype}", fwd=False, kv=False)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_8_row_blocks_of_dk_dv(dtype):
    for wit, form, keys, thr in (("A", None, ("dV Z", "dV"), 4), ("B", "code", ("dV",), 10)):
        w = world("plain", wit, dtype, form)
        for count, what in ((0.0, "missing"), (2.0, "counted twice")):
            rw = torch.ones(w.case.ub, w.case.uh, w.case.L, dtype=torch.float64)
            rw[:, :, RB:2 * RB] = count
            assert_caught(w, w.ref(row_w=rw), keys, thr, f"8 {wit} dK / dV with a row block {what} {dtype}", fwd=False)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_9_dn_row_chunk(dtype):
    for wit, std in (("A", None),):
        w = world("plain", wit, dtype, None, std)
        part = -(w.r["delta"] * w.r["einv"])[:, :, RB:].sum(-1)
        mut = dict(w.clean)
        mut["dn"] = aw.reduce_n(w.case, part).float()
        assert_caught(w, mut, ("dn",), 10, f"9 {wit} {std or ''} dn without its first row chunk {dtype}", whole=True)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_10_key_padding_words(dtype):
    w = world("keypad", "A", dtype)
    wt = aw.weights(w.case, w.inp["um"])
    shifted = torch.cat([wt[..., aw.KT:], torch.zeros_like(wt[..., :aw.KT])], -1)      # tile t reads the word of tile t + 1
    other = wt.flip(0)                                                                      # the length-paired partner's words
    for wm, what in ((shifted, "of the neighbouring tile"), (other, "of the other batch element")):
        mut = w.ref(w=wm)
        assert_caught(w, mut, ("exp(lse)",), 10, f"10 A visibility words {what} {dtype} exp(lse)", kv=False)
        assert_caught(w, mut, ("out Z",), 4, f"10 A visibility words {what} {dtype} out Z", kv=False, exact=True)


def test_11_bias_of_the_neighbouring_head():
    for std in (4, 8):
        w = world("bias", "C", "fp16", None, std)
        assert_caught(w, w.ref(ubias=w.inp["ubias"].roll(1, 1)), ("out",), 10, f"11 C std {std} bias of the neighbouring head fp16", kv=False)


# ---------------------------------------------------------------- the same mutants on the instantiations of attn_witness.NEW
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_new_key_padding_words_d128(dtype):
    """mutant 10 on "d128 keypad" (four lengths: 420, 300, 64, 5)"""
    w = world("d128 keypad", "A", dtype)
    wt = aw.weights(w.case, w.inp["um"])
    shifted = torch.cat([wt[..., aw.KT:], torch.zeros_like(wt[..., :aw.KT])], -1)
    for wm, what in ((shifted, "of the neighbouring tile"), (wt.flip(0), "of the length-paired batch element")):
        mut = w.ref(w=wm)
        assert_caught(w, mut, ("exp(lse)",), 10, f"10 A d128 keypad: visibility words {what} {dtype} exp(lse)", kv=False)
        assert_caught(w, mut, ("out Z",), 4, f"10 A d128 keypad: visibility words {what} {dtype} out Z", kv=False, exact=True)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case_name", ["d128 drop", "d128 drop two-wave"])
def test_new_keep_bits_d128(case_name, dtype):
    """mutant 6 on the D = 128 dropout cases: the one-wave kernels' (grouped K/V) and the two-wave kernels'. The backward's integer gate
    on dV Z runs in fp16, and in bf16 with one query head per K/V head (test_unmutated_reference_passes says why): claimed there"""
    w = world(case_name, "A", dtype)
    flip = w.keep.clone()
    flip[:, :, 7::RB, 100] = 1 - flip[:, :, 7::RB, 100]
    for keep, what in ((flip, "one keep bit flipped"), (w.keep.roll(1, 2), "keep bits of the neighbouring row"),
                       (w.keep.roll(16, 3), "keep bits of the neighbouring 16-key group")):
        mut = w.ref(keep=keep)
        assert_caught(w, mut, ("out Z",), 4, f"6 A {case_name}: {what} {dtype} in the forward", kv=False, exact=True)
        if dtype == "fp16":
            assert_caught(w, mut, ("dV Z", "dV"), 4, f"6 A {case_name}: {what} {dtype} in the backward only", fwd=False, exact=True)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_new_tiles_d64_8wave(dtype):
    """mutant 2 on "d64 8-wave dense mask" (forward only: a tile dropped, counted twice, the partial last tile taken as full)"""
    w = world("d64 8-wave dense mask", "A", dtype)
    for factor, what in ((0.0, "dropped"), (2.0, "counted twice")):
        mut = w.ref(w=_tile_w(w.case, w.inp["um"], factor))
        assert_caught(w, mut, ("exp(lse)",), 10, f"2 A d64 8-wave dense mask: tile {what} {dtype} exp(lse)", kv=False)
        assert_caught(w, mut, ("out Z",), 4, f"2 A d64 8-wave dense mask: tile {what} {dtype} out Z", kv=False, exact=True)
    mut = w.ref(un=w.inp["un"] + (aw.KT - w.case.S % aw.KT))
    assert_caught(w, mut, ("exp(lse)",), 10, f"2 A d64 8-wave dense mask: last tile full {dtype}", kv=False)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_new_kv_heads_d32(dtype):
    """mutant 4 on "d32 gqa": the forward's K/V head map, and dK / dV without one query head of the group"""
    for wit, form, std, keys, thr in (("A", None, None, ("out Z",), 4), ("B", "code", None, ("out",), 10), ("C", None, 4, ("out",), 10)):
        w = world("d32 gqa", wit, dtype, form, std)
        assert_caught(w, w.ref(swap_kv=True), keys, thr, f"4 {wit} d32 gqa: neighbouring K/V head {dtype}", kv=False)
    if dtype == "fp16":
        w = world("d32 gqa", "A", dtype)
        mut = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in w.clean.items()}
        for key, full in (("dk", w.r["dK"]), ("dv", w.r["dV"])):
            mut[key] = aw._tile(w.case, aw.group_sum(w.case, full) - full[:, ::w.case.G], "kv").to(w.dt)
        assert_caught(w, mut, ("dV Z", "dV"), 4, f"4 A d32 gqa: dK / dV without one query head {dtype}", fwd=False)


# ---------------------------------------------------------------- witness C's derivation: the kernels' arithmetic stays inside it
from attn_emulate import emulate as _emulate   # noqa: E402  (shared with tests/test_biaswitness_cpu.py; here: the absolute-score model)


@pytest.mark.parametrize("std", [4, 8])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case_name", ["plain", "causal L>S", "gqa", "keypad", "drop", "bias"])
def test_c_gates_hold_for_the_kernels_arithmetic(case_name, dtype, std):
    w = world(case_name, "C", dtype, None, std)
    rat = aw.judge_c(w.case, w.dt, _emulate(w), w.r, w.g)
    print(f"C {case_name} std {std} {dtype}: emulated kernel arithmetic at {rat} of the gates")
    assert rat.worst() <= 0.5, dict(rat)


NEW16 = [n for n in aw.NEW if "fp32" not in aw.SHAPES[n].dtypes]
FP32 = [n for n, c in aw.SHAPES.items() if c.dtypes == ("fp32",)]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", NEW16)
def test_c_gates_hold_for_the_new_instantiations(name, dtype):
    """every 16-bit case of attn_witness.NEW, at both logit standard deviations, whatever witnesses it runs on the GPU (witness A reads the
    same gates for dQ, dV, dn and dbias); the absolute-score model: no case of NEW draws a bias beyond N(0, 1)"""
    assert dtype in aw.SHAPES[name].dtypes
    for std in (4, 8):
        w = world(name, "C", dtype, None, std)
        rat = aw.judge_c(w.case, w.dt, _emulate(w), w.r, w.g)
        print(f"C {name} std {std} {dtype}: emulated kernel arithmetic at {rat} of the gates")
        assert rat.worst() <= 0.5, (std, dict(rat))


@pytest.mark.parametrize("std", [4, 8])
@pytest.mark.parametrize("name", FP32)
def test_c_gates_hold_in_fp32(name, std):
    """witness C in fp32, u = unit(case, fp32) = (S + D) 2^-24: an independent fp32 evaluation of the closed forms - torch fp32, the online
    softmax and every sum over keys in tile order, no rounding point but fp32's own - stays at or below 0.5 of every gate"""
    w = world(name, "C", "fp32", None, std)
    assert w.u == (w.case.S + w.case.D) * 2.0 ** -24
    rat = aw.judge_c(w.case, w.dt, _emulate(w), w.r, w.g)
    print(f"C {name} std {std} fp32: fp32 evaluation at {rat} of the gates")
    assert rat.worst() <= 0.5, dict(rat)
    assert {"out", "lse", "dQ", "dK", "dV", "dn"} <= set(rat)


@pytest.mark.parametrize("name", list(aw.NEW))
def test_new_cases_on_the_reference_alone(name):
    """witness A's class-count condition holds in every type the case runs A in, from the reference alone; the rounded reference passes the
    gates of every witness the case runs"""
    case = aw.SHAPES[name]
    for dtype in case.a_dtypes if "A" in case.wit else ():
        w = world(name, "A", dtype)
        aw.condition_a(w.case, w.r, w.dt, w.p_eff)
        rat = w.judge(w.clean)
        assert "refused" not in rat and rat.worst() <= 0.8 + 1e-9, (dtype, dict(rat))
    for dtype in case.dtypes:
        for form in (aw.B_FORMS if "B" in case.wit else ()):
            if form.startswith("code") and (dtype == "fp32" or not case.bwd):
                continue
            w = world(name, "B", dtype, form)
            rat, kinds = aw.judge_b(w.case, form, w.dt, w.clean, w.r, w.g, w.inp)
            assert rat.worst() <= 1.0 and (1 in kinds or form == "code_sink") and (2 in kinds or "sink" not in form), (dtype, form, dict(rat), kinds)


# ---------------------------------------------------------------- the fp64 reference against the suite's oracle and autograd
@pytest.mark.parametrize("case_name", ["causal L<S", "gqa", "keypad", "bias"])
def test_reference_agrees_with_the_oracle_and_autograd(case_name):
    from oracle.ref_attention import ref_attention_n
    case = CASES[case_name].but(L=70, S=90, lens=None if CASES[case_name].lens is None else [90, 33])
    inp = aw.inputs_c(case, 0.25, torch.bfloat16, CPU, 40)   # the suite's ordinary data: scale = 1 / sqrt(D)
    assert inp["scale"] == 1 / math.sqrt(case.D)
    r = aw.reference(case, inp)
    q, k, v, do, un, ubias = aw.unique_operands(case, inp)
    for b in range(case.ub):
        for h in range(case.uh):
            n = un[b, h].clone().requires_grad_()
            ops = [t[b, h].clone().requires_grad_() for t in (q, k, v)]
            bias = None if ubias is None else ubias[0, h].clone().requires_grad_()
            mask = None if inp["um"] is None else inp["um"][b, 0]
            out = ref_attention_n(*ops, softmax_n_param=n if n > 0 else 0.0, scale=inp["scale"], attn_mask=mask, attn_bias=bias, is_causal=case.causal)
            out.backward(do[b, h])
            pairs = [("out", out.detach(), r["out"][b, h]), ("dQ", ops[0].grad, r["dQ"][b, h]), ("dK", ops[1].grad, r["dK"][b, h]),
                     ("dV", ops[2].grad, r["dV"][b, h])]
            if n > 0:
                pairs.append(("dn", n.grad, r["dn"][b, h]))
            if bias is not None:
                pairs.append(("dbias", bias.grad, r["dS"][b, h]))
            for what, got, want in pairs:
                assert (got - want).abs().max() <= 1e-11 * (1 + want.abs().max()), (case_name, b, h, what)


# ---------------------------------------------------------------- the routes, without a GPU
def test_plans_match_the_golden_file(pkg, golden_dir):
    with open(os.path.join(golden_dir, "attn_witness_plans.txt")) as fh:
        assert aw.plans_file_text(pkg) == fh.read(), "the launch plans of attn_witness.SHAPES changed: tests/golden/attn_witness_plans.txt"


@pytest.mark.parametrize("name", list(aw.SHAPES))
def test_each_case_reaches_the_family_it_is_named_for(pkg, name):
    case = aw.SHAPES[name]
    for dt in case.dtypes:
        text = aw.plan_text(pkg, case, dt)
        for prop in case.want:
            if prop == "pair":   # block r runs with block nblk - 1 - r: half the blocks (rounded up) per (batch, head)
                line = [ln for ln in text.splitlines() if "fasn_fwd_kernel<" in ln][0]
                cfg = dict(kv.split("=") for kv in line.split("cfg=")[1].split(",") if "=" in kv)
                rows = 32 * int(cfg["QB"]) * int(cfg["NW"])
                nblk = -(-case.L // rows)
                assert f"grid={case.B * case.H * ((nblk + 1) // 2)} " in line, (name, dt, line)
            else:
                assert prop in text, (name, dt, prop, text)
        assert " rc=-" not in text
    # every kernel family (template) of DESIGN 4.2 is reached by at least one A, one B and one C case; fasn_bwd_dn, which no launch plan shows
    # (n travels as a pointer per call), runs for a [H], a [B, 1] and a [B, H] n among the cases with a backward
    if name == list(aw.SHAPES)[0]:
        assert {"H", "B1", "BH"} <= {c.nshape for c in aw.SHAPES.values() if c.bwd}
        for fam in ("QB=1,plain", "QB=2,plain", "FOLD=1", "D=128", "D=32", "fasn_fwd_ws256_kernel", "fasn_bwd_dq_pipe_kernel", "fasn_bwd_dkdv_pipe_kernel",
                    "fasn_bwd_dq_ws_kernel", "fasn_bwd_dkdv_ws_kernel", "fasn_bwd_dq_ws256_kernel", "fasn_bwd_dkdv_ws256_kernel", "fasn_bwd_dq_kernel",
                    "fasn_bwd_dkdv_kernel", "fasn_fwd_combine_kernel", "DROP=1", "GQA=1", "element-load"):
            for wit in "ABC":
                assert any(wit in c.wit and fam in aw.plan_text(pkg, c, c.dtypes[0]) for c in aw.SHAPES.values()), (fam, wit)
        for fam, wits in (("fasn_bwd_dbias_ws_kernel", "AC"), ("fasn_bwd_dbias_kernel", "AC"), ("fasn_f32_", "AB")):
            for wit in wits:
                assert any(wit in c.wit and fam in aw.plan_text(pkg, c, c.dtypes[0]) for c in aw.SHAPES.values()), (fam, wit)
