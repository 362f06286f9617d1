"""The test of the witnesses of tests/kv_witness.py, without a GPU: on the fp64 reference alone.

For each witness the visible set of the reference is mutated the way K/V kernels go wrong - the causal limit, the length or the window's
lower edge moved by one key, a 64-key tile dropped or counted twice, the K/V head of a query head off by one, the split partials merged
with weights of 1 instead of e^(m_s - m*) - and the mutated result is put through the witness's gate as if a kernel had returned it. The
gate must break by at least 10x in at least one row of EVERY sequence the fault touches, the 4000-key one included: that is what the
whole-tensor gate of the other K/V tests cannot do (at lens = [300, 5, 4000] a causal limit one key off moves the rows of the 4000-key
sequence by 1e-3 against a bf16 gate of 2.2e-2). What each witness claims:

  A  every fault of the visible set (it counts keys), and the head mapping. Not the merge: with query = 0 every m_s is 0 and the right
     weights are all 1.
  B  the three edges - the winner is the last or the first visible key - and the merge. Not a tile inside the visible range.
  C  the merge (and, like the existing tests, whatever moves a row by more than 3 u A).

The unmutated reference, rounded to the output type, passes every gate with the stated conditions met; an emulation of the kernels'
arithmetic (fp32 scores, 64-key online tiles, P rounded to the operand type, fp32 accumulation) stays inside witness C's bound; and the
fp64 reference agrees with the suite's fp32 _reference on an ordinary case under the suite's _check."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_witness as kw   # noqa: E402
import kv_support as ks   # noqa: E402

CPU = torch.device("cpu")
LENS = [300, 5, 4000]
BASE = kw.Case("prefill", H=4, Hkv=2, D=64, Sq=3, lens=LENS)
CASES = {"causal": BASE, "full": BASE.but(causal=False), "window": BASE.but(route="window_prefill", window=200)}
# (fault, delta) -> the case whose visible set it changes. The length moves the visible set only where the causal limit does not cap it.
FAULTS = {"causal+1": "causal", "causal-1": "causal", "len+1": "full", "len-1": "full", "wlo+1": "window", "wlo-1": "window",
          "drop": "causal", "dup": "causal"}


def _weights(case, b, fault):
    """w [qlen_b, S] of sequence b under `fault`, S = len_b + 1 (the row behind the length is there to be seen by a length one too long)"""
    ln, ql = case.total[b], case.qlens[b]
    S = ln + 1
    i = torch.arange(ql).view(-1, 1)
    j = torch.arange(S).view(1, -1)
    p = i + ln - ql
    d = {"+1": 1, "-1": -1}.get(fault[-2:], 0) if fault else 0
    w = (j < ln + (d if fault.startswith("len") else 0)).expand(ql, S).clone()
    if case.causal:
        w &= j <= p + (d if fault.startswith("causal") else 0)
    if case.window is not None:
        w &= j > p - case.window + (d if fault.startswith("wlo") else 0)
    w = w.double()
    t = (ln // kw.KT) // 2   # a tile in the middle of the sequence
    if fault == "drop":
        w[:, t * kw.KT:(t + 1) * kw.KT] = 0
    if fault == "dup":
        w[:, t * kw.KT:(t + 1) * kw.KT] *= 2
    return w


def _faulty(case, inp, fault, swap_heads=False):
    res = []
    for b in range(case.B):
        q, k, v, n, sl = kw.sequence(case, inp, b)
        w = _weights(case, b, fault)
        S = w.shape[1]
        if swap_heads:
            k, v = k.roll(1, 0), v.roll(1, 0)
        res.append(kw.attend(q, k[:, :S], v[:, :S], w, n, inp["scale"]))
    return res


def _merged(case, inp, nsplit, equal):
    """the reference cut into `nsplit` tile-aligned key ranges (the sink on range 0) and merged: with the weights e^(m_s - m*), or, the
    fault, with weights of 1"""
    res = []
    for b in range(case.B):
        q, k, v, n, sl = kw.sequence(case, inp, b)
        ln, ql = case.total[b], case.qlens[b]
        w = kw.visible(ln, ql, ln, case.causal, case.window).double()
        tiles = -(-ln // kw.KT)
        tps = -(-tiles // nsplit)
        parts = []
        for s in range(nsplit):
            lo, hi = min(s * tps * kw.KT, ln), min((s + 1) * tps * kw.KT, ln)
            ws = torch.zeros_like(w)
            ws[:, lo:hi] = w[:, lo:hi]
            parts.append(kw.attend(q, k[:, :ln], v[:, :ln], ws, n if s == 0 else torch.zeros_like(n), inp["scale"]))
        m = torch.stack([r["m"] for r in parts]).amax(0)
        wt = [torch.ones_like(m) if equal else torch.exp(r["m"] - m) for r in parts]
        l = sum(r["l"] * c for r, c in zip(parts, wt))
        acc = sum(r["acc"] * c.unsqueeze(-1) for r, c in zip(parts, wt))
        safe = torch.where(l > 0, l, torch.ones_like(l))
        res.append(dict(out=acc / safe.unsqueeze(-1), lse=torch.where(l > 0, m + torch.log(safe), torch.full_like(m, -math.inf)), l=l))
    return res


def _touched(case, fault):
    return [b for b in range(case.B) if not torch.equal(_weights(case, b, fault), _weights(case, b, ""))]


# ---------------------------------------------------------------- A
@pytest.fixture(scope="module")
def a_inputs():
    return {name: kw.inputs_a(c, torch.float16, CPU, 10) for name, c in CASES.items()}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_a_sees_every_fault_of_the_visible_set_in_every_sequence(a_inputs, fault):
    case, inp = CASES[FAULTS[fault]], a_inputs[FAULTS[fault]]
    refs = kw.reference(case, inp)
    kw.condition_a(refs, torch.float16)
    bad = _faulty(case, inp, fault)
    touched = _touched(case, fault)
    assert 2 in touched and 0 in touched, "the fault must reach the long sequences"
    for b in touched:
        rz, ro = kw.gate_a(bad[b]["out"], bad[b]["lse"], refs[b])
        print(f"A {fault} sequence {b} ({case.total[b]} keys): exp(lse) {rz:.1f}x its gate, out {ro:.1f}x its gate")
        assert max(rz, ro) >= 10, (fault, b, rz, ro)
        assert ro > 1, "the class counts see it too"


def test_a_sees_a_wrong_head_mapping(a_inputs):
    case, inp = CASES["causal"], a_inputs["causal"]
    refs = kw.reference(case, inp)
    bad = _faulty(case, inp, "", swap_heads=True)
    for b in (0, 2):
        rz, ro = kw.gate_a(bad[b]["out"], bad[b]["lse"], refs[b])
        print(f"A swapped K/V heads, sequence {b}: out {ro:.1f}x its gate")
        assert ro >= 10


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_passes_unmutated(name, dtype):
    dt = kw.DTYPES[dtype]
    case = CASES[name] if dtype == "fp16" else CASES[name].but(lens=[300, 5, 900], total=[300, 5, 900])   # bf16: one half tile per class
    inp = kw.inputs_a(case, dt, CPU, 10)
    refs = kw.reference(case, inp)
    cmax = kw.condition_a(refs, dt)
    for b, r in enumerate(refs):
        count = r["l"] - kw.sequence(case, inp, b)[3].view(-1, 1)
        assert torch.equal(count, count.round()) and (r["acc"][..., :-1] == r["acc"][..., :-1].round()).all(), "counts are integers"
        assert torch.equal(r["acc"][..., :case.D // 2].sum(-1), count), "every visible key is in exactly one class of the first half"
        rz, ro = kw.gate_a(r["out"].to(dt), r["lse"].float(), r)
        print(f"A {name} {dtype} sequence {b}: max class count {cmax}, rounded reference at {rz:.3f} / {ro:.3f} of the gates")
        assert rz <= 1 and ro <= 0.8 + 1e-9   # the output's own rounding stays under 0.2 of 0.25


# ---------------------------------------------------------------- B
B_CLAIMS = {"causal+1": "ascending", "causal-1": "ascending", "len+1": "ascending", "len-1": "ascending", "wlo+1": "descending",
            "wlo-1": "descending"}


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("fault", sorted(B_CLAIMS))
def test_b_sees_the_edges_in_every_sequence(fault, dtype):
    dt = kw.DTYPES[dtype]
    case = CASES[FAULTS[fault]]
    inp = kw.inputs_b(case, B_CLAIMS[fault], dt, CPU, 20)
    refs = kw.reference(case, inp)
    bad = _faulty(case, inp, fault)
    for b in _touched(case, fault):
        kind, want = kw.expect_b(refs[b], kw.sequence(case, inp, b)[2][:, :case.total[b]], case.H // case.Hkv)
        r = kw.gate_b(bad[b]["out"], kind, want, dt)
        print(f"B {B_CLAIMS[fault]} {fault} {dtype} sequence {b}: {r:.3g}x the gate")
        assert r >= 10
        if B_CLAIMS[fault] == "ascending":   # (descending: the logits reach 2e6 nats and 1e-4 of that is wider than one key's 32)
            with pytest.raises(AssertionError):
                ks._check_lse(bad[b]["lse"], refs[b]["lse"], "mutated lse")


@pytest.mark.parametrize("form", kw.B_FORMS)
def test_b_sees_an_equal_weight_merge_and_passes_unmutated(form):
    dt = torch.bfloat16
    for name, case in CASES.items():
        if (form == "descending") != (name == "window"):
            continue
        inp = kw.inputs_b(case, form, dt, CPU, 21)
        refs = kw.reference(case, inp)
        good, bad = _merged(case, inp, 4, equal=False), _merged(case, inp, 4, equal=True)
        for b in range(case.B):
            kind, want = kw.expect_b(refs[b], kw.sequence(case, inp, b)[2][:, :case.total[b]], case.H // case.Hkv)
            assert {1, 2} <= set(kind.unique().tolist()) or form != "sink", "the sink decides in some heads and a key in others"
            assert kw.gate_b(refs[b]["out"].to(dt), kind, want, dt) <= 0.5 + 1e-9, "the rounded reference: one rounding of two"
            assert kw.gate_b(good[b]["out"], kind, want, dt) <= 0.5   # (where the sink decides, e^-32 |v| / n is a quarter of 1e-12)
            ks._check_lse(good[b]["lse"], refs[b]["lse"], "merged lse")
            if case.total[b] > 4 * kw.KT:   # more than one range holds a key
                r = kw.gate_b(bad[b]["out"], kind, want, dt)
                print(f"B {form} {name} sequence {b}: equal-weight merge {r:.3g}x the gate")
                assert r >= 10


# ---------------------------------------------------------------- C
@pytest.mark.parametrize("std", [4, 8])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_c_sees_an_equal_weight_merge_and_passes_unmutated(dtype, std):
    dt = kw.DTYPES[dtype]
    case = CASES["causal"]
    inp = kw.inputs_c(case, std, dt, CPU, 30)
    refs = kw.reference(case, inp)
    good, bad = _merged(case, inp, 4, equal=False), _merged(case, inp, 4, equal=True)
    for b in range(case.B):
        x = refs[b]["x"]
        if b == 2:
            got = x[torch.isfinite(x)].std().item()
            assert 0.9 * std <= got <= 1.1 * std, f"logit standard deviation {got}"
        assert kw.gate_c(refs[b]["out"].to(dt), refs[b], dt) <= 1 / 3 + 1e-9, "the rounded reference: one rounding of three"
        assert kw.gate_c(good[b]["out"], refs[b], dt) <= 1e-6
        if case.total[b] > 4 * kw.KT:
            r = kw.gate_c(bad[b]["out"], refs[b], dt)
            print(f"C std {std} {dtype} sequence {b}: equal-weight merge {r:.3g}x the gate")
            assert r >= 10


def _emulate(q, k, v, w, n, scale, dt):
    """the kernels' arithmetic on the CPU: fp32 scores in the log2 domain, online softmax over 64-key tiles, P rounded to the operand type
    for the P.V product, l summed from the unrounded p, fp32 accumulation, one rounding of out"""
    H, L, D = q.shape
    Hkv, S, _ = k.shape
    G = H // Hkv
    c = torch.tensor(scale * math.log2(math.e), dtype=torch.float32)
    qf, kf, vf = q.float().view(Hkv, G, L, D), k.float(), v.float()
    m = torch.where(n.view(H, 1) > 0, 0.0, -math.inf).float().expand(H, L).clone()
    l = n.float().view(H, 1).expand(H, L).clone()
    acc = torch.zeros(H, L, D, dtype=torch.float32)
    for k0 in range(0, S, kw.KT):
        s = torch.einsum("kgld,ksd->kgls", qf, kf[:, k0:k0 + kw.KT]).reshape(H, L, -1) * c
        s = torch.where(w[:, k0:k0 + kw.KT] > 0, s, torch.full_like(s, -math.inf))
        m_new = torch.maximum(m, s.amax(-1))
        m_use = torch.where(torch.isfinite(m_new), m_new, torch.zeros_like(m_new))
        alpha = torch.exp2(m - m_use)
        p = torch.exp2(s - m_use.unsqueeze(-1))
        l = l * alpha + p.sum(-1)
        pv = torch.einsum("kgls,ksd->kgld", p.to(dt).float().view(Hkv, G, L, -1), vf[:, k0:k0 + kw.KT]).reshape(H, L, D)
        acc = acc * alpha.unsqueeze(-1) + pv
        m = m_new
    return (acc / torch.where(l > 0, l, torch.ones_like(l)).unsqueeze(-1)).to(dt)


@pytest.mark.parametrize("std", [4, 8])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_c_bound_holds_for_the_kernels_arithmetic(dtype, std):
    dt = kw.DTYPES[dtype]
    case = CASES["causal"]
    inp = kw.inputs_c(case, std, dt, CPU, 31)
    refs = kw.reference(case, inp)
    for b in range(case.B):
        q, k, v, n, _ = kw.sequence(case, inp, b)
        ln = case.total[b]
        got = _emulate(q, k[:, :ln], v[:, :ln], kw.visible(ln, case.qlens[b], ln, True, None).double(), n, inp["scale"], dt)
        r = kw.gate_c(got, refs[b], dt)
        print(f"C std {std} {dtype} sequence {b}: emulated kernel arithmetic at {r:.3f} of the gate 3 u A + 1e-6")
        assert r <= 0.5, "three roundings of u A each are allowed; the emulation should need about one"


# ---------------------------------------------------------------- the fp64 reference against the suite's own
def test_reference_agrees_with_the_suites_reference():
    dt = torch.bfloat16
    case = kw.Case("prefill", H=8, Hkv=2, D=64, Sq=5, lens=[130, 64, 5, 0], qlens=[5, 1, 3, 2])
    inp = kw.inputs_c(case, 0.25, dt, CPU, 40)   # the suite's ordinary data: scale = 1 / sqrt(D)
    assert inp["scale"] == 1 / math.sqrt(case.D)
    for causal in (True, False):
        refs = kw.reference(case.but(causal=causal), inp)
        for b, ql in enumerate(case.qlens):
            ln = case.total[b]
            S = max(ln, 1)
            kd = torch.zeros(1, case.Hkv, S, case.D, dtype=dt)
            vd = torch.zeros(1, case.Hkv, S, case.D, dtype=dt)
            kd[0, :, :ln], vd[0, :, :ln] = inp["kd"][b, :, :ln], inp["vd"][b, :, :ln]
            o, lse = ks.reference(inp["q"][b:b + 1, :, :ql], kd, vd, ks._visibility([ln], ql, S, causal, CPU), inp["n"].view(1, -1))
            ks._check(refs[b]["out"], o[0], dt, f"fp64 reference vs _reference, sequence {b} causal={causal} out")
            ks._check_lse(refs[b]["lse"], lse[0], f"fp64 reference vs _reference, sequence {b} causal={causal} lse")
            assert (refs[b]["out"].float() - o[0]).abs().max() <= 1e-5
