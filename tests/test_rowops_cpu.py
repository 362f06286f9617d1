"""The test of the witnesses of tests/row_witness.py, without a GPU.

  - The plan calls run here (they touch no device): the golden plans of every case, the coverage of every selectable template, and the
    error codes of the plan calls against those of the real calls for arguments both refuse before any launch.
  - An emulation of the kernels' arithmetic in fp32 - the same shift, the same n e^-m term, the sum blocked as the named kernel blocks it
    (each thread's terms in sequence, six butterfly levels, four waves), one rounding to the output type - stays inside every gate on A, B
    and C. In fp32 it is held to half the gate. In the 16-bit types one rounding to nearest may take all of u y by itself (a value just
    above a power of two), so there the emulation BEFORE its output rounding is held to half of what the gate grants the arithmetic (the gate
    without u and t), and the rounded result to the gate.
  - The faults row kernels have: the last vector of a row dropped, a tail element counted twice, padding lanes entering the sum as e^0, the
    exponentials shifted by an unclamped maximum, the n term dropped, the dot product of the wrong row, dx without the dot product. Each is
    injected into the fp64 reference and must break its gate by 10x in every row it touches - for the three faults that move a count, in
    every touched row whose count the output type can resolve, n + c_row <= COUNT_LIMIT (row_witness: witness A keeps its sparse rows
    under it; the output type cannot show one entry among thousands).
  - One element missing or doubled changes the exact power sums; and the cancellation the pivot removes is shown on the issue's ladder."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_witness as rw   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowops_plans.txt")
COUNT_LIMIT = {torch.bfloat16: 20, torch.float16: 160, torch.float32: 8192}
LOG2E = torch.tensor(1.4426950408889634, dtype=torch.float32)
# one shape per kind of kernel and seam side: wave with padding lanes, wave full, block, element cached / uncached (fp32: halved)
EMU_COLS = (8, 1024, 1032, 8200, 16392, 257, 4097, 32776)


def _golden():
    with open(GOLDEN) as f:
        return [l.rstrip("\n") for l in f if l.strip()]


# ---------------------------------------------------------------- plans
def test_golden_plans(pkg):
    got, want = rw.plan_table(pkg._lib), _golden()
    assert got == want, "\n".join(f"{g!r} != {w!r}" for g, w in zip(got, want) if g != w)[:4000] + f" ({len(got)} / {len(want)} lines)"


def test_golden_plans_cover_every_selectable_kernel():
    lines = _golden()
    for direction in ("fwd", "bwd"):
        for dn in rw.DTYPES:
            named = {l.split(" | ")[1].split(" grid=")[0] for l in lines if l.startswith(f"{direction} {dn} ")}
            assert named == rw.selectable(direction, dn), (direction, dn, named ^ rw.selectable(direction, dn))
    for dn, code in rw.CODE.items():
        grids = {int(l.split(" grid=")[1].split()[0]) for l in lines if l.startswith(f"moments {dn} ") and f"moments_kernel<{code}>" in l}
        assert {1, 2, 3, 2045} <= grids, grids   # one chunk, a second chunk of one element, three chunks, the chunk above 4096


def test_seams_sit_on_both_sides_of_every_threshold(pkg):
    """at each dispatch threshold (in vectors) the row at it and the row one vector above name different kernels, and both are cases"""
    for direction, bounds in (("fwd", (128, 256, 512, 1024, 2048, 4096)), ("bwd", (128, 256, 512, 1024, 2048, 4096))):
        for dn, dt in rw.DTYPES.items():
            for nvec in bounds:
                at, above = (rw.plan_of_case(pkg._lib, rw.Case(v * rw.epv(dt)), direction, dn)[0][0] for v in (nvec, nvec + 1))
                assert at != above, (direction, dn, nvec, at)
                keys = {c.cols for c in rw.cases(direction, dn)}
                assert nvec * rw.epv(dt) in keys and (nvec + 1) * rw.epv(dt) in keys


def test_views_reach_the_kernels_the_issue_names(pkg):
    L = pkg._lib
    for direction in ("fwd", "bwd"):
        for dn in rw.DTYPES:
            kind = lambda case: rw.kernel_of(rw.plan_of_case(L, case, direction, dn))[1]   # noqa: E731
            assert kind(rw.Case(4096, 1, 4097)) == "element" and kind(rw.Case(4104, 1, 4105)) == "element"
            assert kind(rw.Case(1024, 8, 1040)) == "wave"
            assert kind(rw.Case(1024, 4, 1040)) == ("wave" if dn == "fp32" else "element")
            for cols in rw.ELEMENT_COLS:
                assert kind(rw.Case(cols)) == "element"
            big = 32776 // (2 if dn == "fp32" else 1)
            assert kind(rw.Case(big)) == "element" and kind(rw.Case(big - rw.epv(rw.DTYPES[dn]))) == "block"


def test_plan_calls_return_the_codes_of_the_real_calls(pkg):
    """arguments the real calls refuse before any launch (so they can be made here): the plan gives the same code"""
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(512)
    p = 4096
    for rows, cols, a, b, c, dt in ((0, 8, p, p, p, 0), (5, 0, p, p, p, 1), (-1, 8, p, p, p, 2), (5, 8, None, p, p, 0), (5, 8, p, None, p, 0),
                                    (5, 8, p, p, p, 3), (5, 8, p, p, p, -1)):
        want_f = lib.fasn_softmax_n_fwd(a, b, rows, cols, cols, cols, 1.0, dt, None)
        want_b = lib.fasn_softmax_n_bwd(a, b, c, rows, cols, cols, cols, cols, dt, None)
        assert want_f < 0 and want_b < 0
        assert lib.fasn_softmax_n_plan(rw.FWD, a, b, c, rows, cols, cols, cols, cols, dt, buf, 512) == want_f
        assert lib.fasn_softmax_n_plan(rw.BWD, a, b, c, rows, cols, cols, cols, cols, dt, buf, 512) == want_b
    assert lib.fasn_softmax_n_bwd(p, p, None, 5, 8, 8, 8, 8, 0, None) == lib.fasn_softmax_n_plan(rw.BWD, p, p, None, 5, 8, 8, 8, 8, 0, buf, 512) == -1
    assert lib.fasn_softmax_n_plan(rw.FWD, p, p, None, 5, 8, 8, 8, 8, 0, buf, 512) > 0, "the forward plan does not read c"
    assert lib.fasn_softmax_n_plan(2, p, p, p, 5, 8, 8, 8, 8, 0, buf, 512) == -1
    assert lib.fasn_softmax_n_plan(rw.FWD, p, p, p, 5, 8, 8, 8, 8, 0, buf, 8) == -1 and lib.fasn_softmax_n_plan(rw.FWD, p, p, p, 5, 8, 8, 8, 8, 0, None, 512) == -1
    assert lib.fasn_softmax_n_fwd(p, p, 5, 8, 8, 8, -1.0, 0, None) == -1 and lib.fasn_softmax_n_fwd(p, p, 5, 8, 8, 8, math.nan, 0, None) == -1
    for x, s, rows, cols, stride, dt in ((None, p, 1, 8, 8, 0), (p, None, 1, 8, 8, 0), (p, p, 0, 8, 8, 0), (p, p, 1, 0, 8, 0), (p, p, 2, 8, 7, 0),
                                         (p, p, 65536, 8, 8, 0), (p, p, 1, 8, 8, 3)):
        want = lib.fasn_moments(x, s, rows, cols, stride, dt, None)
        assert want < 0 and lib.fasn_moments_plan(x, s, rows, cols, stride, dt, buf, 512) == want
    assert lib.fasn_moments_plan(p, p, 1, 8, 8, 0, buf, 4) == -1


# ---------------------------------------------------------------- the kernels' arithmetic, emulated
def _layout(plan, cols, dtype):
    """[T, P] int64: the column thread t adds at its step p in the kernel `plan` names; cols (one past the end) where it adds a padding 0"""
    direction, kind, nv = rw.kernel_of(plan)
    if kind == "element":
        P, T = (16 if (direction == "fwd" and cols <= 4096) else -(-cols // 256)), 256
        idx = torch.arange(T).view(T, 1) + 256 * torch.arange(P).view(1, P)
    else:
        T, E = (64 if kind == "wave" else 256), rw.epv(dtype)
        idx = ((torch.arange(T).view(T, 1, 1) + T * torch.arange(nv).view(1, nv, 1)) * E + torch.arange(E).view(1, 1, E)).reshape(T, nv * E)
    assert idx.shape[1] + 6 + (0 if kind == "wave" else 3) == rw.depth(plan, cols, dtype)
    return torch.where(idx < cols, idx, torch.full_like(idx, cols))


def _blocked_sum(terms, plan, dtype, fused_with=None):
    """sum over the last dimension of fp32 `terms` [rows, cols] the way the kernel does; with fused_with: sum of terms * fused_with by fused
    multiply-adds (one rounding per step)"""
    rows, cols = terms.shape
    idx = _layout(plan, cols, dtype)
    pad = lambda t: torch.cat([t, torch.zeros(rows, 1, dtype=t.dtype)], 1)[:, idx]   # noqa: E731  [rows, T, P]
    a = pad(terms)
    b = None if fused_with is None else pad(fused_with)
    acc = torch.zeros(rows, idx.shape[0], dtype=torch.float32)
    for p in range(idx.shape[1]):
        acc = acc + a[:, :, p] if b is None else (acc.double() + a[:, :, p].double() * b[:, :, p].double()).float()
    acc = acc.view(rows, -1, 64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc[:, :, :o] + acc[:, :, o:2 * o]
    acc = acc[:, :, 0]
    total = acc[:, 0]
    for w in range(1, acc.shape[1]):
        total = total + acc[:, w]
    return total


def emulate_fwd(x, n, plan, dtype):
    """fp32 y before the output rounding"""
    xf = x.float()
    m = xf.amax(-1)
    if n > 0:
        m = m.clamp_min(0.0)
    m = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), m)
    e = torch.exp2((xf - m.unsqueeze(-1)) * LOG2E)
    total = _blocked_sum(e, plan, dtype)
    den = torch.tensor(n, dtype=torch.float32) * torch.exp2(-m * LOG2E) + total if n > 0 else total
    return e * (1.0 / den).unsqueeze(-1)


def emulate_bwd(y, dy, plan, dtype):
    yf, gf = y.float(), dy.float()
    dot = _blocked_sum(yf, plan, dtype, fused_with=gf)
    return yf * (gf - dot.unsqueeze(-1))


def _operands(cols, dtype):
    for n in (0.0, 1.0):
        yield f"A n={n:g}", rw.inputs_a(rw.ROWS, cols, n, dtype)
    for form in rw.B_FORMS:
        yield f"B {form}", rw.inputs_b(rw.ROWS, cols, form, dtype)
    for std in rw.C_STDS:
        for n in rw.C_NS:
            yield f"C std={std} n={n:g}", rw.inputs_c(rw.ROWS, cols, std, n, dtype)


@pytest.mark.parametrize("dn", sorted(rw.DTYPES))
def test_emulated_kernel_arithmetic_stays_inside_the_gates(pkg, dn):
    dt = rw.DTYPES[dn]
    worst = {}
    for cols16 in EMU_COLS:
        cols = cols16 // 2 if (dn == "fp32" and cols16 % 8 == 0) else cols16
        case = rw.Case(cols)
        pf, pb = (rw.plan_of_case(pkg._lib, case, d, dn) for d in ("fwd", "bwd"))
        Kf, Kb = rw.depth(pf, cols, dt), rw.depth(pb, cols, dt)
        for label, inp in _operands(cols, dt):
            ref = rw.softmax_ref(inp["x"], inp["n"])
            y32 = emulate_fwd(inp["x"], inp["n"], pf, dt)
            y = y32.to(dt)
            bref = rw.softmax_bwd_ref(y, inp["dy"])
            dx32 = emulate_bwd(y, inp["dy"], pb, dt)
            res = {"fwd": (rw.gate_forward(y, ref, Kf, dt), rw.gate_forward(y32, ref, Kf, dt, rounding=False)),
                   "bwd": (rw.gate_backward(dx32.to(dt), bref, Kb, dt), rw.gate_backward(dx32, bref, Kb, dt, rounding=False))}
            for d, (rounded, arithmetic) in res.items():
                k = (label.split()[0], d)
                worst[k] = tuple(max(a, b) for a, b in zip(worst.get(k, (0.0, 0.0)), (rounded, arithmetic)))
                if dt == torch.float32:
                    assert rounded <= 0.5, (label, d, cols, rounded)
                else:
                    assert rounded <= 1.0 and arithmetic <= 0.5, (label, d, cols, rounded, arithmetic)
    for (wit, d), (rounded, arithmetic) in sorted(worst.items()):
        print(f"emulation {dn} witness {wit} {d}: rounded result at {rounded:.3f} of its gate, fp32 arithmetic alone at {arithmetic:.3f} of its share")


# ---------------------------------------------------------------- the faults
def _mutation_case(pkg, dn):
    """a wave row with a tail and padding lanes: one vector past the NV = 2 capacity"""
    dt = rw.DTYPES[dn]
    cols = 129 * rw.epv(dt)
    pf, pb = (rw.plan_of_case(pkg._lib, rw.Case(cols), d, dn) for d in ("fwd", "bwd"))
    assert rw.kernel_of(pf)[1:] == ("wave", 4) and rw.kernel_of(pb)[1:] == ("wave", 4)
    return dt, cols, rw.depth(pf, cols, dt), rw.depth(pb, cols, dt), 64 * 4 * rw.epv(dt) - cols


def _assert_caught(name, bad_rows, clean_rows, claim, ratio):
    """every touched row (its result differs from the clean one) that `claim` covers breaks the gate by 10x"""
    touched = (bad_rows != clean_rows).any(-1) & ~(torch.isnan(bad_rows).all(-1) & torch.isnan(clean_rows).all(-1))
    rows = (touched & claim).nonzero().flatten().tolist()
    assert rows, f"{name}: touches no row the claim covers"
    low = {r: ratio[r].item() for r in rows if not ratio[r] >= 10}
    print(f"{name}: rows {rows} of touched {touched.nonzero().flatten().tolist()}, smallest ratio {min(ratio[r].item() for r in rows):.3g}")
    assert not low, (name, low)
    return rows


@pytest.mark.parametrize("dn", sorted(rw.DTYPES))
def test_count_faults_break_witness_a(pkg, dn):
    dt, cols, Kf, _, pad = _mutation_case(pkg, dn)
    rows = 10   # every row kind twice
    for n in (0.0, 1.0):
        inp = rw.inputs_a(rows, cols, n, dt)
        ref = rw.softmax_ref(inp["x"], n)
        count = rw.expect_a(inp, ref).flatten()
        claim = (count + n <= COUNT_LIMIT[dt]) & (count > 0)
        kinds = {int(r) % 5 for r in claim.nonzero().flatten()}
        assert {0, 3} <= kinds, "the single-entry and the sparse rows are inside the claim"
        drop = torch.ones(cols, dtype=torch.float64)
        drop[cols - rw.epv(dt):] = 0
        twice = torch.ones(cols, dtype=torch.float64)
        twice[-1] = 2
        faults = {"last vector dropped": dict(w=drop), "tail element counted twice": dict(w=twice), "padding lanes as e^0": dict(extra=float(pad))}
        if n > 0:
            faults["n term dropped"] = dict(n_term=False)
        for name, kw in faults.items():
            bad = rw.softmax_ref(inp["x"], n, **kw)
            got = _assert_caught(f"A {dn} n={n:g} {name}", bad["y"], ref["y"], claim, rw.gate_forward(bad["y"], ref, Kf, dt, per_row=True))
            assert 3 in {r % 5 for r in got}, "a sparse row sees it"


@pytest.mark.parametrize("dn", sorted(rw.DTYPES))
def test_shift_and_n_term_faults_break_witness_b(pkg, dn):
    dt, cols, Kf, _, _ = _mutation_case(pkg, dn)
    inp = rw.inputs_b(rw.ROWS, cols, "negative", dt)
    ref = rw.softmax_ref(inp["x"], inp["n"])
    assert (ref["m"] == 0).all() and (ref["y"] < 1e-27).all()
    every = torch.ones(rw.ROWS, dtype=torch.bool)
    for name, kw in (("exponentials shifted by the unclamped maximum", dict(clamp=False)), ("n term dropped", dict(n_term=False))):
        bad = rw.softmax_ref(inp["x"], inp["n"], **kw)
        got = _assert_caught(f"B negative {dn} {name}", bad["y"], ref["y"], every, rw.gate_forward(bad["y"], ref, Kf, dt, per_row=True))
        assert len(got) == rw.ROWS
    # the defect of the n == 0 regime: 0 * e^100 = NaN in the denominator
    inp = rw.inputs_b(rw.ROWS, cols, "negative0", dt)
    ref = rw.softmax_ref(inp["x"], 0.0)
    assert torch.allclose(ref["y"], torch.softmax(inp["x"].double(), -1), rtol=1e-12, atol=0)
    assert (rw.gate_forward(torch.full_like(ref["y"], math.nan), ref, Kf, dt, per_row=True) == math.inf).all()


@pytest.mark.parametrize("dn", sorted(rw.DTYPES))
def test_dot_faults_break_the_backward_gate(pkg, dn):
    dt, cols, Kf, Kb, _ = _mutation_case(pkg, dn)
    every = torch.ones(rw.ROWS, dtype=torch.bool)
    sets = [("A n=1", rw.inputs_a(rw.ROWS, cols, 1.0, dt)), ("B spike", rw.inputs_b(rw.ROWS, cols, "spike", dt)), ("C std=8 n=1", rw.inputs_c(rw.ROWS, cols, 8, 1.0, dt))]
    for label, inp in sets:
        y = rw.softmax_ref(inp["x"], inp["n"])["y"].to(dt)
        ref = rw.softmax_bwd_ref(y, inp["dy"])
        for name, kw in (("dot of the next row", dict(roll=1)), ("dx without the dot", dict(no_dot=True))):
            bad = rw.softmax_bwd_ref(y, inp["dy"], **kw)
            got = _assert_caught(f"{label} {dn} {name}", bad["dx"], ref["dx"], every, rw.gate_backward(bad["dx"], ref, Kb, dt, per_row=True))
            assert len(got) >= (rw.ROWS - 1 if label.startswith("A") else rw.ROWS)   # (A's row without entries has y = 0 and dx = 0 whatever the dot)


# ---------------------------------------------------------------- moments
def test_one_element_missing_or_doubled_changes_an_exact_sum():
    x = rw.small_integers((3, 4097), 3, torch.float32)
    want = rw.power_sums_ref(x)
    for j in (1, 7, 4095, 4096):
        for r in range(3):
            if x[r, j] == x[r, 0]:
                continue   # (an element equal to the pivot adds 0 to every sum: losing it loses nothing)
            gone = torch.cat([x[r:r + 1, :j], x[r:r + 1, j + 1:]], 1)
            twice = torch.cat([x[r:r + 1], x[r:r + 1, j:j + 1]], 1)
            for bad in (gone, twice):
                got = rw.power_sums_ref(bad)[0]
                assert got[1] != want[r, 1] and got[3] != want[r, 3], (r, j)


def test_the_pivot_removes_the_cancellation_of_the_raw_sums():
    """the issue's table in numpy fp64: 65536 fp32 samples of R + N(0, 1); central moments from power sums about 0 against those from
    power sums about x[0], both against two passes"""
    rng = np.random.default_rng(0)
    z = rng.standard_normal(65536)

    def kurt(s, c):
        s1, s2, s3, s4 = (v / c for v in s)
        m2 = s2 - s1 * s1
        return (s4 - 4 * s1 * s3 + 6 * s1 * s1 * s2 - 3 * s1 ** 4) / m2 ** 2 - 3.0

    for R, raw_fails in ((1.0, False), (1e3, True), (1e4, True)):
        x = (R + z).astype(np.float32).astype(np.float64)
        want = rw.moments_ref(torch.from_numpy(x).view(1, -1))[2].item()
        raw = kurt([np.sum(x ** k) for k in (1, 2, 3, 4)], x.size)
        piv = kurt([np.sum((x - x[0]) ** k) for k in (1, 2, 3, 4)], x.size)
        print(f"R = {R:g}: excess kurtosis off by {abs(raw - want):.3g} from raw sums, {abs(piv - want):.3g} about the pivot")
        assert abs(piv - want) <= 1e-12
        assert (abs(raw - want) > 2e-5) == raw_fails
