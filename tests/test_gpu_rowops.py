"""The row kernels on the GPU under the witnesses of tests/row_witness.py: softmax_n forward and backward on either side of every dispatch
threshold and through every way into the element-load kernels, the C ABI's own row strides, the grid-stride loops, the front end; the power
sums bit for bit at every chunk seam, through the vector fallback and the slab loop, and the moments of data with a large offset.

Every case asserts first that the plan of the call it is about to make is the golden one (tests/golden/rowops_plans.txt), so a case cannot
drift to another kernel unnoticed, and prints its largest ratio to its gate before asserting it.

Not reached: the grid-stride loops of the BLOCK kernels. They turn only above 2^20 rows of more than 4096 (backward) or 8192 (forward) 16-bit
elements, about 17 GB a tensor; the loops of the wave and the element-load kernels, the same three lines, are run below."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_witness as rw   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowops_plans.txt")
NAMES = sorted(rw.DTYPES)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return dict(l.rstrip("\n").split(" | ") for l in f if l.strip())


def _framed(t, lead, width):
    """t [rows, cols] as base[:, lead:lead + cols] of a NaN-filled [rows, width] base; returns (view, base)"""
    base = torch.full((t.shape[0], width), math.nan, dtype=t.dtype, device=t.device)
    base[:, lead:lead + t.shape[1]] = t
    return base[:, lead:lead + t.shape[1]], base


def _frame_intact(base, lead, cols, what):
    assert torch.isnan(base[:, :lead]).all() and torch.isnan(base[:, lead + cols:]).all(), f"{what}: written outside its rows"


def c_fwd(pkg, x, y, n):
    """fasn_softmax_n_fwd on 2-D views, called as softmax.py calls it"""
    lib = pkg._lib.load()
    rc = lib.fasn_softmax_n_fwd(x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], x.stride(0), y.stride(0), n, rw.CODE[_name(x)],
                                torch.cuda.current_stream(x.device).cuda_stream)
    pkg._lib.check(rc, "fasn_softmax_n_fwd")


def c_bwd(pkg, y, dy, dx):
    lib = pkg._lib.load()
    rc = lib.fasn_softmax_n_bwd(y.data_ptr(), dy.data_ptr(), dx.data_ptr(), y.shape[0], y.shape[1], y.stride(0), dy.stride(0), dx.stride(0),
                                rw.CODE[_name(y)], torch.cuda.current_stream(y.device).cuda_stream)
    pkg._lib.check(rc, "fasn_softmax_n_bwd")


def _name(t):
    return {v: k for k, v in rw.DTYPES.items()}[t.dtype]


def _run_case(pkg, golden, case, direction, dn, inp):
    """the case's forward (or, on the forward's output, its backward) through the C ABI with every operand in the case's geometry; returns
    (ratio to the gate, kernel kind)"""
    dt = rw.DTYPES[dn]
    nan = torch.full((case.rows, case.cols), math.nan, dtype=dt, device=inp["x"].device)
    x, _ = _framed(inp["x"], case.lead, case.width)
    y, yb = _framed(nan, case.lead, case.width)
    want_plan = golden[case.key(direction, dn)]
    if direction == "fwd":
        plan = rw.plan_of_tensors(pkg._lib, "fwd", x, y)
        assert rw.plan_line(plan) == want_plan, (case.key(direction, dn), plan)
        c_fwd(pkg, x, y, inp["n"])
        _frame_intact(yb, case.lead, case.cols, "y")
        ref = rw.softmax_ref(inp["x"], inp["n"])
        if "vis" in inp:
            rw.expect_a(inp, ref)
        return rw.gate_forward(y, ref, rw.depth(plan, case.cols, dt), dt), rw.kernel_of(plan)[1]
    c_fwd(pkg, x, y, inp["n"])   # the backward's y is the forward's output tensor, whatever kernel made it
    dy, _ = _framed(inp["dy"], case.lead, case.width)
    dx, dxb = _framed(nan, case.lead, case.width)
    plan = rw.plan_of_tensors(pkg._lib, "bwd", y, dy, dx)
    assert rw.plan_line(plan) == want_plan, (case.key(direction, dn), plan)
    c_bwd(pkg, y, dy, dx)
    _frame_intact(dxb, case.lead, case.cols, "dx")
    if torch.isnan(y).any():   # (a row without entries at n == 0: NaN in, NaN out)
        assert torch.equal(torch.isnan(dx).all(-1), torch.isnan(y).all(-1))
    ref = rw.softmax_bwd_ref(y, inp["dy"])
    return rw.gate_backward(dx, ref, rw.depth(plan, case.cols, dt), dt), rw.kernel_of(plan)[1]


def _report(label, worst):
    for kind, (r, where) in sorted(worst.items()):
        print(f"{label} {kind} kernels: largest ratio to the gate {r:.3f} at {where}")
    bad = {k: v for k, v in worst.items() if not v[0] <= 1.0}
    assert not bad, (label, bad)


def _note(worst, kind, r, where):
    if not r <= worst.get(kind, (-1.0, ""))[0]:
        worst[kind] = (r, where)


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("dn", NAMES)
def test_witness_a_counts_at_every_seam(pkg, dev, golden, dn, direction):
    dt, worst = rw.DTYPES[dn], {}
    for case in rw.cases(direction, dn):
        for n in (0.0, 1.0):
            r, kind = _run_case(pkg, golden, case, direction, dn, rw.inputs_a(case.rows, case.cols, n, dt, dev))
            _note(worst, kind, r, f"{case.key(direction, dn)} n={n:g}")
    _report(f"A {direction} {dn}", worst)


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("form", rw.B_FORMS)
@pytest.mark.parametrize("dn", NAMES)
def test_witness_b_one_entry_decides_at_every_seam(pkg, dev, golden, dn, form, direction):
    dt, worst = rw.DTYPES[dn], {}
    for case in rw.cases(direction, dn):
        r, kind = _run_case(pkg, golden, case, direction, dn, rw.inputs_b(case.rows, case.cols, form, dt, dev))
        _note(worst, kind, r, case.key(direction, dn))
    _report(f"B {form} {direction} {dn}", worst)


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("dn", NAMES)
def test_witness_c_dynamic_range_in_every_template(pkg, dev, golden, dn, direction):
    dt, worst, seen = rw.DTYPES[dn], {}, set()
    for case in rw.cases(direction, dn):
        name = golden[case.key(direction, dn)].split(" grid=")[0]
        if name in seen:
            continue
        seen.add(name)
        for std in rw.C_STDS:
            for n in rw.C_NS:
                r, kind = _run_case(pkg, golden, case, direction, dn, rw.inputs_c(case.rows, case.cols, std, n, dt, dev))
                _note(worst, name, r, f"{case.key(direction, dn)} std={std} n={n:g}")
    assert seen == rw.selectable(direction, dn)
    _report(f"C {direction} {dn}", worst)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dn", NAMES)
def test_c_abi_row_strides_differ_per_operand(pkg, dev, dn, aligned):
    """x, y, dy and dx each in a wider buffer of its own row stride and offset; the frames around the rows stay as they were"""
    dt, cols = rw.DTYPES[dn], 1024
    geo = dict(x=(8, 1048), y=(16, 1064), dy=(24, 1080), dx=(32, 1096)) if aligned else dict(x=(1, 1031), y=(3, 1049), dy=(8, 1040), dx=(5, 1061))
    inp = rw.inputs_c(rw.ROWS, cols, 8, 1.0, dt, dev)
    nan = torch.full((rw.ROWS, cols), math.nan, dtype=dt, device=dev)
    x, xb = _framed(inp["x"], *geo["x"])
    y, yb = _framed(nan, *geo["y"])
    pf = rw.plan_of_tensors(pkg._lib, "fwd", x, y)
    assert rw.kernel_of(pf)[1] == ("wave" if aligned else "element")
    c_fwd(pkg, x, y, 1.0)
    _frame_intact(yb, geo["y"][0], cols, "y")
    _frame_intact(xb, geo["x"][0], cols, "x")
    rf = rw.gate_forward(y, rw.softmax_ref(inp["x"], 1.0), rw.depth(pf, cols, dt), dt)
    dy, _ = _framed(inp["dy"], *geo["dy"])
    dx, dxb = _framed(nan, *geo["dx"])
    pb = rw.plan_of_tensors(pkg._lib, "bwd", y, dy, dx)
    assert rw.kernel_of(pb)[1] == ("wave" if aligned else "element")
    c_bwd(pkg, y, dy, dx)
    _frame_intact(dxb, geo["dx"][0], cols, "dx")
    rb = rw.gate_backward(dx, rw.softmax_bwd_ref(y, inp["dy"]), rw.depth(pb, cols, dt), dt)
    print(f"C ABI strides {dn} {'aligned' if aligned else 'unaligned'}: forward {rf:.3f}, backward {rb:.3f} of the gates")
    assert rf <= 1 and rb <= 1


@pytest.mark.parametrize("dn,rows,cols,kind", [("bf16", 4 * 2 ** 20 + 5, 8, "wave"), ("fp16", 2 ** 20 + 3, 3, "element")])
def test_grid_stride_loops(pkg, dev, dn, rows, cols, kind):
    """more rows than the grid holds workgroups for. Witness B's spike, the expectation built from arange on the device: y is `hi` at
    t(r) = (7 r + 3) mod cols and `lo` elsewhere; a row the loop skips keeps its NaN."""
    dt, n = rw.DTYPES[dn], 1.0
    u, t_ = rw.U[dt], rw.T[dt] + 2.0 ** -149
    r = torch.arange(rows, device=dev)
    spike = (torch.arange(cols, device=dev).view(1, -1) == ((7 * r + 3) % cols).view(-1, 1))
    x = torch.where(spike, 64.0, 0.0).to(dt)
    y = torch.full((rows, cols), math.nan, dtype=dt, device=dev)
    pf = rw.plan_of_tensors(pkg._lib, "fwd", x, y)
    assert rw.kernel_of(pf)[1] == kind and pf[0][1] == 2 ** 20, pf
    c_fwd(pkg, x, y, n)
    den = 1.0 + (cols - 1 + n) * math.exp(-64.0)
    hi, lo = 1.0 / den, math.exp(-64.0) / den
    want = torch.where(spike, hi, lo).double()
    err, bound = (y.double() - want).abs(), 2 * u * want + t_
    ratio = (err / bound).nan_to_num(math.inf).max().item()
    print(f"grid-stride forward {dn} [{rows}, {cols}] {pf[0][0]} grid={pf[0][1]}: {ratio:.3f} of 2 u y + t")
    assert ratio <= 1
    dy = (torch.arange(cols, device=dev) + 1).to(dt).view(1, -1).expand(rows, cols).contiguous()
    dx = torch.full((rows, cols), math.nan, dtype=dt, device=dev)
    pb = rw.plan_of_tensors(pkg._lib, "bwd", y, dy, dx)
    assert rw.kernel_of(pb)[1] == kind and pb[0][1] == 2 ** 20, pb
    c_bwd(pkg, y, dy, dx)
    K = rw.depth(pb, cols, dt)
    y64, g64 = y.double(), dy.double()
    dot = (y64 * g64).sum(-1, keepdim=True)
    ref = y64 * (g64 - dot)
    bound = (u + 3 * rw.E24) * ref.abs() + y64 * (K + 2) * rw.E24 * (y64 * g64).abs().sum(-1, keepdim=True) + t_
    ratio = ((dx.double() - ref).abs() / bound).nan_to_num(math.inf).max().item()
    print(f"grid-stride backward {dn} [{rows}, {cols}] {pb[0][0]} grid={pb[0][1]}: {ratio:.3f} of the gate")
    assert ratio <= 1


# ---------------------------------------------------------------- the front end
@pytest.mark.parametrize("dn", NAMES)
def test_front_end_views_dims_and_dtype(pkg, dev, dn):
    dt = rw.DTYPES[dn]
    K = 16 + 9   # the register-cached element-load forward; the wave NV = 2 sum is shorter
    # x[:, 1:]: what a caller writes to reach the element-load kernels
    for cols in (4096, 1024):
        inp = rw.inputs_c(rw.ROWS, cols, 8, 1.0, dt, dev)
        xv, _ = _framed(inp["x"], 1, cols + 1)
        r = rw.gate_forward(pkg.softmax_n(xv, n=1.0), rw.softmax_ref(inp["x"], 1.0), K, dt)
        print(f"front end {dn} x[:, 1:] cols={cols}: {r:.3f}")
        assert r <= 1
    # a dim other than the last, on a non-contiguous input
    base = rw.inputs_c(6, 7 * 40, 4, 0.0, dt, dev)["x"].view(6, 7, 40)
    xt = base.transpose(0, 2)                      # [40, 7, 6], non-contiguous
    got = pkg.softmax_n(xt, n=0.5, dim=0)
    assert got.shape == xt.shape
    ref = rw.softmax_ref(xt.movedim(0, -1).reshape(-1, 40), 0.5)
    r = rw.gate_forward(got.movedim(0, -1).reshape(-1, 40), ref, K, dt)
    assert r <= 1, r
    # dtype=: compute in x's type, then cast - bit for bit the cast of the plain call
    other = torch.float32 if dt != torch.float32 else torch.bfloat16
    assert torch.equal(pkg.softmax_n(base, n=1.0, dtype=other), pkg.softmax_n(base, n=1.0).to(other))
    # n=None is n = 0
    assert torch.equal(pkg.softmax_n(base), pkg.softmax_n(base, n=0.0))
    r = rw.gate_forward(pkg.softmax_n(base).reshape(-1, 40), rw.softmax_ref(base.reshape(-1, 40), 0.0), K, dt)
    assert r <= 1, r
    # what the C call refuses
    for bad in (lambda: pkg.softmax_n(base, n=-1.0), lambda: pkg.softmax_n(base[:0].reshape(0, 40))):
        with pytest.raises(pkg._lib.FasnError, match="code -1"):
            bad()
    lib = pkg._lib.load()
    assert lib.fasn_softmax_n_fwd(base.data_ptr(), base.data_ptr(), 4, 0, 40, 40, 0.0, rw.CODE[dn], None) == -1


@pytest.mark.parametrize("dn", NAMES)
def test_wholly_hidden_rows(pkg, dev, dn):
    """a row of -inf alone is exactly 0 under n > 0 and NaN under n == 0, in every kind of kernel; its neighbours are untouched by it"""
    dt = rw.DTYPES[dn]
    for cols, kind in ((3, "element"), (8, "wave"), (8200, "block")):
        x = torch.zeros(rw.ROWS, cols, dtype=dt, device=dev)
        x[1] = -math.inf
        x[4] = -math.inf
        y = torch.empty_like(x)
        assert rw.kernel_of(rw.plan_of_tensors(pkg._lib, "fwd", x, y))[1] == kind
        y1, y0 = pkg.softmax_n(x, n=1.0), pkg.softmax_n(x, n=0.0)
        assert (y1[[1, 4]] == 0).all() and torch.isnan(y0[[1, 4]]).all()
        for y, n in ((y1, 1.0), (y0, 0.0)):
            # the sum of ones is exact; the reciprocal (1 ulp = 2 u in fp32), the product and the output rounding are not
            assert ((y[[0, 2, 3]].double() - 1.0 / (n + cols)).abs() <= 4 * rw.U[dt] / (n + cols)).all()


@pytest.mark.parametrize("dn", NAMES)
def test_autograd_round_trip_with_a_strided_dy(pkg, dev, dn):
    dt, cols = rw.DTYPES[dn], 1032
    inp = rw.inputs_c(rw.ROWS, cols, 8, 1.0, dt, dev)
    x = inp["x"].clone().requires_grad_()
    y = pkg.softmax_n(x, n=1.0)
    dyt = inp["dy"].t().contiguous().t()           # [rows, cols] with strides (1, rows)
    assert not dyt.is_contiguous()
    y.backward(dyt)
    yd = y.detach()
    dxbuf = torch.empty_like(yd)
    plan = rw.plan_of_tensors(pkg._lib, "bwd", yd, inp["dy"], dxbuf)
    r = rw.gate_backward(x.grad, rw.softmax_bwd_ref(yd, inp["dy"]), rw.depth(plan, cols, dt), dt)
    print(f"autograd {dn}: {plan[0][0]}, {r:.3f} of the gate")
    assert r <= 1


# ---------------------------------------------------------------- moments
def _exact(pkg, x, dim, x2d, what):
    count, sums, _ = pkg.statistics._power_sums(x, dim)
    want = rw.power_sums_ref(x2d)
    assert count == x2d.shape[1] and sums.shape == (x2d.shape[0], 4)
    got = sums.cpu()
    assert torch.equal(got, want.double()), f"{what}: rows {(got != want.double()).any(-1).nonzero().flatten()[:8].tolist()} differ, e.g. {got[(got != want.double()).any(-1)][:1].tolist()} != {want[(got != want.double()).any(-1)][:1].tolist()}"


@pytest.mark.parametrize("dn", NAMES)
def test_power_sums_are_exact_at_every_chunk_seam(pkg, dev, golden, dn):
    dt = rw.DTYPES[dn]
    for rows, cols in rw.MOMENT_SHAPES[:-2]:
        x = rw.small_integers((rows, cols), 100 + cols, dt, dev)
        plan = pkg._lib.moments_plan(x.data_ptr(), x.data_ptr(), rows, cols, cols, rw.CODE[dn])
        assert rw.plan_line(plan) == golden[f"moments {dn} rows={rows} cols={cols}"]
        _exact(pkg, x, -1, x, f"[{rows}, {cols}]")


@pytest.mark.parametrize("dn", NAMES)
def test_power_sums_are_exact_through_the_element_path(pkg, dev, dn):
    dt = rw.DTYPES[dn]
    x = rw.small_integers((9001,), 7, dt, dev)
    _exact(pkg, x[1:], None, x[1:].view(1, -1), "x[1:] of a 1-D tensor (a pointer off 16 bytes)")
    x = rw.small_integers((4, 1024), 8, dt, dev)
    _exact(pkg, x[:, 3:1003], -1, x[:, 3:1003], "x[:, 3:1003]")
    x = rw.small_integers((3, 1001), 9, dt, dev)
    _exact(pkg, x, -1, x, "[3, 1001]: the rows alternate between the vector and the element path")


def test_power_sums_of_one_long_row_and_of_the_slab_loop(pkg, dev, golden):
    rows, cols = rw.MOMENT_SHAPES[-2]
    x = rw.small_integers((rows, cols), 11, torch.float32, dev)
    assert golden[f"moments fp32 rows={rows} cols={cols}"].split(" grid=")[1].startswith("2045 "), "a chunk of 4104: above 4096"
    _exact(pkg, x, -1, x, "one row of 2048 * 4096 + 9")
    x = rw.small_integers((65536, 3), 12, torch.bfloat16, dev)
    assert pkg.statistics._MAX_ROWS == 65535
    _exact(pkg, x, -1, x, "[65536, 3]: the last slab holds one row")


def _close(got, want, tol, what):
    got, want = got.double().cpu(), want.double()
    err, lim = (got - want).abs(), tol + tol * want.abs()
    print(f"{what}: largest error {(err / lim).max().item():.3g} x its bound, {tol:g} (1 + |want|) (got {got.tolist()}, want {want.tolist()})")
    assert (err <= lim).all(), what


@pytest.mark.parametrize("dn,R", [("fp32", 0.0), ("fp32", 1e2), ("fp32", 1e3), ("fp32", 1e4), ("bf16", 1e2), ("fp16", 1e2)])
def test_moments_of_data_with_a_large_offset(pkg, dev, dn, R):
    """R + N(0, 1) against two passes in fp64 on the same rounded values, under the tolerances of tests/test_statistics.py"""
    from flash_attention_softmax_n_amd import synth
    dt, st = rw.DTYPES[dn], pkg.statistics
    z = synth.counter_normal((3, 65536), 21, std=1.0, dtype=torch.float32).double()
    x = (R + z).float().to(dt)
    var, skew, kurt = rw.moments_ref(x)
    xd = x.to(dev)
    tol = rw.MOMENT_TOL[dt]
    fails = []
    for name, fn, want in (("variance", st.variance, var), ("skewness", st.skewness, skew), ("kurtosis", st.kurtosis, kurt)):
        try:
            _close(fn(xd, dim=-1), want, tol, f"{name} at mean / std = {R:g} {dn}")
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, fails
