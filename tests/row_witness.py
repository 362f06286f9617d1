"""Witnesses for the two stand-alone row kernels, softmax_n (csrc/fasn_softmax.hip) and the power sums behind statistics.* (csrc/fasn_moments.hip):
fp64 references written from the formulas alone, per-element gates derived below, operands where one count or one entry decides a row, and
the table of cases that puts a row on either side of every dispatch threshold. A helper module (no test is collected from it):
tests/test_gpu_rowops.py runs the kernels, tests/test_rowops_cpu.py is the test of these tests.

The formulas.
    y_i = e^(x_i - m) / (n e^-m + sum_j e^(x_j - m)),   m = max_j x_j, at least 0 when n > 0, and 0 when the row is wholly -inf;
    at n == 0 the n term is absent (not 0 * e^-m: e^-m overflows below m = -88.7 in fp32), so softmax_n(x, 0) = softmax(x);
    a wholly -inf row is exactly 0 when n > 0 (0 / n) and NaN when n == 0 (0 / 0, as torch.softmax).
    dx_i = y_i (dy_i - sum_j dy_j y_j).
    power sums S_k = sum_j (x_j - x_0)^k, k = 1 .. 4, about the row's first element; central moments by two passes in fp64.

The gates. u is the unit roundoff of the tensor's type (U below: 2^-8 bf16, 2^-11 fp16, 2^-24 fp32; one rounding to nearest moves a value by
at most u of itself) and t the underflow step: T of the type (half the spacing of its subnormals, 2^-25 fp16, 2^-134 bf16, 2^-150 fp32: what one
rounding may move a value below the normal range by) plus 2^-149 for the last fp32 product, which may fall below fp32's normal range first. K is the number of fp32 additions on the longest path of the sum in the kernel that
the plan names (depth()): the terms one thread adds in sequence, 6 shuffle levels, and 3 more where four waves meet in LDS.

  forward.  |y - y_ref| <= y_ref (u + d_i + sum_j p_j d_j + s (2 + 2 |m|) 2^-24 + (K + 4) 2^-24) + floor + t.
      d_i = (4 + 5 |x_i - m|) 2^-24: the exponent (x_i - m) log2 e is formed by a subtraction and a product (at most 2^-24 |x_i - m| each, in
            nats) with a constant that is itself rounded (half of that): 2.5 |x_i - m| at worst, and fp32 rows 64 nats deep come to 1.9 of it.
            The gate grants twice the worst case, 5, so that the emulated arithmetic sits at or below half of it. v_exp_f32 is good to
            1 ulp = 2 * 2^-24, likewise doubled: 4. (The kernels once formed the exponent as fma(x, log2 e, -round(m log2 e)): one rounding
            less per element, but the rounding of m log2 e, 2^-24 |m|, in every exponent of the row - no bound in |x_i - m| covers that.)
      sum_j p_j d_j: the same errors in the denominator's terms, weighted by the reference's probabilities p_j = y_ref_j.
      s (2 + 2 |m|) 2^-24: the n term n e^-m is one more exponential (argument -m log2 e: a product with the rounded constant, and 1 ulp)
            and one product; it enters the denominator with its share s = n e^-m / denominator.
      (K + 4) 2^-24: K additions of the sum, the addition of the n term, the reciprocal, the product e_i * (1 / denominator), and one to spare.
      floor = 2^-120 / denominator: v_exp_f32 has no subnormal results, an exponential below 2^-126 comes out as 0; 2^-120 is the numerator
            lost that way, with room for 63 such terms of the sum.
      Where x_i = -inf the expected value is exactly 0 and the bound is 0.
  backward. The kernel under test is the backward, so its reference uses the y it was given (the forward's output tensor, widened exactly):
      |dx - dx_ref| <= (u + 3 * 2^-24) |dx_ref| + y_i (K + 2) 2^-24 sum_j |y_j dy_j| + t:
      the output rounding, the subtraction dy_i - dot and the product with y_i relative to the result, and the dot product's K fused
      multiply-adds (plus two to spare) relative to sum |y_j dy_j|, times y_i.
  power sums on integer-valued data: equality, bit for bit (every term and every partial sum is an integer below 2^53).
  moments on random data: tests/test_statistics.py's tolerances, relative and absolute, from the cast of the result to x.dtype (MOMENT_TOL).

The operands.
  A  counting. x is 0 at visible entries and -inf at hidden ones, so y_i (n + c_row) = 1 at visible entries and exactly 0 at hidden ones: a
     dropped vector, a tail read twice or padding lanes entering the sum move c_row by at least 1. Rows go by r mod 5: one visible entry at
     t(r) = (7 r + 3) mod cols; all visible; none visible (n > 0; at n == 0 the last entry alone); a sparse row - entry 0, the first entry of the
     last 16-byte vector, the last entry and pseudo-random others, at most SPARSE[dtype] in all; a pseudo-random half with the last entry.
     One count shows by 10 gates only where 1 / (n + c_row) >= 10 u: the sparse rows are kept that short (8 bf16, 64 fp16 and fp32); the
     output type itself cannot tell 4096 from 4097 equal entries in bf16. The backward takes dy = 1: dx_i = y_i n / (n + c_row), which is
     0 at n = 0 and leaves the gate's cancellation term alone.
  B  one entry decides. spike: x = 0 but x[r, t(r)] = 64: y[r, t] is 1 to a rounding, every other entry at most e^-64. negative (n > 0):
     x = -64 - (c mod 5): m is clamped to 0, y_i = e^x_i / (n + sum e^x_j), about 1e-28 / n - in fp16 it underflows and the gate's t = 2^-25
     says |y| <= 2^-24 there. negative0 (n == 0): x = -100 - (c mod 5), a plain softmax although e^100 is inf in fp32. large: x = 85 +
     (c mod 3) in fp32, 60000 - 8 (c mod 4) in fp16, 1e30 (1 + (c mod 2)) in bf16: e^-m underflows, m log2 e loses digits.
  C  dynamic range: synth.counter_normal at a standard deviation of 4, 8 and 16, dy at 1, n in {0, 1e-3, 1, 4}."""
import math
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
CODE = {"fp16": 0, "bf16": 1, "fp32": 2}   # FASN_DTYPE_*
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
T = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150}
ESZ = {torch.bfloat16: 2, torch.float16: 2, torch.float32: 4}
SPARSE = {torch.bfloat16: 8, torch.float16: 64, torch.float32: 64}
MOMENT_TOL = {torch.float32: 2e-5, torch.float16: 2e-3, torch.bfloat16: 1.6e-2}
E24 = 2.0 ** -24
ROWS = 5   # not a multiple of the wave kernels' 4 rows per workgroup: the second workgroup holds one live wave
FWD, BWD = 0, 1
DIRS = {"fwd": FWD, "bwd": BWD}


def epv(dtype):
    return 16 // ESZ[dtype]


def _f64(t):
    return t.detach().to("cpu", torch.float64)


# ---------------------------------------------------------------- the cases: every dispatch seam, every way into the element-load kernels
class Case:
    """x = base[:, lead:lead + cols] of a [rows, width] tensor; lead = 0 and width = cols is the contiguous case"""

    def __init__(self, cols, lead=0, width=None, rows=ROWS):
        self.rows, self.cols, self.lead, self.width = rows, cols, lead, cols if width is None else width
        assert self.lead + cols <= self.width

    def key(self, direction, dtype_name):
        return f"{direction} {dtype_name} rows={self.rows} cols={self.cols} lead={self.lead} width={self.width}"

    def view(self, t):
        """the case's view of `t` [rows, cols]: a copy inside a wider NaN-filled tensor, or t itself"""
        if self.lead == 0 and self.width == self.cols:
            return t.contiguous()
        base = torch.full((self.rows, self.width), math.nan, dtype=t.dtype, device=t.device)
        base[:, self.lead:self.lead + self.cols] = t
        return base[:, self.lead:self.lead + self.cols]


SEAMS16 = {"fwd": (8, 1016, 1024, 1032, 2048, 2056, 4096, 4104, 8192, 8200, 16384, 16392, 32768, 32776),
           "bwd": (1024, 1032, 2048, 2056, 4096, 4104, 8192, 8200, 16384, 16392, 32768, 32776)}
ELEMENT_COLS = (1, 3, 255, 257, 4095, 4097)


def cases(direction, dtype_name):
    """the seam shapes (fp32: halved, its vector holds 4), then the element-load shapes, then the four views"""
    half = 2 if dtype_name == "fp32" else 1
    out = [Case(c // half) for c in SEAMS16[direction]]
    out += [Case(c) for c in ELEMENT_COLS]
    out += [Case(4096, 1, 4097), Case(4104, 1, 4105),   # x[:, 1:]: a base off 16 bytes and an odd stride
            Case(1024, 8, 1040),                        # aligned, stride != cols: still the wave kernel
            Case(1024, 4, 1040)]                        # 8 bytes off at 16 bit: element loads (fp32: 16 bytes, the wave kernel)
    return out


def plan_of_case(L, case, direction, dtype_name):
    """the plan of the case from numbers alone (no tensor): every operand of the call in the case's geometry at an address that is 4096 plus
    the view's offset"""
    esz = ESZ[DTYPES[dtype_name]]
    p = 4096 + case.lead * esz
    return L.softmax_plan(DIRS[direction], p, p, p, case.rows, case.cols, case.width, case.width, case.width, CODE[dtype_name])


def plan_of_tensors(L, direction, a, b, c=None):
    """the plan of the call on these 2-D tensors (forward: x, y; backward: y, dy, dx)"""
    name = {v: k for k, v in DTYPES.items()}[a.dtype]
    cp, cs = (c.data_ptr(), c.stride(0)) if c is not None else (16, a.shape[1])
    return L.softmax_plan(DIRS[direction], a.data_ptr(), b.data_ptr(), cp, a.shape[0], a.shape[1], a.stride(0), b.stride(0), cs, CODE[name])


def plan_line(plan):
    (name, grid, block, lds), = plan
    return f"{name} grid={grid} block={block} lds={lds}"


def plan_table(L):
    """the golden file's lines: every case of every direction and dtype, and the moments cases"""
    lines = []
    for direction in ("fwd", "bwd"):
        for dn in DTYPES:
            for case in cases(direction, dn):
                lines.append(f"{case.key(direction, dn)} | {plan_line(plan_of_case(L, case, direction, dn))}")
    for dn in DTYPES:
        for rows, cols in MOMENT_SHAPES:
            lines.append(f"moments {dn} rows={rows} cols={cols} | {plan_line(L.moments_plan(4096, 4096, rows, cols, cols, CODE[dn]))}")
    return lines


def selectable(direction, dtype_name):
    """every template instantiation the launchers can select, as the plans name them"""
    d, wave, block = CODE[dtype_name], {"fwd": (2, 4, 8, 16), "bwd": (2, 4, 8)}[direction], {"fwd": (8, 16), "bwd": (4, 8, 16)}[direction]
    return ({f"softmax_n_{direction}_kernel<{d}>"} | {f"softmax_n_{direction}_wave_kernel<{d}, {nv}>" for nv in wave}
            | {f"softmax_n_{direction}_block_kernel<{d}, {nv}>" for nv in block})


_NAME = re.compile(r"softmax_n_(fwd|bwd)_(wave_|block_|)kernel<(\d)(?:, (\d+))?>$")


def kernel_of(plan):
    """(direction, kind, NV) of a one-line plan: kind is "element", "wave" or "block" """
    m = _NAME.match(plan[0][0])
    assert m and len(plan) == 1, plan
    return m.group(1), {"": "element", "wave_": "wave", "block_": "block"}[m.group(2)], int(m.group(4) or 0)


def depth(plan, cols, dtype):
    """K: the fp32 additions on the longest path of the kernel's sum (forward) or dot product (backward)"""
    direction, kind, nv = kernel_of(plan)
    if kind == "wave":
        return nv * epv(dtype) + 6
    if kind == "block":
        return nv * epv(dtype) + 6 + 3
    per_thread = 16 if (direction == "fwd" and cols <= 4096) else -(-cols // 256)   # the register-cached forward adds all 16 slots
    return per_thread + 6 + 3


# ---------------------------------------------------------------- the references: fp64, from the formulas
def softmax_ref(x, n, w=None, extra=0.0, clamp=True, n_term=True):
    """x [rows, cols] (any type, widened exactly), n a float. Returns y, m, den, s (the n term's share of den) in fp64. The arguments
    after n are the faults tests/test_rowops_cpu.py injects: w [cols] or [rows, cols] counts entry j w_j times in the sum; `extra` is added
    to the sum (padding lanes as e^0); clamp=False shifts the exponentials by the unclamped maximum while the n term keeps the clamped one;
    n_term=False drops n e^-m."""
    x = _f64(x)
    top = x.amax(-1)
    m = top.clamp_min(0.0) if n > 0 else top.clone()
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    shift = m if clamp else torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    e = torch.exp(x - shift.unsqueeze(-1))
    total = (e if w is None else e * w).sum(-1) + extra
    sink = n * torch.exp(-m) if (n > 0 and n_term) else torch.zeros_like(m)
    den = sink + total
    return dict(y=e / den.unsqueeze(-1), m=m, den=den, s=sink / den, x=x)


def softmax_bwd_ref(y, dy, roll=0, no_dot=False):
    """dx in fp64 from the y and dy tensors as given; the faults: the dot product of row r + roll, or none"""
    y, dy = _f64(y), _f64(dy)
    dot = (y * dy).sum(-1, keepdim=True)
    if roll:
        dot = dot.roll(-roll, 0)
    if no_dot:
        dot = torch.zeros_like(dot)
    return dict(dx=y * (dy - dot), mass=(y * dy).abs().sum(-1, keepdim=True), y=y)


def power_sums_ref(x):
    """[rows, 4] int64: sum_j (x_j - x_0)^k of integer-valued x [rows, cols], in integer arithmetic"""
    xi = _f64(x).to(torch.int64)
    assert torch.equal(xi.double(), _f64(x))
    d = xi - xi[:, :1]
    return torch.stack([d.sum(-1), (d * d).sum(-1), (d * d * d).sum(-1), (d * d * d * d).sum(-1)], -1)


def moments_ref(x):
    """(variance, skewness, excess kurtosis) per row of x [rows, cols] by two passes in fp64 on the values as given"""
    x = _f64(x)
    d = x - x.mean(-1, keepdim=True)
    m2, m3, m4 = (d ** 2).mean(-1), (d ** 3).mean(-1), (d ** 4).mean(-1)
    return m2, m3 / m2 ** 1.5, m4 / m2 ** 2 - 3.0


# ---------------------------------------------------------------- the gates
def _ratio(err, bound):
    """largest err / bound; a bound of 0 is met by an error of 0 only; NaN (a value missing on one side) counts as inf"""
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return r


def forward_bound(ref, K, dtype, rounding=True):
    """the forward gate per element [rows, cols]; rounding=False leaves out the output's own rounding, u and t (what the fp32 arithmetic
    alone may use: t is then fp32's, a product below its normal range)"""
    x, m, y = ref["x"], ref["m"].unsqueeze(-1), ref["y"]
    hidden = torch.isinf(x) & (x < 0)
    d = torch.where(hidden, torch.zeros_like(x), (4 + 5 * (torch.where(hidden, m, x) - m).abs()) * E24)
    pd = (torch.where(hidden, torch.zeros_like(y), y) * d).sum(-1, keepdim=True)
    rel = (U[dtype] if rounding else 0.0) + d + pd + ref["s"].unsqueeze(-1) * (2 + 2 * m.abs()) * E24 + (K + 4) * E24
    bound = y * rel + 2.0 ** -120 / ref["den"].unsqueeze(-1) + (T[dtype] if rounding else 0.0) + 2.0 ** -149
    return torch.where(hidden, torch.zeros_like(bound), bound)


def gate_forward(y, ref, K, dtype, per_row=False, rounding=True):
    """largest ratio of |y - y_ref| to the forward gate (per row with per_row). A row the reference has as NaN (wholly -inf, n == 0) must be
    all NaN."""
    y = _f64(y)
    nan_rows = torch.isnan(ref["y"]).all(-1)
    assert torch.equal(torch.isnan(ref["y"]).any(-1), nan_rows)
    r = _ratio((y - ref["y"]).abs(), forward_bound(ref, K, dtype, rounding))
    r = torch.where(nan_rows.unsqueeze(-1), torch.where(torch.isnan(y), torch.zeros_like(r), torch.full_like(r, math.inf)), r)
    r = r.amax(-1)
    return r if per_row else r.max().item()


def gate_backward(dx, ref, K, dtype, per_row=False, rounding=True):
    """largest ratio of |dx - dx_ref| to the backward gate"""
    dx = _f64(dx)
    bound = ((U[dtype] if rounding else 0.0) + 3 * E24) * ref["dx"].abs() + ref["y"] * (K + 2) * E24 * ref["mass"] + (T[dtype] if rounding else 0.0) + 2.0 ** -149
    r = _ratio((dx - ref["dx"]).abs(), bound).amax(-1)
    return r if per_row else r.max().item()


# ---------------------------------------------------------------- the operands
def spike_at(rows, cols, dev="cpu"):
    return (7 * torch.arange(rows, device=dev) + 3) % cols


def _hash(rows, cols, dev):
    r = torch.arange(rows, device=dev, dtype=torch.int64).view(-1, 1)
    c = torch.arange(cols, device=dev, dtype=torch.int64).view(1, -1)
    return ((c * 2654435761 + r * 40503 + 12345) >> 7) & 0xFFFF


def visible_a(rows, cols, n, dtype, dev="cpu"):
    """[rows, cols] bool: witness A's visible entries (the row kinds of the module docstring, by r mod 5)"""
    r = torch.arange(rows, device=dev).view(-1, 1)
    c = torch.arange(cols, device=dev).view(1, -1)
    h = _hash(rows, cols, dev)
    kind = r % 5
    last, lastvec = c == cols - 1, c == max(cols - epv(dtype), 0)
    one = c == spike_at(rows, cols, dev).view(-1, 1)
    none = last if n == 0 else torch.zeros_like(last)
    keep = max(SPARSE[dtype] - 3, 0)
    sparse = (c == 0) | last | lastvec | (h * cols < keep * 65536)          # expected keep others: a density of keep / cols
    half = last | (h < 32768)
    vis = torch.where(kind == 0, one, torch.where(kind == 1, torch.ones_like(one), torch.where(kind == 2, none, torch.where(kind == 3, sparse, half))))
    return vis


def inputs_a(rows, cols, n, dtype, dev="cpu"):
    vis = visible_a(rows, cols, n, dtype, dev)
    x = torch.where(vis, 0.0, -math.inf).to(dtype)
    return dict(x=x, dy=torch.ones(rows, cols, dtype=dtype, device=dev), n=float(n), vis=vis)


B_FORMS = ("spike", "negative", "negative0", "large")
B_N = {"spike": 1.0, "negative": 1.0, "negative0": 0.0, "large": 1.0}


def inputs_b(rows, cols, form, dtype, dev="cpu", seed=5):
    from flash_attention_softmax_n_amd import synth
    c = torch.arange(cols, device=dev).view(1, -1).expand(rows, cols)
    if form == "spike":
        x = torch.zeros(rows, cols, device=dev)
        x[torch.arange(rows, device=dev), spike_at(rows, cols, dev)] = 64.0
    elif form == "negative":
        x = -64.0 - (c % 5).float()
    elif form == "negative0":
        x = -100.0 - (c % 5).float()
    else:
        assert form == "large"
        x = {torch.float32: 85.0 + (c % 3).float(), torch.float16: 60000.0 - 8.0 * (c % 4).float(), torch.bfloat16: 1e30 * (1 + (c % 2)).float()}[dtype]
    dy = synth.counter_normal((rows, cols), seed, std=1.0, dtype=dtype, device=dev)
    return dict(x=x.to(dtype).contiguous(), dy=dy, n=B_N[form])


C_STDS = (4, 8, 16)
C_NS = (0.0, 1e-3, 1.0, 4.0)


def inputs_c(rows, cols, std, n, dtype, dev="cpu", seed=9):
    from flash_attention_softmax_n_amd import synth
    return dict(x=synth.counter_normal((rows, cols), seed, std=float(std), dtype=dtype, device=dev),
                dy=synth.counter_normal((rows, cols), seed + 1, std=1.0, dtype=dtype, device=dev), n=float(n))


def expect_a(inp, ref):
    """the reference itself counts: y_i (n + c_row) = 1 at visible entries, 0 at hidden ones, NaN in a row without entries at n == 0"""
    vis, n = inp["vis"].cpu(), inp["n"]
    count = vis.sum(-1, keepdim=True).double()
    want = torch.where(vis, 1.0 / (n + count), torch.zeros_like(ref["y"]))
    assert torch.equal(torch.isnan(want), torch.isnan(ref["y"])) and ((want - ref["y"]).abs().nan_to_num(0.0) <= 1e-15).all()
    return count


# ---------------------------------------------------------------- moments: shapes and integer data
MOMENT_SHAPES = tuple((r, c) for r in (1, 3) for c in (1, 7, 8, 9, 4095, 4096, 4097, 8191, 8193, 12289)) + ((1, 2048 * 4096 + 9), (65535, 3))


def small_integers(shape, seed, dtype, dev="cpu"):
    """values from {+-1, +-2, +-3}: exact in every type, and 4th powers of differences are at most 6^4"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, 6, shape, generator=g)
    return torch.tensor([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0])[v].to(dtype).to(dev)
