"""The plain / key-padding D = 64 forward of the big-grid tuning point (64 rows per wave, 16x16x32 MFMA tiles: DESIGN 4.2, T16 in
csrc/fasn_fwd_kernel.h) at the smallest shapes that reach it: the dispatch wants B H ceil(L / 256) >= 512 and L >= 256. A query row
lives in four lanes (g = lane >> 4), register r of key chunk c holds key 16 c + 4 g + r of a 64-key tile, the row sum is a per-lane
partial, and the exact path reduces its maximum over the four lanes. What can go wrong there and nowhere else:
  - the key range ending inside a 16-key chunk, on a chunk edge, inside the second pair of chunks, on a tile edge, in the third tile;
  - row chunks (16 rows) that are partly filled or empty, and waves without rows;
  - the unseeded start (n = 0: exact path first, fast path after), a scalar n, a per-head n tensor;
  - a guard trip: a key far above everything before it, in the second tile, in each of the four lane groups - the tile is redone on
    the exact path, the maximum moves and O is rescaled in all four lanes of the row;
  - key-padding lengths that end inside a chunk, on an edge, and at one key;
  - the LSE the backward reads.
Runner, references and gates are those of tests/attn_witness.py (witness A: every visible key exactly once; B: one key decides;
C: per-element first-order bounds): no tolerance is introduced here. Every case asserts that the kernel is in its launch plan."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_witness as aw   # noqa: E402

pytestmark = pytest.mark.gpu
DT = ("bf16", "fp16")
# n per head (nshape "H"): the even heads have n = 0 (unseeded start), the odd ones a sink - both in every case below
KEYS = (1, 15, 16, 17, 31, 33, 64, 65, 130, 300)   # (300: L < S)
PADS = [130, 129, 17, 1]


def plain(S, L=256, B=8, **kw):
    return aw.Case(B, 64, L, S, 64, ub=2, uh=2, bwd=False, want=("D=64,QB=2,plain",), **kw)


KEYPAD = aw.Case(8, 64, 256, 130, 64, mask="keypad", lens=PADS, ub=4, uh=2, bwd=False, want=("D=64,QB=2,keypad",))


def in_plan(pkg, case, dtype):
    text = aw.plan_text(pkg, case, dtype)
    for w in case.want:
        assert w in text, (w, text)


def forward_a(pkg, dev, case, dtype, seed):
    dt = aw.DTYPES[dtype]
    inp = aw.inputs_a(case, dt, dev, seed)
    res = aw.run(pkg, case, inp, seed)
    r = aw.reference(case, inp, backward=False)
    cmax = aw.condition_a(case, r, dt, 0.0)
    rat = aw.judge_a(case, dt, res, r, None)
    print(f"A {case.L}x{case.S} {dtype}: largest class count {cmax:g}; ratios to the gates: {rat}")
    assert rat.worst() <= 1, str(rat)


def forward_c(pkg, dev, case, dtype, seed, std=8, n=None):
    dt = aw.DTYPES[dtype]
    inp = aw.inputs_c(case, std, dt, dev, seed)
    if n is not None:   # a scalar n for every head
        inp["n"], inp["un"] = float(n), torch.full((case.ub, case.uh), float(n), dtype=torch.float64)
    res = aw.run(pkg, case, inp, seed)
    r = aw.reference(case, inp, backward=case.bwd)
    g = aw.with_bounds(case, inp, r, aw.unit(case, dt), aw.unit_abs(dt))
    rat = aw.judge_c(case, dt, res, r, g)
    print(f"C {case.L}x{case.S} std {std} n {n} {dtype}: ratios to the gates: {rat}")
    assert rat.worst() <= 1, str(rat)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("S", KEYS)
def test_key_range(pkg, dev, S, dtype):
    case = plain(S)
    in_plan(pkg, case, dtype)
    forward_a(pkg, dev, case, dtype, 1600 + S)
    forward_c(pkg, dev, case, dtype, 1700 + S)


@pytest.mark.parametrize("dtype", DT)
def test_ragged_rows(pkg, dev, dtype):
    """L = 300: the last block of a head holds 44 rows - wave 0 two full, one partly filled and one empty row chunk, waves 1 - 3 none"""
    case = plain(130, L=300, B=4)
    in_plan(pkg, case, dtype)
    forward_a(pkg, dev, case, dtype, 1801)
    forward_c(pkg, dev, case, dtype, 1802)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", (0.0, 1.0, None))
def test_n_variants(pkg, dev, n, dtype):
    """a scalar n = 0 (every row starts unseeded), a scalar n = 1, and the per-head tensor (None)"""
    case = plain(130)
    in_plan(pkg, case, dtype)
    forward_c(pkg, dev, case, dtype, 1900, std=4, n=n)
    forward_c(pkg, dev, case, dtype, 1901, std=8, n=n)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("g", (0, 1, 2, 3))
def test_guard_trip_in_each_lane_group(pkg, dev, g, dtype):
    """Logits of standard deviation 1, and key t = 64 + 4 g + 1 - second tile, lane group g - at 48 nats (69 log2 units) through a
    feature of its own: its weight against the running maximum overflows the fast path's limit in ONE of the row's four lanes, the
    wave redoes the tile on the exact path and every lane of the row rescales. Witness B: the row is V[t] within 2 u."""
    case, dt, t = plain(130), aw.DTYPES[dtype], 64 + 4 * g + 1
    in_plan(pkg, case, dtype)
    inp = aw.inputs_c(case, 1, dt, dev, 2000 + g)
    inp["q"][..., -1] = 8.0
    inp["k"][..., -1] = 0.0
    inp["k"][:, :, t, -1] = 12.0   # scale 0.5: 48 nats on key t, nothing on the others
    res = aw.run(pkg, case, inp, 2000 + g)
    r = aw.reference(case, inp, backward=False)
    gate = aw.with_bounds(case, inp, r, aw.unit(case, dt), aw.unit_abs(dt))
    rat, kinds = aw.judge_b(case, "ascending", dt, res, r, gate, inp)
    print(f"B guard trip at key {t} {dtype}: row kinds {sorted(kinds)}; ratios to the gates: {rat}")
    assert kinds == {1}, kinds
    assert (r["x"].argmax(-1) == t).all()
    assert rat.worst() <= 1, str(rat)


@pytest.mark.parametrize("dtype", DT)
def test_key_padding(pkg, dev, dtype):
    in_plan(pkg, KEYPAD, dtype)
    forward_a(pkg, dev, KEYPAD, dtype, 2101)
    forward_c(pkg, dev, KEYPAD, dtype, 2102)


@pytest.mark.parametrize("dtype", DT)
def test_forward_then_backward(pkg, dev, dtype):
    """the LSE of the new tiling (four partial sums per row, combined in the epilogue) feeds the pipelined backward"""
    case = plain(130).but(bwd=True, want=("D=64,QB=2,plain", "fasn_bwd_dq_pipe_kernel", "fasn_bwd_dkdv_pipe_kernel"))
    in_plan(pkg, case, dtype)
    forward_c(pkg, dev, case, dtype, 2201, std=4)
