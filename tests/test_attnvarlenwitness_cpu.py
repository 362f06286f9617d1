"""The test of the witnesses of tests/attn_varlen_witness.py, without a GPU, in the pattern of tests/test_attnwitness_cpu.py: a mutant is
judged slice by slice - one (head, 128-row block) mutated, everything else clean - and every touched slice must break the claimed gate.

Which witness is claimed to catch which mutant of ONE sequence of a pack (thresholds: 4x for witness A's integer gates, 10x elsewhere):

  mutant                                                             caught by
  1  causal limit + 1 / - 1 key                                      A: exp(lse);  B ascending: out
  2  coff = sk - sq taken from the next sequence                     A: exp(lse);  B ascending: out
  3  the next sequence's first key visible (the descriptor's         A: exp(lse)
     range one row too long)
  4  the sequence's last key hidden                                  A: exp(lse);  B ascending: out (plain: every row; causal: the last)
  5  a 64-key tile dropped at a tile seam of a sequence that         A: exp(lse), out Z
     starts at a token offset that is no multiple of 64
  6  the K/V head of the neighbouring group                          A: out Z (the spare class);  C: out
  7  lse and delta of head h + 1 read by the backward                C: dV, dQ
  8  a row block served as the block the launch's count gives        A: exp(lse);  B ascending: out
     (nqblk - 1 - qi from max_seqlen) instead of the sequence's own
  9  the rows of a dK/dV key block started one query tile late       A: dV Z / dV [fp16];  B code: dV
     (tq0 off by one)

Then: the unmutated reference passes every judge for each pack and witness; an integer model of the item maps (block_to_work,
causal_head_group, block_to_work_grouped, the launch sizes of csrc/fasn_attnvarlen.hip) serves every (sequence, head, block) in range
exactly once in the regime each pack is named for; tests/attn_emulate.py stays at or below 0.5 of witness C's gates on two sequences of
LONG8; and the launch plans of the packs are pinned in tests/golden/attn_varlen_witness_plans.txt."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_witness as aw          # noqa: E402
import attn_varlen as av           # noqa: E402
import attn_varlen_witness as vw   # noqa: E402
from attn_emulate import emulate as _emulate   # noqa: E402

CPU = torch.device("cpu")
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


class SeqWorld:
    """one sequence of a pack's world with the attributes tw.assert_caught and attn_emulate.emulate read"""

    def __init__(self, w, b):
        self.w, self.b = w, b
        self.case, self.inp, self.r, self.g = w.seq[b]
        self.dt, self.bwd, self.wit, self.form = w.dt, w.backward, w.wit, w.form
        self.keep, self.p_eff = None, 0.0
        self.clean = aw.as_result(self.case, self.r, self.dt, backward=self.bwd)
        self.clean64 = aw.as_result(self.case, self.r, torch.float64, backward=self.bwd)

    def ref(self, **kw):
        return aw.reference(self.case, self.inp, backward=self.bwd, **kw)

    def judge(self, res):
        try:
            return vw.judge_seq(self.w, self.b, res)
        except aw.GateRefused:
            return aw.Ratios(refused=math.inf)


class tw:
    """the slice judge of tests/test_attnwitness_cpu.py, restated for one sequence (no test module imports another)"""
    RB = 128

    @staticmethod
    def assert_caught(s, mut_r, keys, thr, what, fwd=True, kv=True, exact=False):
        """every slice (head, 128 rows; and the K/V head of that head in dK, dV) in which the mutated result differs from the clean one
        breaks one of the gates `keys` by `thr`. exact: the mutated result is not rounded to the output type (witness A's integer gates:
        one count is four gates up to the last ulps of fp64, hence the 1e-12)"""
        if exact:
            thr = thr * (1 - 1e-12)
        case, clean = s.case, (s.clean64 if exact else s.clean)
        mut = aw.as_result(case, mut_r, torch.float64 if exact else s.dt, backward=s.bwd) if "_ops" in mut_r else mut_r
        row_keys = (("out", "lse") if fwd else ()) + (("dq",) if s.bwd else ())
        touched, worst = 0, math.inf
        for h in range(case.H):
            hk = h // case.G
            for r0 in range(0, case.L, tw.RB):
                rows = slice(r0, min(r0 + tw.RB, case.L))
                differs = any(not torch.equal(mut[k][0, h, rows], clean[k][0, h, rows]) for k in row_keys)
                if s.bwd and kv and r0 == 0:
                    differs |= not (torch.equal(mut["dk"][0, hk], clean["dk"][0, hk]) and torch.equal(mut["dv"][0, hk], clean["dv"][0, hk]))
                if not differs:
                    continue
                touched += 1
                res = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in clean.items()}
                for k in row_keys:
                    res[k][0, h, rows] = mut[k][0, h, rows]
                if s.bwd and kv:
                    res["dk"][0, hk], res["dv"][0, hk] = mut["dk"][0, hk], mut["dv"][0, hk]
                rat = s.judge(res)
                best = max(rat.get(k, 0.0) for k in tuple(keys) + ("refused",))
                worst = min(worst, best)
                assert best >= thr, (what, h, r0, dict(rat))
        assert touched, f"{what}: the mutant changes nothing"
        print(f"{what}: {touched} slices touched, the weakest breaks {' / '.join(keys)} by {worst:.3g}x")


_SEQ = {}


def seq_world(wp, b, wit, dtype, causal, form=None, std=None, keep=True):
    """keep: the mutant tests share their (short) sequences; the tests that walk every sequence of a pack, the 1100-long ones included,
    build each world for themselves and drop it"""
    key = (wp.key, b, wit, dtype, causal, form, std)
    if key in _SEQ:
        return _SEQ[key]
    bwd = not (wit == "B" and not form.startswith("code"))
    s = SeqWorld(vw.World(wp, wit, DT[dtype], CPU, causal, form, std, seed=3, backward=bwd, only=(b,)), b)
    if keep:
        _SEQ[key] = s
    return s


# ---------------------------------------------------------------- 1. the unmutated reference passes every judge
PACKS = {"LONG8 self": lambda: vw.long8(2), "LONG8 unequal": lambda: vw.long8(2, True), "LONG4": lambda: vw.long4(8, 1), "MANY": lambda: vw.many()}
# (the sequences judged here: every live sequence of the long packs; of MANY one of each length at either end)
SHORT = {"LONG8 self": (0, 2, 3, 4, 5, 6, 7), "LONG8 unequal": (0, 3, 4, 5, 6, 7), "LONG4": (0, 1, 2, 3), "MANY": (0, 1, 2, 4, 509, 510)}
UNMUTATED = [("A", None, None), *[("B", f, None) for f in aw.B_FORMS], ("C", None, 4), ("C", None, 8)]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("wit,form,std", UNMUTATED)
@pytest.mark.parametrize("pack_name", list(PACKS))
def test_unmutated_reference_passes(pack_name, wit, form, std, causal):
    wp = PACKS[pack_name]()
    for dtype in ("fp16", "bf16"):
        rat, kinds = aw.Ratios(), set()
        assert pack_name == "MANY" or list(SHORT[pack_name]) == wp.live()
        for b in SHORT[pack_name]:
            s = seq_world(wp, b, wit, dtype, causal, form, std, keep=False)
            one = vw.judge_seq(s.w, b, s.clean, kinds=kinds)
            for key, val in one.items():
                rat.up(key, val)
        print(f"{pack_name} {wit} {form or std or ''} {dtype} {'causal' if causal else 'plain'}: rounded reference at {rat}; kinds {sorted(kinds)}")
        assert rat.worst() <= {"A": 0.8 + 1e-9, "B": 1.0, "C": 0.5}[wit], dict(rat)
        if wit == "B":
            assert 1 in kinds or form == "code_sink"
            assert 2 in kinds or "sink" not in form
            if causal and pack_name == "LONG8 unequal":
                assert 0 in kinds, "sq > sk causal: rows that see nothing in a head without a sink"
        if wit == "A" and not causal and dtype == "fp16" and pack_name == "LONG8 self":
            assert "dV Z" in rat, "the sequence of 300 keys: Z = 512"


def test_whole_pack_round_trip():
    """as_raw -> cut -> judge over a whole pack, its empty sequences and tail included: the layout code of the GPU file"""
    wp = vw.WPack("tiny", [70, 0, 5, 130, 3], [40, 9, 0, 130, 300], H=4, Hkv=2, tail=7)
    for wit, form, std in (("A", None, None), ("B", "code", None), ("C", None, 4)):
        w = vw.world(wp, wit, torch.float16, CPU, True, form, std, seed=1)
        rat, kinds = vw.judge(w, vw.as_raw(wp, w))
        print(f"tiny {wit}: {rat}")
        assert rat.worst() <= 1.0 and "dn" in rat
    raw = vw.as_raw(wp, w)
    raw["dk"][wp.pack.cu_k[1]] = 1.0     # a key row of the sequence without queries
    with pytest.raises(AssertionError, match="without queries"):
        vw.judge(w, raw)
    raw = vw.as_raw(wp, w)
    raw["lse"][1, wp.pack.cu_q[-1]] = 0.0
    with pytest.raises(AssertionError, match="behind the last sequence"):
        vw.judge(w, raw)


# ---------------------------------------------------------------- 2. the mutants
U8 = lambda: vw.long8(2, True)   # noqa: E731
S8 = lambda: vw.long8(2)         # noqa: E731


def _tril(case, diag):
    return aw.visible_set(case.L, case.S, False).tril(diag).view(1, 1, case.L, case.S)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("delta", [1, -1])
def test_1_causal_limit(delta, dtype):
    for wp, b in ((S8(), 6), (U8(), 7), (U8(), 3)):   # 300 x 300, 959 x 31 (sq > sk), 517 x 1100 (sq < sk)
        if not vw.a_integer(wp.case(b, True), DT[dtype]):
            continue
        s = seq_world(wp, b, "A", dtype, True)
        tw.assert_caught(s, s.ref(w=_tril(s.case, s.case.S - s.case.L + delta)), ("exp(lse)",), 10, f"1 A seq {b} limit {delta:+d} {dtype}", kv=False)
        s = seq_world(wp, b, "B", dtype, True, "ascending")
        tw.assert_caught(s, s.ref(w=_tril(s.case, s.case.S - s.case.L + delta)), ("out",), 10, f"1 B ascending seq {b} limit {delta:+d} {dtype}")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_2_coff_of_the_next_sequence(dtype):
    wp = vw.WPack("close", [300, 297, 64], [300, 300, 64], H=4, Hkv=2)   # two close lengths: coff 0 and 3
    p = wp.pack
    for b in (0, 1):
        nxt = p.lens_k[b + 1] - p.lens_q[b + 1]
        s = seq_world(wp, b, "A", dtype, True)
        assert nxt != s.case.S - s.case.L
        tw.assert_caught(s, s.ref(w=_tril(s.case, nxt)), ("exp(lse)",), 10, f"2 A seq {b} coff {nxt} of the next sequence {dtype}", kv=False)
        s = seq_world(wp, b, "B", dtype, True, "ascending")
        tw.assert_caught(s, s.ref(w=_tril(s.case, nxt)), ("out",), 10, f"2 B ascending seq {b} coff of the next sequence {dtype}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_3_next_sequences_first_key_visible(dtype, causal):
    wp, b = S8(), 6
    s = seq_world(wp, b, "A", dtype, causal)
    nxt = seq_world(wp, 7, "A", dtype, causal)
    case2 = s.case.but(S=s.case.S + 1)
    inp2 = dict(s.inp)
    for x in ("k", "v"):
        inp2[x] = torch.cat([s.inp[x], nxt.inp[x][:, :, :1]], dim=2)
    w = torch.cat([aw.weights(s.case, None), torch.ones(1, 1, s.case.L, 1, dtype=torch.float64)], dim=-1)   # (causal: the clipped row lies behind every limit, and is seen)
    mut = aw.as_result(case2, aw.reference(case2, inp2, w=w, backward=False), s.dt, backward=False)
    res = {**s.clean, "out": mut["out"], "lse": mut["lse"]}
    tw.assert_caught(s, res, ("exp(lse)",), 10, f"3 A the next sequence's first key visible {dtype}", kv=False)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_4_last_key_hidden(dtype, causal):
    wp, b = U8(), 6
    for wit, form, keys in (("A", None, ("exp(lse)",)), ("B", "ascending", ("out",))):
        s = seq_world(wp, b, wit, dtype, causal, form)
        w = aw.weights(s.case, None).clone()
        w[..., s.case.S - 1] = 0
        tw.assert_caught(s, s.ref(w=w), keys, 10, f"4 {wit} the last key hidden {dtype}", kv=False)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_5_tile_dropped_at_a_seam(dtype):
    wp, b = S8(), 6
    assert wp.pack.cu_k[b] % 64 != 0
    for causal in (False, True):
        s = seq_world(wp, b, "A", dtype, causal)
        for t in (1, 3):
            w = aw.weights(s.case, None).clone()
            w[..., t * aw.KT:(t + 1) * aw.KT] = 0
            mut = s.ref(w=w)
            tw.assert_caught(s, mut, ("exp(lse)",), 10, f"5 A tile {t} dropped {dtype}", kv=False)
            tw.assert_caught(s, mut, ("out Z",), 4, f"5 A tile {t} dropped {dtype} out Z", kv=False, exact=True)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_6_kv_head_of_the_neighbouring_group(dtype):
    wp, b = S8(), 6
    for wit, std, keys, thr in (("A", None, ("out Z",), 4), ("C", 4, ("out",), 10)):
        s = seq_world(wp, b, wit, dtype, False, None, std)
        tw.assert_caught(s, s.ref(swap_kv=True), keys, thr, f"6 {wit} neighbouring K/V head {dtype}", kv=False)


def _backward_with_stats_of_next_head(s):
    """the closed-form backward of the sequence with lse and delta of head h + 1 (the reference's own P, dP: docstring of attn_witness)"""
    r, scale = s.r, s.inp["scale"]
    q, k, v, do = r["_ops"]
    lse, delta = r["lse"][0].roll(-1, 0), r["delta"][0].roll(-1, 0)
    P = torch.where(torch.isfinite(r["x"][0]), torch.exp(r["x"][0] - lse.unsqueeze(-1)), torch.zeros_like(r["x"][0]))
    dS = P * (r["dP"][0] - delta.unsqueeze(-1))
    mut = dict(r)
    mut.update(dV=(P.transpose(1, 2) @ do[0]).unsqueeze(0), dQ=(scale * (dS @ k[0])).unsqueeze(0), dK=(scale * (dS.transpose(1, 2) @ q[0])).unsqueeze(0))
    return mut


@pytest.mark.parametrize("std", [4, 8])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_7_lse_and_delta_of_the_next_head(dtype, std):
    wp, b = S8(), 6
    s = seq_world(wp, b, "C", dtype, True, None, std)
    tw.assert_caught(s, _backward_with_stats_of_next_head(s), ("dV", "dQ"), 10, f"7 C std {std} lse / delta of head h + 1 {dtype}", fwd=False)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_8_block_order_of_the_launch(dtype):
    wp, b = S8(), 3   # 517 rows: 5 blocks where the launch (max_seqlen 1100) has 9
    nq_launch, nq = -(-wp.pack.max_q // vw.BLOCK), -(-wp.pack.lens_q[b] // vw.BLOCK)
    assert nq_launch > nq > 1
    for wit, form, keys in (("A", None, ("exp(lse)",)), ("B", "ascending", ("out",))):
        s = seq_world(wp, b, wit, dtype, True, form)
        src = aw.weights(s.case, None)
        w = src.clone()
        for qi in range(nq_launch):   # item qi: rows of block nq_launch - 1 - qi, served as if they were the sequence's block nq - 1 - qi
            rows_blk, as_blk = nq_launch - 1 - qi, nq - 1 - qi
            if rows_blk >= nq:
                continue
            n = min(vw.BLOCK, s.case.L - rows_blk * vw.BLOCK)
            if as_blk < 0:
                w[..., rows_blk * vw.BLOCK:rows_blk * vw.BLOCK + n, :] = 0
            else:
                n = min(n, s.case.L - as_blk * vw.BLOCK)
                w[..., rows_blk * vw.BLOCK:rows_blk * vw.BLOCK + n, :] = src[..., as_blk * vw.BLOCK:as_blk * vw.BLOCK + n, :]
        tw.assert_caught(s, s.ref(w=w), keys, 10, f"8 {wit} blocks in the launch's order {dtype}", kv=False)


def test_9_dkdv_rows_one_tile_late():
    QT = 64
    wp, b = S8(), 6
    for wit, form, keys, thr in (("A", None, ("dV Z", "dV"), 4), ("B", "code", ("dV",), 10)):
        for causal in ((False, True) if wit == "B" else (False,)):   # (A's integer gate on dV Z: non-causal; causal under B)
            s = seq_world(wp, b, wit, "fp16", causal, form)
            mut = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.clean.items()}
            for kblk in range(-(-s.case.S // vw.BLOCK)):
                first = kblk * vw.BLOCK - (s.case.S - s.case.L) if causal else 0
                tq0 = 0 if first <= 0 else first // QT
                rw = torch.ones(1, s.case.H, s.case.L, dtype=torch.float64)
                rw[:, :, tq0 * QT:(tq0 + 1) * QT] = 0
                late = aw.as_result(s.case, s.ref(row_w=rw), s.dt)
                keys_of = slice(kblk * vw.BLOCK, (kblk + 1) * vw.BLOCK)
                mut["dk"][:, :, keys_of], mut["dv"][:, :, keys_of] = late["dk"][:, :, keys_of], late["dv"][:, :, keys_of]
            tw.assert_caught(s, mut, keys, thr, f"9 {wit} dK/dV rows one tile late {'causal' if causal else 'plain'}", fwd=False, exact=False)


# ---------------------------------------------------------------- 3. the item maps
REGIME = {   # variant -> (dQ: G under causal, 8-aligned), (dK/dV: G under causal, 8-aligned)
    "LONG8 self Hkv=4": ((4, True), (4, True)), "LONG8 self Hkv=2": ((4, True), (2, True)), "LONG8 self Hkv=1": ((4, True), (1, True)),
    "LONG8 unequal Hkv=4": ((4, True), (4, True)), "LONG8 unequal Hkv=2": ((4, True), (2, True)), "LONG8 unequal Hkv=1": ((4, True), (1, True)),
    "LONG4 H=8 Hkv=1": ((4, True), (1, False)), "LONG4 H=4 Hkv=4": ((2, True), (2, True)), "LONG4 H=3 Hkv=3": ((1, False), (1, False)),
    "MANY": ((4, True), (4, True)),
}
HINTS = (None, (2048, 1100), (1100, 2500), (4096, 4096))


def _check_items(wp, m, kern):
    p = wp.pack
    side, heads = (p.lens_k, wp.Hkv) if kern == "dkdv" else (p.lens_q, wp.H)
    items = m[kern]["items"]
    assert len(items) == m[kern]["grid"] == m[kern]["nbh"] * m[kern]["nblk"]
    assert len(set(items)) == len(items), f"{kern}: an item is served twice"
    assert all(0 <= b < p.B and 0 <= h < heads and 0 <= blk < m[kern]["nblk"] for b, h, blk in items), f"{kern}: an item out of range"
    need = {(b, h, blk) for b in range(p.B) for h in range(heads) for blk in range(-(-side[b] // vw.BLOCK))}
    assert need <= set(items), f"{kern}: a block with a row in range is not served"


@pytest.mark.parametrize("name", list(vw.VARIANTS))
def test_item_maps_serve_every_block_once(name):
    wp = vw.VARIANTS[name]()
    (gq, aq), (gk, ak) = REGIME[name]
    for causal in (False, True):
        for hints in (HINTS if name.startswith("LONG8") else (None,)):
            m = vw.item_model(wp, causal, hints)
            for kern in ("fwd", "dq", "dkdv"):
                _check_items(wp, m, kern)
            if hints is None:
                assert (m["dq"]["G"], m["dq"]["aligned"]) == (gq if causal else 1, aq), (name, causal, m["dq"]["G"])
                assert (m["dkdv"]["G"], m["dkdv"]["aligned"]) == (gk if causal else 1, ak), (name, causal, m["dkdv"]["G"])
                assert m["fwd"]["aligned"] == aq
    if name == "MANY":
        assert vw.item_model(wp, True)["fwd"]["grid"] == 2048


def test_item_maps_reach_every_regime():
    seen = {"dq": set(), "dkdv": set()}
    for name, make in vw.VARIANTS.items():
        m = vw.item_model(make(), True)
        for kern in seen:
            seen[kern].add((m[kern]["G"], m[kern]["aligned"]))
    for kern in seen:
        assert {g for g, _ in seen[kern]} == {1, 2, 4}, (kern, seen[kern])
        assert {a for _, a in seen[kern]} == {True, False}, (kern, seen[kern])
    # the heaviest-first walk: a causal sequence's last block is the first of its head to be handed out
    m = vw.item_model(vw.long8(4), True)
    first = {}
    for pos, (b, h, blk) in enumerate(m["dq"]["items"]):
        if blk * vw.BLOCK < vw.LONG8_Q[b]:
            first.setdefault((b, h), blk)
    assert all(blk == -(-vw.LONG8_Q[b] // vw.BLOCK) - 1 for (b, h), blk in first.items())


def test_model_is_the_source():
    """a tripwire: the expressions the model restates are still in the sources (compared without white space)"""
    root = os.path.join(av.ROOT, "flash-attention-softmax-n_amd", "csrc")

    def text_of(name):
        with open(os.path.join(root, name)) as fh:
            return "".join(fh.read().split())

    def has(text, expr):
        assert "".join(expr.split()) in text, expr

    text = text_of("fasn_common.h")
    for expr in ("bh = (j / nblk_per_head) * 8 + xcd;", "while (g < 4 && (hx % (2 * g)) == 0 && 2L * g * per_head <= (4L << 20)) g *= 2;",
                 "const long per_head = 4L * rows * D;", "blk = r / G;", "bh = (g * G + r % G) * 8 + xcd;"):
        has(text, expr)
    text = text_of("fasn_attnvarlen.hip")
    for expr in ("constexpr int kBlock = 128;", "dim3((unsigned)(nqblk * p.B * p.H))", "dim3((unsigned)(nqblk * nbh))", "dim3((unsigned)(nkblk * (nbh / p.f.kvg)))"):
        has(text, expr)
    text = text_of("fasn_bwd_kernel.h")
    has(text, "causal_head_group(p.B * p.H, p.Sk, D)")
    has(text, "causal_head_group(p.B * Hkv, p.Sq * kvg, D)")


# ---------------------------------------------------------------- 4. the kernels' arithmetic stays under the gates
@pytest.mark.parametrize("std", [4, 8])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("which", ["sq > sk causal", "1100 long"])
def test_c_gates_hold_for_the_kernels_arithmetic(which, dtype, std):
    wp, b, causal = (vw.long8(2, True), 7, True) if which == "sq > sk causal" else (vw.long8(2), 0, True)
    s = seq_world(wp, b, "C", dtype, causal, None, std, keep=False)
    rat = aw.judge_c(s.case, s.dt, _emulate(s), s.r, s.g)
    print(f"C {which} std {std} {dtype}: emulated kernel arithmetic at {rat} of the gates")
    assert rat.worst() <= 0.5, dict(rat)


# ---------------------------------------------------------------- 5. the plans
def test_plans_match_the_golden_file(pkg, golden_dir):
    with open(os.path.join(golden_dir, "attn_varlen_witness_plans.txt")) as fh:
        assert vw.plans_file_text(pkg) == fh.read(), "the launch plans of the witness packs changed: tests/golden/attn_varlen_witness_plans.txt"


def test_plans_agree_with_the_model(pkg):
    text = vw.plans_file_text(pkg)
    assert " rc=-" not in text and "_ws" not in text
    for name, make in vw.VARIANTS.items():
        m = vw.item_model(make(), True)
        blk = text.split(f"{name} causal bf16 [fwd] ok\n")[1].split("\n" + name)[0]
        assert f"grid={m['fwd']['grid']}" in blk and "fasn_fwd_kernel<" in blk, (name, blk)
        blk = text.split(f"{name} causal bf16 [bwd] ok\n")[1]
        lines = blk.splitlines()[:3]
        assert "fasn_bwd_dq_kernel<" in lines[1] and lines[1].endswith(f"grid={m['dq']['grid']}"), (name, lines)
        assert "fasn_bwd_dkdv_kernel<" in lines[2] and lines[2].endswith(f"grid={m['dkdv']['grid']}"), (name, lines)
