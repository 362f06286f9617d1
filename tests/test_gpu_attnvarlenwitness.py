"""The witnesses of tests/attn_varlen_witness.py on the GPU, through flash_attention_n_varlen and its backward: long packs (up to 9 blocks
per sequence), the grouped causal item map (G = 2 and 4), 512 sequences, loose hints, determinism, the front end's copy paths and token
rows a MiB apart.

Every expectation is the fp64 reference of tests/attn_witness.py per sequence, compared per row and per element in EVERY (sequence, head,
row) with sq_b > 0, under the gates derived there (A: integer counts; B: one key decides; C: first-order bounds at logit standard
deviations 4 and 8). Sequences with an empty side and the rows behind cu[B] are checked exactly (0, -inf, gradients 0; lse = log n of a
sequence without keys within the fp32 term of the lse gate: attn_varlen_witness.exact_rest). Each test prints its largest ratios
before it asserts <= 1. tests/test_attnvarlenwitness_cpu.py shows what each gate catches, which item-map regime each pack reaches and
that an emulation of the kernels' arithmetic stays at or below 0.5 of witness C's gates."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_witness as aw          # noqa: E402
import attn_varlen as av           # noqa: E402
import attn_varlen_witness as vw   # noqa: E402

pytestmark = pytest.mark.gpu
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
DTYPES = ["fp16", "bf16"]
MODES = [False, True]
TENSORS = ("out", "lse", "dq", "dk", "dv", "dn")


@pytest.fixture(scope="module", autouse=True)
def _release_shared_worlds():
    """the worlds that tests 4, 6 and 7 share are dropped when the module is done, with their operands on the device"""
    yield
    vw.forget_worlds()


def _go(pkg, dev, wp, wit, dtype, causal, form=None, std=None, backward=True):
    w = vw.World(wp, wit, DT[dtype], dev, causal, form, std, 0, backward)   # (this test's own: dropped with it)
    raw = vw.run(pkg, wp, w.packed(), causal, backward)
    rat, kinds = vw.judge(w, raw)
    return w, raw, rat, kinds


def _same(a, b, what):
    for name in TENSORS:
        if a[name] is not None or b[name] is not None:
            assert torch.equal(a[name], b[name]), f"{what}: {name} differs"


def _tag(wp, causal, dtype):
    return f"{wp.name} H={wp.H} Hkv={wp.Hkv} {'causal' if causal else 'plain'} {dtype}"


# ---------------------------------------------------------------- 1. A: every visible key exactly once
A_PACKS = {"LONG8 self": lambda: vw.long8(4), "LONG8 unequal": lambda: vw.long8(2, True), "LONG4": lambda: vw.long4(8, 1),
           "LONG4 H=4": lambda: vw.long4(4, 4)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", MODES)
@pytest.mark.parametrize("pack", list(A_PACKS))
def test_a_every_visible_key_exactly_once(pkg, dev, pack, causal, dtype):
    wp = A_PACKS[pack]()
    w, raw, rat, _ = _go(pkg, dev, wp, "A", dtype, causal)
    print(f"A {_tag(wp, causal, dtype)}: ratios to the gates: {rat}")
    assert rat.worst() <= 1, f"witness A {_tag(wp, causal, dtype)}: {rat}"
    assert {"exp(lse)", "out Z", "dK = 0", "dQ", "dV", "dn"} <= set(rat)
    if pack == "LONG8 self" and not causal and dtype == "fp16":
        # the integer gate on dV Z ran in a sequence of at least 3 key tiles: the two of 300 keys (Z = 212 + 300 = 512)
        ran = [b for b in w.seq if "dV Z" in vw.judge_seq(w, b, vw.cut(wp, raw, b))]
        assert any(wp.pack.lens_k[b] >= 3 * aw.KT for b in ran), ran


# ---------------------------------------------------------------- 2. B: one key decides
def _b_cases():
    s8, u8, l4, many = (lambda: vw.long8(2)), (lambda: vw.long8(2, True)), (lambda: vw.long4(8, 1)), (lambda: vw.many())
    for name, make in (("LONG8 self", s8), ("LONG8 unequal", u8), ("LONG4", l4), ("MANY", many)):
        for causal in MODES:
            for dtype in DTYPES:
                yield name, make, "ascending", causal, dtype
    for causal in MODES:
        for dtype in DTYPES:
            yield "LONG8 unequal", u8, "descending", causal, dtype
            yield "LONG8 unequal", u8, "code", causal, dtype
        yield "LONG8 unequal", u8, "sink", causal, "bf16"
        yield "LONG8 unequal", u8, "code_sink", causal, "fp16"
        yield "LONG8 self", s8, "code", causal, "bf16"
        yield "LONG4", l4, "code", causal, "fp16"
        yield "LONG4", l4, "code_sink", causal, "bf16"
        yield "LONG4", (lambda: vw.long4(4, 4)), "sink", causal, "fp16"
        for dtype in DTYPES:   # H = Hkv = 4: under causal the dQ and the dK/dV kernel both place their items at G = 2
            yield "LONG4", (lambda: vw.long4(4, 4)), "code", causal, dtype


@pytest.mark.parametrize("name,make,form,causal,dtype", list(_b_cases()), ids=lambda v: "" if callable(v) else str(v))
def test_b_one_key_decides(pkg, dev, name, make, form, causal, dtype):
    wp = make()
    backward = form.startswith("code")
    w, raw, rat, kinds = _go(pkg, dev, wp, "B", dtype, causal, form=form, backward=backward)
    print(f"B {form} {_tag(wp, causal, dtype)}: row kinds {sorted(kinds)}; ratios to the gates: {rat}")
    assert rat.worst() <= 1, f"witness B {form} {_tag(wp, causal, dtype)}: {rat}"
    assert 1 in kinds or form == "code_sink"
    assert 2 in kinds or "sink" not in form
    if causal and name == "LONG8 unequal":
        assert 0 in kinds, "sq > sk under causal: rows that see no key, in a head without a sink"
    if backward:
        assert {"dQ", "dK", "dV", "dn"} <= set(rat)


# ---------------------------------------------------------------- 3. C: a realistic dynamic range
C_PACKS = {f"LONG8 {'unequal' if uneq else 'self'} Hkv={hkv}": (lambda hkv=hkv, uneq=uneq: vw.long8(hkv, uneq)) for uneq in (False, True) for hkv in (4, 2, 1)}
C_PACKS["LONG4 H=8 Hkv=1"] = lambda: vw.long4(8, 1)
C_PACKS["LONG4 H=4 Hkv=4"] = lambda: vw.long4(4, 4)    # (G = 2 in the causal dQ and dK/dV kernels)
C_PACKS["LONG4 H=3 Hkv=3"] = lambda: vw.long4(3, 3)    # (the dQ kernel's plain, non-8-aligned map)


@pytest.mark.parametrize("std", [4, 8])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", MODES)
@pytest.mark.parametrize("pack", list(C_PACKS))
def test_c_realistic_dynamic_range(pkg, dev, pack, causal, dtype, std):
    wp = C_PACKS[pack]()
    w, raw, rat, _ = _go(pkg, dev, wp, "C", dtype, causal, std=std)
    print(f"C std {std} {_tag(wp, causal, dtype)}: ratios to the gates: {rat}")
    assert rat.worst() <= 1, f"witness C std {std} {_tag(wp, causal, dtype)}: {rat}"
    assert {"out", "lse", "dQ", "dK", "dV", "dn"} <= set(rat)
    if causal and "unequal" in pack:
        # n holds an exact 0 and sequence 7 (959 rows, 31 keys) has rows that see no key: nothing may turn NaN, and dn stays gated (above)
        assert (w.n == 0).any() and 7 in w.seq
        for name in ("out", "dq", "dk", "dv", "dn"):
            assert torch.isfinite(raw[name].float()).all(), f"{name}: non-finite values"
        rows = slice(wp.pack.cu_q[7], wp.pack.cu_q[7] + 959 - 31)
        zero_n = w.n == 0
        assert (raw["lse"][zero_n][:, rows] == -math.inf).all() and (raw["out"][rows][:, zero_n].float() == 0).all()
        assert (raw["dq"][rows].float() == 0).all()


# ---------------------------------------------------------------- 4. hints do not change bits
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", MODES)
def test_hints_do_not_change_bits(pkg, dev, causal, dtype):
    for wp in (vw.long8(2), vw.long8(2, True)):
        w = vw.world(wp, "C", DT[dtype], dev, causal, None, 4, 0, True)
        tight = vw.run(pkg, wp, w.packed(), causal)
        for hints in ((2048, 1100), (1100, 2500), (4096, 4096)):
            _same(tight, vw.run(pkg, wp, w.packed(), causal, hints=hints), f"{_tag(wp, causal, dtype)} hints {hints}")


# ---------------------------------------------------------------- 5. 512 sequences
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", MODES)
def test_many_sequences(pkg, dev, causal, dtype):
    wp = vw.many()
    assert wp.pack.B == 512 and wp.pack.max_q == 3
    _, _, rat, _ = _go(pkg, dev, wp, "A", dtype, causal, backward=False)
    print(f"A MANY {_tag(wp, causal, dtype)}: {rat}")
    assert rat.worst() <= 1, dict(rat)
    _, _, rat, _ = _go(pkg, dev, wp, "C", dtype, causal, std=4)
    print(f"C MANY {_tag(wp, causal, dtype)}: {rat}")
    assert rat.worst() <= 1 and "dn" in rat, dict(rat)


@pytest.mark.parametrize("causal", MODES)
def test_many_with_a_trailing_run_of_empty_sequences(pkg, dev, causal):
    wp = vw.many(empty_from=300)
    p = wp.pack
    assert p.cu_q[300:] == [p.cu_q[300]] * 213 and p.cu_q[-1] < p.Tq - 300
    w, raw, rat, _ = _go(pkg, dev, wp, "C", "bf16", causal, std=4)   # (judge: the rows behind cu[B] exactly 0 / -inf)
    print(f"C MANY empty from 300 {_tag(wp, causal, 'bf16')}: {rat}")
    assert rat.worst() <= 1, dict(rat)
    eq = p.cu_q[-1]
    assert (raw["out"][eq:].view(torch.int16) == 0).all() and (raw["dk"][eq:].view(torch.int16) == 0).all()   # +0, not -0


# ---------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_call_is_deterministic(pkg, dev, dtype):
    wp = vw.long8(2)
    w = vw.world(wp, "C", DT[dtype], dev, True, None, 4, 0, True)
    a, b = vw.run(pkg, wp, w.packed(), True), vw.run(pkg, wp, w.packed(), True)
    _same(a, b, f"{_tag(wp, True, dtype)} run twice")


# ---------------------------------------------------------------- 7. front-end paths
def test_scale(pkg, dev):
    wp = vw.long8(2, True)
    for dtype in DTYPES:
        w, raw, rat, _ = _go(pkg, dev, wp, "C", dtype, True, std=0.6)
        assert w.scale == 0.3
        print(f"C scale 0.3 {_tag(wp, True, dtype)}: {rat}")
        assert rat.worst() <= 1, dict(rat)
        ops = w.packed()
        neg = vw.run(pkg, wp, {**ops, "q": -ops["q"]}, True, scale=-0.3)     # -0.3 on -query: the same logits
        for name in TENSORS:
            want = -raw[name] if name == "dq" else raw[name]
            assert torch.equal(neg[name], want), f"scale = -0.3: {name} differs from the call on -query at 0.3"


def _front(pkg, dev, causal, dtype):
    wp = vw.long8(2, True)
    w = vw.world(wp, "C", DT[dtype], dev, causal, None, 4, 0, True)
    return wp, w.packed(), vw.run(pkg, wp, w.packed(), causal)


@pytest.mark.parametrize("causal", MODES)
def test_misaligned_query_and_strided_key(pkg, dev, causal):
    wp, ops, want = _front(pkg, dev, causal, "bf16")
    q = ops["q"]
    buf = torch.empty(q.numel() + 8, dtype=q.dtype, device=dev)
    q_off = buf[1:1 + q.numel()].view(q.shape)
    q_off.copy_(q)
    assert q_off.data_ptr() % 16 == 2
    _same(want, vw.run(pkg, wp, {**ops, "q": q_off}, causal), "a query 2 bytes off 16-byte alignment")
    k = ops["k"]
    k2 = torch.empty(*k.shape[:2], 2 * vw.D, dtype=k.dtype, device=dev)[..., ::2]
    k2.copy_(k)
    assert k2.stride(2) == 2
    _same(want, vw.run(pkg, wp, {**ops, "k": k2}, causal), "a key with feature stride 2")


@pytest.mark.parametrize("causal", MODES)
def test_expanded_dout(pkg, dev, causal):
    wp, ops, _ = _front(pkg, dev, causal, "fp16")
    p = wp.pack
    cu_q, cu_k = p.cu(dev)
    wvec = aw._counter_normal((vw.D,), 77, 1.0, torch.float16, dev)
    seen = []

    def call(loss):
        q, k, v, n = (ops[x].detach().clone().requires_grad_() for x in ("q", "k", "v", "n"))
        out = pkg.flash_attention_n_varlen(q, k, v, cu_q, p.max_q, cu_k, p.max_k, softmax_n_param=n, scale=ops["scale"], is_causal=causal)
        out.register_hook(lambda g: seen.append(g.stride()))
        loss(out)
        torch.cuda.synchronize()
        return dict(dq=q.grad, dk=k.grad, dv=v.grad, dn=n.grad)

    wide = wvec.expand(p.Tq, wp.H, vw.D)
    ones = torch.ones(p.Tq, wp.H, vw.D, dtype=torch.float16, device=dev)
    # ((out * w).sum() reaches the call as a dense product - autograd multiplies the expanded 1 by w first; the expanded w itself is
    # what arrives with strides (0, 0, 1))
    for what, do, loss, strides in (("(out * w).sum()", wide, lambda out: (out * wvec).sum().backward(), None),
                                    ("w [64] expanded", wide, lambda out: out.backward(wide), (0, 0, 1)),
                                    ("out.sum()", ones, lambda out: out.sum().backward(), (0, 0, 0))):
        got = call(loss)
        assert strides is None or seen[-1] == strides, f"dout of {what} arrives with strides {seen[-1]}"
        want = call(lambda out: out.backward(do.contiguous()))
        for name in got:
            assert torch.equal(got[name], want[name]), f"dout of {what} (strides {seen[-2]}): {name} differs from the materialised dout"


def test_fp16_scale_limit_is_named(pkg, dev):
    q = torch.zeros(16, 4, 64, dtype=torch.float16, device=dev)
    cu = torch.tensor([0, 7, 16], dtype=torch.int32, device=dev)
    for scale in (5.6, -5.6):
        with pytest.raises(NotImplementedError, match=r"log2\(e\) <= 8"):
            pkg.flash_attention_n_varlen(q, q, q, cu, 9, scale=scale)
    assert 5.5 * math.log2(math.e) < 8 < 5.6 * math.log2(math.e)
    assert pkg.flash_attention_n_varlen(q, q, q, cu, 9, scale=5.5).shape == q.shape
    assert pkg.flash_attention_n_varlen(q.bfloat16(), q.bfloat16(), q.bfloat16(), cu, 9, scale=5.6).shape == q.shape


# ---------------------------------------------------------------- 8. far tokens, through the C ABI
@pytest.mark.parametrize("causal", MODES)
def test_far_tokens(pkg, dev, causal):
    """token rows 1 MiB apart: every operand spans (2046 * 2^19 + 64) * 2 bytes, just under the 2^31 of check_packed"""
    dt, H, Hkv, ROW = torch.bfloat16, 4, 2, 1 << 19
    pack = av.Pack([257, 1500, 290])
    T = pack.Tq
    span = ((T - 1) * ROW + vw.D) * 2
    assert T == 2047 and (1 << 31) - (1 << 21) < span < (1 << 31)
    inp = av.inputs(pack, Hkv, vw.D, dt, seed=81)
    cu_q, cu_k = pack.cu(dev)

    def outputs(t):
        t["lse"] = torch.full((H, T), 12345.0, dtype=torch.float32, device=dev)
        t["delta"] = torch.full((H, T), float("nan"), dtype=torch.float32, device=dev)
        return t

    near = outputs({x: inp[x].to(dev) for x in inp})
    for x, heads in (("o", H), ("dq", H), ("dk", Hkv), ("dv", Hkv)):
        near[x] = torch.full((T, heads, vw.D), float("nan"), dtype=dt, device=dev)
    assert av.run_abi(pkg, pack, near, 1.0, causal, cu_q, cu_k) == (0, 0)

    arenas = [torch.full((T, ROW), av.SENT[dt], dtype=torch.int16, device=dev) for _ in range(2)]
    heads_of = [a.view(dt).view(T, ROW // vw.D, vw.D) for a in arenas]
    far, h0 = outputs({}), 0
    for x, n in (("q", H), ("k", Hkv), ("v", Hkv), ("do", H)):
        far[x] = heads_of[0][:, h0:h0 + n]
        far[x].copy_(near[x])
        h0 += n
    used = [h0, 0]
    for x, n in (("o", H), ("dq", H), ("dk", Hkv), ("dv", Hkv)):
        far[x] = heads_of[1][:, used[1]:used[1] + n]
        used[1] += n
    assert far["q"].stride(0) == ROW and far["dv"].stride(0) == ROW
    assert av.run_abi(pkg, pack, far, 1.0, causal, cu_q, cu_k) == (0, 0)
    for x in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(far[x], near[x]), f"{x}: rows 1 MiB apart differ from the contiguous call"
    for x in ("q", "k", "v", "do"):
        assert torch.equal(far[x], near[x]), f"{x}: an input was written"
    for a, n in zip(arenas, used):   # on the device: every element outside the views still holds the sentinel
        assert bool((a.view(T, ROW // vw.D, vw.D)[:, n:] == av.SENT[dt]).all()), "an arena element outside the views was written"
