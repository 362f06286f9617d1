"""flash_attention_n_varlen(..., window=) on the GPU: sliding-window attention on packed operands, forward and backward.
Parity with the per-sequence fp32 reference under the band mask; exact visibility in integers; rows outside the memory contract poisoned
with NaN; the sharp-softmax witnesses where one key decides and where waves 1 - 3 of a block begin on hidden tiles; the large window that
is the causal call; a tensor n; strided operands and the C ABI; graph capture; refusals. tests/attn_varlen_window.py is what they share;
the gates are av.check / av.check_lse and the witnesses' own - no tolerance is introduced here."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_varlen as av            # noqa: E402
import attn_varlen_window as avn    # noqa: E402
import attn_varlen_witness as avw   # noqa: E402
import attn_witness as aw           # noqa: E402
from test_gpu_attnvarlen import _call, _check_pack, _check_tail   # noqa: E402

pytestmark = pytest.mark.gpu
H = av.H
DTYPES = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    avn._REF.clear()


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("n", [1.0, 0.0])
@pytest.mark.parametrize("Hkv", [4, 2])
@pytest.mark.parametrize("window", avn.WINDOWS)
@pytest.mark.parametrize("pack_name", sorted(avn.PACKS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity(pkg, dev, dtype, pack_name, window, Hkv, n):
    pack = avn.PACKS[pack_name]
    inp = av.inputs(pack, Hkv, 64, dtype, seed=101 + Hkv)
    ref = avn.reference((pack_name, Hkv, dtype, window, n), pack, inp, n, window)
    _check_pack(avn.call(pkg, dev, pack, inp, n, window), ref, pack, dtype, f"{pack_name} window={window} n={n}")


# ---------------------------------------------------------------- 2. exact visibility
def _indicator_inputs(pack, Hkv, dtype):
    f = torch.arange(64)
    v = (torch.arange(pack.Tk).view(-1, 1, 1) % 64 == f).expand(pack.Tk, Hkv, 64)
    do = (torch.arange(pack.Tq).view(-1, 1, 1) % 64 == f).expand(pack.Tq, H, 64)
    g = torch.Generator().manual_seed(7)
    return dict(q=torch.zeros(pack.Tq, H, 64, dtype=dtype), k=torch.randn(pack.Tk, Hkv, 64, generator=g).to(dtype), v=v.to(dtype).contiguous(),
                do=do.to(dtype).contiguous())


@pytest.mark.parametrize("Hkv", [4, 2])
@pytest.mark.parametrize("window", [1, 2, 63, 64])
@pytest.mark.parametrize("pack_name", sorted(avn.PACKS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_visibility_is_exact(pkg, dev, dtype, pack_name, window, Hkv):
    """q = 0: every logit is 0, every visible key weighs 1 / (1 + cnt_i). V and dO are indicators of the token index mod 64 (token index,
    not index in the sequence: the classes of neighbouring sequences interleave), so every integer below names one (row, key) pair."""
    pack = avn.PACKS[pack_name]
    inp = _indicator_inputs(pack, Hkv, dtype)
    got = {k: t.float().cpu() for k, t in avn.call(pkg, dev, pack, inp, 1.0, window).items()}
    for b in range(pack.B):
        rq, rk = av.seq_rows(pack, "q", b), av.seq_rows(pack, "k", b)
        sq, sk = pack.lens_q[b], pack.lens_k[b]
        if sq == 0:
            continue
        m = avn.band(sq, sk, window)
        cnt = m.sum(1)
        cls_k = (torch.arange(rk.start, rk.stop) % 64)
        cls_q = (torch.arange(rq.start, rq.stop) % 64)
        want_out = torch.zeros(sq, 64)
        if sk:
            want_out.index_add_(1, cls_k, m.float())
        assert want_out.max() <= 1                                    # at most one key of a class in a window of 64
        out = got["out"][rq] * (1 + cnt).view(-1, 1, 1).float()
        assert torch.equal(out.round(), want_out.view(sq, 1, 64).expand(sq, H, 64)), f"seq {b}: out names other keys than the window's"
        assert torch.equal((torch.exp(got["lse"][:, rq].double()) - 1).round().long(), cnt.view(1, -1).expand(H, sq)), f"seq {b}: exp(lse) - 1 is not the window's count"
        if sk:
            want_dv = torch.zeros(sk, 64)
            want_dv.index_add_(1, cls_q, m.t().float())              # rows of class f that see key j
            nz = got["dv"][rk] != 0
            assert torch.equal(nz, (want_dv > 0).view(sk, 1, 64).expand(sk, Hkv, 64)), f"seq {b}: dv is nonzero for other (key, row class) pairs than the window's"
    _check_tail({k: got[k] for k in got}, pack)


@pytest.mark.parametrize("window", [65, 128, 200])
@pytest.mark.parametrize("pack_name", sorted(avn.PACKS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_lse_counts_the_window(pkg, dev, dtype, pack_name, window):
    pack = avn.PACKS[pack_name]
    inp = _indicator_inputs(pack, 2, dtype)
    got = avn.call(pkg, dev, pack, inp, 1.0, window)
    for b in range(pack.B):
        rq = av.seq_rows(pack, "q", b)
        cnt = avn.count(pack.lens_q[b], pack.lens_k[b], window)
        assert torch.equal((torch.exp(got["lse"][:, rq].double().cpu()) - 1).round().long(), cnt.view(1, -1).expand(H, -1)), f"seq {b}"


# ---------------------------------------------------------------- 3. keys below the window are not read
@pytest.mark.parametrize("dtype", DTYPES)
def test_keys_below_the_window_are_not_read(pkg, dev, dtype):
    pack, window, poisoned = avn.POISON_K
    inp = av.inputs(pack, 2, 64, dtype, seed=131)
    zeroed, nan = dict(inp), dict(inp)
    for x in ("k", "v"):
        zeroed[x], nan[x] = inp[x].clone(), inp[x].clone()
        zeroed[x][:poisoned] = 0
        nan[x][:poisoned] = float("nan")
    a, b = avn.call(pkg, dev, pack, zeroed, 1.0, window), avn.call(pkg, dev, pack, nan, 1.0, window)
    for name in ("out", "lse", "dq"):
        assert torch.isfinite(b[name].float()).all(), f"{name}: a K / V row below the window was read"
        assert torch.equal(a[name], b[name]), name
    assert (b["dk"][:poisoned].float() == 0).all() and (b["dv"][:poisoned].float() == 0).all()
    assert torch.equal(a["dk"][poisoned:], b["dk"][poisoned:]) and torch.equal(a["dv"][poisoned:], b["dv"][poisoned:])
    ref = avn.reference(("poison_k", dtype), pack, inp, 1.0, window)
    av.check(b["out"], ref["out"], dtype, "out")
    av.check(b["dk"], ref["dk"], dtype, "dk")


# ---------------------------------------------------------------- 4. rows beyond the window are not used by dK/dV
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_beyond_the_window_are_not_used_by_dkdv(pkg, dev, dtype):
    pack, window, poisoned, judged = avn.POISON_Q
    inp = av.inputs(pack, 2, 64, dtype, seed=141)
    nan = dict(inp)
    for x in ("q", "do"):
        nan[x] = inp[x].clone()
        nan[x][poisoned:] = float("nan")
    a, b = avn.call(pkg, dev, pack, inp, 1.0, window), avn.call(pkg, dev, pack, nan, 1.0, window)
    for name in ("dk", "dv"):
        assert torch.isfinite(b[name][:judged].float()).all(), f"{name}: a q / dO row beyond the window was used"
        assert torch.equal(a[name][:judged], b[name][:judged]), name


# ---------------------------------------------------------------- 5. sharp softmax, one key decides
WPACKS = {"longw": lambda: avw.WPack("LONGW", avn.LONGW.lens_q, None, H=4, Hkv=2, tail=20),
          "seams": lambda: avw.WPack("SEAMS", av.SEAM_LENS, None, H=4, Hkv=2, tail=40)}


def _judge(pkg, w, what):
    rat, kinds = avw.judge(w, avn.run_world(pkg, w))
    print(f"{what}: {rat}")
    assert rat.worst() <= 1.0, f"{what}: {rat}"
    return kinds


@pytest.mark.parametrize("where", avn.WHERE)
@pytest.mark.parametrize("window", [64, 65, 128])
@pytest.mark.parametrize("pack_name", sorted(WPACKS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_key_decides(pkg, dev, dtype, pack_name, window, where):
    """witness B's bounded code aimed at the window's first visible key, its middle and its last: every row of every block - rows
    q0 + 0 .. 127, so waves 1 - 3 begin on tiles hidden from them - returns its target's V row"""
    w = avn.WindowWorld(WPACKS[pack_name](), "B", dtype, dev, window, form=where, seed=3)
    kinds = _judge(pkg, w, f"B {where} {pack_name} window={window}")
    assert 1 in kinds


@pytest.mark.parametrize("std", [4.0, 8.0])
@pytest.mark.parametrize("window", [64, 65, 128])
@pytest.mark.parametrize("pack_name", sorted(WPACKS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_sharp_softmax(pkg, dev, dtype, pack_name, window, std):
    w = avn.WindowWorld(WPACKS[pack_name](), "C", dtype, dev, window, std=std, seed=5)
    _judge(pkg, w, f"C std={std} {pack_name} window={window}")


# ---------------------------------------------------------------- 6. large window
@pytest.mark.parametrize("pack_name", ["seams", "unequal"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_large_window_is_the_causal_call(pkg, dev, dtype, pack_name):
    pack = avn.PACKS[pack_name]
    inp = av.inputs(pack, 2, 64, dtype, seed=161)
    causal = _call(pkg, dev, pack, inp, 1.0, True)
    for window in (pack.max_k, 2 * pack.max_k):
        got = avn.call(pkg, dev, pack, inp, 1.0, window)
        for name in causal:
            assert torch.equal(got[name], causal[name]), f"{name}: window {window} differs from the causal call"
    window = pack.max_k - 1
    ref = avn.reference((pack_name, "large", dtype), pack, inp, 1.0, window)
    _check_pack(avn.call(pkg, dev, pack, inp, 1.0, window), ref, pack, dtype, f"{pack_name} window={window}")


# ---------------------------------------------------------------- 7. tensor n
@pytest.mark.parametrize("pack_name", ["unequal", "longw"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_n_gradient_and_float_twin(pkg, dev, dtype, pack_name):
    pack, window, Hkv = avn.PACKS[pack_name], 128, 4
    inp = av.inputs(pack, Hkv, 64, dtype, seed=171)
    s0 = torch.tensor([-0.5, 0.0, 0.7, 1.5])
    s = s0.to(dev).requires_grad_()
    q, k, v = (inp[x].to(dev).requires_grad_() for x in ("q", "k", "v"))
    cu_q, cu_k = pack.cu(dev)
    out = pkg.flash_attention_n_varlen(q, k, v, cu_q, pack.max_q, None if pack.self_attn else cu_k, pack.max_k, softmax_n_param=torch.exp(s),
                                       is_causal=True, window=window)
    out.backward(inp["do"].to(dev))
    torch.cuda.synchronize()
    ref = avn.reference((pack_name, "tensor_n", dtype), pack, inp, None, window, log_n=s0)
    got, want = s.grad.float().cpu(), ref["ds"]
    err, top = (got - want).abs().max().item(), want.abs().max().item()
    print(f"ds: max-abs error {err:.3e}, max |want| {top:.3e}")
    assert err <= av.REL_TRUE[dtype] * max(top, 1e-2), f"ds: {err:.3e} > REL_TRUE gate"
    av.check(out[:pack.cu_q[-1]], ref["out"][:pack.cu_q[-1]], dtype, "tensor n out")
    av.check(q.grad[:pack.cu_q[-1]], ref["dq"][:pack.cu_q[-1]], dtype, "tensor n dq")
    c = 0.75
    a = avn.call(pkg, dev, pack, inp, c, window)
    for shape in ((), (H,), (1, H)):
        b = avn.call(pkg, dev, pack, inp, torch.full(shape, c, device=dev), window)
        for name in a:
            assert torch.equal(a[name], b[name]), f"{name}: tensor n {shape} filled with {c} differs from the float"


# ---------------------------------------------------------------- 8. strided operands and the C ABI
@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_qkv_slices_and_strided_dout(pkg, dev, dtype):
    pack, Hkv, window = av.SEAMS, 2, 64
    inp = av.inputs(pack, Hkv, 64, dtype, seed=181)
    want = avn.call(pkg, dev, pack, inp, 1.0, window)
    qkv = torch.cat([inp["q"], inp["k"], inp["v"]], dim=1).to(dev).requires_grad_()
    q, k, v = qkv[:, :H], qkv[:, H:H + Hkv], qkv[:, H + Hkv:]
    assert not q.is_contiguous()
    do = torch.zeros(pack.Tq, H + 1, 64 + 8, dtype=dtype, device=dev)[:, :H, :64]
    do.copy_(inp["do"])
    cu_q, _ = pack.cu(dev)
    out, lse = pkg.flash_attention_n_varlen(q, k, v, cu_q, pack.max_q, softmax_n_param=1.0, is_causal=True, return_lse=True, window=window)
    out.backward(do)
    torch.cuda.synchronize()
    assert torch.equal(out, want["out"]) and torch.equal(lse, want["lse"])
    g = qkv.grad
    assert torch.equal(g[:, :H], want["dq"]) and torch.equal(g[:, H:H + Hkv], want["dk"]) and torch.equal(g[:, H + Hkv:], want["dv"])


@pytest.mark.parametrize("pack_name", ["seams", "unequal"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tail_rows_and_gaps_through_the_abi(pkg, dev, dtype, pack_name):
    pack, Hkv, window = avn.PACKS[pack_name], 2, 64
    inp = av.inputs(pack, Hkv, 64, dtype, seed=191)
    t, store = {}, {}
    for name, T, heads in (("q", pack.Tq, H), ("k", pack.Tk, Hkv), ("v", pack.Tk, Hkv), ("do", pack.Tq, H), ("o", pack.Tq, H),
                           ("dq", pack.Tq, H), ("dk", pack.Tk, Hkv), ("dv", pack.Tk, Hkv)):
        t[name], store[name] = av.housed(T, heads, 64, dtype, dev)
        if name in inp:
            t[name].copy_(inp[name])
    t["lse"] = torch.full((H, pack.Tq), 12345.0, dtype=torch.float32, device=dev)
    t["delta"] = torch.full((H, pack.Tq), float("nan"), dtype=torch.float32, device=dev)
    cu_q, cu_k = pack.cu(dev)
    assert avn.run_abi(pkg, pack, t, 1.0, window, cu_q, cu_k) == (0, 0)
    got = dict(out=t["o"], lse=t["lse"], dq=t["dq"], dk=t["dk"], dv=t["dv"])
    _check_tail(got, pack)
    for name in store:
        assert av.gaps_intact(store[name], t[name]), f"{name}: a byte outside the view was written"
    for name in ("q", "k", "v", "do"):
        assert torch.equal(t[name].cpu().view(torch.int16), inp[name].view(torch.int16)), f"{name}: an input was written"
    ref = avn.reference((pack_name, "abi", dtype), pack, inp, 1.0, window)
    eq, ek = pack.cu_q[-1], pack.cu_k[-1]
    for name, end in (("out", eq), ("dq", eq), ("dk", ek), ("dv", ek)):
        av.check(got[name][:end], ref[name][:end], dtype, f"abi {name}")


# ---------------------------------------------------------------- 9. graph capture
@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replays_on_new_offsets(pkg, dev, dtype):
    Hkv, window = 2, 64
    first = av.Pack([300, 10, 0, 129, 61], [300, 0, 30, 79, 91], tail_q=12, tail_k=12)
    second = av.Pack([1, 199, 300, 0, 0], [60, 300, 77, 1, 62], tail_q=12, tail_k=12)
    inp = av.inputs(first, Hkv, 64, dtype, seed=201)
    q, k, v = (inp[x].to(dev).requires_grad_() for x in ("q", "k", "v"))
    do = inp["do"].to(dev)
    cu_q, cu_k = first.cu(dev)

    def step():
        out, lse = pkg.flash_attention_n_varlen(q, k, v, cu_q, 300, cu_k, 300, softmax_n_param=1.0, is_causal=True, return_lse=True, window=window)
        out.backward(do)
        return out, lse

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
            q.grad = k.grad = v.grad = None
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        go, glse = step()
    with torch.no_grad():
        cu_q.copy_(torch.tensor(second.cu_q, dtype=torch.int32))
        cu_k.copy_(torch.tensor(second.cu_k, dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    got = dict(out=go.detach().clone(), lse=glse.clone(), dq=q.grad.clone(), dk=k.grad.clone(), dv=v.grad.clone())
    want = avn.call(pkg, dev, second, inp, 1.0, window)
    for name in want:
        assert torch.equal(got[name], want[name]), f"{name}: the replay on new offsets differs from the eager call"
    ref = avn.reference(("graph", dtype), second, inp, 1.0, window)
    _check_pack(got, ref, second, dtype, "graph replay")


# ---------------------------------------------------------------- 10. refusals on the device
def test_refusals_and_window_none(pkg, dev):
    fa = pkg.flash_attention_n_varlen
    q = torch.zeros(16, H, 64, dtype=torch.bfloat16, device=dev)
    cu = torch.tensor([0, 7, 16], dtype=torch.int32, device=dev)
    assert fa(q, q, q, cu, 9, is_causal=True, window=4).shape == q.shape
    for bad in (True, 4.0, torch.tensor(4, device=dev)):
        with pytest.raises(TypeError, match="window"):
            fa(q, q, q, cu, 9, is_causal=True, window=bad)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="window must be >= 1"):
            fa(q, q, q, cu, 9, is_causal=True, window=bad)
    with pytest.raises(ValueError, match="causal and bottom-right aligned"):
        fa(q, q, q, cu, 9, window=4)
    pack = av.UNEQUAL
    inp = av.inputs(pack, 2, 64, torch.bfloat16, seed=211)
    for causal in (False, True):   # window=None is the call it was
        a, b = _call(pkg, dev, pack, inp, 1.0, causal), avn.call(pkg, dev, pack, inp, 1.0, None, causal=causal)
        for name in a:
            assert torch.equal(a[name], b[name]), name
