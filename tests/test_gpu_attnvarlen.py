"""flash_attention_n_varlen on the GPU: packed variable-length training attention, forward and backward, against the per-sequence fp32
reference of tests/attn_varlen.py. Seams (lengths that straddle every tile edge), unequal sides, exact isolation between sequences, the
rows behind the last sequence, strided operands, a tensor n, graph capture with new offsets at replay, refusals.

Parametrised over the head dims (64, 128): a dim this build refuses is asserted to be refused, with the dims served in the message."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_varlen as av   # noqa: E402

pytestmark = pytest.mark.gpu
H = av.H
SERVED = (64,)
DTYPES = [torch.float16, torch.bfloat16]


def _refused_dim(pkg, dev, D):
    """True (after asserting the refusal) when the build does not serve head dim D"""
    if D in SERVED:
        return False
    q = torch.zeros(8, H, D, dtype=torch.bfloat16, device=dev)
    cu = torch.tensor([0, 8], dtype=torch.int32, device=dev)
    with pytest.raises(NotImplementedError, match=r"head dims served: \[64\]"):
        pkg.flash_attention_n_varlen(q, q, q, cu, 8)
    a, vl = av.block(pkg, 64, 64, 4, 4, D)
    assert pkg._lib.load().fasn_fwd_varlen(a.fwd, vl, None, 0, None) == -7   # FASN_EUNSUPPORTED, before any HIP call
    return True


def _call(pkg, dev, pack, inp, n, causal, cu=None):
    q, k, v = (inp[x].to(dev).requires_grad_() for x in ("q", "k", "v"))
    cu_q, cu_k = pack.cu(dev) if cu is None else cu
    out, lse = pkg.flash_attention_n_varlen(q, k, v, cu_q, pack.max_q, None if pack.self_attn else cu_k, pack.max_k, softmax_n_param=n,
                                            is_causal=causal, return_lse=True)
    out.backward(inp["do"].to(dev))
    torch.cuda.synchronize()
    return dict(out=out.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def _check_pack(got, ref, pack, dtype, what):
    """per sequence: out, lse, dq over its query rows, dk, dv over its key rows; then the rows nobody owns"""
    for b in range(pack.B):
        rq, rk = av.seq_rows(pack, "q", b), av.seq_rows(pack, "k", b)
        tag = f"{what} seq {b} ({pack.lens_q[b]}, {pack.lens_k[b]})"
        if pack.lens_q[b]:
            av.check(got["out"][rq], ref["out"][rq], dtype, f"{tag} out")
            av.check_lse(got["lse"][:, rq], ref["lse"][:, rq], dtype, f"{tag} lse")
            av.check(got["dq"][rq], ref["dq"][rq], dtype, f"{tag} dq")
        if pack.lens_k[b]:
            av.check(got["dk"][rk], ref["dk"][rk], dtype, f"{tag} dk")
            av.check(got["dv"][rk], ref["dv"][rk], dtype, f"{tag} dv")
    _check_tail(got, pack)


def _check_tail(got, pack):
    eq, ek = pack.cu_q[-1], pack.cu_k[-1]
    assert (got["out"][eq:].float() == 0).all() and (got["dq"][eq:].float() == 0).all(), "rows behind the last sequence: out / dq not 0"
    assert (got["lse"][:, eq:] == -float("inf")).all(), "rows behind the last sequence: lse not -inf"
    assert (got["dk"][ek:].float() == 0).all() and (got["dv"][ek:].float() == 0).all(), "key rows behind the last sequence: dk / dv not 0"


# ---------------------------------------------------------------- 1. seams
@pytest.mark.parametrize("D", av.DIMS)
@pytest.mark.parametrize("Hkv", [4, 2])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_seams(pkg, dev, dtype, causal, Hkv, D):
    if _refused_dim(pkg, dev, D):
        return
    pack = av.SEAMS
    assert pack.Tq > pack.cu_q[-1]
    inp = av.inputs(pack, Hkv, D, dtype, seed=11 + Hkv)
    ref = av.reference(("seams", Hkv, D, dtype, causal), pack, inp, 1.0, causal)
    _check_pack(_call(pkg, dev, pack, inp, 1.0, causal), ref, pack, dtype, "seams")


# ---------------------------------------------------------------- 2. unequal sides
@pytest.mark.parametrize("D", av.DIMS)
@pytest.mark.parametrize("n", [1.0, 0.0])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_unequal_sides(pkg, dev, dtype, causal, n, D):
    if _refused_dim(pkg, dev, D):
        return
    pack = av.UNEQUAL
    Hkv = 2 if causal else 4
    inp = av.inputs(pack, Hkv, D, dtype, seed=23)
    ref = av.reference(("unequal", Hkv, D, dtype, causal, n), pack, inp, n, causal)
    got = _call(pkg, dev, pack, inp, n, causal)
    _check_pack(got, ref, pack, dtype, f"unequal n={n}")
    if causal:   # (200, 5): 195 rows that see no key; (70, 0): no key at all - 0 with lse log n (-inf at n = 0), gradients 0
        for rows in (slice(pack.cu_q[1], pack.cu_q[1] + 195), av.seq_rows(pack, "q", 4)):
            assert (got["out"][rows].float() == 0).all() and (got["dq"][rows].float() == 0).all()
            want = 0.0 if n == 1.0 else -float("inf")
            assert (got["lse"][:, rows] == want).all()


# ---------------------------------------------------------------- 3. isolation, exact
@pytest.mark.parametrize("D", av.DIMS)
@pytest.mark.parametrize("subject", [0, 6, 13])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_isolation_is_exact(pkg, dev, dtype, causal, subject, D):
    if _refused_dim(pkg, dev, D):
        return
    pack, Hkv = av.SEAMS, 2
    G = H // Hkv
    inp = av.inputs(pack, Hkv, D, dtype, seed=31)
    rq, rk = av.seq_rows(pack, "q", subject), av.seq_rows(pack, "k", subject)
    assert pack.lens_q[subject] > 0
    # every other sequence (and the tail): keys aligned with the subject's queries and queries with its keys, 32 times as long - a score
    # of about 32 |q|^2 / 8 = 64 where the subject's own are of order 1 -, values and dout at the largest normal / 4
    big = torch.finfo(dtype).max / 4
    adv = {x: t.clone() for x, t in inp.items()}
    qs, ks = inp["q"][rq].float(), inp["k"][rk].float()
    tq, tk = torch.arange(pack.Tq), torch.arange(pack.Tk)
    adv["k"] = (32.0 * qs[tk % qs.shape[0]][:, ::G]).to(dtype)
    adv["q"] = (32.0 * ks[tq % ks.shape[0]].repeat_interleave(G, dim=1)).to(dtype)
    adv["v"] = torch.full_like(inp["v"], big)
    adv["do"] = torch.full_like(inp["do"], -big)
    for x, rows in (("q", rq), ("do", rq), ("k", rk), ("v", rk)):
        adv[x][rows] = inp[x][rows]
    assert all(torch.isfinite(t.float()).all() for t in adv.values())
    a, b = _call(pkg, dev, pack, inp, 1.0, causal), _call(pkg, dev, pack, adv, 1.0, causal)
    for name, rows in (("out", rq), ("dq", rq), ("dk", rk), ("dv", rk)):
        assert torch.equal(a[name][rows], b[name][rows]), f"{name} of sequence {subject} changed with the other sequences' data"
    assert torch.equal(a["lse"][:, rq], b["lse"][:, rq]), f"lse of sequence {subject} changed with the other sequences' data"
    assert torch.isfinite(a["out"][rq].float()).all() and torch.isfinite(a["dk"][rk].float()).all()


# ---------------------------------------------------------------- 4. tail and gaps, through the C ABI
@pytest.mark.parametrize("D", av.DIMS)
@pytest.mark.parametrize("pack_name", ["seams", "unequal"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tail_rows_and_gaps(pkg, dev, dtype, pack_name, D):
    if _refused_dim(pkg, dev, D):
        return
    pack = av.SEAMS if pack_name == "seams" else av.UNEQUAL
    Hkv, causal = 2, pack_name == "seams"
    inp = av.inputs(pack, Hkv, D, dtype, seed=41)
    t, store = {}, {}
    for name, T, heads in (("q", pack.Tq, H), ("k", pack.Tk, Hkv), ("v", pack.Tk, Hkv), ("do", pack.Tq, H), ("o", pack.Tq, H),
                           ("dq", pack.Tq, H), ("dk", pack.Tk, Hkv), ("dv", pack.Tk, Hkv)):
        t[name], store[name] = av.housed(T, heads, D, dtype, dev)
        if name in inp:
            t[name].copy_(inp[name])
    t["lse"] = torch.full((H, pack.Tq), 12345.0, dtype=torch.float32, device=dev)   # sentinel-filled outputs
    t["delta"] = torch.full((H, pack.Tq), float("nan"), dtype=torch.float32, device=dev)
    cu_q, cu_k = pack.cu(dev)
    assert av.run_abi(pkg, pack, t, 1.0, causal, cu_q, cu_k) == (0, 0)
    got = dict(out=t["o"], lse=t["lse"], dq=t["dq"], dk=t["dk"], dv=t["dv"])
    _check_tail(got, pack)
    for name in store:
        assert av.gaps_intact(store[name], t[name]), f"{name}: a byte outside the view was written"
    for name in ("q", "k", "v", "do"):
        assert torch.equal(t[name].cpu().view(torch.int16), inp[name].view(torch.int16)), f"{name}: an input was written"
    ref = av.reference((pack_name, Hkv, D, dtype, causal, "abi"), pack, inp, 1.0, causal)
    eq, ek = pack.cu_q[-1], pack.cu_k[-1]
    av.check(got["out"][:eq], ref["out"][:eq], dtype, "abi out")
    av.check(got["dq"][:eq], ref["dq"][:eq], dtype, "abi dq")
    av.check(got["dk"][:ek], ref["dk"][:ek], dtype, "abi dk")
    av.check(got["dv"][:ek], ref["dv"][:ek], dtype, "abi dv")


# ---------------------------------------------------------------- 5. strided operands
@pytest.mark.parametrize("D", av.DIMS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_qkv_slices_and_strided_dout(pkg, dev, dtype, causal, D):
    if _refused_dim(pkg, dev, D):
        return
    pack, Hkv = av.SEAMS, 2
    inp = av.inputs(pack, Hkv, D, dtype, seed=51)
    want = _call(pkg, dev, pack, inp, 1.0, causal)
    qkv = torch.cat([inp["q"], inp["k"], inp["v"]], dim=1).to(dev).requires_grad_()   # [T, H + 2 Hkv, D]
    q, k, v = qkv[:, :H], qkv[:, H:H + Hkv], qkv[:, H + Hkv:]
    assert not q.is_contiguous() and q.stride(0) == (H + 2 * Hkv) * D
    do = torch.zeros(pack.Tq, H + 1, D + 8, dtype=dtype, device=dev)[:, :H, :D]
    do.copy_(inp["do"])
    assert not do.is_contiguous()
    cu_q, _ = pack.cu(dev)
    out, lse = pkg.flash_attention_n_varlen(q, k, v, cu_q, pack.max_q, softmax_n_param=1.0, is_causal=causal, return_lse=True)
    out.backward(do)
    torch.cuda.synchronize()
    assert torch.equal(out, want["out"]) and torch.equal(lse, want["lse"])
    g = qkv.grad
    assert torch.equal(g[:, :H], want["dq"]) and torch.equal(g[:, H:H + Hkv], want["dk"]) and torch.equal(g[:, H + Hkv:], want["dv"])


# ---------------------------------------------------------------- 6. tensor n
@pytest.mark.parametrize("D", av.DIMS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_n_gradient_and_float_twin(pkg, dev, dtype, causal, D):
    if _refused_dim(pkg, dev, D):
        return
    pack, Hkv = av.UNEQUAL, 4
    inp = av.inputs(pack, Hkv, D, dtype, seed=61)
    s0 = torch.tensor([-0.5, 0.0, 0.7, 1.5])
    s = s0.to(dev).requires_grad_()
    q, k, v = (inp[x].to(dev).requires_grad_() for x in ("q", "k", "v"))
    cu_q, cu_k = pack.cu(dev)
    out = pkg.flash_attention_n_varlen(q, k, v, cu_q, pack.max_q, cu_k, pack.max_k, softmax_n_param=torch.exp(s), is_causal=causal)
    out.backward(inp["do"].to(dev))
    torch.cuda.synchronize()
    ref = av.reference(("tensor_n", D, dtype, causal), pack, inp, None, causal, log_n=s0)
    got, want = s.grad.float().cpu(), ref["ds"]
    err, top = (got - want).abs().max().item(), want.abs().max().item()
    print(f"ds: max-abs error {err:.3e}, max |want| {top:.3e}")
    assert err <= av.REL_TRUE[dtype] * max(top, 1e-2), f"ds: {err:.3e} > REL_TRUE gate"
    av.check(out[:pack.cu_q[-1]], ref["out"][:pack.cu_q[-1]], dtype, "tensor n out")
    av.check(q.grad[:pack.cu_q[-1]], ref["dq"][:pack.cu_q[-1]], dtype, "tensor n dq")
    # a tensor filled with c gives the float c's results bit for bit
    c = 0.75
    a = _call(pkg, dev, pack, inp, c, causal)
    for shape in ((), (H,), (1, H)):
        b = _call(pkg, dev, pack, inp, torch.full(shape, c, device=dev), causal)
        for name in a:
            assert torch.equal(a[name], b[name]), f"{name}: tensor n {shape} filled with {c} differs from the float"


# ---------------------------------------------------------------- 7. graph capture
@pytest.mark.parametrize("D", av.DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replays_on_new_offsets(pkg, dev, dtype, D):
    if _refused_dim(pkg, dev, D):
        return
    Hkv = 2
    first = av.Pack([300, 10, 0, 129, 61], [300, 0, 30, 79, 91], tail_q=12, tail_k=12)
    second = av.Pack([1, 199, 300, 0, 0], [60, 300, 77, 1, 62], tail_q=12, tail_k=12)
    assert (first.Tq, first.Tk, first.max_q, first.max_k) == (second.Tq, second.Tk, second.max_q, second.max_k) == (512, 512, 300, 300)
    inp = av.inputs(first, Hkv, D, dtype, seed=71)
    q, k, v = (inp[x].to(dev).requires_grad_() for x in ("q", "k", "v"))
    do = inp["do"].to(dev)
    cu_q, cu_k = first.cu(dev)

    def step():
        out, lse = pkg.flash_attention_n_varlen(q, k, v, cu_q, 300, cu_k, 300, softmax_n_param=1.0, is_causal=True, return_lse=True)
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
    want = _call(pkg, dev, second, inp, 1.0, True)
    for name in want:
        assert torch.equal(got[name], want[name]), f"{name}: the replay on new offsets differs from the eager call"


# ---------------------------------------------------------------- 8. refusals
def test_refusals_name_their_reason(pkg, dev):
    fa = pkg.flash_attention_n_varlen
    q = torch.zeros(16, H, 64, dtype=torch.bfloat16, device=dev)
    cu = torch.tensor([0, 7, 16], dtype=torch.int32, device=dev)
    assert fa(q, q, q, cu, 9).shape == q.shape
    for kw in ("attn_mask", "attn_bias", "dropout_p"):   # not arguments of this call
        with pytest.raises(TypeError, match=kw):
            fa(q, q, q, cu, 9, **{kw: None})
    with pytest.raises(NotImplementedError, match="float32"):
        fa(q.float(), q.float(), q.float(), cu, 9)
    with pytest.raises(NotImplementedError, match="E != Ev"):
        fa(q, q, torch.zeros(16, H, 128, dtype=torch.bfloat16, device=dev), cu, 9)
    for D in (32, 256, 48, 128):
        if D in SERVED:
            continue
        x = torch.zeros(16, H, D, dtype=torch.bfloat16, device=dev)
        with pytest.raises(NotImplementedError, match=r"head dims served: \[64\]"):
            fa(x, x, x, cu, 9)
    with pytest.raises(RuntimeError, match="CPU"):
        fa(q.cpu(), q.cpu(), q.cpu(), cu, 9)
    with pytest.raises(TypeError, match="int32"):
        fa(q, q, q, cu.long(), 9)
    with pytest.raises(ValueError, match="cu_seqlens_q is on cpu"):
        fa(q, q, q, cu.cpu(), 9)
    with pytest.raises(ValueError, match="cu_seqlens_k is on cpu"):
        fa(q, q, q, cu, 9, cu.cpu(), 9)
    for shape in ((2, H), (2, 1)):   # one n per sequence
        with pytest.raises(ValueError, match="per-sequence"):
            fa(q, q, q, cu, 9, softmax_n_param=torch.ones(shape, device=dev))
    # nothing to differentiate: no autograd node
    assert fa(q, q, q, cu, 9).grad_fn is None
    assert fa(q.clone().requires_grad_(), q, q, cu, 9).grad_fn is not None
