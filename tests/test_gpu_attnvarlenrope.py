"""flash_attention_n_varlen_rope and fasn_varlen_rope on the GPU: the rotary launch alone against the eager rotation, bit
for bit, on housed views; the whole call against the eager route (positions from the integer model, the rotation with torch ops under
autograd, flash_attention_n_varlen), bit for bit in out, lse and every gradient; random tables under the gates of tests/attn_varlen.py
against the fp32 reference on eagerly rotated operands; long sequences and many sequences; graph capture with new offsets at replay;
refusals. Support: tests/attn_varlen_rope.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_varlen as av          # noqa: E402
import attn_varlen_rope as avr    # noqa: E402

pytestmark = pytest.mark.gpu
H, D = av.H, 64
PACKS = {"seams": av.SEAMS, "unequal": av.UNEQUAL}


def _ops(pack, Hkv, dtype, seed, dev):
    return {x: t.to(dev) for x, t in av.inputs(pack, Hkv, D, dtype, seed).items()}


def _tables_with_nan_rows(pack, rd, table_dtype, dev, extra=8):
    """true tables of max_seqlen_k + extra rows whose rows >= max_seqlen_k hold NaN: no position may read them"""
    cos, sin = avr.true_tables(pack.max_k + extra, rd, table_dtype, dev)
    cos[pack.max_k:], sin[pack.max_k:] = float("nan"), float("nan")
    return cos, sin


# ---------------------------------------------------------------- 1. the launch alone, through the C ABI
LAUNCH_CASES = [   # dtype, interleaved, rotary_dim, table dtype (None: the operands'), Hkv
    (torch.bfloat16, False, 64, torch.float32, 4),
    (torch.bfloat16, True, 64, torch.float32, 2),
    (torch.bfloat16, False, 32, None, 2),
    (torch.bfloat16, True, 16, None, 4),
    (torch.float16, False, 64, None, 2),
    (torch.float16, True, 32, torch.float32, 4),
    (torch.float16, False, 16, torch.float32, 4),
]


@pytest.mark.parametrize("pack_name", sorted(PACKS))
@pytest.mark.parametrize("dtype,interleaved,rd,table_dtype,Hkv", LAUNCH_CASES)
def test_launch_alone_is_the_eager_rotation(pkg, dev, pack_name, dtype, interleaved, rd, table_dtype, Hkv):
    pack = PACKS[pack_name]
    ops = _ops(pack, Hkv, dtype, 101, dev)
    cos, sin = _tables_with_nan_rows(pack, rd, dtype if table_dtype is None else table_dtype, dev)
    cu_q, cu_k = pack.cu(dev)
    where = avr.positions(pack, pack.max_k, dev)   # (clamped to the rows the call is promised: none of the NaN rows)
    src = {"q": ops["q"], "k": ops["k"]}
    for inverse in (0, 1):
        housed = {s: av.housed(src[s].shape[0], src[s].shape[1], D, dtype, dev) for s in ("q", "k")}
        assert avr.run_abi(pkg, pack, src["q"], src["k"], housed["q"][0], housed["k"][0], cos, sin, cu_q, cu_k, interleaved, inverse) == 0
        for s in ("q", "k"):
            view, store = housed[s]
            pos, valid = where[s]
            want = avr.rot(src[s], cos, sin, pos, valid, interleaved, inverse=bool(inverse))
            assert torch.isfinite(view[valid].float()).all(), f"{s}: a NaN table row was read"
            assert torch.equal(view[valid], want[valid]), f"{s} inverse={inverse}: not the eager rotation, bit for bit"
            assert (view.view(torch.int16)[~valid] == av.SENT[dtype]).all(), f"{s}: a row of no sequence was written"
            assert av.gaps_intact(store, view), f"{s}: a byte between the rows was written"
        # in place, on housed copies of the sources: the out-of-place bits, the gaps intact
        inplace = {s: av.housed(src[s].shape[0], src[s].shape[1], D, dtype, dev) for s in ("q", "k")}
        for s in ("q", "k"):
            inplace[s][0].copy_(src[s])
        assert avr.run_abi(pkg, pack, inplace["q"][0], inplace["k"][0], inplace["q"][0], inplace["k"][0], cos, sin, cu_q, cu_k, interleaved, inverse) == 0
        for s in ("q", "k"):
            view, store = inplace[s]
            valid = where[s][1]
            assert torch.equal(view[valid], housed[s][0][valid]), f"{s} inverse={inverse}: in place differs from out of place"
            assert torch.equal(view[~valid], src[s][~valid]), f"{s}: a row of no sequence was written in place"
            assert av.gaps_intact(store, view)


def test_inverse_undoes_nothing_it_should_not(pkg, dev):
    """the transpose is not the identity and not the rotation: on a table whose sines are not 0 the two directions differ"""
    pack, dtype = av.UNEQUAL, torch.bfloat16
    ops = _ops(pack, 4, dtype, 103, dev)
    cos, sin = avr.random_tables(pack.max_k, 64, 5, torch.float32, dev)
    cu_q, cu_k = pack.cu(dev)
    outs = []
    for inverse in (0, 1):
        qo, ko = torch.zeros_like(ops["q"]), torch.zeros_like(ops["k"])
        assert avr.run_abi(pkg, pack, ops["q"], ops["k"], qo, ko, cos, sin, cu_q, cu_k, False, inverse) == 0
        outs.append((qo, ko))
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][1], outs[1][1])


# ---------------------------------------------------------------- 2. the whole call against the eager route, bit for bit
ROUTE_CASES = {   # pack, dtype, Hkv, keyword arguments of the routes
    "seams plain": ("seams", torch.bfloat16, 4, dict()),
    "seams causal gqa": ("seams", torch.bfloat16, 2, dict(causal=True)),
    "seams causal fp16 interleaved": ("seams", torch.float16, 2, dict(causal=True, interleaved=True)),
    "unequal plain": ("unequal", torch.bfloat16, 4, dict()),
    "unequal causal gqa": ("unequal", torch.float16, 2, dict(causal=True)),
    "seams window 64": ("seams", torch.bfloat16, 2, dict(causal=True, window=64)),
    "seams window 65": ("seams", torch.float16, 4, dict(causal=True, window=65)),
    "unequal window 64": ("unequal", torch.bfloat16, 4, dict(causal=True, window=64)),
    "unequal window 65": ("unequal", torch.bfloat16, 2, dict(causal=True, window=65)),
    "seams negative scale": ("seams", torch.bfloat16, 4, dict(causal=True, scale=-0.2)),
}


@pytest.mark.parametrize("name", sorted(ROUTE_CASES))
def test_whole_call_equals_the_eager_route(pkg, dev, name):
    pack_name, dtype, Hkv, kw = ROUTE_CASES[name]
    pack = PACKS[pack_name]
    ops = _ops(pack, Hkv, dtype, 111, dev)
    rd = 32 if "gqa" in name else 64
    cos, sin = _tables_with_nan_rows(pack, rd, torch.float32, dev)
    want = avr.eager_route(pkg, pack, ops, cos[:pack.max_k], sin[:pack.max_k], n=0.75, **kw)
    got = avr.fused_route(pkg, pack, ops, cos, sin, n=0.75, **kw)
    avr.same_bits(got, want, name)
    assert torch.isfinite(got["out"].float()).all() and torch.isfinite(got["dq"].float()).all() and torch.isfinite(got["dk"].float()).all()
    eq, ek = pack.cu_q[-1], pack.cu_k[-1]
    assert (got["dq"][eq:].float() == 0).all() and (got["dk"][ek:].float() == 0).all(), "gradient rows of no sequence are not 0"


@pytest.mark.parametrize("pack_name", sorted(PACKS))
def test_tensor_n_with_gradient_and_16_bit_tables(pkg, dev, pack_name):
    pack, dtype = PACKS[pack_name], torch.bfloat16
    ops = _ops(pack, 2, dtype, 113, dev)
    cos, sin = avr.true_tables(pack.max_k, 64, dtype, dev)
    n = torch.tensor([0.0, 0.5, 1.0, 3.0], device=dev)
    want = avr.eager_route(pkg, pack, ops, cos, sin, n=n, causal=True)
    got = avr.fused_route(pkg, pack, ops, cos, sin, n=n, causal=True)
    assert got["dn"] is not None and got["dn"].abs().max() > 0
    avr.same_bits(got, want, f"{pack_name} tensor n")


def test_slices_of_one_qkv_buffer(pkg, dev):
    pack, dtype, Hkv = av.SEAMS, torch.bfloat16, 2
    inp = av.inputs(pack, Hkv, D, dtype, 115)
    cos, sin = avr.true_tables(pack.max_k, 64, torch.float32, dev)
    cu_q, _ = pack.cu(dev)
    contiguous = avr.fused_route(pkg, pack, {x: t.to(dev) for x, t in inp.items()}, cos, sin, causal=True)
    qkv = torch.cat([inp["q"], inp["k"], inp["v"]], dim=1).to(dev).requires_grad_()   # [T, H + 2 Hkv, D]
    q, k, v = qkv[:, :H], qkv[:, H:H + Hkv], qkv[:, H + Hkv:]
    assert not q.is_contiguous() and q.stride(0) == (H + 2 * Hkv) * D
    out, lse = pkg.flash_attention_n_varlen_rope(q, k, v, cu_q, pack.max_q, cos, sin, is_causal=True, return_lse=True)
    out.backward(inp["do"].to(dev))
    torch.cuda.synchronize()
    g = qkv.grad
    assert torch.equal(out, contiguous["out"]) and torch.equal(lse, contiguous["lse"])
    assert torch.equal(g[:, :H], contiguous["dq"]) and torch.equal(g[:, H:H + Hkv], contiguous["dk"]) and torch.equal(g[:, H + Hkv:], contiguous["dv"])
    want = avr.eager_route(pkg, pack, dict(q=q.detach(), k=k.detach(), v=v.detach(), do=inp["do"].to(dev)), cos, sin, causal=True)
    avr.same_bits(contiguous, want, "qkv slices")


# ---------------------------------------------------------------- 3. random tables, under the gates
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("pack_name", sorted(PACKS))
def test_random_tables_against_the_reference(pkg, dev, pack_name, causal):
    """with tables that relate no row to another, a position taken from the wrong sequence - or the global token index - is a gross error"""
    pack, dtype, Hkv = PACKS[pack_name], torch.bfloat16, 2
    inp = av.inputs(pack, Hkv, D, dtype, 121)
    cos, sin = avr.random_tables(pack.max_k, 64, 7)
    where = avr.positions(pack, pack.max_k, "cpu")
    rotated = dict(inp, q=avr.rot(inp["q"], cos, sin, *where["q"]), k=avr.rot(inp["k"], cos, sin, *where["k"]))
    ref = av.reference(("rope random", pack_name, causal), pack, rotated, 1.0, causal)
    # the reference's dq / dk are the rotated operands': the transpose rotation, in fp32, gives the unrotated operands'
    ref_dq = avr.rot(ref["dq"], cos, sin, *where["q"], inverse=True)
    ref_dk = avr.rot(ref["dk"], cos, sin, *where["k"], inverse=True)
    got = avr.fused_route(pkg, pack, {x: t.to(dev) for x, t in inp.items()}, cos.to(dev), sin.to(dev), n=1.0, causal=causal)
    eq, ek = pack.cu_q[-1], pack.cu_k[-1]
    av.check(got["out"][:eq], ref["out"][:eq], dtype, "out")
    av.check_lse(got["lse"][:, :eq], ref["lse"][:, :eq], dtype, "lse")
    av.check(got["dq"][:eq], ref_dq[:eq], dtype, "dq")
    av.check(got["dk"][:ek], ref_dk[:ek], dtype, "dk")
    av.check(got["dv"][:ek], ref["dv"][:ek], dtype, "dv")
    # and the gate would see the global token index: the same call with one table row per TOKEN differs grossly
    if pack.self_attn:
        wrong = avr.rot(inp["q"], *avr.random_tables(pack.Tq, 64, 7), torch.arange(pack.Tq), where["q"][1])
        assert (wrong.float() - rotated["q"].float()).abs().max() > 0.5


# ---------------------------------------------------------------- 4. long sequences, many sequences
LONG = {"one sequence of 1100": avr.ONE_LONG, "LONG8": avr.LONG8, "MANY": avr.MANY, "MANY empty from 300": avr.MANY_EMPTY}


@pytest.mark.parametrize("name", sorted(LONG))
def test_long_and_many(pkg, dev, name):
    """more token blocks than one workgroup walks inside one sequence; the search across 512 offsets, a constant tail of them included"""
    pack, dtype = LONG[name], torch.bfloat16
    ops = _ops(pack, 2, dtype, 131, dev)
    cos, sin = avr.random_tables(pack.max_k, 64, 9, torch.float32, dev)
    want = avr.eager_route(pkg, pack, ops, cos, sin, causal=True)
    got = avr.fused_route(pkg, pack, ops, cos, sin, causal=True)
    avr.same_bits(got, want, name)


# ---------------------------------------------------------------- 5. graph capture
def test_graph_replays_on_new_offsets(pkg, dev):
    dtype, Hkv = torch.bfloat16, 2
    first = av.Pack([300, 10, 0, 129, 61], [300, 0, 30, 79, 91], tail_q=12, tail_k=12)
    second = av.Pack([1, 199, 300, 0, 0], [60, 300, 77, 1, 62], tail_q=12, tail_k=12)
    assert (first.Tq, first.Tk, first.max_q, first.max_k) == (second.Tq, second.Tk, second.max_q, second.max_k) == (512, 512, 300, 300)
    inp = av.inputs(first, Hkv, D, dtype, seed=141)
    q, k, v = (inp[x].to(dev).requires_grad_() for x in ("q", "k", "v"))
    do = inp["do"].to(dev)
    cos, sin = avr.random_tables(300, 64, 11, torch.float32, dev)
    cu_q, cu_k = first.cu(dev)

    def step():
        out, lse = pkg.flash_attention_n_varlen_rope(q, k, v, cu_q, 300, cos, sin, cu_k, 300, softmax_n_param=1.0, is_causal=True, return_lse=True)
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
    got = dict(out=go.detach().clone(), lse=glse.clone(), dq=q.grad.clone(), dk=k.grad.clone(), dv=v.grad.clone(), dn=None)
    ops = {x: t.to(dev) for x, t in inp.items()}
    avr.same_bits(got, avr.fused_route(pkg, second, ops, cos, sin, causal=True), "replay against the call")
    avr.same_bits(got, avr.eager_route(pkg, second, ops, cos, sin, causal=True), "replay against the eager route")


# ---------------------------------------------------------------- 6. refusals
def test_refusals_name_their_reason(pkg, dev):
    fa = pkg.flash_attention_n_varlen_rope
    q = torch.zeros(16, H, 64, dtype=torch.bfloat16, device=dev)
    cu = torch.tensor([0, 7, 16], dtype=torch.int32, device=dev)
    cos, sin = avr.true_tables(16, 64, torch.float32, dev)
    assert fa(q, q, q, cu, 9, cos, sin).shape == q.shape
    assert fa(q, q, q, cu, 9, cos[:9], sin[:9]).shape == q.shape   # rows == max_seqlen_k
    # the tables
    with pytest.raises(RuntimeError, match="rotary_cos is on cpu"):
        fa(q, q, q, cu, 9, cos.cpu(), sin)
    with pytest.raises(ValueError, match="float32 or the dtype of query"):
        fa(q, q, q, cu, 9, cos.half(), sin.half())
    with pytest.raises(ValueError, match="one shape, dtype and row stride"):
        fa(q, q, q, cu, 9, cos, sin.bfloat16())
    with pytest.raises(ValueError, match=r"must be a \[rows, rotary_dim / 2\] tensor"):
        fa(q, q, q, cu, 9, cos[0], sin[0])
    with pytest.raises(ValueError, match=r"must be a \[rows, rotary_dim / 2\] tensor"):
        fa(q, q, q, cu, 9, None, None)
    with pytest.raises(ValueError, match="cover 8 positions but max_seqlen_k is 9"):
        fa(q, q, q, cu, 9, cos[:8], sin[:8])
    with pytest.raises(ValueError, match="cover 16 positions but max_seqlen_k is 20"):
        fa(q, q, q, cu, 9, cos, sin, cu, 20)
    for half in (4, 12, 40):   # rotary_dim 8, 24, 80
        c = torch.zeros(16, half, device=dev)
        with pytest.raises(ValueError, match=f"rotary_dim = 2 x {half} = {2 * half} is not supported"):
            fa(q, q, q, cu, 9, c, c)
    with pytest.raises(ValueError, match="unit column stride"):
        wide = torch.zeros(16, 64, device=dev)
        fa(q, q, q, cu, 9, wide[:, ::2], wide[:, ::2])
    with pytest.raises(ValueError, match="requires grad"):
        fa(q, q, q, cu, 9, cos.clone().requires_grad_(), sin)
    with pytest.raises(ValueError, match="requires grad"):
        fa(q, q, q, cu, 9, cos, sin.clone().requires_grad_())
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError, match="rotary_interleaved must be a bool"):
            fa(q, q, q, cu, 9, cos, sin, rotary_interleaved=bad)
    # each of the base call's refusals, first, with its words - also when the tables are bad too
    bad_tables = (cos[:8].cpu(), sin[:8].cpu())
    for tables in ((cos, sin), bad_tables):
        with pytest.raises(NotImplementedError, match="float32"):
            fa(q.float(), q.float(), q.float(), cu, 9, *tables)
        with pytest.raises(NotImplementedError, match="E != Ev"):
            fa(q, q, torch.zeros(16, H, 128, dtype=torch.bfloat16, device=dev), cu, 9, *tables)
        for E in (32, 128, 256, 48):
            x = torch.zeros(16, H, E, dtype=torch.bfloat16, device=dev)
            with pytest.raises(NotImplementedError, match=r"head dims served: \[64\]"):
                fa(x, x, x, cu, 9, *tables)
        with pytest.raises(RuntimeError, match="CPU"):
            fa(q.cpu(), q.cpu(), q.cpu(), cu, 9, *tables)
        with pytest.raises(TypeError, match="int32"):
            fa(q, q, q, cu.long(), 9, *tables)
        with pytest.raises(ValueError, match="cu_seqlens_q is on cpu"):
            fa(q, q, q, cu.cpu(), 9, *tables)
        with pytest.raises(ValueError, match="cu_seqlens_k is on cpu"):
            fa(q, q, q, cu, 9, *tables, cu.cpu(), 9)
        for shape in ((2, H), (2, 1)):   # one n per sequence
            with pytest.raises(ValueError, match="per-sequence"):
                fa(q, q, q, cu, 9, *tables, softmax_n_param=torch.ones(shape, device=dev))
        with pytest.raises(ValueError, match="window needs is_causal=True"):
            fa(q, q, q, cu, 9, *tables, window=4)
        with pytest.raises(ValueError, match="window must be >= 1"):
            fa(q, q, q, cu, 9, *tables, window=0, is_causal=True)
        with pytest.raises(NotImplementedError, match="float16 with"):
            fa(q.half(), q.half(), q.half(), cu, 9, *tables, scale=8.0)
    # nothing to differentiate: no autograd node
    assert fa(q, q, q, cu, 9, cos, sin).grad_fn is None
    assert fa(q.clone().requires_grad_(), q, q, cu, 9, cos, sin).grad_fn is not None
