"""flash_attention_n's layout contract on the GPU: "4-D views addressed by element strides, feature stride 1, rows 16-byte aligned,
stride 0 = broadcast" - for the inputs q, k, v, dout AND the outputs o, dq, dk, dv, dbias, dn (include/fasn.h).

Every route of tests/attn_layout.py - one per kernel family, every (batch, head) problem distinct - runs through the C ABI under the
pairings L1 and L2, where q, k, v, o, dout, dq, dk, dv differ from each other in batch, head and row stride, dbias / n / dn / mask / bias
are padded or transposed views and every gap of the storage holds a sentinel; then on contiguous clones. Asserted per case:
  (a) o, lse, dq, dk, dv, dbias, dn are bit-identical between the two calls;
  (b) every gap - and under layout F every alias slot - still holds the sentinel after the call;
  (c) the launch plans of the two calls are equal and the argument block carried the views' strides;
  (d) the strided result itself meets witness C's per-element gates (attn_witness.reference, with_bounds, judge_c) at logit std 4: no
      tolerance of its own.
No route's plan depends on a stride (tests/test_attnlayout_cpu.py asserts the plans of L1, L2 and the contiguous twin equal), so (a) holds
everywhere. The second half goes through flash_attention_n itself: unlike layouts of q / k / v, the gradients autograd really sends (row,
batch, head and feature stride 0, [B, L, H, D]), misaligned operands (the copy path) and a Q whose span reaches 2 GiB."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_layout as al    # noqa: E402
import attn_witness as aw   # noqa: E402

pytestmark = pytest.mark.gpu
_REF = {}


def _case_data(name, dtype, dev, case=None, std=al.STD):
    """(case, inputs on the device, fp64 reference, gates): computed once per (route, dtype) and shared by the pairings; left unchanged"""
    key = (name, dtype, std)
    if key not in _REF:
        case = al.ROUTES[name][0] if case is None else case
        dt = aw.DTYPES[dtype]
        inp = aw.inputs_c(case, std, dt, dev, al.seed_of(name))
        keep, p_eff = aw.keep_of(case, al.STATE if case.p else None)
        r = aw.reference(case, inp, keep=keep, p_eff=p_eff)
        g = aw.with_bounds(case, inp, r, aw.unit(case, dt), aw.unit_abs(dt))
        _REF[key] = (case, inp, r, g)
    return _REF[key]


RESULTS = ("out", "lse", "dq", "dk", "dv", "dbias", "dn")


def _assert_layout(pkg, case, dt, inp, r, g, ops_s, what, stores=None):
    """run the strided ops and a contiguous twin; (a), (b), (c), (d)"""
    ops_c = al.alloc(case, dt, ops_s.t["q"].device, "C")
    al.fill(case, ops_c, inp)
    res_s, a_s = al.run(pkg, case, ops_s, inp["scale"], dt)
    res_c, a_c = al.run(pkg, case, ops_c, inp["scale"], dt)
    for key in RESULTS:
        assert (res_s[key] is None) == (res_c[key] is None)
        if res_s[key] is not None:
            bad = (al.ints(res_s[key].contiguous()) != al.ints(res_c[key].contiguous())).sum().item()
            assert bad == 0, f"{what}: (a) {key} differs from the contiguous call in {bad} of {res_c[key].numel()} elements"
    for name, store in (ops_s.store if stores is None else stores).items():
        if store is not None:
            assert al.gaps_intact(store, ops_s.t[name]), f"{what}: (b) a gap of {name}'s storage was written"
    assert al.plans(pkg, a_s) == al.plans(pkg, a_c), f"{what}: (c) the plans differ"
    assert al.block_carries(a_s, ops_s), f"{what}: (c) the argument block does not carry the views' strides"
    rat = aw.judge_c(case, dt, res_s, r, g)
    print(f"{what}: ratios to witness C's gates: {rat}")
    assert rat.worst() <= 1, f"{what}: (d) {rat}"
    return rat


# ---------------------------------------------------------------- 1. every route under L1 and L2
@pytest.mark.parametrize("pairing", ["L1", "L2"])
@pytest.mark.parametrize("name,dtype", al.route_params())
def test_route_under_unlike_layouts(pkg, dev, name, dtype, pairing):
    case, inp, r, g = _case_data(name, dtype, dev)
    dt = aw.DTYPES[dtype]
    ops = al.alloc(case, dt, dev, pairing)
    al.fill(case, ops, inp)
    _assert_layout(pkg, case, dt, inp, r, g, ops, f"{name} {dtype} {pairing}")


# ---------------------------------------------------------------- 2. layout F: offsets beyond 2^31 and 2^32 bytes
@pytest.fixture(scope="module")
def arena(dev):
    a = torch.empty(al.FAR_BYTES // 2, dtype=torch.int16, device=dev)   # uninitialised: only the used and the alias slots are written
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", sorted(al.FAR))
def test_far_offsets(pkg, dev, arena, name):
    """q, k, v, o, dout, dq, dk, dv in one arena, batch elements (F': K/V heads) 2^31 + 32 MiB bytes apart: element 0 below 2^31 bytes,
    element 1 in [2^31, 2^32), element 2 beyond 2^32 bytes and beyond 2^31 16-bit elements. (a), (c), (d) as under L1; (b) over the
    three used regions and the alias slots of every tensor. One case per address-forming source text."""
    case, dtype, dim = al.FAR[name]
    _, inp, r, g = _case_data("far " + name, dtype, dev, case=case)
    dt = aw.DTYPES[dtype]
    ops, far = al.far_ops(case, dt, arena, dim)
    esize = 4 if dtype == "fp32" else 2
    for t in (ops.t[x] for x in far):
        off = [(t.select(dim, i).data_ptr() - arena.data_ptr()) for i in range(3)]
        assert off[0] < 2 ** 31 <= off[1] < 2 ** 32 <= off[2] and (esize == 4 or (t.select(dim, 2).data_ptr() - t.data_ptr()) // esize >= 2 ** 31)
    al.fill(case, ops, inp)
    stores = {k: v for k, v in ops.store.items() if k not in far}
    _assert_layout(pkg, case, dt, inp, r, g, ops, f"far {name}", stores=stores)
    assert al.far_intact(arena, ops, far, dt), f"far {name}: (b) a gap or an alias slot of the arena was written"


# ---------------------------------------------------------------- 3. the largest row stride the host admits
@pytest.mark.parametrize("D", [64, 128])
def test_largest_legal_row_stride(pkg, dev, D):
    """65 keys and 65 rows whose rows lie max_row_stride apart - K and V (refused beyond it by every call) and Q and dO (refused beyond it by
    fasn_bwd): the kernels' 32-bit tile and lane offsets (grow * ks[2] * 2, tq * QT * dos[2] * 2, the _ws_ kernels' sq / sd and voff*) at
    the bound they are sized for. About 2.1 GB of address space per tensor, only the used rows written. Bit-compared with the contiguous
    call, and (d)."""
    case = aw.Case(1, 2, 65, 65, D, want=("_ws_",) if D == 128 else ())
    dtype, dt = "bf16", torch.bfloat16
    _, inp, r, g = _case_data(f"largest stride {D}", dtype, dev, case=case)
    stride = al.max_row_stride(65, D)
    ops = al.alloc(case, dt, dev, "L1")
    try:
        for name in ("q", "k", "v", "dout"):
            ops.put(name, al.wide_view(tuple(ops.t[name].shape), dt, dev, stride, 1 << 20), None)
            assert ops.t[name].stride(2) == stride
        al.fill(case, ops, inp)
        _assert_layout(pkg, case, dt, inp, r, g, ops, f"largest row stride D={D}")
    finally:
        ops = None
        torch.cuda.empty_cache()


def test_bias_and_mask_of_2_gib_take_the_element_path(pkg, dev):
    """A bias and a mask whose (Sq - 1) * row_stride + Sk reaches 2^31 bytes are legal: build_fwd demotes them to the element-load kernels,
    which address every element in 64 bits. The plan depends on a stride here (fasn_api.hip, build_fwd: "slices of 2 GiB or more use the
    element path"), so the contiguous twin takes the vector kernels and (a) gives way to (d) on the strided result."""
    L, S, D = 65, 72, 64
    case = aw.Case(1, 2, L, S, D, bias="bhls", mask="dense")
    dtype, dt = "bf16", torch.bfloat16
    _, inp, r, g = _case_data("2 GiB bias and mask", dtype, dev, case=case)
    ops = al.alloc(case, dt, dev, "L1")
    try:
        brow, mrow = al._up(-(-(2 ** 31 // 2 - S) // (L - 1)), 8), al._up(-(-(2 ** 31 - S) // (L - 1)), 16)
        assert ((L - 1) * brow + S) * 2 >= 2 ** 31 and (L - 1) * mrow + S >= 2 ** 31
        ops.put("bias", al.wide_view((1, 2, L, S), dt, dev, brow, 1 << 12), None)
        ops.put("mask", al.wide_view((1, 2, L, S), torch.uint8, dev, mrow, 1 << 12), None)
        al.fill(case, ops, inp)
        res, a = al.run(pkg, case, ops, inp["scale"], dt)
        assert all("element-load" in k or "fasn_bwd_delta" in k for k in al.described(pkg, a)), al.described(pkg, a)
        assert pkg._lib.load().fasn_fwd_path(a.fwd) == pkg._lib.FASN_PATH_ELEMENT
        for name, store in ops.store.items():
            if store is not None:
                assert al.gaps_intact(store, ops.t[name]), f"(b) a gap of {name}'s storage was written"
        rat = aw.judge_c(case, dt, res, r, g)
        print(f"2 GiB bias and mask: ratios to witness C's gates: {rat}")
        assert rat.worst() <= 1, rat
        # one of the two alone demotes the call as well
        for keep in ("bias", "mask"):
            b2 = al.block(pkg, case, ops, inp["scale"], dt)
            dense = al.alloc(case, dt, "meta", "C")
            other = "mask" if keep == "bias" else "bias"
            setattr(b2.fwd, other, al.view4(pkg, dense.t[other]))
            assert pkg._lib.load().fasn_fwd_path(b2.fwd) == pkg._lib.FASN_PATH_ELEMENT, keep
    finally:
        ops = None
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 4. through flash_attention_n itself
def _kwargs(case, inp, n, bias):
    return dict(softmax_n_param=n, scale=inp["scale"], dropout_p=case.p, attn_mask=inp["mask"], attn_bias=bias, is_causal=case.causal)


def _leaf(t):
    """a leaf with t's values and strides (t is a view without autograd history: it becomes the leaf itself)"""
    return t.detach().requires_grad_()


def _call(pkg, case, inp, q, k, v, loss=None, dout=None):
    """forward and backward through flash_attention_n on leaves q, k, v (their own strides), a leaf n and a leaf bias. `loss` maps out to a
    scalar (the gradient autograd then sends is recorded), or `dout` is sent as it is. Returns the result dict and the dO the
    backward got."""
    q, k, v = _leaf(q), _leaf(k), _leaf(v)
    n = inp["n"].detach().clone().requires_grad_() if torch.is_tensor(inp["n"]) else inp["n"]
    bias = None if inp["bias"] is None else aw._leaf_like(inp["bias"])
    out = pkg.flash_attention_n(q, k, v, **_kwargs(case, inp, n, bias))
    seen = []
    out.register_hook(seen.append)
    if loss is not None:
        loss(out).backward()
    else:
        out.backward(dout)
    res = dict(out=out.detach(), lse=None, dq=q.grad, dk=k.grad, dv=v.grad, dn=n.grad if torch.is_tensor(n) else None,
               dbias=None if bias is None else bias.grad, state=None)
    return res, seen[0]


def _same(res_a, res_b, what):
    for key in RESULTS:
        if res_a[key] is not None:
            assert res_a[key].shape == res_b[key].shape
            bad = (al.ints(res_a[key].contiguous()) != al.ints(res_b[key].contiguous())).sum().item()
            assert bad == 0, f"{what}: {key} differs in {bad} of {res_b[key].numel()} elements"


PY_LAYOUTS = dict(q=("pad", 1), k=("blhd", 3, 0), v=("hb", 2))


@pytest.mark.parametrize("name", ["d64 plain", "d64 keypad", "d128 plain", "d256 plain", "d64 bias", "fp32"])
def test_python_layer_three_unlike_layouts(pkg, dev, name):
    """q padded, k a slot of a packed [B, T, 3, H, D] buffer, v [H, B, T, D] permuted, at once, forward and backward: no copy is made
    (_canon hands the very tensors on), the results equal those of contiguous clones bit for bit and meet (d)"""
    from flash_attention_softmax_n_amd import flash_attn
    dtype = al.ROUTES[name][1][0]
    case, inp, r, g = _case_data(name, dtype, dev)
    dt = aw.DTYPES[dtype]
    views = {}
    for key in ("q", "k", "v"):
        views[key], _ = al.house(tuple(inp[key].shape), dt, dev, PY_LAYOUTS[key])
        views[key].copy_(inp[key])
        assert flash_attn._canon(views[key]) is views[key] and not views[key].is_contiguous()
    res_s, _ = _call(pkg, case, inp, views["q"], views["k"], views["v"], dout=inp["do"])
    res_c, _ = _call(pkg, case, inp, inp["q"], inp["k"], inp["v"], dout=inp["do"])
    _same(res_s, res_c, name)
    rat = aw.judge_c(case, dt, res_s, r, g)
    print(f"python layer {name}: ratios to witness C's gates: {rat}")
    assert rat.worst() <= 1, rat


@pytest.mark.parametrize("kind", ["shared 3-D", "gqa"])
def test_python_layer_kv_sliced_from_a_wider_buffer(pkg, dev, kind):
    """one K/V for all heads given as [B, S, D] (head stride 0 inside), and grouped K/V heads, each a slice of a wider buffer"""
    Hkv = 1 if kind == "shared 3-D" else 2
    case = aw.Case(3, 4, 300, 420, 64, Hkv=Hkv, nshape="BH", want=("GQA=1",))
    _, inp, r, g = _case_data("py kv " + kind, "bf16", dev, case=case)
    dt = torch.bfloat16
    wide = {}
    for key in ("k", "v"):
        buf = torch.full((3, Hkv + 2, 420 + 1, 64 + 8), float("nan"), dtype=dt, device=dev)
        wide[key] = buf[:, 1:1 + Hkv, :420, :64]
        wide[key].copy_(inp[key])
    pick = (lambda t: t[:, 0]) if Hkv == 1 else (lambda t: t)
    res_s, _ = _call(pkg, case, inp, inp["q"], pick(wide["k"]), pick(wide["v"]), dout=inp["do"])
    res_c, _ = _call(pkg, case, inp, inp["q"], pick(inp["k"]).contiguous(), pick(inp["v"]).contiguous(), dout=inp["do"])
    _same(res_s, res_c, kind)
    for key in ("dk", "dv"):
        res_s[key] = res_s[key].reshape(3, Hkv, 420, 64)
    rat = aw.judge_c(case, dt, res_s, r, g)
    print(f"python layer {kind}: ratios to witness C's gates: {rat}")
    assert rat.worst() <= 1, rat


def _w(shape, dev, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


# the losses whose gradient autograd sends as a view: name -> (loss, the strides of dO that must be 0 - None: whatever autograd makes)
DOUT_FORMS = {
    "out.sum(2)": (lambda o, w: (o.sum(2) * w[:, :, 0]).sum(), (2,)),
    "out.mean((0,1))": (lambda o, w: (o.mean((0, 1)) * w[0, 0]).sum(), None),
    "out.sum((0,1))": (lambda o, w: (o.sum((0, 1)) * w[0, 0]).sum(), (0, 1)),
    "out.sum(1)": (lambda o, w: (o.sum(1) * w[:, 0]).sum(), (1,)),
    "out.sum(0)": (lambda o, w: (o.sum(0) * w[0]).sum(), (0,)),
    "out * w[:, None, :, None]": (lambda o, w: (o * w[:, 0, :, 0][:, None, :, None]).sum(), None),
    "out.sum()": (lambda o, w: o.sum(), (0, 1, 2, 3)),
    "[B,L,H,D] dO": (lambda o, w: (o.permute(0, 2, 1, 3).reshape(o.shape[0], o.shape[2], -1) * w.permute(0, 2, 1, 3).reshape(o.shape[0], o.shape[2], -1)).sum(), None),
}
DOUT_CASES = ["d64 plain", "d64 keypad", "d64 gqa", "d128 plain", "d256 plain", "d64 bias", "d128 bias keypad", "fp32"]


@pytest.mark.parametrize("name", DOUT_CASES)
def test_python_layer_dout_as_autograd_sends_it(pkg, dev, name):
    """dO as autograd really produces it - expanded views with row, batch, head or feature stride 0, a [B, L, H, D] gradient: every
    gradient equals, bit for bit, that of the same call given dout.contiguous(). One case per backward family that reads dO (the
    pipelined, the one-wave, the two-wave D = 128 and D = 256 kernels with fasn_bwd_delta, both dbias kernels, the fp32 kernels; dn reads
    it too)."""
    dtype = al.ROUTES[name][1][0]
    case, inp, _, _ = _case_data(name, dtype, dev)
    w = _w((case.B, case.H, case.L, case.D), dev, 5).to(aw.DTYPES[dtype])
    for form, (loss, zero) in DOUT_FORMS.items():
        res_s, dout = _call(pkg, case, inp, inp["q"], inp["k"], inp["v"], loss=lambda o: loss(o, w))
        if zero is not None:
            assert all(dout.stride(i) == 0 for i in zero), (form, dout.stride())
        if form == "[B,L,H,D] dO":
            assert dout.stride(1) == case.D and dout.stride(2) == case.H * case.D, dout.stride()
        res_c, d2 = _call(pkg, case, inp, inp["q"], inp["k"], inp["v"], dout=dout.contiguous())
        assert d2.is_contiguous() and torch.equal(d2, dout)
        _same(res_s, res_c, f"{name}, dO of {form} with strides {tuple(dout.stride())}")
        for key in ("dq", "dk", "dv"):
            assert torch.isfinite(res_s[key].float()).all(), (form, key)


@pytest.mark.parametrize("name", ["d64 plain", "d128 plain"])
def test_python_layer_misaligned_operands_take_the_copy(pkg, dev, name):
    """operands 8 bytes off the 16-byte alignment, and with row strides that are no multiple of 8 elements, are legal for
    flash_attention_n: _canon copies them; no error, results bit-equal to the aligned call"""
    from flash_attention_softmax_n_amd import flash_attn
    dtype = "bf16"
    case, inp, _, _ = _case_data(name, dtype, dev)
    dt = aw.DTYPES[dtype]

    def off8(t):   # the same values 4 elements (8 bytes) into a flat buffer
        buf = torch.empty(t.numel() + 4, dtype=dt, device=dev)
        view = buf[4:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 8
        return view

    def odd_rows(t):   # rows D + 4 elements apart
        buf = torch.empty(t.shape[:3] + (t.shape[3] + 4,), dtype=dt, device=dev)
        view = buf[..., :t.shape[3]]
        view.copy_(t)
        assert view.stride(2) % 8 == 4
        return view

    res_c, _ = _call(pkg, case, inp, inp["q"], inp["k"], inp["v"], dout=inp["do"])
    for make in (off8, odd_rows):
        ops = [make(inp[key]) for key in ("q", "k", "v", "do")]
        assert all(flash_attn._canon(t) is not t for t in ops)
        res_s, _ = _call(pkg, case, inp, ops[0], ops[1], ops[2], dout=ops[3])
        _same(res_s, res_c, f"{name} {make.__name__}")


def test_python_layer_q_whose_span_reaches_2_gib(pkg, dev):
    """include/fasn.h, the span rule: fasn_fwd reads a Q of any span, fasn_bwd refuses a Q or dO whose (b, h) matrix spans 2^31 bytes or
    more. flash_attention_n copies such an operand (flash_attn._canon), so a call whose forward ran never dies in its backward with a bare
    FASN_EINVAL. Q and dO: 65 rows one alignment step beyond the largest legal row stride."""
    from flash_attention_softmax_n_amd import flash_attn
    D = 64
    case = aw.Case(1, 2, 65, 65, D)
    dt = torch.bfloat16
    _, inp, r, g = _case_data("largest stride 64", "bf16", dev, case=case)
    stride = al.max_row_stride(65, D) + 8
    q = do = None
    try:
        q, do = (al.wide_view((1, 2, 65, D), dt, dev, stride, 1 << 20) for _ in range(2))
        q.copy_(inp["q"])
        do.copy_(inp["do"])
        assert flash_attn._rows_ok(q) and not flash_attn._span_ok(q) and flash_attn._canon(q) is not q
        res_s, _ = _call(pkg, case, inp, q, inp["k"], inp["v"], dout=do)
        res_c, _ = _call(pkg, case, inp, inp["q"], inp["k"], inp["v"], dout=inp["do"])
        _same(res_s, res_c, "Q and dO beyond the span rule")
        rat = aw.judge_c(case, dt, res_s, r, g)
        assert rat.worst() <= 1, rat
    finally:
        q = do = None
        torch.cuda.empty_cache()
