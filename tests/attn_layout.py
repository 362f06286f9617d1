"""What the layout tests of flash_attention_n share (tests/test_attnlayout_cpu.py, tests/test_gpu_attnlayout.py): the layout rule of
include/fasn.h - "4-D views addressed by element strides, feature stride 1, rows 16-byte aligned, stride 0 = broadcast" - turned into
operands for q, k, v, dout AND the outputs o, dq, dk, dv, dbias, dn. A plain module: no tests, importable without a GPU. It is the
training-path twin of tests/kv_layout.py and reuses tests/attn_witness.py for operands, reference and gates (no tolerance of its own).

  house      one [B, heads, T, D] operand in fresh integer storage filled with a sentinel, under a named layout:
               ("pad", a)      storage [B, heads + 1, T + 1, D + 8a] sliced: every stride differs from the dense one
               ("blhd", n, a)  slot 1 of a packed [B, T, n, heads, D + 8a] buffer (n = 3: a fused QKV projection)
               ("hb", a)       [heads, B + 1, T, D + 8a] permuted
             The parameters only make the eight tensors of one call pairwise unlike: PAIRINGS L1 and L2 give q, k, v, o, dout, dq, dk,
             dv layouts that differ from each other in batch, head and row stride (alloc asserts it). "C" is the contiguous twin.
  alloc      every operand and output of a Case under a pairing: dense dbias in rows of S + 8 (pre-zeroed: the ABI wants that under
             causal), reduced dbias [1, H, L, S] sliced from [H + 1, L + 1, S + 8], n and dn as the transpose of [H + 1, B + 1] storage,
             mask / bias as padded views that stay vector-movable (rows a multiple of 16 bytes, mask base a multiple of 4), lse and
             delta contiguous. Gaps hold a sentinel: a NaN with a payload for floating data, 0xff for mask bytes. With device "meta"
             nothing is allocated: the strides alone, for the plans and the address model of the CPU suite.
  block      the BwdArgs of the call over these tensors (what flash_attn._fill_fwd / _view4 make of them), with real or fake pointers.
  run        the call through the C ABI: fasn_fwd / fasn_fwd_ws (by fasn_fwd_workspace_bytes) or fasn_fwd_n, fasn_bwd, fasn_bwd_dn;
             dropout by (seed, offset) by value. The Python front end allocates its outputs contiguous, which is why it is bypassed.
  ROUTES     one case per kernel family at its smallest shape, every (batch, head) problem distinct (ub = B, uh = H): tiled operands
             would make a wrong batch or head stride bit-identical to the right answer. tests/golden/attn_layout_plans.txt pins the plans.
  addr_map / strided_addr / write_model   the address arithmetic in plain integers, for the mutants the CPU suite shows checks (a) / (b) catch.
  far_ops    layout F: the eight 4-D tensors in one arena of about 4.1 GiB whose batch stride (F; F': the K/V head stride, under grouped
             K/V) of 2^31 + 32 MiB bytes puts element 0 below 2^31 bytes, element 1 in [2^31, 2^32) and element 2 beyond 2^32 bytes and
             (16-bit types) beyond 2^31 elements; the slots the wrapped offsets would hit (bytes mod 2^32, bytes mod 2^31, elements mod
             2^31) hold the sentinel. Only the slots in use and the alias slots are ever written.
  wide_view  an operand at the largest row stride the host admits (max_row_stride), in an uninitialised buffer."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_witness as aw   # noqa: E402

SENT = {torch.bfloat16: 0x7FA5, torch.float16: 0x7DA5, torch.float32: 0x7FA5A5A5, torch.uint8: 0xFF}   # NaN with a payload; 0xff mask bytes
INT = {2: torch.int16, 4: torch.int32, 1: torch.uint8}
PAIRINGS = {
    "L1": dict(q=("pad", 1), k=("blhd", 3, 0), v=("hb", 0), o=("blhd", 4, 1), dout=("hb", 2), dq=("pad", 3), dk=("hb", 4), dv=("pad", 5)),
    "L2": dict(q=("blhd", 3, 0), k=("hb", 0), v=("pad", 1), o=("hb", 2), dout=("pad", 3), dq=("blhd", 4, 1), dk=("pad", 5), dv=("blhd", 5, 2)),
}
STATE = (0x1234ABCD5678, 12)   # dropout (seed, offset), by value


def ints(t):
    return t.view(INT[t.element_size()])


def _full(shape, dtype, dev):
    """integer storage of `shape` elements of dtype, every element the sentinel"""
    return torch.full(shape, SENT[dtype], dtype=INT[torch.empty((), dtype=dtype).element_size()], device=dev)


def house(shape, dtype, dev, layout):
    """(view [B, heads, T, D] in dtype, integer storage) under a named layout; the view holds the sentinel too until it is filled"""
    B, Hx, T, D = shape
    kind = layout[0]
    if kind == "pad":
        store = _full((B, Hx + 1, T + 1, D + 8 * layout[1]), dtype, dev)
        view = store[:, :Hx, :T, :D]
    elif kind == "blhd":
        store = _full((B, T, layout[1], Hx, D + 8 * layout[2]), dtype, dev)
        view = store[:, :, 1, :, :D].permute(0, 2, 1, 3)
    elif kind == "hb":
        store = _full((Hx, B + 1, T, D + 8 * layout[1]), dtype, dev)
        view = store[:, :B, :, :D].permute(1, 0, 2, 3)
    else:
        assert kind == "c"
        store = _full((B, Hx, T, D), dtype, dev)
        view = store
    return view.view(dtype), store


def gaps_intact(store, view):
    """True iff every element of the storage outside the view still holds the sentinel (integer bits)"""
    inside = torch.zeros(store.numel(), dtype=torch.bool, device=store.device)
    torch.as_strided(inside, tuple(view.shape), tuple(view.stride()), view.storage_offset() - store.storage_offset()).fill_(True)
    return bool((store.reshape(-1)[~inside] == SENT[view.dtype]).all())


def _up(x, m):
    return (x + m - 1) // m * m


class Ops:
    """the tensors of one call: t[name] the view the call gets (or None), store[name] its integer storage"""

    def __init__(self):
        self.t, self.store = {}, {}

    def put(self, name, view, store):
        self.t[name], self.store[name] = view, store


def n_shape(case):
    return {"H": (1, case.H), "B1": (case.B, 1), "BH": (case.B, case.H)}.get(case.nshape)


def dbias_reduced(case, dtype):
    return case.bias == "hls" and case.B > 1 and case.p == 0.0 and dtype != torch.float32


def alloc(case, dtype, dev, pairing, backward=True):
    """every tensor of the case's call under `pairing` ("L1", "L2" or "C"), inputs still holding the sentinel"""
    B, H, Hkv, L, S, D = case.B, case.H, case.Hkv, case.L, case.S, case.D
    strided = pairing != "C"
    lay = PAIRINGS[pairing] if strided else {}
    ops = Ops()
    names = ("q", "k", "v", "o") + (("dout", "dq", "dk", "dv") if backward else ())
    for name in names:
        shape = (B, H, L, D) if name in ("q", "o", "dout", "dq") else (B, Hkv, S, D)
        ops.put(name, *house(shape, dtype, dev, lay.get(name, ("c",))))
    if strided:   # pairwise unlike in batch, head and row stride (a size-1 dimension has no stride to speak of)
        for i in range(3):
            seen = {}
            for name in names:
                t = ops.t[name]
                if t.size(i) > 1:
                    assert t.stride(i) not in seen, f"{pairing}: {name} and {seen[t.stride(i)]} share stride {i} = {t.stride(i)}"
                    seen[t.stride(i)] = name
                assert t.stride(i) % (16 // t.element_size()) == 0 and t.stride(3) == 1
    ops.put("lse", torch.empty((B, H, L), dtype=torch.float32, device=dev), None)
    if backward:
        ops.put("delta", torch.empty((B, H, L), dtype=torch.float32, device=dev), None)
    # mask: uint8, 0xff in the gaps (a stray read sees a visible key)
    ops.put("mask", None, None)
    if case.mask == "keypad":
        Sp = _up(S, 16) + 16 if strided else S
        st = _full((B, Sp), torch.uint8, dev)
        ops.put("mask", st[:, :S].unflatten(0, (B, 1, 1)), st)
    elif case.mask == "dense":
        Sp = _up(S, 16) + 16 if strided else S
        st = _full((B, H, L + (1 if strided else 0), Sp), torch.uint8, dev)
        ops.put("mask", st[:, :, :L, :S], st)
    elif case.mask == "misaligned":   # rows of S + 1 bytes from an odd address: the element loads, in both twins
        st = _full((B * H * L * (S + 1) + 1,), torch.uint8, dev)
        ops.put("mask", st[1:].view(B, H, L, S + 1)[..., :S], st)
    ops.put("bias", None, None)
    ops.put("dbias", None, None)
    if case.bias is not None:
        Bb = 1 if case.bias == "hls" else B
        Sp = _up(S, 8) + 8 if strided else S
        st = _full((Bb, H, L + (1 if strided else 0), Sp), dtype, dev)
        view = st[:, :, :L, :S].view(dtype)
        ops.put("bias", view.expand(B, H, L, S), st)
        if backward:
            if dbias_reduced(case, dtype):
                st = _full((H + 1, L + 1, S + 8) if strided else (H, L, S), dtype, dev)
                ops.put("dbias", st[:H, :L, :S].view(dtype).unsqueeze(0), st)
            else:
                st = _full((B, H, L, S + 8) if strided else (B, H, L, S), dtype, dev)
                ops.put("dbias", st[..., :S].view(dtype), st)
                ops.t["dbias"].zero_()   # the caller pre-zeroes a dense dbias (tiles the causal walk skips are never written)
    ops.put("n", None, None)
    ops.put("dn", None, None)
    if n_shape(case) is not None:
        nb, nh = n_shape(case)
        for name in ("n", "dn") if backward else ("n",):
            st = _full((H + 1, B + 1) if strided else (nb, nh), torch.float32, dev)
            ops.put(name, (st.t()[:nb, :nh] if strided else st).view(torch.float32), st)
    return ops


def fill(case, ops, inp):
    """the inputs of attn_witness.inputs_* into the views (bit copies)"""
    for name, key in (("q", "q"), ("k", "k"), ("v", "v"), ("dout", "do")):
        if name in ops.t:
            ops.t[name].copy_(inp[key])
    if ops.t["mask"] is not None:
        ops.t["mask"].copy_(inp["mask"].view(torch.uint8) if inp["mask"].dtype == torch.bool else inp["mask"])
    if ops.t["bias"] is not None:
        b = inp["bias"]
        ops.t["bias"][:1 if case.bias == "hls" else case.B].copy_(b.unsqueeze(0) if b.dim() == 3 else b)
    if ops.t["n"] is not None:
        ops.t["n"].copy_(inp["n"].reshape(n_shape(case)))


# ---------------------------------------------------------------- the argument block
def _ptr(t):
    return t.data_ptr() if t.device.type != "meta" else aw.DUMMY + t.storage_offset() * t.element_size()


def view4(pkg, t):
    """flash_attn._view4 with a fake aligned address on the meta device"""
    v = pkg._lib.View4()
    if t is None:
        v.ptr = None
        return v
    v.ptr = _ptr(t)
    for i in range(4):
        v.stride[i] = t.stride(i) if t.size(i) > 1 else 0
    v.stride[3] = 1 if t.size(3) == 1 else t.stride(3)
    return v


def n_strides(t):
    return (t.stride(0) if t.shape[0] > 1 else 0), (t.stride(1) if t.shape[1] > 1 else 0)


def block(pkg, case, ops, scale, dtype, backward=True):
    """the BwdArgs of the case's call over ops (flash_attn._fill_fwd's fields; n as a tensor leaves softmax_n = 0 in the block)"""
    Lb = pkg._lib
    a = Lb.BwdArgs()
    f = a.fwd
    t = ops.t
    f.q, f.k, f.v, f.o = (view4(pkg, t[x]) for x in ("q", "k", "v", "o"))
    f.lse = _ptr(t["lse"])
    f.mask, f.bias = view4(pkg, t["mask"]), view4(pkg, t["bias"])
    f.bias_dtype = Lb.FASN_BIAS_NONE if t["bias"] is None else Lb.FASN_BIAS_SAME
    f.dtype = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}[dtype]
    f.B, f.H, f.Sq, f.Sk, f.D, f.Dv = case.B, case.H, case.L, case.S, case.D, case.D
    f.kv_group = case.G if case.G > 1 else 0
    f.scale, f.softmax_n = scale, (1.5 if case.nshape == "float" else 0.0)
    f.causal, f.dropout_p = int(case.causal), case.p
    f.seed, f.offset = STATE if case.p else (0, 0)
    f.rng_state = None
    if backward:
        a.dout, a.dq, a.dk, a.dv = (view4(pkg, t[x]) for x in ("dout", "dq", "dk", "dv"))
        a.delta = _ptr(t["delta"])
        a.workspace, a.workspace_bytes, a.flags = None, 0, 0
        a.dbias = view4(pkg, t["dbias"])
        a.dbias_dtype = Lb.FASN_BIAS_SAME if (t["dbias"] is not None and t["dbias"].shape[0] == 1 and case.B > 1) else 0
    return a


BLOCK_VIEWS = (("q", "fwd.q"), ("k", "fwd.k"), ("v", "fwd.v"), ("o", "fwd.o"), ("dout", "dout"), ("dq", "dq"), ("dk", "dk"), ("dv", "dv"))


def block_carries(a, ops, backward=True):
    """the argument block holds the views' own strides (and addresses)"""
    for name, path in BLOCK_VIEWS[:8 if backward else 4]:
        v = a
        for part in path.split("."):
            v = getattr(v, part)
        t = ops.t[name]
        if v.ptr != _ptr(t) or any(v.stride[i] != (t.stride(i) if t.size(i) > 1 else 0) for i in range(3)) or v.stride[3] != 1:
            return False
    return True


def plans(pkg, a, backward=True):
    """(forward plan with its workspace, backward plan) of the block: lists of (kernel, grid, block, lds); nothing is launched"""
    Lb = pkg._lib
    return Lb.launch_plan(a, Lb.FASN_PLAN_FWD_WS), (Lb.launch_plan(a, Lb.FASN_PLAN_BWD) if backward else [])


def described(pkg, a, backward=True):
    """the kernels of both plans as family<named template arguments>"""
    Lb = pkg._lib
    pl = Lb.launch_plan_described(a, Lb.FASN_PLAN_FWD_WS) + (Lb.launch_plan_described(a, Lb.FASN_PLAN_BWD) if backward else [])
    return [k for k, *_ in pl]


# ---------------------------------------------------------------- the call through the C ABI
def run(pkg, case, ops, scale, dtype, backward=True):
    """forward (and backward) over ops through libfasn's C ABI. Returns (result dict in the layout of attn_witness.run, the block)."""
    from flash_attention_softmax_n_amd import flash_attn
    Lb = pkg._lib
    lib = Lb.load()
    t = ops.t
    dev = t["q"].device
    a = block(pkg, case, ops, scale, dtype, backward)
    f = a.fwd
    stream = flash_attn._stream_ptr(dev)
    wsb = lib.fasn_fwd_workspace_bytes(f)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    if t["n"] is not None:
        nsb, nsh = n_strides(t["n"])
        Lb.check(lib.fasn_fwd_n(f, t["n"].data_ptr(), nsb, nsh, None if ws is None else ws.data_ptr(), wsb, stream), "fasn_fwd_n")
    elif wsb:
        Lb.check(lib.fasn_fwd_ws(f, ws.data_ptr(), wsb, stream), "fasn_fwd_ws")
    else:
        Lb.check(lib.fasn_fwd(f, stream), "fasn_fwd")
    res = dict(out=t["o"], lse=t["lse"], dq=None, dk=None, dv=None, dn=None, dbias=None, state=STATE if case.p else None)
    if backward:
        Lb.check(lib.fasn_bwd(a, stream), "fasn_bwd")
        res.update(dq=t["dq"], dk=t["dk"], dv=t["dv"])
        if t["dbias"] is not None:
            res["dbias"] = t["dbias"][0] if t["dbias"].shape[0] == 1 and case.B > 1 else t["dbias"]
        if t["dn"] is not None:
            nb = lib.fasn_bwd_dn_workspace_bytes(a)
            wsn = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
            dsb, dsh = n_strides(t["dn"])
            Lb.check(lib.fasn_bwd_dn(a, t["dn"].data_ptr(), dsb, dsh, wsn.data_ptr(), nb, stream), "fasn_bwd_dn")
            res["dn"] = {"H": t["dn"][0], "B1": t["dn"], "BH": t["dn"]}[case.nshape]
    torch.cuda.synchronize()
    return res, a


# ---------------------------------------------------------------- the routes
def _route(*kernels, dtypes=("bf16",), **kw):
    """(case, dtypes): `kernels` are what the case is there for - strings its plan text must hold (the CPU suite asserts it); they are
    the case's `want`, on which attn_witness keys rounding point 7 (a two-wave kernel in the plan)"""
    return aw.Case(want=kernels, dtypes=dtypes, **kw), dtypes


ROUTES = {
    "d64 plain": _route("fasn_fwd_kernel<", "fasn_bwd_dq_pipe_kernel", "fasn_bwd_dkdv_pipe_kernel", dtypes=("bf16", "fp16"), B=3, H=4, L=300, S=420, D=64),
    "d64 causal L>S": _route("causal", "fasn_bwd_dq_pipe_kernel", B=3, H=4, L=420, S=300, D=64, causal=True, nshape="BH"),
    "d64 keypad": _route("keypad", "fasn_bwd_dq_kernel", "fasn_bwd_dkdv_kernel", dtypes=("bf16", "fp16"), B=3, H=4, L=300, S=420, D=64, mask="keypad",
                         lens=[420, 77, 300], nshape="B1"),
    "d64 QB=2": _route("D=64,QB=2,plain", B=8, H=64, L=256, S=70, D=64, nshape="BH"),
    "d64 float n": _route("fasn_fwd_kernel<", B=3, H=4, L=130, S=200, D=64, nshape="float"),
    "d64 gqa": _route("GQA=1", "fasn_bwd_dkdv_kernel", B=3, H=8, L=300, S=420, D=64, Hkv=2),
    "d64 drop": _route("DROP=1", B=3, H=4, L=300, S=420, D=64, p=0.1),
    "d64 bias": _route("fasn_bwd_dbias_kernel", dtypes=("bf16", "fp16"), B=3, H=4, L=300, S=420, D=64, bias="hls"),
    "d64 bias causal S%8": _route("fasn_bwd_dbias_ws_kernel", dtypes=("bf16", "fp16"), B=3, H=4, L=300, S=424, D=64, bias="hls", causal=True),
    "d64 dense dbias causal": _route("bias+mask", B=3, H=4, L=300, S=420, D=64, bias="bhls", mask="dense", causal=True),
    "element loads": _route("element-load", B=3, H=4, L=130, S=200, D=64, mask="misaligned"),
    "split": _route("SPLIT=1", "fasn_fwd_combine_kernel", dtypes=("bf16", "fp16"), B=1, H=4, L=130, S=4090, D=64, causal=True),
    "d32 plain": _route("D=32,QB=2", "KB=2", B=3, H=4, L=300, S=420, D=32, nshape="BH"),
    "d128 plain": _route("fasn_bwd_delta_kernel", "fasn_bwd_dq_ws_kernel", "fasn_bwd_dkdv_ws_kernel", dtypes=("bf16", "fp16"), B=3, H=4, L=300, S=420, D=128, nshape="BH"),
    "d128 bias keypad": _route("bias+keypad", "fasn_bwd_dq_ws_kernel", "fasn_bwd_dbias_ws_kernel", B=3, H=4, L=300, S=424, D=128, bias="hls", mask="keypad",
                               lens=[424, 77, 300]),
    "d256 plain": _route("fasn_fwd_ws256_kernel", "fasn_bwd_dq_ws256_kernel", "fasn_bwd_dkdv_ws256_kernel", dtypes=("bf16", "fp16"), B=3, H=4, L=200, S=320, D=256),
    "d256 causal gqa": _route("fasn_fwd_ws256_kernel", "fasn_bwd_dkdv_ws256_kernel", "GQA=1", B=3, H=8, L=200, S=200, D=256, Hkv=2, causal=True),
    "d256 bias": _route("fasn_bwd_dq_ws256_kernel", "fasn_bwd_dbias_kernel", "FAST=true", B=3, H=4, L=200, S=200, D=256, bias="hls"),
    "fp32": _route("fasn_f32_fwd_kernel", "fasn_f32_delta_kernel", "fasn_f32_dq_kernel", "fasn_f32_dkdv_kernel", dtypes=("fp32",), B=3, H=2, L=130, S=96, D=32),
}
STD = 4   # logit standard deviation of the operands (attn_witness.inputs_c)


def route_params():
    return [(name, dt) for name, (_, dts) in ROUTES.items() for dt in dts]


def seed_of(name):
    return 3000 + aw.seed_of(name)


def plan_lines(pl):
    return [f"    {k} grid={g} block={b} lds={l}" for k, g, b, l in pl]


def plans_file_text(pkg):
    """the plans of every route under L1, L2 and C from strides alone (meta tensors, fake addresses): one text per route, asserted the
    same under the three"""
    Lb = pkg._lib
    out = []
    for name, dt in route_params():
        case, dtype = ROUTES[name][0], aw.DTYPES[dt]
        texts = []
        for pairing in ("L1", "L2", "C"):
            ops = alloc(case, dtype, "meta", pairing)
            a = block(pkg, case, ops, 1.0 / math.sqrt(case.D), dtype)
            fw = Lb.launch_plan_described(a, Lb.FASN_PLAN_FWD_WS)
            bw = Lb.launch_plan_described(a, Lb.FASN_PLAN_BWD)
            texts.append("\n".join(["  [fwd]"] + plan_lines(fw) + ["  [bwd]"] + plan_lines(bw)))
        assert texts[0] == texts[1] == texts[2], f"{name} {dt}: the plan depends on the layout"
        out += [f"{name} [{dt}]", texts[0]]
    return "\n".join(out) + "\n"


# ---------------------------------------------------------------- the address arithmetic in plain integers
def addr_map(view):
    """element offsets [B, heads, T, D] (int64, CPU) of a view within its storage, from its strides and offset alone"""
    off = torch.full(tuple(view.shape), view.storage_offset(), dtype=torch.int64)
    for i, (n, s) in enumerate(zip(view.shape, view.stride())):
        shape = [1] * view.dim()
        shape[i] = n
        off = off + (torch.arange(n, dtype=torch.int64) * s).view(shape)
    return off


def write_model(view, store_numel, addr):
    """A kernel that writes element e of the view's logical tensor to storage offset addr[e] (same shape as the view), modelled on
    integers: the storage starts as the sentinel (-1), logical element e carries the id e. Returns (a_ok: the view reads back its own
    ids - check (a), the result equals the contiguous call's; b_ok: everything outside the view is still the sentinel - check (b);
    outside: how many writes fell out of the storage, which the model drops)."""
    ids = torch.arange(view.numel(), dtype=torch.int64).view(tuple(view.shape))
    flat = torch.full((store_numel,), -1, dtype=torch.int64)
    a = addr.reshape(-1)
    ok = (a >= 0) & (a < store_numel)
    flat[a[ok]] = ids.reshape(-1)[ok]
    right = addr_map(view)
    a_ok = bool((flat[right.reshape(-1)] == ids.reshape(-1)).all())
    inside = torch.zeros(store_numel, dtype=torch.bool)
    inside[right.reshape(-1)] = True
    b_ok = bool((flat[~inside] == -1).all())
    return a_ok, b_ok, int((~ok).sum())


def strided_addr(view, strides, offset=None, row_shift=0):
    """offsets of the view's elements under (batch, head, row) element strides `strides`, feature stride 1"""
    B, Hx, T, D = view.shape
    off = view.storage_offset() if offset is None else offset
    b, h, i, d = (torch.arange(n, dtype=torch.int64) for n in (B, Hx, T, D))
    return (off + b.view(B, 1, 1, 1) * strides[0] + h.view(1, Hx, 1, 1) * strides[1] + (i.view(1, 1, T, 1) + row_shift) * strides[2] + d.view(1, 1, 1, D))


# ---------------------------------------------------------------- layout F: offsets beyond 2^31 and 2^32 bytes
FAR_SLOT = 4 << 20          # bytes of arena per tensor (and per far element of it)
FAR_M = 32 << 20            # the far stride is 2^31 + FAR_M bytes: wrapped offsets land FAR_M and 2 FAR_M beyond the tensor's base
FAR_STRIDE = (1 << 31) + FAR_M
FAR_NAMES = ("q", "k", "v", "o", "dout", "dq", "dk", "dv")
FAR_BYTES = (1 << 32) + 2 * FAR_M + len(FAR_NAMES) * FAR_SLOT   # about 4.1 GiB
# regions of len(FAR_NAMES) slots each: where far elements 0, 1, 2 of the tensors lie, and the aliases of elements 1 and 2
FAR_USED = (0, FAR_STRIDE, 2 * FAR_STRIDE)
FAR_ALIAS = (FAR_M, 2 * FAR_M)


def far_offsets(j, esize=2):
    """tensor j of the arena: byte offsets of its far elements 0, 1, 2 and of the slots the wrapped offsets would hit - element 1 taken
    mod 2^31 bytes, element 2 mod 2^32 bytes, mod 2^31 bytes and (16-bit types) mod 2^31 elements"""
    base = j * FAR_SLOT
    used = [base + i * FAR_STRIDE for i in range(3)]
    rel = [i * FAR_STRIDE for i in range(3)]
    wrapped = {rel[1] % (1 << 31), rel[2] % (1 << 32), rel[2] % (1 << 31), ((rel[2] // esize) % (1 << 31)) * esize}
    alias = sorted(base + w for w in wrapped)
    return used, alias


def far_view(arena, j, shape, dtype, dim):
    """tensor j as a [B, heads, T, D] view of the arena (int16 storage) whose dimension `dim` (0: batch - layout F; 1: heads - F') has the
    far stride and whose other dimensions are dense"""
    B, Hx, T, D = shape
    esize = torch.empty((), dtype=dtype).element_size()
    assert shape[dim] == 3 and FAR_STRIDE % (8 * esize) == 0
    a = arena.view(INT[esize])
    far = FAR_STRIDE // esize
    strides = (far, T * D, D, 1) if dim == 0 else (T * D, far, D, 1)
    assert shape[1 - dim] * T * D * esize <= FAR_SLOT
    return torch.as_strided(a, shape, strides, j * FAR_SLOT // esize).view(dtype)


def far_regions(arena):
    """the five regions as int16 views: used 0 / 1 / 2 and alias 1 / 2"""
    n = len(FAR_NAMES) * FAR_SLOT // 2
    return [arena[o // 2:o // 2 + n] for o in FAR_USED + FAR_ALIAS]


def far_ops(case, dtype, arena, dim):
    """the case's operands with the eight 4-D tensors (dim 0), or K, V, dK, dV (dim 1: the K/V heads far apart, under grouped K/V), in
    the arena and everything else as under L1. The five regions are refilled with the sentinel first."""
    assert arena.dtype == torch.int16 and arena.numel() * 2 >= FAR_BYTES
    esize = torch.empty((), dtype=dtype).element_size()
    for reg in far_regions(arena):
        reg.view(INT[esize]).fill_(SENT[dtype])
    ops = alloc(case, dtype, arena.device, "L1")
    far = []
    for j, name in enumerate(FAR_NAMES):
        if dim == 1 and name not in ("k", "v", "dk", "dv"):
            continue
        ops.put(name, far_view(arena, j, tuple(ops.t[name].shape), dtype, dim), None)
        far.append(name)
    return ops, far


def far_intact(arena, ops, far, dtype):
    """check (b) under F: outside the views the three used regions, and the whole of the two alias regions, still hold the sentinel"""
    esize = torch.empty((), dtype=dtype).element_size()
    a = arena.view(INT[esize])
    inside = {}
    for name in far:   # mark the views' own elements in a scratch copy of the used regions
        t = ops.t[name]
        for i in range(3):
            lo = FAR_USED[i] // esize
            n = len(FAR_NAMES) * FAR_SLOT // esize
            if i not in inside:
                inside[i] = a[lo:lo + n].clone()
            sub = t[i] if t.stride(0) == FAR_STRIDE // esize else t[:, i]
            torch.as_strided(inside[i], tuple(sub.shape), tuple(sub.stride()), sub.storage_offset() - lo).fill_(SENT[dtype])
    ok = all(bool((r == SENT[dtype]).all()) for r in inside.values())
    return ok and all(bool((reg.view(INT[esize]) == SENT[dtype]).all()) for reg in far_regions(arena)[3:])


# one case per address-forming source text: (case, dtype, far dimension - 0: the batch elements of all eight tensors, 1: the K/V heads)
FAR = {
    "fwd_kernel + bwd_pipe": (ROUTES["d64 plain"][0], "bf16", 0),
    "bwd_kernel, K/V heads far (F')": (_route("GQA=1", "fasn_bwd_dq_kernel", "fasn_bwd_dkdv_kernel", B=3, H=6, L=300, S=420, D=64, Hkv=3, nshape="BH")[0], "bf16", 1),
    "bwd_kernel keypad": (ROUTES["d64 keypad"][0], "bf16", 0),
    "split-K combine": (_route("SPLIT=1", "fasn_fwd_combine_kernel", B=3, H=4, L=130, S=4090, D=64, causal=True)[0], "bf16", 0),
    "f32_kernels": (ROUTES["fp32"][0], "fp32", 0),
    "dq_ws + dkdv_ws": (ROUTES["d128 plain"][0], "bf16", 0),
    "fwd_ws256 + bwd_ws256": (ROUTES["d256 plain"][0], "bf16", 0),
    "fwd_ws256 + bwd_ws256, K/V heads far (F')": (_route("fasn_fwd_ws256_kernel", "fasn_bwd_dkdv_ws256_kernel", "GQA=1", B=3, H=6, L=200, S=200, D=256, Hkv=3, causal=True)[0], "bf16", 1),
    "bwd_dbias": (ROUTES["d64 bias"][0], "bf16", 0),
    "bwd_dbias_ws": (ROUTES["d128 bias keypad"][0], "bf16", 0),
}


# ---------------------------------------------------------------- the largest row stride the host admits
def max_row_stride(rows, D, esize=2):
    """the largest row stride (elements, a multiple of 16 bytes) at which `rows` rows of D elements span less than 2^31 bytes"""
    q = 16 // esize
    s = (((1 << 31) - 1) // esize - D) // (rows - 1) // q * q
    assert ((rows - 1) * s + D) * esize < (1 << 31) <= ((rows - 1) * (s + q) + D) * esize
    return s


def wide_view(shape, dtype, dev, row_stride, head_stride):
    """[1, heads, T, D] in an uninitialised buffer, rows `row_stride` elements apart, the heads `head_stride` apart inside a row's stretch"""
    B, Hx, T, D = shape
    assert B == 1 and (Hx - 1) * head_stride + D <= row_stride
    buf = torch.empty((T - 1) * row_stride + (Hx - 1) * head_stride + D, dtype=dtype, device=dev)
    return torch.as_strided(buf, shape, (buf.numel(), head_stride, row_stride, 1))
