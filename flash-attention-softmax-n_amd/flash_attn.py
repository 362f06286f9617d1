"""Host side of the hot path: the reference's attention API on top of libfasn (HIP, gfx950).

Mirrors, argument for argument:
  * flash_attention_n          — flash_attention_softmax_n/core/flash_attn.py:42-124
  * flash_attention_n_triton   — flash_attention_softmax_n/core/flash_attn_triton.py:339-357
  * slow_attention_n           — flash_attention_softmax_n/core/functional.py:32-93 (signature only; same kernel)
What the reference does by materialising tensors is passed to the kernel as scalars and strides:
  n zero-padded K/V rows (flash_attn.py:66-73)        -> `softmax_n` float (real-valued n allowed)
  q * scale/default (flash_attn.py:81-83)             -> `scale` float; the vector kernels multiply Q (or K) by scale*log2e once, in
                                                         registers, rounded to the operand type like the reference's pre-scaled q;
                                                         only the element-load kernels apply it in fp32 inside the exp2 argument
  dense [B,H,L,S] mask & bias (flash_attn.py:87-113)  -> broadcast strides (0 = broadcast), `causal` flag
PyTorch is used for device memory, streams and autograd only.
"""
from math import sqrt
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import BwdArgs, FwdArgs, View4

_SUPPORTED_D = (32, 64, 128, 256)
_DTYPES = {torch.float16: _lib.FASN_DTYPE_F16, torch.bfloat16: _lib.FASN_DTYPE_BF16, torch.float32: _lib.FASN_DTYPE_F32}


def _view4(t: Optional[Tensor]) -> View4:
    v = View4()
    if t is None:
        v.ptr = None
        return v
    v.ptr = t.data_ptr()
    for i in range(4):
        v.stride[i] = t.stride(i) if t.size(i) > 1 else 0
    v.stride[3] = 1 if t.size(3) == 1 else t.stride(3)
    return v


def _rows_ok(t: Tensor) -> bool:
    """16-byte row alignment rule of the C ABI (strides % 8 elements for 16-bit types, % 4 for fp32)."""
    if t.stride(-1) != 1 and t.size(-1) != 1:
        return False
    if t.data_ptr() % 16 != 0:
        return False
    q = 16 // t.element_size()
    return all(t.stride(i) % q == 0 or t.size(i) == 1 for i in range(t.dim() - 1))


def _span_ok(t: Tensor) -> bool:
    """The span rule of the C ABI (include/fasn.h): one (batch, head) matrix - the last row's start plus one row - spans less than 2^31
    bytes. fasn_fwd refuses a K or V beyond it and fasn_bwd a Q or dO as well (the forward reads Q by 64-bit addresses), so a packed
    buffer at a very long context would run its forward and fail its backward with a bare FASN_EINVAL."""
    return ((t.size(-2) - 1) * t.stride(-2) + t.size(-1)) * t.element_size() < (1 << 31)


def _canon(t: Tensor) -> Tensor:
    """the operand as the kernels take it: itself, or a contiguous copy where its rows break the alignment rule or its (b, h) span the
    span rule (a contiguous tensor beyond the span rule stays as it is: the call reports it)"""
    if t.is_contiguous() and t.data_ptr() % 16 == 0 and (t.shape[-1] * t.element_size()) % 16 == 0:
        return t   # the common case, one C++ call instead of a stride walk
    if _rows_ok(t) and _span_ok(t):
        return t
    c = t.contiguous()
    # a contiguous tensor whose base is off the 16-byte alignment (a slice of a flat buffer) is its own .contiguous(): only a clone moves it
    return c.clone() if c.data_ptr() % 16 else c


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # the current stream's handle without building a torch.cuda.Stream object (6 us of host time per launch)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream_ptr(device) -> int:
    if _raw_stream is not None and device.index is not None:
        return _raw_stream(device.index)
    return torch.cuda.current_stream(device).cuda_stream


def _current_device() -> int:
    return _raw_device() if _raw_device is not None else torch.cuda.current_device()


# ---- dropout stream (reference: torch's philox generator behind core/flash_attn.py:122 and core/functional.py:92) ----
# Eager calls: a call's (seed, offset) is a PURE FUNCTION of torch's CUDA generator of the device at call time - seed =
# initial_seed(), offset = its philox offset, which the call then advances by 4 as any torch random op would - and travels by
# value. torch.manual_seed reproduces a run, and whatever saves / restores the generator state (torch.utils.checkpoint,
# HF gradient_checkpointing) makes the recomputed forward draw the mask of the original one.
# Under HIP-graph capture nothing on the host runs at replay time, so captured calls draw from a {seed, offset} pair in DEVICE
# memory instead: one tiny captured kernel (fasn_rng_advance) hands the call its copy and advances the pair, so every replay
# resamples. The pair is created by the first eager dropout call after the generator was (re)seeded, with bit 62 of the offset
# set: the graph stream and the eager stream of one seed never share a position.
_RNG_STATE = {}
_GRAPH_STREAM_BIT = 1 << 62


def _next_rng_state(device):
    """(seed, offset) Python ints for one eager forward call, or - while the current stream is capturing - an int64[2] device
    tensor {seed, offset} filled by a captured kernel. The backward of the call gets the same object."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _RNG_STATE.get(idx)
    if not torch.cuda.is_current_stream_capturing():
        gen = torch.cuda.default_generators[idx]
        seed, off = gen.initial_seed(), gen.get_offset()
        gen.set_offset(off + 4)
        if st is None or st["seed"] != seed:   # first use, or the generator was re-seeded: (re)start the graph stream
            signed = seed - (1 << 64) if seed >= (1 << 63) else seed
            fresh = torch.tensor([signed, _GRAPH_STREAM_BIT + off], dtype=torch.int64)
            if st is None:
                _RNG_STATE[idx] = {"seed": seed, "state": fresh.to(device)}
            else:   # IN PLACE: a HIP graph captured earlier holds this tensor's address (fasn_rng_advance adds to it at every replay);
                    # a new allocation would leave that graph writing into memory the caching allocator hands out again
                st["state"].copy_(fresh)
                st["seed"] = seed
        return seed & 0xFFFFFFFFFFFFFFFF, off & 0xFFFFFFFFFFFFFFFF
    if st is None:
        raise RuntimeError("dropout inside a HIP graph capture: run one dropout call on this device before capturing "
                           "(the device-side random state is created on first use)")
    out = torch.empty(2, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().fasn_rng_advance(st["state"].data_ptr(), out.data_ptr(), 1, _stream_ptr(device)), "fasn_rng_advance")
    return out


def _fill_fwd(a: FwdArgs, q, k, v, o, lse, mask, bias, n, scale, causal, dropout_p=0.0, seed=0, offset=0, rng=None):
    a.q, a.k, a.v, a.o = _view4(q), _view4(k), _view4(v), _view4(o)
    a.lse = lse.data_ptr()
    a.mask = _view4(mask)
    a.bias = _view4(bias)
    if bias is not None:
        a.bias_dtype = _lib.FASN_BIAS_F32 if bias.dtype == torch.float32 else _lib.FASN_BIAS_SAME
    else:
        a.bias_dtype = _lib.FASN_BIAS_NONE
    a.dtype = _DTYPES[q.dtype]
    a.B, a.H, a.Sq, a.D = q.shape
    a.Sk = k.shape[2]
    a.Dv = v.shape[3]
    a.kv_group = q.shape[1] // k.shape[1] if k.shape[1] != q.shape[1] else 0   # grouped-query attention: fewer K/V heads
    a.scale = scale
    a.softmax_n = n
    a.causal = 1 if causal else 0
    a.dropout_p = dropout_p
    if isinstance(rng, tuple):     # eager call: this call's (seed, offset) by value
        a.seed, a.offset = rng
        a.rng_state = None
    else:                          # captured call: device {seed, offset} (or no dropout)
        a.seed, a.offset = seed, offset
        a.rng_state = None if rng is None else rng.data_ptr()


# ---- host path: one planned ABI call per pass, argument blocks cached per call signature -------------------------------------
# Filling a ctypes struct costs ~0.15 us per field and a fasn_*_workspace_bytes() round trip ~2 us; both depend only on shapes,
# strides, dtype and the scalar arguments. They are computed once per distinct signature (per thread: the cached block is
# mutated in place) and a call only rewrites the pointers (reference launch site: core/flash_attn_triton.py:278-291, which
# likewise passes raw pointers + strides per call).
import threading

_TLS = threading.local()


def _sig(t: Optional[Tensor]):
    return None if t is None else (t.shape, t.stride(), t.dtype)


def _cache():
    c = getattr(_TLS, "cache", None)
    if c is None:
        c = _TLS.cache = {}
    return c


class _Plan:
    __slots__ = ("fwd", "fwd_ws", "bwd", "bwd_ws", "path", "bwd_path", "dn_ws")


# n given as a tensor (per batch element / head): its values travel as a pointer per call (fasn_fwd_n), never in the cached argument block,
# whose softmax_n is then 0 - so a cached plan can never replay another call's n
_N_TENSOR = "tensor"


def _n_strides(nt: Tensor):
    """(batch, head) element strides of a [1 or B, 1 or H] fp32 n for fasn_fwd_n / fasn_bwd_dn: 0 over a size-1 dimension (broadcast on the way
    in, the sum over that dimension on the way out)."""
    return (nt.stride(0) if nt.shape[0] > 1 else 0), (nt.stride(1) if nt.shape[1] > 1 else 0)


_WARNED_SLOW = set()


def _plan_for(q, k, v, mask, bias, n, scale, causal, dropout_p):
    if isinstance(n, Tensor) or n is _N_TENSOR:
        n = _N_TENSOR
    key = (_sig(q), _sig(k), _sig(v), _sig(mask), _sig(bias), n, scale, causal, dropout_p, q.device.index)
    c = _cache()
    pl = c.get(key)
    if pl is None:
        if len(c) > 256:
            c.clear()
        lib = _lib.load()
        B, H, L, _ = q.shape
        o = torch.empty((B, H, L, v.shape[3]), dtype=q.dtype, device=q.device)
        lse = torch.empty((B, H, L), dtype=torch.float32, device=q.device)
        pl = _Plan()
        n_val = 0.0 if n is _N_TENSOR else n
        pl.fwd = FwdArgs()
        _fill_fwd(pl.fwd, q, k, v, o, lse, mask, bias, n_val, scale, causal, dropout_p)
        pl.bwd = BwdArgs()
        _fill_fwd(pl.bwd.fwd, q, k, v, o, lse, mask, bias, n_val, scale, causal, dropout_p)
        pl.dn_ws = None   # asked at the first backward that wants the gradient of a tensor n
        dk = torch.empty((B, k.shape[1], k.shape[2], k.shape[3]), dtype=q.dtype, device=q.device)   # contiguous outputs: only the strides matter here
        pl.bwd.dout, pl.bwd.dq, pl.bwd.dk, pl.bwd.dv = _view4(o), _view4(o), _view4(dk), _view4(dk)
        pl.bwd.flags = 0
        with torch.cuda.device(q.device):
            pl.fwd_ws = lib.fasn_fwd_workspace_bytes(pl.fwd)     # > 0: short-query / long-key shape, keys split over workgroups
            pl.bwd_ws = lib.fasn_bwd_workspace_bytes(pl.bwd)     # 0 with libfasn.so (the ABI keeps the hook for plans that need scratch)
            pl.path = lib.fasn_fwd_path(pl.fwd)
            pl.bwd_path = None   # asked at the first backward (fasn_bwd_path wants the backward's real argument block)
        if pl.path == _lib.FASN_PATH_ELEMENT:   # same results, 3-5 x slower: say so once per kind of call instead of silently
            why = (_sig(mask), _sig(bias), dropout_p > 0.0)
            if why not in _WARNED_SLOW:
                _WARNED_SLOW.add(why)
                import warnings
                warnings.warn("flash_attention_n: this call takes the element-load kernels (3-5x slower than the vector path): "
                              "a mask / bias whose rows are not aligned vectors (unaligned or strided rows; an fp32 bias with 16-bit q at head dim 256, under dropout or with rows not 16-byte aligned), "
                              "scale <= 0 with a bias, or fp16 with a very large scale. "
                              "See fasn_fwd_path in include/fasn.h.", RuntimeWarning, stacklevel=4)
        c[key] = pl
    return pl


def _set_rng(a: FwdArgs, rng):
    if isinstance(rng, tuple):     # eager call: this call's (seed, offset) by value
        a.seed, a.offset = rng
        a.rng_state = None
    else:                          # captured call: device {seed, offset} (or no dropout)
        a.seed = a.offset = 0
        a.rng_state = None if rng is None else rng.data_ptr()


def _launch_fwd(q, k, v, mask, bias, n, scale, causal, dropout_p, rng):
    lib = _lib.load()
    B, H, L, _ = q.shape
    o = torch.empty((B, H, L, v.shape[3]), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=q.device)
    pl = _plan_for(q, k, v, mask, bias, n, scale, causal, dropout_p)
    a = pl.fwd
    a.q.ptr, a.k.ptr, a.v.ptr, a.o.ptr, a.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr()
    if mask is not None:
        a.mask.ptr = mask.data_ptr()
    if bias is not None:
        a.bias.ptr = bias.data_ptr()
    if dropout_p > 0.0:
        _set_rng(a, rng)
    dev = q.device

    def launch():
        if isinstance(n, Tensor):   # per-(batch, head) n: same plan as fasn_fwd_ws, n read per work item
            ws = torch.empty(pl.fwd_ws, dtype=torch.uint8, device=dev) if pl.fwd_ws else None
            nsb, nsh = _n_strides(n)
            _lib.check(lib.fasn_fwd_n(a, n.data_ptr(), nsb, nsh, None if ws is None else ws.data_ptr(), pl.fwd_ws, _stream_ptr(dev)), "fasn_fwd_n")
        elif pl.fwd_ws:
            ws = torch.empty(pl.fwd_ws, dtype=torch.uint8, device=dev)
            _lib.check(lib.fasn_fwd_ws(a, ws.data_ptr(), pl.fwd_ws, _stream_ptr(dev)), "fasn_fwd_ws")
        else:
            rc = lib.fasn_fwd(a, _stream_ptr(dev))
            if rc:
                _lib.check(rc, "fasn_fwd")

    if _current_device() == dev.index:   # the usual case: no device-guard object on the plain path
        launch()
    else:
        with torch.cuda.device(dev):
            launch()
    return o, lse


_POISON_SCRATCH = False   # test hook: fill the backward's scratch (delta) with NaN before the launch


class _FlashAttentionSoftmaxN(torch.autograd.Function):
    """autograd glue; same role as _FlashAttentionN (flash_attn_triton.py:241-336)."""

    @staticmethod
    def forward(ctx, q, k, v, mask, bias, n, scale: float, causal: bool, dropout_p: float = 0.0, rng=None, bias_small: bool = False):
        # bias_small: `bias` is the caller's [1 or B, 1 or H, L, S] tensor, not yet expanded - its gradient then comes back in that
        # shape, summed over the broadcast batch / head dimensions inside the dbias kernel (no [B,H,L,S] buffer)
        # n: a float, or a [1 or B, 1 or H] fp32 tensor (per batch element / head; its gradient comes back in that shape, fasn_bwd_dn)
        bias_k = bias.expand(q.shape[0], q.shape[1], q.shape[2], k.shape[2]) if bias_small else bias
        o, lse = _launch_fwd(q, k, v, mask, bias_k, n, scale, causal, dropout_p, rng)
        ctx.save_for_backward(q, k, v, o, lse, mask, bias)
        ctx.n_shape = tuple(n.shape) if isinstance(n, Tensor) else None
        if isinstance(n, Tensor):
            n = _N_TENSOR
        ctx.n, ctx.scale, ctx.causal, ctx.dropout_p, ctx.rng, ctx.bias_small = n, scale, causal, dropout_p, rng, bias_small
        return o

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        q, k, v, o, lse, mask, bias = ctx.saved_tensors
        dout = _canon(dout)
        B, H, L, D = q.shape
        S = k.shape[2]
        dev = q.device
        bias_small = bias if ctx.bias_small else None
        if ctx.bias_small:
            bias = bias.expand(B, H, L, S)
        dq = torch.empty((B, H, L, D), dtype=q.dtype, device=dev)
        Hkv = k.shape[1]   # grouped-query attention: each dK/dV workgroup sums the query heads of its K/V head in registers
        dk = torch.empty((B, Hkv, S, D), dtype=q.dtype, device=dev)
        dv = torch.empty((B, Hkv, S, v.shape[3]), dtype=q.dtype, device=dev)
        delta = torch.empty((B, H, L), dtype=torch.float32, device=dev)
        if _POISON_SCRATCH:   # tests: every kernel that reads delta must find it written (by fasn_bwd_delta or the dQ kernel's prologue)
            delta.fill_(float("nan"))
        pl = _plan_for(q, k, v, mask, bias, ctx.n, ctx.scale, ctx.causal, ctx.dropout_p)
        a = pl.bwd
        f = a.fwd
        f.q.ptr, f.k.ptr, f.v.ptr, f.o.ptr, f.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr()
        if mask is not None:
            f.mask.ptr = mask.data_ptr()
        if bias is not None:
            f.bias.ptr = bias.data_ptr()
        if ctx.dropout_p > 0.0:
            _set_rng(f, ctx.rng)
        if dout.stride() == o.stride():
            a.dout.ptr = dout.data_ptr()
        else:
            a.dout = _view4(dout)
        a.dq.ptr, a.dk.ptr, a.dv.ptr, a.delta = dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr()
        a.workspace, a.workspace_bytes = None, 0
        # gradient of attn_bias: the kernel writes dS densely; autograd sums it over the dimensions the caller's bias broadcasts
        # (the expand / unsqueeze / dtype cast in _attention are ordinary autograd ops)
        dbias = None
        a.dbias_dtype = 0
        if bias is not None and ctx.needs_input_grad[4]:
            if bias_small is not None:   # reduced form: the kernel sums over the bias's broadcast batch / head dimensions
                dbias = torch.empty(bias_small.shape, dtype=bias_small.dtype, device=dev)
                a.dbias = _view4(dbias)   # (size-1 dimensions get stride 0 = "reduce over this dimension")
                a.dbias_dtype = _lib.FASN_BIAS_F32 if dbias.dtype == torch.float32 else _lib.FASN_BIAS_SAME
            else:
                dbias = torch.zeros((B, H, L, S), dtype=q.dtype, device=dev)   # tiles the causal walk skips are never written
                a.dbias = _view4(dbias)
        else:
            a.dbias.ptr = None
        if pl.bwd_path is None:   # once per cached call signature
            path = lib.fasn_bwd_path(a)
            if path >= 0:   # (a refusal is no answer: the fasn_bwd below reports the same code, and the next backward asks again)
                pl.bwd_path = path
            if path == _lib.FASN_PATH_ELEMENT and pl.path != _lib.FASN_PATH_ELEMENT:
                why = ("bwd", _sig(mask), _sig(bias), D)
                if why not in _WARNED_SLOW:
                    _WARNED_SLOW.add(why)
                    import warnings
                    warnings.warn("flash_attention_n backward: dQ / dK / dV of this call take the element-load kernels (3-5x slower) although its forward "
                                  "is on the vector path. See fasn_bwd_path in include/fasn.h.", RuntimeWarning, stacklevel=2)

        dn = None
        if ctx.n_shape is not None and ctx.needs_input_grad[5]:
            dn = torch.empty(ctx.n_shape, dtype=torch.float32, device=dev)

        def launch():
            if pl.bwd_ws:
                ws = torch.empty(pl.bwd_ws, dtype=torch.uint8, device=dev)
                a.workspace, a.workspace_bytes = ws.data_ptr(), pl.bwd_ws
            rc = lib.fasn_bwd(a, _stream_ptr(dev))
            if rc:
                _lib.check(rc, "fasn_bwd")
            if dn is not None:   # dL/dn = -sum_i delta_i exp(-lse_i), summed over the dimensions n broadcasts over
                if pl.dn_ws is None:
                    pl.dn_ws = lib.fasn_bwd_dn_workspace_bytes(a)
                wsn = torch.empty(pl.dn_ws, dtype=torch.uint8, device=dev)
                dsb, dsh = _n_strides(dn)
                _lib.check(lib.fasn_bwd_dn(a, dn.data_ptr(), dsb, dsh, wsn.data_ptr(), pl.dn_ws, _stream_ptr(dev)), "fasn_bwd_dn")

        try:
            if _current_device() == dev.index:   # the usual case: no device-guard object (about 10 us of host time per step)
                launch()
            else:
                with torch.cuda.device(dev):
                    launch()
        finally:   # the block is cached per call signature: whatever this call changed beyond pointers goes back, also when the launch raised
            if dout.stride() != o.stride():
                a.dout = _view4(o)
            a.dbias.ptr = None
        if dbias is not None and dbias.dtype != bias.dtype:
            dbias = dbias.to(bias.dtype)
        return dq, dk, dv, None, dbias, dn, None, None, None, None, None


def _pad_feature(t: Tensor, d: int) -> Tensor:
    return t if t.shape[-1] == d else torch.nn.functional.pad(t, (0, d - t.shape[-1]))


def _n_tensor(n: Tensor, query: Tensor) -> Tensor:
    """softmax_n given as a tensor that broadcasts to [B, H] ([H], [1, H], [B, 1], [B, H] or 0-d; H = query heads): the fp32 [1 or B,
    1 or H] view the kernels read per (batch, head). `.float()` and the reshape are autograd ops, so the gradient reaches the caller's
    tensor in its own shape and dtype. The values are not looked at (no host round trip: capturable)."""
    B, H = query.shape[0], query.shape[1]
    if not n.is_floating_point():
        raise TypeError(f"softmax_n_param as a tensor must be floating point; got {n.dtype}")
    if n.device != query.device:
        raise ValueError(f"softmax_n_param is on {n.device}, query on {query.device}: pass n on the query's device")
    if n.dim() > 2:
        raise ValueError(f"softmax_n_param must broadcast to [B, H] = [{B}, {H}] ([H], [1, H], [B, 1], [B, H] or 0-d); got {tuple(n.shape)}")
    nt = n.float().reshape((1,) * (2 - n.dim()) + tuple(n.shape))
    if nt.shape[0] not in (1, B) or nt.shape[1] not in (1, H):
        raise ValueError(f"softmax_n_param must broadcast to [B, H] = [{B}, {H}] ([H], [1, H], [B, 1], [B, H] or 0-d); got {tuple(n.shape)}")
    return nt


def _prepare(query, key, value, n, scale, dropout_p, mask, bias):
    """Argument normalisation shared by flash_attention_n and kernel_path: validation, K/V head expansion, sign of the scale, feature
    padding, row alignment, mask / bias broadcasting. Returns (q, k, v, mask, bias, n, scale, dropout_p, dpad, Ev, bias_small)."""
    if not query.is_cuda:
        raise RuntimeError("flash_attention_softmax_n_amd runs on MI355X device tensors only; got a CPU tensor "
                           "(there is deliberately no CPU fallback)")
    if query.dtype not in _DTYPES:
        raise NotImplementedError(f"dtype {query.dtype}: supported are torch.float16, torch.bfloat16 and torch.float32")
    if key.dtype != query.dtype or value.dtype != query.dtype:
        raise TypeError("query, key and value must share one dtype")
    dropout_p = float(dropout_p or 0.0)
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError("dropout_p must be in [0, 1)")
    if query.dim() != 4:
        raise ValueError("query must be [B, H, L, E]")
    B, H, L, E = query.shape
    if isinstance(n, Tensor):
        n = _n_tensor(n, query)
    else:
        n = 0.0 if n is None else float(n)
        if n < 0:
            raise ValueError("softmax_n_param must be >= 0")

    # 3-D key/value [B, S, E] = one K/V shared by all heads: a stride-0 head dimension, no copy
    if key.dim() == 3:
        key = key.unsqueeze(1).expand(B, H, key.shape[1], key.shape[2])
    if value.dim() == 3:
        value = value.unsqueeze(1).expand(B, H, value.shape[1], value.shape[2])
    S, Ev = key.shape[2], value.shape[3]
    if key.shape[3] != E or value.shape[2] != S:
        raise ValueError("key must be [B,H,S,E] and value [B,H,S,Ev]")
    Hkv = key.shape[1]
    if Hkv not in (1, H) and (H % Hkv != 0 or value.shape[1] != Hkv):
        raise ValueError(f"key/value have {Hkv} heads: must be 1, {H}, or a divisor of {H} (grouped-query attention)")
    if Hkv == H:
        pass
    elif Hkv == 1:
        key = key.expand(B, H, S, E)
        value = value.expand(B, H, S, Ev)
    else:   # grouped-query attention: query head h reads K/V head h // (H // Hkv), through the head stride (no copy)
        key = key.expand(B, Hkv, S, E)
        value = value.expand(B, Hkv, S, Ev)

    scale = (1.0 / sqrt(E)) if scale is None else float(scale)
    if scale < 0:  # exp2 folding assumes scale >= 0: move the sign into q
        query, scale = -query, -scale

    # feature dims: kernels exist for D == Dv in {32, 64, 128} and (fp16 / bf16) 256; anything else is zero-padded (exact)
    dmax = 128 if query.dtype == torch.float32 else 256
    dpad = next((d for d in _SUPPORTED_D if max(E, Ev) <= d <= dmax), None)
    if dpad is None:
        raise NotImplementedError(f"head dim {max(E, Ev)} > {dmax} is not supported for {query.dtype}")
    if E == dpad and Ev == dpad:
        q, k, v = _canon(query), _canon(key), _canon(value)
    else:
        q, k, v = (_canon(_pad_feature(t, dpad)) for t in (query, key, value))

    if mask is not None:
        if mask.dim() != 4:
            raise AssertionError("attn_mask must be 4-D and broadcastable to [B, H, L, S]")  # flash_attn.py:88
        if mask.dtype != torch.bool:
            raise TypeError("attn_mask must be boolean (True = attend); pass additive masks as attn_bias")
        # bool -> uint8 reinterpretation keeps the (possibly stride-0) broadcast strides: no dense copy
        mask = mask.expand(B, H, L, S).view(torch.uint8)
    if bias is not None:
        if bias.dim() == 3:
            bias = bias.unsqueeze(0)  # [H,L,S] -> [1,H,L,S]  (flash_attn.py:101-102)
        if bias.dim() != 4:
            raise ValueError("attn_bias must be [H, L, S] or broadcastable to [B, H, L, S]")
        if bias.dtype not in (query.dtype, torch.float32):
            bias = bias.to(query.dtype)
        # a bias that needs a gradient and broadcasts over batch and / or heads only ([H,L,S], [1,H,L,S], [B,1,L,S], [1,1,L,S]) keeps
        # its own shape: fasn_bwd then returns the gradient already summed over those dimensions (csrc/fasn_bwd_dbias.h).
        # (L == 1 stays on the dense path: a one-row bias is also a ROW broadcast, whose stride 0 the reduced form rejects)
        # Round 5: a bias that ALSO broadcasts over rows ([1,H,1,S], [B,1,1,S], [1,1,1,S] - per-key biases) is expanded over the rows as a
        # view (row stride 0: the kernels read one row) and takes the same reduced form: the kernel sums over batch / heads into a
        # [1 or B, 1 or H, L, S] buffer and the expand's own backward sums that over the rows - 1/B or 1/H of the dense [B,H,L,S] dS buffer
        # round 4 wrote for these shapes. (The sum over rows inside the kernel would be a column sum of dS in the dK/dV kernels: not built.)
        if (bias.requires_grad and torch.is_grad_enabled() and L > 1 and bias.shape[2] == 1 and bias.shape[3] == S
                and bias.shape[0] in (1, B) and bias.shape[1] in (1, H)):
            bias = bias.expand(bias.shape[0], bias.shape[1], L, S)
        bias_small = (bias.requires_grad and torch.is_grad_enabled() and dropout_p == 0.0 and query.dtype != torch.float32
                      and L > 1 and bias.shape[2] == L and bias.shape[3] == S and bias.shape[0] in (1, B) and bias.shape[1] in (1, H)
                      and ((bias.shape[0] == 1 and B > 1) or (bias.shape[1] == 1 and H > 1)) and bias.stride(3) == 1)
        if not bias_small:
            bias = bias.expand(B, H, L, S)
    if bias is None:
        bias_small = False
    return q, k, v, mask, bias, n, scale, dropout_p, dpad, Ev, bias_small


def _regroup_decode(q, k, mask, bias, dropout_p):
    """Grouped-query decode (one query position, fewer K/V heads than query heads, no dropout): the G query heads of a group become G
    query ROWS of one problem per K/V head, so each K/V head is streamed once instead of G times. With one query position a row sees
    every key, so causal needs no flag, and a [B,H,1,S] mask / bias is a per-row mask / bias of the regrouped problem. All of it is
    views. Returns (q, mask, bias) of the regrouped problem, or None when the call keeps the per-head launch."""
    B, H, L, dpad = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    if not (L == 1 and Hkv != H and dropout_p == 0.0):
        return None
    G = H // Hkv
    try:
        mask_g = None if mask is None else mask.view(B, Hkv, G, S)
        bias_g = None if bias is None else bias.expand(B, H, L, S).view(B, Hkv, G, S)
    except RuntimeError:      # strides that cannot be regrouped without a copy: keep the per-head launch
        return None
    return q.view(B, Hkv, G, dpad), mask_g, bias_g


def _attention(query, key, value, n, scale, dropout_p, mask, bias, is_causal) -> Tensor:
    q, k, v, mask, bias, n, scale, dropout_p, dpad, Ev, bias_small = _prepare(query, key, value, n, scale, dropout_p, mask, bias)
    B, H, L, _ = q.shape
    S = k.shape[2]
    # dropout: this call's (seed, offset) (see _next_rng_state); the kernels derive every keep/drop bit from
    # (seed, offset, b, h, row, key) - dropout.py is the host mirror
    rng = _next_rng_state(query.device) if dropout_p > 0.0 else None
    _TLS.last_rng_state = rng   # per thread: what last_dropout_state() / last_rng_state() report
    tensor_n = isinstance(n, Tensor)
    rg = None if tensor_n else _regroup_decode(q, k, mask, bias, dropout_p)   # (per-row n in the regrouped problem: not built)
    if rg is not None:
        q_g, mask_g, bias_g = rg
        out = _FlashAttentionSoftmaxN.apply(q_g, k, v, mask_g, bias_g, n, scale, False, 0.0, None)
        out = out.view(B, H, 1, dpad)
        return out if Ev == dpad else out[..., :Ev]
    if not (torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad or (bias is not None and bias.requires_grad)
                                         or (tensor_n and n.requires_grad))):
        out = _launch_fwd(q, k, v, mask, bias, n, scale, bool(is_causal), dropout_p, rng)[0]   # nothing to differentiate: no autograd node
    else:
        out = _FlashAttentionSoftmaxN.apply(q, k, v, mask, bias, n, scale, bool(is_causal), dropout_p, rng, bias_small)
    return out if Ev == dpad else out[..., :Ev]


def kernel_path(query: Tensor, key: Tensor, value: Tensor, attn_mask: Optional[Tensor] = None, attn_bias: Optional[Tensor] = None,
                is_causal: bool = False, dropout_p: float = 0.0, scale: Optional[float] = None, softmax_n_param=None) -> str:
    """Name of the kernel family a flash_attention_n call with these arguments is routed to (fasn_fwd_path): "plain", "key-padding",
    "vector mask/bias", "vector bias + key-padding", "element-load (slow)" or "fp32". Launches no attention kernel and leaves the
    per-thread plan cache alone: it runs the argument normalisation of the real call (which may issue its small device ops - a feature
    pad, the copy of a misaligned operand, a bias cast) and asks fasn_fwd_path about a throw-away argument block built from the
    canonical tensors, including the regrouping of a grouped-query decode call. fasn_fwd_path looks at layouts and modes only. A tensor
    softmax_n_param (per batch element / head) takes the same kernels, and keeps a grouped-query decode call on the per-head launch."""
    tensor_n = isinstance(softmax_n_param, Tensor)
    if tensor_n:
        _n_tensor(softmax_n_param, query)   # (validation only)
    q, k, v, mask, bias, n, sc, dp, _, _, bias_small = _prepare(query, key, value, 1.0, scale, dropout_p, attn_mask, attn_bias)
    if bias_small:
        bias = bias.expand(q.shape[0], q.shape[1], q.shape[2], k.shape[2])
    causal = bool(is_causal)
    rg = None if tensor_n else _regroup_decode(q, k, mask, bias, dp)
    if rg is not None:
        (q, mask, bias), causal = rg, False
    a = FwdArgs()
    _fill_fwd(a, q, k, v, q, q, mask, bias, n, sc, causal, dp)   # (o / lse: any device pointer, the query stands in - nothing is launched)
    with torch.cuda.device(q.device):
        return _lib.FASN_PATH_NAMES[_lib.load().fasn_fwd_path(a)]


def last_rng_state():
    """What the calling thread's most recent flash_attention_n call used as its dropout state: None (no dropout), a (seed, offset)
    tuple (eager calls: passed by value) or the device tensor {seed, offset} a HIP-graph capture reads at every replay."""
    return getattr(_TLS, "last_rng_state", None)


def last_dropout_state():
    """(seed, offset) of the most recent dropout call as Python ints (one device read), for dropout.keep_mask; None if that call
    had dropout_p == 0. Test / reproduction helper."""
    t = getattr(_TLS, "last_rng_state", None)
    if t is None:
        return None
    if isinstance(t, tuple):
        return t
    s, o = (int(x) for x in t.cpu().tolist())
    return s & 0xFFFFFFFFFFFFFFFF, o & 0xFFFFFFFFFFFFFFFF


def flash_attention_n(
        query: Tensor,
        key: Tensor,
        value: Tensor,
        softmax_n_param: Optional[float] = None,
        scale: Optional[float] = None,
        dropout_p: float = 0.,
        attn_mask: Optional[Tensor] = None,
        attn_bias: Optional[Tensor] = None,
        is_causal: bool = False
) -> Tensor:
    """Fused attention with softmax_n on MI355X; drop-in for flash_attention_softmax_n.flash_attention_n.

    :param query: [B, H, L, E] fp16 / bf16 device tensor, E <= 256 (fp32 also accepted: exact-fp32 kernels, ~1/16 of the bf16
                  rate, E <= 128).
    :param key: [B, H, S, E] (or [B, S, E], shared by all heads).
    :param value: [B, H, S, Ev].
    :param softmax_n_param: n >= 0; real values allowed (the reference's SDPA path takes integers only). Or a floating tensor on the
                            query's device that broadcasts to [B, H] ([H], [1, H], [B, 1], [B, H] or 0-d; H = query heads, also under
                            grouped K/V): one n per batch element and head (learned attention sinks: n_h = exp(s_h)), read as fp32 and
                            differentiated (dL/dn = -sum_i delta_i exp(-lse_i), summed over the dimensions n broadcasts over) when it
                            requires grad. Its values are not checked (no host synchronisation; capturable): an entry that is not > 0
                            (negative, NaN) acts as n = 0. A tensor filled with c gives the results of the float c bit for bit.
    :param scale: multiplies q.k^T; default 1/sqrt(E).
    :param dropout_p: attention-weight dropout, realised in 1/65536 steps (dropout.effective_p); the mask is a pure function of
                      the call's (seed, offset) - drawn from a per-device stream seeded by torch's CUDA generator, advanced on the
                      device so that HIP-graph replays resample - and regenerated in backward.
    :param attn_mask: bool, 4-D, broadcastable to [B, H, L, S]; True = attend.
    :param attn_bias: additive bias [H, L, S] or broadcastable to [B, H, L, S] (e.g. ALiBi). Differentiated like the reference's
                      additive mask (core/flash_attn.py:100-113): a bias that requires grad gets dS summed over the dimensions it
                      broadcasts - inside the kernel for batch / head broadcasts ([H,L,S], [B,1,L,S], ...: no [B,H,L,S] buffer).
    :param is_causal: bottom-right aligned causal mask (key j visible to row i iff j <= i + S - L).
    :return: [B, H, L, Ev] in query's dtype.
    Rows with no visible key and n == 0 return 0 (the reference returns NaN there).
    """
    return _attention(query, key, value, softmax_n_param, scale, dropout_p, attn_mask, attn_bias, is_causal)


def flash_attention_n_triton(query: Tensor, key: Tensor, value: Tensor, is_causal: bool = False,
                             scale: Optional[float] = None, softmax_n_param: Optional[float] = None) -> Tensor:
    """Signature of flash_attn_triton.py:339-345; served by the same HIP kernel (bf16 too, any L/S)."""
    return _attention(query, key, value, softmax_n_param, scale, 0.0, None, None, is_causal)


def slow_attention_n(query: Tensor, key: Tensor, value: Tensor, attn_mask: Optional[Tensor] = None, dropout_p: float = 0.0,
                     is_causal: bool = False, scale: Optional[float] = None, softmax_n_param: Optional[float] = None,
                     softmax_dtype=None, train: bool = True) -> Tensor:
    """Signature of functional.py:32-42 on the fused kernel. Accepts (N, ..., L, E) with 3-D or 4-D inputs.
    Float masks are additive (broadcast over leading dims), boolean masks hide keys (the reference's
    eager version silently ignores boolean masks, functional.py:85-86).
    softmax_dtype: the reference casts the softmax_n weights to it (default: query's dtype, functional.py:72-73,91) and multiplies them
    with `value` next (:93) - so the only values that do not raise there are None and value's own dtype, and for those the weights reach
    the P.V contraction rounded to value's dtype. That is what the kernel does as well (P is packed to the operand dtype for the MFMA; the
    scores, the running max and the row sum stay in fp32 registers, where the reference keeps them in query's dtype). Any other
    softmax_dtype raises the RuntimeError torch's matmul raises in the reference."""
    if is_causal and attn_mask is not None:
        raise AssertionError("attn_mask and is_causal are mutually exclusive")  # functional.py:79
    if softmax_dtype is not None and softmax_dtype != value.dtype:
        raise RuntimeError(f"expected m1 and m2 to have the same dtype, but got: {softmax_dtype} != {value.dtype} "
                           "(softmax_dtype must be None or value's dtype: the weights are multiplied with value next, functional.py:91-93)")
    squeeze = query.dim() == 3
    if squeeze:
        query, key, value = query.unsqueeze(1), key.unsqueeze(1), value.unsqueeze(1)
    mask = bias = None
    if attn_mask is not None:
        am = attn_mask
        while am.dim() < 4:
            am = am.unsqueeze(0)
        if am.dtype == torch.bool:
            mask = am
        else:
            bias = am
    p = dropout_p if train else 0.0
    out = _attention(query, key, value, softmax_n_param, scale, p, mask, bias, is_causal)
    return out.squeeze(1) if squeeze else out


# ---- packed variable-length training attention (include/fasn.h: fasn_fwd_varlen / fasn_bwd_varlen) -----------------
_VARLEN_D = (64,)   # the head dims fasn_fwd_varlen serves in this build (any other: FASN_EUNSUPPORTED)
_VARLEN_LOG2E = 1.4426950408889634
_VARLEN_F16_MAX_PRESCALE = 8.0   # float16: |scale * log2e| beyond this is FASN_EUNSUPPORTED (build_varlen, csrc/fasn_attnvarlen.hip)


def _view_packed(t: Tensor) -> View4:
    """a packed [T, heads, E] operand as the [1, heads, T, E] view of the C ABI: stride[1] between heads, stride[2] between tokens"""
    v = View4()
    v.ptr = t.data_ptr()
    v.stride[0], v.stride[1], v.stride[2], v.stride[3] = 0, t.stride(1), t.stride(0), 1
    return v


def _packed_ok(t: Tensor) -> bool:
    return t.stride(2) == 1 and t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0


def _varlen_block(cu_q, cu_k, max_q, max_k):
    vl = _lib.Varlen()
    vl.cu_seqlens_q, vl.cu_seqlens_k = cu_q.data_ptr(), cu_k.data_ptr()
    vl.num_seqs, vl.max_seqlen_q, vl.max_seqlen_k, vl.reserved = cu_q.numel() - 1, max_q, max_k, 0
    return vl


def _fill_fwd_varlen(a: FwdArgs, q, k, v, o, lse, n, scale, causal):
    a.q, a.k, a.v, a.o = _view_packed(q), _view_packed(k), _view_packed(v), _view_packed(o)
    a.lse = lse.data_ptr()
    a.mask.ptr = a.bias.ptr = None
    a.bias_dtype = _lib.FASN_BIAS_NONE
    a.dtype = _DTYPES[q.dtype]
    a.B, a.H, a.Sq, a.Sk, a.D, a.Dv = 1, q.shape[1], q.shape[0], k.shape[0], q.shape[2], v.shape[2]
    a.kv_group = q.shape[1] // k.shape[1] if k.shape[1] != q.shape[1] else 0
    a.scale, a.softmax_n, a.causal, a.dropout_p = scale, n, 1 if causal else 0, 0.0
    a.seed = a.offset = 0
    a.rng_state = None


def _window_block(window):
    w = _lib.KvWindow()
    w.window, w.reserved = min(window, 2 ** 31 - 1), 0
    return w


def _launch_fwd_varlen(q, k, v, cu_q, cu_k, max_q, max_k, n, scale, causal, window=None):
    """out [Tq, H, E] and lse [H, Tq]: every row is written by the call (rows at or beyond cu_q[B]: 0 / -inf, by its tail kernel).
    window: None - fasn_fwd_varlen - or the sliding window of fasn_fwd_varlen_window"""
    lib = _lib.load()
    dev = q.device
    o = torch.empty((q.shape[0], q.shape[1], q.shape[2]), dtype=q.dtype, device=dev)
    lse = torch.empty((q.shape[1], q.shape[0]), dtype=torch.float32, device=dev)
    a = FwdArgs()
    tensor_n = isinstance(n, Tensor)
    _fill_fwd_varlen(a, q, k, v, o, lse, 0.0 if tensor_n else n, scale, causal)
    vl = _varlen_block(cu_q, cu_k, max_q, max_k)
    n_ptr, n_stride = (n.data_ptr(), n.stride(1) if n.shape[1] > 1 else 0) if tensor_n else (None, 0)
    with torch.cuda.device(dev):
        if window is None:
            rc = lib.fasn_fwd_varlen(a, vl, n_ptr, n_stride, _stream_ptr(dev))
        else:
            rc = lib.fasn_fwd_varlen_window(a, vl, _window_block(window), n_ptr, n_stride, _stream_ptr(dev))
    if rc:
        _lib.check(rc, "fasn_fwd_varlen" if window is None else "fasn_fwd_varlen_window")
    return o, lse


class _FlashAttentionSoftmaxNVarlen(torch.autograd.Function):
    """autograd glue of flash_attention_n_varlen, beside _FlashAttentionSoftmaxN: dq / dk / dv through fasn_bwd_varlen (under a window:
    fasn_bwd_varlen_window), the gradient of a tensor n through fasn_bwd_dn on the [1, H, Tq] view of out, lse and dout (rows behind the
    last sequence are 0 / -inf: no term; lse carries the window, so the kernel is the same)."""

    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, max_q: int, max_k: int, n, scale: float, causal: bool, window=None):
        o, lse = _launch_fwd_varlen(q, k, v, cu_q, cu_k, max_q, max_k, n, scale, causal, window)
        ctx.save_for_backward(q, k, v, o, lse, cu_q, cu_k)
        ctx.n_shape = tuple(n.shape) if isinstance(n, Tensor) else None
        ctx.n = 0.0 if isinstance(n, Tensor) else n
        ctx.max_q, ctx.max_k, ctx.scale, ctx.causal, ctx.window = max_q, max_k, scale, causal, window
        ctx.mark_non_differentiable(lse)
        return o, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        q, k, v, o, lse, cu_q, cu_k = ctx.saved_tensors
        dq, dk, dv, dn = _bwd_varlen(ctx, q, k, v, o, lse, cu_q, cu_k, dout)
        return dq, dk, dv, None, None, None, None, dn, None, None, None


def _bwd_varlen(ctx, q, k, v, o, lse, cu_q, cu_k, dout):
    """(dq, dk, dv, dn) of the packed call on the saved operands; ctx: the node's constants (n at input 7). Freshly allocated, contiguous."""
    lib = _lib.load()
    dev = q.device
    if not _packed_ok(dout):
        dout = dout.contiguous()
        if dout.data_ptr() % 16:
            dout = dout.clone()
    dq = torch.empty(q.shape, dtype=q.dtype, device=dev)
    dk = torch.empty(k.shape, dtype=q.dtype, device=dev)
    dv = torch.empty(v.shape, dtype=q.dtype, device=dev)
    delta = torch.empty(lse.shape, dtype=torch.float32, device=dev)
    a = BwdArgs()
    _fill_fwd_varlen(a.fwd, q, k, v, o, lse, ctx.n, ctx.scale, ctx.causal)
    a.dout, a.dq, a.dk, a.dv = _view_packed(dout), _view_packed(dq), _view_packed(dk), _view_packed(dv)
    a.delta = delta.data_ptr()
    a.workspace, a.workspace_bytes, a.flags, a.dbias_dtype = None, 0, 0, 0
    a.dbias.ptr = None
    vl = _varlen_block(cu_q, cu_k, ctx.max_q, ctx.max_k)
    dn = None
    with torch.cuda.device(dev):
        if ctx.window is None:
            rc = lib.fasn_bwd_varlen(a, vl, _stream_ptr(dev))
        else:
            rc = lib.fasn_bwd_varlen_window(a, vl, _window_block(ctx.window), _stream_ptr(dev))
        if rc:
            _lib.check(rc, "fasn_bwd_varlen" if ctx.window is None else "fasn_bwd_varlen_window")
        if ctx.n_shape is not None and ctx.needs_input_grad[7]:
            # dL/dn_h = -sum_t delta_t exp(-lse_t): the rectangular call's kernel on B = 1, Sq = Tq (views [1, H, Tq, E] as filled above)
            dn = torch.empty(ctx.n_shape, dtype=torch.float32, device=dev)
            a.fwd.softmax_n = 0.0
            ws_bytes = lib.fasn_bwd_dn_workspace_bytes(a)
            ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
            _lib.check(lib.fasn_bwd_dn(a, dn.data_ptr(), 0, dn.stride(1) if dn.shape[1] > 1 else 0, ws.data_ptr(), ws_bytes, _stream_ptr(dev)),
                       "fasn_bwd_dn")
    return dq, dk, dv, dn


def _n_tensor_varlen(n: Tensor, query: Tensor) -> Tensor:
    """softmax_n as a tensor for the packed call: one n per query head ([H], [1, H] or 0-d), read as the fp32 [1, 1 or H] view"""
    H = query.shape[1]
    if not n.is_floating_point():
        raise TypeError(f"softmax_n_param as a tensor must be floating point; got {n.dtype}")
    if n.device != query.device:
        raise ValueError(f"softmax_n_param is on {n.device}, query on {query.device}: pass n on the query's device")
    shape = tuple(n.shape)
    if not (n.dim() == 0 or (n.dim() == 1 and shape[0] in (1, H)) or (n.dim() == 2 and shape[0] == 1 and shape[1] in (1, H))):
        raise ValueError(f"softmax_n_param must broadcast to [H] = [{H}] (0-d, [H] or [1, H]); got {shape}: a per-sequence n is not built "
                         "(the kernels read one n per head)")
    return n.float().reshape((1,) * (2 - n.dim()) + shape)


def flash_attention_n_varlen(query: Tensor, key: Tensor, value: Tensor, cu_seqlens_q: Tensor, max_seqlen_q: int,
                             cu_seqlens_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, softmax_n_param=1, scale: Optional[float] = None,
                             is_causal: bool = False, return_lse: bool = False, window: Optional[int] = None):
    """flash_attention_n on packed variable-length sequences, forward and backward (flash_attn_varlen_func for softmax_n): sequence b is
    flash_attention_n on query[cu_q[b]:cu_q[b+1]] against key, value[cu_k[b]:cu_k[b+1]]; nothing is padded and nothing is read on the host.

    :param query: [Tq, H, E] fp16 / bf16 device tensor; E = 64 in this build. Any token and head strides with unit feature stride and 16-byte
                  aligned rows (slices of one packed [T, H + 2 Hkv, E] buffer go in without a copy; anything else is copied).
    :param key, value: [Tk, Hkv, E], H % Hkv == 0 (grouped-query attention).
    :param cu_seqlens_q, cu_seqlens_k: int32 [B + 1] on the query's device: cu[0] = 0, non-decreasing, cu[B] <= T. cu_seqlens_k = None: the same
                  tensor as cu_seqlens_q (self-attention). Sequences of length 0 on either side are legal.
    :param max_seqlen_q, max_seqlen_k: Python ints that bound every length (the grid's size); max_seqlen_k = None: max_seqlen_q. Rows of a longer
                  sequence beyond the bound are not computed (the caller's error; no access leaves the operands).
    :param softmax_n_param: a float >= 0, or a floating tensor on the query's device that broadcasts to [H] (0-d, [H], [1, H]), differentiated
                  when it requires grad. A tensor filled with c gives the float c's results bit for bit. A per-sequence n is refused.
    :param scale: the logits are scale * q . k; default 1 / sqrt(E). A negative scale negates the query. float16 serves |scale| * log2(e) <= 8
                  (NotImplementedError beyond it).
    :param is_causal: bottom-right aligned per sequence: key j visible to row i iff j <= i + (sk_b - sq_b).
    :param window: None, or a Python int >= 1 - a sliding window, the constant of a layer (Hugging Face's sliding_window; with is_causal only):
                  row i of sequence b sits at p_i = i + (sk_b - sq_b) and sees key j iff p_i - window < j <= p_i and 0 <= j < sk_b - its own
                  position counts, `window` keys. A workgroup walks only the window's tiles; a window >= max_seqlen_k is the causal call,
                  bit for bit. Part of a captured graph.
    :return: out [Tq, H, E]; with return_lse also lse, fp32 [H, Tq]. Rows at or beyond cu_q[B] are 0 with lse -inf, their dq rows and the
             dk / dv rows at or beyond cu_k[B] exactly 0. A row that sees no key is 0 with lse log n (-inf at n = 0), its gradients 0.
    Capturable: one captured graph serves any contents of the cu_seqlens tensors with the same B, T and max_seqlen.
    There is no attn_mask, attn_bias or dropout_p on packed operands."""
    q, k, v, cu_q, cu_k, max_q, max_k, n, scale = _prepare_varlen(query, key, value, cu_seqlens_q, max_seqlen_q, cu_seqlens_k, max_seqlen_k,
                                                                  softmax_n_param, scale, is_causal, window)
    needs_grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad or (isinstance(n, Tensor) and n.requires_grad))
    if needs_grad:
        out, lse = _FlashAttentionSoftmaxNVarlen.apply(q, k, v, cu_q, cu_k, max_q, max_k, n, scale, bool(is_causal), window)
    else:   # nothing to differentiate: no autograd node
        out, lse = _launch_fwd_varlen(q, k, v, cu_q, cu_k, max_q, max_k, n, scale, bool(is_causal), window)
    return (out, lse) if return_lse else out


def _prepare_varlen(query, key, value, cu_seqlens_q, max_seqlen_q, cu_seqlens_k, max_seqlen_k, softmax_n_param, scale, is_causal, window):
    """every refusal of flash_attention_n_varlen, in its order and under its name (flash_attention_n_varlen_rope refuses the same calls with
    the same words), then the operands as the launches take them: (q, k, v, cu_q, cu_k, max_q, max_k, n, scale)"""
    if window is not None:   # (a constant of the layer: refused before anything is read from the operands)
        if isinstance(window, bool) or not isinstance(window, int):
            raise TypeError(f"window must be None or a Python int >= 1; got {type(window).__name__}")
        if window < 1:
            raise ValueError(f"window must be >= 1 (a row's own position counts); got {window}")
        if not is_causal:
            raise ValueError("window needs is_causal=True: the window is causal and bottom-right aligned (row i at position i + sk_b - sq_b "
                             "sees the `window` keys that end at its own position); there is no two-sided window")
    if not isinstance(query, Tensor) or not query.is_cuda:
        raise RuntimeError("flash_attention_n_varlen runs on MI355X device tensors only; got a CPU tensor (there is deliberately no CPU fallback)")
    if query.dtype not in (torch.float16, torch.bfloat16):
        raise NotImplementedError(f"flash_attention_n_varlen: dtype {query.dtype} is not served; packed operands are torch.float16 or torch.bfloat16")
    if key.dtype != query.dtype or value.dtype != query.dtype:
        raise TypeError("query, key and value must share one dtype")
    if query.dim() != 3 or key.dim() != 3 or value.dim() != 3:
        raise ValueError("packed operands: query must be [Tq, H, E], key and value [Tk, Hkv, E]")
    if key.device != query.device or value.device != query.device:
        raise ValueError("query, key and value must be on one device")
    Tq, H, E = query.shape
    Tk, Hkv, Ek = key.shape
    if Ek != E or value.shape[0] != Tk or value.shape[1] != Hkv:
        raise ValueError("key must be [Tk, Hkv, E] and value [Tk, Hkv, Ev]")
    if value.shape[2] != E:
        raise NotImplementedError(f"flash_attention_n_varlen: E != Ev ({E} != {value.shape[2]}) is not served on packed operands")
    if E not in _VARLEN_D:
        raise NotImplementedError(f"flash_attention_n_varlen: head dim {E} is not served on packed operands; head dims served: {list(_VARLEN_D)} "
                                  "(no feature padding here)")
    if Hkv < 1 or H % Hkv != 0:
        raise ValueError(f"key / value have {Hkv} heads: must divide the {H} query heads (grouped-query attention)")
    if Tq < 1 or Tk < 1:
        raise ValueError("packed operands must hold at least one token row per side")
    cu_k = cu_seqlens_q if cu_seqlens_k is None else cu_seqlens_k
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_k)):
        if not isinstance(cu, Tensor) or cu.dtype != torch.int32:
            raise TypeError(f"{name} must be an int32 tensor [B + 1]; got {getattr(cu, 'dtype', type(cu))}")
        if cu.device != query.device:
            raise ValueError(f"{name} is on {cu.device}, query on {query.device}: the offsets are read on the device")
        if cu.dim() != 1 or cu.numel() < 2 or not cu.is_contiguous():
            raise ValueError(f"{name} must be a contiguous [B + 1] tensor with B >= 1")
    if cu_k.numel() != cu_seqlens_q.numel():
        raise ValueError("cu_seqlens_q and cu_seqlens_k must describe the same number of sequences")
    max_q = int(max_seqlen_q)
    max_k = max_q if max_seqlen_k is None else int(max_seqlen_k)
    if max_q < 1 or max_k < 1:
        raise ValueError("max_seqlen_q and max_seqlen_k must be >= 1")
    if isinstance(softmax_n_param, Tensor):
        n = _n_tensor_varlen(softmax_n_param, query)
    else:
        n = 0.0 if softmax_n_param is None else float(softmax_n_param)
        if n < 0:
            raise ValueError("softmax_n_param must be >= 0")
    scale = (1.0 / sqrt(E)) if scale is None else float(scale)
    if scale < 0:
        query, scale = -query, -scale
    # (in fp32, as build_varlen forms it: a scale within a rounding of the limit gets the same answer here and there)
    if query.dtype == torch.float16 and float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(_VARLEN_LOG2E, dtype=torch.float32)) > _VARLEN_F16_MAX_PRESCALE:
        raise NotImplementedError(f"flash_attention_n_varlen: float16 with |scale| = {scale:g} is not served on packed operands: the kernels round "
                                  f"query * scale * log2(e) to float16 and serve |scale| * log2(e) <= {_VARLEN_F16_MAX_PRESCALE:g}, that is |scale| <= "
                                  f"{_VARLEN_F16_MAX_PRESCALE / _VARLEN_LOG2E:.4f}; use bfloat16 or fold the scale into the query")
    q, k, v = (t if _packed_ok(t) else t.contiguous() for t in (query, key, value))
    q, k, v = (t.clone() if t.data_ptr() % 16 else t for t in (q, k, v))
    return q, k, v, cu_seqlens_q, cu_k, max_q, max_k, n, scale


# ---- rotary position embedding on the packed call (include/fasn.h: fasn_varlen_rope) ---------------------------------
def _launch_varlen_rope(q, k, q_out, k_out, cu_q, cu_k, max_q, max_k, rope, inverse):
    """the one rotary launch over packed q [Tq, H, E] and k [Tk, Hkv, E] into q_out / k_out (None: allocated here; rows at or beyond
    cu[B] of a side are not written - no launch reads them). inverse: the transpose rotation. Returns (q_out, k_out)."""
    lib = _lib.load()
    dev = q.device
    if q_out is None:
        q_out = torch.empty(q.shape, dtype=q.dtype, device=dev)
    if k_out is None:
        k_out = torch.empty(k.shape, dtype=k.dtype, device=dev)
    a = FwdArgs()
    a.q, a.k = _view_packed(q), _view_packed(k)
    a.v.ptr = a.o.ptr = a.lse = None   # (not touched by this launch)
    a.mask.ptr = a.bias.ptr = None
    a.bias_dtype = _lib.FASN_BIAS_NONE
    a.dtype = _DTYPES[q.dtype]
    a.B, a.H, a.Sq, a.Sk, a.D, a.Dv = 1, q.shape[1], q.shape[0], k.shape[0], q.shape[2], q.shape[2]
    a.kv_group = q.shape[1] // k.shape[1] if k.shape[1] != q.shape[1] else 0
    a.scale, a.softmax_n, a.causal, a.dropout_p = 1.0, 0.0, 0, 0.0
    a.seed = a.offset = 0
    a.rng_state = None
    vl = _varlen_block(cu_q, cu_k, max_q, max_k)
    with torch.cuda.device(dev):
        rc = lib.fasn_varlen_rope(a, vl, rope, _view_packed(q_out), _view_packed(k_out), 1 if inverse else 0, _stream_ptr(dev))
    if rc:
        _lib.check(rc, "fasn_varlen_rope")
    return q_out, k_out


class _FlashAttentionSoftmaxNVarlenRope(torch.autograd.Function):
    """autograd glue of flash_attention_n_varlen_rope: the rotary launch, then _FlashAttentionSoftmaxNVarlen's forward on the rotated q / k,
    which are what is saved; the backward is that class's on the saved operands, then the transpose rotation of dq / dk in place."""

    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, max_q: int, max_k: int, n, scale: float, causal: bool, window, cos, sin, interleaved: bool):
        from .kvcache import _rope_operand
        qr, kr = _launch_varlen_rope(q, k, None, None, cu_q, cu_k, max_q, max_k, _rope_operand(cos, sin, interleaved, q), False)
        o, lse = _launch_fwd_varlen(qr, kr, v, cu_q, cu_k, max_q, max_k, n, scale, causal, window)
        ctx.save_for_backward(qr, kr, v, o, lse, cu_q, cu_k, cos, sin)
        ctx.n_shape = tuple(n.shape) if isinstance(n, Tensor) else None
        ctx.n = 0.0 if isinstance(n, Tensor) else n
        ctx.max_q, ctx.max_k, ctx.scale, ctx.causal, ctx.window, ctx.interleaved = max_q, max_k, scale, causal, window, interleaved
        ctx.mark_non_differentiable(lse)
        return o, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        from .kvcache import _rope_operand
        qr, kr, v, o, lse, cu_q, cu_k, cos, sin = ctx.saved_tensors
        dq, dk, dv, dn = _bwd_varlen(ctx, qr, kr, v, o, lse, cu_q, cu_k, dout)
        _launch_varlen_rope(dq, dk, dq, dk, cu_q, cu_k, ctx.max_q, ctx.max_k, _rope_operand(cos, sin, ctx.interleaved, qr), True)
        return dq, dk, dv, None, None, None, None, dn, None, None, None, None, None, None


def flash_attention_n_varlen_rope(query: Tensor, key: Tensor, value: Tensor, cu_seqlens_q: Tensor, max_seqlen_q: int, rotary_cos: Tensor,
                                  rotary_sin: Tensor, cu_seqlens_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None,
                                  softmax_n_param=1, scale: Optional[float] = None, is_causal: bool = False, return_lse: bool = False,
                                  window: Optional[int] = None, rotary_interleaved: bool = False):
    """flash_attention_n_varlen with rotary position embedding (RoPE) at per-sequence positions, forward and backward: ONE launch rotates the
    packed query and key rows - positions from the offset tables in device memory, nothing read on the host -, then the packed call runs on
    the rotated operands (flash-attn's apply_rotary_emb(..., cu_seqlens=, max_seqlen=) in front of flash_attn_varlen_func).

    Positions: key token cu_k[b] + j sits at j, query token cu_q[b] + i at p_i = i + (sk_b - sq_b) - the position of the causal mask and of
    `window`; self-attention gives p_i = i, and every sequence restarts at 0. The table row read is clamp(position, 0, rows - 1).

    :param rotary_cos, rotary_sin: [rows, rotary_dim / 2] device tensors, float32 or the query's dtype, unit column stride, 16-byte aligned
                  rows; 16 <= rotary_dim <= E, rotary_dim % 16 == 0 (features beyond rotary_dim pass through); rows >= max_seqlen_k
                  (max_seqlen_q when cu_seqlens_k is None). Scaling rules (YaRN, NTK) live in the tables. A table that requires grad is
                  refused: there is no table gradient.
    :param rotary_interleaved: False: the half-split layout (GPT-NeoX / Llama / GPT-OSS, rotate_half) - the pair of feature d is
                  (d, d + rotary_dim / 2); True: GPT-J pairs (2 d, 2 d + 1).
    Every other parameter, the result and every refusal are flash_attention_n_varlen's (the refusals come first, with its messages).

    out, lse and the gradient of a tensor n are, bit for bit, flash_attention_n_varlen on rot(query), rot(key), value, with rot evaluated in
    fp32 - every product and the sum / difference rounded on its own - and rounded once to the operand type; query.grad and key.grad are,
    bit for bit, eager autograd's for that rot in front of the call: the transpose rotation of the rotated operands' gradients in fp32,
    rounded once. The rotated query and key are allocated once and are what the backward keeps; the unrotated ones are not kept here.
    Capturable as flash_attention_n_varlen is."""
    q, k, v, cu_q, cu_k, max_q, max_k, n, scale = _prepare_varlen(query, key, value, cu_seqlens_q, max_seqlen_q, cu_seqlens_k, max_seqlen_k,
                                                                  softmax_n_param, scale, is_causal, window)
    fn = "flash_attention_n_varlen_rope"
    from .kvcache import _check_rotary_tables, _rope_operand
    if not isinstance(rotary_interleaved, bool):
        raise TypeError(f"{fn}: rotary_interleaved must be a bool; got {type(rotary_interleaved).__name__}")
    _check_rotary_tables(fn, rotary_cos, rotary_sin, q)
    E = q.shape[2]
    rows, rd = rotary_cos.shape[0], 2 * rotary_cos.shape[1]
    esize = rotary_cos.element_size()
    for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
        if t.device != q.device:
            raise RuntimeError(f"{name} is on {t.device}, query on {q.device}: every operand must live on the query's device "
                               "(the tables are read by the kernels, never on the host)")
    if rd < 16 or rd > E or rd % 16 != 0:
        raise ValueError(f"{fn}: rotary_dim = 2 x {rotary_cos.shape[1]} = {rd} is not supported: 16 <= rotary_dim <= head dim {E} and "
                         "rotary_dim % 16 == 0 (a lane rotates 8 pairs)")
    if rows < max_k:
        raise ValueError(f"{fn}: the rotary tables cover {rows} positions but max_seqlen_k is {max_k}: rows >= max_seqlen_k, so that "
                         "no position the offsets in device memory can name lies outside the tables")
    for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
        if t.stride(1) != 1 or t.data_ptr() % 16 != 0 or (rows > 1 and ((t.stride(0) * esize) % 16 != 0 or t.stride(0) < rd // 2)):
            raise ValueError(f"{fn}: {name}: rows must be 16-byte aligned, apart and with unit column stride (base pointer % 16 == 0, row "
                             f"stride x {esize} bytes % 16 == 0, row stride >= rotary_dim / 2 = {rd // 2}); got strides {tuple(t.stride())}. "
                             "A table is never copied here")
        if t.requires_grad:
            raise ValueError(f"{fn}: {name} requires grad: there is no gradient with respect to the rotary tables; pass it detached")
    needs_grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad or (isinstance(n, Tensor) and n.requires_grad))
    if needs_grad:
        out, lse = _FlashAttentionSoftmaxNVarlenRope.apply(q, k, v, cu_q, cu_k, max_q, max_k, n, scale, bool(is_causal), window, rotary_cos,
                                                           rotary_sin, rotary_interleaved)
    else:   # nothing to differentiate: no autograd node
        qr, kr = _launch_varlen_rope(q, k, None, None, cu_q, cu_k, max_q, max_k, _rope_operand(rotary_cos, rotary_sin, rotary_interleaved, q), False)
        out, lse = _launch_fwd_varlen(qr, kr, v, cu_q, cu_k, max_q, max_k, n, scale, bool(is_causal), window)
    return (out, lse) if return_lse else out
