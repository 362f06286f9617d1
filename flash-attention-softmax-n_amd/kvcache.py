"""Attention over a K/V cache (inference): paged or dense cache, lengths in device memory, grouped-query heads as rows of one problem.

Host side of fasn_fwd_kvcache / fasn_kvcache_append (decode: flash_attention_n_kvcache, up to 128 rows per K/V head) and of
fasn_fwd_kvprefill / fasn_kvprefill_append (prefill: flash_attention_n_kvcache_prefill, any number of positions, optional per-batch
query lengths on the device) in include/fasn.h. Nothing about the lengths or the block table is read on the host - no `.item()`, no
synchronisation, the launches depend on shapes and capacity only - so a call can be captured once in a torch.cuda.graph and replayed
while `cache_seqlens`, `query_seqlens`, `block_table`, the cache and `query` change in place. Prompt -> chunked prefill -> decode runs on
the paged cache alone. `alibi_slopes` on both calls adds -slope[b, h] * |p_i - j| to the logits inside the kernels (fasn_fwd_kvcache_alibi /
fasn_fwd_kvprefill_alibi): p_i comes from the lengths in device memory, so no bias tensor exists and the graph stays one graph.
flash_attention_n_kvcache_window is a sliding-window layer on the same cache (fasn_fwd_kvcache_window / fasn_fwd_kvprefill_window): the
window is a host integer, the kernels walk the window's tiles only and never touch the pages below it.
flash_attention_n_kvcache_rope rotates `query` and `k_new` by their absolute positions (RoPE) inside the append launch
(fasn_kvcache_rope_append / fasn_kvprefill_rope_append): the positions come from the lengths in device memory, so the step stays one graph.
flash_attention_n_kvcache_varlen is the prefill call on TOKEN-PACKED queries (fasn_fwd_kvvarlen / fasn_kvvarlen_append): one [T, H, D]
buffer and `cu_seqlens_q` on the device - a continuous-batching step of prompt chunks and decode tokens whose grid follows the tokens.
flash_attention_n_kvcache_varlen_window and flash_attention_n_kvcache_varlen_rope are the sliding-window and the rotary call on the same
packed buffers (fasn_fwd_kvvarlen_window / fasn_kvvarlen_rope_append): a served GPT-OSS or Mistral layer in one token-packed step.
flash_attention_n_kvcache_tree verifies a TREE of draft tokens in one step (speculative decoding: fasn_fwd_kvcache_tree / fasn_fwd_kvprefill_tree,
fasn_kv*_tree_rope_append): one int64 word per node on the device says which nodes it sees, its position is the prefix length plus its
depth; flash_attention_n_kvcache_tree_commit moves the accepted path's cache rows behind the prefix (fasn_kvcache_tree_commit).
flash_attention_n_kvcache_fp8 is the decode / prefill call over a cache of e4m3fn codes with per-(batch, K/V head) fp32 scales on the device
(fasn_fwd_kvcache_fp8 / fasn_fwd_kvprefill_fp8, fasn_kv*_fp8_append): half the cache bytes per key, k_new / v_new quantised on the way in.
flash_attention_n_kvcache_fp8_window is the sliding-window layer on that cache (fasn_fwd_kv*_fp8_window) and flash_attention_n_kvcache_fp8_rope
the rotary call (fasn_kv*_fp8_rope_append: rotate, round to the 16-bit type, quantise, append - one launch), with or without a window.
flash_attention_n_kvcache_fp8_tree verifies a tree of draft tokens on that cache (fasn_fwd_kv*_fp8_tree, fasn_kv*_fp8_tree_rope_append) and
flash_attention_n_kvcache_fp8_tree_commit moves the accepted path's code rows behind the prefix (fasn_kvcache_fp8_tree_commit).
flash_attention_n_kvcache_fp8_varlen, _fp8_varlen_window and _fp8_varlen_rope are the token-packed calls over that cache: the packed FP8
operand sets have no named entry points and go through the operand-set calls (fasn_kv_forward, fasn_kv_append: a fasn_kv_call).
flash_attention_n_kvcache_shared_prefix is the decode call for a batch behind ONE shared prefix (fasn_fwd_shared_prefix): `prefix_table` names
the prefix pages and `prefix_len` - on the device - how many keys they hold; the prefix is attended to once per K/V head for all sequences.
flash_attention_n_kvcache_prefix_groups is that call behind SEVERAL prefixes at once (fasn_fwd_prefix_groups): `prefix_group[b]` - on the
device - names the prefix of batch element b or none, so one call and one captured graph serve every mix of prompts in a batch.
Forward only: the training entry point is flash_attention_n.
"""
from math import sqrt
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import AlibiSlopes, KvCacheArgs, KvFp8, KvPrefillArgs, KvRope, KvTree, KvTreeCommit, KvVarlenArgs, KvWindow, PrefixGroups, SharedPrefix
from .flash_attn import _current_device, _n_strides, _n_tensor, _stream_ptr, _view4

_KV_DTYPES = {torch.float16: _lib.FASN_DTYPE_F16, torch.bfloat16: _lib.FASN_DTYPE_BF16}
_KV_HEAD_DIMS = (32, 64, 128, 256)   # the head dims flash_attention_n trains at; any other size is refused (a cache is never padded)
_FP8_HEAD_DIMS = (64, 128)           # ... and those the FP8-cache kernels are built for
_INT_MAX = 2 ** 31 - 1   # what an int32 member of an argument block holds: host integers are clamped to it
_MAX_ROWS = 128   # query heads per K/V head x query positions: the rows of one workgroup
_MAX_NODES = 64   # nodes of a token tree: one bit of an int64 word each


_BLOCKS = {"kvcache": KvCacheArgs, "kvprefill": KvPrefillArgs, "kvvarlen": KvVarlenArgs}   # entry-point stem -> its argument block


def _check_cache(name: str, t: Tensor, paged: bool, D: int) -> None:
    if t.stride(3) != 1:
        raise ValueError(f"{name}: feature stride must be 1 (got {t.stride(3)}); a cache is never copied, so it cannot be made contiguous here")
    per16 = 16 // t.element_size()   # elements of 16 bytes: 8 in a 16-bit cache, 16 codes in an FP8 cache
    if t.data_ptr() % 16 != 0 or any(t.stride(i) % per16 != 0 for i in range(3) if t.size(i) > 1):
        raise ValueError(f"{name}: rows must be 16-byte aligned (base pointer % 16 == 0, page / row / head strides % {per16} elements); "
                         f"got strides {tuple(t.stride())}")
    if t.size(1) > 1 and t.stride(1) < D:
        raise ValueError(f"{name}: rows overlap (row stride {t.stride(1)} < head dim {D})")


def _slopes_tensor(fn, alibi_slopes, query) -> Tensor:
    """alibi_slopes as the fp32 [1 or B, 1 or H] tensor the kernels read per (batch, query head): _n_tensor's rules under the argument's
    own name. The values are not looked at (no host round trip: capturable)."""
    B, H = query.shape[0], query.shape[1]
    if not isinstance(alibi_slopes, Tensor) or not alibi_slopes.is_floating_point():
        got = alibi_slopes.dtype if isinstance(alibi_slopes, Tensor) else type(alibi_slopes).__name__
        raise TypeError(f"{fn}: alibi_slopes must be a floating-point tensor; got {got}")
    shape = (1,) * (2 - alibi_slopes.dim()) + tuple(alibi_slopes.shape)
    if alibi_slopes.dim() > 2 or shape[0] not in (1, B) or shape[1] not in (1, H):
        raise ValueError(f"{fn}: alibi_slopes must broadcast to [B, H] = [{B}, {H}] ([H], [1, H], [B, 1], [B, H] or 0-d; H = query heads); "
                         f"got {tuple(alibi_slopes.shape)}")
    if alibi_slopes.device != query.device:
        raise RuntimeError(f"alibi_slopes is on {alibi_slopes.device}, query on {query.device}: every operand must live on the query's device "
                           "(the slopes are read by the kernels, never on the host)")
    if torch.is_grad_enabled() and alibi_slopes.requires_grad:
        raise RuntimeError(f"{fn} is forward only (inference): alibi_slopes requires grad and the slopes carry no gradient. Call it under "
                           "torch.no_grad(), or use flash_attention_n with attn_bias, which differentiates the bias")
    return _n_tensor(alibi_slopes.detach(), query).contiguous()


def _check_window(fn, window, or_none="") -> None:
    if isinstance(window, bool) or not isinstance(window, int):
        raise TypeError(f"{fn}: window must be {or_none}a Python int (a constant of the layer, part of a captured graph; never a tensor); "
                        f"got {type(window).__name__}")
    if window < 1:
        raise ValueError(f"{fn}: window must be >= 1 (the keys a position sees, its own included); got {window}")


def _check_query_seqlens(fn, query_seqlens, query) -> None:
    if query_seqlens is None:
        return
    B = query.shape[0] if query.dim() == 4 else -1
    if (not isinstance(query_seqlens, Tensor) or query_seqlens.dtype != torch.int32 or query_seqlens.dim() != 1 or query_seqlens.shape[0] != B
            or not query_seqlens.is_contiguous()):
        got = f"{query_seqlens.dtype} {tuple(query_seqlens.shape)}" if isinstance(query_seqlens, Tensor) else type(query_seqlens).__name__
        raise ValueError(f"query_seqlens must be a contiguous int32 tensor of shape [{B}] on the device; got {got}")
    if query_seqlens.device != query.device:
        raise RuntimeError(f"query_seqlens is on {query_seqlens.device}, query on {query.device}: every operand must live on the query's "
                           "device (the lengths are read by the kernels, never on the host)")


def _check_group_limit(fn, query, k_cache) -> None:
    """the prefill kernels' limit, in front of _prepare (malformed shapes are _prepare's to name)"""
    if query.dim() == 4 and k_cache.dim() == 4 and k_cache.shape[2] >= 1 and query.shape[1] // k_cache.shape[2] > 128 and query.shape[1] % k_cache.shape[2] == 0:
        raise ValueError(f"{fn}: {query.shape[1] // k_cache.shape[2]} query heads per K/V head are not supported (at most 128: the heads of a "
                         "K/V head share one workgroup)")


class _Call:
    """A checked call, ready to launch: `stem` names the entry points (fasn_{stem}_append, fasn_fwd_{stem}...), `args` is the block they
    take and `kv` the fasn_kvcache_args inside it. The rest are the tensors whose addresses the block carries - they live as long as
    the call does, so until its launches are issued."""
    __slots__ = ("stem", "args", "kv", "dev", "packed", "qshape", "dtype", "out", "lse", "k_new", "v_new", "alibi", "keep")


def _scale_tensor(fn, name, value, query, Hkv) -> Tensor:
    """k_scale / v_scale as the fp32 [1 or B, 1 or Hkv] tensor the FP8 kernels read per (batch, K/V head). A Python number becomes a
    one-element tensor on the query's device, filled there; a tensor's values are not looked at (no host round trip: capturable)."""
    B = query.shape[0]
    if isinstance(value, (int, float)) and not isinstance(value, bool):
        return torch.full((1, 1), float(value), dtype=torch.float32, device=query.device)
    if not isinstance(value, Tensor) or not value.is_floating_point():
        got = value.dtype if isinstance(value, Tensor) else type(value).__name__
        raise TypeError(f"{fn}: {name} must be a Python float or a floating-point tensor; got {got}")
    shape = (1,) * (2 - value.dim()) + tuple(value.shape)
    if value.dim() > 2 or shape[0] not in (1, B) or shape[1] not in (1, Hkv):
        raise ValueError(f"{fn}: {name} must broadcast to [B, Hkv] = [{B}, {Hkv}] ([Hkv], [1, Hkv], [B, 1], [B, Hkv] or 0-d; Hkv = K/V heads); "
                         f"got {tuple(value.shape)}")
    if value.device != query.device:
        raise RuntimeError(f"{name} is on {value.device}, query on {query.device}: every operand must live on the query's device "
                           "(the scales are read by the kernels, never on the host)")
    if torch.is_grad_enabled() and value.requires_grad:
        raise RuntimeError(f"{fn} is forward only (inference): {name} requires grad and the scales carry no gradient. Call it under "
                           "torch.no_grad()")
    return value.detach().float().reshape(shape)


def _query_shaped(c) -> Tensor:
    """uninitialised, in the layout of `out` (and of the rotated queries): [B, H, Sq, D], or the [1, H, T, D] view of a packed [T, H, D]"""
    B, H, Sq, D = c.qshape
    if c.packed:   # (Sq is T here: one row per token, whatever B is)
        return torch.empty((Sq, H, D), dtype=c.dtype, device=c.dev).unsqueeze(0).transpose(1, 2)
    return torch.empty((B, H, Sq, D), dtype=c.dtype, device=c.dev)


def _prepare(fn, stem, query, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, is_causal, return_lse,
             alibi_slopes=None, query_seqlens=None, by_shape=False, cu_seqlens_q=None, max_seqlen_q=None, fp8=False) -> _Call:
    """The argument checks every entry point shares (they need no device and come first), the outputs and the filled argument block.
    `stem` says which block: "kvcache" (fasn_kvcache_args, at most _MAX_ROWS rows), "kvprefill" (fasn_kvprefill_args, with
    `query_seqlens`) or "kvvarlen" (fasn_kvvarlen_args: `query` is the [B, H, T, D] view of _packed_query, k_new / v_new and the outputs
    are token-packed, `cu_seqlens_q` and `max_seqlen_q` go into the block). `by_shape` (the window and rope calls, on "kvprefill"): the
    decode kernels run on the block's first member where the shapes allow them. `fp8`: the caches hold e4m3fn codes (the FP8 call)."""
    packed = stem == "kvvarlen"
    if query.dim() != 4 or k_cache.dim() != 4 or v_cache.dim() != 4:
        raise ValueError("query must be [B, H, Sq, D] and the caches [num_pages, page_size, Hkv, D] (paged) or [B, capacity, Hkv, D] (dense)")
    if query.dtype not in _KV_DTYPES:
        raise ValueError(f"{fn}: dtype {query.dtype} is not supported (fp16 and bf16 caches only)")
    B, H, Sq, D = query.shape
    dev = query.device
    tensors = {"k_cache": k_cache, "v_cache": v_cache, "cache_seqlens": cache_seqlens, "block_table": block_table, "k_new": k_new, "v_new": v_new}
    for name, t in tensors.items():
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name} is on {t.device}, query on {dev}: every operand must live on the query's device "
                               "(the lengths and the block table are read by the kernels, never on the host)")
    if fp8:
        if k_cache.dtype != torch.float8_e4m3fn or v_cache.dtype != torch.float8_e4m3fn:
            raise TypeError(f"{fn}: k_cache and v_cache must be torch.float8_e4m3fn (OCP e4m3fn codes; e5m2 and fnuz caches are not supported); "
                            f"got {k_cache.dtype} and {v_cache.dtype}. A 16-bit cache is flash_attention_n_kvcache / _prefill's")
    elif k_cache.dtype != query.dtype or v_cache.dtype != query.dtype:
        raise TypeError("query, k_cache and v_cache must share one dtype")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (query, k_cache, v_cache, k_new, v_new)) or (
            torch.is_grad_enabled() and isinstance(softmax_n_param, Tensor) and softmax_n_param.requires_grad):
        raise RuntimeError(f"{fn} is forward only (inference): an input requires grad. Call it under torch.no_grad(), "
                           "or use flash_attention_n, which differentiates q, k, v and a tensor n")
    if D not in _KV_HEAD_DIMS:
        raise ValueError(f"{fn}: head dim {D} is not supported (supported: {_KV_HEAD_DIMS}); a cache is never "
                         "zero-padded on the host")
    if fp8 and D not in _FP8_HEAD_DIMS:
        raise ValueError(f"{fn}: head dim {D} is not supported on an FP8 cache (supported: {_FP8_HEAD_DIMS}; 32 and 256 have 16-bit kernels only)")
    if k_cache.shape != v_cache.shape or k_cache.shape[3] != D:
        raise ValueError(f"k_cache and v_cache must have one shape [*, *, Hkv, {D}]; got {tuple(k_cache.shape)} and {tuple(v_cache.shape)}")
    page_size, Hkv = k_cache.shape[1], k_cache.shape[2]
    if Hkv < 1 or H % Hkv != 0:
        raise ValueError(f"the cache has {Hkv} K/V heads: must divide the {H} query heads (grouped-query attention)")
    G = H // Hkv
    if stem == "kvcache" and G * Sq > _MAX_ROWS:
        raise ValueError(f"(query heads per K/V head) x (query positions) = {G} x {Sq} = {G * Sq} rows exceed the {_MAX_ROWS} of one pass; "
                         "split the query positions over several calls, or use flash_attention_n_kvcache_prefill")
    if cache_seqlens.dtype != torch.int32 or cache_seqlens.dim() != 1 or cache_seqlens.shape[0] != B or not cache_seqlens.is_contiguous():
        raise ValueError(f"cache_seqlens must be a contiguous int32 tensor of shape [{B}] on the device; got {cache_seqlens.dtype} {tuple(cache_seqlens.shape)}")
    paged = block_table is not None
    if paged:
        if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.stride(1) != 1:
            raise ValueError(f"block_table must be an int32 tensor [B, max_pages] with unit column stride; got {block_table.dtype} {tuple(block_table.shape)}")
        if block_table.shape[0] != B:
            raise ValueError(f"block_table has {block_table.shape[0]} rows but the batch is {B}: one row of page ids per batch element")
        if block_table.shape[1] < 1:
            raise ValueError("block_table must name at least one page per batch element")
        if page_size % 64 != 0:
            raise ValueError(f"page_size {page_size} is not supported: a paged cache needs page_size % 64 == 0 (a 64-key tile never straddles a page)")
    elif k_cache.shape[0] != B:
        raise ValueError(f"dense cache (block_table=None) must be [B, capacity, Hkv, D] with B = {B}; got {tuple(k_cache.shape)}")
    _check_cache("k_cache", k_cache, paged, D)
    _check_cache("v_cache", v_cache, paged, D)
    if (k_new is None) != (v_new is None):
        raise ValueError("k_new and v_new come together")
    if k_new is not None:
        for name, t in (("k_new", k_new), ("v_new", v_new)):
            if packed:   # (Sq is T here)
                if t.dtype != query.dtype or tuple(t.shape) != (Sq, Hkv, D):
                    raise ValueError(f"{name} must be [T, Hkv, D] = [{Sq}, {Hkv}, {D}] in {query.dtype}, token-packed like query; got {tuple(t.shape)} {t.dtype}")
            elif t.dtype != query.dtype or tuple(t.shape) != (B, Hkv, Sq, D):
                raise ValueError(f"{name} must be [B, Hkv, Sq, D] = [{B}, {Hkv}, {Sq}, {D}] in {query.dtype}; got {tuple(t.shape)} {t.dtype}")
        if packed:
            k_new, v_new = k_new.unsqueeze(0).transpose(1, 2), v_new.unsqueeze(0).transpose(1, 2)   # [1, Hkv, T, D] views
        k_new, v_new = _rows(k_new), _rows(v_new)
    query = _rows(query)
    if isinstance(softmax_n_param, Tensor):
        nt = _n_tensor(softmax_n_param.detach(), query).contiguous()
        n = 0.0
    else:
        nt = None
        n = 0.0 if softmax_n_param is None else float(softmax_n_param)
        if n < 0:
            raise ValueError("softmax_n_param must be >= 0")
    st = None if alibi_slopes is None else _slopes_tensor(fn, alibi_slopes, query)
    scale = (1.0 / sqrt(D)) if scale is None else float(scale)
    # (the argument checks above need no device; everything below does)
    if not query.is_cuda:
        raise RuntimeError("flash_attention_softmax_n_amd runs on MI355X device tensors only; got a CPU tensor "
                           "(there is deliberately no CPU fallback)")

    c = _Call()
    c.dev, c.packed, c.qshape, c.dtype = dev, packed, (B, H, Sq, D), query.dtype
    c.out = out = _query_shaped(c)
    c.lse = lse = torch.empty((H, Sq) if packed else (B, H, Sq), dtype=torch.float32, device=dev) if return_lse else None
    top = _BLOCKS[stem]()
    if stem == "kvprefill":
        a = top.kv
        top.q_seqlens = None if query_seqlens is None else query_seqlens.data_ptr()
    elif packed:
        a = top.pf.kv
        top.pf.q_seqlens = None
        top.cu_seqlens_q, top.total_tokens, top.reserved = cu_seqlens_q.data_ptr(), Sq, 0
        Sq = min(max_seqlen_q, _INT_MAX)   # the block carries the bound of a sequence's query length
    else:
        a = top
    a.q, a.o = _view4(query), _view4(out)
    a.lse = None if lse is None else lse.data_ptr()
    a.k_cache, a.v_cache = k_cache.data_ptr(), v_cache.data_ptr()
    for i in range(3):
        a.k_stride[i] = k_cache.stride(i) if k_cache.size(i) > 1 else 0
        a.v_stride[i] = v_cache.stride(i) if v_cache.size(i) > 1 else 0
    if k_cache.size(1) == 1:   # (a one-row page still needs a row stride that covers the row)
        a.k_stride[1] = a.v_stride[1] = D
    if paged:
        a.block_table, a.block_table_stride, a.max_pages = block_table.data_ptr(), block_table.stride(0) if B > 1 else block_table.shape[1], block_table.shape[1]
    else:
        a.block_table, a.block_table_stride, a.max_pages = None, 0, 1
    a.seqlens = cache_seqlens.data_ptr()
    a.seqlen_add = Sq if k_new is not None else 0
    a.page_size = page_size
    a.B, a.H, a.kv_group, a.Sq, a.D = B, H, G, Sq, D
    a.dtype = _KV_DTYPES[query.dtype]
    a.scale, a.softmax_n, a.causal = scale, n, 1 if is_causal else 0
    if nt is not None:
        a.n = nt.data_ptr()
        a.n_stride_b, a.n_stride_h = _n_strides(nt)
    else:
        a.n, a.n_stride_b, a.n_stride_h = None, 0, 0
    c.alibi = None
    if st is not None:
        c.alibi = AlibiSlopes()
        c.alibi.slopes = st.data_ptr()
        c.alibi.stride_b, c.alibi.stride_h = _n_strides(st)
    # the one place that chooses the decode kernels over the prefill kernels, by shapes alone (capturable): both give the same function
    if by_shape and query_seqlens is None and G * Sq <= _MAX_ROWS:
        stem, top = "kvcache", a   # (the prefill block's first member is the decode call's block)
    c.stem, c.args, c.kv, c.k_new, c.v_new, c.keep = stem, top, a, k_new, v_new, (query, nt, st)
    return c


def _on_device(dev, launch) -> None:
    """run the launches with `dev` current"""
    if _current_device() == dev.index:
        launch()
    else:
        with torch.cuda.device(dev):
            launch()


def _append(lib, c, stream, rope=None, q_rot=None, tree=None, fp8=None) -> None:
    """k_new / v_new -> the cache rows behind the lengths; with `rope` the one launch that rotates them on the way and the queries into
    `q_rot`, which the forward then reads - under `tree` at the nodes' depth positions; with `fp8` the launch that quantises them; with
    `fp8` and `rope` the one launch that rotates, then quantises - under `tree` at the nodes' depth positions too. The entry point's
    name and its operands in ABI order follow from the operands present (_lib.kv_append_call)."""
    if rope is None and c.k_new is None:
        return
    views = [None if t is None else _view4(t) for t in (c.k_new, c.v_new)]   # (a rope call without them rotates the queries only)
    if c.packed and fp8 is not None:   # the packed FP8 sets have no named entry points: the operand-set call
        call = _lib.kv_call(c.args, fp8=fp8)
        _lib.check(lib.fasn_kv_append(call, rope, None if rope is None else _view4(q_rot), *views, stream), "fasn_kv_append")
    else:
        name, operands = _lib.kv_append_call(c.stem, fp8=fp8, tree=tree, rope=rope)
        if rope is not None:
            views.insert(0, _view4(q_rot))
        _lib.check(getattr(lib, name)(c.args, *operands, *views, stream), name)
    if rope is not None:
        c.kv.q = _view4(q_rot)


def _forward(lib, c, stream, win=None, tree=None, fp8=None) -> None:
    """workspace bytes -> allocate -> the forward of the base kernels or of their siblings under the operands present: ALiBi slopes
    (c.alibi), a window (`win`), a token tree (`tree`, which carries its window), an FP8 cache (`fp8`), or `fp8` with `win` or `tree`.
    The names and the operands in ABI order follow from the operands present (_lib.kv_forward_call: the ALiBi forward has the base
    call's workspace)."""
    stem = c.stem
    if c.packed and fp8 is not None:   # the packed FP8 sets have no named entry points: the operand-set calls (a packed call has its table)
        call = _lib.kv_call(c.args, fp8=fp8, window=win)
        ws_bytes = lib.fasn_kv_forward_workspace_bytes(call)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=c.dev)
        _lib.check(lib.fasn_kv_forward(call, ws.data_ptr(), ws_bytes, stream), "fasn_kv_forward")
        return
    ws_name, ws_operand, name, _plan, operand = _lib.kv_forward_call(stem, fp8=fp8, tree=tree, window=win, alibi=c.alibi)
    ws_bytes = getattr(lib, ws_name)(c.args, *ws_operand)
    # torch's caching allocator: capturable, as _launch_fwd's. Decode always combines its split partials and a packed call always has its
    # item table: both always pass a pointer; a prefill of one split has no partials and takes no workspace
    if stem != "kvprefill":
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=c.dev)
    else:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=c.dev) if ws_bytes else None
    _lib.check(getattr(lib, name)(c.args, *operand, None if ws is None else ws.data_ptr(), ws_bytes, stream), name)


def _run(c, window=None, rope=None, tree_mask=None, fp8_scales=None):
    """What every call does once it is checked: the library, the rotated-query temporary, then under the query's device the stream,
    the append and the forward; the outputs in the caller's layout. `tree_mask` ([B, Sq] int64): the token-tree operand, which takes the
    window with it. `fp8_scales` (k_scale, v_scale as _scale_tensor returns them): the FP8 operand."""
    lib = _lib.load()
    tree = None
    if tree_mask is not None:
        tree = KvTree(mask=tree_mask.data_ptr(), batch_stride=tree_mask.stride(0) if tree_mask.shape[0] > 1 else tree_mask.shape[1],
                      window=0 if window is None else min(window, _INT_MAX), reserved=0)
        window = None
    win = None if window is None else KvWindow(window=min(window, _INT_MAX), reserved=0)
    q_rot = None if rope is None else _query_shaped(c)   # (torch's caching allocator: a captured graph owns it)
    fp8 = None
    if fp8_scales is not None:
        ks, vs = fp8_scales
        fp8 = KvFp8(k_scale=ks.data_ptr(), v_scale=vs.data_ptr(), reserved=0)
        (fp8.k_sb, fp8.k_sh), (fp8.v_sb, fp8.v_sh) = _n_strides(ks), _n_strides(vs)

    def launch():
        stream = _stream_ptr(c.dev)
        _append(lib, c, stream, rope, q_rot, tree, fp8)
        _forward(lib, c, stream, win, tree, fp8)

    _on_device(c.dev, launch)
    out = c.out.transpose(1, 2).squeeze(0) if c.packed else c.out   # packed: [T, H, D] (lse is [H, T] as allocated)
    return out if c.lse is None else (out, c.lse)


def _packed_query(fn, query, k_cache, cache_seqlens, cu_seqlens_q, max_seqlen_q):
    """The checks of a token-packed step that the packed calls share, in front of _prepare: query, cu_seqlens_q, max_seqlen_q, B.
    Returns (B, T, the [B, H, T, D] view of the buffer - batch stride 0 - that _prepare takes as a query of B sequences)."""
    if not isinstance(query, Tensor) or query.dim() != 3:
        got = tuple(query.shape) if isinstance(query, Tensor) else type(query).__name__
        raise ValueError(f"{fn}: query must be token-packed [T, H, D]; got {got}")
    if (not isinstance(cu_seqlens_q, Tensor) or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.shape[0] < 2
            or not cu_seqlens_q.is_contiguous()):
        got = f"{cu_seqlens_q.dtype} {tuple(cu_seqlens_q.shape)}" if isinstance(cu_seqlens_q, Tensor) else type(cu_seqlens_q).__name__
        raise ValueError(f"{fn}: cu_seqlens_q must be a contiguous int32 tensor of shape [B + 1] on the device (B >= 1); got {got}")
    if cu_seqlens_q.device != query.device:
        raise RuntimeError(f"cu_seqlens_q is on {cu_seqlens_q.device}, query on {query.device}: every operand must live on the query's "
                           "device (the offsets are read by the kernels, never on the host)")
    if isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, int):
        raise TypeError(f"{fn}: max_seqlen_q must be a Python int (a bound of every query length, part of a captured graph; never a tensor); "
                        f"got {type(max_seqlen_q).__name__}")
    if max_seqlen_q < 1:
        raise ValueError(f"{fn}: max_seqlen_q must be >= 1; got {max_seqlen_q}")
    B = cu_seqlens_q.shape[0] - 1
    if isinstance(cache_seqlens, Tensor) and cache_seqlens.dim() == 1 and cache_seqlens.shape[0] != B:
        raise ValueError(f"{fn}: cu_seqlens_q names {B} sequences but cache_seqlens has {cache_seqlens.shape[0]}: B = cu_seqlens_q.shape[0] - 1 "
                         "is the batch of cache_seqlens and block_table")
    T = query.shape[0]
    if T < 1:
        raise ValueError(f"{fn}: the token buffer is empty (query is {tuple(query.shape)})")
    # the [B, H, T, D] view of the buffer (batch stride 0): the query of B sequences that _prepare checks and fills "kvvarlen" from
    q4 = _rows(query.unsqueeze(0).transpose(1, 2)).expand(B, -1, -1, -1)
    _check_group_limit(fn, q4, k_cache)
    return B, T, q4


def _check_rotary_tables(fn, rotary_cos, rotary_sin, query) -> None:
    """what the rotary tables are, whatever the call's shapes: the first checks of the rope calls"""
    for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
        if not isinstance(t, Tensor) or t.dim() != 2:
            got = tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__
            raise ValueError(f"{fn}: {name} must be a [rows, rotary_dim / 2] tensor; got {got}")
    if rotary_cos.shape != rotary_sin.shape or rotary_cos.dtype != rotary_sin.dtype or rotary_cos.stride(0) != rotary_sin.stride(0):
        raise ValueError(f"{fn}: rotary_cos and rotary_sin must have one shape, dtype and row stride; got {tuple(rotary_cos.shape)} "
                         f"{rotary_cos.dtype} and {tuple(rotary_sin.shape)} {rotary_sin.dtype}")
    if rotary_cos.dtype != torch.float32 and rotary_cos.dtype != query.dtype:
        raise ValueError(f"{fn}: rotary_cos / rotary_sin must be float32 or the dtype of query ({query.dtype}); got {rotary_cos.dtype}")


def _check_rotary_fit(fn, rotary_cos, rotary_sin, query, k_cache, block_table) -> None:
    """the tables against the call's shapes (`query`: [B, H, Sq, D], or the view of _packed_query): device, rotary_dim, rows >= capacity,
    alignment. They need no device: in front of _prepare and its CPU-tensor refusal (malformed shapes are _prepare's to name)"""
    rows, rd = rotary_cos.shape[0], 2 * rotary_cos.shape[1]
    esize = rotary_cos.element_size()
    if query.dim() == 4 and k_cache.dim() == 4 and (block_table is None or (isinstance(block_table, Tensor) and block_table.dim() == 2)):
        D = query.shape[3]
        capacity = k_cache.shape[1] * (1 if block_table is None else block_table.shape[1])
        for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
            if t.device != query.device:
                raise RuntimeError(f"{name} is on {t.device}, query on {query.device}: every operand must live on the query's device "
                                   "(the tables are read by the kernels, never on the host)")
        if D in _KV_HEAD_DIMS and (rd < 16 or rd > D or rd % 16 != 0):
            raise ValueError(f"{fn}: rotary_dim = 2 x {rotary_cos.shape[1]} = {rd} is not supported: 16 <= rotary_dim <= head dim {D} and "
                             "rotary_dim % 16 == 0 (a lane rotates 8 pairs)")
        if rows < capacity:
            raise ValueError(f"{fn}: the rotary tables cover {rows} positions but the cache holds up to {capacity}: rows >= capacity, so that "
                             "no position the lengths in device memory can name lies outside the tables")
        for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
            if t.stride(1) != 1 or t.data_ptr() % 16 != 0 or (rows > 1 and ((t.stride(0) * esize) % 16 != 0 or t.stride(0) < rd // 2)):
                raise ValueError(f"{fn}: {name}: rows must be 16-byte aligned, apart and with unit column stride (base pointer % 16 == 0, row "
                                 f"stride x {esize} bytes % 16 == 0, row stride >= rotary_dim / 2 = {rd // 2}); got strides {tuple(t.stride())}. "
                                 "A table is never copied here")


def _rope_operand(rotary_cos, rotary_sin, rotary_interleaved, query) -> KvRope:
    rows, rd = rotary_cos.shape[0], 2 * rotary_cos.shape[1]
    rope = KvRope()
    rope.cos, rope.sin = rotary_cos.data_ptr(), rotary_sin.data_ptr()
    rope.row_stride = rotary_cos.stride(0) if rows > 1 else rd // 2
    rope.rows, rope.rotary_dim = min(rows, _INT_MAX), rd
    rope.table_dtype = _lib.FASN_DTYPE_F32 if rotary_cos.dtype == torch.float32 else _KV_DTYPES[query.dtype]
    rope.interleaved = 1 if rotary_interleaved else 0
    return rope


def flash_attention_n_kvcache(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        is_causal: bool = True,
        return_lse: bool = False,
        alibi_slopes: Optional[Tensor] = None):
    """softmax_n attention of a few new query positions against a K/V cache, on MI355X.

    :param query: [B, H, Sq, D] fp16 / bf16 device tensor, D in {32, 64, 128, 256}; Sq = 1 is decode, a few positions speculative / chunked decode.
    :param k_cache, v_cache: paged [num_pages, page_size, Hkv, D] with `block_table` (page_size a multiple of 64), or dense
                  [B, capacity, Hkv, D] with block_table=None. Any strided view whose rows are 16-byte aligned with feature stride 1
                  (e.g. sliced out of a fused K/V buffer); never copied. H % Hkv == 0 and (H // Hkv) * Sq <= 128: the query heads of a
                  K/V head times the positions are the rows of one problem, so the cache is read once per K/V head.
    :param cache_seqlens: int32 [B] ON THE DEVICE: valid keys per batch element before this call. Not modified (the caller advances it).
    :param block_table: int32 [B, max_pages] on the device: page ids of each batch element, in order. Entries beyond the pages a batch
                  element needs are never read; cache rows at or beyond its length may hold anything (NaN included).
    :param k_new, v_new: optional [B, Hkv, Sq, D]: written to the cache positions cache_seqlens[b] .. + Sq - 1 first (positions at or
                  beyond the capacity are dropped) and then attended to: batch element b sees len_b = cache_seqlens[b] + Sq keys.
    :param softmax_n_param: n >= 0, or a floating tensor that broadcasts to [B, H] as in flash_attention_n (one n per batch element and
                  query head: attention sinks, n_h = exp(s_h)); no gradient here.
    :param scale: multiplies q.k^T; default 1/sqrt(D).
    :param is_causal: bottom-right aligned per batch element: position i sees key j iff j <= i + len_b - Sq. False: every position sees
                  all len_b keys.
    :param return_lse: also return lse [B, H, Sq] fp32 = log(n + sum_j exp(x_ij)).
    :param alibi_slopes: optional floating tensor on the query's device that broadcasts to [B, H] (one slope per query head, or per batch
                  element and head; e.g. synth.alibi_slopes(H)): the logit becomes x_ij = scale * q_i.k_j - slope[b, h] * |p_i - j| with
                  p_i = i + len_b - Sq the absolute position of query i - synth.alibi_bias's convention at S = len_b, L = Sq - computed in
                  the kernel from the length in device memory (no bias tensor; a replayed graph follows cache_seqlens). Converted to fp32,
                  never read on the host, no gradient. What is visible does not change; lse includes the bias.
    :return: [B, H, Sq, D] in query's dtype (and lse). Rows that see no key give exactly 0 and lse = log n (-inf for n = 0).
    """
    return _run(_prepare("flash_attention_n_kvcache", "kvcache", query, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new,
                         softmax_n_param, scale, is_causal, return_lse, alibi_slopes=alibi_slopes))


_SHARED_PREFIX_HEAD_DIMS = (64, 128)   # the head dims the shared-prefix kernels are built for


def _refuse_not_behind_prefix(fn, what, query, k_cache, block_table) -> None:
    """what the calls behind shared prefixes refuse in front of their operands' checks; `what`: "a shared prefix" / "shared prefixes" """
    if block_table is None:
        raise ValueError(f"{fn}: a dense cache (block_table=None) is not supported: a shared prefix is a set of pages that several block "
                         "tables name (paged caches only)")
    if isinstance(k_cache, Tensor) and k_cache.dtype == torch.float8_e4m3fn:
        raise TypeError(f"{fn}: a float8 cache is not supported (fp16 and bf16 caches only; the FP8 call is flash_attention_n_kvcache_fp8, "
                        f"without {what})")
    if query.dim() == 4 and query.shape[3] in _KV_HEAD_DIMS and query.shape[3] not in _SHARED_PREFIX_HEAD_DIMS:
        raise ValueError(f"{fn}: head dim {query.shape[3]} is not supported behind {what} (supported: {_SHARED_PREFIX_HEAD_DIMS}; "
                         "32 and 256 have the kernels of flash_attention_n_kvcache only)")


def _is_int32(t, dims) -> bool:
    return isinstance(t, Tensor) and t.dtype == torch.int32 and t.dim() == dims and t.is_contiguous()


def _got(t) -> str:
    return f"{t.dtype} {tuple(t.shape)}" if isinstance(t, Tensor) else type(t).__name__


def _check_on_query_device(query, read, **operands) -> None:
    for name, t in operands.items():
        if t.device != query.device:
            raise RuntimeError(f"{name} is on {t.device}, query on {query.device}: every operand must live on the query's device "
                               f"({read} are read by the kernels, never on the host)")


def _run_behind_prefix(c, operand, ws_fn, fwd_fn):
    """append -> workspace bytes -> allocate -> the forward `fwd_fn` of the prefix operand, under the query's device"""
    lib = _lib.load()

    def launch():
        stream = _stream_ptr(c.dev)
        _append(lib, c, stream)
        ws_bytes = getattr(lib, ws_fn)(c.args, operand)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=c.dev)   # (torch's caching allocator: capturable)
        _lib.check(getattr(lib, fwd_fn)(c.args, operand, ws.data_ptr(), ws_bytes, stream), fwd_fn)

    _on_device(c.dev, launch)
    return c.out if c.lse is None else (c.out, c.lse)


def flash_attention_n_kvcache_shared_prefix(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        block_table: Tensor,
        prefix_table: Tensor,
        prefix_len: Tensor,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        is_causal: bool = True,
        return_lse: bool = False):
    """flash_attention_n_kvcache for a batch that decodes behind ONE SHARED PREFIX (a system prompt, a few-shot header, N samples of one
    prompt), on MI355X: the prefix pages are attended to once per K/V head for the rows of all batch elements - packed into full 128-row
    blocks - each batch element's own keys as flash_attention_n_kvcache walks them, and the two are merged (fasn_fwd_shared_prefix).

    With P = clamp(prefix_len, 0, min(max_prefix_pages * page_size, capacity)), computed in the kernels, every batch element b has the
    virtual cache whose key row j < P is row j % page_size of page prefix_table[j // page_size] and whose key row j >= P is the row
    block_table[b] names. The result is exactly flash_attention_n_kvcache's on that cache: len_b, the positions, causal visibility,
    n (counted once per row) and lse do not depend on P. A batch element shorter than the prefix sees prefix keys up to its own limit; P
    need not be a multiple of the page size (a partially shared last page, copy on write). `query`, the paged 16-bit caches,
    `cache_seqlens`, `block_table`, `k_new` / `v_new`, `softmax_n_param`, `scale`, `is_causal`, `return_lse`, alignment rules and refusals
    are those of flash_attention_n_kvcache, with (H // Hkv) * Sq <= 128. What differs:

    :param block_table: required (a shared prefix is a set of pages; a dense cache is refused). Slots wholly below P are never read.
    :param prefix_table: contiguous int32 [max_prefix_pages] on the device: the page ids of the shared prefix, in order.
    :param prefix_len: int32 tensor of ONE element on the device; never read on the host, so one captured graph serves every step and
                  every prefix length.
    :param k_new, v_new: appended to the batch element's OWN pages at cache_seqlens[b] + i, as in flash_attention_n_kvcache; rows that
                  land below P are never read.
    Head dims 64 and 128, fp16 / bf16 caches; an FP8 cache, ALiBi, a window, rotary embedding, a token tree and packed queries are not
    served by this call.

    Memory contract. For keys below P, block_table[b] entries and the batch element's own cache rows are never read. Prefix-page rows at
    or beyond P and prefix_table entries at or beyond ceil(P / page_size) are never read. Rows at or beyond len_b may hold anything.
    """
    fn = "flash_attention_n_kvcache_shared_prefix"
    _refuse_not_behind_prefix(fn, "a shared prefix", query, k_cache, block_table)
    if not _is_int32(prefix_table, 1) or prefix_table.shape[0] < 1:
        raise ValueError(f"{fn}: prefix_table must be a contiguous int32 tensor of shape [max_prefix_pages] on the device (at least one "
                         f"page); got {_got(prefix_table)}")
    if not isinstance(prefix_len, Tensor) or prefix_len.dtype != torch.int32 or prefix_len.numel() != 1:
        raise ValueError(f"{fn}: prefix_len must be an int32 tensor of one element on the device (it is read by the kernels, never on "
                         f"the host; not a Python int); got {_got(prefix_len)}")
    _check_on_query_device(query, "the prefix length and its page ids", prefix_table=prefix_table, prefix_len=prefix_len)
    c = _prepare(fn, "kvcache", query, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, is_causal,
                 return_lse)
    prefix = SharedPrefix(prefix_len=prefix_len.data_ptr(), prefix_table=prefix_table.data_ptr(),
                          max_prefix_pages=min(prefix_table.shape[0], _INT_MAX), reserved=0)
    return _run_behind_prefix(c, prefix, "fasn_fwd_shared_prefix_workspace_bytes", "fasn_fwd_shared_prefix")


def flash_attention_n_kvcache_prefix_groups(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        block_table: Tensor,
        prefix_tables: Tensor,
        prefix_lens: Tensor,
        prefix_group: Tensor,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        is_causal: bool = True,
        return_lse: bool = False):
    """flash_attention_n_kvcache for a batch that decodes behind SEVERAL SHARED PREFIXES (a server that holds a few system prompts, N
    samples of each of M prompts, sequences that share nothing), on MI355X, in one call: flash_attention_n_kvcache_shared_prefix with one
    prefix per GROUP of batch elements. A schedule kernel sorts the batch by group on the device; the pages of every prefix that has a
    member are attended to once per K/V head for the rows of its members - packed into 128-row blocks that never mix groups - each batch
    element's own keys as flash_attention_n_kvcache walks them, and the two are merged (fasn_fwd_prefix_groups).

    For a batch element b with g = prefix_group[b] in [0, G): P_b = clamp(prefix_lens[g], 0, min(max_prefix_pages * page_size, capacity)),
    key row j < P_b is row j % page_size of page prefix_tables[g, j // page_size] and key row j >= P_b is the row block_table[b] names.
    For every other b, P_b = 0: its cache is the one flash_attention_n_kvcache sees. The result is exactly flash_attention_n_kvcache's on
    that virtual cache: len_b, the positions, causal visibility, n (counted once per row) and lse do not depend on P_b; P_b need not be a
    multiple of the page size or of 64; a batch element shorter than its prefix sees prefix keys up to its own limit. With every entry of
    prefix_group out of range the result is flash_attention_n_kvcache's bit for bit, with G = 1 and every entry 0
    flash_attention_n_kvcache_shared_prefix's. Operands, append, alignment rules and refusals are those of
    flash_attention_n_kvcache_shared_prefix. What differs:

    :param prefix_tables: contiguous int32 [G, max_prefix_pages] on the device: row g holds the page ids of prefix g, in order.
                  1 <= G <= 1024 (the schedule kernel keeps its counters per group in LDS).
    :param prefix_lens: contiguous int32 [G] on the device.
    :param prefix_group: contiguous int32 [B] on the device: the prefix of batch element b; any value outside [0, G) - -1, say - means
                  "no shared prefix".
    None of the three is read on the host, so one captured graph serves every assignment of sequences to prefixes, every prefix length
    and every step.

    Memory contract. For keys below P_b, block_table[b] entries and the batch element's own cache rows are never read. Rows of a prefix
    page at or beyond that prefix's P and prefix_tables[g] entries at or beyond ceil(P_g / page_size) are never read, nor are the whole
    table row and every page of a group that has no member. Rows at or beyond len_b may hold anything. Whatever prefix_group and
    prefix_lens hold, no access leaves the operands.
    """
    fn = "flash_attention_n_kvcache_prefix_groups"
    _refuse_not_behind_prefix(fn, "shared prefixes", query, k_cache, block_table)
    if not _is_int32(prefix_tables, 2) or prefix_tables.shape[0] < 1 or prefix_tables.shape[1] < 1:
        raise ValueError(f"{fn}: prefix_tables must be a contiguous int32 tensor of shape [G, max_prefix_pages] on the device (at least one "
                         f"group and one page); got {_got(prefix_tables)}")
    G = prefix_tables.shape[0]
    if G > _lib.FASN_PREFIX_GROUPS_MAX:
        raise ValueError(f"{fn}: {G} prefix groups exceed the {_lib.FASN_PREFIX_GROUPS_MAX} of one call (the schedule kernel keeps its "
                         "counters per group in LDS)")
    if not _is_int32(prefix_lens, 1):
        raise ValueError(f"{fn}: prefix_lens must be a contiguous int32 tensor of shape [G] on the device (it is read by the kernels, never "
                         f"on the host); got {_got(prefix_lens)}")
    if prefix_lens.shape[0] != G:
        raise ValueError(f"{fn}: prefix_lens has {prefix_lens.shape[0]} entries, prefix_tables {G} rows: one length per prefix")
    if not _is_int32(prefix_group, 1):
        raise ValueError(f"{fn}: prefix_group must be a contiguous int32 tensor of shape [B] on the device (it is read by the kernels, never "
                         f"on the host); got {_got(prefix_group)}")
    if query.dim() == 4 and prefix_group.shape[0] != query.shape[0]:
        raise ValueError(f"{fn}: prefix_group has {prefix_group.shape[0]} entries, the batch {query.shape[0]} elements: one group per batch "
                         "element (any value outside [0, G) for none)")
    _check_on_query_device(query, "the prefixes, their lengths and the groups", prefix_tables=prefix_tables, prefix_lens=prefix_lens,
                           prefix_group=prefix_group)
    c = _prepare(fn, "kvcache", query, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, is_causal,
                 return_lse)
    groups = PrefixGroups(prefix_lens=prefix_lens.data_ptr(), prefix_tables=prefix_tables.data_ptr(), prefix_group=prefix_group.data_ptr(),
                          num_groups=G, max_prefix_pages=min(prefix_tables.shape[1], _INT_MAX), reserved=0)
    return _run_behind_prefix(c, groups, "fasn_fwd_prefix_groups_workspace_bytes", "fasn_fwd_prefix_groups")


def flash_attention_n_kvcache_prefill(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        query_seqlens: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        is_causal: bool = True,
        return_lse: bool = False,
        alibi_slopes: Optional[Tensor] = None):
    """softmax_n attention of ANY number of new query positions against a K/V cache, on MI355X: prefill, chunked prefill, a prefix-cache hit.

    The cache, `block_table`, `cache_seqlens`, `softmax_n_param`, `scale`, dtypes, head dims, alignment rules and refusals are those of
    flash_attention_n_kvcache. What differs:

    :param query: [B, H, Sq, D], any Sq >= 1 (no row limit: the G = H // Hkv query heads of a K/V head times 128 // G consecutive
                  positions are the rows of one workgroup, so the cache is still read once per K/V head and row block; G <= 128).
    :param k_new, v_new: optional [B, Hkv, Sq, D]: rows i < qlen_b are written to the cache positions cache_seqlens[b] + i first (positions
                  at or beyond the capacity are dropped in the kernel) and then attended to. `cache_seqlens` is not modified.
    :param query_seqlens: optional contiguous int32 [B] ON THE DEVICE: qlen_b = clamp(query_seqlens[b], 0, Sq); None means Sq. A ragged
                  batch of prompts or chunks padded to Sq. Never read on the host.
    :param is_causal: with len_b = clamp(cache_seqlens[b] + (qlen_b if k_new is given else 0), 0, capacity), position i < qlen_b sees key j
                  iff j < len_b and (causal) j <= i + len_b - qlen_b: bottom-right aligned per batch element.
    :param alibi_slopes: as in flash_attention_n_kvcache, with p_i = i + len_b - qlen_b: the absolute position of query i of batch element
                  b follows cache_seqlens and query_seqlens in device memory.
    :return: [B, H, Sq, D] in query's dtype (and lse [B, H, Sq] fp32). A position that sees no key gives exactly 0 and lse = log n (-inf
             for n = 0); padding positions i >= qlen_b give exactly 0 and lse = -inf whatever n is.
    """
    fn = "flash_attention_n_kvcache_prefill"
    _check_query_seqlens(fn, query_seqlens, query)
    _check_group_limit(fn, query, k_cache)
    return _run(_prepare(fn, "kvprefill", query, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale,
                         is_causal, return_lse, alibi_slopes=alibi_slopes, query_seqlens=query_seqlens))


def flash_attention_n_kvcache_varlen(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        cu_seqlens_q: Tensor,
        max_seqlen_q: int,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        is_causal: bool = True,
        return_lse: bool = False,
        alibi_slopes=None,
        window=None,
        rotary_cos=None,
        rotary_sin=None):
    """softmax_n attention of a CONTINUOUS-BATCHING step against a K/V cache, on MI355X: the query positions of all sequences - prompt
    chunks of thousands of tokens beside decode sequences of one - token-packed in one buffer (vLLM's flash_attn_varlen_func with a
    block table). The work, the grid and the memory follow the tokens, not B x the longest chunk.

    The cache, `block_table`, `cache_seqlens`, `softmax_n_param`, `scale`, `is_causal`, dtypes, head dims, alignment rules and refusals
    are those of flash_attention_n_kvcache_prefill. What differs:

    :param query: [T, H, D], T = the size of the step's token buffer (a shape: part of a captured graph).
    :param cu_seqlens_q: contiguous int32 [B + 1] ON THE DEVICE: cu[0] = 0, non-decreasing, cu[B] <= T. Token cu[b] + i is position
                  i < qlen_b of sequence b, qlen_b = clamp(cu[b + 1] - cu[b], 0, max_seqlen_q). B = cu_seqlens_q.shape[0] - 1 must be the
                  B of `cache_seqlens` (and `block_table`). Never read on the host.
    :param max_seqlen_q: a Python int >= 1: an upper bound of every qlen_b, a constant of a captured graph (with T it sizes the grid).
    :param k_new, v_new: optional [T, Hkv, D], token-packed like `query`: token cu[b] + i is written to the cache position
                  cache_seqlens[b] + i first (positions at or beyond the capacity are dropped in the kernel) and then attended to.
    :param softmax_n_param: n >= 0, or a tensor that broadcasts to [B, H]: per sequence and query head, not per token.
    :param alibi_slopes, window, rotary_cos, rotary_sin: anything but None is refused here. A sliding window and rotary embedding on
                  packed queries are calls of their own: flash_attention_n_kvcache_varlen_window, flash_attention_n_kvcache_varlen_rope.
    :return: [T, H, D] in query's dtype (and lse [H, T] fp32). With len_b = clamp(cache_seqlens[b] + (qlen_b if k_new is given else 0),
             0, capacity), position i sees key j iff j < len_b and (causal) j <= i + len_b - qlen_b; a token that sees no key gives
             exactly 0 and lse = log n (-inf for n = 0).

    Tokens at or beyond cu[B] are never read (the buffer may hold NaN there) and their rows of `out` / `lse` are NOT WRITTEN: they hold
    whatever the allocation held. Nothing is read on the host: the launches depend on T, B, max_seqlen_q, the head counts, D and the
    capacity only, so one captured graph serves every step. Whatever values `cu_seqlens_q` holds, no kernel touches memory outside the
    buffers (token indices are clamped to [0, T), lengths as above): malformed offsets give unspecified values but stay safe. One split
    count serves the whole launch, so the decode tokens of a mixed step get the launch's, not their own.
    """
    fn = "flash_attention_n_kvcache_varlen"
    for name, value in (("alibi_slopes", alibi_slopes), ("window", window), ("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
        if value is not None:
            raise NotImplementedError(f"{fn}: {name} is not supported on token-packed queries (no packed ALiBi, window or rotary kernels yet); "
                                      "pad the step and use flash_attention_n_kvcache_prefill / _window / _rope with query_seqlens")
    _B, _T, q4 = _packed_query(fn, query, k_cache, cache_seqlens, cu_seqlens_q, max_seqlen_q)
    return _run(_prepare(fn, "kvvarlen", q4, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale,
                         is_causal, return_lse, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q))


def flash_attention_n_kvcache_varlen_window(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        cu_seqlens_q: Tensor,
        max_seqlen_q: int,
        window: int,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        return_lse: bool = False):
    """softmax_n attention of a SLIDING-WINDOW layer on a CONTINUOUS-BATCHING step, on MI355X: flash_attention_n_kvcache_window on the
    token-packed buffers of flash_attention_n_kvcache_varlen (every other layer of GPT-OSS, Mistral).

    Always causal. With qlen_b = clamp(cu[b + 1] - cu[b], 0, max_seqlen_q), len_b = clamp(cache_seqlens[b] + (qlen_b if k_new is given
    else 0), 0, capacity) and p_i = i + len_b - qlen_b, token cu[b] + i sees key j iff j < len_b and p_i - window < j <= p_i. `query`,
    `cu_seqlens_q`, `max_seqlen_q`, `k_new` / `v_new`, the cache, `softmax_n_param`, `scale`, the outputs ([T, H, D], lse [H, T]; rows at or
    beyond cu[B] are not written) and the refusals are those of flash_attention_n_kvcache_varlen. What differs:

    :param window: a Python int >= 1, a constant of the layer and part of a captured graph. A window at or beyond the capacity sees what
                  flash_attention_n_kvcache_varlen sees.

    Memory contract, per sequence: flash_attention_n_kvcache_window's. Let first_b = 64 * floor(max(0, len_b - qlen_b - window + 1) / 64).
    Cache rows j < first_b are never read and neither are the block-table entries of pages wholly below first_b: a server may free them.
    Nothing is read on the host: the launches depend on T, B, max_seqlen_q, the head counts, D, the capacity and `window` only. One split
    count serves the launch, from the tiles a window can touch: never more splits than flash_attention_n_kvcache_varlen has.
    """
    fn = "flash_attention_n_kvcache_varlen_window"
    _check_window(fn, window)
    _B, _T, q4 = _packed_query(fn, query, k_cache, cache_seqlens, cu_seqlens_q, max_seqlen_q)
    return _run(_prepare(fn, "kvvarlen", q4, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale,
                         True, return_lse, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q), window=window)


def flash_attention_n_kvcache_varlen_rope(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        cu_seqlens_q: Tensor,
        max_seqlen_q: int,
        rotary_cos: Tensor,
        rotary_sin: Tensor,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        is_causal: bool = True,
        return_lse: bool = False,
        window: Optional[int] = None,
        rotary_interleaved: bool = False):
    """softmax_n attention of a CONTINUOUS-BATCHING step with ROTARY POSITION EMBEDDING applied to `query` and `k_new` on the way, on
    MI355X: flash_attention_n_kvcache_rope on the token-packed buffers of flash_attention_n_kvcache_varlen - one layer step of a served
    Llama / Mistral / GPT-OSS: rotate, append, attend.

    With qlen_b, len_b and p_i = i + len_b - qlen_b as in flash_attention_n_kvcache_varlen, ONE launch rotates token cu[b] + i of k_new at
    position cache_seqlens[b] + i into the cache (positions < 0 or >= the capacity are dropped), copies v_new beside it and rotates the
    query token at p_i into a [T, H, D] temporary the forward then reads. Tokens at or beyond cu[B] are neither read nor written.
    `query`, `cu_seqlens_q`, `max_seqlen_q`, `k_new` / `v_new`, the cache, `softmax_n_param`, `scale`, `is_causal`, the outputs and the
    refusals are those of flash_attention_n_kvcache_varlen; `rotary_cos` / `rotary_sin` (layouts, rotary_dim, the table row
    clamp(position, 0, rows - 1), rows >= capacity) and `rotary_interleaved` those of flash_attention_n_kvcache_rope, as is the arithmetic:
    bit for bit (x1.float() * cos.float() - x2.float() * sin.float()).to(dtype) of eager torch.

    :param k_new, v_new: optional [T, Hkv, D]. Without them only `query` is rotated, at p_i over the cache as it is.
    :param window: None: flash_attention_n_kvcache_varlen's attention; a Python int >= 1: flash_attention_n_kvcache_varlen_window's
                  (needs is_causal=True).
    :return: [T, H, D] (and lse [H, T]). `query`, `k_new`, `cache_seqlens` are not modified.

    Nothing is read on the host: the launches depend on T, B, max_seqlen_q, the head counts, D, the capacity and `window` only, so one
    captured graph serves every step. No ALiBi slopes here (a model uses one or the other).
    """
    fn = "flash_attention_n_kvcache_varlen_rope"
    if window is not None:
        _check_window(fn, window, or_none="None or ")
        if not is_causal:
            raise ValueError(f"{fn}: a sliding window is always causal; window={window} needs is_causal=True")
    _B, _T, q4 = _packed_query(fn, query, k_cache, cache_seqlens, cu_seqlens_q, max_seqlen_q)
    _check_rotary_tables(fn, rotary_cos, rotary_sin, query)
    _check_rotary_fit(fn, rotary_cos, rotary_sin, q4, k_cache, block_table)
    c = _prepare(fn, "kvvarlen", q4, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, is_causal,
                 return_lse, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q)
    return _run(c, window=window, rope=_rope_operand(rotary_cos, rotary_sin, rotary_interleaved, query))


def flash_attention_n_kvcache_window(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        window: int,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        query_seqlens: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        return_lse: bool = False):
    """softmax_n attention of a SLIDING-WINDOW layer against a K/V cache, on MI355X: decode, chunked prefill or prefill in one call.

    Always causal. With qlen_b = clamp(query_seqlens[b], 0, Sq) (None: Sq), len_b = clamp(cache_seqlens[b] + (qlen_b if k_new is given
    else 0), 0, capacity) and p_i = i + len_b - qlen_b the absolute position of query i, position i < qlen_b sees key j iff
    j < len_b and p_i - window < j <= p_i: `window` keys, its own included (Hugging Face `sliding_window`, GPT-OSS, Mistral).
    The cache, `block_table`, `cache_seqlens`, `k_new` / `v_new`, `query_seqlens`, `softmax_n_param`, `scale`, dtypes, head dims,
    alignment rules and refusals are those of flash_attention_n_kvcache_prefill. What differs:

    :param window: a Python int >= 1, a constant of the layer: it is part of a captured graph, while the lengths stay on the device. A
                  window at or beyond the capacity sees what the call without a window sees.
    :param query_seqlens: as in flash_attention_n_kvcache_prefill. The kernels are chosen by shapes alone (capturable): with
                  query_seqlens=None and (H // Hkv) * Sq <= 128 the decode kernels run, otherwise the prefill kernels; both give the
                  same function.
    :return: [B, H, Sq, D] in query's dtype (and lse [B, H, Sq] fp32 over the visible keys plus n). A position that sees no key
             (p_i < 0) gives exactly 0 and lse = log n (-inf for n = 0); padding positions i >= qlen_b give exactly 0 and lse = -inf.

    Memory contract. Let first_b = 64 * floor(max(0, len_b - qlen_b - window + 1) / 64). Cache rows j < first_b are never read, and
    neither are the block-table entries of pages that lie wholly below first_b: both may hold anything (NaN, a freed page, a page that
    was handed to another sequence), so a server may free every page wholly below the window. Rows first_b .. len_b - 1 are read in
    tiles of 64 keys and must hold finite values (they are rows an earlier append wrote). Rows at or beyond len_b may hold anything,
    as in the other cache calls. The work and the K/V traffic follow the window, not the length.
    """
    fn = "flash_attention_n_kvcache_window"
    _check_window(fn, window)
    _check_query_seqlens(fn, query_seqlens, query)
    _check_group_limit(fn, query, k_cache)
    return _run(_prepare(fn, "kvprefill", query, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale,
                         True, return_lse, query_seqlens=query_seqlens, by_shape=True), window=window)


def flash_attention_n_kvcache_rope(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        rotary_cos: Tensor,
        rotary_sin: Tensor,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        query_seqlens: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        is_causal: bool = True,
        return_lse: bool = False,
        window: Optional[int] = None,
        rotary_interleaved: bool = False):
    """softmax_n attention against a K/V cache with ROTARY POSITION EMBEDDING applied to `query` and `k_new` on the way, on MI355X: one
    step of a Llama / Mistral / GPT-OSS layer - rotate, append, attend - in the launches of the plain call with `k_new`.

    With qlen_b = clamp(query_seqlens[b], 0, Sq) (None: Sq) and len_b = clamp(cache_seqlens[b] + (qlen_b if k_new is given else 0), 0,
    capacity), ONE launch rotates row i < qlen_b of k_new[b] at position cache_seqlens[b] + i into the cache (positions at or beyond the
    capacity are dropped), copies v_new beside it and rotates query position i at p_i = i + len_b - qlen_b - the absolute position the
    ALiBi and window calls use - into a temporary the forward then reads. The positions come from the lengths in device memory: nothing
    is read on the host, a captured graph follows `cache_seqlens` / `query_seqlens`. The cache, `block_table`, `cache_seqlens`, `k_new` /
    `v_new`, `query_seqlens`, `softmax_n_param`, `scale`, dtypes, head dims, alignment rules and refusals are those of
    flash_attention_n_kvcache_prefill; the kernels are chosen by shapes alone as in flash_attention_n_kvcache_window (query_seqlens=None and
    (H // Hkv) * Sq <= 128: the decode kernels). What differs:

    :param rotary_cos, rotary_sin: [rows, rotary_dim / 2] on the query's device, fp32 or the dtype of `query`, unit column stride, rows
                  16-byte aligned (never copied: pass a slice of a longer table as it is); rows >= capacity, 16 <= rotary_dim <= D,
                  rotary_dim % 16 == 0. Features d >= rotary_dim pass through. The row read is clamp(position, 0, rows - 1): the clamp acts
                  only on the negative p_i of causal rows that see no key. YaRN / NTK scaling and an attention factor live in the tables.
    :param k_new, v_new: optional. Without them only `query` is rotated, at p_i = i + len_b - qlen_b over the cache as it is.
    :param window: None: flash_attention_n_kvcache / _prefill's attention; a Python int >= 1: flash_attention_n_kvcache_window's (needs
                  is_causal=True).
    :param rotary_interleaved: False: the half-split layout (GPT-NeoX / Llama / GPT-OSS, Hugging Face rotate_half) - the pair of feature
                  d < rotary_dim / 2 is (x[d], x[d + rotary_dim / 2]); True: GPT-J - the pair is (x[2 d], x[2 d + 1]). Both use cos[pos, d]:
                  y1 = x1 cos - x2 sin, y2 = x2 cos + x1 sin.
    :return: as the call without rotary. `query`, `k_new`, `cache_seqlens` are not modified.

    Arithmetic: operands widened to fp32, every product and the sum rounded to fp32 on their own (no fused multiply-add), one rounding
    to the 16-bit type - bit for bit (x1.float() * cos.float() - x2.float() * sin.float()).to(dtype) of eager torch. No ALiBi slopes here
    (a model uses one or the other), no explicit position tensor, no gradient.
    """
    fn = "flash_attention_n_kvcache_rope"
    if window is not None:
        _check_window(fn, window, or_none="None or ")
        if not is_causal:
            raise ValueError(f"{fn}: a sliding window is always causal; window={window} needs is_causal=True")
    _check_rotary_tables(fn, rotary_cos, rotary_sin, query)
    _check_query_seqlens(fn, query_seqlens, query)
    _check_group_limit(fn, query, k_cache)
    _check_rotary_fit(fn, rotary_cos, rotary_sin, query, k_cache, block_table)
    c = _prepare(fn, "kvprefill", query, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, is_causal,
                 return_lse, query_seqlens=query_seqlens, by_shape=True)
    return _run(c, window=window, rope=_rope_operand(rotary_cos, rotary_sin, rotary_interleaved, query))


def flash_attention_n_kvcache_fp8(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        k_scale,
        v_scale,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        query_seqlens: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        is_causal: bool = True,
        return_lse: bool = False,
        alibi_slopes=None,
        window=None,
        rotary_cos=None,
        rotary_sin=None,
        cu_seqlens_q=None,
        tree_mask=None):
    """softmax_n attention against an FP8 K/V CACHE, on MI355X: decode, chunked prefill or prefill in one call over a cache of one-byte
    e4m3fn codes with per-(batch element, K/V head) scales - half the bytes a key costs the HBM-bound decode call, twice the tokens per GiB.

    A cache element is an OCP e4m3fn code (torch.float8_e4m3fn) and its value is the exact upcast of the code times the scale of its
    (b, hkv). All 254 finite codes are fp16 and bf16 numbers, so the kernels hand the codes themselves to the 16-bit MFMAs and the scales
    act in fp32 only:
        x_ij  = scale * k_scale[b, hkv] * (q_i . up(Kc_j))
        out_i = v_scale[b, hkv] * sum_j p_ij up(Vc_j) / (n + sum_j p_ij)          rounded once, after the scale
    With power-of-two scales the result is, bit for bit, flash_attention_n_kvcache / _prefill on `k_cache.to(query.dtype)`. `block_table`,
    `cache_seqlens`, `query_seqlens`, `softmax_n_param`, `scale`, `is_causal`, the outputs, visibility (len_b, qlen_b), rows that see
    nothing and the stale-memory rules are those of flash_attention_n_kvcache_prefill; the kernels are chosen by shapes alone as in
    flash_attention_n_kvcache_window (query_seqlens=None and (H // Hkv) * Sq <= 128: the decode kernels). What differs:

    :param query: [B, H, Sq, D] fp16 / bf16, D in {64, 128}.
    :param k_cache, v_cache: torch.float8_e4m3fn, paged [num_pages, page_size, Hkv, D] (page_size % 64 == 0) or dense [B, capacity, Hkv, D];
                  feature stride 1, base pointer and page / row / head strides multiples of 16 BYTES; never copied. Rows at or beyond
                  len_b may hold any byte (the NaN code 0x7f included); a NaN code in a visible row is a NaN.
    :param k_scale, v_scale: a Python float, or a floating tensor on the query's device that broadcasts to [B, Hkv] ([Hkv], [1, Hkv],
                  [B, 1], [B, Hkv] or 0-d). Read by the kernels, never on the host: a captured graph follows them. A non-positive or
                  non-finite scale is the caller's error: the result is unspecified, no memory outside the buffers is touched.
    :param k_new, v_new: optional [B, Hkv, Sq, D] in query's dtype: rows i < qlen_b are QUANTISED and written to the cache positions
                  cache_seqlens[b] + i first - code = rne_e4m3(clamp(float(x) / s, -448, 448)), s the scale of (b, hkv), the division
                  correctly rounded in fp32, saturating, NaN -> a NaN code - and then attended to. `cache_seqlens` is not modified.
    :param alibi_slopes, window, rotary_cos, rotary_sin, cu_seqlens_q, tree_mask: anything but None is refused here. A sliding window
                  and rotary embedding on an FP8 cache are calls of their own: flash_attention_n_kvcache_fp8_window,
                  flash_attention_n_kvcache_fp8_rope; a token tree is flash_attention_n_kvcache_fp8_tree's; token-packed queries are
                  flash_attention_n_kvcache_fp8_varlen's (this call keeps its [B, H, Sq, D] query). ALiBi has 16-bit kernels only.
    :return: [B, H, Sq, D] in query's dtype (and lse [B, H, Sq] fp32).
    """
    fn = "flash_attention_n_kvcache_fp8"
    for name, value in (("alibi_slopes", alibi_slopes), ("window", window), ("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin),
                        ("cu_seqlens_q", cu_seqlens_q), ("tree_mask", tree_mask)):
        if value is not None:
            if name in ("window", "rotary_cos", "rotary_sin"):
                raise NotImplementedError(f"{fn}: {name} is not supported on an FP8 cache by this call; use flash_attention_n_kvcache_fp8_window "
                                          "(a sliding window) or flash_attention_n_kvcache_fp8_rope (rotary embedding, with or without a window)")
            if name == "tree_mask":
                raise NotImplementedError(f"{fn}: {name} is not supported on an FP8 cache by this call; use flash_attention_n_kvcache_fp8_tree "
                                          "(token-tree verification over the FP8 cache)")
            raise NotImplementedError(f"{fn}: {name} is not supported on an FP8 cache (no FP8 ALiBi or packed kernels yet); use a 16-bit "
                                      "cache with the call of that name")
    _check_query_seqlens(fn, query_seqlens, query)
    _check_group_limit(fn, query, k_cache)
    Hkv = k_cache.shape[2] if k_cache.dim() == 4 and query.dim() == 4 else 1
    scales = None
    if query.dim() == 4:
        scales = (_scale_tensor(fn, "k_scale", k_scale, query, Hkv), _scale_tensor(fn, "v_scale", v_scale, query, Hkv))
    c = _prepare(fn, "kvprefill", query, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, is_causal,
                 return_lse, query_seqlens=query_seqlens, by_shape=True, fp8=True)
    return _run(c, fp8_scales=scales)


def _fp8_scales(fn, k_scale, v_scale, query, k_cache):
    """both scales through _scale_tensor (malformed shapes are _prepare's to name)"""
    if query.dim() != 4:
        return None
    Hkv = k_cache.shape[2] if k_cache.dim() == 4 else 1
    return _scale_tensor(fn, "k_scale", k_scale, query, Hkv), _scale_tensor(fn, "v_scale", v_scale, query, Hkv)


def flash_attention_n_kvcache_fp8_window(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        k_scale,
        v_scale,
        window: int,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        query_seqlens: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        return_lse: bool = False):
    """softmax_n attention of a SLIDING-WINDOW layer against an FP8 K/V CACHE, on MI355X: flash_attention_n_kvcache_window's visibility and
    memory contract over flash_attention_n_kvcache_fp8's cache - the sliding layers of GPT-OSS / Mistral keep the capacity gain, and the
    pages below the window can still be freed.

    Always causal. With qlen_b, len_b and p_i = i + len_b - qlen_b as in flash_attention_n_kvcache_window, position i < qlen_b sees key j
    iff j < len_b and p_i - window < j <= p_i; the values, the scales, `k_new` / `v_new` (quantised on the way in), the caches' rules and the
    refusals are those of flash_attention_n_kvcache_fp8, `query_seqlens` and the choice of kernels by shapes alone those of
    flash_attention_n_kvcache_window. With power-of-two scales the result is, bit for bit, flash_attention_n_kvcache_window on
    `k_cache.to(query.dtype)`; a window at or beyond the capacity sees what flash_attention_n_kvcache_fp8(is_causal=True) sees.

    :param window: a Python int >= 1, a constant of the layer and part of a captured graph.
    :return: [B, H, Sq, D] in query's dtype (and lse [B, H, Sq] fp32).

    Memory contract: flash_attention_n_kvcache_window's. With first_b = 64 * floor(max(0, len_b - qlen_b - window + 1) / 64), cache rows
    j < first_b and the block-table entries of pages wholly below first_b are never read and may hold any byte. Nothing is read on the
    host: the launches - those of flash_attention_n_kvcache_window for the same shapes and window - follow shapes, the capacity and
    `window` only, so a captured graph follows `cache_seqlens`, `query_seqlens` and the scales.
    """
    fn = "flash_attention_n_kvcache_fp8_window"
    _check_window(fn, window)
    _check_query_seqlens(fn, query_seqlens, query)
    _check_group_limit(fn, query, k_cache)
    scales = _fp8_scales(fn, k_scale, v_scale, query, k_cache)
    c = _prepare(fn, "kvprefill", query, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, True,
                 return_lse, query_seqlens=query_seqlens, by_shape=True, fp8=True)
    return _run(c, window=window, fp8_scales=scales)


def flash_attention_n_kvcache_fp8_rope(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        k_scale,
        v_scale,
        rotary_cos: Tensor,
        rotary_sin: Tensor,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        query_seqlens: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        is_causal: bool = True,
        return_lse: bool = False,
        window: Optional[int] = None,
        rotary_interleaved: bool = False):
    """softmax_n attention against an FP8 K/V CACHE with ROTARY POSITION EMBEDDING applied to `query` and `k_new` on the way, on MI355X: one
    step of a Llama / Mistral / GPT-OSS layer over the FP8 cache - rotate, quantise, append, attend - in the launches of
    flash_attention_n_kvcache_fp8 with `k_new`.

    ONE launch rotates row i < qlen_b of k_new[b] at position cache_seqlens[b] + i, rounds it once to query's dtype - the key
    flash_attention_n_kvcache_rope would have stored - quantises THAT value with k_scale as flash_attention_n_kvcache_fp8 quantises k_new, and
    writes the codes to the cache; quantises v_new beside it; and rotates query position i at p_i = i + len_b - qlen_b into a 16-bit
    temporary the forward reads. So a rotated key has one definition across both cache types, and the call equals "rotate `query` and
    `k_new` in eager torch, then flash_attention_n_kvcache_fp8 (or _fp8_window)" bit for bit. Positions, dropped rows, the tables
    (`rotary_cos` / `rotary_sin`, `rotary_interleaved`: layouts, rotary_dim, rows >= capacity, the row clamp) and the rotation's
    arithmetic are flash_attention_n_kvcache_rope's; the cache, the scales and the quantisation flash_attention_n_kvcache_fp8's.

    :param k_new, v_new: optional. Without them only `query` is rotated, at p_i over the cache as it is.
    :param window: None: flash_attention_n_kvcache_fp8's attention; a Python int >= 1: flash_attention_n_kvcache_fp8_window's (needs
                  is_causal=True).
    :return: as flash_attention_n_kvcache_fp8. `query`, `k_new`, `cache_seqlens` are not modified.

    Nothing is read on the host: a captured graph follows `cache_seqlens`, `query_seqlens` and the scales. No ALiBi, no packed queries,
    no gradient; a token tree with rotary embedding is flash_attention_n_kvcache_fp8_tree's.
    """
    fn = "flash_attention_n_kvcache_fp8_rope"
    if window is not None:
        _check_window(fn, window, or_none="None or ")
        if not is_causal:
            raise ValueError(f"{fn}: a sliding window is always causal; window={window} needs is_causal=True")
    _check_rotary_tables(fn, rotary_cos, rotary_sin, query)
    _check_query_seqlens(fn, query_seqlens, query)
    _check_group_limit(fn, query, k_cache)
    _check_rotary_fit(fn, rotary_cos, rotary_sin, query, k_cache, block_table)
    scales = _fp8_scales(fn, k_scale, v_scale, query, k_cache)
    c = _prepare(fn, "kvprefill", query, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, is_causal,
                 return_lse, query_seqlens=query_seqlens, by_shape=True, fp8=True)
    return _run(c, window=window, rope=_rope_operand(rotary_cos, rotary_sin, rotary_interleaved, query), fp8_scales=scales)


def _refuse_fp8_packed(fn, alibi_slopes, tree_mask) -> None:
    """what the packed FP8 calls have no kernels for, named with the call that has"""
    if alibi_slopes is not None:
        raise NotImplementedError(f"{fn}: alibi_slopes is not supported (there are no ALiBi kernels on an FP8 cache or on token-packed "
                                  "queries); flash_attention_n_kvcache_prefill takes alibi_slopes on a 16-bit cache and a padded step")
    if tree_mask is not None:
        raise NotImplementedError(f"{fn}: tree_mask is not supported (there are no token-tree kernels on token-packed queries); "
                                  "flash_attention_n_kvcache_fp8_tree verifies a tree on the FP8 cache, one [B, H, Sq, D] step")


def flash_attention_n_kvcache_fp8_varlen(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        k_scale,
        v_scale,
        cu_seqlens_q: Tensor,
        max_seqlen_q: int,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        is_causal: bool = True,
        return_lse: bool = False,
        alibi_slopes=None,
        tree_mask=None):
    """softmax_n attention of a CONTINUOUS-BATCHING step against an FP8 K/V CACHE, on MI355X: the token-packed buffers of
    flash_attention_n_kvcache_varlen over the cache of flash_attention_n_kvcache_fp8 - the grid follows the tokens AND a key costs one byte.

    The product of the two calls. From flash_attention_n_kvcache_varlen: `query` [T, H, D], `cu_seqlens_q` (int32 [B + 1] on the device,
    never read on the host), `max_seqlen_q`, qlen_b, len_b, visibility, `softmax_n_param`, `scale`, `is_causal`, the outputs ([T, H, D], lse
    [H, T]; rows at or beyond cu[B] are neither read nor written) and the safety under malformed offsets. From
    flash_attention_n_kvcache_fp8: the cache (torch.float8_e4m3fn, D in {64, 128}, strides in multiples of 16 bytes), the value of a code,
    the scales, the quantisation of `k_new` / `v_new` and the stale-memory rules. With power-of-two scales the result is, bit for bit,
    flash_attention_n_kvcache_varlen on `k_cache.to(query.dtype)`. What is particular to the product:

    :param k_scale, v_scale: a Python float, or a floating tensor on the query's device that broadcasts to [B, Hkv] with
                  B = cu_seqlens_q.shape[0] - 1: one scale per SEQUENCE and K/V head, read by the kernels at the token's sequence.
    :param k_new, v_new: optional [T, Hkv, D] in query's dtype, token-packed like `query`: token cu[b] + i is quantised with the scales of
                  (b, hkv) and written to the cache position cache_seqlens[b] + i first, then attended to.
    :param alibi_slopes, tree_mask: anything but None is refused: no kernels.
    :return: [T, H, D] in query's dtype (and lse [H, T] fp32).

    Nothing is read on the host; the launches are those of flash_attention_n_kvcache_varlen for the same shapes, so one captured graph
    serves every step and follows `cu_seqlens_q`, `cache_seqlens` and the scales.
    """
    fn = "flash_attention_n_kvcache_fp8_varlen"
    _refuse_fp8_packed(fn, alibi_slopes, tree_mask)
    _B, _T, q4 = _packed_query(fn, query, k_cache, cache_seqlens, cu_seqlens_q, max_seqlen_q)
    scales = _fp8_scales(fn, k_scale, v_scale, q4, k_cache)
    c = _prepare(fn, "kvvarlen", q4, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, is_causal,
                 return_lse, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q, fp8=True)
    return _run(c, fp8_scales=scales)


def flash_attention_n_kvcache_fp8_varlen_window(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        k_scale,
        v_scale,
        cu_seqlens_q: Tensor,
        max_seqlen_q: int,
        window: int,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        return_lse: bool = False,
        alibi_slopes=None,
        tree_mask=None):
    """softmax_n attention of a SLIDING-WINDOW layer on a CONTINUOUS-BATCHING step against an FP8 K/V CACHE, on MI355X:
    flash_attention_n_kvcache_varlen_window's visibility and per-sequence memory contract over flash_attention_n_kvcache_fp8_varlen's
    buffers and cache.

    Always causal: token cu[b] + i sees key j iff j < len_b and p_i - window < j <= p_i, p_i = i + len_b - qlen_b. Everything else is
    flash_attention_n_kvcache_fp8_varlen's. With power-of-two scales the result is, bit for bit, flash_attention_n_kvcache_varlen_window on
    `k_cache.to(query.dtype)`.

    :param window: a Python int >= 1, a constant of the layer and part of a captured graph.

    Memory contract, per sequence: with first_b = 64 * floor(max(0, len_b - qlen_b - window + 1) / 64), cache rows j < first_b and the
    block-table entries of pages wholly below first_b are never read and may hold any byte. The launches are those of
    flash_attention_n_kvcache_varlen_window for the same shapes and window.
    """
    fn = "flash_attention_n_kvcache_fp8_varlen_window"
    _refuse_fp8_packed(fn, alibi_slopes, tree_mask)
    _check_window(fn, window)
    _B, _T, q4 = _packed_query(fn, query, k_cache, cache_seqlens, cu_seqlens_q, max_seqlen_q)
    scales = _fp8_scales(fn, k_scale, v_scale, q4, k_cache)
    c = _prepare(fn, "kvvarlen", q4, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, True,
                 return_lse, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q, fp8=True)
    return _run(c, window=window, fp8_scales=scales)


def flash_attention_n_kvcache_fp8_varlen_rope(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        k_scale,
        v_scale,
        cu_seqlens_q: Tensor,
        max_seqlen_q: int,
        rotary_cos: Tensor,
        rotary_sin: Tensor,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        is_causal: bool = True,
        return_lse: bool = False,
        window: Optional[int] = None,
        rotary_interleaved: bool = False,
        alibi_slopes=None,
        tree_mask=None):
    """softmax_n attention of a CONTINUOUS-BATCHING step against an FP8 K/V CACHE with ROTARY POSITION EMBEDDING applied to `query` and
    `k_new` on the way, on MI355X: one layer step of a served Llama / Mistral / GPT-OSS over the FP8 cache - rotate, quantise, append,
    attend - on token-packed buffers.

    ONE launch rotates token cu[b] + i of k_new at position cache_seqlens[b] + i, rounds it once to query's dtype - the key
    flash_attention_n_kvcache_varlen_rope would have stored - quantises THAT value with k_scale[b, hkv] and writes the codes; quantises
    v_new beside it; and rotates the query token at p_i into a [T, H, D] temporary the forward reads. The call equals "rotate `query`
    and `k_new` in eager torch, then flash_attention_n_kvcache_fp8_varlen (or _varlen_window)" bit for bit. The tables, layouts and the
    rotation's arithmetic are flash_attention_n_kvcache_rope's; tokens, offsets and outputs flash_attention_n_kvcache_fp8_varlen's.

    :param k_new, v_new: optional [T, Hkv, D]. Without them only `query` is rotated, at p_i over the cache as it is.
    :param window: None: flash_attention_n_kvcache_fp8_varlen's attention; a Python int >= 1: flash_attention_n_kvcache_fp8_varlen_window's
                  (needs is_causal=True).
    :return: [T, H, D] (and lse [H, T]). `query`, `k_new`, `cache_seqlens` are not modified.
    """
    fn = "flash_attention_n_kvcache_fp8_varlen_rope"
    _refuse_fp8_packed(fn, alibi_slopes, tree_mask)
    if window is not None:
        _check_window(fn, window, or_none="None or ")
        if not is_causal:
            raise ValueError(f"{fn}: a sliding window is always causal; window={window} needs is_causal=True")
    _B, _T, q4 = _packed_query(fn, query, k_cache, cache_seqlens, cu_seqlens_q, max_seqlen_q)
    _check_rotary_tables(fn, rotary_cos, rotary_sin, query)
    _check_rotary_fit(fn, rotary_cos, rotary_sin, q4, k_cache, block_table)
    scales = _fp8_scales(fn, k_scale, v_scale, q4, k_cache)
    c = _prepare(fn, "kvvarlen", q4, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, is_causal,
                 return_lse, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q, fp8=True)
    return _run(c, window=window, rope=_rope_operand(rotary_cos, rotary_sin, rotary_interleaved, query), fp8_scales=scales)


def _check_tree_mask(fn, tree_mask, query) -> Tensor:
    """tree_mask as the kernels read it: int64 [B, Sq] on the query's device with unit node stride (a small per-step tensor: made contiguous
    when it is not). The values are not looked at: any word is legal."""
    if not isinstance(tree_mask, Tensor) or tree_mask.dtype != torch.int64:
        got = tree_mask.dtype if isinstance(tree_mask, Tensor) else type(tree_mask).__name__
        raise TypeError(f"{fn}: tree_mask must be an int64 tensor (one 64-bit word per node: bit t of word i says node i sees node t); got {got}")
    if query.dim() == 4:
        B, Sq = query.shape[0], query.shape[2]
        if Sq > _MAX_NODES:
            raise ValueError(f"{fn}: a tree of {Sq} nodes is not supported (at most {_MAX_NODES}: one bit of an int64 word per node); verify a "
                             "larger tree in several calls")
        if tuple(tree_mask.shape) != (B, Sq):
            raise ValueError(f"{fn}: tree_mask must be [B, Sq] = [{B}, {Sq}], one word per node of query; got {tuple(tree_mask.shape)}")
    if tree_mask.device != query.device:
        raise RuntimeError(f"tree_mask is on {tree_mask.device}, query on {query.device}: every operand must live on the query's device "
                           "(the words are read by the kernels, never on the host)")
    return tree_mask if tree_mask.stride(-1) == 1 and tree_mask.stride(0) >= 0 else tree_mask.contiguous()


def flash_attention_n_kvcache_tree(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        tree_mask: Tensor,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        query_seqlens: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        return_lse: bool = False,
        window: Optional[int] = None,
        rotary_cos: Optional[Tensor] = None,
        rotary_sin: Optional[Tensor] = None,
        rotary_interleaved: bool = False):
    """softmax_n attention of a TREE of draft tokens against a K/V cache, on MI355X: the verification step of speculative decoding
    (EAGLE, Medusa, SpecInfer). The Sq new positions are the nodes of the tree, in any order in which a node follows its ancestors; every
    node sees the cached prefix and the nodes its mask word names - its ancestors and itself - never its siblings.

    With qlen_b = clamp(query_seqlens[b], 0, Sq) (None: Sq), len_b = clamp(cache_seqlens[b] + (qlen_b if k_new is given else 0), 0,
    capacity) and base_b = len_b - qlen_b, node i sits in cache row base_b + i and sees key j iff
        j < base_b                       (the prefix; under `window` also j > p_i - window), or
        j = base_b + t, t < qlen_b, and bit t of tree_mask[b, i] is set.
    Its position is p_i = base_b + d_i with the depth d_i = max(popcount(tree_mask[b, i] & the low qlen_b bits) - 1, 0): a well-formed row
    holds the node itself and exactly its ancestors, so no position tensor exists. The cache, `block_table`, `cache_seqlens`, `k_new` /
    `v_new`, `query_seqlens`, `softmax_n_param`, `scale`, dtypes, head dims, alignment rules and refusals are those of
    flash_attention_n_kvcache_prefill; the kernels are chosen by shapes alone as in flash_attention_n_kvcache_window (query_seqlens=None and
    (H // Hkv) * Sq <= 128: the decode kernels). What differs:

    :param query: [B, H, Sq, D] with Sq <= 64.
    :param tree_mask: int64 [B, Sq] ON THE DEVICE. Bits t >= qlen_b are ignored; bit 63 - the sign bit - is an ordinary bit. The words may
                  hold anything: upper-triangular bits, a missing self bit and an all-zero row are legal, the result is what the rule
                  above says and no memory access depends on the mask. The chain (bit t iff t <= i) is causal attention, bit for bit.
    :param window: None, or a Python int >= 1: the prefix keys are those of flash_attention_n_kvcache_window at position p_i. With
                  first_b = 64 * floor(max(0, base_b - window + 1) / 64), cache rows below first_b and the block-table entries of pages
                  wholly below it are never read (that call's memory contract).
    :param rotary_cos, rotary_sin, rotary_interleaved: both tables or neither, as in flash_attention_n_kvcache_rope. Node i of k_new is
                  written to cache row cache_seqlens[b] + i but rotated at cache_seqlens[b] + d_i; the query node is rotated at p_i.
    :return: [B, H, Sq, D] in query's dtype (and lse [B, H, Sq] fp32). A node that sees nothing gives exactly 0 and lse = log n (-inf for
             n = 0); padding positions i >= qlen_b give exactly 0 and lse = -inf and are neither read nor rotated.

    After acceptance flash_attention_n_kvcache_tree_commit moves the accepted path's rows behind the prefix; `cache_seqlens` stays the
    caller's to advance. Nothing is read on the host: the launches depend on shapes, the capacity and `window` only, so one captured graph
    serves every step while `tree_mask`, `cache_seqlens` and the cache change in place. Always causal; no ALiBi, no packed queries, no
    gradient."""
    fn = "flash_attention_n_kvcache_tree"
    if window is not None:
        _check_window(fn, window, or_none="None or ")
    tree_mask = _check_tree_mask(fn, tree_mask, query)
    if (rotary_cos is None) != (rotary_sin is None):
        raise ValueError(f"{fn}: rotary_cos and rotary_sin come together (both tables, or neither)")
    rotary = rotary_cos is not None
    if rotary:
        _check_rotary_tables(fn, rotary_cos, rotary_sin, query)
    _check_query_seqlens(fn, query_seqlens, query)
    _check_group_limit(fn, query, k_cache)
    if rotary:
        _check_rotary_fit(fn, rotary_cos, rotary_sin, query, k_cache, block_table)
    c = _prepare(fn, "kvprefill", query, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, True,
                 return_lse, query_seqlens=query_seqlens, by_shape=True)
    return _run(c, window=window, rope=_rope_operand(rotary_cos, rotary_sin, rotary_interleaved, query) if rotary else None, tree_mask=tree_mask)


def flash_attention_n_kvcache_tree_commit(
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        accepted: Tensor,
        accepted_lens: Tensor,
        block_table: Optional[Tensor] = None) -> None:
    """Compaction after acceptance, on MI355X: the K and V rows of the accepted root-to-leaf path of a verified tree move behind the prefix,
    in place, through the block table.

    :param k_cache, v_cache, block_table: the cache of the tree call.
    :param cache_seqlens: int32 [B] ON THE DEVICE: base_b, the prefix length - the value that was passed to the tree call. Not modified:
                  the caller advances it by the accepted length.
    :param accepted: int32 [B, A] on the device, A <= 64: accepted[b, k] is the node (its index in the tree call's `query`) at depth k of
                  the path. A path is strictly increasing, so accepted[b, k] >= k.
    :param accepted_lens: int32 [B] on the device: alen_b = clamp(accepted_lens[b], 0, A) nodes of the path count.

    For k < alen_b row base_b + accepted[b, k] is copied to row base_b + k. An index outside [k, 64), or a row at or beyond the capacity,
    skips that move: a malformed path gives unspecified rows and never touches memory outside the cache; accepted[b, k] == k moves nothing.
    Rotated keys need no re-rotation: node k of a path has depth k and lands at the position it was rotated for. Nothing is read on the
    host: the launch depends on shapes only and replays in a captured graph."""
    _commit("flash_attention_n_kvcache_tree_commit", False, k_cache, v_cache, cache_seqlens, accepted, accepted_lens, block_table)


def flash_attention_n_kvcache_fp8_tree(
        query: Tensor,
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        k_scale,
        v_scale,
        tree_mask: Tensor,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        v_new: Optional[Tensor] = None,
        query_seqlens: Optional[Tensor] = None,
        softmax_n_param=1,
        scale: Optional[float] = None,
        return_lse: bool = False,
        window: Optional[int] = None,
        rotary_cos: Optional[Tensor] = None,
        rotary_sin: Optional[Tensor] = None,
        rotary_interleaved: bool = False):
    """softmax_n attention of a TREE of draft tokens against an FP8 K/V CACHE, on MI355X: the verification step of speculative decoding
    (EAGLE, Medusa, SpecInfer) over flash_attention_n_kvcache_fp8's cache, without dequantising it.

    Visibility, the nodes' rows and positions (base_b, the depth from the popcount of the mask word), `tree_mask`, `window` and its memory
    contract, rotary embedding at depth positions, `query_seqlens`, padding rows and the choice of kernels by shapes alone are
    flash_attention_n_kvcache_tree's; the cache, `k_scale` / `v_scale`, the values, the quantisation of `k_new` / `v_new`, the caches' rules
    and the refusals are flash_attention_n_kvcache_fp8's. With power-of-two scales the result is, bit for bit,
    flash_attention_n_kvcache_tree on `k_cache.to(query.dtype)`; the chain mask is flash_attention_n_kvcache_fp8(is_causal=True) (with a
    window: flash_attention_n_kvcache_fp8_window), bit for bit.

    :param query: [B, H, Sq, D] fp16 / bf16 with Sq <= 64, D in {64, 128}.
    :param k_new, v_new: optional [B, Hkv, Sq, D]: node i < qlen_b is quantised and written to cache row cache_seqlens[b] + i, then attended
                  to as the mask says.
    :param rotary_cos, rotary_sin, rotary_interleaved: both tables or neither. ONE launch rotates node i of k_new at cache_seqlens[b] + d_i,
                  rounds it once to query's dtype, quantises that value with k_scale and writes the codes to row cache_seqlens[b] + i;
                  quantises v_new beside it; and rotates the query node at p_i. The call equals "rotate `query` and `k_new` at the depth
                  positions in eager torch, then this call without tables" bit for bit.
    :return: [B, H, Sq, D] in query's dtype (and lse [B, H, Sq] fp32), as flash_attention_n_kvcache_tree.

    After acceptance flash_attention_n_kvcache_fp8_tree_commit moves the accepted path's code rows behind the prefix. Nothing is read on
    the host: the launches - those of flash_attention_n_kvcache_tree for the same shapes and window - follow shapes, the capacity and
    `window` only, so one captured graph serves every step while `tree_mask`, `cache_seqlens`, the scales and the cache change in place.
    Always causal; no ALiBi, no packed queries, no gradient."""
    fn = "flash_attention_n_kvcache_fp8_tree"
    if window is not None:
        _check_window(fn, window, or_none="None or ")
    tree_mask = _check_tree_mask(fn, tree_mask, query)
    if (rotary_cos is None) != (rotary_sin is None):
        raise ValueError(f"{fn}: rotary_cos and rotary_sin come together (both tables, or neither)")
    rotary = rotary_cos is not None
    if rotary:
        _check_rotary_tables(fn, rotary_cos, rotary_sin, query)
    _check_query_seqlens(fn, query_seqlens, query)
    _check_group_limit(fn, query, k_cache)
    if rotary:
        _check_rotary_fit(fn, rotary_cos, rotary_sin, query, k_cache, block_table)
    scales = _fp8_scales(fn, k_scale, v_scale, query, k_cache)
    c = _prepare(fn, "kvprefill", query, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, softmax_n_param, scale, True,
                 return_lse, query_seqlens=query_seqlens, by_shape=True, fp8=True)
    return _run(c, window=window, rope=_rope_operand(rotary_cos, rotary_sin, rotary_interleaved, query) if rotary else None, tree_mask=tree_mask,
                fp8_scales=scales)


def flash_attention_n_kvcache_fp8_tree_commit(
        k_cache: Tensor,
        v_cache: Tensor,
        cache_seqlens: Tensor,
        accepted: Tensor,
        accepted_lens: Tensor,
        block_table: Optional[Tensor] = None) -> None:
    """flash_attention_n_kvcache_tree_commit on an FP8 K/V CACHE, on MI355X: the code rows of the accepted path of a tree verified by
    flash_attention_n_kvcache_fp8_tree move behind the prefix, in place, through the block table. The scales are per (batch element, K/V
    head), so a moved code keeps its value.

    :param k_cache, v_cache: torch.float8_e4m3fn, D in {64, 128}, under the alignment rules of flash_attention_n_kvcache_fp8 (strides in
                  multiples of 16 codes).
    Every other parameter, the moves, the skip rules for a malformed path and the checks are flash_attention_n_kvcache_tree_commit's.
    `cache_seqlens` is not modified. Nothing is read on the host: the launch depends on shapes only and replays in a captured graph."""
    _commit("flash_attention_n_kvcache_fp8_tree_commit", True, k_cache, v_cache, cache_seqlens, accepted, accepted_lens, block_table)


def _commit(fn, fp8, k_cache, v_cache, cache_seqlens, accepted, accepted_lens, block_table) -> None:
    """the checks, the block and the one launch of both commits; `fp8`: the caches hold e4m3fn codes and the strides count them"""
    if k_cache.dim() != 4 or v_cache.dim() != 4:
        raise ValueError(f"{fn}: the caches must be [num_pages, page_size, Hkv, D] (paged) or [B, capacity, Hkv, D] (dense)")
    if fp8:
        if k_cache.dtype != torch.float8_e4m3fn or v_cache.dtype != torch.float8_e4m3fn:
            raise TypeError(f"{fn}: k_cache and v_cache must be torch.float8_e4m3fn (OCP e4m3fn codes; e5m2 and fnuz caches are not supported); "
                            f"got {k_cache.dtype} and {v_cache.dtype}. A 16-bit cache is flash_attention_n_kvcache_tree_commit's")
    elif k_cache.dtype not in _KV_DTYPES or v_cache.dtype != k_cache.dtype:
        raise TypeError(f"{fn}: k_cache and v_cache must share one dtype, fp16 or bf16; got {k_cache.dtype} and {v_cache.dtype}"
                        + (". An FP8 cache is flash_attention_n_kvcache_fp8_tree_commit's" if k_cache.dtype == torch.float8_e4m3fn else ""))
    dev = k_cache.device
    tensors = {"v_cache": v_cache, "cache_seqlens": cache_seqlens, "accepted": accepted, "accepted_lens": accepted_lens, "block_table": block_table}
    for name, t in tensors.items():
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name} is on {t.device}, k_cache on {dev}: every operand must live on the cache's device "
                               "(the path and the lengths are read by the kernel, never on the host)")
    if k_cache.shape != v_cache.shape:
        raise ValueError(f"k_cache and v_cache must have one shape; got {tuple(k_cache.shape)} and {tuple(v_cache.shape)}")
    page_size, Hkv, D = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    if D not in _KV_HEAD_DIMS:
        raise ValueError(f"{fn}: head dim {D} is not supported (supported: {_KV_HEAD_DIMS})")
    if fp8 and D not in _FP8_HEAD_DIMS:
        raise ValueError(f"{fn}: head dim {D} is not supported on an FP8 cache (supported: {_FP8_HEAD_DIMS}; 32 and 256 have 16-bit kernels only)")
    if cache_seqlens.dtype != torch.int32 or cache_seqlens.dim() != 1 or not cache_seqlens.is_contiguous():
        raise ValueError(f"cache_seqlens must be a contiguous int32 tensor of shape [B] on the device; got {cache_seqlens.dtype} {tuple(cache_seqlens.shape)}")
    B = cache_seqlens.shape[0]
    if accepted.dtype != torch.int32 or accepted.dim() != 2 or accepted.shape[0] != B or accepted.shape[1] < 1:
        raise ValueError(f"{fn}: accepted must be an int32 tensor [B, A] = [{B}, A >= 1] of node indices; got {accepted.dtype} {tuple(accepted.shape)}")
    A = accepted.shape[1]
    if A > _MAX_NODES:
        raise ValueError(f"{fn}: accepted is {A} nodes wide; a path has at most {_MAX_NODES} (the nodes of a tree)")
    if accepted_lens.dtype != torch.int32 or accepted_lens.dim() != 1 or accepted_lens.shape[0] != B or not accepted_lens.is_contiguous():
        raise ValueError(f"{fn}: accepted_lens must be a contiguous int32 tensor of shape [{B}]; got {accepted_lens.dtype} {tuple(accepted_lens.shape)}")
    paged = block_table is not None
    if paged:
        if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.stride(1) != 1:
            raise ValueError(f"block_table must be an int32 tensor [B, max_pages] with unit column stride; got {block_table.dtype} {tuple(block_table.shape)}")
        if block_table.shape[0] != B or block_table.shape[1] < 1:
            raise ValueError(f"block_table must be [{B}, max_pages >= 1]: one row of page ids per batch element; got {tuple(block_table.shape)}")
        if page_size % 64 != 0:
            raise ValueError(f"page_size {page_size} is not supported: a paged cache needs page_size % 64 == 0 (a 64-key tile never straddles a page)")
    elif k_cache.shape[0] != B:
        raise ValueError(f"dense cache (block_table=None) must be [B, capacity, Hkv, D] with B = {B}; got {tuple(k_cache.shape)}")
    _check_cache("k_cache", k_cache, paged, D)
    _check_cache("v_cache", v_cache, paged, D)
    if accepted.stride(1) != 1 or accepted.stride(0) < A:
        accepted = accepted.contiguous()
    if not k_cache.is_cuda:
        raise RuntimeError("flash_attention_softmax_n_amd runs on MI355X device tensors only; got a CPU tensor "
                           "(there is deliberately no CPU fallback)")
    a = KvTreeCommit()
    a.k_cache, a.v_cache = k_cache.data_ptr(), v_cache.data_ptr()
    for i in range(3):
        a.k_stride[i] = k_cache.stride(i) if k_cache.size(i) > 1 else 0
        a.v_stride[i] = v_cache.stride(i) if v_cache.size(i) > 1 else 0
    if k_cache.size(1) == 1:
        a.k_stride[1] = a.v_stride[1] = D
    if paged:
        a.block_table, a.block_table_stride, a.max_pages = block_table.data_ptr(), block_table.stride(0) if B > 1 else block_table.shape[1], block_table.shape[1]
    else:
        a.block_table, a.block_table_stride, a.max_pages = None, 0, 1
    a.page_size, a.seqlens = page_size, cache_seqlens.data_ptr()
    a.B, a.Hkv, a.D, a.A = B, Hkv, D, A
    a.accepted, a.accepted_stride, a.accepted_lens = accepted.data_ptr(), accepted.stride(0) if B > 1 else A, accepted_lens.data_ptr()
    a.nodes, a.reserved = _MAX_NODES, 0
    lib = _lib.load()
    entry = "fasn_kvcache_fp8_tree_commit" if fp8 else "fasn_kvcache_tree_commit"
    _on_device(dev, lambda: _lib.check(getattr(lib, entry)(a, _stream_ptr(dev)), entry))


def _rows(t: Tensor) -> Tensor:
    """query / k_new / v_new: small per-step tensors, made contiguous when their rows are not 16-byte aligned (the cache never is)"""
    ok = t.stride(3) == 1 and t.data_ptr() % 16 == 0 and all(t.stride(i) % 8 == 0 or t.size(i) == 1 for i in range(3))
    return t if ok else t.contiguous()
