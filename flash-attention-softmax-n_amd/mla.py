"""MLA decode: attention over a compressed latent K/V cache (multi-head latent attention in its absorbed form: DeepSeek-V2 / V3 / R1,
Kimi K2). Host side of fasn_fwd_mla / fasn_mla_append, of fasn_fwd_mla_fp8 / fasn_mla_fp8_append, of fasn_fwd_mla_sparse and of
fasn_fwd_mla_sparse_fp8 / fasn_mla_sparse_fp8_append in include/fasn.h: one call path, with the scale of an FP8 latent cache, the top-k
index list of the sparse decode (DeepSeek-V3.2) and the 656-byte FP8 row behind such a list as optional operands. Beside it
flash_attention_n_mla_index, the indexer that builds such a list (fasn_mla_index / fasn_mla_index_append): a call path of its own.

The cache holds ONE row of 576 features per token, shared by every query head: a 512-wide latent and a 64-wide rotated key part. The logit
of head h is q_h[0:576] . row[0:576] and the value is the latent itself, out_h = sum_j p_hj row_j[0:512] - so K and V are one tensor, read
once. The call sits beside the K/V-cache family (kvcache.py) and shares its contract: lengths and block table are read by the kernels only,
the launches depend on shapes and capacity alone, one captured graph serves every step. Forward only.
"""
from typing import Callable, NamedTuple, Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import MlaArgs, MlaFp8, MlaIndexArgs, MlaSparse
from .flash_attn import _n_strides, _n_tensor, _stream_ptr, _view4
from .kvcache import _KV_DTYPES, _check_cache, _on_device, _rows, _scale_tensor

MLA_HEAD_DIM, MLA_VALUE_DIM, MLA_MAX_ROWS = 576, 512, 256
MLA_FP8_ROW_BYTES, MLA_FP8_GROUP = 656, 128   # the FP8 row behind an index list: 512 codes, 4 fp32 scales (one per 128 features), 64 x 16-bit rope
_FP8_E_MIN, _FP8_E_MAX = -30, 120             # the exponents a group's scale 2^e takes (csrc/fasn_mla_sparse_fp8.h)
_LOG2E = 1.4426950408889634
_F16_MAX_PRESCALE = 8.0   # float16: |scale * log2e| beyond this is FASN_EUNSUPPORTED (mla_build, csrc/fasn_mla.hip)
_SERVED = (f"served: a latent cache of head dims exactly {MLA_VALUE_DIM} + 64 = {MLA_HEAD_DIM} in fp16 / bf16 (flash_attention_n_mla) or in "
           f"e4m3fn codes with kv_scale (flash_attention_n_mla_fp8), H * Sq <= {MLA_MAX_ROWS}, causal or not, softmax_n; behind a top-k list "
           "of logical positions: the fp16 / bf16 cache (flash_attention_n_mla_sparse) or 656-byte FP8 rows - 512 e4m3fn codes, four "
           "fp32 scales, 64 16-bit rotated features - as uint8 / float8_e4m3fn bytes (flash_attention_n_mla_sparse_fp8), int32 indices "
           "[B, Sq, topk] on the device with topk a multiple of 64; not served: e5m2 and the fnuz codes, a window, ALiBi, trees, packed "
           f"queries, shared prefixes, the 656-byte rows without indices, physical (pool) indices, more than {MLA_MAX_ROWS} rows, gradients")
_FP8_DTYPES = (torch.float8_e4m3fn, torch.float8_e5m2, torch.float8_e4m3fnuz, torch.float8_e5m2fnuz)
_BYTE_DTYPES = (torch.uint8, torch.float8_e4m3fn)   # what a cache of 656-byte rows may be declared as: both mean bytes


def flash_attention_n_mla(
        query: Tensor,
        kv_cache: Tensor,
        cache_seqlens: Tensor,
        scale: float,
        block_table: Optional[Tensor] = None,
        kv_new: Optional[Tensor] = None,
        softmax_n_param=1,
        is_causal: bool = True,
        return_lse: bool = False):
    """softmax_n attention of a few new query positions against a compressed latent K/V cache (absorbed MLA decode), on MI355X.

    :param query: [B, H, Sq, 576] fp16 / bf16 device tensor: W_UK is absorbed into the first 512 features, the last 64 are rotated.
                  H * Sq <= 256 (DeepSeek-V3's 128 heads with one MTP draft position).
    :param kv_cache: paged [num_pages, page_size, 1, 576] with `block_table` (page_size a multiple of 64), or dense [B, capacity, 1, 576]
                  with block_table=None; a 3-D cache without the head axis is a view of the same thing. Query's dtype, feature stride 1,
                  16-byte aligned rows; never copied.
    :param cache_seqlens: int32 [B] ON THE DEVICE: valid rows per batch element before this call; clamped to [0, capacity] in the kernel,
                  never read on the host, not modified.
    :param scale: multiplies q . row. REQUIRED: an MLA model's scale is (128 + 64) ** -0.5 times its YaRN factor, not 576 ** -0.5, so there
                  is no default. float16 serves |scale| * log2(e) <= 8 (the queries are prescaled in the element type).
    :param block_table: int32 [B, max_pages] on the device. Entries beyond the pages a batch element needs are never read; cache rows at
                  or beyond its length may hold anything (NaN included).
    :param kv_new: optional [B, Sq, 1, 576]: written to the cache positions cache_seqlens[b] .. + Sq - 1 first (positions at or beyond
                  the capacity are dropped in the kernel) and then attended to: batch element b sees len_b = cache_seqlens[b] + Sq rows.
    :param softmax_n_param: n >= 0, or a floating tensor that broadcasts to [B, H]; no gradient. n = 0 is the models as they ship.
    :param is_causal: position i sees key j iff j < len_b and j <= i + len_b - Sq. False: every position sees all len_b keys.
    :param return_lse: also return lse [B, H, Sq] fp32 = log(n + sum_j exp(x_ij)).
    :return: [B, H, Sq, 512] in query's dtype (and lse). Rows that see no key give exactly 0 and lse = log n (-inf for n = 0).
    """
    return _mla(_MLA, query, kv_cache, cache_seqlens, scale, None, block_table, kv_new, softmax_n_param, is_causal, return_lse)


def flash_attention_n_mla_fp8(
        query: Tensor,
        kv_cache: Tensor,
        cache_seqlens: Tensor,
        scale: float,
        kv_scale,
        block_table: Optional[Tensor] = None,
        kv_new: Optional[Tensor] = None,
        softmax_n_param=1,
        is_causal: bool = True,
        return_lse: bool = False):
    """flash_attention_n_mla over a latent cache of FP8 codes: 576 bytes per token instead of 1152. Everything flash_attention_n_mla says
    of shapes, lengths, the block table, stale rows, `scale`, softmax_n, causality and lse holds here; what differs:

    :param query: fp16 / bf16, which is also the dtype of the output and of `kv_new`. Neither the queries nor the weights are quantised.
    :param kv_cache: torch.float8_e4m3fn (OCP e4m3fn codes), paged [num_pages, page_size, 1, 576] or dense [B, capacity, 1, 576] (or 3-D);
                  feature stride 1, row and page strides multiples of 16 bytes, base 16-byte aligned; never copied.
    :param kv_scale: the value of a code is up(code) * kv_scale[b]: a Python float (becomes a one-element device tensor), or a floating
                  tensor that broadcasts to [B] ([B], [B, 1], [1] or 0-d) ON THE DEVICE - read by the kernels only, so a captured graph
                  follows its values. It multiplies the fp32 scores (with `scale`) and the fp32 output before its one rounding. One scale
                  serves the whole row: a model whose rotated 64 features want another scale folds the ratio into the queries' last 64
                  features. A non-positive or non-finite scale gives unspecified values.
    :param kv_new: optional [B, Sq, 1, 576] in query's dtype: quantised as flash_attention_n_kvcache quantises k_new for an FP8 cache -
                  code = rne_e4m3(clamp(float(x) / kv_scale[b], -448, 448)), NaN to a NaN code - written behind the lengths, then seen.
    """
    return _mla(_MLA_FP8, query, kv_cache, cache_seqlens, scale, kv_scale, block_table, kv_new, softmax_n_param, is_causal, return_lse)


def flash_attention_n_mla_sparse(
        query: Tensor,
        kv_cache: Tensor,
        indices: Tensor,
        cache_seqlens: Tensor,
        scale: float,
        block_table: Optional[Tensor] = None,
        kv_new: Optional[Tensor] = None,
        softmax_n_param=1,
        is_causal: bool = True,
        return_lse: bool = False):
    """flash_attention_n_mla over the cache rows that a top-k index list names (DeepSeek-V3.2's sparse attention: an indexer selects a
    fixed budget of tokens per query position, the attention gathers their latent rows). Everything flash_attention_n_mla says of
    `query` (H * Sq <= 256), the paged / dense / 3-D fp16 / bf16 cache, `cache_seqlens`, `block_table`, `scale`, `kv_new` (appended first,
    then nameable), softmax_n, lse and the 512-wide output holds here; what differs:

    :param indices: int32 [B, Sq, topk] ON THE DEVICE, last stride 1, topk a multiple of 64 (the call does not pad: a pad is a copy and
                  a launch). Entry e of (b, i) names the LOGICAL position j = indices[b, i, e] of batch element b - the kernel
                  translates it through the block table - and every head of position i shares the list. j is a key of position i iff
                  0 <= j < len_b and, when is_causal, j <= i + len_b - Sq, with len_b = clamp(cache_seqlens[b] + (Sq if kv_new else 0),
                  0, capacity). Every other value - -1 padding, positions at or beyond the length, causally hidden ones, garbage - is no
                  key: it contributes nothing, and neither its block-table slot nor its cache row is read. A position named twice counts
                  twice. Read by the kernels only: the launches depend on shapes, topk and capacity alone, so one captured graph
                  serves every step.
    :return: [B, H, Sq, 512] in query's dtype (and lse). Rows without a key give exactly 0 and lse = log n.
    """
    return _mla(_MLA_SPARSE, query, kv_cache, cache_seqlens, scale, indices, block_table, kv_new, softmax_n_param, is_causal, return_lse)


def flash_attention_n_mla_sparse_fp8(
        query: Tensor,
        kv_cache: Tensor,
        indices: Tensor,
        cache_seqlens: Tensor,
        scale: float,
        block_table: Optional[Tensor] = None,
        kv_new: Optional[Tensor] = None,
        softmax_n_param=1,
        is_causal: bool = True,
        return_lse: bool = False):
    """flash_attention_n_mla_sparse over the FP8 latent cache the top-k models are served from. Everything flash_attention_n_mla_sparse
    says of `query` (H * Sq <= 256), `indices` (logical positions, topk % 64 == 0, no address formed from an entry that is no key, a
    duplicate counts twice), `cache_seqlens`, `block_table`, `scale` (float16: |scale| * log2(e) <= 8), softmax_n, causality, lse and the
    512-wide output holds here; what differs:

    :param kv_cache: torch.uint8 or torch.float8_e4m3fn (both mean bytes), paged [num_pages, page_size, 1, 656] with `block_table`
                  (page_size a multiple of 64), dense [B, capacity, 1, 656], or 3-D without the head axis; last stride 1, row and page
                  strides multiples of 16 bytes, base 16-byte aligned; never copied. A row is 512 OCP e4m3fn codes of the latent, four
                  fp32 scales (scale g for features 128 g .. 128 g + 127) and the 64 rotated features as 16-bit numbers IN QUERY'S DTYPE,
                  not quantised (mla_fp8_rows_pack writes it, mla_fp8_rows_unpack reads it). Latent feature f of a row is
                  (float32(code[f]) * scale[f // 128]) rounded once to query's dtype - dequantise to 16 bits, then attend - so the call
                  gives, bit for bit, flash_attention_n_mla_sparse on mla_fp8_rows_unpack(kv_cache, query.dtype). There is no kv_scale
                  operand and no factor on scores or output. Scales that are not finite and positive give unspecified values.
    :param kv_new: optional [B, Sq, 1, 576] in query's dtype: quantised by the rule of mla_fp8_rows_pack, byte for byte, into the rows
                  cache_seqlens[b] .. + Sq - 1 (positions at or beyond the capacity are dropped in the kernel), then nameable.
    :return: [B, H, Sq, 512] in query's dtype (and lse). Rows without a key give exactly 0 and lse = log n.
    """
    return _mla(_MLA_SPARSE_FP8, query, kv_cache, cache_seqlens, scale, indices, block_table, kv_new, softmax_n_param, is_causal, return_lse)


def _fp8_group_exponent(amax: Tensor) -> Tensor:
    """int32 e per group from its fp32 amax >= 0: the smallest e with amax <= 448 * 2^e = 1.75 * 2^(e + 8), clamped to [-30, 120], read
    from the exponent and mantissa bits as the append kernel reads it (amax = m * 2^E, 1 <= m < 2: e = E - 8, one more where m > 1.75;
    zero and fp32's subnormals fall to the lower clamp)"""
    bits = amax.contiguous().view(torch.int32)
    e = (bits >> 23) - 127 - 8 + ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)
    return e.clamp(_FP8_E_MIN, _FP8_E_MAX)


def mla_fp8_rows_pack(kv16: Tensor) -> Tensor:
    """[..., 576] fp16 / bf16 latent rows -> uint8 [..., 656] rows of flash_attention_n_mla_sparse_fp8's cache (plain torch, any device),
    by the rule its kv_new append follows byte for byte. Per row and group g of 128 latent features: a = max |x| over the finite
    elements in fp32, scale = 2^e with e the smallest integer such that a <= 448 * 2^e, clamped to [-30, 120] (a = 0: e = -30),
    code = rne_e4m3(clamp(x / scale, -448, 448)) - the division is exact, +-Inf clamps, NaN gives the NaN code 0x7f. The 64 rotated features
    are copied bit for bit: the row's rope part has kv16's dtype."""
    if not isinstance(kv16, Tensor) or kv16.dtype not in _KV_DTYPES or kv16.shape[-1] != MLA_HEAD_DIM:
        raise ValueError(f"mla_fp8_rows_pack: rows must be [..., {MLA_HEAD_DIM}] in fp16 / bf16")
    lead = kv16.shape[:-1]
    x = kv16[..., :MLA_VALUE_DIM].float().reshape(*lead, MLA_VALUE_DIM // MLA_FP8_GROUP, MLA_FP8_GROUP)
    amax = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).amax(-1)
    s = ((_fp8_group_exponent(amax) + 127) << 23).view(torch.float32)
    codes = (x / s[..., None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    codes = torch.where(torch.isnan(x), torch.full_like(codes, 0x7F), codes).reshape(*lead, MLA_VALUE_DIM)   # one NaN code, whatever the sign
    rope = kv16[..., MLA_VALUE_DIM:].contiguous().view(torch.uint8).reshape(*lead, 2 * (MLA_HEAD_DIM - MLA_VALUE_DIM))
    return torch.cat([codes, s.contiguous().view(torch.uint8).reshape(*lead, 16), rope], -1)


def mla_fp8_rows_unpack(rows656: Tensor, dtype: torch.dtype) -> Tensor:
    """uint8 / float8_e4m3fn [..., 656] rows -> [..., 576] in `dtype` (fp16 / bf16; plain torch, any device): the 16-bit rows
    flash_attention_n_mla_sparse_fp8 attends to - latent feature f = (float32(code[f]) * scale[f // 128]).to(dtype), the rope part
    reinterpreted as `dtype`."""
    if not isinstance(rows656, Tensor) or rows656.dtype not in _BYTE_DTYPES or rows656.shape[-1] != MLA_FP8_ROW_BYTES or dtype not in _KV_DTYPES:
        raise ValueError(f"mla_fp8_rows_unpack: rows must be uint8 / float8_e4m3fn [..., {MLA_FP8_ROW_BYTES}] and dtype fp16 / bf16")
    raw = rows656.view(torch.uint8).contiguous()
    lead = raw.shape[:-1]
    codes = raw[..., :MLA_VALUE_DIM].contiguous().view(torch.float8_e4m3fn).float().reshape(*lead, MLA_VALUE_DIM // MLA_FP8_GROUP, MLA_FP8_GROUP)
    s = raw[..., MLA_VALUE_DIM:MLA_VALUE_DIM + 16].contiguous().view(torch.float32)
    rope = raw[..., MLA_VALUE_DIM + 16:].contiguous().view(dtype)
    return torch.cat([(codes * s[..., None]).to(dtype).reshape(*lead, MLA_VALUE_DIM), rope], -1)


def _scale_operand(fn, kv_scale, query):
    if isinstance(kv_scale, Tensor) and kv_scale.dim() == 1:   # the one K/V head has no axis here: a 1-D scale is [B]
        kv_scale = kv_scale[:, None]
    ks = _scale_tensor(fn, "kv_scale", kv_scale, query, 1)   # [1 or B, 1] fp32
    f8 = MlaFp8()
    f8.kv_scale, f8.sb, f8.reserved = ks.data_ptr(), ks.stride(0) if ks.shape[0] > 1 else 0, 0
    return f8, ks


def _list_operand(fn, indices, query):
    sp, (B, Sq, topk) = MlaSparse(), indices.shape
    sp.indices, sp.topk, sp.reserved = indices.data_ptr(), topk, 0
    sp.stride_b, sp.stride_q = indices.stride(0) if B > 1 else 0, indices.stride(1) if Sq > 1 else 0
    return sp, indices


class _Variant(NamedTuple):
    """one public function of the decode (csrc/fasn_mla.hip: MlaVariant): what its cache holds and which operand stands behind the block"""
    fn: str                 # the public name, for messages
    row: int                # elements of a cache row
    cache_dtypes: Optional[tuple]   # the dtypes the cache may have; None: the query's
    refusals: tuple         # (cache dtypes or None for every other, the refusal's text in front of the dtype, behind it), in the order tried
    indices: bool           # the operand is the top-k list, checked beside the queries
    operand: Optional[Callable]   # (fn, kv_scale or indices, query) -> (the ctypes operand, the tensor it points into); None: no operand
    forward: str            # the entry points: the forward, its workspace size ...
    workspace: str
    append: str             # ... and the append ...
    append_operand: bool    # ... which takes the operand too


_MLA = _Variant("flash_attention_n_mla", MLA_HEAD_DIM, None,
                ((_FP8_DTYPES, "an FP8 latent cache (", ") is flash_attention_n_mla_fp8's (e4m3fn codes with kv_scale); " + _SERVED),),
                False, None, "fasn_fwd_mla", "fasn_mla_workspace_bytes", "fasn_mla_append", False)
_MLA_FP8 = _Variant("flash_attention_n_mla_fp8", MLA_HEAD_DIM, (torch.float8_e4m3fn,),
                    ((_FP8_DTYPES, "the cache must hold torch.float8_e4m3fn codes; ", " has no kernel; " + _SERVED),
                     (None, "the cache must hold torch.float8_e4m3fn codes; a ", " cache is flash_attention_n_mla's")),
                    False, _scale_operand, "fasn_fwd_mla_fp8", "fasn_mla_fp8_workspace_bytes", "fasn_mla_fp8_append", True)
_MLA_SPARSE = _Variant("flash_attention_n_mla_sparse", MLA_HEAD_DIM, None,
                       (((torch.uint8,) + _FP8_DTYPES, "an FP8 latent cache (",
                         f") behind indices is flash_attention_n_mla_sparse_fp8's ({MLA_FP8_ROW_BYTES}-byte rows); " + _SERVED),),
                       True, _list_operand, "fasn_fwd_mla_sparse", "fasn_mla_sparse_workspace_bytes", "fasn_mla_append", False)   # (the 16-bit cache's append)
_MLA_SPARSE_FP8 = _Variant("flash_attention_n_mla_sparse_fp8", MLA_FP8_ROW_BYTES, _BYTE_DTYPES,
                           ((None, f"the cache must hold {MLA_FP8_ROW_BYTES}-byte rows as torch.uint8 or torch.float8_e4m3fn; a ",
                             " cache behind indices is flash_attention_n_mla_sparse's; " + _SERVED),),
                           True, _list_operand, "fasn_fwd_mla_sparse_fp8", "fasn_mla_sparse_fp8_workspace_bytes", "fasn_mla_sparse_fp8_append", False)


# how the shared checks call a caller's operands: the queries, the cache, the new rows and their width, the device rule's text
_Names = NamedTuple("_Names", [("query", str), ("cache", str), ("new", str), ("new_dim", int), ("where", str)])
_MLA_NAMES = _Names("query", "kv_cache", "kv_new", MLA_HEAD_DIM, "every operand must live on the query's device (the lengths, the block table "
                    "and the index list are read by the kernels, never on the host); " + _SERVED)
_NO_CPU = "flash_attention_softmax_n_amd runs on MI355X device tensors only; got a CPU tensor (there is deliberately no CPU fallback)"


def _cache_operands(a, stride, fn, names, query, B, Sq, dev, operands, no_grad, cache, row, cache_seqlens, block_table, new):
    """What the decode and the indexer share behind their own checks: every operand on the queries' device, forward only, the rules of
    `cache_seqlens`, `block_table`, the page size and the dense batch, the cache's layout, the new rows; then the cache, table and length
    members of the argument block `a` (stride: its array of the cache's page and row strides). operands: (name, tensor) of all but the
    queries, in the order the device rule names them; no_grad: what must not require grad. Returns (the new rows as the kernels read
    them, page_size)."""
    for name, t in operands:
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name} is on {t.device}, {names.query} on {dev}: {names.where}")
    if torch.is_grad_enabled() and any(isinstance(t, Tensor) and t.requires_grad for t in no_grad):
        raise RuntimeError(f"{fn} is forward only (inference): an input requires grad. Call it under torch.no_grad()")
    if cache_seqlens.dtype != torch.int32 or cache_seqlens.dim() != 1 or cache_seqlens.shape[0] != B or not cache_seqlens.is_contiguous():
        raise ValueError(f"cache_seqlens must be a contiguous int32 tensor of shape [{B}] on the device; got {cache_seqlens.dtype} {tuple(cache_seqlens.shape)}")
    page_size = cache.shape[1]
    paged = block_table is not None
    if paged:
        if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.stride(1) != 1 or block_table.shape[0] != B or block_table.shape[1] < 1:
            raise ValueError(f"block_table must be an int32 tensor [B, max_pages] = [{B}, >= 1] with unit column stride; got {block_table.dtype} {tuple(block_table.shape)}")
        if page_size % 64 != 0:
            raise ValueError(f"page_size {page_size} is not supported: a paged cache needs page_size % 64 == 0 (a 64-key tile never straddles a page)")
    elif cache.shape[0] != B:
        raise ValueError(f"dense cache (block_table=None) must be [B, capacity, 1, {row}] with B = {B}; got {tuple(cache.shape)}")
    _check_cache(names.cache, cache, paged, row)
    if new is not None:
        if new.dtype != query.dtype or tuple(new.shape) != (B, Sq, 1, names.new_dim):
            raise ValueError(f"{names.new} must be [B, Sq, 1, {names.new_dim}] = [{B}, {Sq}, 1, {names.new_dim}] in {query.dtype}; got {tuple(new.shape)} {new.dtype}")
        new = _rows(new)
    stride[0] = cache.stride(0) if cache.size(0) > 1 else 0
    stride[1] = cache.stride(1) if cache.size(1) > 1 else row
    if paged:
        a.block_table, a.block_table_stride, a.max_pages = block_table.data_ptr(), block_table.stride(0) if B > 1 else block_table.shape[1], block_table.shape[1]
    else:
        a.block_table, a.block_table_stride, a.max_pages = None, 0, 1
    a.seqlens, a.seqlen_add, a.page_size = cache_seqlens.data_ptr(), Sq if new is not None else 0, page_size
    return new, page_size


def _mla(v, query, kv_cache, cache_seqlens, scale, operand, block_table, kv_new, softmax_n_param, is_causal, return_lse):
    """the one call path of the four functions; v: the function's variant record; operand: kv_scale or indices, where v takes one"""
    fn, row, cache_dtypes, refusals, takes_list, build_operand, fwd, ws_name, append, append_operand = v
    if not isinstance(query, Tensor) or query.dim() != 4 or not isinstance(kv_cache, Tensor) or kv_cache.dim() not in (3, 4):
        raise ValueError(f"{fn}: query must be [B, H, Sq, {MLA_HEAD_DIM}] and kv_cache [num_pages, page_size, 1, {row}] (paged) or "
                         f"[B, capacity, 1, {row}] (dense); {_SERVED}")
    if kv_cache.dim() == 3:
        kv_cache = kv_cache.unsqueeze(2)
    cache_dtype = kv_cache.dtype
    if cache_dtypes is None or cache_dtype not in cache_dtypes:
        for dtypes, before, behind in refusals:
            if dtypes is None or cache_dtype in dtypes:
                raise TypeError(f"{fn}: {before}{cache_dtype}{behind}")
    B, H, Sq, D = query.shape
    if D != MLA_HEAD_DIM or kv_cache.shape[3] != row or kv_cache.shape[2] != 1:
        raise ValueError(f"{fn}: query is {tuple(query.shape)} and kv_cache {tuple(kv_cache.shape)}: not a latent cache; {_SERVED}. "
                         "Separate K and V of one head dim are flash_attention_n_kvcache's")
    if query.dtype not in _KV_DTYPES:
        raise ValueError(f"{fn}: dtype {query.dtype} is not supported; {_SERVED}")
    if cache_dtypes is None and cache_dtype != query.dtype:
        raise TypeError(f"{fn}: query and kv_cache must share one dtype; got {query.dtype} and {kv_cache.dtype}")
    if H * Sq > MLA_MAX_ROWS:
        raise ValueError(f"{fn}: H * Sq = {H} x {Sq} = {H * Sq} rows exceed {MLA_MAX_ROWS}; {_SERVED}")
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise TypeError(f"{fn}: scale must be a Python float (required: MLA models use (128 + 64) ** -0.5 times their YaRN factor, never "
                        f"{MLA_HEAD_DIM} ** -0.5); got {type(scale).__name__}")
    scale = float(scale)
    if query.dtype == torch.float16 and not abs(scale) * _LOG2E <= _F16_MAX_PRESCALE:
        raise ValueError(f"{fn}: float16 serves |scale| * log2(e) <= {_F16_MAX_PRESCALE:g} (the queries are prescaled in float16); got scale "
                         f"{scale}. Use bfloat16, or fold the factor into the queries")
    dev = query.device
    indices = operand if takes_list else None
    if takes_list:
        if not isinstance(indices, Tensor) or indices.dtype != torch.int32 or tuple(indices.shape[:2]) != (B, Sq) or indices.dim() != 3 \
                or indices.stride(2) != 1:
            got = f"{indices.dtype} {tuple(indices.shape)}" if isinstance(indices, Tensor) else type(indices).__name__
            raise ValueError(f"{fn}: indices must be an int32 tensor [B, Sq, topk] = [{B}, {Sq}, topk] of logical positions with unit last "
                             f"stride; got {got}; {_SERVED}")
        if indices.shape[2] < 64 or indices.shape[2] % 64 != 0:
            raise ValueError(f"{fn}: topk = {indices.shape[2]} is not supported: topk % 64 == 0 and topk >= 64 (pad the list with -1 where "
                             f"it is built: the call does not copy it); {_SERVED}")
    a = MlaArgs()
    operands = (("kv_cache", kv_cache), ("indices", indices), ("cache_seqlens", cache_seqlens), ("block_table", block_table), ("kv_new", kv_new))
    kv_new, _ = _cache_operands(a, a.kv_stride, fn, _MLA_NAMES, query, B, Sq, dev, operands, (query, kv_cache, kv_new, softmax_n_param),
                                kv_cache, row, cache_seqlens, block_table, kv_new)
    query = _rows(query)
    held = build_operand(fn, operand, query) if build_operand else None   # (the ctypes operand, the tensor it points into: alive until the launches)
    if isinstance(softmax_n_param, Tensor):
        nt, n = _n_tensor(softmax_n_param.detach(), query).contiguous(), 0.0
    else:
        nt, n = None, 0.0 if softmax_n_param is None else float(softmax_n_param)
        if n < 0:
            raise ValueError("softmax_n_param must be >= 0")
    if not query.is_cuda:   # (the argument checks above need no device; everything below does)
        raise RuntimeError(_NO_CPU)
    out = torch.empty((B, H, Sq, MLA_VALUE_DIM), dtype=query.dtype, device=dev)
    lse = torch.empty((B, H, Sq), dtype=torch.float32, device=dev) if return_lse else None
    a.q, a.o = _view4(query), _view4(out)
    a.lse = None if lse is None else lse.data_ptr()
    a.kv_cache = kv_cache.data_ptr()
    a.B, a.H, a.Sq, a.D, a.Dv = B, H, Sq, MLA_HEAD_DIM, MLA_VALUE_DIM
    a.dtype = _KV_DTYPES[query.dtype]
    a.scale, a.softmax_n, a.causal, a.reserved = scale, n, 1 if is_causal else 0, 0
    if nt is not None:
        a.n = nt.data_ptr()
        a.n_stride_b, a.n_stride_h = _n_strides(nt)
    lib = _lib.load()
    ops = () if held is None else (held[0],)

    def launch():
        stream = _stream_ptr(dev)
        if kv_new is not None:
            _lib.check(getattr(lib, append)(a, *(ops if append_operand else ()), _view4(kv_new), stream), append)
        ws_bytes = getattr(lib, ws_name)(a, *ops)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)   # torch's caching allocator: capturable
        _lib.check(getattr(lib, fwd)(a, *ops, ws.data_ptr(), ws_bytes, stream), fwd)

    _on_device(dev, launch)
    return out if lse is None else (out, lse)


MLA_INDEX_DIM, MLA_INDEX_HEADS = 128, (32, 64)
_INDEX_SERVED = (f"served: index queries [B, Hi, Sq, {MLA_INDEX_DIM}] with Hi = 32 or 64 and a cache of {MLA_INDEX_DIM}-feature index keys, both fp16 or "
                 "both bf16, fp32 weights [B, Hi, Sq], causal or not, topk a multiple of 64, a paged cache with page_size % 64 == 0 or a dense "
                 f"one; not served: FP8 index keys or queries, other head counts, feature sizes other than {MLA_INDEX_DIM}, packed queries, gradients")


_INDEX_NAMES = _Names("q_index", "k_cache", "k_new", MLA_INDEX_DIM, "every operand must live on the queries' device (the lengths and the block "
                      "table are read by the kernels, never on the host); " + _INDEX_SERVED)


def flash_attention_n_mla_index(
        q_index: Tensor,
        weights: Tensor,
        k_cache: Tensor,
        cache_seqlens: Tensor,
        topk: int,
        block_table: Optional[Tensor] = None,
        k_new: Optional[Tensor] = None,
        is_causal: bool = True,
        return_logits: bool = False):
    """The lightning indexer in front of flash_attention_n_mla_sparse / flash_attention_n_mla_sparse_fp8 (DeepSeek-V3.2), on MI355X: per
    batch element b and query position i the logit of cache position j is

        logit[b, i, j] = sum_h weights[b, h, i] * relu(q_index[b, h, i, :] . k_b[j, :])

    and the call returns the positions of the topk largest logits. There is no scale: the model folds its softmax scale and Hi ** -0.5
    into `weights`. Lengths, block table and cache are read by the kernels only and the launches depend on shapes, topk and capacity
    alone, so one captured graph serves every step.

    :param q_index: [B, Hi, Sq, 128] fp16 / bf16 device tensor, Hi = 32 or 64; feature stride 1, rows 16-byte aligned, other strides
                  free; never copied.
    :param weights: fp32 [B, Hi, Sq], any non-negative strides (the model's [B, Sq, Hi] transposed is a legal view); may be negative.
    :param k_cache: the index keys in q_index's dtype: paged [num_pages, page_size, 1, 128] with `block_table` (page_size a multiple of
                  64), or dense [B, capacity, 1, 128]; a 3-D tensor without the head axis is the same thing. Never copied; rows at or
                  beyond the length may hold anything (NaN included).
    :param cache_seqlens: int32 [B] ON THE DEVICE: valid rows per batch element before this call; never read on the host, not modified.
    :param topk: a Python int, topk % 64 == 0 and topk >= 64. topk > capacity is legal and only pads.
    :param block_table: int32 [B, max_pages] on the device. Entries beyond the pages a row needs are never read.
    :param k_new: optional [B, Sq, 1, 128]: written to the positions cache_seqlens[b] .. + Sq - 1 first (positions at or beyond the
                  capacity are dropped in the kernel); the new rows are then visible.
    :param is_causal: with len_b = clamp(cache_seqlens[b] + (Sq if k_new is given else 0), 0, capacity), position i sees the positions
                  j < L, L = len_b - (Sq - 1 - i). False: L = len_b for every position.
    :param return_logits: also return fp32 [B, Sq, capacity]: the logit where j < L, -inf elsewhere.
    :return: int32 [B, Sq, topk], contiguous: the min(topk, L) positions of largest logit in ASCENDING position order, then -1 - directly
                  the `indices` of both sparse calls. Among equal logits at the cut the lower position wins (-0.0 and +0.0 are equal):
                  the list is the stable descending sort of logit[:L], cut at topk, sorted ascending. L <= 0 gives a row of -1.
    """
    fn = "flash_attention_n_mla_index"
    if not isinstance(q_index, Tensor) or q_index.dim() != 4 or not isinstance(k_cache, Tensor) or k_cache.dim() not in (3, 4):
        raise ValueError(f"{fn}: q_index must be [B, Hi, Sq, {MLA_INDEX_DIM}] and k_cache [num_pages, page_size, 1, {MLA_INDEX_DIM}] (paged) or "
                         f"[B, capacity, 1, {MLA_INDEX_DIM}] (dense); {_INDEX_SERVED}")
    if k_cache.dim() == 3:
        k_cache = k_cache.unsqueeze(2)
    if q_index.dtype in _FP8_DTYPES or k_cache.dtype in (torch.uint8,) + _FP8_DTYPES:
        raise TypeError(f"{fn}: FP8 index keys or queries ({q_index.dtype}, {k_cache.dtype}) have no kernel; {_INDEX_SERVED}")
    if q_index.dtype not in _KV_DTYPES:
        raise ValueError(f"{fn}: dtype {q_index.dtype} is not supported; {_INDEX_SERVED}")
    if k_cache.dtype != q_index.dtype:
        raise TypeError(f"{fn}: q_index and k_cache must share one dtype; got {q_index.dtype} and {k_cache.dtype}")
    B, Hi, Sq, D = q_index.shape
    if D != MLA_INDEX_DIM or k_cache.shape[3] != MLA_INDEX_DIM or k_cache.shape[2] != 1:
        raise ValueError(f"{fn}: q_index is {tuple(q_index.shape)} and k_cache {tuple(k_cache.shape)}: not an index-key cache of feature size "
                         f"{MLA_INDEX_DIM}; {_INDEX_SERVED}")
    if Hi not in MLA_INDEX_HEADS:
        raise ValueError(f"{fn}: Hi = {Hi} index heads are not supported; {_INDEX_SERVED}")
    if isinstance(topk, bool) or not isinstance(topk, int) or topk < 64 or topk % 64 != 0:
        raise ValueError(f"{fn}: topk = {topk} is not supported: a Python int with topk % 64 == 0 and topk >= 64, as the sparse calls take "
                         f"their lists; {_INDEX_SERVED}")
    if not isinstance(weights, Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != (B, Hi, Sq) or any(s < 0 for s in weights.stride()):
        got = f"{weights.dtype} {tuple(weights.shape)}" if isinstance(weights, Tensor) else type(weights).__name__
        raise ValueError(f"{fn}: weights must be an fp32 tensor [B, Hi, Sq] = [{B}, {Hi}, {Sq}] (any non-negative strides); got {got}")
    if q_index.stride(3) != 1 or q_index.data_ptr() % 16 != 0 or any(q_index.stride(i) % 8 != 0 for i in range(3) if q_index.size(i) > 1):
        raise ValueError(f"{fn}: q_index needs feature stride 1 and 16-byte aligned rows (it is never copied); got strides {tuple(q_index.stride())}")
    dev = q_index.device
    a = MlaIndexArgs()
    operands = (("weights", weights), ("k_cache", k_cache), ("cache_seqlens", cache_seqlens), ("block_table", block_table), ("k_new", k_new))
    k_new, page_size = _cache_operands(a, a.k_stride, fn, _INDEX_NAMES, q_index, B, Sq, dev, operands, (q_index, weights, k_cache, k_new),
                                       k_cache, MLA_INDEX_DIM, cache_seqlens, block_table, k_new)
    if not q_index.is_cuda:   # (the argument checks above need no device; everything below does)
        raise RuntimeError(_NO_CPU)
    capacity = block_table.shape[1] * page_size if block_table is not None else page_size
    weights = weights.detach()
    a.q = _view4(q_index)
    a.w = weights.data_ptr()
    for i in range(3):
        a.w_stride[i] = weights.stride(i) if weights.size(i) > 1 else 0
    a.k_cache = k_cache.data_ptr()
    a.B, a.Hi, a.Sq, a.D = B, Hi, Sq, MLA_INDEX_DIM
    a.dtype, a.causal, a.topk, a.reserved = _KV_DTYPES[q_index.dtype], 1 if is_causal else 0, topk, 0
    a.indices_stride[0], a.indices_stride[1] = Sq * topk, topk
    a.logits_stride[0], a.logits_stride[1] = Sq * capacity, capacity
    lib = _lib.load()
    res = []

    def launch():
        stream = _stream_ptr(dev)
        idx = torch.empty((B, Sq, topk), dtype=torch.int32, device=dev)
        # the kernel writes -inf at the hidden positions of the tiles it works on only: the buffer starts as -inf
        logits = torch.full((B, Sq, capacity), float("-inf"), dtype=torch.float32, device=dev) if return_logits else None
        a.indices = idx.data_ptr()
        a.logits = None if logits is None else logits.data_ptr()
        if k_new is not None:
            _lib.check(lib.fasn_mla_index_append(a, _view4(k_new), stream), "fasn_mla_index_append")
        ws_bytes = lib.fasn_mla_index_workspace_bytes(a)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)   # torch's caching allocator: capturable
        _lib.check(lib.fasn_mla_index(a, ws.data_ptr(), ws_bytes, stream), "fasn_mla_index")
        res.extend((idx, logits))

    _on_device(dev, launch)
    return (res[0], res[1]) if return_logits else res[0]
