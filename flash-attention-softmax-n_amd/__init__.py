"""flash-attention-softmax-n for AMD MI355X (gfx950): the reference package's attention API on hand-written HIP.

Public surface = flash_attention_softmax_n/__init__.py:3-9 of the reference:
    flash_attention_n, softmax_n, slow_attention_n, flash_attention_n_triton (+ TRITON_INSTALLED for source compat)
    flash_attention_n_varlen  (training attention on packed variable-length sequences, forward and backward; no counterpart in the reference)
    flash_attention_n_varlen_rope  (the same call with rotary position embedding at per-sequence positions: one launch rotates q and k)
    flash_attention_n_kvcache  (inference over a paged / dense K/V cache with device-side lengths; no counterpart in the reference)
    flash_attention_n_kvcache_prefill  (the same cache, any number of query positions, ragged query lengths on the device)
    flash_attention_n_kvcache_window  (a sliding-window layer on the same cache: decode or prefill, only the window's pages are read)
    flash_attention_n_kvcache_rope  (rotary position embedding fused into the append: q and k_new rotated at the positions in device memory)
    flash_attention_n_kvcache_varlen  (the prefill call on token-packed queries with cu_seqlens_q on the device: a continuous-batching step)
    flash_attention_n_kvcache_varlen_window  (a sliding-window layer on the same token-packed step)
    flash_attention_n_kvcache_varlen_rope  (rotary position embedding fused into the append of the token-packed step, with or without a window)
    flash_attention_n_kvcache_tree  (speculative-decoding verification: the new positions are a tree of draft tokens, one int64 mask word per node)
    flash_attention_n_kvcache_tree_commit  (after acceptance: the accepted path's cache rows move behind the prefix)
    flash_attention_n_kvcache_fp8  (decode / prefill over a cache of e4m3fn codes with per-(batch, K/V head) scales on the device)
    flash_attention_n_kvcache_fp8_window  (a sliding-window layer on the FP8 cache: only the window's pages are read)
    flash_attention_n_kvcache_fp8_rope  (rotary position embedding fused into the quantising append of the FP8 cache, with or without a window)
    flash_attention_n_kvcache_fp8_tree  (speculative-decoding verification over the FP8 cache: the token tree of flash_attention_n_kvcache_tree)
    flash_attention_n_kvcache_fp8_tree_commit  (after acceptance on the FP8 cache: the accepted path's code rows move behind the prefix)
    flash_attention_n_kvcache_fp8_varlen  (the token-packed step over the FP8 cache: cu_seqlens_q on the device, one scale per sequence and K/V head)
    flash_attention_n_kvcache_fp8_varlen_window  (a sliding-window layer on the token-packed step over the FP8 cache)
    flash_attention_n_kvcache_fp8_varlen_rope  (rotary position embedding fused into the quantising append of the token-packed step)
    flash_attention_n_kvcache_shared_prefix  (decode behind one shared prefix: its pages are attended to once per K/V head for the whole batch)
    flash_attention_n_kvcache_prefix_groups  (decode behind several shared prefixes in one call: prefix_group[b] on the device names the prefix of b, or none)
    surgery.apply_attention_softmax_n / surgery.policy_registry  (flash_attention_softmax_n/surgery, composer-free)
Every function runs on device tensors through libfasn.so; importing the package without the built
library raises ImportError (no silent fallback).
"""
from . import _lib, dropout, statistics, surgery
from .flash_attn import flash_attention_n, flash_attention_n_triton, flash_attention_n_varlen, flash_attention_n_varlen_rope, slow_attention_n
from .kvcache import (flash_attention_n_kvcache, flash_attention_n_kvcache_fp8, flash_attention_n_kvcache_fp8_rope, flash_attention_n_kvcache_fp8_tree,
                      flash_attention_n_kvcache_fp8_tree_commit, flash_attention_n_kvcache_fp8_varlen, flash_attention_n_kvcache_fp8_varlen_rope,
                      flash_attention_n_kvcache_fp8_varlen_window, flash_attention_n_kvcache_fp8_window,
                      flash_attention_n_kvcache_prefill, flash_attention_n_kvcache_prefix_groups, flash_attention_n_kvcache_rope, flash_attention_n_kvcache_shared_prefix, flash_attention_n_kvcache_tree,
                      flash_attention_n_kvcache_tree_commit, flash_attention_n_kvcache_varlen,
                      flash_attention_n_kvcache_varlen_rope, flash_attention_n_kvcache_varlen_window, flash_attention_n_kvcache_window)
from .softmax import softmax_n

_lib.load()  # fail loudly at import if the HIP extension is missing

TRITON_INSTALLED = False  # kept for source compatibility: the Triton path is replaced by the HIP kernel
HIP_NATIVE = True

__all__ = ["flash_attention_n", "flash_attention_n_varlen", "flash_attention_n_varlen_rope", "flash_attention_n_kvcache", "flash_attention_n_kvcache_prefill", "flash_attention_n_kvcache_window", "flash_attention_n_kvcache_rope", "flash_attention_n_kvcache_varlen", "flash_attention_n_kvcache_varlen_window", "flash_attention_n_kvcache_varlen_rope", "flash_attention_n_kvcache_tree", "flash_attention_n_kvcache_tree_commit", "flash_attention_n_kvcache_fp8", "flash_attention_n_kvcache_fp8_window", "flash_attention_n_kvcache_fp8_rope", "flash_attention_n_kvcache_fp8_tree", "flash_attention_n_kvcache_fp8_tree_commit", "flash_attention_n_kvcache_fp8_varlen", "flash_attention_n_kvcache_fp8_varlen_window", "flash_attention_n_kvcache_fp8_varlen_rope", "flash_attention_n_kvcache_shared_prefix", "flash_attention_n_kvcache_prefix_groups", "flash_attention_n_triton", "slow_attention_n", "softmax_n", "TRITON_INSTALLED", "HIP_NATIVE"]
