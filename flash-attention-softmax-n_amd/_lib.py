"""ctypes binding of libfasn.so (C ABI declared in include/fasn.h).

The library is the product path: if it is missing or does not export every symbol of the header the
import fails loudly — there is no CPU / eager fallback behind these functions.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int32, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfasn.so")

FASN_ABI_VERSION = 6
FASN_BWD_ONE_PASS = 1
FASN_DTYPE_F16, FASN_DTYPE_BF16, FASN_DTYPE_F32 = 0, 1, 2
FASN_BIAS_NONE, FASN_BIAS_SAME, FASN_BIAS_F32 = 0, 1, 2
FASN_PATH_NAMES = {0: "plain", 1: "key-padding", 2: "vector mask/bias", 3: "vector bias + key-padding", 4: "element-load (slow)", 5: "fp32"}
FASN_PATH_ELEMENT = 4
FASN_PLAN_FWD, FASN_PLAN_BWD, FASN_PLAN_FWD_WS = 0, 1, 2
FASN_ROW_FWD, FASN_ROW_BWD = 0, 1

# every entry point include/fasn.h declares (tests check the .so exports all of them)
EXPORTS = (
    "fasn_abi_version", "fasn_strerror", "fasn_supported", "fasn_fwd", "fasn_fwd_path", "fasn_bwd_path", "fasn_fwd_workspace_bytes", "fasn_fwd_ws",
    "fasn_bwd_workspace_bytes", "fasn_bwd", "fasn_rng_advance", "fasn_launch_plan",
    "fasn_fwd_n", "fasn_bwd_dn_workspace_bytes", "fasn_bwd_dn",
    "fasn_softmax_n_fwd", "fasn_softmax_n_bwd", "fasn_moments", "fasn_softmax_n_plan", "fasn_moments_plan",
    "fasn_fwd_kvcache_workspace_bytes", "fasn_fwd_kvcache", "fasn_kvcache_append", "fasn_kvcache_plan",
    "fasn_fwd_kvprefill_workspace_bytes", "fasn_fwd_kvprefill", "fasn_kvprefill_append", "fasn_kvprefill_plan",
    "fasn_fwd_kvcache_alibi", "fasn_fwd_kvprefill_alibi", "fasn_kvcache_alibi_plan", "fasn_kvprefill_alibi_plan",
    "fasn_fwd_kvcache_window_workspace_bytes", "fasn_fwd_kvcache_window", "fasn_kvcache_window_plan",
    "fasn_fwd_kvprefill_window_workspace_bytes", "fasn_fwd_kvprefill_window", "fasn_kvprefill_window_plan",
    "fasn_kvcache_rope_append", "fasn_kvprefill_rope_append", "fasn_kvcache_rope_append_plan", "fasn_kvprefill_rope_append_plan",
    "fasn_fwd_kvvarlen_workspace_bytes", "fasn_fwd_kvvarlen", "fasn_kvvarlen_append", "fasn_kvvarlen_plan",
    "fasn_fwd_kvvarlen_window_workspace_bytes", "fasn_fwd_kvvarlen_window", "fasn_kvvarlen_window_plan",
    "fasn_kvvarlen_rope_append", "fasn_kvvarlen_rope_append_plan",
    "fasn_fwd_kvcache_tree_workspace_bytes", "fasn_fwd_kvcache_tree", "fasn_kvcache_tree_plan",
    "fasn_fwd_kvprefill_tree_workspace_bytes", "fasn_fwd_kvprefill_tree", "fasn_kvprefill_tree_plan",
    "fasn_kvcache_tree_rope_append", "fasn_kvprefill_tree_rope_append", "fasn_kvcache_tree_commit",
    "fasn_fwd_kvcache_fp8_workspace_bytes", "fasn_fwd_kvcache_fp8", "fasn_kvcache_fp8_plan", "fasn_kvcache_fp8_append",
    "fasn_fwd_kvprefill_fp8_workspace_bytes", "fasn_fwd_kvprefill_fp8", "fasn_kvprefill_fp8_plan", "fasn_kvprefill_fp8_append",
    "fasn_fwd_kvcache_fp8_window_workspace_bytes", "fasn_fwd_kvcache_fp8_window", "fasn_kvcache_fp8_window_plan",
    "fasn_fwd_kvprefill_fp8_window_workspace_bytes", "fasn_fwd_kvprefill_fp8_window", "fasn_kvprefill_fp8_window_plan",
    "fasn_kvcache_fp8_rope_append", "fasn_kvprefill_fp8_rope_append", "fasn_kvcache_fp8_rope_append_plan", "fasn_kvprefill_fp8_rope_append_plan",
    "fasn_fwd_kvcache_fp8_tree_workspace_bytes", "fasn_fwd_kvcache_fp8_tree", "fasn_kvcache_fp8_tree_plan",
    "fasn_fwd_kvprefill_fp8_tree_workspace_bytes", "fasn_fwd_kvprefill_fp8_tree", "fasn_kvprefill_fp8_tree_plan",
    "fasn_kvcache_fp8_tree_rope_append", "fasn_kvprefill_fp8_tree_rope_append", "fasn_kvcache_fp8_tree_rope_append_plan",
    "fasn_kvprefill_fp8_tree_rope_append_plan", "fasn_kvcache_fp8_tree_commit",
    "fasn_kv_forward_workspace_bytes", "fasn_kv_forward", "fasn_kv_forward_plan", "fasn_kv_append", "fasn_kv_append_plan",
    "fasn_fwd_varlen", "fasn_bwd_varlen", "fasn_varlen_plan",
    "fasn_fwd_varlen_window", "fasn_bwd_varlen_window", "fasn_varlen_window_plan",
    "fasn_varlen_rope", "fasn_varlen_rope_plan",
    "fasn_fwd_shared_prefix_workspace_bytes", "fasn_fwd_shared_prefix", "fasn_shared_prefix_plan",
    "fasn_fwd_prefix_groups_workspace_bytes", "fasn_fwd_prefix_groups", "fasn_prefix_groups_plan",
)


class View4(Structure):
    _fields_ = [("ptr", c_void_p), ("stride", c_int64 * 4)]


class FwdArgs(Structure):
    _fields_ = [
        ("q", View4), ("k", View4), ("v", View4), ("o", View4),
        ("lse", c_void_p),
        ("mask", View4), ("bias", View4),
        ("bias_dtype", c_int32), ("dtype", c_int32),
        ("B", c_int32), ("H", c_int32), ("Sq", c_int32), ("Sk", c_int32), ("D", c_int32), ("Dv", c_int32),
        ("scale", c_float), ("softmax_n", c_float), ("causal", c_int32), ("dropout_p", c_float),
        ("seed", c_uint64), ("offset", c_uint64),
        ("kv_group", c_int32),
        ("rng_state", c_void_p),
    ]


class BwdArgs(Structure):
    _fields_ = [
        ("fwd", FwdArgs),
        ("dout", View4), ("dq", View4), ("dk", View4), ("dv", View4),
        ("delta", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
        ("dbias", View4),
        ("flags", c_int32),
        ("dbias_dtype", c_int32),
    ]


class Varlen(Structure):
    """fasn_varlen (include/fasn.h): the packed variable-length training call - the two offset tables in device memory, the number of
    sequences and the host bounds of the lengths; reserved = 0"""
    _fields_ = [("cu_seqlens_q", c_void_p), ("cu_seqlens_k", c_void_p), ("num_seqs", c_int32), ("max_seqlen_q", c_int32),
                ("max_seqlen_k", c_int32), ("reserved", c_int32)]


class KvCacheArgs(Structure):
    """fasn_kvcache_args (include/fasn.h): forward over a paged or dense K/V cache whose lengths live in device memory"""
    _fields_ = [
        ("q", View4), ("o", View4),
        ("lse", c_void_p),
        ("k_cache", c_void_p), ("v_cache", c_void_p),
        ("k_stride", c_int64 * 3), ("v_stride", c_int64 * 3),
        ("block_table", c_void_p), ("block_table_stride", c_int64), ("max_pages", c_int32),
        ("seqlens", c_void_p), ("seqlen_add", c_int32), ("page_size", c_int32),
        ("B", c_int32), ("H", c_int32), ("kv_group", c_int32), ("Sq", c_int32), ("D", c_int32),
        ("dtype", c_int32),
        ("scale", c_float), ("softmax_n", c_float), ("causal", c_int32),
        ("n", c_void_p), ("n_stride_b", c_int64), ("n_stride_h", c_int64),
    ]


class KvPrefillArgs(Structure):
    """fasn_kvprefill_args (include/fasn.h): the K/V-cache arguments plus the per-batch query lengths in device memory"""
    _fields_ = [("kv", KvCacheArgs), ("q_seqlens", c_void_p)]


class KvVarlenArgs(Structure):
    """fasn_kvvarlen_args (include/fasn.h): the prefill arguments on token-packed queries - B sequences, their token offsets in device
    memory, the rows of the token buffers"""
    _fields_ = [("pf", KvPrefillArgs), ("cu_seqlens_q", c_void_p), ("total_tokens", c_int32), ("reserved", c_int32)]


class AlibiSlopes(Structure):
    """fasn_alibi_slopes (include/fasn.h): per-(batch, query head) fp32 ALiBi slopes in device memory, for the *_alibi cache calls"""
    _fields_ = [("slopes", c_void_p), ("stride_b", c_int64), ("stride_h", c_int64)]


class KvWindow(Structure):
    """fasn_kv_window (include/fasn.h): the sliding window of the *_window cache calls, a host integer >= 1; reserved = 0"""
    _fields_ = [("window", c_int32), ("reserved", c_int32)]


class KvRope(Structure):
    """fasn_kv_rope (include/fasn.h): the cos / sin tables of the rotary rotate-and-append calls, [rows, rotary_dim / 2] in device memory"""
    _fields_ = [("cos", c_void_p), ("sin", c_void_p), ("row_stride", c_int64), ("rows", c_int32), ("rotary_dim", c_int32),
                ("table_dtype", c_int32), ("interleaved", c_int32)]


class KvTree(Structure):
    """fasn_kv_tree (include/fasn.h): the token tree of the *_tree cache calls - one int64 word per node in device memory, bit t of word
    (b, i): node i sees node t - and the sliding window (0: none); reserved = 0"""
    _fields_ = [("mask", c_void_p), ("batch_stride", c_int64), ("window", c_int32), ("reserved", c_int32)]


class KvFp8(Structure):
    """fasn_kv_fp8 (include/fasn.h): the per-(batch, K/V head) fp32 scales of an e4m3fn cache in device memory, for the *_fp8 cache calls;
    reserved = 0"""
    _fields_ = [("k_scale", c_void_p), ("v_scale", c_void_p), ("k_sb", c_int64), ("k_sh", c_int64), ("v_sb", c_int64), ("v_sh", c_int64),
                ("reserved", c_int32)]


FASN_KV_CALL_DECODE, FASN_KV_CALL_PREFILL, FASN_KV_CALL_PACKED = 0, 1, 2


class KvCall(Structure):
    """fasn_kv_call (include/fasn.h): a cache call as data - the kind of its block, the block, and the operands present (NULL: not part of
    the call) - for the operand-set entry points fasn_kv_forward* / fasn_kv_append*; reserved = 0"""
    _fields_ = [("kind", c_int32), ("reserved", c_int32), ("block", c_void_p), ("fp8", POINTER(KvFp8)), ("tree", POINTER(KvTree)),
                ("window", POINTER(KvWindow)), ("alibi", POINTER(AlibiSlopes))]


class KvTreeCommit(Structure):
    """fasn_kv_tree_commit (include/fasn.h): the cache and the accepted path of fasn_kvcache_tree_commit"""
    _fields_ = [
        ("k_cache", c_void_p), ("v_cache", c_void_p),
        ("k_stride", c_int64 * 3), ("v_stride", c_int64 * 3),
        ("block_table", c_void_p), ("block_table_stride", c_int64), ("max_pages", c_int32), ("page_size", c_int32),
        ("seqlens", c_void_p),
        ("B", c_int32), ("Hkv", c_int32), ("D", c_int32), ("A", c_int32),
        ("accepted", c_void_p), ("accepted_stride", c_int64), ("accepted_lens", c_void_p),
        ("nodes", c_int32), ("reserved", c_int32),
    ]


class SharedPrefix(Structure):
    """fasn_shared_prefix (include/fasn.h): the shared prefix of fasn_fwd_shared_prefix - its length (one int32) and its page ids
    ([max_prefix_pages] int32), both in device memory; reserved = 0"""
    _fields_ = [("prefix_len", c_void_p), ("prefix_table", c_void_p), ("max_prefix_pages", c_int32), ("reserved", c_int32)]


class PrefixGroups(Structure):
    """fasn_prefix_groups (include/fasn.h): the prefixes of fasn_fwd_prefix_groups - their lengths ([num_groups] int32), their page ids
    ([num_groups, max_prefix_pages] int32) and the group of every batch element ([B] int32), all in device memory; reserved = 0"""
    _fields_ = [("prefix_lens", c_void_p), ("prefix_tables", c_void_p), ("prefix_group", c_void_p),
                ("num_groups", c_int32), ("max_prefix_pages", c_int32), ("reserved", c_int32)]


FASN_PREFIX_GROUPS_MAX = 1024   # include/fasn.h


class FasnError(RuntimeError):
    pass


_lib = None


# The K/V-cache ABI (include/fasn.h) in one description, which _kv_bindings(), the *_plan helpers below and kvcache.py's _forward / _append
# share. A name is the stem of its block plus a suffix made of the operands present: fasn_fwd_{stem}{suffix}[_workspace_bytes] and
# fasn_{stem}{suffix}_plan for a forward - suffix _fp8, then one of _tree / _window / _alibi - and fasn_{stem}{suffix}_append[_plan] for an
# append - suffix _fp8, _tree, then _rope. The operands follow the block in ABI order: a forward's in suffix order, an append's as
# fp8, rope, tree - so the 16-bit tree rope append takes (rope, tree) and the FP8 one (fp8, rope, tree). The one irregularity: there is no
# *_alibi_workspace_bytes, the ALiBi forward uses the base call's.
_KV_BLOCK = {"kvcache": KvCacheArgs, "kvprefill": KvPrefillArgs, "kvvarlen": KvVarlenArgs}
_KV_OPERAND = {"fp8": KvFp8, "tree": KvTree, "window": KvWindow, "alibi": AlibiSlopes, "rope": KvRope}
_KV_FORWARD_SETS = ((), ("alibi",), ("window",), ("tree",), ("fp8",), ("fp8", "window"), ("fp8", "tree"))   # packed: the first and ("window",)
_KV_APPENDS = (((), False), (("rope",), True), (("tree", "rope"), False), (("fp8",), False), (("fp8", "rope"), True),
               (("fp8", "tree", "rope"), True))   # (operands in suffix order, has a *_plan); packed: the first two
# "packed: the first ..." counts NAMES. The packed block also has the forward sets ("fp8",) and ("fp8", "window") and the appends ("fp8",)
# and ("fp8", "rope"): they have no names and are reached through the operand-set entry points (KvCall, _kv_call_bindings(), kv_call()
# below), which serve every named set as well.
_KV_KIND = {"kvcache": FASN_KV_CALL_DECODE, "kvprefill": FASN_KV_CALL_PREFILL, "kvvarlen": FASN_KV_CALL_PACKED}


def kv_stem(args):
    """the stem of the entry points that take the block `args`"""
    return next((stem for stem, block in _KV_BLOCK.items() if isinstance(args, block)), "kvcache")


def kv_forward_call(stem, fp8=None, tree=None, window=None, alibi=None):
    """(workspace-bytes name, its operands, forward name, plan name, their operands in ABI order) of the forward of `stem` under the
    operands that are not None: the FP8 operand, then the first there is of tree, window and ALiBi slopes"""
    one = ("_tree", tree) if tree is not None else ("_window", window) if window is not None else ("_alibi", alibi) if alibi is not None else ("", None)
    sfx = ("_fp8" if fp8 is not None else "") + one[0]
    operands = tuple(o for o in (fp8, one[1]) if o is not None)
    ws = (f"fasn_fwd_{stem}_workspace_bytes", ()) if sfx == "_alibi" else (f"fasn_fwd_{stem}{sfx}_workspace_bytes", operands)
    return (*ws, f"fasn_fwd_{stem}{sfx}", f"fasn_{stem}{sfx}_plan", operands)


def kv_append_call(stem, fp8=None, tree=None, rope=None):
    """(name, operands in ABI order: fp8, rope, tree) of the append of `stem` under the operands that are not None; the tree counts under
    rope only"""
    tree = tree if rope is not None else None
    sfx = ("_fp8" if fp8 is not None else "") + ("_tree" if tree is not None else "") + ("_rope" if rope is not None else "")
    return f"fasn_{stem}{sfx}_append", tuple(o for o in (fp8, rope, tree) if o is not None)


def _kv_bindings():
    """(name, restype, argtypes) of the 69 K/V-cache entry points, from the description above: per block the supported operand sets x
    {workspace_bytes, forward, plan} and the append kinds x {call, plan where there is one}; then the two commits of a token tree (16-bit
    and FP8 cache), which have a block of their own"""
    view, text = POINTER(View4), [c_char_p, c_size_t]
    launch = [c_void_p]                          # the stream
    forward = [c_void_p, c_size_t, c_void_p]     # workspace, its bytes, the stream
    types = {o: POINTER(t) for o, t in _KV_OPERAND.items()}
    for stem, block in _KV_BLOCK.items():
        packed = stem == "kvvarlen"
        for ops in (s for s in _KV_FORWARD_SETS if not packed or s in ((), ("window",))):
            ws, _, fwd, plan, operands = kv_forward_call(stem, **{o: types[o] for o in ops})
            head = [POINTER(block), *operands]
            if ops != ("alibi",):   # (the base call's, yielded with it)
                yield ws, c_size_t, head
            yield fwd, c_int32, head + forward
            yield plan, c_int32, head + text
        for ops, has_plan in _KV_APPENDS[:2] if packed else _KV_APPENDS:
            name, operands = kv_append_call(stem, **{o: types[o] for o in ops})
            head = [POINTER(block), *operands] + [view] * (3 if "rope" in ops else 2)   # (q_out,) k_new, v_new
            yield name, c_int32, head + launch
            if has_plan:
                yield f"{name}_plan", c_int32, head + text
    for name in ("fasn_kvcache_tree_commit", "fasn_kvcache_fp8_tree_commit"):
        yield name, c_int32, [POINTER(KvTreeCommit)] + launch


def _kv_call_bindings():
    """(name, restype, argtypes) of the five operand-set entry points: the call, then what the named entry points take behind their
    operands"""
    call, view, text = POINTER(KvCall), POINTER(View4), [c_char_p, c_size_t]
    append = [call, POINTER(KvRope), view, view, view]   # the call, rope, q_out, k_new, v_new
    yield "fasn_kv_forward_workspace_bytes", c_size_t, [call]
    yield "fasn_kv_forward", c_int32, [call, c_void_p, c_size_t, c_void_p]
    yield "fasn_kv_forward_plan", c_int32, [call] + text
    yield "fasn_kv_append", c_int32, append + [c_void_p]
    yield "fasn_kv_append_plan", c_int32, append + text


def _prefix_bindings(stem, operand):
    """(name, restype, argtypes) of the three entry points of a decode behind shared prefixes: a decode block and the prefix operand.
    They are no part of the K/V-cache description above - the operand belongs to no operand set - and have lists of their own."""
    head = [POINTER(KvCacheArgs), POINTER(operand)]
    yield f"fasn_fwd_{stem}_workspace_bytes", c_size_t, head
    yield f"fasn_fwd_{stem}", c_int32, head + [c_void_p, c_size_t, c_void_p]
    yield f"fasn_{stem}_plan", c_int32, head + [c_char_p, c_size_t]


def _shared_prefix_bindings():
    return _prefix_bindings("shared_prefix", SharedPrefix)


def _prefix_groups_bindings():
    return _prefix_bindings("prefix_groups", PrefixGroups)


def kv_call(args, fp8=None, tree=None, window=None, alibi=None):
    """the KvCall of the block `args` under the operands that are not None. The block and the operands live as long as the KvCall does."""
    c = KvCall(kind=_KV_KIND[kv_stem(args)], reserved=0, block=ctypes.cast(ctypes.pointer(args), c_void_p))
    for name, operand in (("fp8", fp8), ("tree", tree), ("window", window), ("alibi", alibi)):
        if operand is not None:
            setattr(c, name, ctypes.pointer(operand))
    c._block = args   # (the operands are kept by their pointer members; the block's address is a plain integer)
    return c


def load():
    """Load libfasn.so once; raise ImportError with the build recipe if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C {os.path.join(_HERE, 'csrc')}`) — there is no fallback path.")
    lib = ctypes.CDLL(LIB_PATH)
    missing = [s for s in EXPORTS if not hasattr(lib, s)]
    if missing:
        raise ImportError(f"{LIB_PATH} does not export {missing}; rebuild it from csrc/")
    lib.fasn_abi_version.restype = c_int32
    lib.fasn_strerror.restype = c_char_p
    lib.fasn_strerror.argtypes = [c_int32]
    lib.fasn_supported.restype = c_int32
    lib.fasn_supported.argtypes = [c_int32, c_int32, c_int32]
    lib.fasn_fwd.restype = c_int32
    lib.fasn_fwd.argtypes = [POINTER(FwdArgs), c_void_p]
    lib.fasn_fwd_path.restype = c_int32
    lib.fasn_fwd_path.argtypes = [POINTER(FwdArgs)]
    lib.fasn_bwd_path.restype = c_int32
    lib.fasn_bwd_path.argtypes = [POINTER(BwdArgs)]
    lib.fasn_fwd_workspace_bytes.restype = c_size_t
    lib.fasn_fwd_workspace_bytes.argtypes = [POINTER(FwdArgs)]
    lib.fasn_fwd_ws.restype = c_int32
    lib.fasn_fwd_ws.argtypes = [POINTER(FwdArgs), c_void_p, c_size_t, c_void_p]
    lib.fasn_bwd.restype = c_int32
    lib.fasn_bwd.argtypes = [POINTER(BwdArgs), c_void_p]
    lib.fasn_fwd_n.restype = c_int32
    lib.fasn_fwd_n.argtypes = [POINTER(FwdArgs), c_void_p, c_int64, c_int64, c_void_p, c_size_t, c_void_p]
    lib.fasn_bwd_dn_workspace_bytes.restype = c_size_t
    lib.fasn_bwd_dn_workspace_bytes.argtypes = [POINTER(BwdArgs)]
    lib.fasn_bwd_dn.restype = c_int32
    lib.fasn_bwd_dn.argtypes = [POINTER(BwdArgs), c_void_p, c_int64, c_int64, c_void_p, c_size_t, c_void_p]
    lib.fasn_rng_advance.restype = c_int32
    lib.fasn_rng_advance.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p]
    lib.fasn_bwd_workspace_bytes.restype = c_size_t
    lib.fasn_bwd_workspace_bytes.argtypes = [POINTER(BwdArgs)]
    lib.fasn_launch_plan.restype = c_int32
    lib.fasn_launch_plan.argtypes = [POINTER(BwdArgs), c_int32, c_char_p, c_size_t]
    lib.fasn_softmax_n_fwd.restype = c_int32
    lib.fasn_softmax_n_fwd.argtypes = [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_float, c_int32, c_void_p]
    lib.fasn_softmax_n_bwd.restype = c_int32
    lib.fasn_softmax_n_bwd.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int32, c_void_p]
    lib.fasn_moments.restype = c_int32
    lib.fasn_moments.argtypes = [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p]
    lib.fasn_softmax_n_plan.restype = c_int32
    lib.fasn_softmax_n_plan.argtypes = [c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int32, c_char_p, c_size_t]
    lib.fasn_moments_plan.restype = c_int32
    lib.fasn_moments_plan.argtypes = [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int32, c_char_p, c_size_t]
    lib.fasn_fwd_varlen.restype = c_int32
    lib.fasn_fwd_varlen.argtypes = [POINTER(FwdArgs), POINTER(Varlen), c_void_p, c_int64, c_void_p]
    lib.fasn_bwd_varlen.restype = c_int32
    lib.fasn_bwd_varlen.argtypes = [POINTER(BwdArgs), POINTER(Varlen), c_void_p]
    lib.fasn_varlen_plan.restype = c_int32
    lib.fasn_varlen_plan.argtypes = [POINTER(BwdArgs), POINTER(Varlen), c_int32, c_char_p, c_size_t]
    lib.fasn_fwd_varlen_window.restype = c_int32
    lib.fasn_fwd_varlen_window.argtypes = [POINTER(FwdArgs), POINTER(Varlen), POINTER(KvWindow), c_void_p, c_int64, c_void_p]
    lib.fasn_bwd_varlen_window.restype = c_int32
    lib.fasn_bwd_varlen_window.argtypes = [POINTER(BwdArgs), POINTER(Varlen), POINTER(KvWindow), c_void_p]
    lib.fasn_varlen_window_plan.restype = c_int32
    lib.fasn_varlen_window_plan.argtypes = [POINTER(BwdArgs), POINTER(Varlen), POINTER(KvWindow), c_int32, c_char_p, c_size_t]
    lib.fasn_varlen_rope.restype = c_int32
    lib.fasn_varlen_rope.argtypes = [POINTER(FwdArgs), POINTER(Varlen), POINTER(KvRope), POINTER(View4), POINTER(View4), c_int32, c_void_p]
    lib.fasn_varlen_rope_plan.restype = c_int32
    lib.fasn_varlen_rope_plan.argtypes = [POINTER(FwdArgs), POINTER(Varlen), POINTER(KvRope), POINTER(View4), POINTER(View4), c_int32, c_char_p, c_size_t]
    for name, restype, argtypes in (*_kv_bindings(), *_kv_call_bindings(), *_shared_prefix_bindings(), *_prefix_groups_bindings()):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    ver = lib.fasn_abi_version()
    if ver != FASN_ABI_VERSION:
        raise ImportError(f"libfasn ABI version {ver} != expected {FASN_ABI_VERSION}; rebuild csrc/")
    _lib = lib
    return lib


_PLAN_BYTES = 8192   # the one buffer size of every plan read here (the longest plan text of the library is a fraction of it)


def _plan(what, *operands, described=False):
    """The launches the entry point `what` records for `operands`, as (kernel name with template arguments, grid, block, lds bytes): the one
    reader of the plan lines "name grid=G block=T lds=L cfg=C". `described`: the kernel as family<cfg>, where the line has a cfg."""
    buf = ctypes.create_string_buffer(_PLAN_BYTES)
    rc = getattr(load(), what)(*operands, buf, len(buf))
    if rc < 0:
        check(rc, what)
    out = []
    for line in buf.value.decode().splitlines():
        name, g, b, l, cfg = line.rsplit(" ", 4)
        cfg = cfg.split("=", 1)[1]
        if described and cfg != "-":
            name = f"{name.split('<', 1)[0]}<{cfg}>"
        out.append((name, int(g.split("=")[1]), int(b.split("=")[1]), int(l.split("=")[1])))
    return out


_kv_plan = _plan   # (the name the cache tests' support module, tests/kv_layout.py, reads plans by)

def launch_plan(args, which):
    """The kernels fasn_fwd (FASN_PLAN_FWD), fasn_bwd (FASN_PLAN_BWD) or fasn_fwd_ws (FASN_PLAN_FWD_WS) would launch for `args` (a BwdArgs;
    the forward plans read only its .fwd part): a list of (kernel name with template arguments, grid, block, lds bytes). Nothing is
    launched and no device is touched (include/fasn.h: fasn_launch_plan)."""
    return _plan("fasn_launch_plan", args, which)


def launch_plan_described(args, which):
    """The same plan as (kernel family<named template arguments>, grid, block, lds bytes): the `cfg` field of the plan lines (ABI 6) names the
    positional template arguments - fasn_fwd_kernel<bf16,D=64,QB=2,plain,OCC=2,NW=4,RING=2,SEED=2> instead of
    fasn_fwd_kernel<fasn::bf16_tag, 64, 2, 0, 2, 4, 0, 0, 2, 0, 2, 1, 0, 0>. What bench.py prints as roofline.kernels."""
    return _plan("fasn_launch_plan", args, which, described=True)


def _kv_forward_plan(stem, args, **operands):
    *_, plan, ops = kv_forward_call(stem, **operands)
    return _plan(plan, args, *ops)


def _kv_append_plan(args, q_out, k_new, v_new, **operands):
    name, ops = kv_append_call(kv_stem(args), **operands)
    return _plan(f"{name}_plan", args, *ops, q_out, k_new, v_new)


def varlen_plan(args, varlen, which):
    """The kernels fasn_fwd_varlen (FASN_PLAN_FWD) or fasn_bwd_varlen (FASN_PLAN_BWD) would launch for `args` (a BwdArgs that describes the
    packed operands) under `varlen` (a Varlen), as launch_plan returns them. Nothing is launched."""
    return _plan("fasn_varlen_plan", args, varlen, which)


def varlen_window_plan(args, varlen, win, which):
    """The kernels fasn_fwd_varlen_window (FASN_PLAN_FWD) or fasn_bwd_varlen_window (FASN_PLAN_BWD) would launch for `args` and `varlen`
    under `win` (a KvWindow), as launch_plan returns them; varlen_plan's with a window >= max_seqlen_k. Nothing is launched."""
    return _plan("fasn_varlen_window_plan", args, varlen, win, which)


def varlen_rope_plan(args, varlen, rope, q_out, k_out, inverse=0):
    """The one launch of fasn_varlen_rope for `args` (a FwdArgs that describes the packed operands; q and k are the sources) and `varlen`
    under `rope` (a KvRope) into the views `q_out` / `k_out`, as launch_plan returns it. Nothing is launched."""
    return _plan("fasn_varlen_rope_plan", args, varlen, rope, q_out, k_out, inverse)


def kvcache_plan(args, alibi=None):
    """The kernels fasn_fwd_kvcache would launch for `args` (a KvCacheArgs), as launch_plan returns them; with `alibi` (an AlibiSlopes)
    those of fasn_fwd_kvcache_alibi. Nothing is launched."""
    return _kv_forward_plan("kvcache", args, alibi=alibi)


def kvprefill_plan(args, alibi=None):
    """The kernels fasn_fwd_kvprefill would launch for `args` (a KvPrefillArgs), as launch_plan returns them; with `alibi` (an AlibiSlopes)
    those of fasn_fwd_kvprefill_alibi. Nothing is launched."""
    return _kv_forward_plan("kvprefill", args, alibi=alibi)


def kvvarlen_plan(args):
    """The kernels fasn_fwd_kvvarlen would launch for `args` (a KvVarlenArgs), as launch_plan returns them. Nothing is launched."""
    return _kv_forward_plan("kvvarlen", args)


def kvvarlen_window_plan(args, win):
    """The kernels fasn_fwd_kvvarlen_window would launch for `args` (a KvVarlenArgs) under `win` (a KvWindow), as launch_plan returns
    them. Nothing is launched."""
    return _kv_forward_plan("kvvarlen", args, window=win)


def kvcache_window_plan(args, win):
    """The kernels fasn_fwd_kvcache_window would launch for `args` (a KvCacheArgs) under `win` (a KvWindow), as launch_plan returns them.
    Nothing is launched."""
    return _kv_forward_plan("kvcache", args, window=win)


def kvprefill_window_plan(args, win):
    """The kernels fasn_fwd_kvprefill_window would launch for `args` (a KvPrefillArgs) under `win` (a KvWindow), as launch_plan returns
    them. Nothing is launched."""
    return _kv_forward_plan("kvprefill", args, window=win)


def kvtree_plan(args, tree):
    """The kernels fasn_fwd_kvcache_tree (`args` a KvCacheArgs) or fasn_fwd_kvprefill_tree (a KvPrefillArgs) would launch under `tree` (a
    KvTree), as launch_plan returns them. Nothing is launched."""
    return _kv_forward_plan(kv_stem(args), args, tree=tree)


def kvfp8_plan(args, fp8):
    """The kernels fasn_fwd_kvcache_fp8 (`args` a KvCacheArgs) or fasn_fwd_kvprefill_fp8 (a KvPrefillArgs) would launch under `fp8` (a
    KvFp8), as launch_plan returns them. Nothing is launched."""
    return _kv_forward_plan(kv_stem(args), args, fp8=fp8)


def kvfp8_window_plan(args, fp8, win):
    """The kernels fasn_fwd_kvcache_fp8_window (`args` a KvCacheArgs) or fasn_fwd_kvprefill_fp8_window (a KvPrefillArgs) would launch under
    `fp8` (a KvFp8) and `win` (a KvWindow), as launch_plan returns them. Nothing is launched."""
    return _kv_forward_plan(kv_stem(args), args, fp8=fp8, window=win)


def kvfp8_rope_plan(args, fp8, rope, q_out, k_new=None, v_new=None):
    """The one launch of fasn_kvcache_fp8_rope_append (`args` a KvCacheArgs) or fasn_kvprefill_fp8_rope_append (a KvPrefillArgs) under `fp8`
    (a KvFp8) and `rope` (a KvRope), as launch_plan returns it. Nothing is launched."""
    return _kv_append_plan(args, q_out, k_new, v_new, fp8=fp8, rope=rope)


def kvfp8_tree_plan(args, fp8, tree):
    """The kernels fasn_fwd_kvcache_fp8_tree (`args` a KvCacheArgs) or fasn_fwd_kvprefill_fp8_tree (a KvPrefillArgs) would launch under `fp8`
    (a KvFp8) and `tree` (a KvTree), as launch_plan returns them. Nothing is launched."""
    return _kv_forward_plan(kv_stem(args), args, fp8=fp8, tree=tree)


def kvfp8_tree_rope_plan(args, fp8, rope, tree, q_out, k_new=None, v_new=None):
    """The one launch of fasn_kvcache_fp8_tree_rope_append (`args` a KvCacheArgs) or fasn_kvprefill_fp8_tree_rope_append (a KvPrefillArgs)
    under `fp8` (a KvFp8), `rope` (a KvRope) and `tree` (a KvTree), as launch_plan returns it. Nothing is launched."""
    return _kv_append_plan(args, q_out, k_new, v_new, fp8=fp8, rope=rope, tree=tree)


def kv_call_plan(call):
    """The kernels fasn_kv_forward would launch for `call` (a KvCall), as launch_plan returns them: for a set a named entry point serves,
    that entry point's plan. Nothing is launched."""
    return _plan("fasn_kv_forward_plan", call)


def kv_call_append_plan(call, rope=None, q_out=None, k_new=None, v_new=None):
    """The one launch of fasn_kv_append for `call` (a KvCall) - with `rope` (a KvRope) the rotary append into `q_out` - as launch_plan
    returns it. Nothing is launched."""
    return _plan("fasn_kv_append_plan", call, rope, q_out, k_new, v_new)


def kvfp8_varlen_plan(args, fp8, win=None):
    """The kernels of the packed forward over an FP8 cache - `args` a KvVarlenArgs, `fp8` a KvFp8, `win` a KvWindow or None - as
    launch_plan returns them (fasn_kv_forward_plan: the set has no named entry point). Nothing is launched."""
    return kv_call_plan(kv_call(args, fp8=fp8, window=win))


def kvfp8_varlen_append_plan(args, fp8, k_new, v_new, rope=None, q_out=None):
    """The one launch of the packed quantising append (`rope` None) or of the packed rotate-quantise-append (`rope` a KvRope, `q_out` the
    rotated queries' view) over an FP8 cache, as launch_plan returns it (fasn_kv_append_plan). Nothing is launched."""
    return kv_call_append_plan(kv_call(args, fp8=fp8), rope, q_out, k_new, v_new)


def kvrope_plan(args, rope, q_out, k_new=None, v_new=None):
    """The one launch of fasn_kvcache_rope_append (`args` a KvCacheArgs), fasn_kvprefill_rope_append (a KvPrefillArgs) or
    fasn_kvvarlen_rope_append (a KvVarlenArgs) under `rope` (a KvRope), as launch_plan returns it. Nothing is launched."""
    return _kv_append_plan(args, q_out, k_new, v_new, rope=rope)


def shared_prefix_plan(args, prefix):
    """The three launches of fasn_fwd_shared_prefix for `args` (a KvCacheArgs) behind `prefix` (a SharedPrefix) - the prefix pass, the
    suffix pass, the combine - as launch_plan returns them. Nothing is launched."""
    return _plan("fasn_shared_prefix_plan", args, prefix)


def prefix_groups_plan(args, groups):
    """The four launches of fasn_fwd_prefix_groups for `args` (a KvCacheArgs) behind `groups` (a PrefixGroups) - the schedule kernel, the
    prefix pass, the suffix pass, the combine - as launch_plan returns them. Nothing is launched."""
    return _plan("fasn_prefix_groups_plan", args, groups)


def softmax_plan(which, a, b, c, rows, cols, a_stride, b_stride, c_stride, dtype):
    """The one launch of fasn_softmax_n_fwd (`which` = FASN_ROW_FWD: a, b = the addresses of x and y, c is not read) or fasn_softmax_n_bwd
    (FASN_ROW_BWD: y, dy, dx) for these rows, columns, row strides (in elements) and FASN_DTYPE_*, as launch_plan returns it. Only the
    alignment of the addresses is read. Nothing is launched."""
    return _plan("fasn_softmax_n_plan", which, a, b, c, rows, cols, a_stride, b_stride, c_stride, dtype)


def moments_plan(x, sums, rows, cols, row_stride, dtype):
    """The one launch of fasn_moments for these arguments (x, sums: addresses), as launch_plan returns it; the grid is the number of
    chunks a row is cut into. Nothing is launched."""
    return _plan("fasn_moments_plan", x, sums, rows, cols, row_stride, dtype)


def check(rc, what):
    if rc != 0:
        msg = load().fasn_strerror(rc).decode()
        raise FasnError(f"{what} failed: {msg} (code {rc})")
