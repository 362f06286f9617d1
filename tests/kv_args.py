"""What the K/V-cache tests without a GPU share, and the GPU suites borrow for their plan checks: builders of the C ABI's argument blocks
and operands over fake, aligned pointers (nothing built here is ever dereferenced), the shapes whose launch plans are recorded, and the
rules of the host-layer check-order matrices. A plain module: no tests, importable without a GPU."""
import ctypes
import hashlib

DUMMY = 1 << 20
INT_MAX = 2 ** 31 - 1
BIG = ctypes.c_size_t(-1).value
CAPACITY = 256 * 32   # of the default blocks below


# ---------------------------------------------------------------- argument blocks
def _kv(a, B=4, H=64, Hkv=8, Sq=1, D=64, page=256, max_pages=32, dtype=1, paged=True, seqlens=DUMMY):
    """the fields of a fasn_kvcache_args, embedded or free-standing"""
    for v in (a.q, a.o):
        v.ptr = DUMMY
        for i, s in enumerate((H * Sq * D, Sq * D, D, 1)):
            v.stride[i] = s
    a.lse = DUMMY
    a.k_cache = a.v_cache = DUMMY
    for i, s in enumerate((page * Hkv * D, Hkv * D, D)):
        a.k_stride[i] = a.v_stride[i] = s
    a.block_table = DUMMY if paged else None
    a.block_table_stride, a.max_pages = max_pages, max_pages
    a.seqlens, a.seqlen_add, a.page_size = seqlens, 0, page
    a.B, a.H, a.kv_group, a.Sq, a.D, a.dtype = B, H, H // Hkv, Sq, D, dtype
    a.scale, a.softmax_n, a.causal = D ** -0.5, 1.0, 1
    return a


def _args_decode(pkg, **kw):
    return _kv(pkg._lib.KvCacheArgs(), **kw)


def _args_prefill(pkg, q_seqlens=None, **kw):
    pa = pkg._lib.KvPrefillArgs()
    _kv(pa.kv, **kw)
    pa.q_seqlens = q_seqlens
    return pa


def _args_varlen(pkg, T=64, cu=DUMMY + 8192, **kw):
    """a fasn_kvvarlen_args over _kv's block: B sequences, Sq = max_seqlen_q, q / o as [1, H, T, D] views of [T, H, D]"""
    va = pkg._lib.KvVarlenArgs()
    a = _kv(va.pf.kv, **kw)
    for v in (a.q, a.o):
        for i, s in enumerate((0, a.D, a.H * a.D, 1)):
            v.stride[i] = s
    va.pf.q_seqlens = None
    va.cu_seqlens_q, va.total_tokens, va.reserved = cu, T, 0
    return va


# ---------------------------------------------------------------- operands
def _win(pkg, window=128, reserved=0):
    return pkg._lib.KvWindow(window=window, reserved=reserved)


def _slopes(pkg, ptr=DUMMY + 512, sb=0, sh=1):
    s = pkg._lib.AlibiSlopes()
    s.slopes, s.stride_b, s.stride_h = ptr, sb, sh
    return s


def _rope(pkg, rows=CAPACITY, rd=64, table_dtype=2, interleaved=0, row_stride=None, cos=DUMMY, sin=DUMMY):
    r = pkg._lib.KvRope()
    r.cos, r.sin = cos, sin
    r.row_stride = rd // 2 if row_stride is None else row_stride
    r.rows, r.rotary_dim, r.table_dtype, r.interleaved = rows, rd, table_dtype, interleaved
    return r


def _view(pkg, heads, Sq, D, ptr=DUMMY):
    v = pkg._lib.View4()
    v.ptr = ptr
    for i, s in enumerate((heads * Sq * D, Sq * D, D, 1)):
        v.stride[i] = s
    return v


def _tview(pkg, heads, D, ptr=DUMMY):
    """a [1, heads, T, D] view of a [T, heads, D] buffer"""
    v = pkg._lib.View4()
    v.ptr = ptr
    for i, s in enumerate((0, D, heads * D, 1)):
        v.stride[i] = s
    return v


def _renamed(plan, old, new):
    return [(k[0].replace(old + "<", new + "<"),) + tuple(k[1:]) for k in plan]


# ---------------------------------------------------------------- the shapes whose plans are recorded
DECODE_CASES = {
    "gqa": dict(B=4, H=64, Hkv=8, Sq=1, D=64, page=256, max_pages=32),
    "mha": dict(B=64, H=16, Hkv=16, Sq=1, D=128, page=256, max_pages=32),
}

# prefill: one split (many row blocks) / several splits (small batch, long cache)
PREFILL_CASES = {
    "gqa_prompts": dict(B=4, H=64, Hkv=8, Sq=2048, D=64, page=256, max_pages=32),
    "mha_prompts": dict(B=8, H=16, Hkv=16, Sq=4096, D=128, page=256, max_pages=16),
    "gqa_chunk_long_cache": dict(B=1, H=64, Hkv=8, Sq=64, D=64, page=256, max_pages=128),
    "mha_chunk_long_cache": dict(B=2, H=16, Hkv=16, Sq=256, D=128, page=256, max_pages=64),
}
PREFILL_SPLIT = {"gqa_prompts": False, "mha_prompts": False, "gqa_chunk_long_cache": True, "mha_chunk_long_cache": True}


def items_max(B, max_seqlen_q, T, PB):
    return min(B * -(-max_seqlen_q // PB), T // PB + B)


def plan_cases():
    """each head dim x G in {1, 8} x a small step (several splits: few items, long cache) and a large one (one split)"""
    out = {}
    for D in (32, 64, 128, 256):
        for H, Hkv in ((8, 8), (64, 8)):
            out[f"D{D}_G{H // Hkv}_small"] = dict(B=4, H=H, Hkv=Hkv, Sq=48, D=D, page=256, max_pages=64, T=64)
            out[f"D{D}_G{H // Hkv}_large"] = dict(B=257, H=H, Hkv=Hkv, Sq=4096, D=D, page=256, max_pages=32, T=4352)
    return out


# ---------------------------------------------------------------- the check-order matrices: valid blocks, and rules that break one check each
# valid blocks: fields of fasn_kvcache_args (`qlens`: the prefill block also carries q_seqlens). Every block has seqlen_add = Sq and is
# called with k_new / v_new, so the rotary plan is the one with the append.
BASES = {
    "dec_paged": dict(B=4, H=64, Hkv=8, Sq=1, D=64, page=256, max_pages=32, dtype=1, paged=True, qlens=False),
    "dec_dense": dict(B=3, H=8, Hkv=2, Sq=3, D=128, page=1000, max_pages=1, dtype=0, paged=False, qlens=False),
    "pre_paged_qlens": dict(B=2, H=12, Hkv=4, Sq=300, D=64, page=128, max_pages=40, dtype=1, paged=True, qlens=True),
    "pre_dense_oddpage": dict(B=2, H=16, Hkv=16, Sq=150, D=32, page=1001, max_pages=1, dtype=0, paged=False, qlens=False),
    "d256": dict(B=4, H=64, Hkv=8, Sq=1, D=256, page=256, max_pages=32, dtype=1, paged=True, qlens=False),
    "g128": dict(B=2, H=128, Hkv=1, Sq=1, D=64, page=64, max_pages=64, dtype=0, paged=True, qlens=False),
}


class Case:
    """One call's operands: the argument block (`kv`; `null`: a NULL block), q_seqlens, and the operands of the ALiBi, window and rotary
    entry points. A rule is a function that breaks one check on it."""

    def __init__(self, L, c):
        B, H, Hkv, Sq, D = c["B"], c["H"], c["Hkv"], c["Sq"], c["D"]
        self.L, self.null = L, False
        self.pa = L.KvPrefillArgs()
        a = self.kv = self.pa.kv
        for v in (a.q, a.o):
            self._view(v, H, Sq, D)
        a.lse = DUMMY
        a.k_cache = a.v_cache = DUMMY
        for i, s in enumerate((c["page"] * Hkv * D, Hkv * D, D)):
            a.k_stride[i] = a.v_stride[i] = s
        a.block_table = DUMMY if c["paged"] else None
        a.block_table_stride, a.max_pages = c["max_pages"], c["max_pages"]
        a.seqlens, a.seqlen_add, a.page_size = DUMMY, Sq, c["page"]
        a.B, a.H, a.kv_group, a.Sq, a.D, a.dtype = B, H, H // Hkv, Sq, D, c["dtype"]
        a.scale, a.softmax_n, a.causal = D ** -0.5, 1.0, 1
        self.qlens = DUMMY + 4096 if c["qlens"] else None
        self.alibi = L.AlibiSlopes(slopes=DUMMY + 512, stride_b=0, stride_h=1)
        self.win = L.KvWindow(window=100, reserved=0)
        self.rope = L.KvRope(cos=DUMMY, sin=DUMMY, row_stride=16, rows=c["page"] * c["max_pages"], rotary_dim=32, table_dtype=2, interleaved=0)
        self.qo, self.kn, self.vn = (self._view(L.View4(), h, Sq, D) for h in (H, Hkv, Hkv))
        self.has_alibi = self.has_win = self.has_rope = True

    @staticmethod
    def _view(v, heads, Sq, D):
        v.ptr = DUMMY
        for i, s in enumerate((heads * Sq * D, Sq * D, D, 1)):
            v.stride[i] = s
        return v


def _set(**fields):
    def rule(c):
        for k, v in fields.items():
            setattr(c.kv, k, v)
    return rule


def _on(what, **fields):
    def rule(c):
        for k, v in fields.items():
            setattr(getattr(c, what), k, v)
    return rule


def _stride(what, i, value):
    def rule(c):
        getattr(c.kv, what).stride[i] = value
    return rule


def _cache_stride(what, i, value):
    def rule(c):
        getattr(c.kv, what)[i] = value(c.kv) if callable(value) else value
    return rule


def _attr(name, value):
    def rule(c):
        setattr(c, name, value)
    return rule


def _rows_over(c):   # decode: one row more than a workgroup has
    c.kv.Sq = 128 // c.kv.kv_group + 1
    c.kv.seqlen_add = c.kv.Sq


def _capacity(c, cap_paged, cap_dense):
    if c.kv.block_table:
        c.kv.page_size, c.kv.max_pages, c.kv.block_table_stride = 64, cap_paged // 64, cap_paged // 64
    else:
        c.kv.page_size = cap_dense


def _cap_over(c):
    _capacity(c, 2 ** 31, INT_MAX - 100)


def _cap_edge_add(c):   # the largest capacity, and 200 rows more: the decode bound looks at seqlen_add
    _capacity(c, 2 ** 31 - 192, INT_MAX - 128)
    c.kv.seqlen_add = 200


def _cap_edge_sq(c):   # ... the prefill bound looks at Sq
    _capacity(c, 2 ** 31 - 192, INT_MAX - 128)
    c.kv.Sq, c.kv.seqlen_add = 200, 0


def _grid_over(c):
    c.kv.B, c.kv.H = 1 << 16, c.kv.kv_group << 16


def _kn_only(c):
    c.vn = None


def _no_new_rows(c):
    c.kn = c.vn = None
    c.kv.seqlen_add = 0


# the rules of the builders in the order of their checks; the operand rules follow the base rules
BASE_RULES = [
    ("args_null", _attr("null", True)),
    ("B_0", _set(B=0)), ("H_0", _set(H=0)), ("Sq_0", _set(Sq=0)), ("D_0", _set(D=0)), ("page_0", _set(page_size=0)),
    ("dtype_f32", _set(dtype=2)),
    ("D_96", _set(D=96)),
    ("group_7", _set(kv_group=7)),
    ("n_negative", _set(softmax_n=-1.0)), ("scale_inf", _set(scale=float("inf"))),
    ("seqlens_null", _set(seqlens=None)), ("k_cache_null", _set(k_cache=None)), ("v_cache_null", _set(v_cache=None)),
    ("seqlens_odd", _set(seqlens=DUMMY + 2)), ("block_table_odd", _set(block_table=DUMMY + 2)), ("q_seqlens_odd", _attr("qlens", DUMMY + 2)),
    ("seqlen_add_other", lambda c: setattr(c.kv, "seqlen_add", c.kv.Sq + 1)),
    ("q_null", lambda c: setattr(c.kv.q, "ptr", None)),
    ("q_stride3", _stride("q", 3, 2)), ("q_odd", lambda c: setattr(c.kv.q, "ptr", DUMMY + 2)), ("q_stride_mod8", _stride("q", 1, 68)),
    ("o_null", lambda c: setattr(c.kv.o, "ptr", None)),
    ("o_stride3", _stride("o", 3, 2)), ("o_odd", lambda c: setattr(c.kv.o, "ptr", DUMMY + 2)), ("o_stride_mod8", _stride("o", 2, 68)),
    ("k_cache_odd", _set(k_cache=DUMMY + 8)), ("v_cache_odd", _set(v_cache=DUMMY + 8)),
    ("k_stride_mod8", _cache_stride("k_stride", 2, lambda a: a.D + 4)), ("v_stride_negative", _cache_stride("v_stride", 0, -8)),
    ("max_pages_0", _set(max_pages=0)), ("table_stride_short", lambda c: setattr(c.kv, "block_table_stride", c.kv.max_pages - 1)),
    ("page_48", _set(page_size=48)),
    ("rows_over", _rows_over), ("group_256", _set(kv_group=256, H=256)),
    ("capacity_over", _cap_over), ("capacity_plus_add", _cap_edge_add), ("capacity_plus_Sq", _cap_edge_sq),
    ("k_row_huge", _cache_stride("k_stride", 1, 1 << 24)), ("v_row_huge", _cache_stride("v_stride", 1, 1 << 24)),
    ("k_row_short", _cache_stride("k_stride", 1, lambda a: a.D - 8)), ("v_row_short", _cache_stride("v_stride", 1, lambda a: a.D - 8)),
    ("n_odd", _set(n=DUMMY + 2)), ("n_stride_negative", _set(n=DUMMY, n_stride_b=-1)), ("n_stride_over", _set(n=DUMMY, n_stride_b=1 << 31)),
    ("grid_over", _grid_over),
]


def _plan(fn, *operands):
    buf = ctypes.create_string_buffer(4096)
    rc = fn(*operands, buf, len(buf))
    if rc < 0:
        return str(rc)
    assert rc == len(buf.value) > 0
    return "#" + hashlib.sha1(buf.value).hexdigest()[:8]
