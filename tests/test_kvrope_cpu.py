"""Rotary rotate-and-append on the K/V-cache calls, without a GPU: exports and the layout of fasn_kv_rope, the validation codes of the four
new entry points (fake, aligned pointers: validation comes before any HIP call), the one-launch plan - shapes only, smaller without
k_new - the register table of the 8 new kernels, and the front end's refusals."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kv_args as ka   # noqa: E402

DUMMY = ka.DUMMY
NEW = ("fasn_kvcache_rope_append", "fasn_kvprefill_rope_append", "fasn_kvcache_rope_append_plan", "fasn_kvprefill_rope_append_plan")
DIMS = (32, 64, 128, 256)
TAGS = {0: "fasn::f16_tag", 1: "fasn::bf16_tag"}
EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED = -1, -2, -3, -4, -5, -7
CAPACITY, _rope, _view = ka.CAPACITY, ka._rope, ka._view


def _header():
    text = open(os.path.join(ROOT, "include", "fasn.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_are_exported_and_bound(pkg):
    import flash_attention_softmax_n_amd as shim
    lib = shim._lib.load()
    declared = set(re.findall(r"\b(fasn_[a-z0-9_]+)\s*\(", _header()))
    assert set(shim._lib.EXPORTS) == declared
    for name in NEW:
        assert name in declared and name in shim._lib.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.fasn_abi_version() == 6


def test_struct_layout_matches_the_header(pkg):
    body = re.search(r"typedef struct fasn_kv_rope \{(.*?)\} fasn_kv_rope;", _header(), flags=re.S).group(1)
    fields = [(t.strip(), n) for t, n in re.findall(r"([a-z0-9_ ]+?[ *]+)([a-z_]+);", body)]
    assert fields == [("const void*", "cos"), ("const void*", "sin"), ("int64_t", "row_stride"), ("int32_t", "rows"), ("int32_t", "rotary_dim"),
                      ("int32_t", "table_dtype"), ("int32_t", "interleaved")], fields
    R = pkg._lib.KvRope
    assert [f[0] for f in R._fields_] == [n for _t, n in fields]
    assert (R.cos.offset, R.sin.offset, R.row_stride.offset, R.rows.offset, R.rotary_dim.offset, R.table_dtype.offset, R.interleaved.offset) == (
        0, 8, 16, 24, 28, 32, 36) and ctypes.sizeof(R) == 40
    # the argument blocks kept their layouts: the operand travels beside them
    assert pkg._lib.KvPrefillArgs.kv.offset == 0 and pkg._lib.KvPrefillArgs.q_seqlens.offset == ctypes.sizeof(pkg._lib.KvCacheArgs)
    assert pkg._lib.KvCacheArgs.n_stride_h.offset + 8 == ctypes.sizeof(pkg._lib.KvCacheArgs)


def _callers(pkg, which, how):
    lib = pkg._lib.load()
    stem = "kvcache" if which == "dec" else "kvprefill"
    buf = ctypes.create_string_buffer(4096)

    def call(a, r, qo, kn, vn):
        if how == "plan":
            rc = getattr(lib, f"fasn_{stem}_rope_append_plan")(a, r, qo, kn, vn, buf, len(buf))
            return rc if rc < 0 else 0
        return getattr(lib, f"fasn_{stem}_rope_append")(a, r, qo, kn, vn, None)
    return call


@pytest.mark.parametrize("which", ["dec", "pre"])
def test_validation_codes(pkg, which):
    make, kv = (ka._args_decode, lambda a: a) if which == "dec" else (ka._args_prefill, lambda a: a.kv)
    H, Hkv, Sq, D = 64, 8, 1, 64

    def appended(**kw):
        a = make(pkg, **kw)
        kv(a).seqlen_add = kv(a).Sq
        return a
    qo, kn = _view(pkg, H, Sq, D), _view(pkg, Hkv, Sq, D)
    # (an accepted call would launch: the calls that launch are only ever refused here, the accepted ones are recorded by the plan calls)
    for how in ("run", "plan"):
        call = _callers(pkg, which, how)
        good = _rope(pkg)
        # every base code, reached through the new entry points, with a good and with a bad operand: the base arguments come first
        for r in (good, None, _rope(pkg, rd=8)):
            assert call(None, r, qo, kn, kn) == EINVAL
            assert call(make(pkg, B=0), r, qo, kn, kn) == EINVAL
            assert call(make(pkg, dtype=2), r, qo, kn, kn) == EDTYPE and call(make(pkg, dtype=3), r, qo, kn, kn) == EDTYPE
            assert call(make(pkg, D=96), r, qo, kn, kn) == EHEADDIM
            assert call(make(pkg, page=48), r, qo, kn, kn) == EUNSUPPORTED
            a = make(pkg)
            kv(a).kv_group = 7
            assert call(a, r, qo, kn, kn) == EINVAL
            a = make(pkg)
            kv(a).q.ptr = kv(a).q.ptr + 2
            assert call(a, r, qo, kn, kn) == EALIGN
            a = make(pkg)
            kv(a).k_stride[1] = 8 * 64 + 4
            assert call(a, r, qo, kn, kn) == EALIGN
            a = make(pkg)
            kv(a).q.stride[3] = 2
            assert call(a, r, qo, kn, kn) == ESTRIDE
            assert call(make(pkg, seqlens=None), r, qo, kn, kn) == EINVAL
        # then the operand. NULL rope, cos, sin, q_out
        assert call(appended(), None, qo, kn, kn) == EINVAL
        assert call(appended(), _rope(pkg, cos=None), qo, kn, kn) == EINVAL
        assert call(appended(), _rope(pkg, sin=None), qo, kn, kn) == EINVAL
        assert call(appended(), good, None, kn, kn) == EINVAL
        # k_new and v_new come together
        assert call(appended(), good, qo, kn, None) == EINVAL and call(appended(), good, qo, None, kn) == EINVAL
        # k_new / v_new given: seqlen_add == Sq
        assert call(make(pkg), good, qo, kn, kn) == EINVAL
        # rotary_dim in [16, D], a multiple of 16
        for rd in (0, 8, 24, 40, 80, 128, -16):
            assert call(appended(), _rope(pkg, rd=rd, row_stride=64), qo, kn, kn) == EINVAL, rd
        # rows >= capacity
        assert call(appended(), _rope(pkg, rows=CAPACITY - 1), qo, kn, kn) == EINVAL
        assert call(appended(), _rope(pkg, rows=0), qo, kn, kn) == EINVAL
        # interleaved 0 or 1
        assert call(appended(), _rope(pkg, interleaved=2), qo, kn, kn) == EINVAL and call(appended(), _rope(pkg, interleaved=-1), qo, kn, kn) == EINVAL
        # table dtype: fp32 or the dtype of args
        assert call(appended(dtype=1), _rope(pkg, table_dtype=0), qo, kn, kn) == EDTYPE
        assert call(appended(dtype=0), _rope(pkg, table_dtype=1), qo, kn, kn) == EDTYPE
        assert call(appended(), _rope(pkg, table_dtype=3), qo, kn, kn) == EDTYPE
        # alignment of the tables
        assert call(appended(), _rope(pkg, cos=DUMMY + 4), qo, kn, kn) == EALIGN and call(appended(), _rope(pkg, sin=DUMMY + 8), qo, kn, kn) == EALIGN
        assert call(appended(), _rope(pkg, row_stride=34), qo, kn, kn) == EALIGN            # 136 bytes of fp32
        assert call(appended(), _rope(pkg, table_dtype=1, row_stride=36), qo, kn, kn) == EALIGN   # 72 bytes of bf16
        assert call(appended(), _rope(pkg, row_stride=16), qo, kn, kn) == EINVAL            # rows overlap
        # q_out: the codes of q
        v = _view(pkg, H, Sq, D)
        v.stride[3] = 2
        assert call(appended(), good, v, kn, kn) == ESTRIDE
        assert call(appended(), good, _view(pkg, H, Sq, D, ptr=DUMMY + 2), kn, kn) == EALIGN
        assert call(appended(), good, _view(pkg, H, Sq, D, ptr=None), kn, kn) == EINVAL
        v = _view(pkg, H, Sq, D)
        v.stride[1] = 68
        assert call(appended(), good, v, kn, kn) == EALIGN
        # k_new / v_new: the append's codes
        v = _view(pkg, Hkv, Sq, D)
        v.stride[3] = 2
        assert call(appended(), good, qo, v, kn) == ESTRIDE and call(appended(), good, qo, kn, v) == ESTRIDE
        assert call(appended(), good, qo, _view(pkg, Hkv, Sq, D, ptr=DUMMY + 2), kn) == EALIGN
        if how == "plan":   # accepted: every legal rotary_dim and table dtype, a longer table, a wide row stride, queries only
            for D2 in DIMS:
                for rd in range(16, D2 + 1, 16):
                    for td in (2, 1):
                        assert call(appended(D=D2), _rope(pkg, rd=rd, table_dtype=td, interleaved=rd // 16 % 2, rows=CAPACITY + 5, row_stride=128),
                                    _view(pkg, H, Sq, D2), _view(pkg, Hkv, Sq, D2), _view(pkg, Hkv, Sq, D2)) == 0
            assert call(make(pkg), good, qo, None, None) == 0
            if which == "dec":   # queries only, seqlen_add as given
                a = make(pkg)
                a.seqlen_add = 5
                assert call(a, good, qo, None, None) == 0
    lib = pkg._lib.load()
    if which == "dec":   # the decode row limit is the base call's
        assert _callers(pkg, "dec", "plan")(appended(H=64, Hkv=8, Sq=17), _rope(pkg), _view(pkg, 64, 17, 64), _view(pkg, 8, 17, 64),
                                            _view(pkg, 8, 17, 64)) == EUNSUPPORTED
        assert lib.fasn_kvcache_rope_append_plan(appended(), _rope(pkg), qo, kn, kn, None, 10) == EINVAL
        assert lib.fasn_kvcache_rope_append_plan(appended(), _rope(pkg), qo, kn, kn, ctypes.create_string_buffer(8), 8) == EINVAL
    else:
        assert _callers(pkg, "pre", "plan")(appended(H=64, Hkv=8, Sq=17), _rope(pkg), _view(pkg, 64, 17, 64), _view(pkg, 8, 17, 64),
                                            _view(pkg, 8, 17, 64)) == 0
        assert lib.fasn_kvprefill_rope_append(ka._args_prefill(pkg, q_seqlens=DUMMY + 2), _rope(pkg), qo, None, None, None) == EALIGN
        a = ka._args_prefill(pkg, Sq=17)
        a.kv.seqlen_add = 3
        assert lib.fasn_kvprefill_rope_append(a, _rope(pkg), _view(pkg, 64, 17, 64), None, None, None) == EINVAL
        assert lib.fasn_kvprefill_rope_append_plan(appended(), _rope(pkg), qo, kn, kn, ctypes.create_string_buffer(8), 8) == EINVAL


SHAPES = [dict(B=4, H=64, Hkv=8, Sq=1), dict(B=3, H=8, Hkv=2, Sq=3), dict(B=64, H=16, Hkv=16, Sq=1), dict(B=2, H=12, Hkv=4, Sq=70)]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("which", ["dec", "pre"])
def test_plan_is_one_launch_whose_grid_depends_on_shapes_only(pkg, which, D, dtype):
    for c in SHAPES:
        B, H, Hkv, Sq = c["B"], c["H"], c["Hkv"], c["Sq"]
        if which == "dec" and H // Hkv * Sq > 128:
            continue

        def args(seqlens=DUMMY, **kw):
            if which == "dec":
                a = ka._args_decode(pkg, D=D, dtype=dtype, seqlens=seqlens, **c)
                a.seqlen_add = Sq
                return a
            a = ka._args_prefill(pkg, D=D, dtype=dtype, seqlens=seqlens, **dict(c, **kw))
            a.kv.seqlen_add = Sq
            return a
        qo, kn = _view(pkg, H, Sq, D), _view(pkg, Hkv, Sq, D)
        name = f"fasn_kvrope_kernel<{TAGS[dtype]}, {D}>"
        units = D // 16
        plan = pkg._lib.kvrope_plan(args(), _rope(pkg, rd=16), qo, kn, kn)
        assert plan == [(name, -(-(B * (Hkv + H) * Sq * units) // 256), 256, 0)], plan
        # queries only: the K/V units are gone from the grid
        assert pkg._lib.kvrope_plan(args(), _rope(pkg, rd=16), qo) == [(name, -(-(B * H * Sq * units) // 256), 256, 0)]
        # other lengths, another table, other tables and layouts: the same launch
        other = args(seqlens=DUMMY + 4096) if which == "dec" else args(seqlens=DUMMY + 4096, q_seqlens=DUMMY + 8192)
        (other if which == "dec" else other.kv).block_table = DUMMY + 65536
        for r in (_rope(pkg, rd=D, table_dtype=dtype, interleaved=1, rows=CAPACITY + 100, row_stride=512, cos=DUMMY + 64),):
            assert pkg._lib.kvrope_plan(other, r, qo, kn, kn) == plan


def test_plan_line_names_the_kernel(pkg):
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = ka._args_decode(pkg)
    a.seqlen_add = 1
    rc = lib.fasn_kvcache_rope_append_plan(a, _rope(pkg), _view(pkg, 64, 1, 64), _view(pkg, 8, 1, 64), _view(pkg, 8, 1, 64), buf, len(buf))
    assert rc == len(buf.value) > 0
    assert buf.value.decode() == "fasn_kvrope_kernel<fasn::bf16_tag, 64> grid=5 block=256 lds=0 cfg=bf16,D=64\n"
    # the plans of the forwards that follow did not move
    assert [k[0] for k in pkg._lib.kvcache_plan(ka._args_decode(pkg))] == ["fasn_kvcache_fwd_kernel<fasn::bf16_tag, 64>", "fasn_kvcache_combine_kernel<fasn::bf16_tag, 64>"]


def test_new_kernels_do_not_spill(pkg):
    """2 dtypes x 4 head dims = 8 kernels: spill 0, scratch 0"""
    import spill_map
    lib = os.path.join(ROOT, "flash-attention-softmax-n_amd", "libfasn.so")
    if not os.path.exists(spill_map.READELF):
        pytest.skip("llvm-readelf not available")
    table = spill_map.kernel_table(lib)
    names = sorted(table)
    pretty = subprocess.run([spill_map.CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_pretty = dict(zip(pretty, names))
    wanted = set()
    for D in DIMS:
        for dtype in (0, 1):
            a = ka._args_decode(pkg, D=D, dtype=dtype)
            a.seqlen_add = 1
            wanted.add(pkg._lib.kvrope_plan(a, _rope(pkg, rd=16), _view(pkg, 64, 1, D), _view(pkg, 8, 1, D), _view(pkg, 8, 1, D))[0][0])
    assert len(wanted) == 8 and all(n.startswith("fasn_kvrope_kernel<") for n in wanted), wanted
    for name in sorted(wanted):
        hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
        assert len(hit) == 1, (name, hit)
        v = table[hit[0]]
        assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)


# ---------------------------------------------------------------- front end on CPU tensors
def test_front_end_refuses_with_the_reason(pkg):
    """The rotary checks need no device and come before the CPU-tensor refusal; a valid call gets as far as that refusal on both branches."""
    fa = pkg.flash_attention_n_kvcache_rope
    B, H, Hkv, D = 2, 8, 2, 64
    kc = torch.zeros(4, 64, Hkv, D, dtype=torch.float16)
    sl = torch.zeros(B, dtype=torch.int32)
    bt = torch.zeros(B, 2, dtype=torch.int32)           # capacity 128
    cos = torch.zeros(128, 32)
    q1 = torch.zeros(B, H, 1, D, dtype=torch.float16)       # 4 rows: the decode kernels
    q40 = torch.zeros(B, H, 40, D, dtype=torch.float16)     # 160 rows: the prefill kernels
    for q in (q1, q40):
        kn = torch.zeros(B, Hkv, q.shape[2], D, dtype=torch.float16)
        # valid calls reach the CPU refusal: fp32 and 16-bit tables, a partial rotary_dim, longer tables, a slice of a wider table, both
        # layouts, with and without the append, query lengths, a window, a dense cache
        for c in (cos, cos.half(), torch.zeros(128, 8), torch.zeros(500, 32), torch.zeros(128, 64)[:, :32], torch.zeros(300, 32)[100:]):
            for kw in ({}, dict(k_new=kn, v_new=kn), dict(query_seqlens=sl), dict(window=5), dict(window=10 ** 12, k_new=kn, v_new=kn),
                       dict(rotary_interleaved=True), dict(is_causal=False)):
                with pytest.raises(RuntimeError, match="CPU tensor"):
                    fa(q, kc, kc, sl, c, c, block_table=bt, **kw)
        with pytest.raises(RuntimeError, match="CPU tensor"):
            fa(q, torch.zeros(B, 100, Hkv, D, dtype=torch.float16), torch.zeros(B, 100, Hkv, D, dtype=torch.float16), sl, torch.zeros(100, 32),
               torch.zeros(100, 32))
        # rows >= capacity, naming both numbers
        with pytest.raises(ValueError, match="cover 127 positions but the cache holds up to 128"):
            fa(q, kc, kc, sl, cos[:127], cos[:127], block_table=bt)
        with pytest.raises(ValueError, match="cover 99 positions but the cache holds up to 100"):
            fa(q, torch.zeros(B, 100, Hkv, D, dtype=torch.float16), torch.zeros(B, 100, Hkv, D, dtype=torch.float16), sl, torch.zeros(99, 32),
               torch.zeros(99, 32))
        # rotary_dim
        for half in (4, 12, 20, 40, 64):
            with pytest.raises(ValueError, match="rotary_dim"):
                fa(q, kc, kc, sl, torch.zeros(128, half), torch.zeros(128, half), block_table=bt)
        # the tables: shape, dtype, agreement, alignment
        with pytest.raises(ValueError, match="rotary_sin must be a \\[rows, rotary_dim / 2\\] tensor"):
            fa(q, kc, kc, sl, cos, None, block_table=bt)
        with pytest.raises(ValueError, match="rotary_cos must be a \\[rows, rotary_dim / 2\\] tensor"):
            fa(q, kc, kc, sl, cos[None], cos[None], block_table=bt)
        with pytest.raises(ValueError, match="one shape, dtype and row stride"):
            fa(q, kc, kc, sl, cos, cos[:, :16], block_table=bt)
        with pytest.raises(ValueError, match="one shape, dtype and row stride"):
            fa(q, kc, kc, sl, cos, cos.half(), block_table=bt)
        with pytest.raises(ValueError, match="float32 or the dtype of query"):
            fa(q, kc, kc, sl, cos.bfloat16(), cos.bfloat16(), block_table=bt)
        with pytest.raises(ValueError, match="float32 or the dtype of query"):
            fa(q, kc, kc, sl, cos.double(), cos.double(), block_table=bt)
        with pytest.raises(ValueError, match="16-byte aligned"):
            fa(q, kc, kc, sl, torch.zeros(128, 33)[:, 1:], torch.zeros(128, 33)[:, 1:], block_table=bt)
        with pytest.raises(ValueError, match="16-byte aligned"):
            fa(q, kc, kc, sl, torch.zeros(32, 128).t(), torch.zeros(32, 128).t(), block_table=bt)
        with pytest.raises(ValueError, match="row stride >= rotary_dim / 2 = 32"):   # an expanded row: stride 0
            fa(q, kc, kc, sl, torch.zeros(1, 32).expand(128, 32), torch.zeros(1, 32).expand(128, 32), block_table=bt)
        # the window
        with pytest.raises(ValueError, match="always causal"):
            fa(q, kc, kc, sl, cos, cos, block_table=bt, window=4, is_causal=False)
        for bad in (0, -1):
            with pytest.raises(ValueError, match="window must be >= 1"):
                fa(q, kc, kc, sl, cos, cos, block_table=bt, window=bad)
        for bad in (True, 4.0, torch.tensor(4)):
            with pytest.raises(TypeError, match="window must be None or a Python int"):
                fa(q, kc, kc, sl, cos, cos, block_table=bt, window=bad)
        # the refusals of the other cache calls hold
        with pytest.raises(ValueError, match="int32"):
            fa(q, kc, kc, sl.long(), cos, cos, block_table=bt)
        with pytest.raises(ValueError, match="query_seqlens must be a contiguous int32 tensor of shape \\[2\\]"):
            fa(q, kc, kc, sl, cos, cos, block_table=bt, query_seqlens=sl.long())
        with pytest.raises(ValueError, match="k_new and v_new come together"):
            fa(q, kc, kc, sl, cos, cos, block_table=bt, k_new=kn)
        with pytest.raises(RuntimeError, match="forward only"):
            fa(q.clone().requires_grad_(), kc, kc, sl, cos, cos, block_table=bt)
    with pytest.raises(ValueError, match="flash_attention_n_kvcache_rope: 256 query heads per K/V head are not supported"):
        k1 = torch.zeros(4, 64, 1, D, dtype=torch.float16)
        fa(torch.zeros(B, 256, 1, D, dtype=torch.float16), k1, k1, sl, cos, cos, block_table=bt)
    with pytest.raises(ValueError, match="head dim 96"):
        k96 = torch.zeros(4, 64, 2, 96, dtype=torch.float16)
        fa(torch.zeros(B, H, 1, 96, dtype=torch.float16), k96, k96, sl, cos, cos, block_table=bt)


def test_signature_and_exports(pkg):
    import flash_attention_softmax_n_amd as shim
    assert "flash_attention_n_kvcache_rope" in pkg.__all__ and shim.flash_attention_n_kvcache_rope is pkg.kvcache.flash_attention_n_kvcache_rope
    sig = inspect.signature(pkg.flash_attention_n_kvcache_rope)
    assert list(sig.parameters) == [
        "query", "k_cache", "v_cache", "cache_seqlens", "rotary_cos", "rotary_sin", "block_table", "k_new", "v_new", "query_seqlens",
        "softmax_n_param", "scale", "is_causal", "return_lse", "window", "rotary_interleaved"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(block_table=None, k_new=None, v_new=None, query_seqlens=None, softmax_n_param=1, scale=None, is_causal=True,
                     return_lse=False, window=None, rotary_interleaved=False)
    assert "alibi_slopes" not in sig.parameters
    # the three existing calls kept theirs
    assert list(inspect.signature(pkg.flash_attention_n_kvcache).parameters)[-1] == "alibi_slopes"
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_prefill).parameters)[-1] == "alibi_slopes"
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_window).parameters)[-1] == "return_lse"
