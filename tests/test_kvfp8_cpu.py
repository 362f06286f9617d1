"""FP8 (e4m3fn) K/V cache without a GPU: exports and layouts, the validation codes of the eight *_fp8 entry points behind the base checks
(fake, aligned pointers: validation comes before any HIP call), their launch plans - the base call's split rule, equal to
tests/golden/kvfp8_plans.txt - the register tables of the new kernels, the front end's refusals, and the quantisation reference of
tests/kv_fp8.py against a brute-force nearest-code search."""
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
import kv_fp8 as k8    # noqa: E402

DUMMY, BIG = ka.DUMMY, ka.BIG
NEW = ("fasn_fwd_kvcache_fp8", "fasn_fwd_kvcache_fp8_workspace_bytes", "fasn_kvcache_fp8_plan", "fasn_kvcache_fp8_append",
       "fasn_fwd_kvprefill_fp8", "fasn_fwd_kvprefill_fp8_workspace_bytes", "fasn_kvprefill_fp8_plan", "fasn_kvprefill_fp8_append")
DIMS = (64, 128)
TAGS = {0: "fasn::f16_tag", 1: "fasn::bf16_tag"}
EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED, EWORKSPACE = -1, -2, -3, -4, -5, -7, -8
_fp8 = k8._fp8

DECODE_CASES = dict(ka.DECODE_CASES, small=dict(B=1, H=2, Hkv=1, Sq=1, D=64, page=64, max_pages=32))
PREFILL_CASES = ka.PREFILL_CASES


# ---------------------------------------------------------------- exports and layouts
def test_symbols_are_exported_bound_and_declared(pkg):
    import flash_attention_softmax_n_amd as shim
    lib = shim._lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    header = open(os.path.join(ROOT, "include", "fasn.h")).read()
    for name in NEW:
        assert name in exported, name
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
        assert name in shim._lib.EXPORTS and getattr(lib, name).argtypes is not None
    assert lib.fasn_abi_version() == 6
    T = pkg._lib.KvFp8
    assert ctypes.sizeof(T) == 56
    assert (T.k_scale.offset, T.v_scale.offset, T.k_sb.offset, T.k_sh.offset, T.v_sb.offset, T.v_sh.offset, T.reserved.offset) == (0, 8, 16, 24, 32, 40, 48)
    # the argument blocks kept their layouts: the operand travels beside them
    assert pkg._lib.KvPrefillArgs.kv.offset == 0 and pkg._lib.KvPrefillArgs.q_seqlens.offset == ctypes.sizeof(pkg._lib.KvCacheArgs)


def test_struct_layout_matches_the_header(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fasn.h")).read(), flags=re.S)
    body = re.search(r"typedef struct fasn_kv_fp8 \{(.*?)\} fasn_kv_fp8;", text, flags=re.S).group(1)
    names = [n for _t, n in re.findall(r"([a-z0-9_ ]+?[ *]+)([A-Za-z_]+)(?:\[\d+\])?;", body)]
    assert names == [f[0] for f in pkg._lib.KvFp8._fields_], names


# ---------------------------------------------------------------- validation
def _routes(pkg):
    """(route name, argument-block maker, {how: call(args, operand) -> code or size})"""
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    for route, stem, make in (("decode", "kvcache", ka._args_decode), ("prefill", "kvprefill", ka._args_prefill)):
        heads = lambda a: a.H // a.kv_group   # noqa: E731
        kv = (lambda a: a) if route == "decode" else (lambda a: a.kv)
        calls = {
            "plan": lambda a, o, stem=stem: min(getattr(lib, f"fasn_{stem}_fp8_plan")(a, o, buf, len(buf)), 0),
            "forward": lambda a, o, stem=stem: getattr(lib, f"fasn_fwd_{stem}_fp8")(a, o, None, 0, None),
            "append": lambda a, o, stem=stem, kv=kv: getattr(lib, f"fasn_{stem}_fp8_append")(
                a, o, ka._view(pkg, heads(kv(a)), kv(a).Sq, kv(a).D), ka._view(pkg, heads(kv(a)), kv(a).Sq, kv(a).D), None),
        }
        yield route, make, kv, calls


@pytest.mark.parametrize("dtype", (0, 1))
@pytest.mark.parametrize("D", DIMS)
def test_plans_accept_the_supported_shapes(pkg, D, dtype):
    lib = pkg._lib.load()
    for route, make, _kv, calls in _routes(pkg):
        a = make(pkg, D=D, dtype=dtype)
        assert calls["plan"](a, _fp8(pkg)) == 0, route
        stem = "kvcache" if route == "decode" else "kvprefill"
        ws = getattr(lib, f"fasn_fwd_{stem}_fp8_workspace_bytes")(a, _fp8(pkg))
        assert ws == getattr(lib, f"fasn_fwd_{stem}_workspace_bytes")(a), route
        if ws:   # a forward with no workspace is refused for that, after every check of the operand passed (nothing is launched here)
            assert calls["forward"](a, _fp8(pkg)) == EWORKSPACE, route


def test_refusals_and_their_codes(pkg):
    for route, make, kv, calls in _routes(pkg):
        for how in ("plan", "forward", "append"):
            call = calls[how]

            def code(edit=None, op=None, **kw):
                a = make(pkg, **kw)
                if how == "append":
                    kv(a).seqlen_add = kv(a).Sq
                if edit is not None:
                    edit(kv(a))
                return call(a, _fp8(pkg) if op is None else op)

            what = (route, how)
            if how != "append":   # (a valid append would launch: no device here. Both default blocks have split partials)
                assert code() == (EWORKSPACE if how == "forward" else 0), what
            for D in (32, 256):
                assert code(D=D) == EHEADDIM, what
            assert code(D=96) == EHEADDIM, what                 # the base check's refusal, first
            assert call(make(pkg), None) == EINVAL, what
            assert code(op=_fp8(pkg, k_scale=None)) == EINVAL and code(op=_fp8(pkg, v_scale=None)) == EINVAL, what
            assert code(op=_fp8(pkg, reserved=1)) == EINVAL, what
            assert code(op=_fp8(pkg, k_scale=DUMMY + 2)) == EALIGN and code(op=_fp8(pkg, v_scale=DUMMY + 2)) == EALIGN, what
            assert code(op=_fp8(pkg, sb=-1)) == EINVAL and code(op=_fp8(pkg, sh=1 << 31)) == EINVAL, what
            # a cache row stride below D; strides that are multiples of 8 (a 16-bit cache's rule) but not of 16 bytes; a cache off 16 bytes
            assert code(lambda a: a.k_stride.__setitem__(1, a.D - 16)) == EINVAL, what
            assert code(lambda a: a.v_stride.__setitem__(1, a.D - 16)) == EINVAL, what
            for which in ("k_stride", "v_stride"):
                for i in range(3):
                    assert code(lambda a, which=which, i=i: getattr(a, which).__setitem__(i, getattr(a, which)[i] + 8)) == EALIGN, (what, which, i)
            assert code(lambda a: setattr(a, "k_cache", DUMMY + 8)) == EALIGN, what
            # pages below 64 rows, and pages that are no multiple of 64
            assert code(page=32) == EUNSUPPORTED and code(page=96) == EUNSUPPORTED, what
            assert code(dtype=2) == EDTYPE, what
            assert code(lambda a: setattr(a, "seqlens", None)) == EINVAL, what


def test_packed_block_has_no_fp8_call(pkg):
    assert not [n for n in pkg._lib.EXPORTS if "varlen" in n and "fp8" in n]


# ---------------------------------------------------------------- plans
def _plan_text(pkg):
    lib = pkg._lib.load()
    got = []
    for D in DIMS:
        for dtype in (0, 1):
            for route, cases, make, fn in (("decode", DECODE_CASES, ka._args_decode, lib.fasn_kvcache_fp8_plan),
                                           ("prefill", PREFILL_CASES, ka._args_prefill, lib.fasn_kvprefill_fp8_plan)):
                for name in sorted(cases):
                    buf = ctypes.create_string_buffer(4096)
                    a = make(pkg, dtype=dtype, **dict(cases[name], D=D))
                    rc = fn(a, _fp8(pkg), buf, len(buf))
                    assert rc > 0, (name, D, dtype, rc)
                    stem = "kvcache" if route == "decode" else "kvprefill"
                    ws = getattr(lib, f"fasn_fwd_{stem}_fp8_workspace_bytes")(a, _fp8(pkg))
                    got += [f"{route} {name} {line}" for line in buf.value.decode().splitlines()] + [f"{route} {name} workspace={ws}"]
    return got


def test_plans_equal_the_golden_file(pkg, golden_dir):
    want = open(os.path.join(golden_dir, "kvfp8_plans.txt")).read().splitlines()
    assert _plan_text(pkg) == want


@pytest.mark.parametrize("dtype", (0, 1))
@pytest.mark.parametrize("D", DIMS)
def test_split_counts_are_the_16_bit_plans(pkg, D, dtype):
    """same grids as the 16-bit call of the same shape - the split rule did not move - with the FP8 kernels' names and LDS"""
    smem = 2 * (3 if D == 64 else 2) * 64 * D + 2 * 64 * D * 2
    assert smem == {64: 40 * 1024, 128: 64 * 1024}[D]
    tag = f"{TAGS[dtype]}, {D}"
    for name, c in DECODE_CASES.items():
        a = ka._args_decode(pkg, dtype=dtype, **dict(c, D=D))
        base, plan = pkg._lib.kvcache_plan(a), k8.fp8_plan(pkg, a)
        assert [k[0] for k in plan] == [f"fasn_kvcache_fwd_fp8_kernel<{tag}>", f"fasn_kvcache_fp8_combine_kernel<{tag}>"], name
        assert [k[1:3] for k in plan] == [k[1:3] for k in base] and plan[0][3] == smem and plan[1][3] == 0, name
    for name, c in PREFILL_CASES.items():
        a = ka._args_prefill(pkg, dtype=dtype, **dict(c, D=D))
        base, plan = pkg._lib.kvprefill_plan(a), k8.fp8_plan(pkg, a)
        want = [f"fasn_kvprefill_fwd_fp8_kernel<{tag}>"] + ([f"fasn_kvprefill_fp8_combine_kernel<{tag}>"] if ka.PREFILL_SPLIT[name] else [])
        assert [k[0] for k in plan] == want and len(base) == len(plan), name
        assert [k[1:3] for k in plan] == [k[1:3] for k in base] and plan[0][3] == smem, name
        # the plan follows shapes and capacity only: other lengths, other scales, the appended rows
        other = ka._args_prefill(pkg, dtype=dtype, seqlens=DUMMY + 4096, q_seqlens=DUMMY + 8192, **dict(c, D=D))
        other.kv.seqlen_add = c["Sq"]
        assert k8.fp8_plan(pkg, other, _fp8(pkg, k_scale=DUMMY + 64, sb=8, sh=0)) == plan, name


def test_append_plan_is_one_launch_of_16_codes_per_thread(pkg):
    """the append has no plan entry point of its own; its grid is read off the kernel table instead: 16 bytes stored per thread means
    B * Hkv * Sq * D / 16 threads - checked on the GPU by the bytes it writes. Here: the kernels exist, once per dtype and head dim."""
    import spill_map
    lib = os.path.join(ROOT, "flash-attention-softmax-n_amd", "libfasn.so")
    if not os.path.exists(spill_map.READELF) or not os.path.exists(lib):
        pytest.skip("llvm-readelf or libfasn.so not available")
    pretty = set(spill_map.demangle(sorted(spill_map.kernel_table(lib))).values())
    for stem, block in (("kvcache", "KvParams"), ("kvprefill", "KvPrefillParams")):
        for D in DIMS:
            for tag in TAGS.values():
                assert f"void fasn::fasn_{stem}_fp8_append_kernel<{tag}, {D}>(fasn::{block}, fasn::KvFp8)" in pretty


def test_new_kernels_do_not_spill(pkg):
    """2 routes x 2 dtypes x 2 head dims x (forward, combine, append) = 24 kernels: spill 0, scratch 0"""
    import spill_map
    lib = os.path.join(ROOT, "flash-attention-softmax-n_amd", "libfasn.so")
    if not os.path.exists(spill_map.READELF):
        pytest.skip("llvm-readelf not available")
    if not os.path.exists(lib):
        pytest.skip("libfasn.so not built (run __graft_entry__.build() or make -C flash-attention-softmax-n_amd/csrc)")
    table = spill_map.kernel_table(lib)
    by_pretty = {d: m for m, d in spill_map.demangle(sorted(table)).items()}
    wanted = set()
    for D in DIMS:
        for dtype in (0, 1):
            for k in k8.fp8_plan(pkg, ka._args_decode(pkg, dtype=dtype, **dict(DECODE_CASES["gqa"], D=D))):
                wanted.add(k[0])
            for k in k8.fp8_plan(pkg, ka._args_prefill(pkg, dtype=dtype, **dict(PREFILL_CASES["gqa_chunk_long_cache"], D=D))):
                wanted.add(k[0])
            wanted.add(f"fasn_kvcache_fp8_append_kernel<{TAGS[dtype]}, {D}>")
            wanted.add(f"fasn_kvprefill_fp8_append_kernel<{TAGS[dtype]}, {D}>")
    assert len(wanted) == 24 and sum("_fwd_fp8_kernel<" in n for n in wanted) == 8, wanted
    for name in sorted(wanted):
        hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
        assert len(hit) == 1, (name, hit)
        v = table[hit[0]]
        assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)


def test_no_new_spill_allowance(golden_dir):
    import json
    allowance = json.load(open(os.path.join(golden_dir, "spill_allowance.json")))
    assert not [k for k in map(str, allowance if isinstance(allowance, (list, dict)) else []) if "fp8" in k]


# ---------------------------------------------------------------- the quantisation reference
@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=("float16", "bfloat16"))
@pytest.mark.parametrize("s", (1.0, 2.0 ** -3, 16.0, 0.3, 3.0, 1.7e-3))
def test_quantisation_reference_is_the_nearest_code(dtype, s):
    """kv_fp8.quantise - clamp, then torch's cast - against the brute-force search over the 254 finite codes, on the append's witnesses
    (scaled so that they land on the same codes) and on random values: the GPU test does not hide behind torch's cast"""
    w = k8.append_witnesses(dtype)
    x = torch.cat([w, (w.float() * s).to(dtype), torch.randn(256, generator=torch.Generator().manual_seed(3)).mul(200 * s).to(dtype)])
    got = k8.quantise(x, s)
    want = k8.nearest_code(x.float() / torch.tensor(s, dtype=torch.float32))
    nan = torch.isnan(x.float())
    assert k8.is_nan_code(got[nan]).all() and k8.is_nan_code(want[nan]).all()
    assert torch.equal(got[~nan], want[~nan]), [(float(a), int(b), int(c)) for a, b, c in zip(x[~nan], got[~nan], want[~nan]) if b != c][:8]
    if s == 1.0:   # the witnesses do what they are there for
        exact = dict(zip(w.float().tolist(), k8.quantise(w, 1.0).tolist()))
        assert exact[1.0625] == 0x38 and exact[1.1875] == 0x3A and exact[-1.0625] == 0xB8         # ties go to the even mantissa
        assert exact[2.0 ** -10] == 0x00 and exact[3 * 2.0 ** -10] == 0x02 and exact[2.0 ** -9] == 0x01   # ... among the subnormals too
        assert exact[448.0] == 0x7E and exact[500.0] == 0x7E and exact[float("inf")] == 0x7E and exact[-500.0] == 0xFE
        assert k8.quantise(torch.tensor([-0.0, 0.0]), 1.0).tolist() == [0x80, 0x00]
        assert torch.isnan(torch.tensor(500.0).to(k8.F8).float())   # torch's own cast does not saturate: why the reference clamps first


def test_every_finite_code_is_a_16_bit_number():
    codes, vals = k8.finite_codes()
    for dtype in (torch.float16, torch.bfloat16):
        assert torch.equal(k8.up(codes, dtype).double(), vals)
    assert torch.equal(k8.quantise(vals.float(), 1.0), codes)


# ---------------------------------------------------------------- front end on CPU tensors
def test_front_end_refuses_with_the_reason(pkg):
    fa = pkg.flash_attention_n_kvcache_fp8
    B, H, Hkv = 2, 8, 2
    sl = torch.zeros(B, dtype=torch.int32)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    for Sq in (1, 40):   # the decode kernels; 160 rows: the prefill kernels
        q = torch.zeros(B, H, Sq, 64, dtype=torch.float16)
        kc = torch.zeros(4, 64, Hkv, 64, dtype=torch.uint8).view(k8.F8)
        with pytest.raises(RuntimeError, match="MI355X device tensors only"):   # every check passed
            fa(q, kc, kc, sl, 1.0, 0.5, block_table=bt)
        with pytest.raises(RuntimeError, match="MI355X device tensors only"):
            fa(q, kc, kc, sl, torch.ones(Hkv), torch.ones(B, 1), block_table=bt, k_new=q[:, :Hkv], v_new=q[:, :Hkv])
        for bad in (torch.zeros(4, 64, Hkv, 64, dtype=torch.float16), torch.zeros(4, 64, Hkv, 64, dtype=torch.bfloat16),
                    torch.zeros(4, 64, Hkv, 64, dtype=torch.float8_e5m2), torch.zeros(4, 64, Hkv, 64, dtype=torch.uint8)):
            with pytest.raises(TypeError, match="must be torch.float8_e4m3fn"):
                fa(q, bad, bad, sl, 1.0, 1.0, block_table=bt)
        with pytest.raises(ValueError, match="dtype torch.float32 is not supported"):
            fa(q.float(), kc, kc, sl, 1.0, 1.0, block_table=bt)
        for D in (32, 256):
            with pytest.raises(ValueError, match=f"head dim {D} is not supported on an FP8 cache"):
                fa(torch.zeros(B, H, Sq, D, dtype=torch.float16), torch.zeros(4, 64, Hkv, D, dtype=torch.uint8).view(k8.F8),
                   torch.zeros(4, 64, Hkv, D, dtype=torch.uint8).view(k8.F8), sl, 1.0, 1.0, block_table=bt)
        for name, value in (("alibi_slopes", torch.ones(H)), ("window", 128), ("rotary_cos", torch.zeros(128, 16)), ("rotary_sin", torch.zeros(128, 16)),
                            ("cu_seqlens_q", sl), ("tree_mask", torch.zeros(B, Sq, dtype=torch.int64))):
            with pytest.raises(NotImplementedError, match=f"{name} is not supported on an FP8 cache"):
                fa(q, kc, kc, sl, 1.0, 1.0, block_table=bt, **{name: value})
        # the scales
        with pytest.raises(TypeError, match="k_scale must be a Python float or a floating-point tensor"):
            fa(q, kc, kc, sl, torch.ones(Hkv, dtype=torch.int32), 1.0, block_table=bt)
        with pytest.raises(TypeError, match="v_scale must be a Python float or a floating-point tensor"):
            fa(q, kc, kc, sl, 1.0, None, block_table=bt)
        with pytest.raises(ValueError, match=r"k_scale must broadcast to \[B, Hkv\] = \[2, 2\]"):
            fa(q, kc, kc, sl, torch.ones(H), 1.0, block_table=bt)
        with pytest.raises(RuntimeError, match="v_scale is on meta"):
            fa(q, kc, kc, sl, 1.0, torch.ones(Hkv, device="meta"), block_table=bt)
        with pytest.raises(RuntimeError, match="forward only"):
            fa(q, kc, kc, sl, torch.ones(Hkv, requires_grad=True), 1.0, block_table=bt)
        # the cache's rules, in bytes
        with pytest.raises(ValueError, match="feature stride must be 1"):
            fa(q, kc.transpose(2, 3).contiguous().transpose(2, 3), kc, sl, 1.0, 1.0, block_table=bt)
        wide = torch.zeros(4, 64, Hkv, 72, dtype=torch.uint8).view(k8.F8)[..., :64]   # row and head strides of 72 bytes
        with pytest.raises(ValueError, match="strides % 16 elements"):
            fa(q, wide, wide, sl, 1.0, 1.0, block_table=bt)
        with pytest.raises(ValueError, match="page_size 32 is not supported"):
            fa(q, kc[:, :32], kc[:, :32], sl, 1.0, 1.0, block_table=bt)
        # the base calls keep refusing what they refuse
        with pytest.raises(ValueError, match="int32"):
            fa(q, kc, kc, sl.long(), 1.0, 1.0, block_table=bt)
        with pytest.raises(ValueError, match="query_seqlens must be a contiguous int32 tensor of shape \\[2\\]"):
            fa(q, kc, kc, sl, 1.0, 1.0, block_table=bt, query_seqlens=sl.long())
        with pytest.raises(ValueError, match="k_new must be"):
            fa(q, kc, kc, sl, 1.0, 1.0, block_table=bt, k_new=q[:, :Hkv].float(), v_new=q[:, :Hkv].float())
    # a 16-bit call does not take an FP8 cache either
    with pytest.raises(TypeError, match="must share one dtype"):
        pkg.flash_attention_n_kvcache(torch.zeros(B, H, 1, 64, dtype=torch.float16), kc, kc, sl, block_table=bt)


def test_signature_and_exports(pkg):
    import flash_attention_softmax_n_amd as shim
    assert "flash_attention_n_kvcache_fp8" in pkg.__all__ and shim.flash_attention_n_kvcache_fp8 is pkg.kvcache.flash_attention_n_kvcache_fp8
    sig = inspect.signature(pkg.flash_attention_n_kvcache_fp8)
    assert list(sig.parameters)[:14] == ["query", "k_cache", "v_cache", "cache_seqlens", "k_scale", "v_scale", "block_table", "k_new", "v_new",
                                         "query_seqlens", "softmax_n_param", "scale", "is_causal", "return_lse"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d["softmax_n_param"] == 1 and d["is_causal"] is True and d["return_lse"] is False and d["scale"] is None
    assert all(d[k] is None for k in ("alibi_slopes", "window", "rotary_cos", "rotary_sin", "cu_seqlens_q", "tree_mask"))
    # the 16-bit calls are what they were
    assert list(inspect.signature(pkg.flash_attention_n_kvcache).parameters)[-1] == "alibi_slopes"
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_window).parameters)[-1] == "return_lse"
