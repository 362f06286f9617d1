"""The FP8 K/V cache's layer calls without a GPU - the sliding window (fasn_fwd_kv*_fp8_window) and the rotate-quantise-append
(fasn_kv*_fp8_rope_append): exports and unchanged layouts, the validation codes of the ten new entry points in the family's order (base
checks, the FP8 operand, then the window's rule or the rope operand; fake, aligned pointers: validation comes before any HIP call), their
launch plans - the 16-bit window call's grids and workspace, the 16-bit rope append's grid, equal to tests/golden/kvfp8_layer_plans.txt -
the register tables of the new kernels, and the front end of the two new functions on CPU tensors."""
import ctypes
import inspect
import json
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

DUMMY = ka.DUMMY
WINDOW_SYMBOLS = ("fasn_fwd_kvcache_fp8_window", "fasn_fwd_kvcache_fp8_window_workspace_bytes", "fasn_kvcache_fp8_window_plan",
                  "fasn_fwd_kvprefill_fp8_window", "fasn_fwd_kvprefill_fp8_window_workspace_bytes", "fasn_kvprefill_fp8_window_plan")
ROPE_SYMBOLS = ("fasn_kvcache_fp8_rope_append", "fasn_kvprefill_fp8_rope_append", "fasn_kvcache_fp8_rope_append_plan",
                "fasn_kvprefill_fp8_rope_append_plan")
NEW = WINDOW_SYMBOLS + ROPE_SYMBOLS
DIMS = (64, 128)
TAGS = {0: "fasn::f16_tag", 1: "fasn::bf16_tag"}
EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED, EWORKSPACE = -1, -2, -3, -4, -5, -7, -8
_fp8, _win, _rope, _view = k8._fp8, ka._win, ka._rope, ka._view
ROUTES = (("decode", "kvcache", ka._args_decode), ("prefill", "kvprefill", ka._args_prefill))


def _kv(route, a):
    return a if route == "decode" else a.kv


def _capacity(c):
    return c["page"] * c["max_pages"]


def _windows(c):
    return (1, 128, 1000, _capacity(c))


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
    assert lib.fasn_abi_version() == 6 and pkg._lib.FASN_ABI_VERSION == 6
    # no packed (token-buffer) entry point over an FP8 cache
    assert not [n for n in exported if "varlen" in n and "fp8" in n]


def test_operand_layouts_are_unchanged(pkg):
    L = pkg._lib
    T = L.KvFp8
    assert ctypes.sizeof(T) == 56
    assert (T.k_scale.offset, T.v_scale.offset, T.k_sb.offset, T.k_sh.offset, T.v_sb.offset, T.v_sh.offset, T.reserved.offset) == (0, 8, 16, 24, 32, 40, 48)
    W = L.KvWindow
    assert ctypes.sizeof(W) == 8 and (W.window.offset, W.reserved.offset) == (0, 4)
    R = L.KvRope
    assert (R.cos.offset, R.sin.offset, R.row_stride.offset, R.rows.offset, R.rotary_dim.offset, R.table_dtype.offset, R.interleaved.offset) == (
        0, 8, 16, 24, 28, 32, 36) and ctypes.sizeof(R) == 40
    assert L.KvPrefillArgs.kv.offset == 0 and L.KvPrefillArgs.q_seqlens.offset == ctypes.sizeof(L.KvCacheArgs)
    assert L.KvCacheArgs.n_stride_h.offset + 8 == ctypes.sizeof(L.KvCacheArgs)
    # the header declares the three operand structs with the members the bindings have
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fasn.h")).read(), flags=re.S)
    for struct, T in (("fasn_kv_fp8", L.KvFp8), ("fasn_kv_window", L.KvWindow), ("fasn_kv_rope", L.KvRope)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        names = [n for _t, n in re.findall(r"([a-z0-9_ ]+?[ *]+)([A-Za-z_]+)(?:\[\d+\])?;", body)]
        assert names == [f[0] for f in T._fields_], (struct, names)


# ---------------------------------------------------------------- validation
def _window_calls(pkg, stem):
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    return {
        "plan": lambda a, o, w: min(getattr(lib, f"fasn_{stem}_fp8_window_plan")(a, o, w, buf, len(buf)), 0),
        "forward": lambda a, o, w: getattr(lib, f"fasn_fwd_{stem}_fp8_window")(a, o, w, None, 0, None),
    }


def test_window_refusals_and_their_codes(pkg):
    lib = pkg._lib.load()
    for route, stem, make in ROUTES:
        for how, call in _window_calls(pkg, stem).items():
            def code(edit=None, op=None, win=None, **kw):
                a = make(pkg, **kw)
                if edit is not None:
                    edit(_kv(route, a))
                return call(a, _fp8(pkg) if op is None else op, _win(pkg) if win is None else win)

            what = (route, how)
            # accepted. Under a window at the capacity both default blocks have split partials: a forward without a workspace is refused
            # for that, behind every check (a forward that needs none would launch: no device here)
            assert code(win=_win(pkg, window=ka.CAPACITY)) == (EWORKSPACE if how == "forward" else 0), what
            if how == "plan":
                assert code() == 0, what
            # NULL operands
            assert call(None, _fp8(pkg), _win(pkg)) == EINVAL, what
            assert call(make(pkg), None, _win(pkg)) == EINVAL and call(make(pkg), _fp8(pkg), None) == EINVAL, what
            assert code(op=_fp8(pkg, k_scale=None)) == EINVAL and code(op=_fp8(pkg, v_scale=None)) == EINVAL, what
            # the window's rule
            assert code(win=_win(pkg, window=0)) == EINVAL and code(win=_win(pkg, window=-5)) == EINVAL, what
            assert code(win=_win(pkg, reserved=1)) == EINVAL and code(op=_fp8(pkg, reserved=1)) == EINVAL, what
            assert code(lambda a: setattr(a, "causal", 0)) == EUNSUPPORTED, what
            # head dims: 96 is the base check's refusal, 32 / 256 the FP8 operand's
            for D in (32, 96, 256):
                assert code(D=D) == EHEADDIM, (what, D)
            # misaligned scales; a byte stride that is a multiple of 8 but not of 16; page 32
            assert code(op=_fp8(pkg, k_scale=DUMMY + 2)) == EALIGN and code(op=_fp8(pkg, v_scale=DUMMY + 2)) == EALIGN, what
            for which in ("k_stride", "v_stride"):
                for i in range(3):
                    assert code(lambda a, which=which, i=i: getattr(a, which).__setitem__(i, getattr(a, which)[i] + 8)) == EALIGN, (what, which, i)
            assert code(page=32) == EUNSUPPORTED, what
            assert code(dtype=2) == EDTYPE, what
            # the order: base checks, then the FP8 operand, then the window
            assert code(lambda a: setattr(a, "seqlens", None), op=_fp8(pkg, reserved=1), win=_win(pkg, window=0)) == EINVAL, what
            assert code(D=96, op=_fp8(pkg, k_scale=DUMMY + 2), win=_win(pkg, window=0)) == EHEADDIM, what            # base first
            assert code(op=_fp8(pkg, k_scale=DUMMY + 2), win=_win(pkg, window=0)) == EALIGN, what                     # FP8 before the window
            assert code(lambda a: setattr(a, "causal", 0), op=_fp8(pkg, k_scale=DUMMY + 2)) == EALIGN, what
            assert code(D=32, win=_win(pkg, window=0)) == EHEADDIM, what
        # workspace: 0 for a refused block, the 16-bit window call's otherwise
        ws = getattr(lib, f"fasn_fwd_{stem}_fp8_window_workspace_bytes")
        assert ws(make(pkg), _fp8(pkg), _win(pkg, window=0)) == 0 and ws(make(pkg), None, _win(pkg)) == 0 and ws(make(pkg, D=32), _fp8(pkg), _win(pkg)) == 0
        full = _win(pkg, window=ka.CAPACITY)
        assert ws(make(pkg), _fp8(pkg), full) == getattr(lib, f"fasn_fwd_{stem}_window_workspace_bytes")(make(pkg), full) > 0
        assert ws(make(pkg), _fp8(pkg), _win(pkg)) == getattr(lib, f"fasn_fwd_{stem}_window_workspace_bytes")(make(pkg), _win(pkg))


def _rope_calls(pkg, stem):
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    return {
        "plan": lambda a, o, r, qo, kn, vn: min(getattr(lib, f"fasn_{stem}_fp8_rope_append_plan")(a, o, r, qo, kn, vn, buf, len(buf)), 0),
        "run": lambda a, o, r, qo, kn, vn: getattr(lib, f"fasn_{stem}_fp8_rope_append")(a, o, r, qo, kn, vn, None),
    }


def test_rope_append_refusals_and_their_codes(pkg):
    """(an accepted call would launch: the launching entry points are only ever refused here, the accepted blocks go through the plans)"""
    H, Hkv, Sq = 64, 8, 1
    for route, stem, make in ROUTES:
        for how, call in _rope_calls(pkg, stem).items():
            def code(edit=None, op=None, rope=None, D=64, appended=True, qo=True, kn=True, vn=True, **kw):
                a = make(pkg, D=D, **kw)
                if appended:
                    _kv(route, a).seqlen_add = _kv(route, a).Sq
                if edit is not None:
                    edit(_kv(route, a))
                return call(a, _fp8(pkg) if op is None else op, _rope(pkg) if rope is None else rope,
                            _view(pkg, H, Sq, D) if qo is True else qo, _view(pkg, Hkv, Sq, D) if kn is True else kn,
                            _view(pkg, Hkv, Sq, D) if vn is True else vn)

            what = (route, how)
            if how == "plan":
                assert code() == 0, what
                assert code(appended=False, kn=None, vn=None) == 0, what   # queries only
                assert code(D=128, rope=_rope(pkg, rd=128, table_dtype=1, interleaved=1, row_stride=64)) == 0, what
            # NULL operands
            assert call(None, _fp8(pkg), _rope(pkg), _view(pkg, H, Sq, 64), None, None) == EINVAL, what
            assert call(make(pkg), None, _rope(pkg), _view(pkg, H, Sq, 64), None, None) == EINVAL, what
            assert call(make(pkg), _fp8(pkg), None, _view(pkg, H, Sq, 64), None, None) == EINVAL, what
            assert code(qo=None) == EINVAL and code(kn=None) == EINVAL and code(vn=None) == EINVAL, what
            assert code(op=_fp8(pkg, k_scale=None)) == EINVAL and code(op=_fp8(pkg, reserved=1)) == EINVAL, what
            assert code(rope=_rope(pkg, cos=None)) == EINVAL and code(rope=_rope(pkg, sin=None)) == EINVAL, what
            assert code(appended=False) == EINVAL, what   # k_new / v_new given: seqlen_add == Sq
            # head dims
            for D in (32, 96, 256):
                assert code(D=D, rope=_rope(pkg, rd=32)) == EHEADDIM, (what, D)
            # misaligned scales; a byte stride that is a multiple of 8 but not of 16; page 32
            assert code(op=_fp8(pkg, k_scale=DUMMY + 2)) == EALIGN and code(op=_fp8(pkg, v_scale=DUMMY + 2)) == EALIGN, what
            for which in ("k_stride", "v_stride"):
                for i in range(3):
                    assert code(lambda a, which=which, i=i: getattr(a, which).__setitem__(i, getattr(a, which)[i] + 8)) == EALIGN, (what, which, i)
            assert code(page=32) == EUNSUPPORTED, what
            assert code(dtype=2) == EDTYPE, what
            # the rope operand's existing checks
            for rd in (0, 8, 24, 80):
                assert code(rope=_rope(pkg, rd=rd, row_stride=64)) == EINVAL, (what, rd)
            assert code(rope=_rope(pkg, rows=ka.CAPACITY - 1)) == EINVAL and code(rope=_rope(pkg, interleaved=2)) == EINVAL, what
            assert code(dtype=1, rope=_rope(pkg, table_dtype=0)) == EDTYPE, what
            assert code(rope=_rope(pkg, cos=DUMMY + 4)) == EALIGN and code(rope=_rope(pkg, row_stride=34)) == EALIGN, what
            assert code(qo=_view(pkg, H, Sq, 64, ptr=DUMMY + 2)) == EALIGN and code(kn=_view(pkg, Hkv, Sq, 64, ptr=DUMMY + 2)) == EALIGN, what
            # the order: base, FP8 operand, rope operand
            assert code(D=96, op=_fp8(pkg, k_scale=DUMMY + 2), rope=_rope(pkg, rd=8)) == EHEADDIM, what
            assert code(op=_fp8(pkg, k_scale=DUMMY + 2), rope=_rope(pkg, rd=8)) == EALIGN, what
            assert code(D=32, rope=_rope(pkg, rd=8)) == EHEADDIM, what
            assert code(lambda a: setattr(a, "seqlens", None), op=_fp8(pkg, k_scale=DUMMY + 2)) == EINVAL, what


# ---------------------------------------------------------------- plans
def _plan_text(pkg):
    lib = pkg._lib.load()
    got = []
    for D in DIMS:
        for dtype in (0, 1):
            for route, stem, make in ROUTES:
                cases = ka.DECODE_CASES if route == "decode" else ka.PREFILL_CASES
                for name in sorted(cases):
                    c = dict(cases[name], D=D)
                    for W in _windows(c):
                        a = make(pkg, dtype=dtype, **c)
                        plan = pkg._lib.kvfp8_window_plan(a, _fp8(pkg), _win(pkg, window=W))
                        ws = getattr(lib, f"fasn_fwd_{stem}_fp8_window_workspace_bytes")(a, _fp8(pkg), _win(pkg, window=W))
                        got += [f"{route} {name} W={W} {k[0]} grid={k[1]} block={k[2]} lds={k[3]}" for k in plan] + [f"{route} {name} W={W} workspace={ws}"]
                    a = make(pkg, dtype=dtype, **c)
                    _kv(route, a).seqlen_add = c["Sq"]
                    r = _rope(pkg, rows=_capacity(c), rd=D)
                    plan = pkg._lib.kvfp8_rope_plan(a, _fp8(pkg), r, _view(pkg, c["H"], c["Sq"], D), _view(pkg, c["Hkv"], c["Sq"], D), _view(pkg, c["Hkv"], c["Sq"], D))
                    got += [f"{route} {name} rope {k[0]} grid={k[1]} block={k[2]} lds={k[3]}" for k in plan]
    return got


def test_plans_equal_the_golden_file(pkg, golden_dir):
    want = open(os.path.join(golden_dir, "kvfp8_layer_plans.txt")).read().splitlines()
    assert _plan_text(pkg) == want


@pytest.mark.parametrize("dtype", (0, 1))
@pytest.mark.parametrize("D", DIMS)
def test_window_plans_are_the_16_bit_window_plans(pkg, D, dtype):
    """names of the FP8 window and FP8 combine kernels, the grids and the workspace of the 16-bit window plan of the same shape and window,
    the FP8 kernels' LDS, and no dependence on lengths or scales"""
    lib = pkg._lib.load()
    smem = {64: 40 * 1024, 128: 64 * 1024}[D]
    tag = f"{TAGS[dtype]}, {D}"
    several = 0
    for route, stem, make in ROUTES:
        cases = ka.DECODE_CASES if route == "decode" else ka.PREFILL_CASES
        base_plan = pkg._lib.kvcache_window_plan if route == "decode" else pkg._lib.kvprefill_window_plan
        for name, c in cases.items():
            c = dict(c, D=D)
            for W in _windows(c):
                a = make(pkg, dtype=dtype, **c)
                win = _win(pkg, window=W)
                base, plan = base_plan(a, win), pkg._lib.kvfp8_window_plan(a, _fp8(pkg), win)
                want = [f"fasn_{stem}_fwd_fp8_window_kernel<{tag}>"] + ([f"fasn_{stem}_fp8_combine_kernel<{tag}>"] if len(base) == 2 else [])
                assert [k[0] for k in plan] == want, (name, W, plan)
                assert route == "prefill" or len(plan) == 2, (name, W)   # decode always combines
                assert [k[1:3] for k in plan] == [k[1:3] for k in base], (name, W, plan, base)
                assert plan[0][3] == smem and all(k[3] == 0 for k in plan[1:]), (name, W)
                assert base[0][0] == f"fasn_{stem}_fwd_window_kernel<{tag}>"
                ws = getattr(lib, f"fasn_fwd_{stem}_fp8_window_workspace_bytes")(a, _fp8(pkg), win)
                assert ws == getattr(lib, f"fasn_fwd_{stem}_window_workspace_bytes")(a, win), (name, W)
                several += len(plan) == 2 and route == "prefill"
                # other lengths, other scales, the appended rows: the same plan
                kw = dict(seqlens=DUMMY + 4096) if route == "decode" else dict(seqlens=DUMMY + 4096, q_seqlens=DUMMY + 8192)
                other = make(pkg, dtype=dtype, **dict(c, **kw))
                if route == "prefill":
                    other.kv.seqlen_add = c["Sq"]
                assert pkg._lib.kvfp8_window_plan(other, _fp8(pkg, k_scale=DUMMY + 64, sb=8, sh=0), win) == plan, (name, W)
            # the window at the capacity: the grids of the FP8 call without a window
            full = pkg._lib.kvfp8_window_plan(make(pkg, dtype=dtype, **c), _fp8(pkg), _win(pkg, window=_capacity(c)))
            assert [k[1:] for k in full] == [k[1:] for k in k8.fp8_plan(pkg, make(pkg, dtype=dtype, **c))], name
    assert several > 0   # a prefill with several splits and the FP8 combine kernel is among the cases


@pytest.mark.parametrize("dtype", (0, 1))
@pytest.mark.parametrize("D", DIMS)
def test_rope_append_plan_is_one_launch_on_the_16_bit_grid(pkg, D, dtype):
    name = f"fasn_kvrope_fp8_kernel<{TAGS[dtype]}, {D}>"
    for route, stem, make in ROUTES:
        for c in (dict(B=4, H=64, Hkv=8, Sq=1), dict(B=3, H=8, Hkv=2, Sq=3), dict(B=2, H=12, Hkv=4, Sq=70)):
            B, H, Hkv, Sq = c["B"], c["H"], c["Hkv"], c["Sq"]
            if route == "decode" and H // Hkv * Sq > 128:
                continue

            def args(**kw):
                a = make(pkg, D=D, dtype=dtype, **dict(c, **kw))
                _kv(route, a).seqlen_add = Sq
                return a
            qo, kn = _view(pkg, H, Sq, D), _view(pkg, Hkv, Sq, D)
            plan = pkg._lib.kvfp8_rope_plan(args(), _fp8(pkg), _rope(pkg, rd=16), qo, kn, kn)
            base = pkg._lib.kvrope_plan(args(), _rope(pkg, rd=16), qo, kn, kn)
            assert plan == [(name, -(-(B * (Hkv + H) * Sq * (D // 16)) // 256), 256, 0)], plan
            assert len(base) == 1 and plan[0][1:] == base[0][1:]
            assert pkg._lib.kvfp8_rope_plan(args(), _fp8(pkg), _rope(pkg, rd=16), qo) == [(name, -(-(B * H * Sq * (D // 16)) // 256), 256, 0)]
            # other lengths, scales, tables and layouts: the same launch
            other = args(seqlens=DUMMY + 4096)
            r = _rope(pkg, rd=D, table_dtype=dtype, interleaved=1, rows=ka.CAPACITY + 100, row_stride=512, cos=DUMMY + 64)
            assert pkg._lib.kvfp8_rope_plan(other, _fp8(pkg, k_scale=DUMMY + 64, sb=8, sh=0), r, qo, kn, kn) == plan


def test_plan_lines_describe_the_kernels(pkg):
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    rc = lib.fasn_kvcache_fp8_window_plan(ka._args_decode(pkg), _fp8(pkg), _win(pkg), buf, len(buf))
    assert rc == len(buf.value) > 0
    lines = buf.value.decode().splitlines()
    assert lines[0].startswith("fasn_kvcache_fwd_fp8_window_kernel<fasn::bf16_tag, 64> grid=") and lines[0].endswith(" block=256 lds=40960 cfg=bf16,D=64")
    assert lib.fasn_kvcache_fp8_window_plan(ka._args_decode(pkg), _fp8(pkg), _win(pkg), None, 10) == EINVAL
    assert lib.fasn_kvcache_fp8_window_plan(ka._args_decode(pkg), _fp8(pkg), _win(pkg), ctypes.create_string_buffer(8), 8) == EINVAL
    a = ka._args_decode(pkg)
    a.seqlen_add = 1
    rc = lib.fasn_kvcache_fp8_rope_append_plan(a, _fp8(pkg), _rope(pkg), _view(pkg, 64, 1, 64), _view(pkg, 8, 1, 64), _view(pkg, 8, 1, 64), buf, len(buf))
    assert rc == len(buf.value) > 0
    assert buf.value.decode() == "fasn_kvrope_fp8_kernel<fasn::bf16_tag, 64> grid=5 block=256 lds=0 cfg=bf16,D=64\n"
    # the plans of the calls that were there did not move
    assert [k[0] for k in k8.fp8_plan(pkg, ka._args_decode(pkg))] == ["fasn_kvcache_fwd_fp8_kernel<fasn::bf16_tag, 64>",
                                                                     "fasn_kvcache_fp8_combine_kernel<fasn::bf16_tag, 64>"]


# ---------------------------------------------------------------- the kernels
def test_new_kernels_are_there_once_and_do_not_spill(pkg):
    """(decode window, prefill window, rope append) x 2 dtypes x 2 head dims = 12 kernels: once each, spill 0, scratch 0"""
    import spill_map
    lib = os.path.join(ROOT, "flash-attention-softmax-n_amd", "libfasn.so")
    if not os.path.exists(spill_map.READELF):
        pytest.skip("llvm-readelf not available")
    table = spill_map.kernel_table(lib)
    by_pretty = {d: m for m, d in spill_map.demangle(sorted(table)).items()}
    wanted = {}
    for D in DIMS:
        for tag in TAGS.values():
            wanted[f"fasn_kvcache_fwd_fp8_window_kernel<{tag}, {D}>"] = "(fasn::KvParams, fasn::KvFp8, fasn::KvWindow)"
            wanted[f"fasn_kvprefill_fwd_fp8_window_kernel<{tag}, {D}>"] = "(fasn::KvPrefillParams, fasn::KvFp8, fasn::KvWindow)"
            wanted[f"fasn_kvrope_fp8_kernel<{tag}, {D}>"] = "(fasn::KvRopeParams, fasn::KvFp8)"
    assert len(wanted) == 12
    for name, params in sorted(wanted.items()):
        hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
        assert len(hit) == 1, (name, hit)
        assert ("void fasn::" + name + params) in by_pretty, name
        v = table[hit[0]]
        assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)
    # built for the FP8 head dims only, and no tree or packed sibling
    fp8_layer = [d for d in by_pretty if "fp8_window_kernel<" in d or "kvrope_fp8_kernel<" in d]
    assert len(fp8_layer) == 12, fp8_layer


def test_no_new_spill_allowance(golden_dir):
    allowance = json.load(open(os.path.join(golden_dir, "spill_allowance.json")))
    assert not [k for k in map(str, allowance if isinstance(allowance, (list, dict)) else []) if "fp8" in k]


# ---------------------------------------------------------------- front end on CPU tensors
def _cpu_case(Sq, D=64, dtype=torch.float16):
    B, H, Hkv = 2, 8, 2
    q = torch.zeros(B, H, Sq, D, dtype=dtype)
    kc = torch.zeros(4, 64, Hkv, D, dtype=torch.uint8).view(k8.F8)
    return q, kc, torch.zeros(B, dtype=torch.int32), torch.zeros(B, 2, dtype=torch.int32)


def test_window_front_end_refuses_with_the_reason(pkg):
    fa = pkg.flash_attention_n_kvcache_fp8_window
    B, H, Hkv = 2, 8, 2
    for Sq in (1, 40):   # the decode kernels; 160 rows: the prefill kernels
        q, kc, sl, bt = _cpu_case(Sq)
        with pytest.raises(RuntimeError, match="MI355X device tensors only"):   # every check passed
            fa(q, kc, kc, sl, 1.0, 0.5, 128, block_table=bt)
        with pytest.raises(RuntimeError, match="MI355X device tensors only"):
            fa(q, kc, kc, sl, torch.ones(Hkv), torch.ones(B, 1), 1, block_table=bt, k_new=q[:, :Hkv], v_new=q[:, :Hkv], query_seqlens=sl, return_lse=True)
        for bad, err in ((0, ValueError), (-3, ValueError), (None, TypeError), (True, TypeError), (128.0, TypeError), (torch.tensor(128), TypeError)):
            with pytest.raises(err, match="flash_attention_n_kvcache_fp8_window: window must be"):
                fa(q, kc, kc, sl, 1.0, 1.0, bad, block_table=bt)
        for bad in (torch.zeros(4, 64, Hkv, 64, dtype=torch.float16), torch.zeros(4, 64, Hkv, 64, dtype=torch.float8_e5m2)):
            with pytest.raises(TypeError, match="must be torch.float8_e4m3fn"):
                fa(q, bad, bad, sl, 1.0, 1.0, 128, block_table=bt)
        for D in (32, 256):
            qd, kd, _sl, _bt = _cpu_case(Sq, D)
            with pytest.raises(ValueError, match=f"head dim {D} is not supported on an FP8 cache"):
                fa(qd, kd, kd, sl, 1.0, 1.0, 128, block_table=bt)
        with pytest.raises(TypeError, match="k_scale must be a Python float or a floating-point tensor"):
            fa(q, kc, kc, sl, torch.ones(Hkv, dtype=torch.int32), 1.0, 128, block_table=bt)
        with pytest.raises(ValueError, match=r"v_scale must broadcast to \[B, Hkv\] = \[2, 2\]"):
            fa(q, kc, kc, sl, 1.0, torch.ones(H), 128, block_table=bt)
        with pytest.raises(RuntimeError, match="k_scale is on meta"):
            fa(q, kc, kc, sl, torch.ones(Hkv, device="meta"), 1.0, 128, block_table=bt)
        wide = torch.zeros(4, 64, Hkv, 72, dtype=torch.uint8).view(k8.F8)[..., :64]
        with pytest.raises(ValueError, match="strides % 16 elements"):
            fa(q, wide, wide, sl, 1.0, 1.0, 128, block_table=bt)
        with pytest.raises(ValueError, match="page_size 32 is not supported"):
            fa(q, kc[:, :32], kc[:, :32], sl, 1.0, 1.0, 128, block_table=bt)
        with pytest.raises(ValueError, match="query_seqlens must be a contiguous int32 tensor of shape \\[2\\]"):
            fa(q, kc, kc, sl, 1.0, 1.0, 128, block_table=bt, query_seqlens=sl.long())
        # flash_attention_n_kvcache_fp8 itself still refuses, with a message that begins as it did
        for name, value in (("window", 128), ("rotary_cos", torch.zeros(128, 16)), ("rotary_sin", torch.zeros(128, 16)), ("alibi_slopes", torch.ones(H)),
                            ("cu_seqlens_q", sl), ("tree_mask", torch.zeros(B, Sq, dtype=torch.int64))):
            with pytest.raises(NotImplementedError, match=f"{name} is not supported on an FP8 cache"):
                pkg.flash_attention_n_kvcache_fp8(q, kc, kc, sl, 1.0, 1.0, block_table=bt, **{name: value})
        with pytest.raises(NotImplementedError, match="flash_attention_n_kvcache_fp8_window"):
            pkg.flash_attention_n_kvcache_fp8(q, kc, kc, sl, 1.0, 1.0, block_table=bt, window=128)
        with pytest.raises(NotImplementedError, match="flash_attention_n_kvcache_fp8_rope"):
            pkg.flash_attention_n_kvcache_fp8(q, kc, kc, sl, 1.0, 1.0, block_table=bt, rotary_cos=torch.zeros(128, 16))


def test_rope_front_end_refuses_with_the_reason(pkg):
    fa = pkg.flash_attention_n_kvcache_fp8_rope
    B, H, Hkv = 2, 8, 2
    for Sq in (1, 40):
        q, kc, sl, bt = _cpu_case(Sq)
        cos, sin = torch.zeros(128, 32), torch.zeros(128, 32)
        with pytest.raises(RuntimeError, match="MI355X device tensors only"):   # every check passed
            fa(q, kc, kc, sl, 1.0, 0.5, cos, sin, block_table=bt)
        with pytest.raises(RuntimeError, match="MI355X device tensors only"):
            fa(q, kc, kc, sl, torch.ones(Hkv), torch.ones(B, 1), cos.half()[:, :16], sin.half()[:, :16], block_table=bt, k_new=q[:, :Hkv], v_new=q[:, :Hkv],
               query_seqlens=sl, window=96, rotary_interleaved=True, return_lse=True)
        with pytest.raises(ValueError, match="a sliding window is always causal"):
            fa(q, kc, kc, sl, 1.0, 1.0, cos, sin, block_table=bt, window=96, is_causal=False)
        with pytest.raises(ValueError, match="window must be >= 1"):
            fa(q, kc, kc, sl, 1.0, 1.0, cos, sin, block_table=bt, window=0)
        with pytest.raises(TypeError, match="window must be None or a Python int"):
            fa(q, kc, kc, sl, 1.0, 1.0, cos, sin, block_table=bt, window=96.0)
        with pytest.raises(ValueError, match=r"rotary_cos must be a \[rows, rotary_dim / 2\] tensor"):
            fa(q, kc, kc, sl, 1.0, 1.0, None, sin, block_table=bt)
        with pytest.raises(ValueError, match="must have one shape, dtype and row stride"):
            fa(q, kc, kc, sl, 1.0, 1.0, cos, sin[:, :16], block_table=bt)
        with pytest.raises(ValueError, match="must be float32 or the dtype of query"):
            fa(q, kc, kc, sl, 1.0, 1.0, cos.bfloat16(), sin.bfloat16(), block_table=bt)
        with pytest.raises(ValueError, match="rotary_dim = 2 x 12 = 24 is not supported"):
            fa(q, kc, kc, sl, 1.0, 1.0, cos[:, :12].contiguous(), sin[:, :12].contiguous(), block_table=bt)
        with pytest.raises(ValueError, match="the rotary tables cover 100 positions but the cache holds up to 128"):
            fa(q, kc, kc, sl, 1.0, 1.0, cos[:100], sin[:100], block_table=bt)
        with pytest.raises(ValueError, match="rows must be 16-byte aligned"):
            fa(q, kc, kc, sl, 1.0, 1.0, torch.zeros(128, 34)[:, 2:], torch.zeros(128, 34)[:, 2:], block_table=bt)
        with pytest.raises(TypeError, match="must be torch.float8_e4m3fn"):
            fa(q, kc.view(torch.uint8), kc.view(torch.uint8), sl, 1.0, 1.0, cos, sin, block_table=bt)
        for D in (32, 256):
            qd, kd, _sl, _bt = _cpu_case(Sq, D)
            with pytest.raises(ValueError, match=f"head dim {D} is not supported on an FP8 cache"):
                fa(qd, kd, kd, sl, 1.0, 1.0, torch.zeros(128, 16), torch.zeros(128, 16), block_table=bt)
        with pytest.raises(TypeError, match="v_scale must be a Python float or a floating-point tensor"):
            fa(q, kc, kc, sl, 1.0, None, cos, sin, block_table=bt)
        with pytest.raises(RuntimeError, match="forward only"):
            fa(q, kc, kc, sl, torch.ones(Hkv, requires_grad=True), 1.0, cos, sin, block_table=bt)
        with pytest.raises(ValueError, match="k_new and v_new come together"):
            fa(q, kc, kc, sl, 1.0, 1.0, cos, sin, block_table=bt, k_new=q[:, :Hkv])
        with pytest.raises(ValueError, match="k_new must be"):
            fa(q, kc, kc, sl, 1.0, 1.0, cos, sin, block_table=bt, k_new=q[:, :Hkv].float(), v_new=q[:, :Hkv].float())


def test_signatures_and_exports(pkg):
    import flash_attention_softmax_n_amd as shim
    for name in ("flash_attention_n_kvcache_fp8_window", "flash_attention_n_kvcache_fp8_rope"):
        assert name in pkg.__all__ and getattr(shim, name) is getattr(pkg.kvcache, name)
    sig = inspect.signature(pkg.flash_attention_n_kvcache_fp8_window)
    assert list(sig.parameters) == ["query", "k_cache", "v_cache", "cache_seqlens", "k_scale", "v_scale", "window", "block_table", "k_new", "v_new",
                                    "query_seqlens", "softmax_n_param", "scale", "return_lse"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(block_table=None, k_new=None, v_new=None, query_seqlens=None, softmax_n_param=1, scale=None, return_lse=False)
    sig = inspect.signature(pkg.flash_attention_n_kvcache_fp8_rope)
    assert list(sig.parameters) == ["query", "k_cache", "v_cache", "cache_seqlens", "k_scale", "v_scale", "rotary_cos", "rotary_sin", "block_table",
                                    "k_new", "v_new", "query_seqlens", "softmax_n_param", "scale", "is_causal", "return_lse", "window",
                                    "rotary_interleaved"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(block_table=None, k_new=None, v_new=None, query_seqlens=None, softmax_n_param=1, scale=None, is_causal=True, return_lse=False,
                     window=None, rotary_interleaved=False)
    # the calls that were there are what they were
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_fp8).parameters)[-6:] == ["alibi_slopes", "window", "rotary_cos", "rotary_sin",
                                                                                         "cu_seqlens_q", "tree_mask"]
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_window).parameters)[-1] == "return_lse"
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_rope).parameters)[-1] == "rotary_interleaved"
