"""flash_attention_n_kvcache_varlen_window / flash_attention_n_kvcache_varlen_rope without a GPU: the front end's refusals (CPU tensors: the
argument checks come before the device check), the order of the C ABI's checks on fasn_fwd_kvvarlen_window and fasn_kvvarlen_rope_append
(the packed block's rules first, then the operand's with the operand's codes), the recorded launch plans
(tests/golden/kvvarlen_layer_plans.txt), a Python mirror of the split rule under a window, and the registers of the new kernels.

Nothing is ever launched: the pointers are fake. The calls that would launch are only made with blocks that are refused; accepted blocks go
through the *_plan and *_workspace_bytes calls.

    python tests/test_kvvarlen_layer_cpu.py --record     rewrites the fixture from the library of this tree
"""
import ctypes
import inspect
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kv_args as ka   # noqa: E402

DUMMY, BIG = ka.DUMMY, ka.BIG
PLANS = os.path.join(ROOT, "tests", "golden", "kvvarlen_layer_plans.txt")
EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED, EWORKSPACE = -1, -2, -3, -4, -5, -7, -8
NEW = ("fasn_fwd_kvvarlen_window_workspace_bytes", "fasn_fwd_kvvarlen_window", "fasn_kvvarlen_window_plan", "fasn_kvvarlen_rope_append",
       "fasn_kvvarlen_rope_append_plan")
DIMS = (32, 64, 128, 256)
TAGS = {0: "fasn::f16_tag", 1: "fasn::bf16_tag"}
_args, items_max, _win, _tview = ka._args_varlen, ka.items_max, ka._win, ka._tview


def _appended(pkg, **kw):
    va = _args(pkg, **kw)
    va.pf.kv.seqlen_add = va.pf.kv.Sq
    return va


# ---------------------------------------------------------------- exports
def test_symbols_are_exported_and_bound(pkg):
    import flash_attention_softmax_n_amd as shim
    lib = shim._lib.load()
    for name in NEW:
        assert name in shim._lib.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.fasn_abi_version() == 6
    for name in ("flash_attention_n_kvcache_varlen_window", "flash_attention_n_kvcache_varlen_rope"):
        assert name in pkg.__all__ and getattr(shim, name) is getattr(pkg, name)
    w = inspect.signature(pkg.flash_attention_n_kvcache_varlen_window)
    assert list(w.parameters) == ["query", "k_cache", "v_cache", "cache_seqlens", "cu_seqlens_q", "max_seqlen_q", "window", "block_table", "k_new",
                                  "v_new", "softmax_n_param", "scale", "return_lse"]
    r = inspect.signature(pkg.flash_attention_n_kvcache_varlen_rope)
    assert list(r.parameters) == ["query", "k_cache", "v_cache", "cache_seqlens", "cu_seqlens_q", "max_seqlen_q", "rotary_cos", "rotary_sin",
                                  "block_table", "k_new", "v_new", "softmax_n_param", "scale", "is_causal", "return_lse", "window",
                                  "rotary_interleaved"]
    assert r.parameters["window"].default is None and r.parameters["is_causal"].default is True and r.parameters["rotary_interleaved"].default is False


# ---------------------------------------------------------------- the front end
def _operands():
    f16 = torch.float16
    return dict(q=torch.zeros(10, 8, 64, dtype=f16), kc=torch.zeros(4, 64, 2, 64, dtype=f16), sl=torch.zeros(2, dtype=torch.int32),
                cu=torch.tensor([0, 4, 9], dtype=torch.int32), bt=torch.zeros(2, 2, dtype=torch.int32), kn=torch.zeros(10, 2, 64, dtype=f16),
                cos=torch.zeros(128, 32), sin=torch.zeros(128, 32))


def _packed_refusals(fn, call):
    """every refusal the packed calls share, through `call(q, kc, sl, cu, max_seqlen_q, bt, **kw)`, with the function's own name"""
    o = _operands()
    q, kc, sl, cu, bt, kn = o["q"], o["kc"], o["sl"], o["cu"], o["bt"], o["kn"]
    f16 = torch.float16
    with pytest.raises(RuntimeError, match="CPU tensor"):      # arguments that are right get as far as the device check
        call(q, kc, sl, cu, 8, bt)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        call(q, kc, sl, cu, 8, bt, k_new=kn, v_new=kn, softmax_n_param=torch.ones(2, 8), return_lse=True)
    with pytest.raises(RuntimeError, match="CPU tensor"):      # a bound beyond the buffer is a bound
        call(q, kc, sl, cu, 1 << 20, bt)
    for bad in (torch.zeros(2, 8, 5, 64, dtype=f16), torch.zeros(10, 64, dtype=f16)):
        with pytest.raises(ValueError, match=fn + r": query must be token-packed \[T, H, D\]"):
            call(bad, kc, sl, cu, 8, bt)
    for bad in (cu.long(), cu.view(3, 1), torch.zeros(6, dtype=torch.int32)[::2], [0, 4, 9], torch.zeros(1, dtype=torch.int32)):
        with pytest.raises(ValueError, match=fn + r": cu_seqlens_q must be a contiguous int32 tensor of shape \[B \+ 1\]"):
            call(q, kc, sl, bad, 8, bt)
    with pytest.raises(RuntimeError, match="cu_seqlens_q is on meta, query on cpu"):
        call(q, kc, sl, cu.to("meta"), 8, bt)
    with pytest.raises(ValueError, match=fn + ": cu_seqlens_q names 3 sequences but cache_seqlens has 2"):
        call(q, kc, sl, torch.tensor([0, 4, 9, 9], dtype=torch.int32), 8, bt)
    with pytest.raises(ValueError, match="block_table has 3 rows but the batch is 2"):
        call(q, kc, sl, cu, 8, torch.zeros(3, 2, dtype=torch.int32))
    for bad in (8.0, torch.tensor(8), True, None):
        with pytest.raises(TypeError, match=fn + ": max_seqlen_q must be a Python int"):
            call(q, kc, sl, cu, bad, bt)
    with pytest.raises(ValueError, match=fn + ": max_seqlen_q must be >= 1; got 0"):
        call(q, kc, sl, cu, 0, bt)
    with pytest.raises(ValueError, match=fn + ": the token buffer is empty"):
        call(q[:0], kc, sl, cu, 8, bt)
    with pytest.raises(ValueError, match="k_new and v_new come together"):
        call(q, kc, sl, cu, 8, bt, k_new=kn)
    for bad in (torch.zeros(2, 2, 5, 64, dtype=f16), torch.zeros(9, 2, 64, dtype=f16), torch.zeros(10, 8, 64, dtype=f16), kn.bfloat16()):
        with pytest.raises(ValueError, match=r"k_new must be \[T, Hkv, D\] = \[10, 2, 64\]"):
            call(q, kc, sl, cu, 8, bt, k_new=bad, v_new=bad)
    for bad in (torch.ones(10, 8), torch.ones(3, 8), torch.ones(2, 8, 1)):
        with pytest.raises(ValueError, match=r"softmax_n_param must broadcast to \[B, H\] = \[2, 8\]"):
            call(q, kc, sl, cu, 8, bt, softmax_n_param=bad)
    with pytest.raises(ValueError, match=fn + ": head dim 96"):
        k96 = torch.zeros(4, 64, 2, 96, dtype=f16)
        call(torch.zeros(10, 8, 96, dtype=f16), k96, sl, cu, 8, bt)
    with pytest.raises(ValueError, match=fn + ".*fp16 and bf16"):
        call(q.float(), kc.float(), sl, cu, 8, bt)
    with pytest.raises(ValueError, match="page_size 16"):
        call(q, torch.zeros(4, 16, 2, 64, dtype=f16), sl, cu, 8, bt)
    with pytest.raises(ValueError, match=fn + ": 256 query heads per K/V head"):
        call(torch.zeros(10, 256, 64, dtype=f16), torch.zeros(4, 64, 1, 64, dtype=f16), sl, cu, 8, bt)
    with pytest.raises(RuntimeError, match=fn + " is forward only"):
        call(q.clone().requires_grad_(), kc, sl, cu, 8, bt)


def test_window_front_end_refuses_with_the_reason(pkg):
    fn = "flash_attention_n_kvcache_varlen_window"
    fa = pkg.flash_attention_n_kvcache_varlen_window
    _packed_refusals(fn, lambda q, kc, sl, cu, mq, bt, **kw: fa(q, kc, kc, sl, cu, mq, 128, block_table=bt, **kw))
    o = _operands()
    for bad in (128.0, torch.tensor(128), True, None):
        with pytest.raises(TypeError, match=fn + ": window must be a Python int"):
            fa(o["q"], o["kc"], o["kc"], o["sl"], o["cu"], 8, bad, block_table=o["bt"])
    for bad in (0, -5):
        with pytest.raises(ValueError, match=fn + f": window must be >= 1 .*got {bad}"):
            fa(o["q"], o["kc"], o["kc"], o["sl"], o["cu"], 8, bad, block_table=o["bt"])
    with pytest.raises(RuntimeError, match="CPU tensor"):      # any window >= 1, one beyond the capacity (and beyond int32) included
        fa(o["q"], o["kc"], o["kc"], o["sl"], o["cu"], 8, 1 << 40, block_table=o["bt"])
    with pytest.raises(TypeError):                              # always causal: there is no is_causal to turn off
        fa(o["q"], o["kc"], o["kc"], o["sl"], o["cu"], 8, 128, block_table=o["bt"], is_causal=False)


def test_rope_front_end_refuses_with_the_reason(pkg):
    fn = "flash_attention_n_kvcache_varlen_rope"
    fa = pkg.flash_attention_n_kvcache_varlen_rope
    o = _operands()
    q, kc, sl, cu, bt, cos, sin = o["q"], o["kc"], o["sl"], o["cu"], o["bt"], o["cos"], o["sin"]
    _packed_refusals(fn, lambda q_, kc_, sl_, cu_, mq, bt_, **kw: fa(q_, kc_, kc_, sl_, cu_, mq, cos, sin, block_table=bt_, **kw))
    for kw in (dict(window=64), dict(rotary_interleaved=True), dict(is_causal=False), dict(window=1 << 40)):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            fa(q, kc, kc, sl, cu, 8, cos, sin, block_table=bt, **kw)
    with pytest.raises(RuntimeError, match="CPU tensor"):      # 16-bit tables, rotary_dim 16, a longer table
        fa(q, kc, kc, sl, cu, 8, torch.zeros(500, 8, dtype=torch.float16), torch.zeros(500, 8, dtype=torch.float16), block_table=bt)
    # the window
    for bad in (64.0, torch.tensor(64), True):
        with pytest.raises(TypeError, match=fn + ": window must be None or a Python int"):
            fa(q, kc, kc, sl, cu, 8, cos, sin, block_table=bt, window=bad)
    with pytest.raises(ValueError, match=fn + ": window must be >= 1"):
        fa(q, kc, kc, sl, cu, 8, cos, sin, block_table=bt, window=0)
    with pytest.raises(ValueError, match=fn + ": a sliding window is always causal; window=64 needs is_causal=True"):
        fa(q, kc, kc, sl, cu, 8, cos, sin, block_table=bt, window=64, is_causal=False)
    # the tables
    for bad in (None, [1.0], torch.zeros(128), torch.zeros(1, 128, 32)):
        with pytest.raises(ValueError, match=fn + r": rotary_cos must be a \[rows, rotary_dim / 2\] tensor"):
            fa(q, kc, kc, sl, cu, 8, bad, sin, block_table=bt)
        with pytest.raises(ValueError, match=fn + r": rotary_sin must be a \[rows, rotary_dim / 2\] tensor"):
            fa(q, kc, kc, sl, cu, 8, cos, bad, block_table=bt)
    for bad in (torch.zeros(128, 16), torch.zeros(129, 32), cos.half(), torch.zeros(128, 64)[:, :32]):
        with pytest.raises(ValueError, match=fn + ": rotary_cos and rotary_sin must have one shape, dtype and row stride"):
            fa(q, kc, kc, sl, cu, 8, cos, bad, block_table=bt)
    with pytest.raises(ValueError, match=fn + r": rotary_cos / rotary_sin must be float32 or the dtype of query \(torch.float16\); got torch.bfloat16"):
        fa(q, kc, kc, sl, cu, 8, cos.bfloat16(), sin.bfloat16(), block_table=bt)
    with pytest.raises(RuntimeError, match="rotary_cos is on meta, query on cpu"):
        fa(q, kc, kc, sl, cu, 8, cos.to("meta"), sin.to("meta"), block_table=bt)
    for half in (4, 12, 40):
        with pytest.raises(ValueError, match=fn + f": rotary_dim = 2 x {half} = {2 * half} is not supported"):
            fa(q, kc, kc, sl, cu, 8, torch.zeros(128, half), torch.zeros(128, half), block_table=bt)
    with pytest.raises(ValueError, match=fn + ": the rotary tables cover 127 positions but the cache holds up to 128"):
        fa(q, kc, kc, sl, cu, 8, cos[:127], sin[:127], block_table=bt)
    wide = torch.zeros(128, 34)
    with pytest.raises(ValueError, match=fn + ": rotary_cos: rows must be 16-byte aligned"):
        fa(q, kc, kc, sl, cu, 8, wide[:, :32], wide[:, :32], block_table=bt)           # a row stride of 136 bytes
    with pytest.raises(ValueError, match=fn + ": rotary_cos: rows must be 16-byte aligned"):
        fa(q, kc, kc, sl, cu, 8, torch.zeros(128, 64)[:, ::2], torch.zeros(128, 64)[:, ::2], block_table=bt)   # column stride 2
    # the packed checks come in front of the tables'
    with pytest.raises(ValueError, match=fn + r": query must be token-packed \[T, H, D\]"):
        fa(torch.zeros(2, 8, 5, 64, dtype=torch.float16), kc, kc, sl, cu, 8, None, None, block_table=bt)


# ---------------------------------------------------------------- the order of the C ABI's checks
def _base_breaks(pkg):
    """(a block that breaks one rule of fasn_fwd_kvvarlen, its code): base rules and packed rules"""
    def broken(code, fix, **kw):
        va = _appended(pkg, **kw)
        if fix is not None:
            fix(va)
        return va, code
    yield None, EINVAL
    yield broken(EINVAL, None, B=0)
    yield broken(EDTYPE, None, dtype=2)
    yield broken(EHEADDIM, None, D=96)
    yield broken(EUNSUPPORTED, None, page=48)
    yield broken(EINVAL, lambda va: setattr(va.pf.kv, "kv_group", 7))
    yield broken(EALIGN, lambda va: setattr(va.pf.kv.q, "ptr", DUMMY + 2))
    yield broken(ESTRIDE, lambda va: va.pf.kv.q.stride.__setitem__(3, 2))
    yield broken(EINVAL, None, seqlens=None)
    yield broken(EINVAL, lambda va: setattr(va.pf.kv, "seqlen_add", 3), Sq=17)
    yield broken(EINVAL, None, cu=None)                                             # the packed block's own rules
    yield broken(EINVAL, lambda va: setattr(va.pf, "q_seqlens", DUMMY + 4096))
    yield broken(EINVAL, None, T=0)
    yield broken(EINVAL, lambda va: setattr(va, "reserved", 1))
    yield broken(EALIGN, None, cu=DUMMY + 2)


def test_window_return_codes(pkg):
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    good = _win(pkg)
    # the base packed rules come before the operand's, whatever the operand is
    for w in (good, None, _win(pkg, 0), _win(pkg, 128, reserved=1)):
        for va, code in _base_breaks(pkg):
            assert lib.fasn_kvvarlen_window_plan(va, w, buf, len(buf)) == code, (code, w)
            assert lib.fasn_fwd_kvvarlen_window(va, w, 256, BIG, None) == code
            assert lib.fasn_fwd_kvvarlen_window_workspace_bytes(va, w) == 0
    # then the operand
    for w in (None, _win(pkg, 0), _win(pkg, -3), _win(pkg, 128, reserved=1)):
        assert lib.fasn_kvvarlen_window_plan(_args(pkg), w, buf, len(buf)) == EINVAL
        assert lib.fasn_fwd_kvvarlen_window(_args(pkg), w, 256, BIG, None) == EINVAL
        assert lib.fasn_fwd_kvvarlen_window_workspace_bytes(_args(pkg), w) == 0
    nc = _args(pkg)
    nc.pf.kv.causal = 0
    assert lib.fasn_kvvarlen_window_plan(nc, good, buf, len(buf)) == EUNSUPPORTED
    assert lib.fasn_fwd_kvvarlen_window(nc, good, 256, BIG, None) == EUNSUPPORTED
    assert lib.fasn_kvvarlen_window_plan(nc, _win(pkg, 0), buf, len(buf)) == EINVAL   # the operand's own values before what it asks of the block
    # accepted: any window >= 1; the workspace is always asked for (the item table), NULL / short EWORKSPACE, misaligned EALIGN
    for W in (1, 128, 1 << 13, 2 ** 31 - 1):
        for c in ka.plan_cases().values():
            va = _args(pkg, **c)
            assert lib.fasn_kvvarlen_window_plan(va, _win(pkg, W), buf, len(buf)) > 0
            assert lib.fasn_fwd_kvvarlen_window_workspace_bytes(va, _win(pkg, W)) >= 32
            assert lib.fasn_fwd_kvvarlen_window(va, _win(pkg, W), None, BIG, None) == EWORKSPACE
            assert lib.fasn_fwd_kvvarlen_window(va, _win(pkg, W), 256, 8, None) == EWORKSPACE
            assert lib.fasn_fwd_kvvarlen_window(va, _win(pkg, W), 260, BIG, None) == EALIGN
    assert lib.fasn_kvvarlen_window_plan(_args(pkg), good, None, 10) == EINVAL
    assert lib.fasn_kvvarlen_window_plan(_args(pkg), good, buf, 8) == EINVAL


def test_rope_return_codes(pkg):
    """the operand's codes as tests/test_kvrope_cpu.py has them for the padded calls"""
    lib = pkg._lib.load()
    H, Hkv, D, CAP = 64, 8, 64, ka.CAPACITY
    _rope = ka._rope
    qo, kn = _tview(pkg, H, D), _tview(pkg, Hkv, D)
    buf = ctypes.create_string_buffer(4096)

    def plan(a, r, q_, k_, v_):
        rc = lib.fasn_kvvarlen_rope_append_plan(a, r, q_, k_, v_, buf, len(buf))
        return rc if rc < 0 else 0

    for call in (lambda a, r, q_, k_, v_: lib.fasn_kvvarlen_rope_append(a, r, q_, k_, v_, None), plan):
        good = _rope(pkg)
        for r in (good, None, _rope(pkg, rd=8)):   # the base packed rules first
            for va, code in _base_breaks(pkg):
                assert call(va, r, qo, kn, kn) == code, code
        ap = lambda **kw: _appended(pkg, **kw)   # noqa: E731
        assert call(ap(), None, qo, kn, kn) == EINVAL
        assert call(ap(), _rope(pkg, cos=None), qo, kn, kn) == EINVAL and call(ap(), _rope(pkg, sin=None), qo, kn, kn) == EINVAL
        assert call(ap(), good, None, kn, kn) == EINVAL
        assert call(ap(), good, qo, kn, None) == EINVAL and call(ap(), good, qo, None, kn) == EINVAL
        assert call(_args(pkg), good, qo, kn, kn) == EINVAL                      # k_new / v_new given: seqlen_add == Sq
        for rd in (0, 8, 24, 40, 80, 128, -16):
            assert call(ap(), _rope(pkg, rd=rd, row_stride=64), qo, kn, kn) == EINVAL, rd
        assert call(ap(), _rope(pkg, rows=CAP - 1), qo, kn, kn) == EINVAL and call(ap(), _rope(pkg, rows=0), qo, kn, kn) == EINVAL
        assert call(ap(), _rope(pkg, interleaved=2), qo, kn, kn) == EINVAL and call(ap(), _rope(pkg, interleaved=-1), qo, kn, kn) == EINVAL
        assert call(ap(dtype=1), _rope(pkg, table_dtype=0), qo, kn, kn) == EDTYPE
        assert call(ap(dtype=0), _rope(pkg, table_dtype=1), qo, kn, kn) == EDTYPE
        assert call(ap(), _rope(pkg, table_dtype=3), qo, kn, kn) == EDTYPE
        assert call(ap(), _rope(pkg, cos=DUMMY + 4), qo, kn, kn) == EALIGN and call(ap(), _rope(pkg, sin=DUMMY + 8), qo, kn, kn) == EALIGN
        assert call(ap(), _rope(pkg, row_stride=34), qo, kn, kn) == EALIGN
        assert call(ap(), _rope(pkg, table_dtype=1, row_stride=36), qo, kn, kn) == EALIGN
        assert call(ap(), _rope(pkg, row_stride=16), qo, kn, kn) == EINVAL
        v = _tview(pkg, H, D)
        v.stride[3] = 2
        assert call(ap(), good, v, kn, kn) == ESTRIDE
        assert call(ap(), good, _tview(pkg, H, D, ptr=DUMMY + 2), kn, kn) == EALIGN
        assert call(ap(), good, _tview(pkg, H, D, ptr=None), kn, kn) == EINVAL
        v = _tview(pkg, H, D)
        v.stride[1] = 68
        assert call(ap(), good, v, kn, kn) == EALIGN
        v = _tview(pkg, Hkv, D)
        v.stride[3] = 2
        assert call(ap(), good, qo, v, kn) == ESTRIDE and call(ap(), good, qo, kn, v) == ESTRIDE
        assert call(ap(), good, qo, _tview(pkg, Hkv, D, ptr=DUMMY + 2), kn) == EALIGN
    # accepted (plan only): every legal rotary_dim and table dtype, a longer table, a wide row stride, queries only
    for D2 in DIMS:
        for rd in range(16, D2 + 1, 16):
            for td in (2, 1):
                assert plan(_appended(pkg, D=D2), _rope(pkg, rd=rd, table_dtype=td, interleaved=rd // 16 % 2, rows=CAP + 5, row_stride=128),
                            _tview(pkg, H, D2), _tview(pkg, Hkv, D2), _tview(pkg, Hkv, D2)) == 0
    assert plan(_args(pkg), _rope(pkg), qo, None, None) == 0
    assert lib.fasn_kvvarlen_rope_append_plan(_appended(pkg), _rope(pkg), qo, kn, kn, None, 10) == EINVAL
    assert lib.fasn_kvvarlen_rope_append_plan(_appended(pkg), _rope(pkg), qo, kn, kn, ctypes.create_string_buffer(8), 8) == EINVAL


# ---------------------------------------------------------------- launch plans
GOLDEN_WINDOWS = (1, 128, 3000)


def plan_lines(pkg):
    lib = pkg._lib.load()
    got = []
    for name, c in sorted(ka.plan_cases().items()):
        for W in GOLDEN_WINDOWS:
            va = _args(pkg, **c)
            buf = ctypes.create_string_buffer(4096)
            rc = lib.fasn_kvvarlen_window_plan(va, _win(pkg, W), buf, len(buf))
            assert rc > 0, (name, W, rc)
            got += [f"{name} W={W} {line}" for line in buf.value.decode().splitlines()]
            got.append(f"{name} W={W} workspace={lib.fasn_fwd_kvvarlen_window_workspace_bytes(va, _win(pkg, W))}")
        H, Hkv, D = c["H"], c["Hkv"], c["D"]
        for new in (True, False):
            va = _appended(pkg, **c) if new else _args(pkg, **c)
            kn = _tview(pkg, Hkv, D) if new else None
            buf = ctypes.create_string_buffer(4096)
            rc = lib.fasn_kvvarlen_rope_append_plan(va, ka._rope(pkg, rows=c["page"] * c["max_pages"], rd=min(D, 64)), _tview(pkg, H, D), kn, kn, buf, len(buf))
            assert rc > 0, (name, new, rc)
            got += [f"{name} rope{'+append' if new else ''} {line}" for line in buf.value.decode().splitlines()]
    return got


def test_launch_plans_equal_the_recorded_ones(pkg):
    assert plan_lines(pkg) == open(PLANS).read().splitlines()


def window_nsplit(B, max_seqlen_q, T, G, W, capacity, D=64):
    """the split rule of fasn_fwd_kvvarlen_window, from include/fasn.h: the prefill rule - as many splits as bring the blocks to 1024
    workgroups (512 at D = 256), each with at least 16 tiles - over items_max * Hkv blocks (Hkv is the caller's: returned per K/V head
    count by the lambda) and min(capacity tiles, ceil((W + PB - 1) / 64) + 1) tiles; W = None: the base rule over the capacity's tiles"""
    PB = 128 // G
    items = items_max(B, max_seqlen_q, T, PB)
    cap_tiles = -(-capacity // 64)
    tiles = cap_tiles if W is None else min(cap_tiles, -(-(W + PB - 1) // 64) + 1)
    return items, lambda Hkv: max(1, min(-(-(512 if D == 256 else 1024) // (items * Hkv)), tiles // 16))


SWEEP = [(B, mq, T, G, W, pages)
         for B, mq, T in ((1, 1, 1), (3, 40, 51), (4, 48, 64), (6, 100, 300), (256, 2048, 2303), (257, 4096, 4352), (64, 1, 64))
         for G in (1, 3, 8, 128)
         for W in (1, 5, 64, 128, 200, 1000, 3000, 5000, 1 << 20)
         for pages in (1, 4, 16, 64)]


@pytest.mark.parametrize("D", [64, 256])
def test_window_split_rule_mirror_equals_the_plan(pkg, D):
    lib = pkg._lib.load()
    seen = set()
    for B, mq, T, G, W, pages in SWEEP:
        Hkv = 2 if G < 128 else 1
        c = dict(B=B, H=G * Hkv, Hkv=Hkv, Sq=mq, D=D, page=256, max_pages=pages, T=T)
        tag = "fasn::bf16_tag, %d" % D
        items, rule = window_nsplit(B, mq, T, G, W, 256 * pages, D)
        nsplit = rule(Hkv)
        plan = pkg._lib.kvvarlen_window_plan(_args(pkg, **c), _win(pkg, W))
        want = ["fasn_kvvarlen_schedule_kernel<256>", f"fasn_kvvarlen_fwd_window_kernel<{tag}>"] + ([f"fasn_kvvarlen_combine_kernel<{tag}>"] if nsplit > 1 else [])
        assert [k[0] for k in plan] == want, (c, W, plan)
        assert plan[0][1:] == (1, 256, 0) and plan[1][1] == items * Hkv * nsplit, (c, W, plan, nsplit)
        # never more splits than the base plan on the same block; the same LDS and block size
        base = pkg._lib.kvvarlen_plan(_args(pkg, **c))
        base_nsplit = window_nsplit(B, mq, T, G, None, 256 * pages, D)[1](Hkv)
        assert base[1][1] == items * Hkv * base_nsplit and nsplit <= base_nsplit and plan[1][2:] == base[1][2:]
        ws = lib.fasn_fwd_kvvarlen_window_workspace_bytes(_args(pkg, **c), _win(pkg, W))
        assert ws == 16 + 16 * items + (items * Hkv * nsplit * 128 * (D + 2) * 4 if nsplit > 1 else 0) <= lib.fasn_fwd_kvvarlen_workspace_bytes(_args(pkg, **c))
        if W >= 256 * pages:   # a window at or beyond the capacity: the base plan under the window kernel's name
            assert [(k[0].replace("_fwd_kernel<", "_fwd_window_kernel<"),) + k[1:] for k in base] == plan
        # other offsets and lengths (other device pointers), the rows appended or not: the same launches
        other = _args(pkg, cu=DUMMY + 64, seqlens=DUMMY + 4096, **c)
        other.pf.kv.seqlen_add = mq
        assert pkg._lib.kvvarlen_window_plan(other, _win(pkg, W)) == plan
        seen.add((nsplit > 1, nsplit < base_nsplit))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}, seen


def test_the_several_splits_case_of_the_gpu_tests(pkg):
    """H/Hkv 8/1, D 64, page 256, 16 pages, qlens [1, 40, 3] + 7 tail rows, W = 3000: items_max = 6, 49 tiles, 16 per split: 3 splits"""
    c = dict(B=3, H=8, Hkv=1, Sq=40, D=64, page=256, max_pages=16, T=51)
    assert items_max(3, 40, 51, 16) == 6 and window_nsplit(3, 40, 51, 8, 3000, 4096)[1](1) == 3
    assert pkg._lib.kvvarlen_window_plan(_args(pkg, **c), _win(pkg, 3000))[1][1] == 6 * 3


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("dtype", [0, 1])
def test_rope_plan_is_one_launch_whose_grid_depends_on_shapes_only(pkg, dtype, D):
    for c in (dict(B=4, H=64, Hkv=8, Sq=48, T=64), dict(B=3, H=8, Hkv=2, Sq=3, T=1), dict(B=257, H=16, Hkv=16, Sq=4096, T=4352), dict(B=2, H=12, Hkv=4, Sq=70, T=77)):
        H, Hkv, T = c["H"], c["Hkv"], c["T"]
        qo, kn = _tview(pkg, H, D), _tview(pkg, Hkv, D)
        rope = ka._rope(pkg, rd=16)
        plan = pkg._lib.kvrope_plan(_appended(pkg, D=D, dtype=dtype, **c), rope, qo, kn, kn)
        assert plan == [(f"fasn_kvvarlen_rope_kernel<{TAGS[dtype]}, {D}>", -(-((T * Hkv + T * H) * (D // 16)) // 256), 256, 0)]
        only_q = pkg._lib.kvrope_plan(_args(pkg, D=D, dtype=dtype, **c), rope, qo)
        assert only_q == [(plan[0][0], -(-(T * H * (D // 16)) // 256), 256, 0)]
        other = _appended(pkg, D=D, dtype=dtype, cu=DUMMY + 64, seqlens=DUMMY + 4096, **c)   # other offsets and lengths: the same launch
        assert pkg._lib.kvrope_plan(other, ka._rope(pkg, rd=16, interleaved=1, table_dtype=dtype), qo, kn, kn) == plan


# ---------------------------------------------------------------- registers
@pytest.mark.parametrize("D", DIMS)
def test_new_kernels_do_not_spill(pkg, D):
    import spill_map
    lib = os.path.join(ROOT, "flash-attention-softmax-n_amd", "libfasn.so")
    if not os.path.exists(spill_map.READELF):
        pytest.skip("llvm-readelf not available")
    table = spill_map.kernel_table(lib)
    names = sorted(table)
    pretty = subprocess.run([spill_map.CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_pretty = dict(zip(pretty, names))
    for dtype in (0, 1):
        c = ka.plan_cases()[f"D{D}_G8_small"]
        wanted = [pkg._lib.kvvarlen_window_plan(_args(pkg, dtype=dtype, **c), _win(pkg, 3000))[1][0],
                  pkg._lib.kvrope_plan(_args(pkg, dtype=dtype, **c), ka._rope(pkg, rows=c["page"] * c["max_pages"], rd=16), _tview(pkg, c["H"], D))[0][0]]
        assert wanted == [f"fasn_kvvarlen_fwd_window_kernel<{TAGS[dtype]}, {D}>", f"fasn_kvvarlen_rope_kernel<{TAGS[dtype]}, {D}>"]
        for name in wanted:
            hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
            assert len(hit) == 1, (name, hit)
            v = table[hit[0]]
            assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path.insert(0, ROOT)
    import flash_attention_softmax_n_amd
    text = plan_lines(flash_attention_softmax_n_amd)
    with open(PLANS, "w") as fh:
        fh.write("\n".join(text) + "\n")
    print(f"recorded {len(text)} lines in {PLANS}")
