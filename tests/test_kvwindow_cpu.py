"""The sliding window on the K/V-cache decode and prefill calls, without a GPU: exports and layouts, the validation codes of the six *_window
entry points (fake, aligned pointers: validation comes before any HIP call), their launch plans - the base rule over the tiles a window
can touch, independent of the length and table pointers, equal to tests/golden/kvwindow_plans.txt - the register tables of the 16 new
forward kernels, and the front end's refusals."""
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

DUMMY = ka.DUMMY
NEW = ("fasn_fwd_kvcache_window_workspace_bytes", "fasn_fwd_kvcache_window", "fasn_kvcache_window_plan",
       "fasn_fwd_kvprefill_window_workspace_bytes", "fasn_fwd_kvprefill_window", "fasn_kvprefill_window_plan")
DIMS = (32, 64, 128, 256)
TAGS = {0: "fasn::f16_tag", 1: "fasn::bf16_tag"}
GOLDEN_WINDOWS = (1, 128, 1000)
_win, _renamed = ka._win, ka._renamed


def test_symbols_are_exported_and_bound(pkg):
    import flash_attention_softmax_n_amd as shim
    lib = shim._lib.load()
    for name in NEW:
        assert name in shim._lib.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.fasn_abi_version() == 6
    W = pkg._lib.KvWindow
    assert ctypes.sizeof(W) == 8 and W.window.offset == 0 and W.reserved.offset == 4
    # the argument blocks kept their layouts: the operand travels beside them
    assert pkg._lib.KvPrefillArgs.kv.offset == 0 and pkg._lib.KvPrefillArgs.q_seqlens.offset == ctypes.sizeof(pkg._lib.KvCacheArgs)
    assert pkg._lib.KvCacheArgs.n_stride_h.offset + 8 == ctypes.sizeof(pkg._lib.KvCacheArgs)


def test_validation_codes(pkg):
    lib = pkg._lib.load()
    big = ctypes.c_size_t(-1).value
    buf = ctypes.create_string_buffer(4096)

    def run(which, how):
        stem = "kvcache" if which == "dec" else "kvprefill"

        def call(a, w):
            if how == "plan":
                rc = getattr(lib, f"fasn_{stem}_window_plan")(a, w, buf, len(buf))
                return rc if rc < 0 else 0
            if how == "ws":   # the size call has no code to give: 0 stands for every refusal
                return 0 if getattr(lib, f"fasn_fwd_{stem}_window_workspace_bytes")(a, w) > 0 else None
            return getattr(lib, f"fasn_fwd_{stem}_window")(a, w, DUMMY, big, None)
        return call

    for which, make, kv in (("dec", ka._args_decode, lambda a: a), ("pre", ka._args_prefill, lambda a: a.kv)):
        for how in ("fwd", "plan"):
            call = run(which, how)
            good = _win(pkg)
            # every base code, reached through the window entry points, with a good and with a bad operand: the base arguments come first
            for w in (good, None, _win(pkg, window=0)):
                assert call(None, w) == -1
                assert call(make(pkg, B=0), w) == -1
                assert call(make(pkg, dtype=2), w) == -2 and call(make(pkg, dtype=3), w) == -2
                assert call(make(pkg, D=96), w) == -3
                assert call(make(pkg, page=48), w) == -7
                a = make(pkg)
                kv(a).kv_group = 7
                assert call(a, w) == -1
                a = make(pkg)
                kv(a).q.ptr = kv(a).q.ptr + 2
                assert call(a, w) == -4
                a = make(pkg)
                kv(a).k_stride[1] = 8 * 64 + 4
                assert call(a, w) == -4
                a = make(pkg)
                kv(a).q.stride[3] = 2
                assert call(a, w) == -5
                assert call(make(pkg, seqlens=None), w) == -1
            if which == "dec" or how == "plan":   # (accepted arguments are only ever recorded, never launched)
                assert call(make(pkg, H=64, Hkv=8, Sq=17), good) == (-7 if which == "dec" else 0)   # the decode row limit
            # then the operand
            assert call(make(pkg), None) == -1
            assert call(make(pkg), _win(pkg, window=0)) == -1
            assert call(make(pkg), _win(pkg, window=-1)) == -1
            assert call(make(pkg), _win(pkg, reserved=1)) == -1
            a = make(pkg)
            kv(a).causal = 0
            assert call(a, good) == -7                                                    # always causal
            assert call(a, _win(pkg, window=0)) == -1                                     # (the operand's own rules come before that)
            if how == "plan":   # (accepted arguments are only ever recorded, never launched)
                for w in (1, 5, 128, 8192, 8193, 2 ** 31 - 1):                            # any window >= 1 is legal
                    assert call(make(pkg), _win(pkg, window=w)) == 0
        # the size call: 0 for every refusal
        ws = run(which, "ws")
        assert ws(None, _win(pkg)) is None and ws(make(pkg, D=96), _win(pkg)) is None
        assert ws(make(pkg), None) is None and ws(make(pkg), _win(pkg, window=0)) is None and ws(make(pkg), _win(pkg, reserved=3)) is None
        a = make(pkg)
        kv(a).causal = 0
        assert ws(a, _win(pkg)) is None
    assert lib.fasn_fwd_kvprefill_window(ka._args_prefill(pkg, q_seqlens=DUMMY + 2), _win(pkg), DUMMY, big, None) == -4
    a = ka._args_prefill(pkg, Sq=17)
    a.kv.seqlen_add = 3
    assert lib.fasn_fwd_kvprefill_window(a, _win(pkg), DUMMY, big, None) == -1
    # then the workspace: missing, too small, misaligned - sized by the window call's own size function
    a = ka._args_decode(pkg)
    need = lib.fasn_fwd_kvcache_window_workspace_bytes(a, _win(pkg))
    assert 0 < need <= lib.fasn_fwd_kvcache_workspace_bytes(a)
    assert lib.fasn_fwd_kvcache_window(a, _win(pkg), DUMMY, need - 1, None) == -8
    assert lib.fasn_fwd_kvcache_window(a, _win(pkg), None, need, None) == -8
    assert lib.fasn_fwd_kvcache_window(a, _win(pkg), DUMMY + 4, need, None) == -4
    assert lib.fasn_fwd_kvcache_window(a, None, None, 0, None) == -1                      # (the operand before the workspace)
    a = ka._args_prefill(pkg, **ka.PREFILL_CASES["gqa_chunk_long_cache"])
    wide = _win(pkg, window=1 << 20)                                                      # several splits: the base plan
    need = lib.fasn_fwd_kvprefill_window_workspace_bytes(a, wide)
    assert need == lib.fasn_fwd_kvprefill_workspace_bytes(a) > 0
    assert lib.fasn_fwd_kvprefill_window(a, wide, DUMMY, need - 1, None) == -8
    assert lib.fasn_fwd_kvprefill_window(a, wide, None, need, None) == -8
    assert lib.fasn_fwd_kvprefill_window(a, wide, DUMMY + 4, need, None) == -4
    assert lib.fasn_fwd_kvprefill_window_workspace_bytes(a, _win(pkg)) == 0               # one split under W = 128: no workspace at all
    assert lib.fasn_kvcache_window_plan(ka._args_decode(pkg), _win(pkg), None, 10) == -1
    assert lib.fasn_kvcache_window_plan(ka._args_decode(pkg), _win(pkg), buf, 8) == -1
    assert lib.fasn_kvprefill_window_plan(ka._args_prefill(pkg), _win(pkg), buf, 8) == -1


def _dec_window_nsplit(c, D, W):
    """the documented rule: the base rule with min(capacity tiles, ceil((W + Sq - 1) / 64) + 1) tiles"""
    base, R = c["B"] * c["Hkv"], c["H"] // c["Hkv"] * c["Sq"]
    tiles = min(-(-c["page"] * c["max_pages"] // 64), -(-(W + c["Sq"] - 1) // 64) + 1)
    return max(1, min(-(-(512 if D == 256 else 1024) // base), tiles // max(4, R // 8)))


def _pre_window_nsplit(c, D, W):
    PB = 128 // (c["H"] // c["Hkv"])
    base = c["B"] * c["Hkv"] * -(-c["Sq"] // PB)
    tiles = min(-(-c["page"] * c["max_pages"] // 64), -(-(W + PB - 1) // 64) + 1)
    return base, max(1, min(-(-(512 if D == 256 else 1024) // base), tiles // 16))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", sorted(ka.DECODE_CASES))
def test_decode_plan(pkg, case, D, dtype):
    c = dict(ka.DECODE_CASES[case], D=D)
    lib = pkg._lib.load()
    capacity = c["page"] * c["max_pages"]
    base = pkg._lib.kvcache_plan(ka._args_decode(pkg, dtype=dtype, **c))
    base_ws = lib.fasn_fwd_kvcache_workspace_bytes(ka._args_decode(pkg, dtype=dtype, **c))
    tag = "%s, %d" % (TAGS[dtype], D)
    BK, R = c["B"] * c["Hkv"], c["H"] // c["Hkv"] * c["Sq"]
    # W >= capacity: the base plan under the new kernel name
    for W in (capacity, capacity + 1, 2 ** 31 - 1):
        plan = pkg._lib.kvcache_window_plan(ka._args_decode(pkg, dtype=dtype, **c), _win(pkg, W))
        assert plan == _renamed(base, "fasn_kvcache_fwd_kernel", "fasn_kvcache_fwd_window_kernel") and plan != base
        assert lib.fasn_fwd_kvcache_window_workspace_bytes(ka._args_decode(pkg, dtype=dtype, **c), _win(pkg, W)) == base_ws
    for W in (1, 128, 1000, 3000):
        plan = pkg._lib.kvcache_window_plan(ka._args_decode(pkg, dtype=dtype, **c), _win(pkg, W))
        assert [k[0] for k in plan] == [f"fasn_kvcache_fwd_window_kernel<{tag}>", f"fasn_kvcache_combine_kernel<{tag}>"]
        nsplit = _dec_window_nsplit(c, D, W)
        assert plan[0][1] == BK * nsplit <= base[0][1] and plan[0][2:] == base[0][2:] and plan[1] == base[1]
        ws = lib.fasn_fwd_kvcache_window_workspace_bytes(ka._args_decode(pkg, dtype=dtype, **c), _win(pkg, W))
        assert ws == BK * nsplit * R * (D + 2) * 4 <= base_ws
        if W <= 128 and capacity >= 2048:
            assert nsplit == 1
        # other lengths, another table (other device pointers), an append: the same launches
        other = ka._args_decode(pkg, dtype=dtype, seqlens=DUMMY + 4096, **c)
        other.block_table = DUMMY + 65536
        assert pkg._lib.kvcache_window_plan(other, _win(pkg, W)) == plan
        appended = ka._args_decode(pkg, dtype=dtype, **c)
        appended.seqlen_add = c["Sq"]
        assert pkg._lib.kvcache_window_plan(appended, _win(pkg, W)) == plan
    # and the base plan did not move
    assert [k[0] for k in base] == [f"fasn_kvcache_fwd_kernel<{tag}>", f"fasn_kvcache_combine_kernel<{tag}>"]
    assert pkg._lib.kvcache_plan(ka._args_decode(pkg, dtype=dtype, **c)) == base


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", sorted(ka.PREFILL_CASES))
def test_prefill_plan(pkg, case, D, dtype):
    c = dict(ka.PREFILL_CASES[case], D=D)
    lib = pkg._lib.load()
    capacity = c["page"] * c["max_pages"]
    base = pkg._lib.kvprefill_plan(ka._args_prefill(pkg, dtype=dtype, **c))
    base_ws = lib.fasn_fwd_kvprefill_workspace_bytes(ka._args_prefill(pkg, dtype=dtype, **c))
    tag = "%s, %d" % (TAGS[dtype], D)
    for W in (capacity, capacity + 1, 2 ** 31 - 1):
        plan = pkg._lib.kvprefill_window_plan(ka._args_prefill(pkg, dtype=dtype, **c), _win(pkg, W))
        assert plan == _renamed(base, "fasn_kvprefill_fwd_kernel", "fasn_kvprefill_fwd_window_kernel") and plan != base
        assert lib.fasn_fwd_kvprefill_window_workspace_bytes(ka._args_prefill(pkg, dtype=dtype, **c), _win(pkg, W)) == base_ws
    for W in (1, 128, 1000, 3000):
        plan = pkg._lib.kvprefill_window_plan(ka._args_prefill(pkg, dtype=dtype, **c), _win(pkg, W))
        blocks, nsplit = _pre_window_nsplit(c, D, W)
        want = [f"fasn_kvprefill_fwd_window_kernel<{tag}>"] + ([f"fasn_kvprefill_combine_kernel<{tag}>"] if nsplit > 1 else [])
        assert [k[0] for k in plan] == want                                               # one split: one launch
        assert plan[0][1] == blocks * nsplit <= base[0][1] and plan[0][2:] == base[0][2:]
        ws = lib.fasn_fwd_kvprefill_window_workspace_bytes(ka._args_prefill(pkg, dtype=dtype, **c), _win(pkg, W))
        assert ws == (blocks * nsplit * 128 * (D + 2) * 4 if nsplit > 1 else 0) <= base_ws
        if W <= 128 and capacity >= 2048:
            assert nsplit == 1 and ws == 0 and len(plan) == 1
        other = ka._args_prefill(pkg, dtype=dtype, seqlens=DUMMY + 4096, q_seqlens=DUMMY + 8192, **c)
        other.kv.block_table = DUMMY + 65536
        assert pkg._lib.kvprefill_window_plan(other, _win(pkg, W)) == plan
        appended = ka._args_prefill(pkg, dtype=dtype, **c)
        appended.kv.seqlen_add = c["Sq"]
        assert pkg._lib.kvprefill_window_plan(appended, _win(pkg, W)) == plan
    assert base[0][0] == f"fasn_kvprefill_fwd_kernel<{tag}>"
    assert pkg._lib.kvprefill_plan(ka._args_prefill(pkg, dtype=dtype, **c)) == base


def test_a_window_of_128_on_an_8192_key_cache_is_one_split(pkg):
    c = dict(B=64, H=64, Hkv=8, Sq=1, D=64, page=256, max_pages=32)
    assert c["page"] * c["max_pages"] == 8192
    assert pkg._lib.kvcache_window_plan(ka._args_decode(pkg, **c), _win(pkg, 128))[0][1] == 64 * 8
    c["B"] = 1
    assert pkg._lib.kvcache_plan(ka._args_decode(pkg, **c))[0][1] == 8 * 32                     # the base plan: 32 splits of 4 tiles
    assert pkg._lib.kvcache_window_plan(ka._args_decode(pkg, **c), _win(pkg, 128))[0][1] == 8
    assert pkg._lib.kvcache_window_plan(ka._args_decode(pkg, **c), _win(pkg, 3000))[0][1] == 8 * 12   # 48 tiles, 4 per split


def _plan_text(pkg):
    lib = pkg._lib.load()
    got = []
    for W in GOLDEN_WINDOWS:
        for D in DIMS:
            for dtype in (0, 1):
                for name in sorted(ka.DECODE_CASES):
                    buf = ctypes.create_string_buffer(4096)
                    rc = lib.fasn_kvcache_window_plan(ka._args_decode(pkg, dtype=dtype, **dict(ka.DECODE_CASES[name], D=D)), _win(pkg, W), buf, len(buf))
                    assert rc > 0, (name, D, dtype, W, rc)
                    got += [f"W={W} decode {name} {line}" for line in buf.value.decode().splitlines()]
                for name in sorted(ka.PREFILL_CASES):
                    buf = ctypes.create_string_buffer(4096)
                    rc = lib.fasn_kvprefill_window_plan(ka._args_prefill(pkg, dtype=dtype, **dict(ka.PREFILL_CASES[name], D=D)), _win(pkg, W), buf, len(buf))
                    assert rc > 0, (name, D, dtype, W, rc)
                    got += [f"W={W} prefill {name} {line}" for line in buf.value.decode().splitlines()]
    return got


def test_plans_equal_the_golden_file(pkg, golden_dir):
    want = open(os.path.join(golden_dir, "kvwindow_plans.txt")).read().splitlines()
    assert _plan_text(pkg) == want


def test_new_kernels_do_not_spill(pkg):
    """2 calls x 2 dtypes x 4 head dims = 16 forward kernels: spill 0, scratch 0"""
    import spill_map
    lib = os.path.join(ROOT, "flash-attention-softmax-n_amd", "libfasn.so")
    if not os.path.exists(spill_map.READELF):
        pytest.skip("llvm-readelf not available")
    if not os.path.exists(lib):
        pytest.skip("libfasn.so not built (run __graft_entry__.build() or make -C flash-attention-softmax-n_amd/csrc)")
    table = spill_map.kernel_table(lib)
    names = sorted(table)
    pretty = subprocess.run([spill_map.CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_pretty = dict(zip(pretty, names))
    wanted = set()
    for D in DIMS:
        for dtype in (0, 1):
            wanted.add(pkg._lib.kvcache_window_plan(ka._args_decode(pkg, dtype=dtype, **dict(ka.DECODE_CASES["gqa"], D=D)), _win(pkg))[0][0])
            wanted.add(pkg._lib.kvprefill_window_plan(ka._args_prefill(pkg, dtype=dtype, **dict(ka.PREFILL_CASES["gqa_prompts"], D=D)), _win(pkg))[0][0])
    assert len(wanted) == 16 and all("_fwd_window_kernel<" in n for n in wanted), wanted
    for name in sorted(wanted):
        hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
        assert len(hit) == 1, (name, hit)
        v = table[hit[0]]
        assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)


def test_no_new_spill_allowance(golden_dir):
    import json
    allowance = json.load(open(os.path.join(golden_dir, "spill_allowance.json")))
    assert not [k for k in map(str, allowance if isinstance(allowance, (list, dict)) else []) if "kvcache" in k or "kvprefill" in k]


# ---------------------------------------------------------------- front end on CPU tensors
def test_front_end_refuses_with_the_reason(pkg):
    """The window checks need no device and come before the CPU-tensor refusal; a valid call gets as far as that refusal on both branches."""
    fa = pkg.flash_attention_n_kvcache_window
    B, H, Hkv = 2, 8, 2
    kc = torch.zeros(4, 64, Hkv, 64, dtype=torch.float16)
    sl = torch.zeros(B, dtype=torch.int32)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    q1 = torch.zeros(B, H, 1, 64, dtype=torch.float16)      # 4 rows: the decode kernels
    q40 = torch.zeros(B, H, 40, 64, dtype=torch.float16)    # 160 rows: the prefill kernels
    for q in (q1, q40):
        for bad in (True, 4.0, "4", None, torch.tensor(4), torch.tensor([4], dtype=torch.int32)):
            with pytest.raises(TypeError, match="window must be a Python int"):
                fa(q, kc, kc, sl, bad, block_table=bt)
        for bad in (0, -1):
            with pytest.raises(ValueError, match="window must be >= 1"):
                fa(q, kc, kc, sl, bad, block_table=bt)
        for ok in (1, 128, 10 ** 12):
            with pytest.raises(RuntimeError, match="CPU tensor"):
                fa(q, kc, kc, sl, ok, block_table=bt)
            with pytest.raises(RuntimeError, match="CPU tensor"):
                fa(q, kc, kc, sl, ok, block_table=bt, query_seqlens=sl)                   # (query lengths: the prefill kernels at any Sq)
            kn = torch.zeros(B, Hkv, q.shape[2], 64, dtype=torch.float16)
            with pytest.raises(RuntimeError, match="CPU tensor"):
                fa(q, kc, kc, sl, ok, block_table=bt, k_new=kn, v_new=kn)
        with pytest.raises(RuntimeError, match="CPU tensor"):
            fa(q, torch.zeros(B, 100, Hkv, 64, dtype=torch.float16), torch.zeros(B, 100, Hkv, 64, dtype=torch.float16), sl, 7)   # dense
        # the refusals of the other cache calls hold, and the window's own come first
        with pytest.raises(ValueError, match="int32"):
            fa(q, kc, kc, sl.long(), 4, block_table=bt)
        with pytest.raises(TypeError, match="window must be a Python int"):
            fa(q, kc, kc, sl.long(), 4.5, block_table=bt)
        with pytest.raises(ValueError, match="query_seqlens must be a contiguous int32 tensor of shape \\[2\\]"):
            fa(q, kc, kc, sl, 4, block_table=bt, query_seqlens=sl.long())
        with pytest.raises(RuntimeError, match="forward only"):
            fa(q.clone().requires_grad_(), kc, kc, sl, 4, block_table=bt)
    with pytest.raises(ValueError, match="flash_attention_n_kvcache_window: 256 query heads per K/V head are not supported"):
        k1 = torch.zeros(4, 64, 1, 64, dtype=torch.float16)
        fa(torch.zeros(B, 256, 1, 64, dtype=torch.float16), k1, k1, sl, 4, block_table=bt)
    with pytest.raises(ValueError, match="head dim 96"):
        k96 = torch.zeros(4, 64, 2, 96, dtype=torch.float16)
        fa(torch.zeros(B, H, 1, 96, dtype=torch.float16), k96, k96, sl, 4, block_table=bt)


def test_signature_and_exports(pkg):
    import flash_attention_softmax_n_amd as shim
    assert "flash_attention_n_kvcache_window" in pkg.__all__ and shim.flash_attention_n_kvcache_window is pkg.kvcache.flash_attention_n_kvcache_window
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_window).parameters) == [
        "query", "k_cache", "v_cache", "cache_seqlens", "window", "block_table", "k_new", "v_new", "query_seqlens", "softmax_n_param", "scale",
        "return_lse"]
    # the two existing calls kept theirs
    assert list(inspect.signature(pkg.flash_attention_n_kvcache).parameters)[-1] == "alibi_slopes"
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_prefill).parameters)[-1] == "alibi_slopes"
    assert "window" not in inspect.signature(pkg.flash_attention_n_kvcache).parameters
