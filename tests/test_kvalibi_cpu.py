"""ALiBi slopes on the K/V-cache decode and prefill calls, without a GPU: validation codes of the four *_alibi entry points (fake, aligned
pointers: validation comes before any HIP call), their launch plans - the non-ALiBi plans under other kernel names, independent of the
length and slope pointers - the register tables of the new kernels, the front end's argument errors, the exports."""
import ctypes
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
NEW = ("fasn_fwd_kvcache_alibi", "fasn_fwd_kvprefill_alibi", "fasn_kvcache_alibi_plan", "fasn_kvprefill_alibi_plan")
_slopes, _renamed = ka._slopes, ka._renamed


def test_symbols_are_exported_and_bound(pkg):
    import flash_attention_softmax_n_amd as shim
    lib = shim._lib.load()
    for name in NEW:
        assert name in shim._lib.EXPORTS and hasattr(lib, name)
    assert lib.fasn_abi_version() == 6
    assert ctypes.sizeof(pkg._lib.AlibiSlopes) == 24 and pkg._lib.AlibiSlopes.stride_h.offset == 16
    # the argument blocks kept their layouts: the operand travels beside them
    assert pkg._lib.KvPrefillArgs.q_seqlens.offset == ctypes.sizeof(pkg._lib.KvCacheArgs)


def test_validation_codes(pkg):
    lib = pkg._lib.load()
    big = ctypes.c_size_t(-1).value
    buf = ctypes.create_string_buffer(4096)

    def run(which, plan):
        fn = getattr(lib, {("dec", False): "fasn_fwd_kvcache_alibi", ("dec", True): "fasn_kvcache_alibi_plan",
                           ("pre", False): "fasn_fwd_kvprefill_alibi", ("pre", True): "fasn_kvprefill_alibi_plan"}[which, plan])

        def call(a, s):
            if plan:
                rc = fn(a, s, buf, len(buf))
                return rc if rc < 0 else 0
            return fn(a, s, DUMMY, big, None)
        return call

    for which, make, kv in (("dec", ka._args_decode, lambda a: a), ("pre", ka._args_prefill, lambda a: a.kv)):
        for plan in (False, True):
            call = run(which, plan)
            good = _slopes(pkg)
            # the operand
            assert call(make(pkg), None) == -1
            assert call(make(pkg), _slopes(pkg, ptr=None)) == -1
            assert call(make(pkg), _slopes(pkg, ptr=DUMMY + 2)) == -4                     # the slopes are fp32 words
            assert call(make(pkg), _slopes(pkg, sh=-1)) == -1
            assert call(make(pkg), _slopes(pkg, sb=1 << 31, sh=1)) == -1                  # (B-1) stride_b + (H-1) stride_h < 2^31
            if plan:   # (accepted arguments are only ever recorded, never launched)
                assert call(make(pkg), _slopes(pkg, sb=64, sh=1)) == 0 and call(make(pkg), _slopes(pkg, sb=0, sh=0)) == 0
            # everything else: the base call's rules and codes
            assert call(None, good) == -1
            assert call(make(pkg, B=0), good) == -1
            assert call(make(pkg, dtype=2), good) == -2
            assert call(make(pkg, D=96), good) == -3
            assert call(make(pkg, page=48), good) == -7
            a = make(pkg)
            kv(a).kv_group = 7
            assert call(a, good) == -1
            a = make(pkg)
            kv(a).q.ptr = kv(a).q.ptr + 2
            assert call(a, good) == -4
            a = make(pkg)
            kv(a).k_stride[1] = 8 * 64 + 4
            assert call(a, good) == -4
            a = make(pkg)
            kv(a).q.stride[3] = 2
            assert call(a, good) == -5
            assert call(make(pkg, seqlens=None), good) == -1
            assert call(make(pkg, D=96), None) == -3                                      # the base arguments are checked first
        assert run(which, True)(make(pkg, H=64, Hkv=8, Sq=17), _slopes(pkg)) == (-7 if which == "dec" else 0)   # the decode row limit
    assert lib.fasn_fwd_kvprefill_alibi(ka._args_prefill(pkg, q_seqlens=DUMMY + 2), _slopes(pkg), DUMMY, big, None) == -4
    a = ka._args_prefill(pkg, Sq=17)
    a.kv.seqlen_add = 3
    assert lib.fasn_fwd_kvprefill_alibi(a, _slopes(pkg), DUMMY, big, None) == -1
    # the workspace is the base call's
    a = ka._args_decode(pkg)
    need = lib.fasn_fwd_kvcache_workspace_bytes(a)
    assert need > 0
    assert lib.fasn_fwd_kvcache_alibi(a, _slopes(pkg), DUMMY, need - 1, None) == -8
    assert lib.fasn_fwd_kvcache_alibi(a, _slopes(pkg), None, need, None) == -8
    assert lib.fasn_fwd_kvcache_alibi(a, _slopes(pkg), DUMMY + 4, need, None) == -4
    a = ka._args_prefill(pkg, **ka.PREFILL_CASES["gqa_chunk_long_cache"])
    need = lib.fasn_fwd_kvprefill_workspace_bytes(a)
    assert need > 0
    assert lib.fasn_fwd_kvprefill_alibi(a, _slopes(pkg), DUMMY, need - 1, None) == -8
    assert lib.fasn_fwd_kvprefill_alibi(a, _slopes(pkg), None, need, None) == -8
    assert lib.fasn_fwd_kvprefill_alibi(a, _slopes(pkg), DUMMY + 4, need, None) == -4
    assert lib.fasn_kvcache_alibi_plan(ka._args_decode(pkg), _slopes(pkg), None, 10) == -1
    assert lib.fasn_kvcache_alibi_plan(ka._args_decode(pkg), _slopes(pkg), buf, 8) == -1
    assert lib.fasn_kvprefill_alibi_plan(ka._args_prefill(pkg), _slopes(pkg), buf, 8) == -1


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", sorted(ka.DECODE_CASES))
def test_decode_plan_is_the_base_plan_under_another_name(pkg, case, dtype):
    c = ka.DECODE_CASES[case]
    base = pkg._lib.kvcache_plan(ka._args_decode(pkg, dtype=dtype, **c))
    plan = pkg._lib.kvcache_plan(ka._args_decode(pkg, dtype=dtype, **c), _slopes(pkg))
    tag = "fasn::%s_tag, %d" % ("bf16" if dtype else "f16", c["D"])
    assert [k[0] for k in plan] == [f"fasn_kvcache_fwd_alibi_kernel<{tag}>", f"fasn_kvcache_combine_kernel<{tag}>"]
    assert plan == _renamed(base, "fasn_kvcache_fwd_kernel", "fasn_kvcache_fwd_alibi_kernel")   # grid, block, LDS: equal
    # other lengths, other slopes, other slope strides (other device pointers): the same launches
    other = pkg._lib.kvcache_plan(ka._args_decode(pkg, dtype=dtype, seqlens=DUMMY + 4096, **c), _slopes(pkg, ptr=DUMMY + 8192, sb=c["H"], sh=1))
    assert other == plan
    # and the base plan did not move
    assert [k[0] for k in base] == [f"fasn_kvcache_fwd_kernel<{tag}>", f"fasn_kvcache_combine_kernel<{tag}>"]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", sorted(ka.PREFILL_CASES))
def test_prefill_plan_is_the_base_plan_under_another_name(pkg, case, dtype):
    c = ka.PREFILL_CASES[case]
    lib = pkg._lib.load()
    base = pkg._lib.kvprefill_plan(ka._args_prefill(pkg, dtype=dtype, **c))
    plan = pkg._lib.kvprefill_plan(ka._args_prefill(pkg, dtype=dtype, **c), _slopes(pkg))
    tag = "fasn::%s_tag, %d" % ("bf16" if dtype else "f16", c["D"])
    assert plan[0][0] == f"fasn_kvprefill_fwd_alibi_kernel<{tag}>"
    assert len(plan) == (2 if ka.PREFILL_SPLIT[case] else 1)                                     # one split / several: both plans
    assert plan == _renamed(base, "fasn_kvprefill_fwd_kernel", "fasn_kvprefill_fwd_alibi_kernel")
    assert base[0][0] == f"fasn_kvprefill_fwd_kernel<{tag}>"
    other = pkg._lib.kvprefill_plan(ka._args_prefill(pkg, dtype=dtype, seqlens=DUMMY + 4096, q_seqlens=DUMMY + 8192, **c), _slopes(pkg, ptr=DUMMY + 16384, sb=c["H"]))
    assert other == plan
    appended = ka._args_prefill(pkg, dtype=dtype, **c)
    appended.kv.seqlen_add = c["Sq"]
    assert pkg._lib.kvprefill_plan(appended, _slopes(pkg)) == plan
    # the workspace is the base call's: the size fits exactly
    ws = lib.fasn_fwd_kvprefill_workspace_bytes(ka._args_prefill(pkg, dtype=dtype, **c))
    assert (ws > 0) == ka.PREFILL_SPLIT[case]
    if ws:
        assert ws == plan[0][1] * 128 * (c["D"] + 2) * 4


def test_new_kernels_do_not_spill(pkg):
    """both dtypes, both head dims, the decode plan and both plans of the prefill (one split and several)"""
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
    for dtype in (0, 1):
        for c in ka.DECODE_CASES.values():
            wanted.add(pkg._lib.kvcache_plan(ka._args_decode(pkg, dtype=dtype, **c), _slopes(pkg))[0][0])
        for c in ka.PREFILL_CASES.values():
            wanted.add(pkg._lib.kvprefill_plan(ka._args_prefill(pkg, dtype=dtype, **c), _slopes(pkg))[0][0])
    assert len(wanted) == 8 and all("_alibi_kernel<" in n for n in wanted), wanted         # 2 kernels x 2 dtypes x 2 head dims
    for name in sorted(wanted):
        hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
        assert len(hit) == 1, (name, hit)
        v = table[hit[0]]
        assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)


@pytest.mark.parametrize("which", ["decode", "prefill"])
def test_front_end_refuses_with_the_reason(pkg, which):
    """The slope checks need no device and come before the CPU-tensor refusal; valid CPU slopes get as far as that refusal."""
    B, H, Hkv = 2, 8, 2
    fa = pkg.flash_attention_n_kvcache if which == "decode" else pkg.flash_attention_n_kvcache_prefill
    q = torch.zeros(B, H, 1 if which == "decode" else 40, 64, dtype=torch.float16)
    kc = torch.zeros(4, 64, Hkv, 64, dtype=torch.float16)
    sl = torch.zeros(B, dtype=torch.int32)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    from flash_attention_softmax_n_amd import synth
    slopes = synth.alibi_slopes(H).float()
    assert slopes.shape == (H,)
    with pytest.raises(TypeError, match="alibi_slopes must be a floating-point tensor"):
        fa(q, kc, kc, sl, block_table=bt, alibi_slopes=torch.ones(H, dtype=torch.int32))
    with pytest.raises(TypeError, match="alibi_slopes must be a floating-point tensor"):
        fa(q, kc, kc, sl, block_table=bt, alibi_slopes=[0.5] * H)
    with pytest.raises(ValueError, match="alibi_slopes must broadcast to \\[B, H\\] = \\[2, 8\\]"):
        fa(q, kc, kc, sl, block_table=bt, alibi_slopes=torch.ones(H + 1))
    with pytest.raises(ValueError, match="alibi_slopes must broadcast to \\[B, H\\]"):
        fa(q, kc, kc, sl, block_table=bt, alibi_slopes=torch.ones(1, B, H))
    with pytest.raises(RuntimeError, match="forward only.*alibi_slopes requires grad"):
        fa(q, kc, kc, sl, block_table=bt, alibi_slopes=slopes.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="alibi_slopes is on meta"):
        fa(q, kc, kc, sl, block_table=bt, alibi_slopes=torch.ones(H, device="meta"))
    with torch.no_grad():   # nothing to differentiate: the same call gets as far as the device check
        with pytest.raises(RuntimeError, match="CPU tensor"):
            fa(q, kc, kc, sl, block_table=bt, alibi_slopes=slopes.clone().requires_grad_())
    for ok in (slopes, slopes.view(1, H), slopes.expand(B, H), torch.ones(B, 1), torch.tensor(0.25), slopes.bfloat16(), slopes.double(), torch.ones(2 * H)[::2]):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            fa(q, kc, kc, sl, block_table=bt, alibi_slopes=ok)
    # the other refusals still come first / still hold next to slopes, and None is the call as it was
    with pytest.raises(ValueError, match="int32"):
        fa(q, kc, kc, sl.long(), block_table=bt, alibi_slopes=slopes)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        fa(q, kc, kc, sl, block_table=bt, alibi_slopes=None)
    import inspect
    assert list(inspect.signature(fa).parameters)[-1] == "alibi_slopes"                   # last: positional callers are untouched
