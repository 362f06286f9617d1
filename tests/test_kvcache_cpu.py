"""K/V-cache entry points without a GPU: validation codes of the C ABI (fake, aligned pointers: validation comes before any HIP call), the
recorded launch plan and its independence from the lengths, the register tables of the new kernels, the unchanged launch plans of the
BASELINE configs, and the front end's argument errors."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kv_args import DECODE_CASES as CASES, DUMMY, _args_decode as _args   # noqa: E402


def test_validation_codes(pkg):
    lib = pkg._lib.load()
    big = ctypes.c_size_t(-1).value

    def fwd(a):
        return lib.fasn_fwd_kvcache(a, DUMMY, big, None)

    nv = pkg._lib.View4()
    nv.ptr = DUMMY
    for i, s in enumerate((8 * 64, 64, 64, 1)):
        nv.stride[i] = s

    def app(a):
        return lib.fasn_kvcache_append(a, nv, nv, None)

    for call in (fwd, app):
        assert call(None) == -1
        assert call(_args(pkg, B=0)) == -1
        assert call(_args(pkg, dtype=2)) == -2 and call(_args(pkg, dtype=3)) == -2        # fp32 caches: not built
        assert call(_args(pkg, D=96)) == -3
        assert call(_args(pkg, page=48)) == -7
        a = _args(pkg)
        a.kv_group = 7                                                                    # H % kv_group != 0
        assert call(a) == -1
        assert call(_args(pkg, H=64, Hkv=8, Sq=17)) == -7                                 # G * Sq = 136 rows
        a = _args(pkg)
        a.q.ptr = a.q.ptr + 2
        assert call(a) == -4
        a = _args(pkg)
        a.k_stride[1] = 8 * 64 + 4
        assert call(a) == -4
        a = _args(pkg)
        a.q.stride[3] = 2
        assert call(a) == -5
        assert call(_args(pkg, seqlens=None)) == -1
    assert lib.fasn_fwd_kvcache_workspace_bytes(None) == 0
    assert lib.fasn_fwd_kvcache_workspace_bytes(_args(pkg, D=96)) == 0
    assert lib.fasn_kvcache_append(_args(pkg), None, nv, None) == -1
    a = _args(pkg)
    need = lib.fasn_fwd_kvcache_workspace_bytes(a)
    assert need > 0
    assert lib.fasn_fwd_kvcache(a, DUMMY, need - 1, None) == -8
    assert lib.fasn_fwd_kvcache(a, None, need, None) == -8
    assert lib.fasn_fwd_kvcache(a, DUMMY + 4, need, None) == -4
    buf = ctypes.create_string_buffer(4096)
    assert lib.fasn_kvcache_plan(None, buf, len(buf)) == -1 and lib.fasn_kvcache_plan(a, buf, 8) == -1
    assert lib.fasn_kvcache_plan(_args(pkg, D=96), buf, len(buf)) == -3
    # the dense cache: one page per batch element whose size need not be a multiple of 64
    assert lib.fasn_fwd_kvcache_workspace_bytes(_args(pkg, page=200, paged=False)) > 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_depends_on_shapes_and_capacity_only(pkg, case):
    c = CASES[case]
    plan = pkg._lib.kvcache_plan(_args(pkg, **c))
    tag = "fasn::bf16_tag, %d" % c["D"]
    assert [k[0] for k in plan] == [f"fasn_kvcache_fwd_kernel<{tag}>", f"fasn_kvcache_combine_kernel<{tag}>"]
    assert all(k[1] > 0 and k[2] == 256 for k in plan)
    BK = c["B"] * c["Hkv"]
    assert plan[0][1] % BK == 0 and plan[0][1] >= min(1024, BK)        # (batch element, K/V head, split) workgroups: ~1024, or one per item
    other = pkg._lib.kvcache_plan(_args(pkg, seqlens=DUMMY + 4096, **c))   # other lengths (another device pointer): the same launches
    assert other == plan


@pytest.mark.parametrize("case", sorted(CASES))
def test_new_kernels_do_not_spill(pkg, case):
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
    wanted = [k[0] for k in pkg._lib.kvcache_plan(_args(pkg, **CASES[case]))] + ["fasn_kvcache_append_kernel<%d>" % CASES[case]["D"]]
    for name in wanted:
        hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
        assert len(hit) == 1, (name, hit)
        v = table[hit[0]]
        assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)


def test_baseline_launch_plans_did_not_move(pkg, golden_dir):
    """The plan lines of the BASELINE configs, byte for byte those recorded from the commit before the K/V-cache kernels were added"""
    from baseline_plans import CONFIGS, bwd_args
    lib = pkg._lib.load()
    got = []
    for name in sorted(CONFIGS):
        for which, code in (("fwd", pkg._lib.FASN_PLAN_FWD_WS), ("bwd", pkg._lib.FASN_PLAN_BWD)):
            buf = ctypes.create_string_buffer(8192)
            rc = lib.fasn_launch_plan(bwd_args(pkg, name), code, buf, len(buf))
            assert rc > 0, (name, which, rc)
            got += [f"{name} {which} {line}" for line in buf.value.decode().splitlines()]
    want = open(os.path.join(golden_dir, "baseline_launch_plans.txt")).read().splitlines()
    assert got == want


def test_front_end_refuses_with_the_reason(pkg):
    """The argument checks need no device and come first; a call whose arguments are otherwise right is refused for its CPU tensors."""
    fa = pkg.flash_attention_n_kvcache
    q = torch.zeros(2, 8, 1, 64, dtype=torch.float16)
    kc = torch.zeros(4, 64, 2, 64, dtype=torch.float16)
    sl = torch.zeros(2, dtype=torch.int32)
    bt = torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        fa(q, kc, kc, sl, block_table=bt)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        fa(q, torch.zeros(2, 100, 2, 64, dtype=torch.float16), torch.zeros(2, 100, 2, 64, dtype=torch.float16), sl)   # dense
    with pytest.raises(ValueError, match="int32"):
        fa(q, kc, kc, sl.long(), block_table=bt)
    with pytest.raises(ValueError, match="block_table has 3 rows but the batch is 2"):
        fa(q, kc, kc, sl, block_table=torch.zeros(3, 2, dtype=torch.int32))
    k16 = torch.zeros(4, 16, 2, 64, dtype=torch.float16)
    with pytest.raises(ValueError, match="page_size 16"):
        fa(q, k16, k16, sl, block_table=bt)
    with pytest.raises(RuntimeError, match="forward only.*flash_attention_n"):
        fa(q.clone().requires_grad_(), kc, kc, sl, block_table=bt)
    with torch.no_grad():   # nothing to differentiate: the same call gets as far as the device check
        with pytest.raises(RuntimeError, match="CPU tensor"):
            fa(q.clone().requires_grad_(), kc, kc, sl, block_table=bt)
    with pytest.raises(ValueError, match="head dim 96"):
        k96 = torch.zeros(4, 64, 2, 96, dtype=torch.float16)
        fa(torch.zeros(2, 8, 1, 96, dtype=torch.float16), k96, k96, sl, block_table=bt)
    with pytest.raises(ValueError, match="rows exceed"):
        fa(torch.zeros(2, 8, 40, 64, dtype=torch.float16), kc, kc, sl, block_table=bt)
    with pytest.raises(ValueError, match="fp16 and bf16"):
        fa(q.float(), kc.float(), kc.float(), sl, block_table=bt)
    with pytest.raises(ValueError, match="16-byte aligned"):
        odd = torch.zeros(40000, dtype=torch.float16).as_strided((4, 64, 2, 64), (8068, 126, 63, 1))   # head stride 63 elements
        fa(q, odd, kc, sl, block_table=bt)
