"""K/V-cache PREFILL entry points without a GPU: validation codes of the C ABI (fake, aligned pointers: validation comes before any HIP
call), workspace sizes, the recorded launch plans and their independence from the lengths, the register tables of the new kernels, the
front end's argument errors, and the decode plans, which the prefill kernels must not have moved."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kv_args import DECODE_CASES, DUMMY, PREFILL_CASES as CASES, PREFILL_SPLIT as SPLIT, _args_decode, _args_prefill as _args   # noqa: E402


def test_args_struct_extends_the_cache_struct(pkg):
    L = pkg._lib
    assert L.KvPrefillArgs.kv.offset == 0 and L.KvPrefillArgs.kv.size == ctypes.sizeof(L.KvCacheArgs)
    assert L.KvPrefillArgs.q_seqlens.offset == ctypes.sizeof(L.KvCacheArgs)
    assert L.load().fasn_abi_version() == 6


def test_validation_codes(pkg):
    lib = pkg._lib.load()
    big = ctypes.c_size_t(-1).value

    def fwd(a):
        return lib.fasn_fwd_kvprefill(a, DUMMY, big, None)

    nv = pkg._lib.View4()
    nv.ptr = DUMMY
    for i, s in enumerate((8 * 64, 64, 64, 1)):
        nv.stride[i] = s

    def app(a):
        return lib.fasn_kvprefill_append(a, nv, nv, None)

    buf = ctypes.create_string_buffer(4096)

    def plan(a):
        rc = lib.fasn_kvprefill_plan(a, buf, len(buf))
        return rc if rc < 0 else 0

    for call in (fwd, app, plan):
        assert call(None) == -1
        assert call(_args(pkg, B=0)) == -1
        assert call(_args(pkg, dtype=2)) == -2 and call(_args(pkg, dtype=3)) == -2        # fp32 caches: not built
        assert call(_args(pkg, D=96)) == -3
        assert call(_args(pkg, page=48)) == -7
        a = _args(pkg)
        a.kv.kv_group = 7                                                                 # H % kv_group != 0
        assert call(a) == -1
        a = _args(pkg)
        a.kv.q.ptr = a.kv.q.ptr + 2
        assert call(a) == -4
        a = _args(pkg)
        a.kv.k_stride[1] = 8 * 64 + 4
        assert call(a) == -4
        a = _args(pkg)
        a.kv.q.stride[3] = 2
        assert call(a) == -5
        assert call(_args(pkg, seqlens=None)) == -1
        assert call(_args(pkg, q_seqlens=DUMMY + 2)) == -4                                # the query lengths are int32 words
        a = _args(pkg, Sq=17)
        a.kv.seqlen_add = 3                                                               # 0 or Sq
        assert call(a) == -1
        a.kv.seqlen_add = 17
        assert plan(a) == 0                                                               # (accepted arguments are only ever recorded here, never launched)
    # no row limit: what the decode call refuses (G * Sq = 136 rows) and a long prompt are accepted, with and without query lengths
    for Sq in (17, 4096):
        for qs in (None, DUMMY + 64):
            a = _args(pkg, H=64, Hkv=8, Sq=Sq, q_seqlens=qs)
            assert lib.fasn_fwd_kvcache(a.kv, DUMMY, big, None) == -7
            assert plan(a) == 0 and lib.fasn_fwd_kvprefill_workspace_bytes(a) >= 0
            nv.stride[0], nv.stride[1] = 8 * Sq * 64, Sq * 64
            assert lib.fasn_kvprefill_append(a, None, nv, None) == -1
    assert plan(_args(pkg, H=256, Hkv=1)) == -7                                           # 256 query heads on one K/V head
    assert plan(_args(pkg, H=128, Hkv=1, Sq=5)) == 0
    assert lib.fasn_fwd_kvprefill_workspace_bytes(None) == 0
    assert lib.fasn_fwd_kvprefill_workspace_bytes(_args(pkg, D=96)) == 0
    assert lib.fasn_kvprefill_plan(_args(pkg), buf, 8) == -1
    # the dense cache: one page per batch element whose size need not be a multiple of 64
    assert plan(_args(pkg, page=200, paged=False, Sq=300)) == 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_workspace_and_plan(pkg, case):
    c = CASES[case]
    lib = pkg._lib.load()
    a = _args(pkg, **c)
    plan = pkg._lib.kvprefill_plan(a)
    ws = lib.fasn_fwd_kvprefill_workspace_bytes(a)
    tag = "fasn::bf16_tag, %d" % c["D"]
    names = [k[0] for k in plan]
    assert all(n.startswith("fasn_kvprefill_") for n in names), names                     # only the new kernels
    assert names[0] == f"fasn_kvprefill_fwd_kernel<{tag}>"
    assert (ws > 0) == SPLIT[case]
    assert (f"fasn_kvprefill_combine_kernel<{tag}>" in names) == (ws > 0) and len(names) == (2 if ws > 0 else 1)
    assert all(k[1] > 0 and k[2] == 256 for k in plan)
    G = c["H"] // c["Hkv"]
    blocks = c["B"] * c["Hkv"] * -(-c["Sq"] // (128 // G))
    assert plan[0][1] % blocks == 0 and (plan[0][1] == blocks) == (ws == 0)               # (batch element, K/V head, row block, split)
    big = ctypes.c_size_t(-1).value
    if ws > 0:   # (one split: a NULL workspace is accepted - every GPU test of the one-split plan passes none)
        assert ws == plan[0][1] * 128 * (c["D"] + 2) * 4
        assert lib.fasn_fwd_kvprefill(a, None, big, None) == -8
        assert lib.fasn_fwd_kvprefill(a, DUMMY, ws - 1, None) == -8
        assert lib.fasn_fwd_kvprefill(a, DUMMY + 4, ws, None) == -4
    # other lengths (other device pointers): the same launches, the same workspace
    other = _args(pkg, seqlens=DUMMY + 4096, q_seqlens=DUMMY + 8192, **c)
    assert pkg._lib.kvprefill_plan(other) == plan and lib.fasn_fwd_kvprefill_workspace_bytes(other) == ws
    appended = _args(pkg, **c)
    appended.kv.seqlen_add = c["Sq"]
    assert pkg._lib.kvprefill_plan(appended) == plan


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
    for dtype, tag in ((0, "fasn::f16_tag"), (1, "fasn::bf16_tag")):
        wanted = [k[0] for k in pkg._lib.kvprefill_plan(_args(pkg, dtype=dtype, **CASES[case]))] + ["fasn_kvprefill_append_kernel<%d>" % CASES[case]["D"]]
        assert tag in wanted[0]
        for name in wanted:
            hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
            assert len(hit) == 1, (name, hit)
            v = table[hit[0]]
            assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)


def test_decode_plans_did_not_move(pkg, golden_dir):
    """The decode plans of kv_args.DECODE_CASES, byte for byte those recorded from the commit before the prefill kernels were added"""
    lib = pkg._lib.load()
    got = []
    for name in sorted(DECODE_CASES):
        buf = ctypes.create_string_buffer(4096)
        rc = lib.fasn_kvcache_plan(_args_decode(pkg, **DECODE_CASES[name]), buf, len(buf))
        assert rc > 0, (name, rc)
        got += [f"{name} {line}" for line in buf.value.decode().splitlines()]
    want = open(os.path.join(golden_dir, "kvcache_plans.txt")).read().splitlines()
    assert got == want


def test_front_end_refuses_with_the_reason(pkg):
    """The argument checks need no device and come first; a call whose arguments are otherwise right is refused for its CPU tensors."""
    fa = pkg.flash_attention_n_kvcache_prefill
    import flash_attention_softmax_n_amd as shim
    assert shim.flash_attention_n_kvcache_prefill is fa and "flash_attention_n_kvcache_prefill" in pkg.__all__
    q = torch.zeros(2, 8, 40, 64, dtype=torch.float16)          # 4 x 40 = 160 rows: the decode call refuses them
    kc = torch.zeros(4, 64, 2, 64, dtype=torch.float16)
    sl = torch.zeros(2, dtype=torch.int32)
    ql = torch.zeros(2, dtype=torch.int32)
    bt = torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="rows exceed"):
        pkg.flash_attention_n_kvcache(q, kc, kc, sl, block_table=bt)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        fa(q, kc, kc, sl, block_table=bt)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        fa(q, kc, kc, sl, block_table=bt, query_seqlens=ql)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        fa(q, torch.zeros(2, 100, 2, 64, dtype=torch.float16), torch.zeros(2, 100, 2, 64, dtype=torch.float16), sl)   # dense
    with pytest.raises(ValueError, match="query_seqlens must be a contiguous int32 tensor of shape \\[2\\]"):
        fa(q, kc, kc, sl, block_table=bt, query_seqlens=ql.long())
    with pytest.raises(ValueError, match="query_seqlens must be a contiguous int32 tensor of shape \\[2\\]"):
        fa(q, kc, kc, sl, block_table=bt, query_seqlens=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="query_seqlens must be a contiguous int32 tensor of shape \\[2\\]"):
        fa(q, kc, kc, sl, block_table=bt, query_seqlens=torch.zeros(2, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="query_seqlens must be a contiguous int32 tensor of shape \\[2\\]"):
        fa(q, kc, kc, sl, block_table=bt, query_seqlens=torch.zeros(4, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="query_seqlens"):
        fa(q, kc, kc, sl, block_table=bt, query_seqlens=[40, 40])
    with pytest.raises(ValueError, match="int32"):
        fa(q, kc, kc, sl.long(), block_table=bt)
    with pytest.raises(ValueError, match="block_table has 3 rows but the batch is 2"):
        fa(q, kc, kc, sl, block_table=torch.zeros(3, 2, dtype=torch.int32))
    k16 = torch.zeros(4, 16, 2, 64, dtype=torch.float16)
    with pytest.raises(ValueError, match="page_size 16"):
        fa(q, k16, k16, sl, block_table=bt)
    with pytest.raises(RuntimeError, match="flash_attention_n_kvcache_prefill is forward only.*flash_attention_n"):
        fa(q.clone().requires_grad_(), kc, kc, sl, block_table=bt)
    with torch.no_grad():   # nothing to differentiate: the same call gets as far as the device check
        with pytest.raises(RuntimeError, match="CPU tensor"):
            fa(q.clone().requires_grad_(), kc, kc, sl, block_table=bt)
    with pytest.raises(ValueError, match="head dim 96"):
        k96 = torch.zeros(4, 64, 2, 96, dtype=torch.float16)
        fa(torch.zeros(2, 8, 40, 96, dtype=torch.float16), k96, k96, sl, block_table=bt)
    with pytest.raises(ValueError, match="fp16 and bf16"):
        fa(q.float(), kc.float(), kc.float(), sl, block_table=bt)
    with pytest.raises(ValueError, match="16-byte aligned"):
        odd = torch.zeros(40000, dtype=torch.float16).as_strided((4, 64, 2, 64), (8068, 126, 63, 1))   # head stride 63 elements
        fa(q, odd, kc, sl, block_table=bt)
    with pytest.raises(ValueError, match="k_new and v_new come together"):
        fa(q, kc, kc, sl, block_table=bt, k_new=torch.zeros(2, 2, 40, 64, dtype=torch.float16))
    with pytest.raises(ValueError, match="k_new must be \\[B, Hkv, Sq, D\\]"):
        kn = torch.zeros(2, 2, 39, 64, dtype=torch.float16)
        fa(q, kc, kc, sl, block_table=bt, k_new=kn, v_new=kn)
    with pytest.raises(ValueError, match="query heads per K/V head"):
        k1 = torch.zeros(4, 64, 1, 64, dtype=torch.float16)
        fa(torch.zeros(2, 256, 3, 64, dtype=torch.float16), k1, k1, sl, block_table=bt)
