"""Head dims 32 and 256 on the K/V-cache decode and prefill calls, without a GPU: the plan entry points accept them (and still refuse every
size outside {32, 64, 128, 256}), the validation codes of the existing tests hold there, the launch plans (kernel names, block, LDS,
independence from length / table / slope pointers, the ALiBi plan as the base plan under the other kernel name, the workspace formula)
equal tests/golden/kvheaddim_plans.txt, the register tables of every new kernel show no spill and no scratch, and the front end gets as
far as the CPU-tensor refusal with unchanged signatures."""
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
NEW_DIMS = (32, 256)
TAGS = {0: "fasn::f16_tag", 1: "fasn::bf16_tag"}
LDS_BYTES = {32: 2 * 3 * 64 * 32 * 2, 256: 2 * 2 * 64 * 256 * 2}   # K and V, three / two buffers of 64 keys

# one fixed set of cases per call (every one at both head dims and both dtypes): the plans of these are the golden file
DEC_CASES = {
    "mha": dict(B=64, H=16, Hkv=16, Sq=1, page=256, max_pages=32),
    "gqa": dict(B=4, H=64, Hkv=8, Sq=1, page=256, max_pages=32),
    "gqa_rows": dict(B=32, H=16, Hkv=8, Sq=64, page=256, max_pages=32),       # 128 rows: 16 tiles per split at the least
    "short": dict(B=3, H=8, Hkv=1, Sq=4, page=64, max_pages=4),               # 4 tiles of capacity: one split
}
PRE_CASES = {
    "prompts": dict(B=4, H=16, Hkv=8, Sq=2048, page=256, max_pages=32),       # row blocks fill the chip: one split, no workspace
    "chunk_long_cache": dict(B=1, H=16, Hkv=2, Sq=64, page=256, max_pages=40),
    "g3": dict(B=2, H=12, Hkv=4, Sq=300, page=64, max_pages=64),
}
PRE_SPLIT = {"prompts": False, "chunk_long_cache": True, "g3": True}


def _dec_nsplit(c, D):
    """the documented decode rule: ~1024 workgroups (512 at D = 256), at least max(4, R / 8) tiles of a full cache per split"""
    base, R = c["B"] * c["Hkv"], c["H"] // c["Hkv"] * c["Sq"]
    target = 512 if D == 256 else 1024
    cap_tiles = -(-c["page"] * c["max_pages"] // 64)
    return max(1, min(-(-target // base), cap_tiles // max(4, R // 8)))


def _pre_nsplit(c, D):
    """the documented prefill rule: base = B * Hkv * row blocks, at least 16 tiles of a full cache per split"""
    PB = 128 // (c["H"] // c["Hkv"])
    base = c["B"] * c["Hkv"] * -(-c["Sq"] // PB)
    target = 512 if D == 256 else 1024
    cap_tiles = -(-c["page"] * c["max_pages"] // 64)
    return base, max(1, min(-(-target // base), cap_tiles // 16))


# ---------------------------------------------------------------- plan entry points and validation codes
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("D", NEW_DIMS)
def test_plan_entry_points_accept_the_new_head_dims(pkg, D, dtype):
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    s = ka._slopes(pkg)
    assert lib.fasn_kvcache_plan(ka._args_decode(pkg, D=D, dtype=dtype), buf, len(buf)) > 0
    assert lib.fasn_kvcache_alibi_plan(ka._args_decode(pkg, D=D, dtype=dtype), s, buf, len(buf)) > 0
    assert lib.fasn_kvprefill_plan(ka._args_prefill(pkg, D=D, dtype=dtype, Sq=300), buf, len(buf)) > 0
    assert lib.fasn_kvprefill_alibi_plan(ka._args_prefill(pkg, D=D, dtype=dtype, Sq=300), s, buf, len(buf)) > 0
    assert lib.fasn_fwd_kvcache_workspace_bytes(ka._args_decode(pkg, D=D, dtype=dtype)) > 0
    assert lib.fasn_abi_version() == 6


@pytest.mark.parametrize("D", [96, 48, 512, 16, 192])
def test_other_head_dims_are_still_refused(pkg, D):
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    s = ka._slopes(pkg)
    big = ctypes.c_size_t(-1).value
    nv = pkg._lib.View4()
    nv.ptr = DUMMY
    for i, st in enumerate((8 * D, D, D, 1)):
        nv.stride[i] = st
    assert lib.fasn_kvcache_plan(ka._args_decode(pkg, D=D), buf, len(buf)) == -3
    assert lib.fasn_kvcache_alibi_plan(ka._args_decode(pkg, D=D), s, buf, len(buf)) == -3
    assert lib.fasn_kvprefill_plan(ka._args_prefill(pkg, D=D), buf, len(buf)) == -3
    assert lib.fasn_kvprefill_alibi_plan(ka._args_prefill(pkg, D=D), s, buf, len(buf)) == -3
    assert lib.fasn_fwd_kvcache(ka._args_decode(pkg, D=D), DUMMY, big, None) == -3
    assert lib.fasn_fwd_kvprefill(ka._args_prefill(pkg, D=D), DUMMY, big, None) == -3
    assert lib.fasn_kvcache_append(ka._args_decode(pkg, D=D), nv, nv, None) == -3
    assert lib.fasn_kvprefill_append(ka._args_prefill(pkg, D=D), nv, nv, None) == -3
    assert lib.fasn_fwd_kvcache_workspace_bytes(ka._args_decode(pkg, D=D)) == 0
    assert lib.fasn_fwd_kvprefill_workspace_bytes(ka._args_prefill(pkg, D=D)) == 0


@pytest.mark.parametrize("D", NEW_DIMS)
def test_validation_codes_hold_at_the_new_head_dims(pkg, D):
    """the codes of test_kvcache_cpu / test_kvprefill_cpu / test_kvalibi_cpu::test_validation_codes, with D = 32 / 256 arguments (plan entry
    points and the append, whose validation comes before any HIP call; an accepted forward is only ever recorded, never launched)"""
    lib = pkg._lib.load()
    big = ctypes.c_size_t(-1).value
    buf = ctypes.create_string_buffer(4096)
    good = ka._slopes(pkg)
    nv = pkg._lib.View4()
    nv.ptr = DUMMY
    for i, st in enumerate((8 * D, D, D, 1)):
        nv.stride[i] = st

    def neg(rc):
        return rc if rc < 0 else 0

    calls = {
        "dec": [lambda a: neg(lib.fasn_kvcache_plan(a, buf, len(buf))), lambda a: neg(lib.fasn_kvcache_alibi_plan(a, good, buf, len(buf)))],
        "pre": [lambda a: neg(lib.fasn_kvprefill_plan(a, buf, len(buf))), lambda a: neg(lib.fasn_kvprefill_alibi_plan(a, good, buf, len(buf)))],
    }
    for which, make, kv in (("dec", ka._args_decode, lambda a: a), ("pre", ka._args_prefill, lambda a: a.kv)):
        for call in calls[which]:
            assert call(make(pkg, D=D)) == 0
            assert call(make(pkg, D=D, B=0)) == -1
            assert call(make(pkg, D=D, dtype=2)) == -2 and call(make(pkg, D=D, dtype=3)) == -2
            assert call(make(pkg, D=D, page=48)) == -7
            assert call(make(pkg, D=D, page=200, paged=False)) == 0                       # dense: any capacity
            a = make(pkg, D=D)
            kv(a).kv_group = 7
            assert call(a) == -1
            a = make(pkg, D=D)
            kv(a).q.ptr = kv(a).q.ptr + 2
            assert call(a) == -4
            a = make(pkg, D=D)
            kv(a).k_stride[1] = 8 * D + 4
            assert call(a) == -4
            a = make(pkg, D=D)
            kv(a).k_stride[1] = D - 8                                                     # rows overlap
            assert call(a) == -1
            a = make(pkg, D=D)
            kv(a).q.stride[3] = 2
            assert call(a) == -5
            assert call(make(pkg, D=D, seqlens=None)) == -1
            assert call(make(pkg, D=D, H=64, Hkv=8, Sq=17)) == (-7 if which == "dec" else 0)   # the decode row limit: G * Sq = 136 rows
            assert call(make(pkg, D=D, H=64, Hkv=8, Sq=16)) == 0                          # 128 rows
    assert lib.fasn_kvprefill_plan(ka._args_prefill(pkg, D=D, H=256, Hkv=1), buf, len(buf)) == -7
    assert lib.fasn_kvprefill_plan(ka._args_prefill(pkg, D=D, q_seqlens=DUMMY + 2), buf, len(buf)) == -4
    # the operand of the *_alibi entry points
    assert lib.fasn_kvcache_alibi_plan(ka._args_decode(pkg, D=D), None, buf, len(buf)) == -1
    assert lib.fasn_kvprefill_alibi_plan(ka._args_prefill(pkg, D=D), ka._slopes(pkg, ptr=DUMMY + 2), buf, len(buf)) == -4
    # append: the same argument rules, then the views
    assert lib.fasn_kvcache_append(ka._args_decode(pkg, D=D, page=48), nv, nv, None) == -7
    assert lib.fasn_kvcache_append(ka._args_decode(pkg, D=D), None, nv, None) == -1
    assert lib.fasn_kvprefill_append(ka._args_prefill(pkg, D=D, page=48), nv, nv, None) == -7
    assert lib.fasn_kvprefill_append(ka._args_prefill(pkg, D=D), nv, None, None) == -1
    # workspace too small, missing, unaligned: decode, and the several-split prefill plan
    a = ka._args_decode(pkg, D=D)
    need = lib.fasn_fwd_kvcache_workspace_bytes(a)
    assert need > 0
    for fwd in (lambda w, n: lib.fasn_fwd_kvcache(a, w, n, None), lambda w, n: lib.fasn_fwd_kvcache_alibi(a, good, w, n, None)):
        assert fwd(DUMMY, need - 1) == -8 and fwd(None, need) == -8 and fwd(DUMMY + 4, need) == -4
    pa = ka._args_prefill(pkg, D=D, **PRE_CASES["chunk_long_cache"])
    need = lib.fasn_fwd_kvprefill_workspace_bytes(pa)
    assert need > 0
    for fwd in (lambda w, n: lib.fasn_fwd_kvprefill(pa, w, n, None), lambda w, n: lib.fasn_fwd_kvprefill_alibi(pa, good, w, n, None)):
        assert fwd(DUMMY, need - 1) == -8 and fwd(None, big) == -8 and fwd(DUMMY + 4, need) == -4


# ---------------------------------------------------------------- plan contents
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", sorted(DEC_CASES))
@pytest.mark.parametrize("D", NEW_DIMS)
def test_decode_plan(pkg, D, case, dtype):
    c = dict(DEC_CASES[case], D=D)
    lib = pkg._lib.load()
    plan = pkg._lib.kvcache_plan(ka._args_decode(pkg, dtype=dtype, **c))
    tag = "%s, %d" % (TAGS[dtype], D)
    assert [k[0] for k in plan] == [f"fasn_kvcache_fwd_kernel<{tag}>", f"fasn_kvcache_combine_kernel<{tag}>"]
    assert all(k[1] > 0 and k[2] == 256 for k in plan)
    assert plan[0][3] == LDS_BYTES[D] <= 163840 and plan[1][3] == 0
    BK, R = c["B"] * c["Hkv"], c["H"] // c["Hkv"] * c["Sq"]
    nsplit = _dec_nsplit(c, D)
    assert plan[0][1] == BK * nsplit
    assert plan[1][1] == -(-BK * R * (D // 4) // 256)
    assert lib.fasn_fwd_kvcache_workspace_bytes(ka._args_decode(pkg, dtype=dtype, **c)) == BK * nsplit * R * (D + 2) * 4
    # other lengths, another table, other slopes (other device pointers): the same launches
    other = ka._args_decode(pkg, dtype=dtype, seqlens=DUMMY + 4096, **c)
    other.block_table = DUMMY + 65536
    assert pkg._lib.kvcache_plan(other) == plan
    appended = ka._args_decode(pkg, dtype=dtype, **c)
    appended.seqlen_add = c["Sq"]
    assert pkg._lib.kvcache_plan(appended) == plan
    al = pkg._lib.kvcache_plan(ka._args_decode(pkg, dtype=dtype, **c), ka._slopes(pkg))
    assert al == ka._renamed(plan, "fasn_kvcache_fwd_kernel", "fasn_kvcache_fwd_alibi_kernel") and al != plan
    assert pkg._lib.kvcache_plan(other, ka._slopes(pkg, ptr=DUMMY + 8192, sb=c["H"], sh=1)) == al


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", sorted(PRE_CASES))
@pytest.mark.parametrize("D", NEW_DIMS)
def test_prefill_plan(pkg, D, case, dtype):
    c = dict(PRE_CASES[case], D=D)
    lib = pkg._lib.load()
    plan = pkg._lib.kvprefill_plan(ka._args_prefill(pkg, dtype=dtype, **c))
    tag = "%s, %d" % (TAGS[dtype], D)
    base, nsplit = _pre_nsplit(c, D)
    assert (nsplit > 1) == PRE_SPLIT[case]
    want = [f"fasn_kvprefill_fwd_kernel<{tag}>"] + ([f"fasn_kvprefill_combine_kernel<{tag}>"] if nsplit > 1 else [])
    assert [k[0] for k in plan] == want
    assert all(k[1] > 0 and k[2] == 256 for k in plan)
    assert plan[0][3] == LDS_BYTES[D] <= 163840 and plan[0][1] == base * nsplit
    ws = lib.fasn_fwd_kvprefill_workspace_bytes(ka._args_prefill(pkg, dtype=dtype, **c))
    assert ws == (base * nsplit * 128 * (D + 2) * 4 if nsplit > 1 else 0)
    if nsplit > 1:
        assert plan[1][3] == 0 and plan[1][1] == -(-base * 128 * (D // 4) // 256)
    else:   # one split: a NULL workspace is accepted by the recording call
        buf = ctypes.create_string_buffer(4096)
        assert lib.fasn_kvprefill_plan(ka._args_prefill(pkg, dtype=dtype, **c), buf, len(buf)) > 0
    other = ka._args_prefill(pkg, dtype=dtype, seqlens=DUMMY + 4096, q_seqlens=DUMMY + 8192, **c)
    other.kv.block_table = DUMMY + 65536
    assert pkg._lib.kvprefill_plan(other) == plan and lib.fasn_fwd_kvprefill_workspace_bytes(other) == ws
    appended = ka._args_prefill(pkg, dtype=dtype, **c)
    appended.kv.seqlen_add = c["Sq"]
    assert pkg._lib.kvprefill_plan(appended) == plan
    al = pkg._lib.kvprefill_plan(ka._args_prefill(pkg, dtype=dtype, **c), ka._slopes(pkg))
    assert al == ka._renamed(plan, "fasn_kvprefill_fwd_kernel", "fasn_kvprefill_fwd_alibi_kernel") and al != plan
    assert pkg._lib.kvprefill_plan(other, ka._slopes(pkg, ptr=DUMMY + 16384, sb=c["H"])) == al


def _plan_text(pkg):
    lib = pkg._lib.load()
    got = []
    for D in NEW_DIMS:
        for dtype in (0, 1):
            for name in sorted(DEC_CASES):
                buf = ctypes.create_string_buffer(4096)
                rc = lib.fasn_kvcache_plan(ka._args_decode(pkg, D=D, dtype=dtype, **DEC_CASES[name]), buf, len(buf))
                assert rc > 0, (name, D, dtype, rc)
                got += [f"decode {name} {line}" for line in buf.value.decode().splitlines()]
            for name in sorted(PRE_CASES):
                buf = ctypes.create_string_buffer(4096)
                rc = lib.fasn_kvprefill_plan(ka._args_prefill(pkg, D=D, dtype=dtype, **PRE_CASES[name]), buf, len(buf))
                assert rc > 0, (name, D, dtype, rc)
                got += [f"prefill {name} {line}" for line in buf.value.decode().splitlines()]
    return got


def test_plans_equal_the_golden_file(pkg, golden_dir):
    want = open(os.path.join(golden_dir, "kvheaddim_plans.txt")).read().splitlines()
    assert _plan_text(pkg) == want


def test_plans_of_the_existing_head_dims_did_not_move(pkg, golden_dir):
    """the decode plans recorded before the prefill kernels existed, read again here next to the new ones (D = 64 / 128 keep ~1024
    workgroups), and the prefill cases of test_kvprefill_cpu: the grids its own test derives"""
    lib = pkg._lib.load()
    got = []
    for name in sorted(ka.DECODE_CASES):
        buf = ctypes.create_string_buffer(4096)
        assert lib.fasn_kvcache_plan(ka._args_decode(pkg, **ka.DECODE_CASES[name]), buf, len(buf)) > 0
        got += [f"{name} {line}" for line in buf.value.decode().splitlines()]
    assert got == open(os.path.join(golden_dir, "kvcache_plans.txt")).read().splitlines()
    for name, c in ka.PREFILL_CASES.items():
        base, nsplit = _pre_nsplit(c, c["D"])
        assert pkg._lib.kvprefill_plan(ka._args_prefill(pkg, **c))[0][1] == base * nsplit


# ---------------------------------------------------------------- registers
def test_new_kernels_do_not_spill(pkg):
    """16 forward kernels (2 calls x with / without ALiBi x 2 dtypes x 2 head dims), 8 combine and 4 append kernels: spill 0, scratch 0"""
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
    fwd, side = set(), set()
    for D in NEW_DIMS:
        for dtype in (0, 1):
            for al in (None, ka._slopes(pkg)):
                d = pkg._lib.kvcache_plan(ka._args_decode(pkg, D=D, dtype=dtype, **DEC_CASES["gqa"]), al)
                p = pkg._lib.kvprefill_plan(ka._args_prefill(pkg, D=D, dtype=dtype, **PRE_CASES["chunk_long_cache"]), al)
                fwd |= {d[0][0], p[0][0]}
                side |= {d[1][0], p[1][0]}
        side |= {"fasn_kvcache_append_kernel<%d>" % D, "fasn_kvprefill_append_kernel<%d>" % D}
    assert len(fwd) == 16 and len(side) == 12, (sorted(fwd), sorted(side))
    for name in sorted(fwd | side):
        hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
        assert len(hit) == 1, (name, hit)
        v = table[hit[0]]
        assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)


def test_no_new_spill_allowance(golden_dir):
    import json
    allowance = json.load(open(os.path.join(golden_dir, "spill_allowance.json")))
    assert not [k for k in map(str, allowance if isinstance(allowance, (list, dict)) else []) if "kvcache" in k or "kvprefill" in k]


# ---------------------------------------------------------------- front end on CPU tensors
@pytest.mark.parametrize("which", ["decode", "prefill"])
def test_front_end_accepts_the_new_head_dims(pkg, which):
    fa = pkg.flash_attention_n_kvcache if which == "decode" else pkg.flash_attention_n_kvcache_prefill
    Sq = 1 if which == "decode" else 40
    sl = torch.zeros(2, dtype=torch.int32)
    bt = torch.zeros(2, 2, dtype=torch.int32)
    for D in NEW_DIMS:
        for dtype in (torch.float16, torch.bfloat16):
            q = torch.zeros(2, 8, Sq, D, dtype=dtype)
            kc = torch.zeros(4, 64, 2, D, dtype=dtype)
            with pytest.raises(RuntimeError, match="CPU tensor"):
                fa(q, kc, kc, sl, block_table=bt)
            with pytest.raises(RuntimeError, match="CPU tensor"):
                fa(q, kc, kc, sl, block_table=bt, alibi_slopes=torch.ones(8))
            with pytest.raises(RuntimeError, match="CPU tensor"):
                fa(q, torch.zeros(2, 100, 2, D, dtype=dtype), torch.zeros(2, 100, 2, D, dtype=dtype), sl)   # dense
            kn = torch.zeros(2, 2, Sq, D, dtype=dtype)
            with pytest.raises(RuntimeError, match="CPU tensor"):
                fa(q, kc, kc, sl, block_table=bt, k_new=kn, v_new=kn)
    for D in (96, 48, 512):
        k = torch.zeros(4, 64, 2, D, dtype=torch.float16)
        with pytest.raises(ValueError, match=f"head dim {D} is not supported"):
            fa(torch.zeros(2, 8, Sq, D, dtype=torch.float16), k, k, sl, block_table=bt)
    want = ["query", "k_cache", "v_cache", "cache_seqlens", "block_table", "k_new", "v_new"]
    want += (["query_seqlens"] if which == "prefill" else []) + ["softmax_n_param", "scale", "is_causal", "return_lse", "alibi_slopes"]
    assert list(inspect.signature(fa).parameters) == want
    assert pkg.kvcache._KV_HEAD_DIMS == (32, 64, 128, 256)
