"""Decode behind a shared prefix (fasn_fwd_shared_prefix), without a GPU: the operand's layout, the exports against the header and the
bindings, the validation codes and their order behind the base checks (fake, aligned pointers: validation comes before any HIP call), the
launch plans - equal to tests/golden/kvshared_plans.txt and to the rule restated in tests/kv_prefix.py - the workspace formula, the
register tables of the new kernels and the front end's refusals."""
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
import kv_args as ka     # noqa: E402
import kv_prefix as sp   # noqa: E402

DUMMY, BIG = ka.DUMMY, ka.BIG
NEW = ("fasn_fwd_shared_prefix_workspace_bytes", "fasn_fwd_shared_prefix", "fasn_shared_prefix_plan")
DIMS = (64, 128)
TAGS = {0: "fasn::f16_tag", 1: "fasn::bf16_tag"}
EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED, EWORKSPACE = -1, -2, -3, -4, -5, -7, -8
_prefix = sp._prefix


def test_symbols_are_exported_and_bound(pkg):
    lib = pkg._lib.load()
    for name in NEW:
        assert name in pkg._lib.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert [b[0] for b in pkg._lib._shared_prefix_bindings()] == list(NEW)
    assert lib.fasn_abi_version() == 6 and pkg._lib.FASN_ABI_VERSION == 6
    S = pkg._lib.SharedPrefix
    assert ctypes.sizeof(S) == 24
    assert (S.prefix_len.offset, S.prefix_table.offset, S.max_prefix_pages.offset, S.reserved.offset) == (0, 8, 16, 20)
    # the families the other suites count keep their members: the new names belong to none of them
    assert len(list(pkg._lib._kv_bindings())) == 69 and ctypes.sizeof(pkg._lib.KvCall) == 48
    for name in NEW:
        assert not any(s in name for s in ("kvcache", "kvprefill", "kvvarlen")) and not name.startswith("fasn_kv_")


def test_header_declares_what_is_bound(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fasn.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fasn_[a-z0-9_]+)\s*\(", text))
    assert set(NEW) <= declared and declared == set(pkg._lib.EXPORTS)
    body = re.search(r"typedef struct fasn_shared_prefix \{(.*?)\} fasn_shared_prefix;", text, flags=re.S).group(1)
    names = [n for _t, n in re.findall(r"([a-z0-9_ ]+?[ *]+)([A-Za-z_]+)(?:\[\d+\])?;", body)]
    assert names == [f[0] for f in pkg._lib.SharedPrefix._fields_]
    assert "#define FASN_ABI_VERSION 6" in text


def _calls(lib):
    buf = ctypes.create_string_buffer(4096)

    def plan(a, p):
        rc = lib.fasn_shared_prefix_plan(a, p, buf, len(buf))
        return rc if rc < 0 else 0
    return {"fwd": lambda a, p: lib.fasn_fwd_shared_prefix(a, p, DUMMY, BIG, None), "plan": plan}


def test_validation_codes_and_their_order(pkg):
    lib = pkg._lib.load()
    make = ka._args_decode
    good = _prefix(pkg)
    for how, call in _calls(lib).items():
        # every base code with a good and with a bad operand: the base block's rules come first, with their codes
        for p in (good, None, _prefix(pkg, reserved=1), _prefix(pkg, pages=0), _prefix(pkg, plen=DUMMY + 2)):
            assert call(None, p) == EINVAL
            assert call(make(pkg, B=0), p) == EINVAL
            assert call(make(pkg, dtype=2), p) == EDTYPE
            assert call(make(pkg, D=96), p) == EHEADDIM
            assert call(make(pkg, page=48), p) == EUNSUPPORTED
            a = make(pkg)
            a.q.ptr = a.q.ptr + 2
            assert call(a, p) == EALIGN
            a = make(pkg)
            a.q.stride[3] = 2
            assert call(a, p) == ESTRIDE
            assert call(make(pkg, seqlens=None), p) == EINVAL
            assert call(make(pkg, H=64, Hkv=8, Sq=17), p) == EUNSUPPORTED      # the decode row limit is a base rule
        # then the call's own rules, in the documented order: paged, head dim, the operand, its alignment
        for p in (good, None, _prefix(pkg, plen=DUMMY + 2)):
            assert call(make(pkg, paged=False, page=8192), p) == EUNSUPPORTED
            assert call(make(pkg, D=32), p) == EUNSUPPORTED and call(make(pkg, D=256), p) == EUNSUPPORTED
        assert call(make(pkg), None) == EINVAL
        assert call(make(pkg), _prefix(pkg, plen=None)) == EINVAL and call(make(pkg), _prefix(pkg, table=None)) == EINVAL
        assert call(make(pkg), _prefix(pkg, pages=0)) == EINVAL and call(make(pkg), _prefix(pkg, pages=-3)) == EINVAL
        assert call(make(pkg), _prefix(pkg, reserved=1)) == EINVAL
        assert call(make(pkg), _prefix(pkg, reserved=1, plen=DUMMY + 2)) == EINVAL   # (reserved comes before the alignment)
        assert call(make(pkg), _prefix(pkg, plen=DUMMY + 2)) == EALIGN and call(make(pkg), _prefix(pkg, table=DUMMY + 1)) == EALIGN
        if how == "plan":   # (accepted arguments are only ever recorded, never launched)
            for pages in (1, 8, 32, 33, 2 ** 31 - 1):
                assert call(make(pkg), _prefix(pkg, pages=pages)) == 0
            assert call(make(pkg, D=128, dtype=0, H=8, Hkv=8, Sq=128), good) == 0
    ws = lib.fasn_fwd_shared_prefix_workspace_bytes
    assert ws(None, good) == 0 and ws(make(pkg), None) == 0 and ws(make(pkg, D=32), good) == 0 and ws(make(pkg, paged=False, page=8192), good) == 0
    assert ws(make(pkg), _prefix(pkg, reserved=2)) == 0 and ws(make(pkg), _prefix(pkg, table=DUMMY + 2)) == 0
    # then the workspace: missing, too small, misaligned
    a = make(pkg)
    need = ws(a, good)
    assert need > lib.fasn_fwd_kvcache_workspace_bytes(a) > 0
    assert lib.fasn_fwd_shared_prefix(a, good, DUMMY, need - 1, None) == EWORKSPACE
    assert lib.fasn_fwd_shared_prefix(a, good, None, need, None) == EWORKSPACE
    assert lib.fasn_fwd_shared_prefix(a, good, DUMMY + 4, need, None) == EALIGN
    assert lib.fasn_fwd_shared_prefix(a, None, None, 0, None) == EINVAL          # (the operand before the workspace)
    buf = ctypes.create_string_buffer(4096)
    assert lib.fasn_shared_prefix_plan(a, good, None, 10) == EINVAL and lib.fasn_shared_prefix_plan(a, good, buf, 8) == EINVAL


# ---------------------------------------------------------------- plans
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", sorted(sp.SHARED_PLAN_CASES))
def test_plan_and_workspace_follow_the_rule(pkg, case, D, dtype):
    """three launches; the grids, the LDS and the workspace as include/fasn.h states them, recomputed in Python; the suffix pass has the
    base call's grid"""
    shape, pages = sp.SHARED_PLAN_CASES[case]
    lib = pkg._lib.load()
    tag = "%s, %d" % (TAGS[dtype], D)
    args = lambda **kw: ka._args_decode(pkg, dtype=dtype, D=D, **dict(shape, **kw))   # noqa: E731
    plan = pkg._lib.shared_prefix_plan(args(), _prefix(pkg, pages=pages))
    gp, gs, gc, ws = sp.shared_plan_rule(D=D, prefix_pages=pages, **shape)
    assert plan == [(f"fasn_kvshared_prefix_kernel<{tag}>", gp, 256, sp.lds_bytes(D)), (f"fasn_kvshared_suffix_kernel<{tag}>", gs, 256, sp.lds_bytes(D)),
                    (f"fasn_kvshared_combine_kernel<{tag}>", gc, 256, 0)]
    base = pkg._lib.kvcache_plan(args())
    assert plan[1][1:] == base[0][1:] and plan[2][1:] == base[1][1:]
    assert lib.fasn_fwd_shared_prefix_workspace_bytes(args(), _prefix(pkg, pages=pages)) == ws
    R = (shape["H"] // shape["Hkv"]) * shape["Sq"]
    assert ws == lib.fasn_fwd_kvcache_workspace_bytes(args()) + (gp // -(-shape["B"] * R // 128)) * shape["B"] * R * (D + 2) * 4


def test_grids_do_not_depend_on_device_memory(pkg):
    """other lengths, another block table, another prefix table and length (other device pointers), an append: the same launches"""
    for case, (shape, pages) in sp.SHARED_PLAN_CASES.items():
        a = ka._args_decode(pkg, **shape)
        plan = pkg._lib.shared_prefix_plan(a, _prefix(pkg, pages=pages))
        other = ka._args_decode(pkg, seqlens=DUMMY + 4096, **shape)
        other.block_table = DUMMY + 65536
        other.seqlen_add = shape["Sq"]
        other.causal = 0
        assert pkg._lib.shared_prefix_plan(other, _prefix(pkg, pages=pages, plen=DUMMY + 1024, table=DUMMY + 2048)) == plan, case
        lib = pkg._lib.load()
        assert lib.fasn_fwd_shared_prefix_workspace_bytes(other, _prefix(pkg, pages=pages, plen=DUMMY + 1024)) == lib.fasn_fwd_shared_prefix_workspace_bytes(
            a, _prefix(pkg, pages=pages))


def _plan_text(pkg):
    lib = pkg._lib.load()
    got = []
    for D in DIMS:
        for dtype in (0, 1):
            for name in sorted(sp.SHARED_PLAN_CASES):
                shape, pages = sp.SHARED_PLAN_CASES[name]
                buf = ctypes.create_string_buffer(4096)
                rc = lib.fasn_shared_prefix_plan(ka._args_decode(pkg, dtype=dtype, D=D, **shape), _prefix(pkg, pages=pages), buf, len(buf))
                assert rc > 0, (name, D, dtype, rc)
                got += [f"{name} {line}" for line in buf.value.decode().splitlines()]
    return got


def test_plans_equal_the_golden_file(pkg, golden_dir):
    want = open(os.path.join(golden_dir, "kvshared_plans.txt")).read().splitlines()
    assert _plan_text(pkg) == want


def test_new_kernels_do_not_spill(pkg):
    """3 kernels x 2 dtypes x 2 head dims = 12: each present once, spill 0, scratch 0"""
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
            shape, pages = sp.SHARED_PLAN_CASES["straddle"]
            wanted |= {k[0] for k in pkg._lib.shared_prefix_plan(ka._args_decode(pkg, dtype=dtype, D=D, **shape), _prefix(pkg, pages=pages))}
    assert len(wanted) == 12, wanted
    for name in sorted(wanted):
        hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
        assert len(hit) == 1, (name, hit)
        v = table[hit[0]]
        assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)
    assert sum("kvshared" in d for d in by_pretty) == 12


def test_no_new_spill_allowance(golden_dir):
    import json
    allowance = json.load(open(os.path.join(golden_dir, "spill_allowance.json")))
    assert not [k for k in map(str, allowance if isinstance(allowance, (list, dict)) else []) if "kvshared" in k or "shared_prefix" in k]


# ---------------------------------------------------------------- front end on CPU tensors
def test_front_end_refuses_with_the_reason(pkg):
    fa = pkg.flash_attention_n_kvcache_shared_prefix
    B, H, Hkv = 2, 8, 2
    q = torch.zeros(B, H, 4, 64, dtype=torch.float16)
    kc = torch.zeros(6, 64, Hkv, 64, dtype=torch.float16)
    sl = torch.zeros(B, dtype=torch.int32)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    pt = torch.zeros(2, dtype=torch.int32)
    pl = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="a dense cache .block_table=None. is not supported: a shared prefix is a set of pages"):
        fa(q, kc, kc, sl, None, pt, pl)
    with pytest.raises(TypeError, match="a float8 cache is not supported .fp16 and bf16 caches only"):
        fa(q, kc.to(torch.float8_e4m3fn), kc.to(torch.float8_e4m3fn), sl, bt, pt, pl)
    for D in (32, 256):
        with pytest.raises(ValueError, match=r"head dim %d is not supported behind a shared prefix \(supported: \(64, 128\)" % D):
            fa(torch.zeros(B, H, 4, D, dtype=torch.float16), torch.zeros(6, 64, Hkv, D, dtype=torch.float16), kc, sl, bt, pt, pl)
    with pytest.raises(ValueError, match="head dim 96 is not supported"):
        fa(torch.zeros(B, H, 4, 96, dtype=torch.float16), kc, kc, sl, bt, pt, pl)
    with pytest.raises(ValueError, match=r"4 x 33 = 132 rows exceed the 128 of one pass"):
        fa(torch.zeros(B, H, 33, 64, dtype=torch.float16), kc, kc, sl, bt, pt, pl)
    for bad in (pt.long(), pt.view(1, 2), pt[:0], torch.zeros(4, dtype=torch.int32)[::2], [0, 1], None):
        with pytest.raises(ValueError, match="prefix_table must be a contiguous int32 tensor of shape .max_prefix_pages. on the device"):
            fa(q, kc, kc, sl, bt, bad, pl)
    for bad in (pl.long(), torch.zeros(2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 64, None):
        with pytest.raises(ValueError, match="prefix_len must be an int32 tensor of one element on the device"):
            fa(q, kc, kc, sl, bt, pt, bad)
    with pytest.raises(RuntimeError, match="prefix_table is on meta"):
        fa(q, kc, kc, sl, bt, pt.to("meta"), pl)
    with pytest.raises(RuntimeError, match="prefix_len is on meta"):
        fa(q, kc, kc, sl, bt, pt, pl.to("meta"))
    with pytest.raises(RuntimeError, match="forward only"):
        fa(q.clone().requires_grad_(), kc, kc, sl, bt, pt, pl)
    with pytest.raises(RuntimeError, match="forward only"):
        fa(q, kc, kc, sl, bt, pt, pl, softmax_n_param=torch.ones(H, requires_grad=True))
    # the base call keeps refusing what it refuses
    with pytest.raises(ValueError, match="int32"):
        fa(q, kc, kc, sl.long(), bt, pt, pl)
    with pytest.raises(ValueError, match="k_new and v_new come together"):
        fa(q, kc, kc, sl, bt, pt, pl, k_new=torch.zeros(B, Hkv, 4, 64, dtype=torch.float16))
    # a valid call gets as far as the CPU-tensor refusal: 0-d and [1] lengths, with and without new rows
    kn = torch.zeros(B, Hkv, 4, 64, dtype=torch.float16)
    for plen in (pl, pl.view(()), pl.view(1, 1)):
        for new in ({}, dict(k_new=kn, v_new=kn)):
            with pytest.raises(RuntimeError, match="device tensors only"):
                fa(q, kc, kc, sl, bt, pt, plen, **new)


def test_signature_and_membership(pkg):
    fa = pkg.flash_attention_n_kvcache_shared_prefix
    assert "flash_attention_n_kvcache_shared_prefix" in pkg.__all__ and "flash_attention_n_kvcache_shared_prefix" in pkg.__doc__
    sig = inspect.signature(fa)
    assert list(sig.parameters) == ["query", "k_cache", "v_cache", "cache_seqlens", "block_table", "prefix_table", "prefix_len", "k_new", "v_new",
                                    "softmax_n_param", "scale", "is_causal", "return_lse"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(k_new=None, v_new=None, softmax_n_param=1, scale=None, is_causal=True, return_lse=False)
    assert pkg._lib.shared_prefix_plan.__doc__ and "prefix" in fa.__doc__
