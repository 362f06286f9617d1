"""Token-tree attention over the FP8 K/V cache without a GPU - fasn_fwd_kv*_fp8_tree, fasn_kv*_fp8_tree_rope_append and
fasn_kvcache_fp8_tree_commit: exports within ABI 6, the validation codes of the new entry points in the family's order (base checks, the
FP8 operand, the tree operand, then the rope operand; fake, aligned pointers: validation comes before any HIP call), their launch plans -
the 16-bit tree call's grids, split counts and workspace with the FP8 kernels' LDS, the tree rope append's grid, equal to
tests/golden/kvfp8_tree_plans.txt - the register tables of the fourteen new kernels, and the front end of the two new functions on CPU
tensors."""
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
import kv_fp8_tree as k8t   # noqa: E402
import kv_tree as kt   # noqa: E402

DUMMY, BIG = ka.DUMMY, ka.BIG
FORWARD_SYMBOLS = ("fasn_fwd_kvcache_fp8_tree", "fasn_fwd_kvcache_fp8_tree_workspace_bytes", "fasn_kvcache_fp8_tree_plan",
                   "fasn_fwd_kvprefill_fp8_tree", "fasn_fwd_kvprefill_fp8_tree_workspace_bytes", "fasn_kvprefill_fp8_tree_plan")
ROPE_SYMBOLS = ("fasn_kvcache_fp8_tree_rope_append", "fasn_kvprefill_fp8_tree_rope_append", "fasn_kvcache_fp8_tree_rope_append_plan",
                "fasn_kvprefill_fp8_tree_rope_append_plan")
NEW = FORWARD_SYMBOLS + ROPE_SYMBOLS + ("fasn_kvcache_fp8_tree_commit",)
DIMS = (64, 128)
TAGS = {0: "fasn::f16_tag", 1: "fasn::bf16_tag"}
EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED, EWORKSPACE = -1, -2, -3, -4, -5, -7, -8
_fp8, _tree, _rope, _view, _win = k8._fp8, kt._tree, ka._rope, ka._view, ka._win
ROUTES = (("decode", "kvcache", ka._args_decode, kt.DECODE_CASES), ("prefill", "kvprefill", ka._args_prefill, kt.PREFILL_CASES))
SMEM = {64: 40 * 1024, 128: 64 * 1024}


def _kv(route, a):
    return a if route == "decode" else a.kv


# ---------------------------------------------------------------- exports
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
    # the operands are the structs that were there: nothing about their layouts moved
    assert ctypes.sizeof(pkg._lib.KvFp8) == 56 and ctypes.sizeof(pkg._lib.KvTree) == 24 and ctypes.sizeof(pkg._lib.KvTreeCommit) == 144
    assert not [n for n in exported if "varlen" in n and "fp8" in n]
    assert "no tree variant" not in header.lower()


# ---------------------------------------------------------------- validation
def _forward_calls(pkg, stem):
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    return {
        "plan": lambda a, o, t: min(getattr(lib, f"fasn_{stem}_fp8_tree_plan")(a, o, t, buf, len(buf)), 0),
        "forward": lambda a, o, t: getattr(lib, f"fasn_fwd_{stem}_fp8_tree")(a, o, t, DUMMY, BIG, None),
    }


def test_forward_refusals_and_their_order(pkg):
    """(the launching entry point is only ever refused here: accepted blocks go through the plans)"""
    lib = pkg._lib.load()
    for route, stem, make, _cases in ROUTES:
        shape = dict(Sq=8) if route == "decode" else dict(Sq=40)
        for how, call in _forward_calls(pkg, stem).items():
            def code(edit=None, op=None, tree=None, **kw):
                a = make(pkg, **dict(shape, **kw))
                if edit is not None:
                    edit(_kv(route, a))
                return call(a, _fp8(pkg) if op is None else op, _tree(pkg) if tree is None else tree)

            what = (route, how)
            if how == "plan":
                for w in (0, 1, 128, 8192, 8193, 2 ** 31 - 1):
                    assert code(tree=_tree(pkg, window=w)) == 0, (what, w)
                assert code(H=8, Hkv=8, Sq=64) == 0 and code(D=128) == 0, what
            # NULL operands
            assert call(None, _fp8(pkg), _tree(pkg)) == EINVAL, what
            assert call(make(pkg, **shape), None, _tree(pkg)) == EINVAL and call(make(pkg, **shape), _fp8(pkg), None) == EINVAL, what
            assert code(op=_fp8(pkg, k_scale=None)) == EINVAL and code(op=_fp8(pkg, v_scale=None)) == EINVAL and code(op=_fp8(pkg, reserved=1)) == EINVAL, what
            # the tree operand, with the codes of fasn_fwd_kv*_tree
            assert code(tree=_tree(pkg, mask=None)) == EINVAL and code(tree=_tree(pkg, reserved=1)) == EINVAL, what
            assert code(H=8, Hkv=8, Sq=65) == EUNSUPPORTED, what                                   # one word per node
            assert code(H=8, Hkv=8, Sq=65, tree=_tree(pkg, reserved=1)) == EINVAL, what           # (reserved comes before the node count)
            assert code(lambda a: setattr(a, "causal", 0)) == EUNSUPPORTED, what
            assert code(lambda a: setattr(a, "causal", 0), tree=_tree(pkg, window=-1)) == EUNSUPPORTED, what   # (causal before the window)
            assert code(tree=_tree(pkg, window=-1)) == EINVAL and code(tree=_tree(pkg, stride=-1)) == EINVAL, what
            assert code(tree=_tree(pkg, mask=DUMMY + 4)) == EALIGN, what
            # head dims: 96 is the base check's refusal, 32 / 256 the FP8 operand's
            for D in (32, 96, 256):
                assert code(D=D) == EHEADDIM, (what, D)
            # the FP8 operand: misaligned scales; a byte stride that is a multiple of 8 but not of 16
            assert code(op=_fp8(pkg, k_scale=DUMMY + 2)) == EALIGN and code(op=_fp8(pkg, v_scale=DUMMY + 2)) == EALIGN, what
            for which in ("k_stride", "v_stride"):
                for i in range(3):
                    assert code(lambda a, which=which, i=i: getattr(a, which).__setitem__(i, getattr(a, which)[i] + 8)) == EALIGN, (what, which, i)
            # base rules
            assert code(page=32) == EUNSUPPORTED and code(dtype=2) == EDTYPE and code(B=0) == EINVAL, what
            if route == "decode":
                assert code(H=64, Hkv=8, Sq=17) == EUNSUPPORTED, what                             # the decode row limit is a base rule
            # the order: base, then the FP8 operand, then the tree operand
            assert code(lambda a: setattr(a, "seqlens", None), op=_fp8(pkg, reserved=1), tree=_tree(pkg, mask=None)) == EINVAL, what
            assert code(D=96, op=_fp8(pkg, k_scale=DUMMY + 2), tree=_tree(pkg, mask=None)) == EHEADDIM, what               # base first
            assert code(op=_fp8(pkg, k_scale=DUMMY + 2), tree=_tree(pkg, mask=None)) == EALIGN, what                       # FP8 before the tree
            assert code(op=_fp8(pkg, k_scale=DUMMY + 2), tree=None, H=8, Hkv=8, Sq=65) == EALIGN, what
            assert code(lambda a: setattr(a, "causal", 0), op=_fp8(pkg, k_scale=DUMMY + 2)) == EALIGN, what
            assert code(D=32, tree=_tree(pkg, mask=DUMMY + 4)) == EHEADDIM, what
            assert code(D=256, H=8, Hkv=8, Sq=65 if route == "prefill" else 8, tree=_tree(pkg, reserved=1)) == EHEADDIM, what
        # workspace: 0 for a refused block, the 16-bit tree call's otherwise
        ws = getattr(lib, f"fasn_fwd_{stem}_fp8_tree_workspace_bytes")
        ws16 = getattr(lib, f"fasn_fwd_{stem}_tree_workspace_bytes")
        a = lambda **kw: make(pkg, **dict(shape, **kw))   # noqa: E731
        assert ws(a(), _fp8(pkg), None) == 0 and ws(a(), None, _tree(pkg)) == 0 and ws(a(D=32), _fp8(pkg), _tree(pkg)) == 0
        assert ws(a(), _fp8(pkg), _tree(pkg, reserved=3)) == 0 and ws(a(H=8, Hkv=8, Sq=65), _fp8(pkg), _tree(pkg)) == 0
        for w in (0, 128, 1000):
            assert ws(a(), _fp8(pkg), _tree(pkg, window=w)) == ws16(a(), _tree(pkg, window=w)), (route, w)
    # then the workspace: missing, too small, misaligned
    a = ka._args_decode(pkg, Sq=8)
    need = lib.fasn_fwd_kvcache_fp8_tree_workspace_bytes(a, _fp8(pkg), _tree(pkg))
    assert need == lib.fasn_fwd_kvcache_tree_workspace_bytes(a, _tree(pkg)) > 0
    assert lib.fasn_fwd_kvcache_fp8_tree(a, _fp8(pkg), _tree(pkg), DUMMY, need - 1, None) == EWORKSPACE
    assert lib.fasn_fwd_kvcache_fp8_tree(a, _fp8(pkg), _tree(pkg), None, need, None) == EWORKSPACE
    assert lib.fasn_fwd_kvcache_fp8_tree(a, _fp8(pkg), _tree(pkg), DUMMY + 4, need, None) == EALIGN
    assert lib.fasn_fwd_kvcache_fp8_tree(a, _fp8(pkg), None, None, 0, None) == EINVAL                 # (the operand before the workspace)
    buf = ctypes.create_string_buffer(4096)
    assert lib.fasn_kvcache_fp8_tree_plan(a, _fp8(pkg), _tree(pkg), None, 10) == EINVAL
    assert lib.fasn_kvcache_fp8_tree_plan(a, _fp8(pkg), _tree(pkg), buf, 8) == EINVAL


def test_rope_append_refusals_and_their_order(pkg):
    """the base checks, the FP8 operand's, the tree operand's, then the rope operand's"""
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    for route, stem, make, _cases in ROUTES:
        Sq0 = 8 if route == "decode" else 40
        calls = {
            "plan": lambda a, o, r, t, qo, kn, vn, stem=stem: min(getattr(lib, f"fasn_{stem}_fp8_tree_rope_append_plan")(a, o, r, t, qo, kn, vn, buf, len(buf)), 0),
            "run": lambda a, o, r, t, qo, kn, vn, stem=stem: getattr(lib, f"fasn_{stem}_fp8_tree_rope_append")(a, o, r, t, qo, kn, vn, None),
        }
        for how, call in calls.items():
            def code(edit=None, op=None, rope=None, tree=None, D=64, H=64, Hkv=8, Sq=Sq0, appended=True, qo=True, kn=True, vn=True, **kw):
                a = make(pkg, D=D, H=H, Hkv=Hkv, Sq=Sq, **kw)
                if appended:
                    _kv(route, a).seqlen_add = Sq
                if edit is not None:
                    edit(_kv(route, a))
                return call(a, _fp8(pkg) if op is None else op, _rope(pkg) if rope is None else rope, _tree(pkg) if tree is None else tree,
                            _view(pkg, H, Sq, D) if qo is True else qo, _view(pkg, Hkv, Sq, D) if kn is True else kn,
                            _view(pkg, Hkv, Sq, D) if vn is True else vn)

            what = (route, how)
            if how == "plan":
                assert code() == 0 and code(appended=False, kn=None, vn=None) == 0, what
                assert code(D=128, rope=_rope(pkg, rd=128, table_dtype=1, interleaved=1, row_stride=64), tree=_tree(pkg, window=77)) == 0, what
            # NULL operands
            v = _view(pkg, 64, Sq0, 64)
            assert call(None, _fp8(pkg), _rope(pkg), _tree(pkg), v, None, None) == EINVAL, what
            assert call(make(pkg, Sq=Sq0), None, _rope(pkg), _tree(pkg), v, None, None) == EINVAL, what
            assert call(make(pkg, Sq=Sq0), _fp8(pkg), None, _tree(pkg), v, None, None) == EINVAL, what
            assert call(make(pkg, Sq=Sq0), _fp8(pkg), _rope(pkg), None, v, None, None) == EINVAL, what
            assert code(qo=None) == EINVAL and code(kn=None) == EINVAL and code(vn=None) == EINVAL and code(appended=False) == EINVAL, what
            # each operand's own codes
            assert code(op=_fp8(pkg, k_scale=None)) == EINVAL and code(op=_fp8(pkg, k_scale=DUMMY + 2)) == EALIGN, what
            for D in (32, 96, 256):
                assert code(D=D, rope=_rope(pkg, rd=32)) == EHEADDIM, (what, D)
            assert code(tree=_tree(pkg, mask=None)) == EINVAL and code(tree=_tree(pkg, reserved=2)) == EINVAL, what
            assert code(H=8, Hkv=8, Sq=65) == EUNSUPPORTED and code(lambda a: setattr(a, "causal", 0)) == EUNSUPPORTED, what
            assert code(tree=_tree(pkg, window=-2)) == EINVAL and code(tree=_tree(pkg, mask=DUMMY + 4)) == EALIGN, what
            for rd in (0, 8, 24, 80):
                assert code(rope=_rope(pkg, rd=rd, row_stride=64)) == EINVAL, (what, rd)
            assert code(rope=_rope(pkg, rows=ka.CAPACITY - 1)) == EINVAL and code(rope=_rope(pkg, interleaved=2)) == EINVAL, what
            assert code(dtype=1, rope=_rope(pkg, table_dtype=0)) == EDTYPE and code(rope=_rope(pkg, cos=DUMMY + 4)) == EALIGN, what
            assert code(qo=_view(pkg, 64, Sq0, 64, ptr=DUMMY + 2)) == EALIGN and code(kn=_view(pkg, 8, Sq0, 64, ptr=DUMMY + 2)) == EALIGN, what
            # the order: base, FP8 operand, tree operand, rope operand
            assert code(D=96, op=_fp8(pkg, k_scale=DUMMY + 2), tree=_tree(pkg, mask=None), rope=_rope(pkg, table_dtype=3)) == EHEADDIM, what
            assert code(op=_fp8(pkg, k_scale=DUMMY + 2), tree=_tree(pkg, mask=None), rope=_rope(pkg, table_dtype=3)) == EALIGN, what
            assert code(tree=_tree(pkg, mask=DUMMY + 4), rope=_rope(pkg, table_dtype=3)) == EALIGN, what                 # the tree before the rope
            assert code(H=8, Hkv=8, Sq=65, rope=_rope(pkg, rd=8)) == EUNSUPPORTED, what
            assert code(rope=_rope(pkg, table_dtype=3)) == EDTYPE, what
            assert code(lambda a: setattr(a, "seqlens", None), op=_fp8(pkg, k_scale=DUMMY + 2)) == EINVAL, what


def test_commit_refusals(pkg):
    """the codes of fasn_kvcache_tree_commit, under the rules of a cache of codes: D = 64 / 128, strides in multiples of 16"""
    lib = pkg._lib.load()
    call = lambda **over: lib.fasn_kvcache_fp8_tree_commit(kt._commit(pkg, **over), None)   # noqa: E731
    assert lib.fasn_kvcache_fp8_tree_commit(None, None) == EINVAL
    assert call(B=0) == EINVAL and call(Hkv=0) == EINVAL and call(page_size=0) == EINVAL
    for D in (32, 96, 256):
        assert call(D=D) == EHEADDIM, D
    assert lib.fasn_kvcache_tree_commit(kt._commit(pkg, D=32), None) != EHEADDIM                      # (the 16-bit commit keeps its head dims)
    assert call(seqlens=None) == EINVAL and call(k_cache=None) == EINVAL and call(v_cache=None) == EINVAL
    assert call(seqlens=DUMMY + 2) == EALIGN and call(block_table=DUMMY + 2) == EALIGN and call(k_cache=DUMMY + 8) == EALIGN
    assert call(max_pages=0) == EINVAL and call(block_table_stride=3) == EINVAL
    assert call(page_size=48) == EUNSUPPORTED
    assert call(accepted=None) == EINVAL and call(accepted_lens=None) == EINVAL and call(reserved=1) == EINVAL
    assert call(A=65, accepted_stride=65) == EUNSUPPORTED and call(nodes=65) == EUNSUPPORTED
    assert call(A=0) == EINVAL and call(nodes=0) == EINVAL and call(accepted_stride=3) == EINVAL
    assert call(accepted=DUMMY + 2) == EALIGN and call(accepted_lens=DUMMY + 2) == EALIGN
    c = kt._commit(pkg)
    c.k_stride[1] = 32
    assert lib.fasn_kvcache_fp8_tree_commit(c, None) == EINVAL
    for which in ("k_stride", "v_stride"):
        for i in range(3):
            c = kt._commit(pkg)
            getattr(c, which)[i] += 8        # 16 bytes of a 16-bit cache, half a chunk of codes
            assert lib.fasn_kvcache_fp8_tree_commit(c, None) == EALIGN, (which, i)
            assert lib.fasn_kvcache_tree_commit(c, None) != EALIGN, (which, i)
    c = kt._commit(pkg, D=96)
    c.v_stride[0] = 12
    assert lib.fasn_kvcache_fp8_tree_commit(c, None) == EHEADDIM                                          # (the head dim before the strides)


# ---------------------------------------------------------------- plans
def _plan_text(pkg):
    lib = pkg._lib.load()
    got = []
    for W in kt.GOLDEN_WINDOWS:
        for D in DIMS:
            for dtype in (0, 1):
                for route, stem, make, cases in ROUTES:
                    for name in sorted(cases):
                        c = dict(cases[name], D=D)
                        a = make(pkg, dtype=dtype, **c)
                        plan = pkg._lib.kvfp8_tree_plan(a, _fp8(pkg), _tree(pkg, window=W))
                        ws = getattr(lib, f"fasn_fwd_{stem}_fp8_tree_workspace_bytes")(a, _fp8(pkg), _tree(pkg, window=W))
                        got += [f"W={W} {route} {name} {k[0]} grid={k[1]} block={k[2]} lds={k[3]}" for k in plan] + [f"W={W} {route} {name} workspace={ws}"]
                        if W == 0:
                            a = make(pkg, dtype=dtype, **c)
                            _kv(route, a).seqlen_add = c["Sq"]
                            r = _rope(pkg, rows=c["page"] * c["max_pages"], rd=D)
                            views = (_view(pkg, c["H"], c["Sq"], D), _view(pkg, c["Hkv"], c["Sq"], D), _view(pkg, c["Hkv"], c["Sq"], D))
                            plan = pkg._lib.kvfp8_tree_rope_plan(a, _fp8(pkg), r, _tree(pkg), *views)
                            got += [f"{route} {name} rope {k[0]} grid={k[1]} block={k[2]} lds={k[3]}" for k in plan]
    return got


def test_plans_equal_the_golden_file(pkg, golden_dir):
    want = open(os.path.join(golden_dir, "kvfp8_tree_plans.txt")).read().splitlines()
    assert _plan_text(pkg) == want


@pytest.mark.parametrize("dtype", (0, 1))
@pytest.mark.parametrize("D", DIMS)
def test_plans_are_the_16_bit_tree_plans(pkg, D, dtype):
    """names of the FP8 tree and FP8 combine kernels; grids, split counts and workspace of the 16-bit tree plan of the same shape and window;
    the FP8 kernels' LDS; no dependence on lengths, scales or the mask"""
    lib = pkg._lib.load()
    tag = f"{TAGS[dtype]}, {D}"
    several = 0
    for route, stem, make, cases in ROUTES:
        for name, c in cases.items():
            c = dict(c, D=D)
            capacity = c["page"] * c["max_pages"]
            for W in (0, 1, 128, 1000, 3000, capacity, capacity + 1, 2 ** 31 - 1):
                a = make(pkg, dtype=dtype, **c)
                tree = _tree(pkg, window=W)
                base, plan = pkg._lib.kvtree_plan(a, tree), pkg._lib.kvfp8_tree_plan(a, _fp8(pkg), tree)
                assert base[0][0] == f"fasn_{stem}_fwd_tree_kernel<{tag}>"
                want = [f"fasn_{stem}_fwd_fp8_tree_kernel<{tag}>"] + ([f"fasn_{stem}_fp8_combine_kernel<{tag}>"] if len(base) == 2 else [])
                assert [k[0] for k in plan] == want, (name, W, plan)
                assert route == "prefill" or len(plan) == 2, (name, W)   # decode always combines
                assert [k[1:3] for k in plan] == [k[1:3] for k in base], (name, W, plan, base)
                assert plan[0][3] == SMEM[D] and all(k[3] == 0 for k in plan[1:]), (name, W)
                ws = getattr(lib, f"fasn_fwd_{stem}_fp8_tree_workspace_bytes")(a, _fp8(pkg), tree)
                assert ws == getattr(lib, f"fasn_fwd_{stem}_tree_workspace_bytes")(a, tree), (name, W)
                several += len(plan) == 2 and route == "prefill"
                kw = dict(seqlens=DUMMY + 4096) if route == "decode" else dict(seqlens=DUMMY + 4096, q_seqlens=DUMMY + 8192)
                other = make(pkg, dtype=dtype, **dict(c, **kw))
                _kv(route, other).seqlen_add = c["Sq"]
                assert pkg._lib.kvfp8_tree_plan(other, _fp8(pkg, k_scale=DUMMY + 64, sb=8, sh=0), _tree(pkg, window=W, mask=DUMMY + 8192, stride=128)) == plan
            # no window: the grids of the FP8 call of the same shape
            none = pkg._lib.kvfp8_tree_plan(make(pkg, dtype=dtype, **c), _fp8(pkg), _tree(pkg))
            assert [k[1:] for k in none] == [k[1:] for k in k8.fp8_plan(pkg, make(pkg, dtype=dtype, **c))], name
    assert several > 0   # a prefill with several splits and the FP8 combine kernel is among the cases


@pytest.mark.parametrize("dtype", (0, 1))
@pytest.mark.parametrize("D", DIMS)
def test_rope_append_plan_is_one_launch_on_the_16_bit_tree_rope_grid(pkg, D, dtype):
    """fasn_kv*_tree_rope_append launches fasn_kvrope_tree_kernel on the grid of fasn_kv*_rope_append - ceil(B (Hkv + H) Sq (D / 16) / 256)
    workgroups of 256, which its plan records - and so does this call"""
    name = f"fasn_kvrope_fp8_tree_kernel<{TAGS[dtype]}, {D}>"
    for route, stem, make, _cases in ROUTES:
        for c in (dict(B=4, H=64, Hkv=8, Sq=2), dict(B=3, H=8, Hkv=2, Sq=13), dict(B=2, H=12, Hkv=4, Sq=64)):
            B, H, Hkv, Sq = c["B"], c["H"], c["Hkv"], c["Sq"]
            if route == "decode" and H // Hkv * Sq > 128:
                continue

            def args(**kw):
                a = make(pkg, D=D, dtype=dtype, **dict(c, **kw))
                _kv(route, a).seqlen_add = Sq
                return a
            qo, kn = _view(pkg, H, Sq, D), _view(pkg, Hkv, Sq, D)
            plan = pkg._lib.kvfp8_tree_rope_plan(args(), _fp8(pkg), _rope(pkg, rd=16), _tree(pkg), qo, kn, kn)
            base = pkg._lib.kvrope_plan(args(), _rope(pkg, rd=16), qo, kn, kn)
            assert plan == [(name, -(-(B * (Hkv + H) * Sq * (D // 16)) // 256), 256, 0)], plan
            assert len(base) == 1 and plan[0][1:] == base[0][1:]
            assert pkg._lib.kvfp8_tree_rope_plan(args(), _fp8(pkg), _rope(pkg, rd=16), _tree(pkg), qo) == [(name, -(-(B * H * Sq * (D // 16)) // 256), 256, 0)]
            other = args(seqlens=DUMMY + 4096)
            r = _rope(pkg, rd=D, table_dtype=dtype, interleaved=1, rows=ka.CAPACITY + 100, row_stride=512, cos=DUMMY + 64)
            assert pkg._lib.kvfp8_tree_rope_plan(other, _fp8(pkg, k_scale=DUMMY + 64, sb=8, sh=0), r, _tree(pkg, window=99, mask=DUMMY + 8192), qo, kn, kn) == plan


def test_plan_lines_describe_the_kernels(pkg):
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    rc = lib.fasn_kvcache_fp8_tree_plan(ka._args_decode(pkg, Sq=8), _fp8(pkg), _tree(pkg), buf, len(buf))
    assert rc == len(buf.value) > 0
    lines = buf.value.decode().splitlines()
    assert lines[0].startswith("fasn_kvcache_fwd_fp8_tree_kernel<fasn::bf16_tag, 64> grid=") and lines[0].endswith(" block=256 lds=40960 cfg=bf16,D=64")
    assert lines[1].startswith("fasn_kvcache_fp8_combine_kernel<fasn::bf16_tag, 64> grid=")
    # the plans of the calls that were there did not move
    assert [k[0] for k in k8.fp8_plan(pkg, ka._args_decode(pkg))] == ["fasn_kvcache_fwd_fp8_kernel<fasn::bf16_tag, 64>",
                                                                     "fasn_kvcache_fp8_combine_kernel<fasn::bf16_tag, 64>"]
    assert pkg._lib.kvtree_plan(ka._args_decode(pkg, Sq=8), _tree(pkg))[0][0] == "fasn_kvcache_fwd_tree_kernel<fasn::bf16_tag, 64>"


# ---------------------------------------------------------------- the kernels
def test_new_kernels_are_there_once_and_do_not_spill(pkg):
    """(decode tree, prefill tree, tree rope append) x 2 dtypes x 2 head dims and the commit at 2 head dims = 14 kernels: once each, spill 0,
    scratch 0"""
    import spill_map
    lib = os.path.join(ROOT, "flash-attention-softmax-n_amd", "libfasn.so")
    if not os.path.exists(spill_map.READELF):
        pytest.skip("llvm-readelf not available")
    table = spill_map.kernel_table(lib)
    by_pretty = {d: m for m, d in spill_map.demangle(sorted(table)).items()}
    wanted = {}
    for D in DIMS:
        for tag in TAGS.values():
            wanted[f"fasn_kvcache_fwd_fp8_tree_kernel<{tag}, {D}>"] = "(fasn::KvParams, fasn::KvFp8, fasn::KvTree)"
            wanted[f"fasn_kvprefill_fwd_fp8_tree_kernel<{tag}, {D}>"] = "(fasn::KvPrefillParams, fasn::KvFp8, fasn::KvTree)"
            wanted[f"fasn_kvrope_fp8_tree_kernel<{tag}, {D}>"] = "(fasn::KvRopeParams, fasn::KvFp8, fasn::KvTree)"
        wanted[f"fasn_kvcache_fp8_tree_commit_kernel<{D}>"] = "(fasn::KvCommit)"
    assert len(wanted) == 14
    for name, params in sorted(wanted.items()):
        hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
        assert len(hit) == 1, (name, hit)
        assert ("void fasn::" + name + params) in by_pretty, name
        v = table[hit[0]]
        assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)
    # built for the FP8 head dims only
    fp8_tree = [d for d in by_pretty if "fp8_tree_kernel<" in d or "fp8_tree_commit_kernel<" in d]
    assert len(fp8_tree) == 14, fp8_tree


def test_no_new_spill_allowance(golden_dir):
    allowance = json.load(open(os.path.join(golden_dir, "spill_allowance.json")))
    assert not [k for k in map(str, allowance if isinstance(allowance, (list, dict)) else []) if "fp8" in k or "tree" in k]


# ---------------------------------------------------------------- the cases of the bit-for-bit comparison on the GPU
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", sorted(k8t.TWIN_CASES))
def test_twin_cases_stay_inside_the_cap_on_subnormal_results(case, D):
    """kv_fp8.assert_bitwise compares exactly where the 16-bit call's result and its product with v_scale are normal fp16 numbers, and lets
    at most 5 % of the elements be anything else. Whether a case meets that is a property of its operands, decided here from the fp32
    reference alone (kv_tree.reference_tree on the upcast cache, scale * k_scale, V unscaled: the twin's own out), on the operands the GPU
    test builds. bf16 has the exponent range of fp32: nothing to check there."""
    o = k8t.twin_operands(case, D, torch.float16, "cpu")
    masks = kt.words_tensor(o["rows"])
    out16, _lse = k8t.reference_fp8_tree(o["q"], o["kd"], o["vd"], o["lens"], o["ql"], o["n"], masks, o["k_scale"], o["v_scale"], o["window"],
                                         dequantise_v=False)
    share = k8t.subnormal_fraction(out16, o["v_scale"].repeat_interleave(o["H"] // o["Hkv"], dim=1), torch.float16)
    print(f"{case} D={D}: {100 * share:.2f} % of the reference's elements are in the subnormal range of fp16")
    assert share <= 0.05, (case, D, share)
    # the case is what its name says
    assert k8t.route_of(o["H"], o["Hkv"], o["Sq"], o["qlens"]) == ("prefill" if "prefill" in case or case == "full_g4" else "decode")
    if o["window"] is not None:
        assert o["window"] == 70 and sum(64 * (max(0, ln - x - 70 + 1) // 64) for ln, x in zip(o["lens"], o["ql"])) >= 128


# ---------------------------------------------------------------- front end on CPU tensors
def _cpu_case(Sq, D=64, dtype=torch.float16):
    B, H, Hkv = 2, 8, 2
    q = torch.zeros(B, H, Sq, D, dtype=dtype)
    kc = torch.zeros(4, 64, Hkv, D, dtype=torch.uint8).view(k8.F8)
    return q, kc, torch.zeros(B, dtype=torch.int32), torch.zeros(B, 2, dtype=torch.int32), torch.zeros(B, Sq, dtype=torch.int64)


def test_tree_front_end_refuses_with_the_reason(pkg):
    fa = pkg.flash_attention_n_kvcache_fp8_tree
    B, H, Hkv = 2, 8, 2
    for Sq in (13, 40):   # the decode kernels; 160 rows: the prefill kernels
        q, kc, sl, bt, tm = _cpu_case(Sq)
        cos, sin = torch.zeros(128, 32), torch.zeros(128, 32)
        with pytest.raises(RuntimeError, match="MI355X device tensors only"):   # every check passed
            fa(q, kc, kc, sl, 1.0, 0.5, tm, block_table=bt)
        with pytest.raises(RuntimeError, match="MI355X device tensors only"):
            fa(q, kc, kc, sl, torch.ones(Hkv), torch.ones(B, 1), tm, block_table=bt, k_new=q[:, :Hkv], v_new=q[:, :Hkv], query_seqlens=sl, return_lse=True,
               window=96, rotary_cos=cos.half()[:, :16], rotary_sin=sin.half()[:, :16], rotary_interleaved=True)
        # the tree's reasons
        with pytest.raises(TypeError, match="flash_attention_n_kvcache_fp8_tree: tree_mask must be an int64 tensor"):
            fa(q, kc, kc, sl, 1.0, 1.0, tm.int(), block_table=bt)
        with pytest.raises(TypeError, match="tree_mask must be an int64 tensor"):
            fa(q, kc, kc, sl, 1.0, 1.0, None, block_table=bt)
        with pytest.raises(ValueError, match=rf"tree_mask must be \[B, Sq\] = \[2, {Sq}\]"):
            fa(q, kc, kc, sl, 1.0, 1.0, tm[:, :-1], block_table=bt)
        with pytest.raises(RuntimeError, match="tree_mask is on meta"):
            fa(q, kc, kc, sl, 1.0, 1.0, tm.to("meta"), block_table=bt)
        with pytest.raises(ValueError, match="window must be >= 1"):
            fa(q, kc, kc, sl, 1.0, 1.0, tm, block_table=bt, window=0)
        with pytest.raises(TypeError, match="window must be None or a Python int"):
            fa(q, kc, kc, sl, 1.0, 1.0, tm, block_table=bt, window=96.0)
        with pytest.raises(ValueError, match="rotary_cos and rotary_sin come together"):
            fa(q, kc, kc, sl, 1.0, 1.0, tm, block_table=bt, rotary_cos=cos)
        with pytest.raises(ValueError, match="the rotary tables cover 100 positions but the cache holds up to 128"):
            fa(q, kc, kc, sl, 1.0, 1.0, tm, block_table=bt, rotary_cos=cos[:100], rotary_sin=sin[:100])
        with pytest.raises(ValueError, match="rotary_dim = 2 x 12 = 24 is not supported"):
            fa(q, kc, kc, sl, 1.0, 1.0, tm, block_table=bt, rotary_cos=cos[:, :12].contiguous(), rotary_sin=sin[:, :12].contiguous())
        # the FP8 cache's reasons
        for bad in (torch.zeros(4, 64, Hkv, 64, dtype=torch.float16), torch.zeros(4, 64, Hkv, 64, dtype=torch.float8_e5m2)):
            with pytest.raises(TypeError, match="must be torch.float8_e4m3fn"):
                fa(q, bad, bad, sl, 1.0, 1.0, tm, block_table=bt)
        for D in (32, 256):
            qd, kd, _sl, _bt, _tm = _cpu_case(Sq, D)
            with pytest.raises(ValueError, match=f"head dim {D} is not supported on an FP8 cache"):
                fa(qd, kd, kd, sl, 1.0, 1.0, tm, block_table=bt)
        with pytest.raises(TypeError, match="k_scale must be a Python float or a floating-point tensor"):
            fa(q, kc, kc, sl, torch.ones(Hkv, dtype=torch.int32), 1.0, tm, block_table=bt)
        with pytest.raises(ValueError, match=r"v_scale must broadcast to \[B, Hkv\] = \[2, 2\]"):
            fa(q, kc, kc, sl, 1.0, torch.ones(H), tm, block_table=bt)
        with pytest.raises(RuntimeError, match="forward only"):
            fa(q, kc, kc, sl, torch.ones(Hkv, requires_grad=True), 1.0, tm, block_table=bt)
        wide = torch.zeros(4, 64, Hkv, 72, dtype=torch.uint8).view(k8.F8)[..., :64]
        with pytest.raises(ValueError, match="strides % 16 elements"):
            fa(q, wide, wide, sl, 1.0, 1.0, tm, block_table=bt)
        with pytest.raises(ValueError, match="page_size 32 is not supported"):
            fa(q, kc[:, :32], kc[:, :32], sl, 1.0, 1.0, tm, block_table=bt)
        with pytest.raises(ValueError, match="k_new and v_new come together"):
            fa(q, kc, kc, sl, 1.0, 1.0, tm, block_table=bt, k_new=q[:, :Hkv])
    q, kc, sl, bt, _tm = _cpu_case(65)
    with pytest.raises(ValueError, match="a tree of 65 nodes is not supported"):
        fa(q, kc, kc, sl, 1.0, 1.0, torch.zeros(B, 65, dtype=torch.int64), block_table=bt)
    # the calls that were there keep their refusals, and name the new call
    q, kc, sl, bt, tm = _cpu_case(13)
    with pytest.raises(NotImplementedError, match="tree_mask is not supported on an FP8 cache"):
        pkg.flash_attention_n_kvcache_fp8(q, kc, kc, sl, 1.0, 1.0, block_table=bt, tree_mask=tm)
    with pytest.raises(NotImplementedError, match="flash_attention_n_kvcache_fp8_tree"):
        pkg.flash_attention_n_kvcache_fp8(q, kc, kc, sl, 1.0, 1.0, block_table=bt, tree_mask=tm)
    with pytest.raises(TypeError, match="query, k_cache and v_cache must share one dtype"):
        pkg.flash_attention_n_kvcache_tree(q, kc, kc, sl, tm, block_table=bt)


def test_commit_front_end_refuses_with_the_reason(pkg):
    fc = pkg.flash_attention_n_kvcache_fp8_tree_commit
    fn = "flash_attention_n_kvcache_fp8_tree_commit"
    B, Hkv = 2, 2
    kc = torch.zeros(4, 64, Hkv, 64, dtype=torch.uint8).view(k8.F8)
    sl, bt = torch.zeros(B, dtype=torch.int32), torch.zeros(B, 2, dtype=torch.int32)
    acc, alens = torch.zeros(B, 4, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X device tensors only"):   # every check passed
        fc(kc, kc, sl, acc, alens, block_table=bt)
    with pytest.raises(RuntimeError, match="MI355X device tensors only"):
        fc(kc[:B], kc[:B], sl, acc, alens)                                    # dense
    for bad in (kc.view(torch.uint8), torch.zeros(4, 64, Hkv, 64, dtype=torch.float16), torch.zeros(4, 64, Hkv, 64, dtype=torch.float8_e5m2)):
        with pytest.raises(TypeError, match=f"{fn}: k_cache and v_cache must be torch.float8_e4m3fn"):
            fc(bad, bad, sl, acc, alens, block_table=bt)
    with pytest.raises(ValueError, match=f"{fn}: the caches must be"):
        fc(kc[0], kc[0], sl, acc, alens, block_table=bt)
    for D in (32, 256):
        kd = torch.zeros(4, 64, Hkv, D, dtype=torch.uint8).view(k8.F8)
        with pytest.raises(ValueError, match=f"head dim {D} is not supported on an FP8 cache"):
            fc(kd, kd, sl, acc, alens, block_table=bt)
    with pytest.raises(ValueError, match="k_cache and v_cache must have one shape"):
        fc(kc, kc[:3], sl, acc, alens, block_table=bt)
    with pytest.raises(ValueError, match="cache_seqlens must be a contiguous int32 tensor"):
        fc(kc, kc, sl.long(), acc, alens, block_table=bt)
    with pytest.raises(ValueError, match=r"accepted must be an int32 tensor \[B, A\]"):
        fc(kc, kc, sl, acc.long(), alens, block_table=bt)
    with pytest.raises(ValueError, match="accepted is 65 nodes wide"):
        fc(kc, kc, sl, torch.zeros(B, 65, dtype=torch.int32), alens, block_table=bt)
    with pytest.raises(ValueError, match="accepted_lens must be a contiguous int32 tensor of shape \\[2\\]"):
        fc(kc, kc, sl, acc, alens[:1], block_table=bt)
    with pytest.raises(ValueError, match="page_size 32 is not supported"):
        fc(kc[:, :32], kc[:, :32], sl, acc, alens, block_table=bt)
    with pytest.raises(ValueError, match="dense cache"):
        fc(kc, kc, sl, acc, alens)
    wide = torch.zeros(4, 64, Hkv, 72, dtype=torch.uint8).view(k8.F8)[..., :64]
    with pytest.raises(ValueError, match="strides % 16 elements"):
        fc(wide, wide, sl, acc, alens, block_table=bt)
    with pytest.raises(RuntimeError, match="accepted is on meta"):
        fc(kc, kc, sl, acc.to("meta"), alens, block_table=bt)
    # the 16-bit commit still refuses a float8 cache, and names this call
    with pytest.raises(TypeError, match="flash_attention_n_kvcache_tree_commit: k_cache and v_cache must share one dtype, fp16 or bf16"):
        pkg.flash_attention_n_kvcache_tree_commit(kc, kc, sl, acc, alens, block_table=bt)
    with pytest.raises(TypeError, match="flash_attention_n_kvcache_fp8_tree_commit"):
        pkg.flash_attention_n_kvcache_tree_commit(kc, kc, sl, acc, alens, block_table=bt)


def test_signatures_and_exports(pkg):
    import flash_attention_softmax_n_amd as shim
    for name in ("flash_attention_n_kvcache_fp8_tree", "flash_attention_n_kvcache_fp8_tree_commit"):
        assert name in pkg.__all__ and getattr(shim, name) is getattr(pkg.kvcache, name)
    sig = inspect.signature(pkg.flash_attention_n_kvcache_fp8_tree)
    assert list(sig.parameters) == ["query", "k_cache", "v_cache", "cache_seqlens", "k_scale", "v_scale", "tree_mask", "block_table", "k_new", "v_new",
                                    "query_seqlens", "softmax_n_param", "scale", "return_lse", "window", "rotary_cos", "rotary_sin", "rotary_interleaved"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(block_table=None, k_new=None, v_new=None, query_seqlens=None, softmax_n_param=1, scale=None, return_lse=False, window=None,
                     rotary_cos=None, rotary_sin=None, rotary_interleaved=False)
    sig = inspect.signature(pkg.flash_attention_n_kvcache_fp8_tree_commit)
    assert list(sig.parameters) == ["k_cache", "v_cache", "cache_seqlens", "accepted", "accepted_lens", "block_table"]
    assert sig.parameters["block_table"].default is None
    # the calls that were there are what they were
    assert inspect.signature(pkg.flash_attention_n_kvcache_tree_commit) == sig
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_tree).parameters) == [p for p in inspect.signature(pkg.flash_attention_n_kvcache_fp8_tree).parameters
                                                                                      if p not in ("k_scale", "v_scale")]
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_fp8).parameters)[-1] == "tree_mask"
