"""Token-tree attention over the K/V cache (speculative-decoding verification), without a GPU: exports and layouts, the validation codes
of the nine *_tree entry points behind the base checks (fake, aligned pointers: validation comes before any HIP call), their launch plans
- the base call's rule, under a window the window call's rule with span Sq, equal to tests/golden/kvtree_plans.txt - the register tables
of the new kernels, the front end's refusals, and the reference of tests/kv_tree.py against a per-key loop."""
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
import kv_tree as kt   # noqa: E402

DUMMY, BIG = ka.DUMMY, ka.BIG
NEW = ("fasn_fwd_kvcache_tree_workspace_bytes", "fasn_fwd_kvcache_tree", "fasn_kvcache_tree_plan",
       "fasn_fwd_kvprefill_tree_workspace_bytes", "fasn_fwd_kvprefill_tree", "fasn_kvprefill_tree_plan",
       "fasn_kvcache_tree_rope_append", "fasn_kvprefill_tree_rope_append", "fasn_kvcache_tree_commit")
DIMS = (32, 64, 128, 256)
TAGS = {0: "fasn::f16_tag", 1: "fasn::bf16_tag"}
EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED, EWORKSPACE = -1, -2, -3, -4, -5, -7, -8
_tree, _win, _renamed = kt._tree, ka._win, ka._renamed


def test_symbols_are_exported_and_bound(pkg):
    import flash_attention_softmax_n_amd as shim
    lib = shim._lib.load()
    for name in NEW:
        assert name in shim._lib.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.fasn_abi_version() == 6
    T = pkg._lib.KvTree
    assert ctypes.sizeof(T) == 24 and (T.mask.offset, T.batch_stride.offset, T.window.offset, T.reserved.offset) == (0, 8, 16, 20)
    C = pkg._lib.KvTreeCommit
    assert ctypes.sizeof(C) == 144 and C.accepted.offset == 112 and C.nodes.offset == 136
    # the argument blocks kept their layouts: the operand travels beside them
    assert pkg._lib.KvPrefillArgs.kv.offset == 0 and pkg._lib.KvPrefillArgs.q_seqlens.offset == ctypes.sizeof(pkg._lib.KvCacheArgs)
    assert pkg._lib.KvCacheArgs.n_stride_h.offset + 8 == ctypes.sizeof(pkg._lib.KvCacheArgs)


def test_struct_layouts_match_the_header(pkg):
    import re
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fasn.h")).read(), flags=re.S)
    for cname, S in (("fasn_kv_tree", pkg._lib.KvTree), ("fasn_kv_tree_commit", pkg._lib.KvTreeCommit)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), text, flags=re.S).group(1)
        names = [n for _t, n in re.findall(r"([a-z0-9_ ]+?[ *]+)([A-Za-z_]+)(?:\[\d+\])?;", body)]
        assert names == [f[0] for f in S._fields_], (cname, names)


def _calls(lib, which):
    """(how -> call(args, tree)) of one route: forward, plan, workspace size (None for every refusal)"""
    stem = "kvcache" if which == "dec" else "kvprefill"
    buf = ctypes.create_string_buffer(4096)

    def plan(a, t):
        rc = getattr(lib, f"fasn_{stem}_tree_plan")(a, t, buf, len(buf))
        return rc if rc < 0 else 0
    return {"fwd": lambda a, t: getattr(lib, f"fasn_fwd_{stem}_tree")(a, t, DUMMY, BIG, None), "plan": plan,
            "ws": lambda a, t: 0 if getattr(lib, f"fasn_fwd_{stem}_tree_workspace_bytes")(a, t) > 0 else None}


def test_validation_codes_and_their_order(pkg):
    lib = pkg._lib.load()
    for which, make, kv in (("dec", ka._args_decode, lambda a: a), ("pre", ka._args_prefill, lambda a: a.kv)):
        shape = dict(Sq=8) if which == "dec" else dict(Sq=40)
        calls = _calls(lib, which)
        for how in ("fwd", "plan"):
            call = calls[how]
            good = _tree(pkg)
            # every base code through the tree entry points, with a good and with a bad operand: the base arguments come first
            for t in (good, None, _tree(pkg, reserved=1), _tree(pkg, window=-1)):
                assert call(None, t) == EINVAL
                assert call(make(pkg, B=0, **shape), t) == EINVAL
                assert call(make(pkg, dtype=2, **shape), t) == EDTYPE
                assert call(make(pkg, D=96, **shape), t) == EHEADDIM
                assert call(make(pkg, page=48, **shape), t) == EUNSUPPORTED
                a = make(pkg, **shape)
                kv(a).q.ptr = kv(a).q.ptr + 2
                assert call(a, t) == EALIGN
                a = make(pkg, **shape)
                kv(a).q.stride[3] = 2
                assert call(a, t) == ESTRIDE
                assert call(make(pkg, seqlens=None, **shape), t) == EINVAL
            if which == "dec":
                assert call(make(pkg, H=64, Hkv=8, Sq=17), good) == EUNSUPPORTED        # the decode row limit is a base rule
            # then the operand, in the documented order
            assert call(make(pkg, **shape), None) == EINVAL
            assert call(make(pkg, **shape), _tree(pkg, mask=None)) == EINVAL
            assert call(make(pkg, **shape), _tree(pkg, reserved=1)) == EINVAL
            wide = make(pkg, H=8, Hkv=8, Sq=65)                                           # 65 rows: fine for both base calls
            assert call(wide, good) == EUNSUPPORTED
            assert call(wide, _tree(pkg, reserved=1)) == EINVAL                           # (reserved comes before the node count)
            kv(wide).causal = 0
            assert call(wide, good) == EUNSUPPORTED
            a = make(pkg, **shape)
            kv(a).causal = 0
            assert call(a, good) == EUNSUPPORTED                                          # always causal
            assert call(a, _tree(pkg, window=-1)) == EUNSUPPORTED                         # (causal comes before the window)
            assert call(make(pkg, **shape), _tree(pkg, window=-1)) == EINVAL
            assert call(make(pkg, **shape), _tree(pkg, stride=-1)) == EINVAL
            assert call(make(pkg, **shape), _tree(pkg, mask=DUMMY + 4)) == EALIGN
            if how == "plan":   # (accepted arguments are only ever recorded, never launched)
                for w in (0, 1, 5, 128, 8192, 8193, 2 ** 31 - 1):
                    assert call(make(pkg, **shape), _tree(pkg, window=w)) == 0
                assert call(make(pkg, H=8, Hkv=8, Sq=64), good) == 0
        ws = calls["ws"]
        assert ws(None, _tree(pkg)) is None and ws(make(pkg, D=96, **shape), _tree(pkg)) is None
        assert ws(make(pkg, **shape), None) is None and ws(make(pkg, **shape), _tree(pkg, reserved=3)) is None
        assert ws(make(pkg, H=8, Hkv=8, Sq=65), _tree(pkg)) is None
    # then the workspace: missing, too small, misaligned - sized by the tree call's own size function
    a = ka._args_decode(pkg, Sq=8)
    need = lib.fasn_fwd_kvcache_tree_workspace_bytes(a, _tree(pkg))
    assert need == lib.fasn_fwd_kvcache_workspace_bytes(a) > 0
    assert 0 < lib.fasn_fwd_kvcache_tree_workspace_bytes(a, _tree(pkg, window=128)) == lib.fasn_fwd_kvcache_window_workspace_bytes(a, _win(pkg, 128)) < need
    assert lib.fasn_fwd_kvcache_tree(a, _tree(pkg), DUMMY, need - 1, None) == EWORKSPACE
    assert lib.fasn_fwd_kvcache_tree(a, _tree(pkg), None, need, None) == EWORKSPACE
    assert lib.fasn_fwd_kvcache_tree(a, _tree(pkg), DUMMY + 4, need, None) == EALIGN
    assert lib.fasn_fwd_kvcache_tree(a, None, None, 0, None) == EINVAL                    # (the operand before the workspace)
    buf = ctypes.create_string_buffer(4096)
    assert lib.fasn_kvcache_tree_plan(a, _tree(pkg), None, 10) == EINVAL and lib.fasn_kvcache_tree_plan(a, _tree(pkg), buf, 8) == EINVAL


def test_rope_append_validation(pkg):
    """the base checks, then the rope operand's, then the tree's"""
    lib = pkg._lib.load()
    for stem, make, kv, Sq in (("kvcache", ka._args_decode, lambda a: a, 8), ("kvprefill", ka._args_prefill, lambda a: a.kv, 40)):
        fn = getattr(lib, f"fasn_{stem}_tree_rope_append")

        def call(a, rope, tree, H=64, Hkv=8, S=Sq):
            return fn(a, rope, tree, ka._view(pkg, H, S, 64), ka._view(pkg, Hkv, S, 64), ka._view(pkg, Hkv, S, 64), None)

        def args(**kw):
            a = make(pkg, **dict(dict(Sq=Sq), **kw))
            kv(a).seqlen_add = kv(a).Sq
            return a
        assert call(args(D=96), ka._rope(pkg, rd=7), None) == EHEADDIM
        assert call(args(), ka._rope(pkg, rd=7), None) == EINVAL
        assert call(args(), None, _tree(pkg)) == EINVAL
        assert call(args(), ka._rope(pkg, table_dtype=3), None) == EDTYPE                 # (the rope operand before the tree operand)
        assert call(args(), ka._rope(pkg), None) == EINVAL
        assert call(args(), ka._rope(pkg), _tree(pkg, mask=None)) == EINVAL
        assert call(args(), ka._rope(pkg), _tree(pkg, reserved=2)) == EINVAL
        assert call(args(H=8, Hkv=8, Sq=65), ka._rope(pkg), _tree(pkg), H=8, Hkv=8, S=65) == EUNSUPPORTED
        a = args()
        kv(a).causal = 0
        assert call(a, ka._rope(pkg), _tree(pkg)) == EUNSUPPORTED
        assert call(args(), ka._rope(pkg), _tree(pkg, window=-2)) == EINVAL
        assert call(args(), ka._rope(pkg), _tree(pkg, mask=DUMMY + 4)) == EALIGN


def test_commit_validation(pkg):
    lib = pkg._lib.load()
    call = lambda **over: lib.fasn_kvcache_tree_commit(kt._commit(pkg, **over), None)   # noqa: E731
    assert lib.fasn_kvcache_tree_commit(None, None) == EINVAL
    assert call(B=0) == EINVAL and call(Hkv=0) == EINVAL and call(page_size=0) == EINVAL
    assert call(D=96) == EHEADDIM
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
    assert lib.fasn_kvcache_tree_commit(c, None) == EINVAL
    c = kt._commit(pkg)
    c.v_stride[0] = 12
    assert lib.fasn_kvcache_tree_commit(c, None) == EALIGN


# ---------------------------------------------------------------- plans
def _nsplit(D, blocks, tiles, R):
    return max(1, min(-(-(512 if D == 256 else 1024) // blocks), tiles // max(4, R // 8)))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", sorted(kt.DECODE_CASES))
def test_decode_plan(pkg, case, D, dtype):
    """no window: the base plan; a window: the window call's plan (its span is Sq on this route) - up to the forward kernel's name"""
    c = dict(kt.DECODE_CASES[case], D=D)
    lib = pkg._lib.load()
    tag = "%s, %d" % (TAGS[dtype], D)
    args = lambda **kw: ka._args_decode(pkg, dtype=dtype, **dict(c, **kw))   # noqa: E731
    base = pkg._lib.kvcache_plan(args())
    capacity = c["page"] * c["max_pages"]
    for W in (0, capacity, capacity + 1, 2 ** 31 - 1):
        plan = pkg._lib.kvtree_plan(args(), _tree(pkg, window=W))
        assert plan == _renamed(base, "fasn_kvcache_fwd_kernel", "fasn_kvcache_fwd_tree_kernel") and plan != base
        assert lib.fasn_fwd_kvcache_tree_workspace_bytes(args(), _tree(pkg, window=W)) == lib.fasn_fwd_kvcache_workspace_bytes(args())
    for W in (1, 128, 1000, 3000):
        plan = pkg._lib.kvtree_plan(args(), _tree(pkg, window=W))
        assert plan == _renamed(pkg._lib.kvcache_window_plan(args(), _win(pkg, W)), "fasn_kvcache_fwd_window_kernel", "fasn_kvcache_fwd_tree_kernel")
        assert [k[0] for k in plan] == [f"fasn_kvcache_fwd_tree_kernel<{tag}>", f"fasn_kvcache_combine_kernel<{tag}>"]
        assert lib.fasn_fwd_kvcache_tree_workspace_bytes(args(), _tree(pkg, window=W)) == lib.fasn_fwd_kvcache_window_workspace_bytes(args(), _win(pkg, W))
        # other lengths, another table, another mask (other device pointers), an append: the same launches
        other = args(seqlens=DUMMY + 4096)
        other.block_table = DUMMY + 65536
        other.seqlen_add = c["Sq"]
        assert pkg._lib.kvtree_plan(other, _tree(pkg, window=W, mask=DUMMY + 8192, stride=128)) == plan
    assert pkg._lib.kvcache_plan(args()) == base


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", sorted(kt.PREFILL_CASES))
def test_prefill_plan(pkg, case, D, dtype):
    """no window: the base plan; a window: the window call's rule with span Sq - the window plan itself wherever PB and Sq touch as many tiles"""
    c = dict(kt.PREFILL_CASES[case], D=D)
    lib = pkg._lib.load()
    tag = "%s, %d" % (TAGS[dtype], D)
    args = lambda **kw: ka._args_prefill(pkg, dtype=dtype, **dict(c, **kw))   # noqa: E731
    base = pkg._lib.kvprefill_plan(args())
    capacity = c["page"] * c["max_pages"]
    PB = 128 // (c["H"] // c["Hkv"])
    blocks = c["B"] * c["Hkv"] * -(-c["Sq"] // PB)
    for W in (0, capacity, 2 ** 31 - 1):
        plan = pkg._lib.kvtree_plan(args(), _tree(pkg, window=W))
        assert plan == _renamed(base, "fasn_kvprefill_fwd_kernel", "fasn_kvprefill_fwd_tree_kernel") and plan != base
        assert lib.fasn_fwd_kvprefill_tree_workspace_bytes(args(), _tree(pkg, window=W)) == lib.fasn_fwd_kvprefill_workspace_bytes(args())
    for W in (1, 128, 1000, 3000):
        plan = pkg._lib.kvtree_plan(args(), _tree(pkg, window=W))
        tiles = lambda span: min(-(-capacity // 64), -(-(W + span - 1) // 64) + 1)   # noqa: E731
        nsplit = _nsplit(D, blocks, tiles(c["Sq"]), 128)
        want = [f"fasn_kvprefill_fwd_tree_kernel<{tag}>"] + ([f"fasn_kvprefill_combine_kernel<{tag}>"] if nsplit > 1 else [])
        assert [k[0] for k in plan] == want and plan[0][1] == blocks * nsplit <= base[0][1] and plan[0][2:] == base[0][2:]
        ws = lib.fasn_fwd_kvprefill_tree_workspace_bytes(args(), _tree(pkg, window=W))
        assert ws == (blocks * nsplit * 128 * (D + 2) * 4 if nsplit > 1 else 0)
        if tiles(PB) == tiles(c["Sq"]):
            win = pkg._lib.kvprefill_window_plan(args(), _win(pkg, W))
            assert plan == _renamed(win, "fasn_kvprefill_fwd_window_kernel", "fasn_kvprefill_fwd_tree_kernel")
        other = args(seqlens=DUMMY + 4096, q_seqlens=DUMMY + 8192)
        other.kv.seqlen_add = c["Sq"]
        assert pkg._lib.kvtree_plan(other, _tree(pkg, window=W, mask=DUMMY + 8192)) == plan
    assert pkg._lib.kvprefill_plan(args()) == base


def _plan_text(pkg):
    lib = pkg._lib.load()
    got = []
    for W in kt.GOLDEN_WINDOWS:
        for D in DIMS:
            for dtype in (0, 1):
                for route, cases, make, fn in (("decode", kt.DECODE_CASES, ka._args_decode, lib.fasn_kvcache_tree_plan),
                                               ("prefill", kt.PREFILL_CASES, ka._args_prefill, lib.fasn_kvprefill_tree_plan)):
                    for name in sorted(cases):
                        buf = ctypes.create_string_buffer(4096)
                        rc = fn(make(pkg, dtype=dtype, **dict(cases[name], D=D)), _tree(pkg, window=W), buf, len(buf))
                        assert rc > 0, (name, D, dtype, W, rc)
                        got += [f"W={W} {route} {name} {line}" for line in buf.value.decode().splitlines()]
    return got


def test_plans_equal_the_golden_file(pkg, golden_dir):
    want = open(os.path.join(golden_dir, "kvtree_plans.txt")).read().splitlines()
    assert _plan_text(pkg) == want


def test_new_kernels_do_not_spill(pkg):
    """2 routes x 2 dtypes x 4 head dims = 16 forward kernels, the 8 rotary kernels and the 4 commit kernels: spill 0, scratch 0"""
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
            wanted.add(pkg._lib.kvtree_plan(ka._args_decode(pkg, dtype=dtype, **dict(kt.DECODE_CASES["gqa16"], D=D)), _tree(pkg))[0][0])
            wanted.add(pkg._lib.kvtree_plan(ka._args_prefill(pkg, dtype=dtype, **dict(kt.PREFILL_CASES["gqa40"], D=D)), _tree(pkg, window=128))[0][0])
            wanted.add(f"fasn_kvrope_tree_kernel<{TAGS[dtype]}, {D}>")
        wanted.add(f"fasn_kvcache_tree_commit_kernel<{D}>")
    assert len(wanted) == 28 and sum("_fwd_tree_kernel<" in n for n in wanted) == 16, wanted
    for name in sorted(wanted):
        hit = [m for d, m in by_pretty.items() if d.startswith("void fasn::" + name + "(")]
        assert len(hit) == 1, (name, hit)
        v = table[hit[0]]
        assert v.get("spill", 0) == 0 and v.get("scratch", 0) == 0, (name, v)


def test_no_new_spill_allowance(golden_dir):
    import json
    allowance = json.load(open(os.path.join(golden_dir, "spill_allowance.json")))
    assert not [k for k in map(str, allowance if isinstance(allowance, (list, dict)) else []) if "tree" in k or "kvcache" in k or "kvprefill" in k]


# ---------------------------------------------------------------- front end on CPU tensors
def test_front_end_refuses_with_the_reason(pkg):
    fa = pkg.flash_attention_n_kvcache_tree
    B, H, Hkv = 2, 8, 2
    kc = torch.zeros(4, 64, Hkv, 64, dtype=torch.float16)
    sl = torch.zeros(B, dtype=torch.int32)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    cos = torch.zeros(128, 16)
    for Sq in (13, 40):   # 52 rows: the decode kernels; 160 rows: the prefill kernels
        q = torch.zeros(B, H, Sq, 64, dtype=torch.float16)
        tm = torch.zeros(B, Sq, dtype=torch.int64)
        for bad in (tm.int(), tm.bool(), tm.float(), None, [[0] * Sq] * B):
            with pytest.raises(TypeError, match="tree_mask must be an int64 tensor"):
                fa(q, kc, kc, sl, bad, block_table=bt)
        for bad in (tm[:, :-1], tm[:1], tm.view(-1), tm.unsqueeze(1)):
            with pytest.raises(ValueError, match=r"tree_mask must be \[B, Sq\] = \[2, %d\]" % Sq):
                fa(q, kc, kc, sl, bad, block_table=bt)
        with pytest.raises(RuntimeError, match="tree_mask is on meta"):
            fa(q, kc, kc, sl, tm.to("meta"), block_table=bt)
        with pytest.raises(ValueError, match="rotary_cos and rotary_sin come together"):
            fa(q, kc, kc, sl, tm, block_table=bt, rotary_cos=cos)
        with pytest.raises(ValueError, match="rotary_cos and rotary_sin come together"):
            fa(q, kc, kc, sl, tm, block_table=bt, rotary_sin=cos)
        with pytest.raises(ValueError, match="the rotary tables cover 64 positions but the cache holds up to 128"):
            fa(q, kc, kc, sl, tm, block_table=bt, rotary_cos=cos[:64], rotary_sin=cos[:64])
        with pytest.raises(ValueError, match="rotary_dim = 2 x 4 = 8 is not supported"):
            fa(q, kc, kc, sl, tm, block_table=bt, rotary_cos=cos[:, :4], rotary_sin=cos[:, :4])
        with pytest.raises(TypeError, match="window must be None or a Python int"):
            fa(q, kc, kc, sl, tm, block_table=bt, window=4.0)
        with pytest.raises(ValueError, match="window must be >= 1"):
            fa(q, kc, kc, sl, tm, block_table=bt, window=0)
        # the base calls keep refusing what they refuse
        with pytest.raises(ValueError, match="int32"):
            fa(q, kc, kc, sl.long(), tm, block_table=bt)
        with pytest.raises(ValueError, match="query_seqlens must be a contiguous int32 tensor of shape \\[2\\]"):
            fa(q, kc, kc, sl, tm, block_table=bt, query_seqlens=sl.long())
        with pytest.raises(RuntimeError, match="forward only"):
            fa(q.clone().requires_grad_(), kc, kc, sl, tm, block_table=bt)
        with pytest.raises(ValueError, match="k_new and v_new come together"):
            fa(q, kc, kc, sl, tm, block_table=bt, k_new=torch.zeros(B, Hkv, Sq, 64, dtype=torch.float16))
        # a valid call gets as far as the CPU-tensor refusal, on both routes, with and without window, rotary, lengths and new rows
        kn = torch.zeros(B, Hkv, Sq, 64, dtype=torch.float16)
        for kw in ({}, dict(window=5), dict(rotary_cos=cos, rotary_sin=cos), dict(query_seqlens=sl), dict(k_new=kn, v_new=kn),
                   dict(window=10 ** 12, rotary_cos=cos.half(), rotary_sin=cos.half(), rotary_interleaved=True, k_new=kn, v_new=kn)):
            with pytest.raises(RuntimeError, match="CPU tensor"):
                fa(q, kc, kc, sl, tm, block_table=bt, **kw)
    with pytest.raises(ValueError, match="a tree of 65 nodes is not supported \\(at most 64"):
        fa(torch.zeros(B, H, 65, 64, dtype=torch.float16), kc, kc, sl, torch.zeros(B, 65, dtype=torch.int64), block_table=bt)
    with pytest.raises(ValueError, match="head dim 96"):
        k96 = torch.zeros(4, 64, 2, 96, dtype=torch.float16)
        fa(torch.zeros(B, H, 4, 96, dtype=torch.float16), k96, k96, sl, torch.zeros(B, 4, dtype=torch.int64), block_table=bt)


def test_commit_front_end_refuses_with_the_reason(pkg):
    fc = pkg.flash_attention_n_kvcache_tree_commit
    B, Hkv = 2, 2
    kc = torch.zeros(4, 64, Hkv, 64, dtype=torch.float16)
    sl = torch.zeros(B, dtype=torch.int32)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    acc = torch.zeros(B, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="accepted is 65 nodes wide; a path has at most 64"):
        fc(kc, kc, sl, torch.zeros(B, 65, dtype=torch.int32), sl, block_table=bt)
    with pytest.raises(ValueError, match=r"accepted must be an int32 tensor \[B, A\]"):
        fc(kc, kc, sl, acc.long(), sl, block_table=bt)
    with pytest.raises(ValueError, match=r"accepted must be an int32 tensor \[B, A\]"):
        fc(kc, kc, sl, acc[:1], sl, block_table=bt)
    with pytest.raises(ValueError, match="accepted_lens must be a contiguous int32 tensor of shape \\[2\\]"):
        fc(kc, kc, sl, acc, sl.long(), block_table=bt)
    with pytest.raises(ValueError, match="cache_seqlens must be a contiguous int32"):
        fc(kc, kc, sl.long(), acc, sl, block_table=bt)
    with pytest.raises(TypeError, match="one dtype"):
        fc(kc, kc.bfloat16(), sl, acc, sl, block_table=bt)
    with pytest.raises(ValueError, match="dense cache"):
        fc(kc, kc, sl, acc, sl)
    with pytest.raises(ValueError, match="page_size 48"):
        k48 = torch.zeros(4, 48, Hkv, 64, dtype=torch.float16)
        fc(k48, k48, sl, acc, sl, block_table=bt)
    with pytest.raises(RuntimeError, match="accepted is on meta"):
        fc(kc, kc, sl, acc.to("meta"), sl, block_table=bt)
    for kw in (dict(block_table=bt), ):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            fc(kc, kc, sl, acc, sl, **kw)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        kd = torch.zeros(B, 100, Hkv, 64, dtype=torch.float16)
        fc(kd, kd, sl, acc, sl)


def test_signatures_and_exports(pkg):
    import flash_attention_softmax_n_amd as shim
    for name in ("flash_attention_n_kvcache_tree", "flash_attention_n_kvcache_tree_commit"):
        assert name in pkg.__all__ and getattr(shim, name) is getattr(pkg.kvcache, name)
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_tree).parameters) == [
        "query", "k_cache", "v_cache", "cache_seqlens", "tree_mask", "block_table", "k_new", "v_new", "query_seqlens", "softmax_n_param", "scale",
        "return_lse", "window", "rotary_cos", "rotary_sin", "rotary_interleaved"]
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_tree_commit).parameters) == [
        "k_cache", "v_cache", "cache_seqlens", "accepted", "accepted_lens", "block_table"]
    # the existing calls kept theirs
    assert "tree_mask" not in inspect.signature(pkg.flash_attention_n_kvcache).parameters
    assert list(inspect.signature(pkg.flash_attention_n_kvcache_window).parameters)[-1] == "return_lse"


# ---------------------------------------------------------------- tests/kv_tree.py itself
def test_mask_builders():
    gen = torch.Generator().manual_seed(3)
    assert kt.chain(4) == [1, 3, 7, 15] and kt.star(4) == [1, 3, 5, 9]
    words, parents = kt.random_tree(40, gen)
    for i, (w, par) in enumerate(zip(words, parents)):
        anc, a = {i}, par
        while a >= 0:
            anc.add(a)
            a = parents[a]
        assert w == sum(1 << t for t in anc) and kt.depth(w, 40) == len(anc) - 1 and par < i
    for Sq in (13, 64):
        arb = kt.arbitrary(Sq, gen)
        assert 0 in arb and any((w & ((1 << Sq) - 1)) >> (i + 1) for i, w in enumerate(arb)) and any(not (w >> i) & 1 for i, w in enumerate(arb))
    arb = kt.arbitrary(64, gen)
    assert arb[63] >> 63 and any(w >> 63 for w in arb[:63]) and kt.words_of(kt.words_tensor([arb])) == [arb]
    assert kt.words_tensor([[1 << 63]]).item() == -2 ** 63 and kt.depth(kt.FULL, 64) == 63 and kt.depth(kt.FULL, 5) == 4 and kt.depth(0, 9) == 0
    assert kt.depths(kt.words_tensor([kt.chain(5), kt.star(5)]), [5, 3]).tolist() == [[0, 1, 2, 3, 4], [0, 1, 1, 0, 0]]


@pytest.mark.parametrize("window", [None, 1, 5, 64, 1000])
def test_reference_visibility_against_a_per_key_loop(window):
    gen = torch.Generator().manual_seed(11)
    for Sq, lens, qlens in ((13, [13, 73, 141], [13, 13, 13]), (40, [110, 7, 200], [40, 7, 0]), (64, [64, 191], [64, 64]), (5, [3, 5], [5, 5])):
        S = max(lens) + 9
        for kind in ("chain", "tree", "star", "arbitrary"):
            rows = [{"chain": kt.chain(Sq), "tree": kt.random_tree(Sq, gen)[0], "star": kt.star(Sq), "arbitrary": kt.arbitrary(Sq, gen)}[kind]
                    for _ in lens]
            vis = kt.tree_vis(lens, qlens, Sq, S, kt.words_tensor(rows), window)
            assert vis.shape == (len(lens), 1, Sq, S)
            for b, (ln, ql) in enumerate(zip(lens, qlens)):
                assert torch.equal(vis[b, 0, :ql], kt.tree_vis_brute(ln, ql, S, rows[b], window)), (Sq, kind, b)
                assert not vis[b, 0, ql:].any() and not vis[b, 0, :, ln:].any()
            if kind == "chain" and (window is None or window >= Sq):   # the chain is the causal rule of the other cache calls (a window does
                # not hide a node's ancestors: the window rule only where it holds all Sq of them)
                import kv_support as ks
                assert torch.equal(vis, ks._rule_mask(lens, qlens, Sq, S, True if window is None else window, "cpu"))
