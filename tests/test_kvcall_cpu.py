"""The cache calls by operand set (fasn_kv_forward_workspace_bytes, fasn_kv_forward, fasn_kv_forward_plan, fasn_kv_append,
fasn_kv_append_plan: a fasn_kv_call names the block and the operands present) and the packed FP8 sets they alone reach, without a GPU.

1. For every set a named entry point serves - every block of kv_args.BASES as a decode and as a prefill block, packed blocks of
   kv_args._args_varlen - the operand-set call returns the named call's code, workspace bytes and plan text, byte for byte; with one rule
   broken (every one of kv_args.BASE_RULES, the FP8 operand's, the window's) the two routes return one code.
2. The census of the new family: five names, bound as declared, a NULL call refused.
3. Sets without kernels are FASN_EUNSUPPORTED behind the base checks; the new sets are accepted.
4. The plans of the packed FP8 sets (tests/golden/kvfp8_varlen_plans.txt): schedule, forward, the FP8 combine with several splits only;
   grids and launch count of the 16-bit packed plan of the same shape; the appends are one launch.
5. The front end of flash_attention_n_kvcache_fp8_varlen, _fp8_varlen_window and _fp8_varlen_rope on CPU tensors: the refusals come first.

Nothing is ever launched: the pointers are fake. The calls that would launch are only made with calls the plan has just refused.

    python tests/test_kvcall_cpu.py --record     rewrites the fixture from the library of this tree
"""
import ctypes
import hashlib
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kv_args as ka   # noqa: E402
import kv_fp8 as k8    # noqa: E402

DUMMY, BIG = ka.DUMMY, ka.BIG
PLANS = os.path.join(ROOT, "tests", "golden", "kvfp8_varlen_plans.txt")
EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED, EWORKSPACE = -1, -2, -3, -4, -5, -7, -8
FIVE = ("fasn_kv_forward_workspace_bytes", "fasn_kv_forward", "fasn_kv_forward_plan", "fasn_kv_append", "fasn_kv_append_plan")
F8 = torch.float8_e4m3fn


def _text(fn, *operands):
    """(return value, the plan text) of a *_plan call"""
    buf = ctypes.create_string_buffer(4096)
    rc = fn(*operands, buf, len(buf))
    return rc, buf.value if rc > 0 else b""


def _tree(pkg, window=0):
    return pkg._lib.KvTree(mask=DUMMY + 4096, batch_stride=64, window=window, reserved=0)


def _operands(pkg, c=None):
    """one operand of each kind over fake pointers; the window and the slopes of a kv_args.Case where there is one"""
    return dict(fp8=k8._fp8(pkg), tree=_tree(pkg), window=c.win if c is not None else ka._win(pkg, window=100),
                alibi=c.alibi if c is not None else ka._slopes(pkg))


def _both_forward(pkg, stem, args, ops):
    """((code or bytes written, text), workspace bytes) of the named forward of `stem` under the operands `ops` and of the operand-set call"""
    L, lib = pkg._lib, pkg._lib.load()
    ws_name, ws_ops, _fwd, plan, operands = L.kv_forward_call(stem, **ops)
    named = _text(getattr(lib, plan), args, *operands), getattr(lib, ws_name)(args, *ws_ops)
    call = L.kv_call(args, **ops)
    return named, (_text(lib.fasn_kv_forward_plan, call), lib.fasn_kv_forward_workspace_bytes(call))


def _blocks(pkg, base):
    """(stem, block, Case) of a kv_args.BASES block as a decode and as a prefill block"""
    out = []
    for stem in ("kvcache", "kvprefill"):
        c = ka.Case(pkg._lib, ka.BASES[base])
        c.pa.q_seqlens = c.qlens
        out.append((stem, c.kv if stem == "kvcache" else c.pa, c))
    return out


PACKED = {
    "small": dict(B=4, H=64, Hkv=8, Sq=48, D=64, page=256, max_pages=64, T=64),
    "large": dict(B=257, H=8, Hkv=8, Sq=4096, D=128, page=256, max_pages=32, T=4352),
    "d32": dict(B=3, H=8, Hkv=2, Sq=40, D=32, page=64, max_pages=8, T=100, dtype=0),
}


def _packed(pkg, name, appended=True):
    va = ka._args_varlen(pkg, **PACKED[name])
    if appended:
        va.pf.kv.seqlen_add = va.pf.kv.Sq
    return va


# ---------------------------------------------------------------- 1. equivalence with the named entry points
def test_forward_plan_and_workspace_equal_every_named_call(pkg):
    L = pkg._lib
    seen = accepted = 0
    for base in ka.BASES:
        for stem, args, c in _blocks(pkg, base):
            every = _operands(pkg, c)
            for ops in L._KV_FORWARD_SETS:
                named, generic = _both_forward(pkg, stem, args, {o: every[o] for o in ops})
                assert named == generic, (base, stem, ops, named[0][0], generic[0][0])
                seen, accepted = seen + 1, accepted + (named[0][0] > 0)
    for name in PACKED:
        every = _operands(pkg)
        for ops in ((), ("window",)):
            named, generic = _both_forward(pkg, "kvvarlen", _packed(pkg, name, False), {o: every[o] for o in ops})
            assert named == generic and named[0][0] > 0 and named[1] > 0, (name, ops)
            seen, accepted = seen + 1, accepted + 1
    assert seen == 2 * len(ka.BASES) * 7 + 2 * len(PACKED) and accepted >= seen // 2, (seen, accepted)


def _both_append(pkg, stem, args, ops, views):
    """(code or bytes written, text) of the named *_append_plan of `stem` under `ops` (in suffix order) and of fasn_kv_append_plan"""
    L, lib = pkg._lib, pkg._lib.load()
    name, operands = L.kv_append_call(stem, **ops)
    q_out, k_new, v_new = views
    named = _text(getattr(lib, name + "_plan"), args, *operands, q_out, k_new, v_new)
    call = L.kv_call(args, fp8=ops.get("fp8"), tree=ops.get("tree"))
    return named, _text(lib.fasn_kv_append_plan, call, ops.get("rope"), q_out, k_new, v_new)


def test_append_plan_equals_every_named_append_plan(pkg):
    L = pkg._lib
    seen = accepted = 0
    for base in ka.BASES:
        for stem, args, c in _blocks(pkg, base):
            every = dict(_operands(pkg, c), rope=c.rope)
            for ops, has_plan in L._KV_APPENDS:
                if not has_plan:
                    continue
                for views in ((c.qo, c.kn, c.vn), (c.qo, None, None)):
                    named, generic = _both_append(pkg, stem, args, {o: every[o] for o in ops}, views)
                    assert named == generic, (base, stem, ops, named[0], generic[0])
                    seen, accepted = seen + 1, accepted + (named[0] > 0)
    for name in PACKED:
        va, p = _packed(pkg, name), PACKED[name]
        views = (ka._tview(pkg, p["H"], p["D"]), ka._tview(pkg, p["Hkv"], p["D"]), ka._tview(pkg, p["Hkv"], p["D"]))
        rope = ka._rope(pkg, rows=p["page"] * p["max_pages"], rd=32)
        named, generic = _both_append(pkg, "kvvarlen", va, dict(rope=rope), views)
        assert named == generic and named[0] > 0, name
        seen, accepted = seen + 1, accepted + 1
    assert seen == 2 * len(ka.BASES) * 3 * 2 + len(PACKED) and accepted >= seen // 3, (seen, accepted)


def test_the_appends_without_a_named_plan_are_one_launch_of_the_named_kernel(pkg):
    """fasn_kv*_append and fasn_kv*_fp8_append have no *_plan sibling: the operand-set plan shows their one launch"""
    L = pkg._lib
    for stem, args, c in _blocks(pkg, "dec_paged") + _blocks(pkg, "pre_paged_qlens")[1:]:   # (300 positions are no decode block)
        for fp8, kernel in ((None, f"fasn_{stem}_append_kernel<"), (k8._fp8(pkg), f"fasn_{stem}_fp8_append_kernel<")):
            plan = L.kv_call_append_plan(L.kv_call(args, fp8=fp8, window=c.win, alibi=c.alibi), None, None, c.kn, c.vn)
            assert len(plan) == 1 and plan[0][0].startswith(kernel) and plan[0][2:] == (256, 0), plan
    va, p = _packed(pkg, "small"), PACKED["small"]
    kn = ka._tview(pkg, p["Hkv"], p["D"])
    plan = L.kv_call_append_plan(L.kv_call(va), None, None, kn, kn)
    assert len(plan) == 1 and plan[0][0].startswith("fasn_kvvarlen_append_kernel<64>") and plan[0][1] == -(-p["T"] * p["Hkv"] * 8 // 256)


FP8_RULES = [
    ("fp8_scale_null", lambda o: setattr(o, "k_scale", None)), ("fp8_reserved", lambda o: setattr(o, "reserved", 1)),
    ("fp8_scale_odd", lambda o: setattr(o, "v_scale", DUMMY + 2)), ("fp8_stride_negative", lambda o: setattr(o, "k_sh", -1)),
]
WINDOW_RULES = [("window_0", lambda w: setattr(w, "window", 0)), ("window_reserved", lambda w: setattr(w, "reserved", 1))]


def test_a_broken_rule_gives_one_code_on_both_routes(pkg):
    """every base rule, every FP8 rule and every window rule, on the sets (), {fp8}, {window}, {fp8, window}: the code of the named call is
    the code of the operand-set call - plan, workspace bytes and, where the plan refused, the forward and the append themselves"""
    L, lib = pkg._lib, pkg._lib.load()
    codes = set()
    for base in ("dec_paged", "pre_paged_qlens", "dec_dense"):
        for stem in ("kvcache", "kvprefill"):
            rules = [(n, "base", r) for n, r in ka.BASE_RULES] + [(n, "fp8", r) for n, r in FP8_RULES] + [(n, "window", r) for n, r in WINDOW_RULES]
            rules.append(("not_causal", "base", ka._set(causal=0)))
            for rname, what, rule in rules:
                c = ka.Case(L, ka.BASES[base])
                every = _operands(pkg, c)
                rule(c if what == "base" else every[what])
                c.pa.q_seqlens = c.qlens
                args = None if c.null else (c.kv if stem == "kvcache" else c.pa)
                for ops in ((), ("fp8",), ("window",), ("fp8", "window")):
                    use = {o: every[o] for o in ops}
                    ws_name, ws_ops, fwd, plan, operands = L.kv_forward_call(stem, **use)
                    named = _text(getattr(lib, plan), args, *operands), getattr(lib, ws_name)(args, *ws_ops)
                    call = L.KvCall(kind=L._KV_KIND[stem], reserved=0, block=None) if args is None else L.kv_call(args, **use)
                    if args is None:
                        for o in ops:
                            setattr(call, o, ctypes.pointer(every[o]))
                    generic = _text(lib.fasn_kv_forward_plan, call), lib.fasn_kv_forward_workspace_bytes(call)
                    assert named == generic, (base, stem, rname, ops, named[0][0], generic[0][0])
                    codes.add(named[0][0] if named[0][0] < 0 else 0)
                    if named[0][0] < 0:   # refused before any HIP call: the calls that would launch say the same
                        assert getattr(lib, fwd)(args, *operands, 256, BIG, None) == lib.fasn_kv_forward(call, 256, BIG, None) == named[0][0]
                        name, a_ops = L.kv_append_call(stem, fp8=use.get("fp8"))
                        rc = getattr(lib, name)(args, *a_ops, c.kn, c.vn, None)
                        assert rc == lib.fasn_kv_append(call, None, None, c.kn, c.vn, None) and rc < 0, (base, stem, rname, ops, rc)
    assert {0, EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED} <= codes, codes


# ---------------------------------------------------------------- 2. the census of the new family
def test_the_operand_set_family_is_five_entry_points(pkg):
    L, lib = pkg._lib, pkg._lib.load()
    family = {e for e in L.EXPORTS if e.startswith("fasn_kv_") and not re.search(r"kvcache|kvprefill|kvvarlen", e)}
    assert family == set(FIVE)
    rows = list(L._kv_call_bindings())
    assert [name for name, _r, _a in rows] == list(FIVE)
    header = open(os.path.join(ROOT, "include", "fasn.h")).read()
    call, view, rope = ctypes.POINTER(L.KvCall), ctypes.POINTER(L.View4), ctypes.POINTER(L.KvRope)
    declared = {
        "fasn_kv_forward_workspace_bytes": (ctypes.c_size_t, [call]),
        "fasn_kv_forward": (ctypes.c_int32, [call, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
        "fasn_kv_forward_plan": (ctypes.c_int32, [call, ctypes.c_char_p, ctypes.c_size_t]),
        "fasn_kv_append": (ctypes.c_int32, [call, rope, view, view, view, ctypes.c_void_p]),
        "fasn_kv_append_plan": (ctypes.c_int32, [call, rope, view, view, view, ctypes.c_char_p, ctypes.c_size_t]),
    }
    for name, restype, argtypes in rows:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert (restype, list(argtypes)) == declared[name], name
        m = re.search(r"\b(int|size_t) %s\(([^;]*)\);" % name, header)
        assert m and (m.group(1) == "size_t") == (restype is ctypes.c_size_t) and m.group(2).count(",") + 1 == len(argtypes), name
        rc = fn(*(None if issubclass(t, (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)) else 0 for t in argtypes))
        assert rc == (0 if name.endswith("_workspace_bytes") else EINVAL), f"{name}(NULL, ...) returned {rc}"
    # the struct as the header lays it out: two int32, then five pointers
    assert ctypes.sizeof(L.KvCall) == 48 and [getattr(L.KvCall, f).offset for f, _t in L.KvCall._fields_] == [0, 4, 8, 16, 24, 32, 40]
    assert (L.FASN_KV_CALL_DECODE, L.FASN_KV_CALL_PREFILL, L.FASN_KV_CALL_PACKED) == (0, 1, 2)
    assert re.search(r"enum \{ FASN_KV_CALL_DECODE = 0, FASN_KV_CALL_PREFILL = 1, FASN_KV_CALL_PACKED = 2 \};", header)
    assert lib.fasn_abi_version() == 6 and L.FASN_ABI_VERSION == 6


def test_the_call_itself_is_checked_and_nothing_else(pkg):
    L, lib = pkg._lib, pkg._lib.load()
    args = ka._args_decode(pkg)
    kn = ka._view(pkg, 8, 1, 64)
    buf = ctypes.create_string_buffer(4096)
    good = L.kv_call(args)
    assert lib.fasn_kv_forward_plan(good, buf, len(buf)) > 0 and lib.fasn_kv_forward_workspace_bytes(good) > 0
    for bad in (dict(kind=3), dict(kind=-1), dict(reserved=1), dict(block=None)):
        c = L.kv_call(args)
        for k, v in bad.items():
            setattr(c, k, v)
        assert lib.fasn_kv_forward_plan(c, buf, len(buf)) == EINVAL and lib.fasn_kv_forward_workspace_bytes(c) == 0, bad
        assert lib.fasn_kv_forward(c, 256, BIG, None) == EINVAL and lib.fasn_kv_append(c, None, None, kn, kn, None) == EINVAL, bad
        assert lib.fasn_kv_append_plan(c, None, None, kn, kn, buf, len(buf)) == EINVAL, bad
    assert lib.fasn_kv_forward_plan(good, None, 0) == EINVAL and lib.fasn_kv_forward_plan(good, buf, 8) == EINVAL   # (the plan's own rule)
    # a prefill block read as what its kind says: the same bytes under another kind are another call
    pa = ka._args_prefill(pkg, Sq=300)
    assert lib.fasn_kv_forward_plan(L.kv_call(pa), buf, len(buf)) > 0
    as_decode = L.kv_call(pa)
    as_decode.kind = L.FASN_KV_CALL_DECODE
    assert lib.fasn_kv_forward_plan(as_decode, buf, len(buf)) == EUNSUPPORTED   # 8 x 300 rows are no decode pass


# ---------------------------------------------------------------- 3. sets with and without kernels
def test_sets_without_kernels_are_unsupported_behind_the_base_checks(pkg):
    L, lib = pkg._lib, pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    every = _operands(pkg)
    plan = lambda call: lib.fasn_kv_forward_plan(call, buf, len(buf))   # noqa: E731
    va, pa, da = _packed(pkg, "small", False), ka._args_prefill(pkg, Sq=40), ka._args_decode(pkg)
    none = [(va, ("tree",)), (va, ("alibi",)), (va, ("fp8", "tree")), (va, ("fp8", "alibi")), (va, ("window", "alibi")),
            (pa, ("fp8", "alibi")), (da, ("fp8", "alibi")), (pa, ("window", "alibi")), (da, ("window", "alibi")), (pa, ("tree", "window")),
            (da, ("fp8", "tree", "window", "alibi"))]
    for args, ops in none:
        call = L.kv_call(args, **{o: every[o] for o in ops})
        assert plan(call) == EUNSUPPORTED and lib.fasn_kv_forward_workspace_bytes(call) == 0, ops
        assert lib.fasn_kv_forward(call, 256, BIG, None) == EUNSUPPORTED, ops
    # ... behind the base checks: a block that breaks one is refused with that rule's code, whatever the set
    bad = _packed(pkg, "small", False)
    bad.pf.kv.D = 96
    assert plan(L.kv_call(bad, tree=every["tree"])) == EHEADDIM
    bad = _packed(pkg, "small", False)
    bad.cu_seqlens_q = None
    assert plan(L.kv_call(bad, alibi=every["alibi"])) == EINVAL
    # the new sets are accepted, and checked in the family's order: the packed operands, the FP8 operand, the window
    for ops in (("fp8",), ("fp8", "window")):
        assert plan(L.kv_call(va, **{o: every[o] for o in ops})) > 0, ops
    odd = _packed(pkg, "small", False)
    odd.cu_seqlens_q = DUMMY + 2
    f8 = k8._fp8(pkg, reserved=1)
    assert plan(L.kv_call(odd, fp8=f8, window=ka._win(pkg, window=0))) == EALIGN        # the packed operands first
    assert plan(L.kv_call(va, fp8=f8, window=ka._win(pkg, window=0))) == EINVAL          # then the FP8 operand
    d32 = _packed(pkg, "d32", False)
    assert plan(L.kv_call(d32, fp8=every["fp8"], window=ka._win(pkg, window=0))) == EHEADDIM
    nc = _packed(pkg, "small", False)
    nc.pf.kv.causal = 0
    assert plan(L.kv_call(nc, fp8=every["fp8"])) > 0 and plan(L.kv_call(nc, fp8=every["fp8"], window=every["window"])) == EUNSUPPORTED
    st = _packed(pkg, "small", False)
    st.pf.kv.k_stride[2] = 72   # a multiple of 8 elements, not of 16 bytes
    assert plan(L.kv_call(st)) > 0 and plan(L.kv_call(st, fp8=every["fp8"])) == EALIGN
    # the appends: a packed tree rotary append has no kernel; the FP8 operand's rules hold behind the new rows' views
    p = PACKED["small"]
    qo, kn = ka._tview(pkg, p["H"], p["D"]), ka._tview(pkg, p["Hkv"], p["D"])
    ap, rope = _packed(pkg, "small"), ka._rope(pkg, rows=p["page"] * p["max_pages"], rd=32)
    assert lib.fasn_kv_append(L.kv_call(ap, tree=every["tree"]), rope, qo, kn, kn, None) == EUNSUPPORTED
    assert lib.fasn_kv_append(L.kv_call(ap, fp8=every["fp8"], tree=every["tree"]), rope, qo, kn, kn, None) == EUNSUPPORTED
    assert lib.fasn_kv_append(L.kv_call(ap, fp8=f8), None, None, kn, kn, None) == EINVAL
    assert lib.fasn_kv_append(L.kv_call(ap, fp8=f8), rope, qo, kn, kn, None) == EINVAL
    assert lib.fasn_kv_append(L.kv_call(ap, fp8=every["fp8"]), None, None, kn, None, None) == EINVAL
    assert lib.fasn_kv_append(L.kv_call(ap, fp8=every["fp8"]), ka._rope(pkg, rows=10, rd=32), qo, kn, kn, None) == EINVAL   # the tables are too short
    # a tree, a window and slopes take no part in an append without rope
    full = L.kv_call(ap, fp8=every["fp8"], tree=every["tree"], window=ka._win(pkg, window=0), alibi=every["alibi"])
    assert L.kv_call_append_plan(full, None, None, kn, kn) == L.kvfp8_varlen_append_plan(ap, every["fp8"], kn, kn)


# ---------------------------------------------------------------- 4. the plans of the packed FP8 sets
def _smem(D):
    return 2 * (3 if D == 64 else 2) * 64 * D + 2 * 64 * D * 2   # kv_fp8_smem: staged codes + one 16-bit image per operand


def _plan_cases():
    return {k: v for k, v in ka.plan_cases().items() if v["D"] in (64, 128)}


def _plan_text(pkg):
    L, lib = pkg._lib, pkg._lib.load()
    f8 = k8._fp8(pkg)
    got = []
    for name, shape in sorted(_plan_cases().items()):
        for dtype in (0, 1):
            va = ka._args_varlen(pkg, dtype=dtype, **shape)
            for W in (None, 128, 4000):
                win = None if W is None else ka._win(pkg, window=W)
                tag = f"{name} dtype={dtype} W={W or 0}"
                for k in L.kvfp8_varlen_plan(va, f8, win):
                    got.append(f"{tag} {k[0]} grid={k[1]} block={k[2]} lds={k[3]}")
                got.append(f"{tag} workspace={lib.fasn_kv_forward_workspace_bytes(L.kv_call(va, fp8=f8, window=win))}")
            va.pf.kv.seqlen_add = va.pf.kv.Sq
            qo, kn = ka._tview(pkg, shape["H"], shape["D"]), ka._tview(pkg, shape["Hkv"], shape["D"])
            rope = ka._rope(pkg, rows=shape["page"] * shape["max_pages"], rd=shape["D"] // 2)
            for what, plan in (("append", L.kvfp8_varlen_append_plan(va, f8, kn, kn)), ("rope", L.kvfp8_varlen_append_plan(va, f8, kn, kn, rope, qo)),
                               ("rope queries", L.kvfp8_varlen_append_plan(va, f8, None, None, rope, qo))):
                assert len(plan) == 1
                got.append(f"{name} dtype={dtype} {what} {plan[0][0]} grid={plan[0][1]} block={plan[0][2]} lds={plan[0][3]}")
    return got


def test_plans_equal_the_recorded_ones(pkg):
    want = open(PLANS).read().splitlines()
    assert _plan_text(pkg) == want


def test_plans_are_the_16_bit_packed_plans_with_the_fp8_kernels(pkg):
    L, lib = pkg._lib, pkg._lib.load()
    f8 = k8._fp8(pkg)
    several = single = 0
    for name, shape in _plan_cases().items():
        B, H, Hkv, Sq, D, T = (shape[k] for k in ("B", "H", "Hkv", "Sq", "D", "T"))
        items = ka.items_max(B, Sq, T, 128 // (H // Hkv))
        for dtype, tag in ((0, "fasn::f16_tag"), (1, "fasn::bf16_tag")):
            va = ka._args_varlen(pkg, dtype=dtype, **shape)
            for W in (None, 128, 4000):
                win = None if W is None else ka._win(pkg, window=W)
                plan = L.kvfp8_varlen_plan(va, f8, win)
                base = L.kvvarlen_plan(va) if W is None else L.kvvarlen_window_plan(va, win)
                assert [k[1:3] for k in plan] == [k[1:3] for k in base], (name, W)   # grids, blocks and the launch count
                ns = plan[1][1] // (items * Hkv)
                assert plan[1][1] == items * Hkv * ns and ns >= 1
                fwd = "fasn_kvvarlen_fwd_fp8_kernel" if W is None else "fasn_kvvarlen_fwd_window_fp8_kernel"
                names = ["fasn_kvvarlen_schedule_kernel<256>", f"{fwd}<{tag}, {D}>"] + ([f"fasn_kvvarlen_fp8_combine_kernel<{tag}, {D}>"] if ns > 1 else [])
                assert [k[0] for k in plan] == names, (name, W, plan)
                assert [k[3] for k in plan] == [0, _smem(D)] + ([0] if ns > 1 else [])
                ws = lib.fasn_kv_forward_workspace_bytes(L.kv_call(va, fp8=f8, window=win))
                ws16 = lib.fasn_fwd_kvvarlen_workspace_bytes(va) if W is None else lib.fasn_fwd_kvvarlen_window_workspace_bytes(va, win)
                assert ws == ws16 > 0, (name, W)
                several, single = several + (ns > 1), single + (ns == 1)
            # the appends: one launch each, on grids from shapes alone
            va.pf.kv.seqlen_add = Sq
            qo, kn = ka._tview(pkg, H, D), ka._tview(pkg, Hkv, D)
            rope = ka._rope(pkg, rows=shape["page"] * shape["max_pages"], rd=D // 2)
            assert L.kvfp8_varlen_append_plan(va, f8, kn, kn) == [(f"fasn_kvvarlen_fp8_append_kernel<{tag}, {D}>", -(-T * Hkv * (D // 16) // 256), 256, 0)]
            grid16 = L.kvrope_plan(va, rope, qo, kn, kn)[0][1]
            assert L.kvfp8_varlen_append_plan(va, f8, kn, kn, rope, qo) == [(f"fasn_kvvarlen_rope_fp8_kernel<{tag}, {D}>", grid16, 256, 0)]
            assert grid16 == -(-(T * Hkv + T * H) * (D // 16) // 256)
            assert L.kvfp8_varlen_append_plan(va, f8, None, None, rope, qo)[0][1] == -(-T * H * (D // 16) // 256)
    assert several and single, (several, single)


# ---------------------------------------------------------------- 5. the front end, on CPU tensors
def _tensors():
    f16 = torch.float16
    return dict(q=torch.zeros(10, 8, 64, dtype=f16), kc=torch.zeros(4, 64, 2, 64, dtype=torch.uint8).view(F8), sl=torch.zeros(2, dtype=torch.int32),
                cu=torch.tensor([0, 4, 9], dtype=torch.int32), bt=torch.zeros(2, 2, dtype=torch.int32), kn=torch.zeros(10, 2, 64, dtype=f16),
                cos=torch.zeros(128, 8), sin=torch.zeros(128, 8))   # rotary_dim 16: inside every head dim


def _calls(pkg):
    """(name, call(q, kc, sl, ks, vs, cu, max_seqlen_q, bt, **kw)) of the three functions, their own operands filled in"""
    o = _tensors()
    base = lambda q, kc, sl, ks_, vs_, cu, m, bt, **kw: pkg.flash_attention_n_kvcache_fp8_varlen(q, kc, kc, sl, ks_, vs_, cu, m, block_table=bt, **kw)   # noqa: E731
    win = lambda q, kc, sl, ks_, vs_, cu, m, bt, **kw: pkg.flash_attention_n_kvcache_fp8_varlen_window(q, kc, kc, sl, ks_, vs_, cu, m, 5, block_table=bt, **kw)   # noqa: E731
    rope = lambda q, kc, sl, ks_, vs_, cu, m, bt, **kw: pkg.flash_attention_n_kvcache_fp8_varlen_rope(q, kc, kc, sl, ks_, vs_, cu, m, o["cos"], o["sin"],   # noqa: E731
                                                                                                    block_table=bt, **kw)
    return [("flash_attention_n_kvcache_fp8_varlen", base), ("flash_attention_n_kvcache_fp8_varlen_window", win),
            ("flash_attention_n_kvcache_fp8_varlen_rope", rope)]


def test_the_three_functions_are_exported(pkg):
    import flash_attention_softmax_n_amd as shim
    for name, _call in _calls(pkg):
        assert name in pkg.__all__ and getattr(shim, name) is getattr(pkg, name)
    head = ["query", "k_cache", "v_cache", "cache_seqlens", "k_scale", "v_scale", "cu_seqlens_q", "max_seqlen_q"]
    tail = ["block_table", "k_new", "v_new", "softmax_n_param", "scale"]
    sig = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    assert sig(pkg.flash_attention_n_kvcache_fp8_varlen)[:15] == head + tail + ["is_causal", "return_lse"]
    assert sig(pkg.flash_attention_n_kvcache_fp8_varlen_window)[:15] == head + ["window"] + tail + ["return_lse"]
    assert sig(pkg.flash_attention_n_kvcache_fp8_varlen_rope)[:19] == head + ["rotary_cos", "rotary_sin"] + tail + ["is_causal", "return_lse", "window",
                                                                                                                     "rotary_interleaved"]
    for name, _call in _calls(pkg):
        extra = inspect.signature(getattr(pkg, name)).parameters
        assert extra["alibi_slopes"].default is None and extra["tree_mask"].default is None


def test_front_end_refuses_with_the_reason_and_cpu_tensors_last(pkg):
    o = _tensors()
    q, kc, sl, cu, bt, kn = o["q"], o["kc"], o["sl"], o["cu"], o["bt"], o["kn"]
    f16 = torch.float16
    for fn, call in _calls(pkg):
        with pytest.raises(RuntimeError, match="CPU tensor"):      # arguments that are right get as far as the device check
            call(q, kc, sl, 0.5, 2.0, cu, 8, bt)
        with pytest.raises(RuntimeError, match="CPU tensor"):
            call(q, kc, sl, torch.ones(2, 2), torch.ones(2), cu, 8, bt, k_new=kn, v_new=kn, softmax_n_param=torch.ones(2, 8), return_lse=True)
        with pytest.raises(RuntimeError, match="CPU tensor"):
            call(q, kc, sl, torch.ones(2, 1), torch.tensor(3.0), cu, 1 << 20, bt)
        # a 16-bit cache, D = 32 / 256
        with pytest.raises(TypeError, match=fn + ": k_cache and v_cache must be torch.float8_e4m3fn"):
            call(q, torch.zeros(4, 64, 2, 64, dtype=f16), sl, 1.0, 1.0, cu, 8, bt)
        for D in (32, 256):
            with pytest.raises(ValueError, match=fn + f": head dim {D} is not supported on an FP8 cache"):
                call(torch.zeros(10, 8, D, dtype=f16), torch.zeros(4, 64, 2, D, dtype=torch.uint8).view(F8), sl, 1.0, 1.0, cu, 8, bt)
        # malformed cu_seqlens_q / max_seqlen_q
        for bad in (torch.zeros(2, 8, 5, 64, dtype=f16), torch.zeros(10, 64, dtype=f16)):
            with pytest.raises(ValueError, match=fn + r": query must be token-packed \[T, H, D\]"):
                call(bad, kc, sl, 1.0, 1.0, cu, 8, bt)
        for bad in (cu.long(), cu.view(3, 1), torch.zeros(6, dtype=torch.int32)[::2], [0, 4, 9], torch.zeros(1, dtype=torch.int32)):
            with pytest.raises(ValueError, match=fn + r": cu_seqlens_q must be a contiguous int32 tensor of shape \[B \+ 1\]"):
                call(q, kc, sl, 1.0, 1.0, bad, 8, bt)
        with pytest.raises(RuntimeError, match="cu_seqlens_q is on meta, query on cpu"):
            call(q, kc, sl, 1.0, 1.0, cu.to("meta"), 8, bt)
        with pytest.raises(ValueError, match=fn + ": cu_seqlens_q names 3 sequences but cache_seqlens has 2"):
            call(q, kc, sl, 1.0, 1.0, torch.tensor([0, 4, 9, 9], dtype=torch.int32), 8, bt)
        for bad in (8.0, torch.tensor(8), True, None):
            with pytest.raises(TypeError, match=fn + ": max_seqlen_q must be a Python int"):
                call(q, kc, sl, 1.0, 1.0, cu, bad, bt)
        with pytest.raises(ValueError, match=fn + ": max_seqlen_q must be >= 1; got 0"):
            call(q, kc, sl, 1.0, 1.0, cu, 0, bt)
        # the scales against B = cu.shape[0] - 1 = 2 sequences (not the 10 tokens) and Hkv = 2
        for bad in (torch.ones(10, 2), torch.ones(3, 2), torch.ones(2, 8), torch.ones(2, 2, 1), torch.ones(10)):
            with pytest.raises(ValueError, match=fn + r": k_scale must broadcast to \[B, Hkv\] = \[2, 2\]"):
                call(q, kc, sl, bad, 1.0, cu, 8, bt)
            with pytest.raises(ValueError, match=fn + r": v_scale must broadcast to \[B, Hkv\] = \[2, 2\]"):
                call(q, kc, sl, 1.0, bad, cu, 8, bt)
        for bad in (None, "1", True, torch.ones(2, 2, dtype=torch.int32)):
            with pytest.raises(TypeError, match=fn + ": k_scale must be a Python float or a floating-point tensor"):
                call(q, kc, sl, bad, 1.0, cu, 8, bt)
        with pytest.raises(RuntimeError, match="v_scale is on meta, query on cpu"):
            call(q, kc, sl, 1.0, torch.ones(2, 2, device="meta"), cu, 8, bt)
        with pytest.raises(RuntimeError, match=fn + " is forward only.*k_scale requires grad"):
            call(q, kc, sl, torch.ones(2, 2, requires_grad=True), 1.0, cu, 8, bt)
        # new rows are token-packed rows in the query's dtype
        for bad in (torch.zeros(2, 2, 5, 64, dtype=f16), torch.zeros(9, 2, 64, dtype=f16), kn.bfloat16(), torch.zeros(10, 2, 64, dtype=torch.uint8).view(F8)):
            with pytest.raises(ValueError, match=r"k_new must be \[T, Hkv, D\] = \[10, 2, 64\]"):
                call(q, kc, sl, 1.0, 1.0, cu, 8, bt, k_new=bad, v_new=bad)
        with pytest.raises(ValueError, match=r"k_cache: rows must be 16-byte aligned .* % 16 elements"):
            call(q, torch.zeros(4, 64, 2, 72, dtype=torch.uint8).view(F8)[..., :64], sl, 1.0, 1.0, cu, 8, bt)
        # no kernels: ALiBi slopes and a token tree
        with pytest.raises(NotImplementedError, match=fn + ": alibi_slopes is not supported .*no ALiBi kernels"):
            call(q, kc, sl, 1.0, 1.0, cu, 8, bt, alibi_slopes=torch.ones(8))
        with pytest.raises(NotImplementedError, match=fn + ": tree_mask is not supported .*flash_attention_n_kvcache_fp8_tree"):
            call(q, kc, sl, 1.0, 1.0, cu, 8, bt, tree_mask=torch.zeros(2, 8, dtype=torch.int64))
    # the window and the rotary tables, as the 16-bit packed calls refuse them
    fw, fr = pkg.flash_attention_n_kvcache_fp8_varlen_window, pkg.flash_attention_n_kvcache_fp8_varlen_rope
    for bad in (5.0, torch.tensor(5), True, None):
        with pytest.raises(TypeError, match="flash_attention_n_kvcache_fp8_varlen_window: window must be a Python int"):
            fw(q, kc, kc, sl, 1.0, 1.0, cu, 8, bad, block_table=bt)
    with pytest.raises(ValueError, match="flash_attention_n_kvcache_fp8_varlen_window: window must be >= 1"):
        fw(q, kc, kc, sl, 1.0, 1.0, cu, 8, 0, block_table=bt)
    with pytest.raises(TypeError):   # always causal: there is no such argument
        fw(q, kc, kc, sl, 1.0, 1.0, cu, 8, 5, block_table=bt, is_causal=False)
    cos, sin = o["cos"], o["sin"]
    with pytest.raises(ValueError, match="flash_attention_n_kvcache_fp8_varlen_rope: a sliding window is always causal; window=5 needs is_causal=True"):
        fr(q, kc, kc, sl, 1.0, 1.0, cu, 8, cos, sin, block_table=bt, window=5, is_causal=False)
    with pytest.raises(TypeError, match="flash_attention_n_kvcache_fp8_varlen_rope: window must be None or a Python int"):
        fr(q, kc, kc, sl, 1.0, 1.0, cu, 8, cos, sin, block_table=bt, window=5.0)
    with pytest.raises(ValueError, match="flash_attention_n_kvcache_fp8_varlen_rope: the rotary tables cover 127 positions but the cache holds up to 128"):
        fr(q, kc, kc, sl, 1.0, 1.0, cu, 8, cos[:127], sin[:127], block_table=bt)
    with pytest.raises(ValueError, match="flash_attention_n_kvcache_fp8_varlen_rope: rotary_cos must be a"):
        fr(q, kc, kc, sl, 1.0, 1.0, cu, 8, cos[0], sin, block_table=bt)
    with pytest.raises(ValueError, match="flash_attention_n_kvcache_fp8_varlen_rope: rotary_dim = 2 x 4 = 8 is not supported"):
        fr(q, kc, kc, sl, 1.0, 1.0, cu, 8, torch.zeros(128, 4), torch.zeros(128, 4), block_table=bt)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        fr(q, kc, kc, sl, 1.0, 1.0, cu, 8, cos, sin, block_table=bt, window=5, rotary_interleaved=True, k_new=kn, v_new=kn)


def test_the_existing_calls_keep_their_refusals(pkg):
    """flash_attention_n_kvcache_fp8 still refuses cu_seqlens_q, flash_attention_n_kvcache_varlen still takes a 16-bit cache only"""
    o = _tensors()
    with pytest.raises(NotImplementedError, match="no FP8 ALiBi or packed kernels yet"):
        pkg.flash_attention_n_kvcache_fp8(torch.zeros(2, 8, 1, 64, dtype=torch.float16), o["kc"], o["kc"], o["sl"], 1.0, 1.0, block_table=o["bt"],
                                          cu_seqlens_q=o["cu"])
    with pytest.raises(TypeError, match="query, k_cache and v_cache must share one dtype"):
        pkg.flash_attention_n_kvcache_varlen(o["q"], o["kc"], o["kc"], o["sl"], o["cu"], 8, block_table=o["bt"])


# ---------------------------------------------------------------- stand-alone checks
def test_the_spill_allowance_is_unchanged(golden_dir):
    raw = open(os.path.join(golden_dir, "spill_allowance.json"), "rb").read()
    assert hashlib.sha256(raw).hexdigest() == SPILL_ALLOWANCE_SHA256
    assert b"fp8" not in raw and b"kvvarlen" not in raw


SPILL_ALLOWANCE_SHA256 = "a5efcccaa38aad79eac31fe5f8bbd1a50395352602806c4b08fe376e4cb65f5a"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path.insert(0, ROOT)
    import flash_attention_softmax_n_amd
    text = _plan_text(flash_attention_softmax_n_amd)
    with open(PLANS, "w") as fh:
        fh.write("\n".join(text) + "\n")
    print(f"recorded {len(text)} lines in {PLANS}")
