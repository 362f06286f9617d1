"""The test of the layout tests (no GPU): tests/attn_layout.py's cases, layouts and checks on integers and fake pointers.

  mutants   the address of element (b, h, i, d) of every tensor, modelled in plain integers from the views' strides (meta tensors: nothing
            is allocated); each mutant - o written with q's strides, dk with dq's head stride under grouped K/V, a head stride taken as
            T * D, a row stride taken as D, a store one row early, dO's row stride taken as o's, a far offset wrapped to 32 bits in bytes and
            in elements - breaks check (a) (the result differs from the contiguous call's: an element lands elsewhere, stays the sentinel,
            or is read from a gap or from another, distinct, problem), check (b) (a gap is written) or the alias sentinel of layout F, in
            every case it touches.
  arena     the far offsets fall in the three ranges; the alias slots are distinct from every used slot.
  dry run   every route and far case with fake pointers: launch_plan succeeds, the blocks carry the views' strides, no plan depends on the
            layout, the plans equal tests/golden/attn_layout_plans.txt, each case reaches the kernels it is named for, and the coverage
            condition: every kernel name of tests/golden/attn_witness_plans.txt is reached by a layout case, every address-forming source
            text by a far case.
  refusals  one alignment step beyond the largest row stride is FASN_EINVAL for K and V in the forward and for Q and dO in the backward
            only; alignment and feature-stride refusals of o, dq, dk, dv, dout, dbias; flash_attn._canon's copy rule on strides alone."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_layout as al    # noqa: E402
import attn_witness as aw   # noqa: E402

EINVAL, EALIGN, ESTRIDE = -1, -4, -5
FIRST = [(name, dts[0]) for name, (_, dts) in al.ROUTES.items()]   # (strides do not depend on the 16-bit type)
SMALL = [(n, d) for n, d in FIRST if n != "d64 QB=2"]              # (the mutant model walks every element: the 8 x 64 grid adds nothing to it)


def _meta(name, dtype, pairing):
    case = al.ROUTES[name][0]
    return case, al.alloc(case, aw.DTYPES[dtype], "meta", pairing)


# ---------------------------------------------------------------- mutants
def _caught(view, store, addr):
    a_ok, b_ok, _ = al.write_model(view, store.numel(), addr)
    return [c for c, ok in (("a", a_ok), ("b", b_ok)) if not ok]


@pytest.mark.parametrize("pairing", ["L1", "L2"])
@pytest.mark.parametrize("name,dtype", SMALL)
def test_the_right_addresses_pass(name, dtype, pairing):
    case, ops = _meta(name, dtype, pairing)
    for x in ("o", "dq", "dk", "dv"):
        v = ops.t[x]
        assert _caught(v, ops.store[x], al.addr_map(v)) == [], x
        assert torch.equal(al.strided_addr(v, v.stride()), al.addr_map(v))


@pytest.mark.parametrize("pairing", ["L1", "L2"])
@pytest.mark.parametrize("name,dtype", SMALL)
def test_output_mutants_break_a_or_b(name, dtype, pairing):
    case, ops = _meta(name, dtype, pairing)
    t, st = ops.t, ops.store
    s = {x: t[x].stride() for x in al.FAR_NAMES}
    # o written with q's strides (and each gradient with its input's)
    for out, src in (("o", "q"), ("dq", "q"), ("dk", "k"), ("dv", "v")):
        assert _caught(t[out], st[out], al.strided_addr(t[out], s[src])), f"{out} with {src}'s strides goes unseen"
    if case.G > 1:   # dk with dq's head stride under grouped K/V
        for out in ("dk", "dv"):
            assert _caught(t[out], st[out], al.strided_addr(t[out], (s[out][0], s["dq"][1], s[out][2]))), out
    touched = {}
    for out in ("o", "dq", "dk", "dv"):
        B, Hx, T, D = t[out].shape
        mutants = {"head stride T * D": (s[out][0], T * D, s[out][2]) if Hx > 1 else None, "row stride D": (s[out][0], s[out][1], D),
                   "batch stride H * T * D": (Hx * T * D, s[out][1], s[out][2]) if B > 1 else None}
        for what, strides in mutants.items():
            if strides is None or strides == tuple(s[out][:3]):   # (a dimension of one element; a layout whose stride happens to be the dense one)
                continue
            touched[what] = touched.get(what, 0) + 1
            assert _caught(t[out], st[out], al.strided_addr(t[out], strides)), f"{out}: {what} goes unseen"
        assert _caught(t[out], st[out], al.strided_addr(t[out], s[out], row_shift=-1)), f"{out}: a store one row early goes unseen"
    assert touched.get("row stride D", 0) >= 3 and touched.get("head stride T * D", 0) >= 3 and (case.B == 1 or touched.get("batch stride H * T * D", 0) >= 3)
    if t["dbias"] is not None:   # the dbias rows taken as dense
        v = t["dbias"]
        addr = al.strided_addr(v, (v.stride(0), v.stride(1), v.shape[3]))
        assert _caught(v, st["dbias"], addr), "dbias: row stride S goes unseen"


@pytest.mark.parametrize("pairing", ["L1", "L2"])
@pytest.mark.parametrize("name,dtype", SMALL)
def test_input_mutants_read_a_gap_or_another_problem(name, dtype, pairing):
    """dO's row stride taken as o's (and q / k / v read with another tensor's strides): some element is read from elsewhere INSIDE the
    storage - a gap (the NaN sentinel: the result is NaN) or another element (every (batch, head) problem is distinct) - so (a) breaks"""
    case, ops = _meta(name, dtype, pairing)
    t, st = ops.t, ops.store
    for x, strides in (("dout", (t["dout"].stride(0), t["dout"].stride(1), t["o"].stride(2))), ("q", t["o"].stride()), ("k", t["v"].stride()),
                       ("v", t["k"].stride()), ("dout", t["q"].stride())):
        right, got = al.addr_map(t[x]), al.strided_addr(t[x], strides)
        wrong = (got != right)
        inside = wrong & (got >= 0) & (got < st[x].numel())
        assert wrong.any() and inside.any(), f"{x} read with strides {strides} goes unseen"


def test_a_wrapped_far_offset_hits_an_alias_slot():
    """layout F in integers: for every tensor of the arena and each way an offset can lose its upper bits - the byte offset mod 2^32, mod
    2^31, the element offset mod 2^31 - some far element's wrapped address differs from the right one and lies in an alias slot, which
    holds the sentinel: a wrapped store breaks the alias check (b), a wrapped load reads NaN and breaks (a)"""
    for esize in (2, 4):
        for j in range(len(al.FAR_NAMES)):
            used, alias = al.far_offsets(j, esize)
            base = used[0]
            wraps = {"bytes mod 2^32": lambda o: o % (1 << 32), "bytes mod 2^31": lambda o: o % (1 << 31)}
            if esize == 2:
                wraps["elements mod 2^31"] = lambda o: ((o // esize) % (1 << 31)) * esize
            for how, wrap in wraps.items():
                hit = [base + wrap(u - base) for u in used if wrap(u - base) != u - base]
                assert hit, (how, j)
                assert all(h in alias for h in hit), (how, j, hit, alias)


def test_far_arena_offsets():
    """element 0 below 2^31 bytes, element 1 in [2^31, 2^32), element 2 beyond 2^32 bytes and (16-bit) beyond 2^31 elements of the tensor's
    own base; alias slots distinct from used slots; everything inside the arena and inside the five regions the GPU test refills"""
    slots = []
    for j in range(len(al.FAR_NAMES)):
        used, alias = al.far_offsets(j)
        assert used[0] + al.FAR_SLOT <= 1 << 31 <= used[1] and used[1] + al.FAR_SLOT <= 1 << 32 <= used[2]
        assert (used[2] - used[0]) // 2 >= 1 << 31 and used[2] + al.FAR_SLOT <= al.FAR_BYTES
        assert len(alias) == 2 and al.FAR_STRIDE % 16 == 0
        slots += [(u, "used") for u in used] + [(a, "alias") for a in alias]
        for off, reg in zip(used + alias, al.FAR_USED + al.FAR_ALIAS):
            assert reg <= off and off + al.FAR_SLOT <= reg + len(al.FAR_NAMES) * al.FAR_SLOT
    slots.sort()
    for (a, _), (b, _) in zip(slots, slots[1:]):
        assert a + al.FAR_SLOT <= b, "two slots of the arena overlap"
    assert al.FAR_BYTES < 9 << 29


# ---------------------------------------------------------------- dry run
def test_plans_match_the_golden_file(pkg, golden_dir):
    """(plans_file_text itself asserts that L1, L2 and the contiguous twin plan alike: no route's plan depends on a stride)"""
    with open(os.path.join(golden_dir, "attn_layout_plans.txt")) as fh:
        assert al.plans_file_text(pkg) == fh.read(), "the launch plans of attn_layout.ROUTES changed: tests/golden/attn_layout_plans.txt"


def _plan_names(text):
    return set(re.findall(r"\b(fasn_\w+_kernel)\b", text))


@pytest.mark.parametrize("pairing", ["L1", "L2", "C"])
@pytest.mark.parametrize("name,dtype", al.route_params())
def test_dry_run_of_every_route(pkg, name, dtype, pairing):
    case, dt = al.ROUTES[name][0], aw.DTYPES[dtype]
    ops = al.alloc(case, dt, "meta", pairing)
    a = al.block(pkg, case, ops, 1.0 / math.sqrt(case.D), dt)
    assert al.block_carries(a, ops)
    fw, bw = al.plans(pkg, a)
    assert fw and bw
    text = " ".join(al.described(pkg, a))
    for want in case.want:
        assert want in text, f"{name}: the plan does not hold {want}: {text}"
    assert case.ub == case.B and case.uh == case.H, "every (batch, head) problem is distinct"
    if pairing != "C":
        for x in al.FAR_NAMES:
            assert not ops.t[x].is_contiguous()


def test_coverage_condition(pkg, golden_dir):
    with open(os.path.join(golden_dir, "attn_witness_plans.txt")) as fh:
        witness = _plan_names(fh.read())
    with open(os.path.join(golden_dir, "attn_layout_plans.txt")) as fh:
        text = fh.read()
    assert witness == {
        "fasn_fwd_kernel", "fasn_fwd_ws256_kernel", "fasn_fwd_combine_kernel", "fasn_f32_fwd_kernel", "fasn_bwd_delta_kernel", "fasn_bwd_dq_kernel",
        "fasn_bwd_dkdv_kernel", "fasn_bwd_dq_pipe_kernel", "fasn_bwd_dkdv_pipe_kernel", "fasn_bwd_dq_ws_kernel", "fasn_bwd_dkdv_ws_kernel",
        "fasn_bwd_dq_ws256_kernel", "fasn_bwd_dkdv_ws256_kernel", "fasn_bwd_dbias_kernel", "fasn_bwd_dbias_ws_kernel", "fasn_f32_delta_kernel",
        "fasn_f32_dq_kernel", "fasn_f32_dkdv_kernel"}
    assert witness <= _plan_names(text), f"kernels no layout case reaches: {sorted(witness - _plan_names(text))}"
    for also in ("element-load", "GQA=1", "keypad", "DROP=1", "D=64,QB=2", "SPLIT=1"):
        assert also in text, also
    # fasn_fwd_n and fasn_bwd_dn run in every case whose n is a tensor; fasn_fwd / fasn_fwd_ws in the float case and the split cases
    assert sum(al.n_shape(c) is not None for c, _ in al.ROUTES.values()) >= 10 and any(c.nshape == "float" for c, _ in al.ROUTES.values())
    assert {c.nshape for c, _ in al.ROUTES.values()} >= {"H", "BH", "B1", "float"}
    assert {"fp16", "bf16", "fp32"} <= {d for _, dts in al.ROUTES.values() for d in dts}


SOURCE_OF = {
    "fasn_fwd_kernel": "fasn_fwd_kernel.h", "fasn_fwd_ws256_kernel": "fasn_fwd_ws256.h", "fasn_fwd_combine_kernel": "split-K combine",
    "fasn_f32_fwd_kernel": "fasn_f32_kernels.h", "fasn_f32_delta_kernel": "fasn_f32_kernels.h", "fasn_f32_dq_kernel": "fasn_f32_kernels.h",
    "fasn_f32_dkdv_kernel": "fasn_f32_kernels.h", "fasn_bwd_delta_kernel": "fasn_bwd_kernel.h", "fasn_bwd_dq_kernel": "fasn_bwd_kernel.h",
    "fasn_bwd_dkdv_kernel": "fasn_bwd_kernel.h", "fasn_bwd_dq_pipe_kernel": "fasn_bwd_pipe.h", "fasn_bwd_dkdv_pipe_kernel": "fasn_bwd_pipe.h",
    "fasn_bwd_dq_ws_kernel": "fasn_bwd_dq_ws.h", "fasn_bwd_dkdv_ws_kernel": "fasn_bwd_dkdv_ws.h", "fasn_bwd_dq_ws256_kernel": "fasn_bwd_ws256.h",
    "fasn_bwd_dkdv_ws256_kernel": "fasn_bwd_ws256.h", "fasn_bwd_dbias_kernel": "fasn_bwd_dbias.h", "fasn_bwd_dbias_ws_kernel": "fasn_bwd_dbias_ws.h",
}


def test_far_cases_reach_every_address_forming_source_text(pkg):
    arena = torch.empty(al.FAR_BYTES // 2, dtype=torch.int16, device="meta")
    reached, far_kv_heads = set(), 0
    for name, (case, dtype, dim) in al.FAR.items():
        dt = aw.DTYPES[dtype]
        ops, far = al.far_ops(case, dt, arena, dim)
        a = al.block(pkg, case, ops, 1.0 / math.sqrt(case.D), dt)
        assert al.block_carries(a, ops), name
        names = al.described(pkg, a)
        for want in case.want:
            assert want in " ".join(names), (name, want, names)
        reached |= {SOURCE_OF[k.split("<")[0]] for k in names}
        esize = ops.t["k"].element_size()
        for x in far:
            assert ops.t[x].stride(dim) * esize == al.FAR_STRIDE and ops.t[x].shape[dim] == 3
        if dim == 1:
            assert case.G > 1 and far == ["k", "v", "dk", "dv"]
            far_kv_heads += 1
        # the plan is that of the contiguous twin
        twin = al.block(pkg, case, al.alloc(case, dt, "meta", "C"), 1.0 / math.sqrt(case.D), dt)
        assert al.plans(pkg, a) == al.plans(pkg, twin), name
    assert reached == set(SOURCE_OF.values()), sorted(set(SOURCE_OF.values()) - reached)
    assert far_kv_heads >= 1


# ---------------------------------------------------------------- refusal codes
def _rc(pkg, a, which):
    buf = ctypes.create_string_buffer(1 << 13)
    return pkg._lib.load().fasn_launch_plan(a, which, buf, len(buf))


def _wide_block(pkg, D, over):
    """the block of the largest-stride case with q, k, v, dout at max_row_stride (+ 8 for the names in `over`)"""
    case = aw.Case(1, 2, 65, 65, D)
    ops = al.alloc(case, torch.bfloat16, "meta", "L1")
    a = al.block(pkg, case, ops, 0.125, torch.bfloat16)
    s = al.max_row_stride(65, D)
    for name, v in (("q", a.fwd.q), ("k", a.fwd.k), ("v", a.fwd.v), ("dout", a.dout)):
        v.stride[1], v.stride[2] = 1 << 20, s + (8 if name in over else 0)
    return a


@pytest.mark.parametrize("D", [64, 128])
def test_one_step_beyond_the_largest_row_stride(pkg, D):
    Lb = pkg._lib
    s = al.max_row_stride(65, D)
    assert (64 * s + D) * 2 < 2 ** 31 <= (64 * (s + 8) + D) * 2
    a = _wide_block(pkg, D, ())
    assert _rc(pkg, a, Lb.FASN_PLAN_FWD) > 0 and _rc(pkg, a, Lb.FASN_PLAN_BWD) > 0
    for name in ("k", "v"):   # refused by the forward (and with it by everything else)
        a = _wide_block(pkg, D, (name,))
        assert _rc(pkg, a, Lb.FASN_PLAN_FWD) == EINVAL and _rc(pkg, a, Lb.FASN_PLAN_FWD_WS) == EINVAL and _rc(pkg, a, Lb.FASN_PLAN_BWD) == EINVAL, name
    for name in ("q", "dout"):   # the forward has no such bound; the backward refuses
        a = _wide_block(pkg, D, (name,))
        assert _rc(pkg, a, Lb.FASN_PLAN_FWD) > 0 and _rc(pkg, a, Lb.FASN_PLAN_BWD) == EINVAL, name


def test_alignment_and_feature_stride_refusals_of_the_outputs(pkg):
    Lb = pkg._lib
    case = al.ROUTES["d64 dense dbias causal"][0]
    dt = torch.bfloat16

    def fresh():
        return al.block(pkg, case, al.alloc(case, dt, "meta", "L1"), 0.125, dt)

    assert _rc(pkg, fresh(), Lb.FASN_PLAN_BWD) > 0
    for name in ("o", "dq", "dk", "dv", "dout", "dbias"):
        which = Lb.FASN_PLAN_FWD if name == "o" else Lb.FASN_PLAN_BWD
        pick = (lambda a: a.fwd.o) if name == "o" else (lambda a, name=name: getattr(a, name))
        a = fresh()
        pick(a).stride[3] = 2
        assert _rc(pkg, a, which) == ESTRIDE, name
        a = fresh()
        pick(a).ptr += 1 if name == "dbias" else 8   # (dbias: element alignment - a dbias off 16 bytes only leaves the vector stores)
        assert _rc(pkg, a, which) == EALIGN, name
        if name != "dbias":
            for i in range(3):
                a = fresh()
                pick(a).stride[i] += 4
                assert _rc(pkg, a, which) == EALIGN, (name, i)
    a = fresh()
    a.fwd.bias.ptr = None   # a dbias without a bias: nothing to differentiate
    assert _rc(pkg, a, Lb.FASN_PLAN_BWD) == EINVAL


# ---------------------------------------------------------------- the copy rule of the Python layer, on strides alone
def test_canon_copies_what_the_abi_would_refuse():
    from flash_attention_softmax_n_amd import flash_attn as fa
    bf = torch.bfloat16
    s = al.max_row_stride(65, 64)

    def strided(rows, row_stride, dtype=bf, D=64):
        return torch.empty_strided((1, 2, rows, D), (0, 1 << 20, row_stride, 1), dtype=dtype, device="meta")

    at, over = strided(65, s), strided(65, s + 8)
    assert fa._span_ok(at) and fa._canon(at) is at
    assert fa._rows_ok(over) and not fa._span_ok(over)
    c = fa._canon(over)
    assert c is not over and c.is_contiguous() and c.shape == over.shape
    # fp32 counts 4-byte elements; one row has no span to speak of; a stride-0 row (an expanded gradient) is one row
    assert fa._span_ok(strided(65, al.max_row_stride(65, 64, 4), torch.float32)) and not fa._span_ok(strided(65, al.max_row_stride(65, 64, 4) + 4, torch.float32))
    assert fa._span_ok(strided(1, 1 << 40)) and fa._span_ok(strided(1 << 20, 0))
    # a packed [B, L, 3, H, D] buffer: legal until the context makes one head's rows span 2 GiB
    H, D = 32, 128
    for L, ok in ((1 << 16, True), (1 << 17, False)):
        qkv = torch.empty((1, L, 3, H, D), dtype=bf, device="meta")
        q = qkv[:, :, 0].permute(0, 2, 1, 3)
        assert fa._rows_ok(q) and fa._span_ok(q) == ok and (fa._canon(q) is q) == ok
    # the alignment rule as before
    odd = torch.empty_strided((1, 2, 65, 64), (2 * 65 * 68, 65 * 68, 68, 1), dtype=bf, device="meta")
    assert not fa._rows_ok(odd) and fa._canon(odd).is_contiguous()
