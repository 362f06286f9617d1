"""fasn_fwd_varlen / fasn_bwd_varlen / fasn_varlen_plan without a GPU: the order and the codes of the argument checks, the recorded launch
plans (tests/golden/attn_varlen_plans.txt), the grid as a function of num_seqs and max_seqlen_* alone, and the front end's refusals that
need no device. Nothing is ever launched: the pointers are fake, and the forward / backward are only called with blocks they refuse
before any HIP call.

    python tests/test_attnvarlen_cpu.py --record     rewrites the fixture from the library of this tree
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import attn_varlen as av   # noqa: E402

PLANS = os.path.join(ROOT, "tests", "golden", "attn_varlen_plans.txt")
OK, EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED = 0, -1, -2, -3, -4, -5, -7
BASE = dict(Tq=700, Tk=520, Hq=8, Hkv=2, D=64)


def _codes(pkg, a, vl, n=None, n_stride=0):
    """(forward, backward, forward plan, backward plan) codes of a block every one of them refuses"""
    import ctypes
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    return (lib.fasn_fwd_varlen(a.fwd if a is not None else None, vl, n, n_stride, None), lib.fasn_bwd_varlen(a, vl, None),
            lib.fasn_varlen_plan(a, vl, 0, buf, len(buf)), lib.fasn_varlen_plan(a, vl, 1, buf, len(buf)))


def _mutants():
    """name -> (mutation of (BwdArgs, Varlen), the code all three entry points answer)"""
    def setter(path, value):
        def m(a, vl):
            obj = {"a": a, "f": a.fwd, "vl": vl}[path[0]]
            for name in path[1:-1]:
                obj = getattr(obj, name)
            if isinstance(path[-1], tuple):
                getattr(obj, path[-1][0])[path[-1][1]] = value
            else:
                setattr(obj, path[-1], value)
        return m
    return {
        "cu_q NULL": (setter(("vl", "cu_seqlens_q"), None), EINVAL),
        "cu_k NULL": (setter(("vl", "cu_seqlens_k"), None), EINVAL),
        "no sequence": (setter(("vl", "num_seqs"), 0), EINVAL),
        "max_seqlen_q 0": (setter(("vl", "max_seqlen_q"), 0), EINVAL),
        "max_seqlen_k 0": (setter(("vl", "max_seqlen_k"), 0), EINVAL),
        "reserved set": (setter(("vl", "reserved"), 1), EINVAL),
        "B = 2": (setter(("f", "B"), 2), EINVAL),
        "no rows": (setter(("f", "Sq"), 0), EINVAL),
        "bad dtype": (setter(("f", "dtype"), 7), EDTYPE),
        "kv_group 3": (setter(("f", "kv_group"), 3), EINVAL),
        "negative scale": (setter(("f", "scale"), -1.0), EINVAL),
        "Dv = 128": (setter(("f", "Dv"), 128), EHEADDIM),
        "fp32": (setter(("f", "dtype"), 2), EUNSUPPORTED),
        "mask": (setter(("f", "mask", "ptr"), av.DUMMY), EUNSUPPORTED),
        "bias": (setter(("f", "bias", "ptr"), av.DUMMY), EUNSUPPORTED),
        "dropout": (setter(("f", "dropout_p"), 0.1), EUNSUPPORTED),
        "q NULL": (setter(("f", "q", "ptr"), None), EINVAL),
        "feature stride 2": (setter(("f", "k", ("stride", 3)), 2), ESTRIDE),
        "v off 16 bytes": (setter(("f", "v", "ptr"), av.DUMMY + 8), EALIGN),
        "o token stride 36": (setter(("f", "o", ("stride", 2)), 36), EALIGN),
        "q of 2 GiB": (setter(("f", "q", ("stride", 2)), 1 << 21), EINVAL),
        "lse NULL": (setter(("f", "lse"), None), EINVAL),
        "cu_q off 4 bytes": (setter(("vl", "cu_seqlens_q"), av.DUMMY + 2), EALIGN),
        "cu_k off 4 bytes": (setter(("vl", "cu_seqlens_k"), av.DUMMY + 1), EALIGN),
    }


@pytest.mark.parametrize("name", sorted(_mutants()))
def test_refusals_and_their_codes(pkg, name):
    mutate, code = _mutants()[name]
    a, vl = av.block(pkg, **BASE)
    mutate(a, vl)
    assert _codes(pkg, a, vl) == (code,) * 4, name


def test_null_blocks_and_backward_only_refusals(pkg):
    import ctypes
    lib = pkg._lib.load()
    a, vl = av.block(pkg, **BASE)
    buf = ctypes.create_string_buffer(4096)
    assert lib.fasn_fwd_varlen(None, vl, None, 0, None) == EINVAL and lib.fasn_fwd_varlen(a.fwd, None, None, 0, None) == EINVAL
    assert lib.fasn_bwd_varlen(None, vl, None) == EINVAL and lib.fasn_bwd_varlen(a, None, None) == EINVAL
    assert lib.fasn_varlen_plan(None, vl, 0, buf, len(buf)) == EINVAL and lib.fasn_varlen_plan(a, None, 0, buf, len(buf)) == EINVAL
    assert lib.fasn_varlen_plan(a, vl, 2, buf, len(buf)) == EINVAL and lib.fasn_varlen_plan(a, vl, 0, None, 0) == EINVAL
    assert lib.fasn_varlen_plan(a, vl, 1, buf, 8) == EINVAL   # the text does not fit
    # n: a pointer off 4 bytes, a negative stride
    assert lib.fasn_fwd_varlen(a.fwd, vl, av.DUMMY + 2, 1, None) == EALIGN and lib.fasn_fwd_varlen(a.fwd, vl, av.DUMMY, -1, None) == EINVAL
    # the backward's own operands, behind the forward block's checks
    for mutate, code in ((lambda b: setattr(b, "delta", None), EINVAL), (lambda b: setattr(b.dbias, "ptr", av.DUMMY), EUNSUPPORTED),
                         (lambda b: setattr(b.dout, "ptr", None), EINVAL), (lambda b: b.dq.stride.__setitem__(3, 2), ESTRIDE),
                         (lambda b: setattr(b.dk, "ptr", av.DUMMY + 4), EALIGN), (lambda b: b.dv.stride.__setitem__(1, 4), EALIGN)):
        b, vl2 = av.block(pkg, **BASE)
        mutate(b)
        assert lib.fasn_bwd_varlen(b, vl2, None) == code and lib.fasn_varlen_plan(b, vl2, 1, buf, len(buf)) == code
        assert lib.fasn_varlen_plan(b, vl2, 0, buf, len(buf)) > 0   # the forward does not read them


def test_check_order(pkg):
    """sizes and enums, then what the build does not serve, then the views, then the alignment of the offsets"""
    a, vl = av.block(pkg, **BASE)
    a.fwd.dropout_p = 0.5
    a.fwd.k.stride[3] = 2
    vl.cu_seqlens_q = av.DUMMY + 2
    assert _codes(pkg, a, vl)[0] == EUNSUPPORTED
    a.fwd.dropout_p = 0.0
    assert _codes(pkg, a, vl)[0] == ESTRIDE
    a.fwd.k.stride[3] = 1
    assert _codes(pkg, a, vl)[0] == EALIGN
    vl.num_seqs = 0
    assert _codes(pkg, a, vl)[0] == EINVAL


@pytest.mark.parametrize("D", av.DIMS)
def test_head_dims_served(pkg, D):
    import ctypes
    a, vl = av.block(pkg, 700, 520, 8, 2, D)
    buf = ctypes.create_string_buffer(4096)
    rc = pkg._lib.load().fasn_varlen_plan(a, vl, 0, buf, len(buf))
    if D == 64:
        assert rc > 0
    else:   # refused, not skipped: FASN_EUNSUPPORTED from all three entry points
        assert _codes(pkg, a, vl) == (EUNSUPPORTED,) * 4
    for D2 in (32, 256):
        a, vl = av.block(pkg, 700, 520, 8, 2, D2)
        assert _codes(pkg, a, vl) == (EUNSUPPORTED,) * 4


def _plan_text(pkg):
    lines = []
    for name, (kw, which) in sorted(av.plan_cases().items()):
        a, vl = av.block(pkg, **kw)
        lines += [f"{name} {k} grid={g} block={b} lds={l}" for k, g, b, l in pkg._lib.varlen_plan(a, vl, which)]
    return lines


def test_plans_are_pinned(pkg):
    assert _plan_text(pkg) == open(PLANS).read().splitlines()


def test_plans_name_only_packed_kernels(pkg):
    """forward: tail + one forward kernel; backward: tail + dQ + dK/dV, no delta launch (the dQ prologue publishes it), every attention kernel
    an instantiation on a *_varlen_tag"""
    for name, (kw, which) in av.plan_cases().items():
        a, vl = av.block(pkg, **kw)
        ks = [k for k, *_ in pkg._lib.varlen_plan(a, vl, which)]
        want = ["fasn_varlen_tail_kernel", "fasn_bwd_dq_kernel", "fasn_bwd_dkdv_kernel"] if which else ["fasn_varlen_tail_kernel", "fasn_fwd_kernel"]
        assert [k.split("<")[0] for k in ks] == want, name
        assert all("_varlen_tag" in k for k in ks[1:]), name
        assert not any(bad in k for k in ks for bad in ("kvcache", "kvprefill", "kvvarlen"))


def test_grid_is_a_function_of_num_seqs_and_max_seqlen(pkg):
    def grids(which, **kw):
        a, vl = av.block(pkg, **{**BASE, **kw})
        return [g for _, g, _, _ in pkg._lib.varlen_plan(a, vl, which)]
    Hq, Hkv = BASE["Hq"], BASE["Hkv"]
    for B, mq, mk in ((1, 1, 1), (3, 128, 128), (3, 129, 128), (5, 300, 64), (7, 64, 1000)):
        nq, nk = -(-mq // 128), -(-mk // 128)
        tail = lambda T: -(-T // 32)   # noqa: E731
        assert grids(0, num_seqs=B, max_q=mq, max_k=mk) == [tail(700), B * Hq * nq]
        assert grids(1, num_seqs=B, max_q=mq, max_k=mk) == [tail(700), B * Hq * nq, B * Hkv * nk]
    # the token rows move the tail kernel's grid alone
    assert grids(1, Tq=4096, Tk=8192, num_seqs=3, max_q=128)[1:] == grids(1, num_seqs=3, max_q=128)[1:]
    assert grids(1, Tq=4096, Tk=8192, num_seqs=3, max_q=128)[0] == 8192 // 32 and grids(0, Tq=4096, Tk=8192, num_seqs=3, max_q=128)[0] == 4096 // 32


def test_plan_text_is_independent_of_the_pointers(pkg):
    for which in (0, 1):
        a, vl = av.block(pkg, causal=True, **BASE)
        b, vl2 = av.block(pkg, causal=True, base=(av.DUMMY << 8) + 4096, q_token_stride=BASE["Hq"] * 64, **BASE)
        assert pkg._lib.varlen_plan(a, vl, which) == pkg._lib.varlen_plan(b, vl2, which)
        c, vl3 = av.block(pkg, causal=True, q_token_stride=(BASE["Hq"] + 2 * BASE["Hkv"]) * 64, **BASE)   # q as a slice of a packed QKV buffer
        assert pkg._lib.varlen_plan(a, vl, which) == pkg._lib.varlen_plan(c, vl3, which)


def test_rectangular_m0_plan_line_unchanged(pkg, golden_dir):
    """flash_attention_n's M0 call reaches the kernels it reached before the packed call existed: its plan lines through fasn_launch_plan
    are the ones of tests/golden/baseline_launch_plans.txt"""
    import ctypes
    from baseline_plans import bwd_args
    lib = pkg._lib.load()
    want = [l for l in open(os.path.join(golden_dir, "baseline_launch_plans.txt")).read().splitlines() if l.startswith("m0 ")]
    assert want
    got = []
    for which, code in (("fwd", pkg._lib.FASN_PLAN_FWD_WS), ("bwd", pkg._lib.FASN_PLAN_BWD)):
        buf = ctypes.create_string_buffer(8192)
        assert lib.fasn_launch_plan(bwd_args(pkg, "m0"), code, buf, len(buf)) > 0
        got += [f"m0 {which} {line}" for line in buf.value.decode().splitlines()]
    assert got == want
    assert not any("varlen" in l for l in got)


def test_front_end_refusals_without_a_device(pkg):
    fa = pkg.flash_attention_n_varlen
    assert "flash_attention_n_varlen" in pkg.__all__
    q = torch.zeros(16, 4, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 7, 16], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        fa(q, q, q, cu, 9)
    for kw in ("attn_mask", "attn_bias", "dropout_p"):
        with pytest.raises(TypeError, match=kw):
            fa(q, q, q, cu, 9, **{kw: None})


def test_exports_and_header_agree(pkg):
    text = open(os.path.join(ROOT, "include", "fasn.h")).read()
    for name in ("fasn_fwd_varlen", "fasn_bwd_varlen", "fasn_varlen_plan"):
        assert name in pkg._lib.EXPORTS and f"int {name}(" in text and hasattr(pkg._lib.load(), name)
    assert "#define FASN_ABI_VERSION 6" in text and pkg._lib.load().fasn_abi_version() == 6


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, ROOT)
    import flash_attention_softmax_n_amd as _pkg
    open(PLANS, "w").write("\n".join(_plan_text(_pkg)) + "\n")
    print("recorded", PLANS)
