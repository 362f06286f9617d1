"""fasn_varlen_rope / fasn_varlen_rope_plan and flash_attention_n_varlen_rope without a GPU: the order and the codes of the
argument checks, the recorded launch plans (tests/golden/attn_varlen_rope_plans.txt), the grid as a function of the token rows alone, the
token -> (sequence, position) rule and the kernel's lookup in integers, and the interface. Nothing is ever launched: the pointers are fake,
and the launch is only called with blocks it refuses before any HIP call.

    python tests/test_attnvarlenrope_cpu.py --record     rewrites the fixture from the library of this tree
"""
import ctypes
import inspect
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import attn_varlen as av          # noqa: E402
import attn_varlen_rope as avr    # noqa: E402
import test_attnvarlen_cpu as base_cpu   # noqa: E402

PLANS = os.path.join(ROOT, "tests", "golden", "attn_varlen_rope_plans.txt")
OK, EINVAL, EDTYPE, EHEADDIM, EALIGN, ESTRIDE, EUNSUPPORTED = 0, -1, -2, -3, -4, -5, -7
BASE = dict(Tq=700, Tk=520, Hq=8, Hkv=2, D=64)
# the mutants of the base call that name an operand this launch does not touch
NOT_MINE = {"v off 16 bytes", "o token stride 36", "lse NULL"}


def _codes(pkg, f, vl, r, qo, ko, inverse=0):
    """(launch, plan) codes of a call both refuse"""
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    return lib.fasn_varlen_rope(f, vl, r, qo, ko, inverse, None), lib.fasn_varlen_rope_plan(f, vl, r, qo, ko, inverse, buf, len(buf))


class _Shim:
    """the (BwdArgs-like, Varlen) pair the base call's mutants address: .fwd is the block"""
    def __init__(self, f):
        self.fwd = f


def _operand_mutants():
    """name -> (mutation of (KvRope, q_out, k_out), code): the rope operand's rules in the order of the cache's rotary calls"""
    def rope(field, value):
        return lambda r, qo, ko: setattr(r, field, value)
    return {
        "cos NULL": (rope("cos", None), EINVAL),
        "sin NULL": (rope("sin", None), EINVAL),
        "rotary_dim 8": (rope("rotary_dim", 8), EINVAL),
        "rotary_dim 24": (rope("rotary_dim", 24), EINVAL),
        "rotary_dim 80": (rope("rotary_dim", 80), EINVAL),
        "rows < max_seqlen_k": (rope("rows", 299), EINVAL),
        "interleaved 2": (rope("interleaved", 2), EINVAL),
        "table dtype fp16 on bf16": (rope("table_dtype", 0), EDTYPE),
        "row stride < rotary_dim / 2": (rope("row_stride", 24), EINVAL),
        "cos off 16 bytes": (rope("cos", av.DUMMY + 8), EALIGN),
        "row stride 37 x 4 bytes": (rope("row_stride", 37), EALIGN),
        "q_out NULL pointer": (lambda r, qo, ko: setattr(qo, "ptr", None), EINVAL),
        "q_out feature stride 2": (lambda r, qo, ko: qo.stride.__setitem__(3, 2), ESTRIDE),
        "k_out off 16 bytes": (lambda r, qo, ko: setattr(ko, "ptr", av.DUMMY + 4), EALIGN),
        "k_out token stride 36": (lambda r, qo, ko: ko.stride.__setitem__(2, 36), EALIGN),
        "q_out of 2 GiB": (lambda r, qo, ko: qo.stride.__setitem__(2, 1 << 21), EINVAL),
    }


@pytest.mark.parametrize("name", sorted(set(base_cpu._mutants()) - NOT_MINE))
def test_base_refusals_keep_their_codes_in_front_of_the_operand(pkg, name):
    """every rule of the packed call that applies, with its code - also when the rope operand, the outputs and `inverse` are bad too"""
    mutate, code = base_cpu._mutants()[name]
    f, vl, r, qo, ko = avr.fake_call(pkg, **BASE)
    mutate(_Shim(f), vl)
    assert _codes(pkg, f, vl, r, qo, ko) == (code, code), name
    r.rotary_dim, r.table_dtype, qo.ptr = 24, 0, None   # EINVAL, EDTYPE, EINVAL of their own
    assert _codes(pkg, f, vl, None, qo, ko, inverse=7) == (code, code), name
    assert _codes(pkg, f, vl, r, qo, ko, inverse=7) == (code, code), name


@pytest.mark.parametrize("name", sorted(NOT_MINE))
def test_v_o_and_lse_are_not_read(pkg, name):
    mutate, _ = base_cpu._mutants()[name]
    f, vl, r, qo, ko = avr.fake_call(pkg, **BASE)
    f.v.ptr, f.o.ptr, f.lse = av.DUMMY, av.DUMMY, av.DUMMY
    mutate(_Shim(f), vl)
    buf = ctypes.create_string_buffer(4096)
    assert pkg._lib.load().fasn_varlen_rope_plan(f, vl, r, qo, ko, 0, buf, len(buf)) > 0, name


@pytest.mark.parametrize("name", sorted(_operand_mutants()))
def test_operand_refusals_and_their_codes(pkg, name):
    mutate, code = _operand_mutants()[name]
    f, vl, r, qo, ko = avr.fake_call(pkg, **BASE)
    mutate(r, qo, ko)
    assert _codes(pkg, f, vl, r, qo, ko) == (code, code), name
    assert _codes(pkg, f, vl, r, qo, ko, inverse=2) == (code, code), name   # in front of `inverse`


def test_null_operands_inverse_and_the_plan_buffer(pkg):
    lib = pkg._lib.load()
    buf = ctypes.create_string_buffer(4096)
    f, vl, r, qo, ko = avr.fake_call(pkg, **BASE)
    assert _codes(pkg, None, vl, r, qo, ko) == (EINVAL, EINVAL) and _codes(pkg, f, None, r, qo, ko) == (EINVAL, EINVAL)
    assert _codes(pkg, f, vl, None, qo, ko) == (EINVAL, EINVAL)
    assert _codes(pkg, f, vl, r, None, ko) == (EINVAL, EINVAL) and _codes(pkg, f, vl, r, qo, None) == (EINVAL, EINVAL)
    for inverse in (-1, 2, 7):
        assert _codes(pkg, f, vl, r, qo, ko, inverse) == (EINVAL, EINVAL)
    assert lib.fasn_varlen_rope_plan(f, vl, r, qo, ko, 0, None, 0) == EINVAL
    assert lib.fasn_varlen_rope_plan(f, vl, r, qo, ko, 0, buf, 8) == EINVAL   # the text does not fit
    assert lib.fasn_varlen_rope_plan(f, vl, r, qo, ko, 0, buf, len(buf)) > 0 and lib.fasn_varlen_rope_plan(f, vl, r, qo, ko, 1, buf, len(buf)) > 0
    # rows == max_seqlen_k is enough; 16-bit tables of the call's type and in-place outputs are served
    r.rows = vl.max_seqlen_k
    assert lib.fasn_varlen_rope_plan(f, vl, r, qo, ko, 0, buf, len(buf)) > 0
    f, vl, r, qo, ko = avr.fake_call(pkg, table_dtype=torch.bfloat16, in_place=True, **BASE)
    assert lib.fasn_varlen_rope_plan(f, vl, r, qo, ko, 1, buf, len(buf)) > 0


def test_check_order(pkg):
    """the base call's rules, then the rope operand in the cache's order (sizes, table type, alignment), then the outputs, then inverse"""
    f, vl, r, qo, ko = avr.fake_call(pkg, **BASE)
    f.dropout_p = 0.5                 # EUNSUPPORTED (base)
    vl.cu_seqlens_q = av.DUMMY + 2    # EALIGN (base, last)
    r.table_dtype = 0                 # EDTYPE
    r.cos = av.DUMMY + 8              # EALIGN
    ko.stride[3] = 2                  # ESTRIDE
    code = lambda inverse=3: _codes(pkg, f, vl, r, qo, ko, inverse)[0]   # noqa: E731
    assert code() == EUNSUPPORTED
    f.dropout_p = 0.0
    assert code() == EALIGN
    vl.cu_seqlens_q = av.DUMMY
    r.rotary_dim = 24
    assert code() == EINVAL
    r.rotary_dim = 64
    assert code() == EDTYPE
    r.table_dtype = 2
    assert code() == EALIGN
    r.cos = av.DUMMY
    assert code() == ESTRIDE
    ko.stride[3] = 1
    assert code() == EINVAL           # inverse = 3
    buf = ctypes.create_string_buffer(4096)
    assert pkg._lib.load().fasn_varlen_rope_plan(f, vl, r, qo, ko, 1, buf, len(buf)) > 0


# ---------------------------------------------------------------- plans
def _plan(pkg, inverse=0, **kw):
    f, vl, r, qo, ko = avr.fake_call(pkg, **kw)
    return pkg._lib.varlen_rope_plan(f, vl, r, qo, ko, inverse)


def _plan_text(pkg):
    lines = []
    for name, kw in sorted(avr.plan_cases().items()):
        lines += [f"{name} {k} grid={g} block={b} lds={l}" for k, g, b, l in _plan(pkg, **kw)]
    return lines


def test_plans_are_pinned(pkg):
    assert _plan_text(pkg) == open(PLANS).read().splitlines()


def test_plan_is_one_launch_of_the_new_kernel(pkg):
    for name, kw in avr.plan_cases().items():
        plan = _plan(pkg, **kw)
        assert len(plan) == 1 and plan[0][0].split("<")[0] == "fasn_varlen_rope_kernel" and plan[0][2] == 256, name
        assert not any(bad in plan[0][0] for bad in ("kvcache", "kvprefill", "kvvarlen"))


def test_grid_is_a_function_of_the_token_rows_alone(pkg):
    grid = lambda **kw: _plan(pkg, **{**BASE, **kw})[0][1]   # noqa: E731
    tiles = lambda T: -(-T // avr.TOKENS)                    # noqa: E731
    assert grid() == tiles(700) + tiles(520)
    for Tq, Tk in ((1, 1), (16, 16), (17, 15), (4096, 8192), (33, 1000)):
        assert grid(Tq=Tq, Tk=Tk) == tiles(Tq) + tiles(Tk)
    # not of the sequences, the hints, the heads, the operand, the pointers, the layout of the views or the direction
    want = _plan(pkg, **BASE)
    assert _plan(pkg, num_seqs=1, max_q=1, max_k=1, rows=1, **BASE) == want
    assert _plan(pkg, num_seqs=512, max_q=3, rows=3, **BASE) == want
    assert _plan(pkg, **{**BASE, "Hq": 64, "Hkv": 8}) == want
    assert _plan(pkg, rd=16, interleaved=True, rows=4096, **BASE) == want
    assert _plan(pkg, inverse=1, **BASE) == want
    assert _plan(pkg, in_place=True, inverse=1, **BASE) == want
    assert _plan(pkg, base=(av.DUMMY << 8) + 4096, **BASE) == want
    assert _plan(pkg, q_token_stride=(BASE["Hq"] + 2 * BASE["Hkv"]) * 64, **BASE) == want   # q as a slice of a packed QKV buffer
    assert _plan(pkg, dtype=torch.float16, **BASE)[0][1:] == want[0][1:]


# ---------------------------------------------------------------- token -> (sequence, position)
PACKS = {"SEAMS": av.SEAMS, "UNEQUAL": av.UNEQUAL, "MANY": avr.MANY, "MANY empty from 300": avr.MANY_EMPTY, "LONG8": avr.LONG8,
         "LONG8 unequal": avr.LONG8_UNEQUAL, "ONE_LONG": avr.ONE_LONG}


@pytest.mark.parametrize("name", sorted(PACKS))
def test_every_token_has_one_sequence_and_position(name):
    pack = PACKS[name]
    m = avr.token_map(pack)
    for side, cu, lens, T in (("q", pack.cu_q, pack.lens_q, pack.Tq), ("k", pack.cu_k, pack.lens_k, pack.Tk)):
        assert len(m[side]) == T
        assert all((e is not None) == (t < cu[-1]) for t, e in enumerate(m[side]))
        seen = {}
        for t, e in enumerate(m[side]):
            if e is not None:
                b, i, pos = e
                assert cu[b] <= t < cu[b + 1] and i == t - cu[b]
                seen[b] = seen.get(b, 0) + 1
                want = i + (pack.lens_k[b] - pack.lens_q[b]) if side == "q" else i
                assert pos == want
        assert seen == {b: n for b, n in enumerate(lens) if n}
    # clamped at 0 where the table is read: the rows of a sequence with more rows than keys
    pos, valid = avr.positions(pack, pack.max_k, "cpu")["q"]
    assert int(pos.min()) >= 0 and int(pos.max()) <= pack.max_k - 1
    for t, e in enumerate(m["q"]):
        if e is not None:
            assert int(pos[t]) == max(e[2], 0) and bool(valid[t])
    if pack.self_attn:   # every sequence restarts at 0
        assert all(e is None or e[2] == e[1] for e in m["q"])
    else:
        assert name != "UNEQUAL" or any(e is not None and e[2] < 0 for e in m["q"])


@pytest.mark.parametrize("name", sorted(PACKS))
def test_the_kernels_lookup_gives_the_rule(name):
    """the workgroup's two bounded searches and the per-token search between them find the sequence of every token, empty sequences and a
    constant tail of offsets included, and no search reads more than ceil(log2(B + 1)) offsets"""
    pack = PACKS[name]
    m = avr.token_map(pack)
    bound = (pack.B + 1).bit_length()
    for side in ("q", "k"):
        got, worst_uniform, worst_lane = avr.lookup_model(pack, side)
        assert got == m[side], (name, side)
        assert worst_uniform <= 2 * bound and worst_lane <= bound
    if name == "ONE_LONG":   # inside one sequence no token searches at all
        assert avr.lookup_model(pack, "q")[2] == 0


def test_lookup_under_malformed_offsets_stays_inside():
    """decreasing offsets, offsets beyond the rows, a negative one: every token the model assigns lies in its (clamped) sequence"""
    for cu in ([0, 50, 20, 90, 400], [0, -5, 30, 30, 64], [10, 20, 30, 40, 64], [0, 0, 0, 0, 0], [0, 70, 70, 10, 33]):
        pack = av.Pack([16, 16, 16, 16])
        pack.cu_q = pack.cu_k = list(cu)
        pack.Tq = pack.Tk = 64
        for side in ("q", "k"):
            got, _, _ = avr.lookup_model(pack, side)   # (asserts every offset index it reads)
            for t, e in enumerate(got):
                if e is not None:
                    b, i, pos = e
                    assert 0 <= b < 4 and 0 <= t < 64 and i >= 0


# ---------------------------------------------------------------- the eager rotation and its transpose
@pytest.mark.parametrize("rd", [64, 32, 16])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_eager_autograd_is_the_transpose_rotation(dtype, interleaved, rd):
    """what the gradient contract rests on: autograd through rot forms g1 c + g2 s and g2 c - g1 s in fp32 and rounds once - rot with
    the sines negated, bit for bit; rows of no sequence and the features beyond rotary_dim pass their gradient through"""
    pack = av.UNEQUAL
    inp = av.inputs(pack, 2, 64, dtype, 3)
    cos, sin = avr.random_tables(pack.max_k, rd, 7)
    pos, valid = avr.positions(pack, pack.max_k, "cpu")["q"]
    x = inp["q"].clone().requires_grad_()
    y = avr.rot(x, cos, sin, pos, valid, interleaved)
    y.backward(inp["do"])
    want = avr.rot(inp["do"], cos, sin, pos, valid, interleaved, inverse=True)
    assert torch.equal(x.grad[valid], want[valid]) and torch.equal(x.grad[~valid], inp["do"][~valid])
    assert torch.equal(y[..., rd:], inp["q"][..., rd:]) and torch.equal(x.grad[..., rd:], inp["do"][..., rd:])
    assert not torch.equal(y[valid][..., :rd], inp["q"][valid][..., :rd])


# ---------------------------------------------------------------- interface
def test_exports_header_and_bindings_agree(pkg):
    text = open(os.path.join(ROOT, "include", "fasn.h")).read()
    lib = pkg._lib.load()
    for name in ("fasn_varlen_rope", "fasn_varlen_rope_plan"):
        assert name in pkg._lib.EXPORTS and f"int {name}(" in text and hasattr(lib, name)
        assert not any(stem in name for stem in ("kvcache", "kvprefill", "kvvarlen"))
        assert getattr(lib, name).restype is ctypes.c_int32
    assert len(lib.fasn_varlen_rope.argtypes) == 7 and len(lib.fasn_varlen_rope_plan.argtypes) == 8
    assert "#define FASN_ABI_VERSION 6" in text and lib.fasn_abi_version() == 6
    assert "v, o and lse are not touched and may be NULL" in " ".join(text.split())


def test_signature_and_defaults(pkg):
    fn = pkg.flash_attention_n_varlen_rope
    assert "flash_attention_n_varlen_rope" in pkg.__all__ and "flash_attention_n_varlen_rope" in pkg.__doc__
    p = inspect.signature(fn).parameters
    assert list(p) == ["query", "key", "value", "cu_seqlens_q", "max_seqlen_q", "rotary_cos", "rotary_sin", "cu_seqlens_k", "max_seqlen_k",
                       "softmax_n_param", "scale", "is_causal", "return_lse", "window", "rotary_interleaved"]
    defaults = {k: v.default for k, v in p.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(cu_seqlens_k=None, max_seqlen_k=None, softmax_n_param=1, scale=None, is_causal=False, return_lse=False, window=None,
                            rotary_interleaved=False)
    base = inspect.signature(pkg.flash_attention_n_varlen).parameters
    assert list(base) == ["query", "key", "value", "cu_seqlens_q", "max_seqlen_q", "cu_seqlens_k", "max_seqlen_k", "softmax_n_param", "scale",
                          "is_causal", "return_lse", "window"]
    assert {k: v.default for k, v in base.items() if v.default is not inspect.Parameter.empty} == {k: v for k, v in defaults.items()
                                                                                                   if k != "rotary_interleaved"}


def test_front_end_refusals_without_a_device(pkg):
    fa = pkg.flash_attention_n_varlen_rope
    q = torch.zeros(16, 4, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 7, 16], dtype=torch.int32)
    cos, sin = avr.true_tables(16, 64)
    with pytest.raises(RuntimeError, match="CPU tensor"):   # the base call's refusal, with its words
        fa(q, q, q, cu, 9, cos, sin)
    with pytest.raises(TypeError, match="window must be None or a Python int"):
        fa(q, q, q, cu, 9, cos, sin, window=2.0, is_causal=True)
    with pytest.raises(ValueError, match="window needs is_causal=True"):
        fa(q, q, q, cu, 9, cos, sin, window=4)
    with pytest.raises(TypeError):   # the tables are positional: a call in flash_attention_n_varlen's form is not silently taken
        fa(q, q, q, cu, 9)
    for kw in ("attn_mask", "attn_bias", "dropout_p"):
        with pytest.raises(TypeError, match=kw):
            fa(q, q, q, cu, 9, cos, sin, **{kw: None})


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, ROOT)
    import flash_attention_softmax_n_amd as _pkg
    open(PLANS, "w").write("\n".join(_plan_text(_pkg)) + "\n")
    print("recorded", PLANS)
