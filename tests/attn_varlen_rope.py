"""What the tests of flash_attention_n_varlen_rope share (tests/test_attnvarlenrope_cpu.py, tests/test_gpu_attnvarlenrope.py).
A plain module: no tests, importable without a GPU. It builds on tests/attn_varlen.py (packs, operands, gates, the C ABI blocks) and
tests/attn_varlen_witness.py (the long packs) and adds no tolerance.

  rot           the rotation, eager: operands and tables widened to fp32, every product and the sum / difference an op of its own (no
                contraction), one rounding to the operand type; under autograd its backward is the transpose rotation in fp32, rounded
                once. inverse=True negates the sines (the transpose, as a forward).
  token_map     the rule in integers: token t of a side belongs to the one sequence b with cu[b] <= t < cu[b + 1]; key j sits at j,
                query i at i + sk_b - sq_b. lookup_model is the KERNEL's way to the same answer, in integers: 16-token workgroups, two
                bounded searches per workgroup, one per token between their results (csrc/fasn_varlen_rope.hip).
  tables        true cos / sin tables - for the bit contract - and random tables in [-1, 1] - for everything judged under a tolerance:
                rotary attention depends on p - j alone, so with true tables a kernel that took the global token index for the position
                would pass any tolerance on a self-attention pack; with random tables a wrong row is a gross error.
  eager_route / fused_route   positions from token_map, rot with torch ops under autograd, flash_attention_n_varlen - against the one call
  run_abi       fasn_varlen_rope on caller-allocated outputs
  plan_cases    tests/golden/attn_varlen_rope_plans.txt"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_varlen as av            # noqa: E402
import attn_varlen_witness as avw   # noqa: E402

D = 64
TOKENS = 16       # tokens of a workgroup (kRopeTokens in csrc/fasn_varlen_rope.hip)
MANY = avw.many().pack
MANY_EMPTY = avw.many(empty_from=300).pack   # the offsets stay constant from sequence 300 on
LONG8 = avw.long8().pack
LONG8_UNEQUAL = avw.long8(unequal=True).pack
ONE_LONG = av.Pack([1100], tail_q=5)         # one sequence of LONG8's longest length: 69 workgroups inside one sequence


# ---------------------------------------------------------------- the rotation, eager
def rot(x, cos, sin, pos, valid, interleaved=False, inverse=False):
    """x [T, heads, E] in its dtype -> the rotation of row t at table row pos[t] (a LongTensor inside the tables) where valid[t], x's row
    itself elsewhere. cos / sin [rows, rotary_dim / 2]. Differentiable in x."""
    rd = 2 * cos.shape[1]
    xf = x.float()
    c, s = cos[pos].float().unsqueeze(1), sin[pos].float().unsqueeze(1)
    if inverse:
        s = -s
    if interleaved:
        x1, x2 = xf[..., 0:rd:2], xf[..., 1:rd:2]
    else:
        x1, x2 = xf[..., :rd // 2], xf[..., rd // 2:rd]
    ac, bs, bc, as_ = x1 * c, x2 * s, x2 * c, x1 * s
    y1, y2 = ac - bs, bc + as_
    y = torch.stack((y1, y2), dim=-1).flatten(-2) if interleaved else torch.cat((y1, y2), dim=-1)
    out = torch.cat((y, xf[..., rd:]), dim=-1).to(x.dtype)
    return torch.where(valid.view(-1, 1, 1), out, x)


# ---------------------------------------------------------------- token -> (sequence, position), in integers
def token_map(pack):
    """{"q": [...], "k": [...]}: per token row of the side (b, i, position) or None for a token of no sequence. position: j for key j,
    i + sk_b - sq_b for query i (not clamped)."""
    out = {"q": [None] * pack.Tq, "k": [None] * pack.Tk}
    for b in range(pack.B):
        q0, q1, k0, k1 = pack.cu_q[b], pack.cu_q[b + 1], pack.cu_k[b], pack.cu_k[b + 1]
        for t in range(q0, q1):
            assert out["q"][t] is None
            out["q"][t] = (b, t - q0, t - q0 + (k1 - k0) - (q1 - q0))
        for t in range(k0, k1):
            assert out["k"][t] is None
            out["k"][t] = (b, t - k0, t - k0)
    return out


def _beyond(cu, t, lo, hi, steps):
    """the kernel's search: the first index in [lo, hi] whose offset lies beyond t; steps[0] counts the loads"""
    while lo < hi:
        mid = (lo + hi) >> 1
        assert 0 <= mid < len(cu) - 1
        steps[0] += 1
        if cu[mid] <= t:
            lo = mid + 1
        else:
            hi = mid
    return lo


def lookup_model(pack, side):
    """csrc/fasn_varlen_rope.hip in integers for one side: ([per token (b, i, position) or None], the largest number of offsets one
    workgroup's uniform searches read, the largest number one token's own search reads)"""
    cu, T = (pack.cu_q, pack.Tq) if side == "q" else (pack.cu_k, pack.Tk)
    other, To = (pack.cu_k, pack.Tk) if side == "q" else (pack.cu_q, pack.Tq)
    clamp = lambda x, lo, hi: min(max(x, lo), hi)   # noqa: E731
    nseq = pack.B
    out = [None] * T
    worst_uniform = worst_lane = 0
    for t0 in range(0, T, TOKENS):
        end = clamp(cu[nseq], 0, T)
        if t0 >= end:
            continue
        ntok = min(TOKENS, end - t0)
        steps = [0]
        i0 = _beyond(cu, t0, 0, nseq, steps)
        i1 = _beyond(cu, t0 + ntok - 1, i0, nseq, steps)
        worst_uniform = max(worst_uniform, steps[0])
        for t in range(t0, t0 + ntok):
            steps = [0]
            b = _beyond(cu, t, i0, i1, steps) - 1
            worst_lane = max(worst_lane, steps[0])
            if b < 0:
                continue
            s0 = clamp(cu[b], 0, T)
            s1 = clamp(max(cu[b + 1], s0), 0, T)
            if not s0 <= t < s1:
                continue
            pos = t - s0
            if side == "q":
                k0 = clamp(other[b], 0, To)
                k1 = clamp(max(other[b + 1], k0), 0, To)
                pos += (k1 - k0) - (s1 - s0)
            out[t] = (b, t - s0, pos)
    return out, worst_uniform, worst_lane


def positions(pack, rows, dev):
    """per side (pos LongTensor [T] clamped into [0, rows - 1], valid BoolTensor [T]) on dev, from token_map"""
    out = {}
    for side, m in token_map(pack).items():
        pos = torch.tensor([0 if e is None else min(max(e[2], 0), rows - 1) for e in m], dtype=torch.long)
        valid = torch.tensor([e is not None for e in m], dtype=torch.bool)
        out[side] = (pos.to(dev), valid.to(dev))
    return out


# ---------------------------------------------------------------- tables
def true_tables(rows, rd, dtype=torch.float32, dev="cpu", base=10000.0):
    """cos / sin [rows, rd / 2] of the usual frequencies base^(-2 d / rd), computed in fp64 and rounded to dtype"""
    inv = base ** (-torch.arange(0, rd, 2, dtype=torch.float64) / rd)
    ang = torch.arange(rows, dtype=torch.float64).unsqueeze(1) * inv
    return ang.cos().to(dtype).to(dev), ang.sin().to(dtype).to(dev)


def random_tables(rows, rd, seed, dtype=torch.float32, dev="cpu"):
    """independent uniform values in [-1, 1]: no two rows alike, no relation between rows"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda: (2.0 * torch.rand(rows, rd // 2, generator=g) - 1.0).to(dtype).to(dev)   # noqa: E731
    return mk(), mk()


# ---------------------------------------------------------------- the two routes
def _kw(pack, cu_k, n, causal, window, scale):
    return dict(cu_seqlens_k=None if pack.self_attn else cu_k, max_seqlen_k=pack.max_k, softmax_n_param=n, scale=scale, is_causal=causal,
                return_lse=True, window=window)


def _grads(out, lse, do, q, k, v, n):
    out.backward(do)
    torch.cuda.synchronize()
    return dict(out=out.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dn=n.grad if torch.is_tensor(n) else None)


def _leaves(ops, n):
    q, k, v = (ops[x].detach().requires_grad_() for x in ("q", "k", "v"))
    n = n.detach().clone().requires_grad_() if torch.is_tensor(n) else n
    return q, k, v, n


def eager_route(pkg, pack, ops, cos, sin, n=1.0, causal=False, window=None, interleaved=False, scale=None, cu=None):
    """positions from the integer model, rot with torch ops under autograd, then flash_attention_n_varlen. ops: q, k, v, do on the
    device (views of one buffer allowed). Returns out, lse, dq, dk, dv, dn."""
    dev = ops["q"].device
    cu_q, cu_k = pack.cu(dev) if cu is None else cu
    q, k, v, n = _leaves(ops, n)
    where = positions(pack, cos.shape[0], dev)
    qr, kr = rot(q, cos, sin, *where["q"], interleaved), rot(k, cos, sin, *where["k"], interleaved)
    out, lse = pkg.flash_attention_n_varlen(qr, kr, v, cu_q, pack.max_q, **_kw(pack, cu_k, n, causal, window, scale))
    return _grads(out, lse, ops["do"], q, k, v, n)


def fused_route(pkg, pack, ops, cos, sin, n=1.0, causal=False, window=None, interleaved=False, scale=None, cu=None):
    """the same through flash_attention_n_varlen_rope"""
    dev = ops["q"].device
    cu_q, cu_k = pack.cu(dev) if cu is None else cu
    q, k, v, n = _leaves(ops, n)
    out, lse = pkg.flash_attention_n_varlen_rope(q, k, v, cu_q, pack.max_q, cos, sin, rotary_interleaved=interleaved,
                                                 **_kw(pack, cu_k, n, causal, window, scale))
    return _grads(out, lse, ops["do"], q, k, v, n)


def same_bits(a, b, what):
    for key in ("out", "lse", "dq", "dk", "dv", "dn"):
        if a[key] is None and b[key] is None:
            continue
        assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), f"{what}: {key} differs"


# ---------------------------------------------------------------- the C ABI
def rope_block(pkg, cos, sin, dtype, interleaved=False, ptrs=None, rows=None, rd=None, row_stride=None, table_dtype=None):
    """the KvRope of two tables - or, with ptrs = (cos, sin) addresses, rows and rd, of fake ones (table_dtype: a torch dtype)"""
    L = pkg._lib
    r = L.KvRope()
    if ptrs is None:
        r.cos, r.sin = cos.data_ptr(), sin.data_ptr()
        rows, rd, row_stride, table_dtype = cos.shape[0], 2 * cos.shape[1], cos.stride(0), cos.dtype
    else:
        r.cos, r.sin = ptrs
        row_stride = rd // 2 if row_stride is None else row_stride
    r.row_stride, r.rows, r.rotary_dim = row_stride, rows, rd
    codes = {torch.float16: L.FASN_DTYPE_F16, torch.bfloat16: L.FASN_DTYPE_BF16, torch.float32: L.FASN_DTYPE_F32}
    r.table_dtype = codes[table_dtype]
    r.interleaved = 1 if interleaved else 0
    return r


def fwd_block(pkg, q, k):
    """the FwdArgs of fasn_varlen_rope over device tensors q [Tq, H, D] and k [Tk, Hkv, D]: v, o and lse NULL"""
    L = pkg._lib
    f = L.FwdArgs()
    f.q, f.k = av.view_packed(pkg, q), av.view_packed(pkg, k)
    f.v.ptr = f.o.ptr = f.lse = None
    f.mask.ptr = f.bias.ptr = None
    f.bias_dtype = 0
    f.dtype = L.FASN_DTYPE_F16 if q.dtype == torch.float16 else L.FASN_DTYPE_BF16
    f.B, f.H, f.Sq, f.Sk, f.D, f.Dv = 1, q.shape[1], q.shape[0], k.shape[0], q.shape[2], q.shape[2]
    f.scale, f.softmax_n, f.causal, f.dropout_p = 1.0 / math.sqrt(q.shape[2]), 1.0, 0, 0.0
    f.seed = f.offset = 0
    f.kv_group = q.shape[1] // k.shape[1] if k.shape[1] != q.shape[1] else 0
    f.rng_state = None
    return f


def run_abi(pkg, pack, q, k, q_out, k_out, cos, sin, cu_q, cu_k, interleaved=False, inverse=0):
    """fasn_varlen_rope over device tensors; returns its code"""
    L = pkg._lib
    vl = L.Varlen()
    vl.cu_seqlens_q, vl.cu_seqlens_k = cu_q.data_ptr(), cu_k.data_ptr()
    vl.num_seqs, vl.max_seqlen_q, vl.max_seqlen_k, vl.reserved = pack.B, pack.max_q, pack.max_k, 0
    stream = torch.cuda.current_stream(q.device).cuda_stream
    with torch.cuda.device(q.device):
        rc = L.load().fasn_varlen_rope(fwd_block(pkg, q, k), vl, rope_block(pkg, cos, sin, q.dtype, interleaved), av.view_packed(pkg, q_out),
                                       av.view_packed(pkg, k_out), inverse, stream)
    torch.cuda.synchronize(q.device)
    return rc


# ---------------------------------------------------------------- named plan cases (tests/golden/attn_varlen_rope_plans.txt)
def fake_call(pkg, rows=300, rd=64, table_dtype=torch.float32, interleaved=False, base=av.DUMMY, in_place=False, **kw):
    """(FwdArgs, Varlen, KvRope, q_out, k_out) over FAKE pointers, for the plans and the refusals: av.block's block with v, o and lse
    NULL, tables at base + 32 MiB .., outputs of the sources' layout at addresses of their own (in_place: the sources themselves)"""
    a, vl = av.block(pkg, base=base, **kw)
    f = a.fwd
    f.v.ptr = f.o.ptr = f.lse = None
    r = rope_block(pkg, None, None, None, interleaved, ptrs=(base + (40 << 24), base + (41 << 24)), rows=rows, rd=rd, table_dtype=table_dtype)
    L = pkg._lib
    outs = []
    for i, src in enumerate((f.q, f.k)):
        v = L.View4()
        v.ptr = src.ptr if in_place else base + ((42 + i) << 24)
        for j in range(4):
            v.stride[j] = src.stride[j]
        outs.append(v)
    return f, vl, r, outs[0], outs[1]


def plan_cases():
    """name -> the keyword arguments of fake_call"""
    big = dict(Tq=2100, Tk=2100, Hq=8, D=64, num_seqs=14, max_q=300)
    return {
        "bf16_mha_rd64": dict(Hkv=8, **big),
        "bf16_gqa4_rd32_interleaved": dict(Hkv=2, rd=32, interleaved=True, **big),
        "bf16_gqa4_rd16_tables16": dict(Hkv=2, rd=16, table_dtype=torch.bfloat16, **big),
        "f16_unequal": dict(Tq=700, Tk=520, Hq=4, Hkv=4, D=64, dtype=torch.float16, num_seqs=6, max_q=257, max_k=200, rows=200),
        "one_token": dict(Tq=1, Tk=1, Hq=1, Hkv=1, D=64, num_seqs=1, max_q=1, rows=1),
    }
