"""What the tests of flash_attention_n_varlen share (tests/test_gpu_attnvarlen.py, tests/test_attnvarlen_cpu.py): the pack builder, the
per-sequence reference, the gates, the C ABI runner and the named cases. A plain module: no tests, importable without a GPU.

  Pack        the lengths of the sequences of both sides, the offset tables and the token rows (offsets' end + a tail nobody owns)
  SEAMS       one pack whose lengths straddle every tile edge of the launched kernels (64-key tiles, the 128-row work items - and the 256
              of two of them -, the 32-row wave blocks), shuffled so that most sequences start at a token offset that is no multiple of 32
  UNEQUAL     cu_seqlens_k != cu_seqlens_q: short against long both ways, an empty side each way, 257 against 64
  reference   oracle.ref_attention.ref_attention_n in fp32 on the CPU, sequence by sequence, with autograd for dq, dk, dv and dn; lse by
              its definition log(n + sum_j exp x_ij). Computed once per (pack, operands, n, causal) and shared.
  check       the two gates of tests/test_gpu_parity.py::_check, restated
  run_abi     forward and backward through fasn_fwd_varlen / fasn_bwd_varlen on caller-allocated outputs (the Python front end allocates
              its own, which is why the tail and gap checks bypass it)
  block       the BwdArgs + Varlen of a call over fake aligned pointers, for the CPU suite (nothing is launched there)"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.ref_attention import ref_attention_n   # noqa: E402

REF_ATOL = {torch.float16: 1e-2, torch.bfloat16: 5e-2}         # reference GPU test tolerances (rtol 0)
REL_TRUE = {torch.float16: 2.0 ** -9, torch.bfloat16: 2.0 ** -6}   # vs the fp32 oracle, relative to the tensor's max |x|
DIMS = (64, 128)      # the head dims the tests are parametrised over
H = 4
DUMMY = 1 << 20       # a fake 16-byte aligned address


def check(got, want, dtype, what):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - want).abs().max().item() if got.numel() else 0.0
    top = want.abs().max().item() if want.numel() else 0.0
    print(f"{what}: max-abs error {err:.3e}, max |want| {top:.3e}")
    atol = REF_ATOL[dtype] * max(1.0, top)
    assert err <= atol, f"{what}: max-abs {err:.3e} > reference atol {atol:.3e}"
    lim = REL_TRUE[dtype] * max(top, 1e-2)
    assert err <= lim, f"{what}: max-abs {err:.3e} > {lim:.3e} (relative gate)"


def check_lse(got, want, dtype, what):
    """lse rows: -inf exactly where the reference has -inf, the gates on the rest"""
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    hidden = torch.isinf(want) & (want < 0)
    assert torch.equal(torch.isinf(got) & (got < 0), hidden), f"{what}: -inf rows differ"
    check(got[~hidden], want[~hidden], dtype, what)


class Pack:
    def __init__(self, lens_q, lens_k=None, tail_q=0, tail_k=None):
        self.lens_q = list(lens_q)
        self.lens_k = list(lens_q if lens_k is None else lens_k)
        assert len(self.lens_q) == len(self.lens_k)
        self.B = len(self.lens_q)
        self.cu_q = [0]
        self.cu_k = [0]
        for a, b in zip(self.lens_q, self.lens_k):
            self.cu_q.append(self.cu_q[-1] + a)
            self.cu_k.append(self.cu_k[-1] + b)
        self.Tq = self.cu_q[-1] + tail_q
        self.Tk = self.cu_k[-1] + (tail_q if tail_k is None else tail_k)
        self.max_q = max(max(self.lens_q), 1)
        self.max_k = max(max(self.lens_k), 1)
        self.self_attn = lens_k is None

    def cu(self, dev):
        """(cu_seqlens_q, cu_seqlens_k) on dev; the same tensor for a self-attention pack"""
        q = torch.tensor(self.cu_q, dtype=torch.int32, device=dev)
        return (q, q) if self.self_attn else (q, torch.tensor(self.cu_k, dtype=torch.int32, device=dev))


SEAM_LENS = [129, 1, 257, 63, 0, 300, 31, 128, 65, 255, 33, 64, 256, 127]   # 1, 31, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300 and one 0, shuffled
SEAMS = Pack(SEAM_LENS, tail_q=40)
assert sorted(SEAM_LENS) == [0, 1, 31, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
assert sum(1 for c in SEAMS.cu_q[:-1] if c % 32) >= 10
UNEQUAL_PAIRS = [(5, 200), (200, 5), (130, 130), (0, 70), (70, 0), (257, 64)]
UNEQUAL = Pack([a for a, _ in UNEQUAL_PAIRS], [b for _, b in UNEQUAL_PAIRS], tail_q=24, tail_k=40)


def inputs(pack, Hkv, D, dtype, seed, std=0.5):
    """q [Tq, H, D], k, v [Tk, Hkv, D], do [Tq, H, D] in dtype on the CPU (the tail rows hold data too: nobody may read them)"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s, sd=std: (sd * torch.randn(*s, generator=g)).to(dtype)   # noqa: E731
    return dict(q=mk(pack.Tq, H, D), k=mk(pack.Tk, Hkv, D), v=mk(pack.Tk, Hkv, D, sd=1.0), do=mk(pack.Tq, H, D, sd=1.0))


_REF = {}


def reference(key, pack, inp, n, causal, log_n=None):
    """fp32 CPU reference of the whole pack, cached under `key` and never modified: out [Tq, H, D], lse [H, Tq], dq, dk, dv and - with
    log_n, an [H] tensor s whose n is exp(s) - ds. Rows beyond the last sequence: out 0, lse -inf, gradients 0."""
    if key in _REF:
        return _REF[key]
    q, k, v = (inp[x].float().requires_grad_() for x in ("q", "k", "v"))
    do = inp["do"].float()
    s = None if log_n is None else log_n.detach().float().cpu().requires_grad_()
    Hq, Hkv, D = q.shape[1], k.shape[1], q.shape[2]
    G = Hq // Hkv
    out = torch.zeros(pack.Tq, Hq, D)
    lse = torch.full((Hq, pack.Tq), -math.inf)
    pieces = []
    for b in range(pack.B):
        q0, q1, k0, k1 = pack.cu_q[b], pack.cu_q[b + 1], pack.cu_k[b], pack.cu_k[b + 1]
        sq, sk = q1 - q0, k1 - k0
        if sq == 0:
            continue
        for h in range(Hq):
            nh = float(n) if s is None else torch.exp(s[h])
            qb, kb, vb = q[q0:q1, h], k[k0:k1, h // G], v[k0:k1, h // G]
            if sk == 0:   # no key at all: 0 with lse = log n
                lse[h, q0:q1] = math.log(n) if (s is None and n > 0) else (-math.inf if s is None else s[h].detach())
                continue
            # causal with more rows than keys: the first sq - sk rows see no key - 0, lse = log n, no gradient. They are left out of the
            # reference's call (at n = 0 its softmax is 0 / 0 there and autograd would answer NaN); the rest keeps its bottom-right mask.
            first = max(0, sq - sk) if causal else 0
            ob = ref_attention_n(qb[first:], kb, vb, softmax_n_param=nh, is_causal=causal)
            pieces.append((ob * do[q0 + first:q1, h]).sum())
            out[q0 + first:q1, h] = ob.detach()
            with torch.no_grad():
                x = qb @ kb.t() / math.sqrt(D)
                if causal:
                    i, j = torch.arange(sq).unsqueeze(-1), torch.arange(sk).unsqueeze(0)
                    x = x.masked_fill(j > i + (sk - sq), -math.inf)
                nv = float(nh)
                sink = torch.full((sq, 1), math.log(nv) if nv > 0 else -math.inf)
                lse[h, q0:q1] = torch.logsumexp(torch.cat([x, sink], dim=1), dim=1)
    if pieces:
        torch.stack(pieces).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad   # noqa: E731
    r = dict(out=out, lse=lse, dq=zero(q), dk=zero(k), dv=zero(v), ds=None if s is None else zero(s))
    _REF[key] = r
    return r


def seq_rows(pack, side, b):
    cu = pack.cu_q if side == "q" else pack.cu_k
    return slice(cu[b], cu[b + 1])


# ---------------------------------------------------------------- the C ABI
def view_packed(pkg, t, ptr=None):
    v = pkg._lib.View4()
    v.ptr = t.data_ptr() if ptr is None else ptr
    v.stride[0], v.stride[1], v.stride[2], v.stride[3] = 0, t.stride(1), t.stride(0), t.stride(2)
    return v


def block(pkg, Tq, Tk, Hq, Hkv, D, dtype=torch.bfloat16, causal=False, n=1.0, num_seqs=3, max_q=300, max_k=None, base=DUMMY, q_token_stride=None):
    """(BwdArgs, Varlen) of a packed call over FAKE pointers `base`, `base` + 1 MiB, ...: contiguous [T, heads, D] operands (q at
    q_token_stride elements between tokens when given). For the plan and the refusals; nothing may be launched with it."""
    L = pkg._lib
    a = L.BwdArgs()
    f = a.fwd
    ptrs = iter(base + (i << 24) for i in range(16))

    def view(T, heads, tok=None):
        v = L.View4()
        v.ptr = next(ptrs)
        v.stride[0], v.stride[1], v.stride[2], v.stride[3] = 0, D, (heads * D if tok is None else tok), 1
        return v

    f.q, f.k, f.v, f.o = view(Tq, Hq, q_token_stride), view(Tk, Hkv), view(Tk, Hkv), view(Tq, Hq)
    f.lse = next(ptrs)
    f.mask.ptr = f.bias.ptr = None
    f.bias_dtype = 0
    f.dtype = {torch.float16: L.FASN_DTYPE_F16, torch.bfloat16: L.FASN_DTYPE_BF16, torch.float32: L.FASN_DTYPE_F32}[dtype]
    f.B, f.H, f.Sq, f.Sk, f.D, f.Dv = 1, Hq, Tq, Tk, D, D
    f.scale, f.softmax_n, f.causal, f.dropout_p = 1.0 / math.sqrt(D), n, 1 if causal else 0, 0.0
    f.seed = f.offset = 0
    f.kv_group = Hq // Hkv if Hkv != Hq else 0
    f.rng_state = None
    a.dout, a.dq, a.dk, a.dv = view(Tq, Hq), view(Tq, Hq), view(Tk, Hkv), view(Tk, Hkv)
    a.delta = next(ptrs)
    a.workspace, a.workspace_bytes, a.flags, a.dbias_dtype = None, 0, 0, 0
    a.dbias.ptr = None
    vl = L.Varlen()
    vl.cu_seqlens_q, vl.cu_seqlens_k = next(ptrs), next(ptrs)
    vl.num_seqs, vl.max_seqlen_q, vl.max_seqlen_k, vl.reserved = num_seqs, max_q, max_q if max_k is None else max_k, 0
    return a, vl


def run_abi(pkg, pack, t, n, causal, cu_q, cu_k, backward=True):
    """fasn_fwd_varlen (and fasn_bwd_varlen) over the device tensors t[...]: q, k, v, do in; o, lse, dq, dk, dv, delta out (allocated
    and pre-filled by the caller). Returns the forward's and the backward's codes."""
    L = pkg._lib
    lib = L.load()
    q = t["q"]
    a = L.BwdArgs()
    f = a.fwd
    f.q, f.k, f.v, f.o = (view_packed(pkg, t[x]) for x in ("q", "k", "v", "o"))
    f.lse = t["lse"].data_ptr()
    f.mask.ptr = f.bias.ptr = None
    f.bias_dtype = 0
    f.dtype = L.FASN_DTYPE_F16 if q.dtype == torch.float16 else L.FASN_DTYPE_BF16
    f.B, f.H, f.Sq, f.Sk, f.D, f.Dv = 1, q.shape[1], q.shape[0], t["k"].shape[0], q.shape[2], q.shape[2]
    f.scale, f.softmax_n, f.causal, f.dropout_p = 1.0 / math.sqrt(q.shape[2]), n, 1 if causal else 0, 0.0
    f.seed = f.offset = 0
    f.kv_group = q.shape[1] // t["k"].shape[1] if t["k"].shape[1] != q.shape[1] else 0
    f.rng_state = None
    vl = L.Varlen()
    vl.cu_seqlens_q, vl.cu_seqlens_k = cu_q.data_ptr(), cu_k.data_ptr()
    vl.num_seqs, vl.max_seqlen_q, vl.max_seqlen_k, vl.reserved = pack.B, pack.max_q, pack.max_k, 0
    stream = torch.cuda.current_stream(q.device).cuda_stream
    with torch.cuda.device(q.device):
        rc_f = lib.fasn_fwd_varlen(a.fwd, vl, None, 0, stream)
        rc_b = None
        if backward and rc_f == 0:
            a.dout, a.dq, a.dk, a.dv = (view_packed(pkg, t[x]) for x in ("do", "dq", "dk", "dv"))
            a.delta = t["delta"].data_ptr()
            a.workspace, a.workspace_bytes, a.flags, a.dbias_dtype = None, 0, 0, 0
            a.dbias.ptr = None
            rc_b = lib.fasn_bwd_varlen(a, vl, stream)
    torch.cuda.synchronize(q.device)
    return rc_f, rc_b


SENT = {torch.bfloat16: 0x7FA5, torch.float16: 0x7DA5}   # a NaN with a payload


def housed(T, heads, D, dtype, dev):
    """(view [T, heads, D] in dtype, int16 storage [T + 1, heads + 1, D + 8]): every element, the view's included, holds the sentinel"""
    store = torch.full((T + 1, heads + 1, D + 8), SENT[dtype], dtype=torch.int16, device=dev)
    return store[:T, :heads, :D].view(dtype), store


def gaps_intact(store, view):
    inside = torch.zeros(store.shape, dtype=torch.bool, device=store.device)
    inside[:view.shape[0], :view.shape[1], :view.shape[2]] = True
    return bool((store[~inside] == SENT[view.dtype]).all())


# ---------------------------------------------------------------- named plan cases (tests/golden/attn_varlen_plans.txt)
def plan_cases():
    """name -> the keyword arguments of block() and the plan (0 forward, 1 backward): per served head dim plain / causal x grouped / not x
    forward / backward"""
    out = {}
    for D in (64,):
        for causal in (False, True):
            for Hkv in (8, 2):
                for which in (0, 1):
                    name = f"D{D}_{'causal' if causal else 'plain'}_{'gqa4' if Hkv != 8 else 'mha'}_{'bwd' if which else 'fwd'}"
                    out[name] = (dict(Tq=2100, Tk=2100, Hq=8, Hkv=Hkv, D=D, causal=causal, num_seqs=14, max_q=300), which)
    out["D64_f16_unequal_bwd"] = (dict(Tq=700, Tk=520, Hq=4, Hkv=4, D=64, dtype=torch.float16, num_seqs=6, max_q=257, max_k=200), 1)
    return out
