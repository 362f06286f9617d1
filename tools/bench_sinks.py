"""Per-(batch, head) softmax_n (tensor n, learned attention sinks) against the scalar n on the same box, alternating:
  - forward with a tensor n vs the float n, at M0 (8,16,4096,64) bf16 and at a GPT-OSS-like causal GQA shape (4,64/8,4096,64) bf16;
  - fasn_bwd_dn (the dn kernels) vs the whole backward (fasn_bwd) of M0.
Prints one JSON line with the medians (ms) and the ratios. usage: python tools/bench_sinks.py [rounds]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flash_attention_softmax_n_amd as fa   # noqa: E402
from flash_attention_softmax_n_amd import _lib, flash_attn   # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
dev = torch.device("cuda:0")
dt = torch.bfloat16


def timed(fn, iters=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, rounds=ROUNDS):
    """median ms of each function, measured in alternation (A B A B ...) after a warm-up of each"""
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            out[i].append(timed(f))
    return [statistics.median(t) for t in out]


res = {}
for name, (B, H, Hkv, S, D, causal) in (("m0", (8, 16, 16, 4096, 64, False)), ("gptoss_gqa_causal", (4, 64, 8, 4096, 64, True))):
    torch.manual_seed(0)
    q = torch.randn(B, H, S, D, device=dev, dtype=dt).mul_(0.5)
    k, v = (torch.randn(B, Hkv, S, D, device=dev, dtype=dt).mul_(0.5) for _ in range(2))
    nt = torch.exp(torch.randn(H, device=dev))
    with torch.no_grad():
        t_scalar, t_tensor = alternate([lambda: fa.flash_attention_n(q, k, v, softmax_n_param=1.0, is_causal=causal),
                                        lambda: fa.flash_attention_n(q, k, v, softmax_n_param=nt, is_causal=causal)])
    res[name] = {"fwd_scalar_ms": round(t_scalar, 4), "fwd_tensor_ms": round(t_tensor, 4), "tensor_over_scalar": round(t_tensor / t_scalar, 4)}

# dn kernels vs the backward at M0: the two C entry points on one argument block
B, H, S, D = 8, 16, 4096, 64
q, k, v = (torch.randn(B, H, S, D, device=dev, dtype=dt).mul_(0.5) for _ in range(3))
do = torch.randn(B, H, S, D, device=dev, dtype=dt)
nt = flash_attn._n_tensor(torch.full((H,), 1.0, device=dev), q)
o, lse = flash_attn._launch_fwd(q, k, v, None, None, nt, D ** -0.5, False, 0.0, None)
lib = _lib.load()
a = _lib.BwdArgs()
flash_attn._fill_fwd(a.fwd, q, k, v, o, lse, None, None, 0.0, D ** -0.5, False)
dq, dk, dv = (torch.empty_like(q) for _ in range(3))
delta = torch.empty(B, H, S, device=dev, dtype=torch.float32)
a.dout, a.dq, a.dk, a.dv, a.delta = flash_attn._view4(do), flash_attn._view4(dq), flash_attn._view4(dk), flash_attn._view4(dv), delta.data_ptr()
dn = torch.empty(1, H, device=dev, dtype=torch.float32)
wsb = lib.fasn_bwd_dn_workspace_bytes(a)
ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
stream = flash_attn._stream_ptr(dev)
t_bwd, t_dn = alternate([lambda: _lib.check(lib.fasn_bwd(a, stream), "fasn_bwd"),
                         lambda: _lib.check(lib.fasn_bwd_dn(a, dn.data_ptr(), 0, 1, ws.data_ptr(), wsb, stream), "fasn_bwd_dn")])
moved = 2 * B * H * S * D * 2 + B * H * S * 4
res["m0_dn"] = {"bwd_ms": round(t_bwd, 4), "dn_ms": round(t_dn, 4), "dn_over_bwd": round(t_dn / t_bwd, 4),
                "dn_GBps": round(moved / (t_dn * 1e-3) / 1e9, 1), "workspace_bytes": wsb}
print(json.dumps(res))
