"""Rotary position embedding on packed training batches: flash_attention_n_varlen_rope (B) against the route it replaces (A), same box,
same process. The method is tools/bench_attnvarlen.py's.

  A  = fully on the device: positions from cu_seqlens by searchsorted (fixed output size, no host read), a gather of two table rows per
       token, the rotation of q and k with torch ops under autograd (fp32, rounded once), then flash_attention_n_varlen.
  B  = flash_attention_n_varlen_rope: one rotary launch in front of the packed call; the backward rotates dq / dk in place.

bf16, causal, n = 1, (H / Hkv, D) = (64 / 8, 64), T = 16384 tokens in two packs: 16 x 1024 and one 8192 + eight 1024; fp32 tables,
rotary_dim 64, half-split. The routes alternate (A, B, A, B, ...); each timing is `iters` eager calls between two device events after a
warm-up. Reported per pack, for the forward and for forward + backward: milliseconds of every alternation, B / A (ratio of medians, < 1 =
B is faster), A's own spread between its alternations (the margin B is judged against), the peak of extra device memory one forward +
backward step takes beyond what is resident before it, max |B - A| over the forward result; then the rotary launch alone (a captured
graph of `--launches` launches, microseconds per launch, achieved bytes/s over its algorithmic bytes 2 T (H + Hkv) 64 2 + the table
rows) beside the plain packed forward. No counter pass is taken.
usage: python tools/bench_attnvarlen_rope.py [--rounds N] [--iters N] [--launches N] [--only SUBSTRING] [--out FILE]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

H, HKV, D = 64, 8, 64


def packs():
    return [("16 x 1024", [1024] * 16), ("8192 + 8 x 1024", [8192] + [1024] * 8)]


def timed(fn, iters):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters   # milliseconds per call


def extra_memory(step):
    """peak device memory of one step beyond what was allocated before it, MiB"""
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attnvarlen_rope needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    lines = [f"device: {torch.cuda.get_device_name(0)}; bf16, causal, n = 1, ({H} / {HKV}, {D}), fp32 tables, rotary_dim {D}; {args.iters} calls per "
             f"timing, {args.rounds} alternations A / B; no counter pass"]
    print(lines[0], flush=True)
    med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
    fmt = lambda ts: "/".join(f"{t:.3f}" for t in ts)   # noqa: E731
    for name, lens in packs():
        if args.only not in name:
            continue
        torch.manual_seed(0)
        B, T, Lmax = len(lens), sum(lens), max(lens)
        q = (torch.randn(T, H, D, device=dev) * 0.5).to(dtype).requires_grad_()
        k = (torch.randn(T, HKV, D, device=dev) * 0.5).to(dtype).requires_grad_()
        v = (torch.randn(T, HKV, D, device=dev) * 0.5).to(dtype).requires_grad_()
        do = torch.randn(T, H, D, device=dev).to(dtype)
        cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)
        inv = 10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
        ang = torch.arange(Lmax, dtype=torch.float64).unsqueeze(1) * inv
        cos, sin = ang.cos().float().to(dev), ang.sin().float().to(dev)
        tok = torch.arange(T, device=dev, dtype=torch.int32)

        def rot(x, c, s):
            xf = x.float()
            x1, x2 = xf[..., :D // 2], xf[..., D // 2:]
            return torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1).to(x.dtype)

        def fwd_a():
            b = torch.searchsorted(cu[1:], tok, right=True).clamp_(max=B - 1)   # [T], no host read
            pos = (tok - cu[b]).long()
            c, s = cos[pos].unsqueeze(1), sin[pos].unsqueeze(1)
            return fa.flash_attention_n_varlen(rot(q, c, s), rot(k, c, s), v, cu, Lmax, softmax_n_param=1.0, is_causal=True)

        def fwd_b():
            return fa.flash_attention_n_varlen_rope(q, k, v, cu, Lmax, cos, sin, softmax_n_param=1.0, is_causal=True)

        def fwd_plain():
            return fa.flash_attention_n_varlen(q, k, v, cu, Lmax, softmax_n_param=1.0, is_causal=True)

        def train(fwd):
            def step():
                return torch.autograd.grad(fwd(), (q, k, v), do)
            return step

        def infer(fwd):
            def step():
                with torch.no_grad():
                    return fwd()
            return step

        diff = (infer(fwd_a)().float() - infer(fwd_b)().float()).abs().max().item()
        mem = {r: extra_memory(train(f)) for r, f in (("A", fwd_a), ("B", fwd_b))}
        for what, wrap in (("forward", infer), ("forward + backward", train)):
            fns = {"A": wrap(fwd_a), "B": wrap(fwd_b)}
            ts = {r: [] for r in fns}
            for _ in range(args.rounds):
                for r, fn in fns.items():
                    ts[r].append(timed(fn, args.iters))
            line = (f"{name:16s} {what:19s} A ms {fmt(ts['A'])}  B ms {fmt(ts['B'])}  B/A {med(ts['B']) / med(ts['A']):.3f}  "
                    f"A spread {max(ts['A']) / min(ts['A']):.3f}  max|B-A| {diff:.2e}")
            if what != "forward":
                line += f"  extra MiB per step A {mem['A']:.0f} B {mem['B']:.0f}"
            print(line, flush=True)
            lines.append(line)

        # the rotary launch alone: a captured graph of `launches` launches
        rope = fa.kvcache._rope_operand(cos, sin, False, q)
        qd, kd = q.detach(), k.detach()
        qo, ko = torch.empty_like(qd), torch.empty_like(kd)
        launch = lambda: fa.flash_attn._launch_varlen_rope(qd, kd, qo, ko, cu, cu, Lmax, Lmax, rope, False)   # noqa: E731
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launch()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.launches):
                launch()
        us = [1e3 * timed(g.replay, args.iters) / args.launches for _ in range(args.rounds)]
        nbytes = 2 * T * (H + HKV) * D * 2 + 2 * Lmax * (D // 2) * 4
        plain = [timed(infer(fwd_plain), args.iters) for _ in range(args.rounds)]
        line = (f"{name:16s} rotary launch alone  us {'/'.join(f'{u:.1f}' for u in us)}  {nbytes / 2 ** 20:.0f} MiB algorithmic  "
                f"{nbytes / (med(us) * 1e-6) / 1e12:.2f} TB/s  plain packed forward ms {fmt(plain)}")
        print(line, flush=True)
        lines.append(line)
        del g
        torch.cuda.empty_cache()
    if args.out:
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
