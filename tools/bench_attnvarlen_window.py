"""Sliding-window layers on packed training batches: flash_attention_n_varlen(..., window=W) (B) against the launch it must beat and the
only route to its result without it, same box, same process. The method is tools/bench_attnvarlen.py's.

  A  = flash_attention_n_varlen(..., is_causal=True) without the window: more work and another result, but the launch B must beat.
  A2 = flash_attention_n on the [1, H, T, D] stream under the dense band-and-block-diagonal boolean mask [1, 1, T, T]: the one route to
       B's result without the window keyword.
  B  = flash_attention_n_varlen(..., is_causal=True, window=128); on the long pack also window = 1024 (B1024).

bf16, n = 1, (H / Hkv, D) = (64 / 8, 64), T = 16384 tokens in two packs: 16 x 1024 and one 8192 + eight 1024. The routes alternate
(A, A2, B, A, A2, B, ...); each timing is `iters` eager calls between two device events after a warm-up. Reported per pack, for the
forward and for forward + backward: milliseconds of every alternation, B / A and B / A2 (ratios of medians, < 1 = B is faster), A's own
spread between its alternations (the margin B is judged against) and max |B - A2| over the forward result. No counter pass is taken.
usage: python tools/bench_attnvarlen_window.py [--rounds N] [--iters N] [--only SUBSTRING] [--no-a2] [--out FILE]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

H, HKV, D, WINDOW, WIDE = 64, 8, 64, 128, 1024


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-a2", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attnvarlen_window needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    lines = [f"device: {torch.cuda.get_device_name(0)}; bf16, causal, n = 1, ({H} / {HKV}, {D}), window {WINDOW}; {args.iters} calls per timing, "
             f"{args.rounds} alternations A / A2 / B; no counter pass"]
    print(lines[0], flush=True)
    med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
    fmt = lambda ts: "/".join(f"{t:.3f}" for t in ts) if ts else "-"   # noqa: E731
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
        b_idx = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(lens, device=dev))
        dense = None
        if not args.no_a2:   # same sequence, key not behind the row, key inside the row's window (token distance = position distance: self-attention)
            t = torch.arange(T, device=dev)
            dense = ((b_idx[:, None] == b_idx[None, :]) & (t[None, :] <= t[:, None]) & (t[None, :] > t[:, None] - WINDOW)).view(1, 1, T, T)

        def fwd_a():
            return fa.flash_attention_n_varlen(q, k, v, cu, Lmax, softmax_n_param=1.0, is_causal=True)

        def fwd_a2():
            o = fa.flash_attention_n(q.transpose(0, 1).unsqueeze(0), k.transpose(0, 1).unsqueeze(0), v.transpose(0, 1).unsqueeze(0),
                                     softmax_n_param=1.0, attn_mask=dense)
            return o.squeeze(0).transpose(0, 1)

        def fwd_b(window=WINDOW):
            return fa.flash_attention_n_varlen(q, k, v, cu, Lmax, softmax_n_param=1.0, is_causal=True, window=window)

        def train(fwd):
            def step():
                return torch.autograd.grad(fwd(), (q, k, v), do)
            return step

        def infer(fwd):
            def step():
                with torch.no_grad():
                    return fwd()
            return step

        routes = [("A", fwd_a)] + ([("A2", fwd_a2)] if dense is not None else []) + [("B", fwd_b)]
        if Lmax > WIDE:
            routes.append((f"B{WIDE}", lambda: fwd_b(WIDE)))
        diff = None
        if dense is not None:
            diff = (infer(fwd_a2)().float() - infer(fwd_b)().float()).abs().max().item()
        for what, wrap in (("forward", infer), ("forward + backward", train)):
            fns = {r: wrap(f) for r, f in routes}
            ts = {r: [] for r in fns}
            for _ in range(args.rounds):
                for r, fn in fns.items():
                    ts[r].append(timed(fn, args.iters))
            line = f"{name:16s} {what:19s} A ms {fmt(ts['A'])}  A2 ms {fmt(ts.get('A2'))}  B ms {fmt(ts['B'])}  B/A {med(ts['B']) / med(ts['A']):.3f}"
            if "A2" in ts:
                line += f"  B/A2 {med(ts['B']) / med(ts['A2']):.3f}"
            line += f"  A spread {max(ts['A']) / min(ts['A']):.3f}"
            wide = f"B{WIDE}"
            if wide in ts:
                line += f"  {wide} ms {fmt(ts[wide])}  {wide}/A {med(ts[wide]) / med(ts['A']):.3f}"
            if diff is not None:
                line += f"  max|B-A2| {diff:.2e}"
            print(line, flush=True)
            lines.append(line)
        del dense
        torch.cuda.empty_cache()
    if args.out:
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
