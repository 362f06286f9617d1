"""Packed training batches: flash_attention_n_varlen (B) against the two routes it replaces, same box, same process.

  A  = the padded route: scatter the packed tokens to [B, H, Lmax, D] (index tensors on the device), flash_attention_n with a
       [B, 1, 1, Lmax] key-padding mask plus is_causal, gather back to [T, H, D]; forward + backward includes the scatter's and the
       gather's backward (autograd).
  A2 = flash_attention_n on the [1, H, T, D] stream under the dense block-diagonal (causal) boolean mask [1, 1, T, T].
  B  = flash_attention_n_varlen on the packed buffers.

bf16, causal, T = 16384 tokens in two packs: 16 x 1024 (nothing to gain from padding-freedom) and one 8192 + eight 1024. The routes
alternate (A, A2, B, A, A2, B, ...); each timing is `iters` eager calls between two device events after a warm-up - the calls are
millisecond-sized, the host side of a call is a few microseconds. Reported per pack, for the forward and for forward + backward:
milliseconds of every alternation, B / A and B / A2 (ratios of medians, < 1 = B is faster), A's own spread between its alternations (the
margin B is judged against), the peak extra device memory of one call of each route (torch's allocator statistics: outputs, temporaries,
saved tensors) and max |A - B| and |A2 - B| over the sequences' rows of the forward result.
usage: python tools/bench_attnvarlen.py [--rounds N] [--iters N] [--only SUBSTRING] [--no-a2]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

SERVED = ((64, 8, 64),)   # (H, Hkv, D); (16, 16, 128) joins when fasn_fwd_varlen serves D = 128


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


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-a2", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attnvarlen needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    print(f"device: {torch.cuda.get_device_name(0)}; bf16, causal, n = 1; {args.iters} calls per timing, {args.rounds} alternations A / A2 / B")
    med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
    fmt = lambda ts: "/".join(f"{t:.3f}" for t in ts) if ts else "-"   # noqa: E731
    for H, Hkv, D in SERVED:
        for name, lens in packs():
            tag = f"{name} ({H}/{Hkv},{D})"
            if args.only not in tag:
                continue
            torch.manual_seed(0)
            B, T, Lmax = len(lens), sum(lens), max(lens)
            q = (torch.randn(T, H, D, device=dev) * 0.5).to(dtype).requires_grad_()
            k = (torch.randn(T, Hkv, D, device=dev) * 0.5).to(dtype).requires_grad_()
            v = (torch.randn(T, Hkv, D, device=dev) * 0.5).to(dtype).requires_grad_()
            do = torch.randn(T, H, D, device=dev).to(dtype)
            ql = torch.tensor(lens, device=dev)
            cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)
            b_idx = torch.repeat_interleave(torch.arange(B, device=dev), ql)
            i_idx = torch.arange(T, device=dev) - cu[:-1].long()[b_idx]
            keypad = (torch.arange(Lmax, device=dev)[None, :] < ql[:, None]).view(B, 1, 1, Lmax)
            dense = None
            if not args.no_a2:   # block-diagonal and causal: same sequence, key not behind the row
                dense = ((b_idx[:, None] == b_idx[None, :]) & (torch.arange(T, device=dev)[None, :] <= torch.arange(T, device=dev)[:, None])).view(1, 1, T, T)

            def pad(x, heads):
                return torch.zeros(B, Lmax, heads, D, device=dev, dtype=dtype).index_put((b_idx, i_idx), x).transpose(1, 2)

            def fwd_a():
                o = fa.flash_attention_n(pad(q, H), pad(k, Hkv), pad(v, Hkv), softmax_n_param=1.0, attn_mask=keypad, is_causal=True)
                return o.transpose(1, 2)[b_idx, i_idx]

            def fwd_a2():
                o = fa.flash_attention_n(q.transpose(0, 1).unsqueeze(0), k.transpose(0, 1).unsqueeze(0), v.transpose(0, 1).unsqueeze(0),
                                         softmax_n_param=1.0, attn_mask=dense)
                return o.squeeze(0).transpose(0, 1)

            def fwd_b():
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

            routes = [("A", fwd_a), ("A2", fwd_a2), ("B", fwd_b)] if dense is not None else [("A", fwd_a), ("B", fwd_b)]
            outs = {r: infer(f)().float() for r, f in routes}
            diffs = {}
            for r in outs:
                if r != "B":
                    diffs[r] = max((outs[r][cu[b]:cu[b + 1]] - outs["B"][cu[b]:cu[b + 1]]).abs().max().item() for b in range(B))
            del outs
            for what, wrap in (("forward", infer), ("forward + backward", train)):
                fns = {r: wrap(f) for r, f in routes}
                mem = {r: peak_extra(fn) for r, fn in fns.items()}
                ts = {r: [] for r in fns}
                for _ in range(args.rounds):
                    for r, fn in fns.items():
                        ts[r].append(timed(fn, args.iters))
                line = f"{tag:28s} {what:19s} A ms {fmt(ts['A'])}  A2 ms {fmt(ts.get('A2'))}  B ms {fmt(ts['B'])}  B/A {med(ts['B']) / med(ts['A']):.3f}"
                if "A2" in ts:
                    line += f"  B/A2 {med(ts['B']) / med(ts['A2']):.3f}"
                line += f"  A spread {max(ts['A']) / min(ts['A']):.3f}  extra MiB A {mem['A']:.0f}" + (f" A2 {mem['A2']:.0f}" if "A2" in mem else "") + f" B {mem['B']:.0f}"
                line += "  max|A-B| " + f"{diffs['A']:.2e}" + (f" max|A2-B| {diffs['A2']:.2e}" if "A2" in diffs else "")
                print(line, flush=True)
            del dense, keypad
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
