"""The sliding window on the K/V-cache calls: what a window of W keys costs or saves inside the cache kernels, and what it saves over the
route a caller had. Same box, same process, four shapes: a GQA decode (64 query heads on 8 K/V heads, D = 64, per-head n) on an 8192-key
cache, its ragged sibling, a 2048-position chunk against a long cache, all at W = 128, and the decode shape again at W = 8192, where the
window covers everything and only its tests remain.

  B  = flash_attention_n_kvcache_window on the paged cache (page 256, shuffled block table, lengths in device memory).
  A0 = flash_attention_n_kvcache / flash_attention_n_kvcache_prefill on the same cache without a window: it reads all len_b keys and
       computes ANOTHER function - a cost baseline only. B / A0 at W = 8192 is the overhead of the window kernels.
  A1 = what a caller did before: flash_attention_n on dense K/V with a dense boolean mask [B, 1, Sq, S] built from the lengths. The
       pages -> dense gather and the construction of the mask, which that route needs per step, are timed separately and reported
       beside A1, NOT inside it.

All go through their Python front ends, captured in a HIP graph of REPS calls so that host time is out of the picture; the graphs are
replayed alternating A0 / B / A1 and timed with device events. Reported: microseconds per call for every alternation, B/A0 next to A0's
own spread between its alternations (the margin B is judged against), B/(A1 + gather + mask) (ratios of medians, < 1 = B is faster) and
max |A1 - B|. usage: python tools/bench_kvwindow.py [--rounds N] [--iters N] [--only SUBSTRING]
--trace-calls N: no graphs and no table, N eager calls of A0 and of B per shape - the program to put behind
`rocprofv3 --kernel-trace --stats --`, where the kernels with and without the window show up under their own names."""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256


# (name, B, H, Hkv, Sq, cache lengths (the Sq positions included), D, window, calls per graph); n is a tensor [H] everywhere
def shapes():
    ragged = [2048 + (b * (8192 - 2048)) // 31 for b in range(32)]
    return [
        ("decode (64,64/8,1,8192,64) W=128", 64, 64, 8, 1, [8192] * 64, 64, 128, 10),
        ("decode (32,64/8,1,2048..8192,64) W=128", 32, 64, 8, 1, ragged, 64, 128, 10),
        ("chunk (4,64/8,2048,6144,64) W=128", 4, 64, 8, 2048, [6144 + 2048] * 4, 64, 128, 4),
        ("decode (64,64/8,1,8192,64) W=8192", 64, 64, 8, 1, [8192] * 64, 64, 8192, 10),
    ]


def graph_of(fn, reps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            out = fn()
    return g, out


def time_graph(g, iters, reps):
    for _ in range(2):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (iters * reps)   # microseconds per call


def time_eager(fn, n=5):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--trace-calls", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvwindow needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    if not args.trace_calls:
        print(f"device: {torch.cuda.get_device_name(0)}; {args.iters} replays per timing, {args.rounds} alternations A0 / B / A1")
        print(f"{'shape (B,H[/Hkv],Sq,S,D)':40s} {'A0 us':>22s} {'B us':>22s} {'A1 us':>22s} {'gather us':>10s} {'mask us':>9s} {'B/A0':>6s} {'A0 spread':>9s} "
              f"{'B/(A1+g+m)':>10s} {'max|A1-B|':>9s}")
    for name, B, H, Hkv, Sq, lens, D, W, reps in shapes():
        if args.only not in name:
            continue
        torch.manual_seed(0)
        S = max(lens)
        max_pages = (S + PAGE - 1) // PAGE
        num_pages = B * max_pages
        q = torch.randn(B, H, Sq, D, device=dev, dtype=dtype) * 0.5
        pool_k = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        pool_v = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        table = torch.randperm(num_pages, device=dev).to(torch.int32).view(B, max_pages)
        tl = table.long()
        sl = torch.tensor(lens, dtype=torch.int32, device=dev)
        n = torch.rand(H, device=dev) + 0.5
        call = fa.flash_attention_n_kvcache if Sq == 1 else fa.flash_attention_n_kvcache_prefill

        if args.trace_calls:
            with torch.no_grad():
                for _ in range(args.trace_calls):
                    call(q, pool_k, pool_v, sl, block_table=table, softmax_n_param=n)
                    fa.flash_attention_n_kvcache_window(q, pool_k, pool_v, sl, W, block_table=table, softmax_n_param=n)
            torch.cuda.synchronize()
            print(f"{name}: {args.trace_calls} eager calls of A0 and of B", flush=True)
            continue

        def gather():
            kd = pool_k[tl].reshape(B, max_pages * PAGE, Hkv, D)[:, :S].permute(0, 2, 1, 3).contiguous()
            vd = pool_v[tl].reshape(B, max_pages * PAGE, Hkv, D)[:, :S].permute(0, 2, 1, 3).contiguous()
            return kd, vd

        def make_mask():   # j < len_b and p_i - W < j <= p_i with p_i = i + len_b - Sq: the offset is per batch element
            p = torch.arange(Sq, device=dev).view(1, 1, Sq, 1) + (sl.view(B, 1, 1, 1) - Sq)
            j = torch.arange(S, device=dev).view(1, 1, 1, S)
            return (j <= p) & (j > p - W)

        kd, vd = gather()
        mask = make_mask()

        def run_a0():
            return call(q, pool_k, pool_v, sl, block_table=table, softmax_n_param=n)

        def run_b():
            return fa.flash_attention_n_kvcache_window(q, pool_k, pool_v, sl, W, block_table=table, softmax_n_param=n)

        def run_a1():
            return fa.flash_attention_n(q, kd, vd, softmax_n_param=n, attn_mask=mask)

        with torch.no_grad():
            g0, _o0 = graph_of(run_a0, reps)
            gb, ob = graph_of(run_b, reps)
            g1, o1 = graph_of(run_a1, reps)
            t0, tb, t1 = [], [], []
            for _ in range(args.rounds):
                t0.append(time_graph(g0, args.iters, reps))
                tb.append(time_graph(gb, args.iters, reps))
                t1.append(time_graph(g1, args.iters, reps))
            torch.cuda.synchronize()
            diff = (o1.float() - ob.float()).abs().max().item()
            tg, tmask = time_eager(gather), time_eager(make_mask)
        med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
        fmt = lambda ts: "/".join(f"{t:.1f}" for t in ts)   # noqa: E731
        print(f"{name:40s} {fmt(t0):>22s} {fmt(tb):>22s} {fmt(t1):>22s} {tg:10.1f} {tmask:9.1f} {med(tb) / med(t0):6.3f} {max(t0) / min(t0):9.3f} "
              f"{med(tb) / (med(t1) + tg + tmask):10.3f} {diff:9.2e}", flush=True)
        del g0, gb, g1, kd, vd, mask, pool_k, pool_v, ob, o1, _o0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
