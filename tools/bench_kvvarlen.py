"""Continuous-batching steps: flash_attention_n_kvcache_varlen on token-packed queries (B) against the route it replaces (A), same box,
same process.

  A = pad scatter (token -> [sequence, position], index tensors on the device) into an UNINITIALISED [B, Sq, H, D] buffer - the padded call
      never reads a padding row, so A pays for no zero fill - then flash_attention_n_kvcache_prefill with query_seqlens, then the gather
      back to [T, H, D]. All captured.
  B = flash_attention_n_kvcache_varlen on the packed buffer.
  dec (all-decode step only) = flash_attention_n_kvcache on the same tokens as [B, H, 1, D]: the decode kernels, beside B.
  B0 = B with every offset 0: the schedule kernel plus a forward grid that leaves at once - an upper bound of what the table costs.

Steps (bf16, page 256, per-head n, cache rows already appended): (a) one chunk of 2048 tokens behind 6144 cached keys plus 255 decode
tokens over 2048 .. 8192 keys; (b) 256 decode tokens over 2048 .. 8192 keys; (c) 4 chunks of 2048 tokens behind 6144 keys.

All go through their Python front ends, captured in a HIP graph of REPS calls; the graphs are replayed alternating and timed with device
events. Reported: microseconds per call of every alternation, B/A (ratio of medians, < 1 = B is faster), A's own spread between its
alternations (the margin B is judged against), max |A - B| over the real tokens, and the peak extra device memory of one eager call of
each route (torch's allocator statistics: outputs, temporaries and workspace).
usage: python tools/bench_kvvarlen.py [--rounds N] [--iters N] [--only SUBSTRING]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256
REPS = 4


def steps():
    spread = [2048 + (b * (8192 - 2048)) // 254 for b in range(255)]
    return [
        ("a mixed 2048@6144 + 255 x 1", [2048] + [1] * 255, [8192] + spread),
        ("b decode 256 x 1", [1] * 256, spread + [8192]),
        ("c chunks 4 x 2048@6144", [2048] * 4, [8192] * 4),
    ]


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            out = fn()
    return g, out


def time_graph(g, iters):
    for _ in range(2):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (iters * REPS)   # microseconds per call


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
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvvarlen needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    print(f"device: {torch.cuda.get_device_name(0)}; {REPS} calls per graph, {args.iters} replays per timing, {args.rounds} alternations A / B")
    print(f"{'step (H/Hkv,D)':44s} {'A us':>26s} {'B us':>26s} {'B/A':>6s} {'A spread':>9s} {'max|A-B|':>9s} {'A MiB':>8s} {'B MiB':>8s} {'B0 us':>7s} {'dec us':>22s}")
    med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
    fmt = lambda ts: "/".join(f"{t:.0f}" for t in ts)   # noqa: E731
    for H, Hkv, D in ((64, 8, 64), (16, 16, 128)):
        for name, qlens, lens in steps():
            name = f"{name} ({H}/{Hkv},{D})"
            if args.only not in name:
                continue
            torch.manual_seed(0)
            B, T, Sq = len(qlens), sum(qlens), max(qlens)
            max_pages = (max(lens) + PAGE - 1) // PAGE
            need = [(ln + PAGE - 1) // PAGE for ln in lens]
            num_pages = sum(need)
            q = torch.randn(T, H, D, device=dev, dtype=dtype) * 0.5
            pool_k = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
            pool_v = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
            ids = torch.randperm(num_pages).tolist()
            table = torch.zeros(B, max_pages, dtype=torch.int32)
            for b in range(B):   # shuffled pages; entries beyond a sequence's pages are never read
                table[b, :need[b]] = torch.tensor([ids.pop() for _ in range(need[b])], dtype=torch.int32)
            table = table.to(dev)
            sl = torch.tensor(lens, dtype=torch.int32, device=dev)
            ql = torch.tensor(qlens, dtype=torch.int32, device=dev)
            cu = torch.tensor([0] + torch.tensor(qlens).cumsum(0).tolist(), dtype=torch.int32, device=dev)
            b_idx = torch.repeat_interleave(torch.arange(B, device=dev), ql.long())
            i_idx = torch.arange(T, device=dev) - cu[:-1].long()[b_idx]
            n = torch.rand(H, device=dev) + 0.5

            def run_a():
                qp = torch.empty(B, Sq, H, D, device=dev, dtype=dtype)
                qp[b_idx, i_idx] = q
                o = fa.flash_attention_n_kvcache_prefill(qp.transpose(1, 2), pool_k, pool_v, sl, block_table=table, query_seqlens=ql, softmax_n_param=n)
                return o.transpose(1, 2)[b_idx, i_idx]

            def run_b():
                return fa.flash_attention_n_kvcache_varlen(q, pool_k, pool_v, sl, cu, Sq, block_table=table, softmax_n_param=n)

            cu0 = torch.zeros_like(cu)

            def run_b0():
                return fa.flash_attention_n_kvcache_varlen(q, pool_k, pool_v, sl, cu0, Sq, block_table=table, softmax_n_param=n)

            def run_dec():
                return fa.flash_attention_n_kvcache(q.unsqueeze(2), pool_k, pool_v, sl, block_table=table, softmax_n_param=n)

            with torch.no_grad():
                mem_a, mem_b = peak_extra(run_a), peak_extra(run_b)
                ga, oa = graph_of(run_a)
                gb, ob = graph_of(run_b)
                g0, _ = graph_of(run_b0)
                gd = graph_of(run_dec)[0] if Sq == 1 else None
                ta, tb, td = [], [], []
                for _ in range(args.rounds):
                    ta.append(time_graph(ga, args.iters))
                    tb.append(time_graph(gb, args.iters))
                    if gd is not None:
                        td.append(time_graph(gd, args.iters))
                t0 = time_graph(g0, args.iters)
                torch.cuda.synchronize()
                diff = (oa.float() - ob.float()).abs().max().item()
            print(f"{name:44s} {fmt(ta):>26s} {fmt(tb):>26s} {med(tb) / med(ta):6.2f} {max(ta) / min(ta):9.3f} {diff:9.2e} {mem_a:8.1f} {mem_b:8.1f} {t0:7.1f} "
                  f"{fmt(td) if td else '-':>22s}", flush=True)
            del ga, gb, g0, gd, pool_k, pool_v, oa, ob
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
