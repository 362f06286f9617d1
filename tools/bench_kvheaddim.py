"""K/V-cache decode and prefill at head dims 256 and 32 (B) against the only route a caller had at those head dims before the cache calls
took them (A + g), same box, same process.

  A   = flash_attention_n on dense K/V [B, Hkv, S, D] of the same lengths: decode with a key-padding mask, prefill with is_causal=True
        (bottom-right aligned: the chunk behind its prefix). These kernels are not touched by the cache calls.
  g   = the pages -> dense gather a paged caller needs before A (index through the block table, permute, copy), timed inside A+g.
  B   = flash_attention_n_kvcache / flash_attention_n_kvcache_prefill on the paged cache (page 256, shuffled block table, lengths in
        device memory; K/V already in the cache).

All go through their Python front ends, captured in a HIP graph of REPS calls so that host time is out of the picture; the graphs are
replayed alternating A / A+g / B and timed with device events. Reported: microseconds per call for every alternation, B/A and B/(A+g)
(ratios of medians, < 1 = B is faster), the visible K+V bytes per second of B, A's own spread between its alternations (the margin B is
judged against) and max |A - B|.
usage: python tools/bench_kvheaddim.py [--rounds N] [--iters N] [--only SUBSTRING] [--trace-calls N]
--trace-calls N: no graphs and no table, N eager calls of A and of B per shape - the program to put behind
`rocprofv3 --kernel-trace --stats --`, where the kernels of both routes show up under their own names."""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256
REPS = 4


# (name, call, B, H, Hkv, Sq, key lengths, D, tensor n)
def shapes():
    ragged = [2048 + (b * (8192 - 2048)) // 31 for b in range(32)]
    out = []
    for D in (256, 32):
        out.append((f"decode (64,16,1,8192,{D})", "decode", 64, 16, 16, 1, [8192] * 64, D, False))
        if D == 256:
            out.append((f"decode (32,16/8,1,2048..8192,{D}) n[H]", "decode", 32, 16, 8, 1, ragged, D, True))
        out.append((f"prefill (4,16/8,2048,6144,{D}) n[H]", "prefill", 4, 16, 8, 2048, [6144 + 2048] * 4, D, True))
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--trace-calls", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvheaddim needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    print(f"device: {torch.cuda.get_device_name(0)}; bf16, {REPS} calls per graph, {args.iters} replays per timing, {args.rounds} alternations A / A+g / B")
    print(f"{'shape (B,H[/Hkv],Sq,S or prefix,D)':42s} {'A us':>22s} {'A+g us':>22s} {'B us':>22s} {'B/A':>6s} {'B/(A+g)':>8s} {'B TB/s':>7s} {'A spread':>9s} {'max|A-B|':>9s}")
    for name, call, B, H, Hkv, Sq, lens, D, tensor_n in shapes():
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
        n = (torch.rand(H, device=dev) + 0.5) if tensor_n else 1.0
        keypad = torch.arange(S, device=dev).view(1, 1, 1, S) < sl.view(B, 1, 1, 1)

        def gather():
            kd = pool_k[tl].reshape(B, max_pages * PAGE, Hkv, D)[:, :S].permute(0, 2, 1, 3).contiguous()
            vd = pool_v[tl].reshape(B, max_pages * PAGE, Hkv, D)[:, :S].permute(0, 2, 1, 3).contiguous()
            return kd, vd

        kd, vd = gather()

        def attn_a(kd_, vd_):
            if call == "decode":
                return fa.flash_attention_n(q, kd_, vd_, softmax_n_param=n, attn_mask=keypad)
            return fa.flash_attention_n(q, kd_, vd_, softmax_n_param=n, is_causal=True)

        def run_a():
            return attn_a(kd, vd)

        def run_ag():
            return attn_a(*gather())

        def run_b():
            if call == "decode":
                return fa.flash_attention_n_kvcache(q, pool_k, pool_v, sl, block_table=table, softmax_n_param=n, is_causal=False)
            return fa.flash_attention_n_kvcache_prefill(q, pool_k, pool_v, sl, block_table=table, softmax_n_param=n, is_causal=True)

        if args.trace_calls:
            with torch.no_grad():
                for _ in range(args.trace_calls):
                    run_a()
                    run_b()
            torch.cuda.synchronize()
            print(f"{name}: {args.trace_calls} eager calls of A and of B", flush=True)
            del kd, vd, pool_k, pool_v
            torch.cuda.empty_cache()
            continue
        with torch.no_grad():
            ga, oa = graph_of(run_a)
            gg, og = graph_of(run_ag)
            gb, ob = graph_of(run_b)
            ta, tg, tb = [], [], []
            for _ in range(args.rounds):
                ta.append(time_graph(ga, args.iters))
                tg.append(time_graph(gg, args.iters))
                tb.append(time_graph(gb, args.iters))
            torch.cuda.synchronize()
            diff = (oa.float() - ob.float()).abs().max().item()
        visible = sum(lens) * Hkv * D * 2 * 2
        med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
        fmt = lambda ts: "/".join(f"{t:.0f}" for t in ts)   # noqa: E731
        print(f"{name:42s} {fmt(ta):>22s} {fmt(tg):>22s} {fmt(tb):>22s} {med(tb) / med(ta):6.2f} {med(tb) / med(tg):8.2f} "
              f"{visible / med(tb) / 1e6:7.2f} {max(ta) / min(ta):9.3f} {diff:9.2e}", flush=True)
        del ga, gg, gb, kd, vd, pool_k, pool_v, oa, og, ob
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
