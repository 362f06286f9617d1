"""Decode behind a shared prefix: flash_attention_n_kvcache_shared_prefix (B) against the route the package offered before it (A), same
box, same process.

  A = flash_attention_n_kvcache on block tables whose first slots name the SAME prefix pages for every sequence (what a server with
      prefix sharing passes today): every sequence's workgroups walk the prefix again, from L2 / Infinity Cache at best.
  B = flash_attention_n_kvcache_shared_prefix on the same pool and tables with `prefix_table` / `prefix_len`: the prefix pass, the
      suffix pass and the combine.

Both go through their Python front ends, captured in a HIP graph of REPS calls so that host time is out of the picture; the graphs are
replayed alternating A / B / A / B and timed with device events. Reported: microseconds per call for every alternation, B's speed-up over
A, A's own spread between its alternations (the margin B is judged against) and max |A - B|. Two more graphs of B bound the launches:
"B empty" - every length and the prefix length 0, three launches that walk nothing - and "B prefix" - every length equal to P, so the
suffix pass walks nothing; B prefix - B empty is the prefix pass's walk alone.
usage: python tools/bench_kvshared.py [--rounds N] [--iters N] [--only I] [--trace N]
(--trace N: no timing - N eager calls of B per selected shape, for a kernel trace taken by a profiler in a run of its own)"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256
REPS = 10


# (name, B, H, Hkv, D, prefix keys, suffix lengths)
def shapes():
    out = []
    for B, H, Hkv, D in ((64, 64, 8, 64), (64, 16, 16, 128)):
        ragged = [64 + (b * (512 - 64)) // (B - 1) for b in range(B)]
        out.append((f"({B},{H}/{Hkv},1,D={D}) P=8192 +64..512", B, H, Hkv, D, 8192, ragged))
        out.append((f"({B},{H}/{Hkv},1,D={D}) P=1024 +4096", B, H, Hkv, D, 1024, [4096] * B))
    out.append(("(1,64/8,1,D=64) P=8192 +512", 1, 64, 8, 64, 8192, [512]))
    out.append(("(1,16/16,1,D=128) P=8192 +512", 1, 16, 16, 128, 8192, [512]))
    return out


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            out = fn()
    return g, out


def time_graph(g, iters):
    for _ in range(3):
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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--trace", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvshared needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    print(f"device: {torch.cuda.get_device_name(0)}; {REPS} calls per graph, {args.iters} replays per timing, {args.rounds} alternations A/B")
    print(f"{'shape (B,H/Hkv,Sq,D) prefix +suffix':40s} {'A us':>22s} {'B us':>22s} {'A/B':>6s} {'A spread':>9s} {'B empty':>8s} {'B prefix':>9s} {'walk':>7s} {'max|A-B|':>9s}")
    for idx, (name, B, H, Hkv, D, P, suffix) in enumerate(shapes()):
        if args.only is not None and idx != args.only:
            continue
        torch.manual_seed(0)
        ppages = P // PAGE
        max_pages = ppages + (max(suffix) + PAGE - 1) // PAGE
        own = max_pages - ppages
        num_pages = ppages + B * own
        q = torch.randn(B, H, 1, D, device=dev, dtype=dtype) * 0.5
        pool_k = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        pool_v = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        ids = torch.randperm(num_pages, device=dev).to(torch.int32)
        prefix_table = ids[:ppages].contiguous()
        table = torch.cat([prefix_table.view(1, -1).expand(B, -1), ids[ppages:].view(B, own)], 1).contiguous()
        sl = torch.tensor([P + s for s in suffix], dtype=torch.int32, device=dev)
        plen = torch.tensor([P], dtype=torch.int32, device=dev)
        zero_len, zero_p, only_p = torch.zeros_like(sl), torch.zeros_like(plen), torch.full_like(sl, P)

        def run_a():
            return fa.flash_attention_n_kvcache(q, pool_k, pool_v, sl, block_table=table)

        def run_b(lens=sl, p=plen):
            return fa.flash_attention_n_kvcache_shared_prefix(q, pool_k, pool_v, lens, table, prefix_table, p)

        with torch.no_grad():
            if args.trace:
                for _ in range(args.trace):
                    run_b()
                torch.cuda.synchronize()
                print(f"{name}: {args.trace} eager calls of B")
                continue
            ga, oa = graph_of(run_a)
            gb, ob = graph_of(run_b)
            ge, _ = graph_of(lambda: run_b(zero_len, zero_p))
            gp, _ = graph_of(lambda: run_b(only_p, plen))
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(time_graph(ga, args.iters))
                tb.append(time_graph(gb, args.iters))
            te, tp = time_graph(ge, args.iters), time_graph(gp, args.iters)
            torch.cuda.synchronize()
            diff = (oa.float() - ob.float()).abs().max().item()
        a_med, b_med = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
        fmt = lambda ts: "/".join(f"{t:.1f}" for t in ts)   # noqa: E731
        print(f"{name:40s} {fmt(ta):>22s} {fmt(tb):>22s} {a_med / b_med:6.2f} {max(ta) / min(ta):9.3f} {te:8.1f} {tp:9.1f} {tp - te:7.1f} {diff:9.2e}", flush=True)
        del ga, gb, ge, gp, pool_k, pool_v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
