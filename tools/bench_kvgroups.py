"""Decode behind several shared prefixes: flash_attention_n_kvcache_prefix_groups (B) against the two routes the package offered before
it (A, A1), same box, same process.

  A  = flash_attention_n_kvcache on block tables whose first slots name the prefix pages of the sequence's group: every sequence's
       workgroups walk their prefix again.
  A1 = the host-side split this call replaces, all of it captured in ONE graph: one flash_attention_n_kvcache_shared_prefix call per
       group on its sub-batch (queries, lengths and tables gathered beforehand, outside the timing) plus the base call for the
       ungrouped sequences.
  B  = flash_attention_n_kvcache_prefix_groups on the whole batch: schedule, prefix pass, suffix pass, combine.

All go through their Python front ends, captured in a HIP graph of REPS calls so that host time is out of the picture; the graphs are
replayed alternating A / A1 / B and timed with device events. Reported: microseconds per call for every alternation, B's speed-up over A
and over A1 (below 1: B is slower), A's and A1's own spread between their alternations (the margin B is judged against), and
max |A - B|. Two more graphs bound the launches: "B empty" - every length 0 and nobody grouped: four launches that walk nothing - and
"S empty", the same of the single-prefix call (three launches). The schedule kernel's own time comes from a kernel trace (--trace).
usage: python tools/bench_kvgroups.py [--rounds N] [--iters N] [--only I] [--trace N]
(--trace N: no timing - N eager calls of B per selected shape, for a kernel trace taken by a profiler in a run of its own)"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256
REPS = 10
P = 8192


# (name, B, H, Hkv, D, group of every sequence (-1: none), G)
def shapes():
    out = []
    for B, H, Hkv, D in ((64, 64, 8, 64), (64, 16, 16, 128)):
        head = f"({B},{H}/{Hkv},1,D={D})"
        out.append((f"{head} 4 groups of 16", B, H, Hkv, D, [b % 4 for b in range(B)], 4))
        out.append((f"{head} 4 groups of 12, 16 alone", B, H, Hkv, D, [b % 4 if b < B - 16 else -1 for b in range(B)], 4))
        out.append((f"{head} 1 group of 64", B, H, Hkv, D, [0] * B, 1))
        out.append((f"{head} 64 groups of 1", B, H, Hkv, D, list(range(B)), 64))
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--trace", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvgroups needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    print(f"device: {torch.cuda.get_device_name(0)}; bf16, page {PAGE}, prefixes of {P} keys, suffixes of 64..512 keys; {REPS} calls per graph, "
          f"{args.iters} replays per timing, {args.rounds} alternations A/A1/B")
    print(f"{'shape (B,H/Hkv,Sq,D) groups':44s} {'A us':>22s} {'A1 us':>22s} {'B us':>22s} {'A/B':>6s} {'A1/B':>6s} {'A spread':>9s} {'A1 spread':>9s} "
          f"{'B empty':>8s} {'S empty':>8s} {'max|A-B|':>9s}")
    for idx, (name, B, H, Hkv, D, group, G) in enumerate(shapes()):
        if args.only is not None and idx != args.only:
            continue
        torch.manual_seed(0)
        suffix = [64 + (b * (512 - 64)) // (B - 1) for b in range(B)]
        ppages = P // PAGE
        own = (max(suffix) + PAGE - 1) // PAGE
        max_pages = ppages + own
        num_pages = G * ppages + B * max_pages   # (an ungrouped sequence owns its first P keys)
        q = torch.randn(B, H, 1, D, device=dev, dtype=dtype) * 0.5
        pool_k = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        pool_v = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        ids = torch.randperm(num_pages, device=dev).to(torch.int32)
        prefix_tables = ids[:G * ppages].view(G, ppages).contiguous()
        table = ids[G * ppages:].view(B, max_pages).clone()
        for b, g in enumerate(group):
            if g >= 0:
                table[b, :ppages] = prefix_tables[g]
        table = table.contiguous()
        sl = torch.tensor([P + s for s in suffix], dtype=torch.int32, device=dev)
        plens = torch.full((G,), P, dtype=torch.int32, device=dev)
        pgroup = torch.tensor(group, dtype=torch.int32, device=dev)
        # the host-side split: the sub-batch of every group, and of the ungrouped sequences
        subs = []
        for g in sorted(set(group)):
            idxs = torch.tensor([b for b in range(B) if group[b] == g], device=dev)
            subs.append((g, q[idxs].contiguous(), sl[idxs].contiguous(), table[idxs].contiguous()))
        one_len = torch.tensor([P], dtype=torch.int32, device=dev)
        zero_len, nobody = torch.zeros_like(sl), torch.full_like(pgroup, -1)

        def run_a():
            return fa.flash_attention_n_kvcache(q, pool_k, pool_v, sl, block_table=table)

        def run_a1():
            outs = []
            for g, qg, slg, tg in subs:
                if g < 0:
                    outs.append(fa.flash_attention_n_kvcache(qg, pool_k, pool_v, slg, block_table=tg))
                else:
                    outs.append(fa.flash_attention_n_kvcache_shared_prefix(qg, pool_k, pool_v, slg, tg, prefix_tables[g], one_len))
            return outs

        def run_b(lens=sl, grp=pgroup):
            return fa.flash_attention_n_kvcache_prefix_groups(q, pool_k, pool_v, lens, table, prefix_tables, plens, grp)

        def run_single_empty():
            return fa.flash_attention_n_kvcache_shared_prefix(q, pool_k, pool_v, zero_len, table, prefix_tables[0], torch.zeros_like(one_len))

        with torch.no_grad():
            if args.trace:
                for _ in range(args.trace):
                    run_b()
                torch.cuda.synchronize()
                print(f"{name}: {args.trace} eager calls of B")
                continue
            ga, oa = graph_of(run_a)
            g1, _ = graph_of(run_a1)
            gb, ob = graph_of(run_b)
            ge, _ = graph_of(lambda: run_b(zero_len, nobody))
            gs, _ = graph_of(run_single_empty)
            ta, t1, tb = [], [], []
            for _ in range(args.rounds):
                ta.append(time_graph(ga, args.iters))
                t1.append(time_graph(g1, args.iters))
                tb.append(time_graph(gb, args.iters))
            te, ts = time_graph(ge, args.iters), time_graph(gs, args.iters)
            torch.cuda.synchronize()
            diff = (oa.float() - ob.float()).abs().max().item()
        med = lambda ts_: sorted(ts_)[len(ts_) // 2]   # noqa: E731
        fmt = lambda ts_: "/".join(f"{t:.1f}" for t in ts_)   # noqa: E731
        print(f"{name:44s} {fmt(ta):>22s} {fmt(t1):>22s} {fmt(tb):>22s} {med(ta) / med(tb):6.2f} {med(t1) / med(tb):6.2f} {max(ta) / min(ta):9.3f} "
              f"{max(t1) / min(t1):9.3f} {te:8.1f} {ts:8.1f} {diff:9.2e}", flush=True)
        del ga, g1, gb, ge, gs, pool_k, pool_v, subs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
