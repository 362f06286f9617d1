"""Token-tree attention over the FP8 K/V cache (flash_attention_n_kvcache_fp8_tree): what the tree costs inside the FP8 cache kernels, what
the FP8 cache costs or saves against the 16-bit tree call, and what the call saves over the route an FP8 cache had. Same box, same process,
the shapes of tools/bench_kvtree.py on an 8192-key paged cache (bf16 queries, page 256, shuffled block table, lengths in device memory,
per-head n, one power-of-two scale per (batch element, K/V head) so that both caches hold the same values): a 16-node tree on a GQA layer
(64 query heads on 8 K/V heads, D = 64), a 64-node tree on an MHA layer (16 heads, D = 128), and the 16-node tree under window = 128. The
nodes are cache rows already (no append in any route).

  B  = flash_attention_n_kvcache_fp8_tree with a random tree (ancestor closure plus self per node).
  A0 = the FP8 call on the same shape with no tree - flash_attention_n_kvcache_fp8(is_causal=True) at the same Sq, under a window
       flash_attention_n_kvcache_fp8_window: the same tiles, the same split plan, another mask on the one or two tiles that hold the nodes.
  A  = flash_attention_n_kvcache_tree on a bf16 cache of the same content: twice the cache bytes, no widening pass.
  A2 = the route the call replaces, ALL of it captured: the pages the call can see (all of them; under the window those the window of the
       shallowest node reaches) dequantised into a bf16 pool - upcast times the page's scale - then flash_attention_n_kvcache_tree on it.

All go through their Python front ends, captured in a HIP graph of REPS calls so that host time is out of the picture; the graphs are
replayed alternating A0 / B / A and timed with device events; A2 - 7 to 25 times as long, all of it memory traffic - is timed the same way
once the alternations are over, so that it does not sit in front of A0 in every alternation: a graph timed right behind that traffic
reads 2 - 4 % slow (--a2-inside puts A2 back there and shows it). Reported: microseconds per call for every alternation, B/A0 next to
A0's own spread between its alternations (the margin B is judged against), B/A and B/A2 (ratios of medians, < 1 = B is faster) and
max |A - B|, max |A2 - B|.
usage: python tools/bench_kvfp8_tree.py [--rounds N] [--iters N] [--only SUBSTRING] [--a2-inside] [--out FILE]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256
F8 = torch.float8_e4m3fn


# (name, B, H, Hkv, nodes, cache length (the nodes included), D, window, calls per graph)
def shapes():
    return [
        ("tree16 (64,64/8,16,8192,64)", 64, 64, 8, 16, 8192, 64, None, 10),
        ("tree64 (64,16/16,64,8192,128)", 64, 16, 16, 64, 8192, 128, None, 4),
        ("tree16 (64,64/8,16,8192,64) W=128", 64, 64, 8, 16, 8192, 64, 128, 10),
    ]


def random_tree_words(B, Sq, gen):
    """int64 [B, Sq]: a random parent among the earlier nodes, a row = its ancestors plus itself"""
    rows = []
    for _ in range(B):
        words = []
        for i in range(Sq):
            par = -1 if i == 0 else int(torch.randint(0, i, (1,), generator=gen))
            words.append((1 << i) | (words[par] if par >= 0 else 0))
        rows.append([w - (1 << 64) if w >> 63 else w for w in words])
    return torch.tensor(rows, dtype=torch.int64)


def random_codes(shape, dev):
    """finite e4m3fn codes, |value| <= 3, either sign, as uint8"""
    mag = torch.randint(0, 0x49, shape, device=dev, dtype=torch.int32)
    sign = torch.randint(0, 2, shape, device=dev, dtype=torch.int32) << 7
    return (mag | sign).to(torch.uint8)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--a2-inside", action="store_true", help="time A2 inside every alternation, behind A and in front of the next A0")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvfp8_tree needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"device: {torch.cuda.get_device_name(0)}; {args.iters} replays per timing, {args.rounds} alternations A0 / B / A"
        + (" / A2" if args.a2_inside else ", then A2"))
    say(f"{'shape (B,H[/Hkv],nodes,S,D)':36s} {'A0 us':>22s} {'B us':>22s} {'A us':>22s} {'A2 us':>25s} {'B/A0':>6s} {'A0 spread':>9s} {'B/A':>6s} {'B/A2':>6s} "
        f"{'max|A-B|':>9s} {'max|A2-B|':>9s}")
    gen = torch.Generator().manual_seed(0)
    for name, B, H, Hkv, Sq, S, D, W, reps in shapes():
        if args.only not in name:
            continue
        torch.manual_seed(0)
        max_pages = (S + PAGE - 1) // PAGE
        num_pages = B * max_pages
        q = torch.randn(B, H, Sq, D, device=dev, dtype=dtype) * 0.5
        pool8_k, pool8_v = random_codes((num_pages, PAGE, Hkv, D), dev), random_codes((num_pages, PAGE, Hkv, D), dev)
        table = torch.randperm(num_pages, device=dev).to(torch.int32).view(B, max_pages)
        tl = table.long()
        sl = torch.full((B,), S, dtype=torch.int32, device=dev)
        n = torch.rand(H, device=dev) + 0.5
        words = random_tree_words(B, Sq, gen).to(dev)
        k_scale = 2.0 ** torch.randint(-1, 2, (B, Hkv), device=dev).float()
        v_scale = 2.0 ** torch.randint(-1, 2, (B, Hkv), device=dev).float()
        # the scale of a page is the scale of the batch element that owns it; the pages a call can see
        page_ks, page_vs = torch.ones(num_pages, Hkv, device=dev), torch.ones(num_pages, Hkv, device=dev)
        page_ks[tl.flatten()] = k_scale.repeat_interleave(max_pages, dim=0)
        page_vs[tl.flatten()] = v_scale.repeat_interleave(max_pages, dim=0)
        lo = 0 if W is None else max(0, S - Sq - W + 1) // PAGE
        seen = tl[:, lo:].reshape(-1)
        # A: the bf16 cache of the same content (exact: a code times a power of two is a bf16 number)
        pool_k = pool8_k.view(F8).to(dtype) * page_ks[:, None, :, None].to(dtype)
        pool_v = pool8_v.view(F8).to(dtype) * page_vs[:, None, :, None].to(dtype)
        # A2: its own bf16 pool, filled inside the graph
        deq_k, deq_v = torch.zeros_like(pool_k), torch.zeros_like(pool_v)
        k8, v8 = pool8_k.view(F8), pool8_v.view(F8)

        def run_a0():
            if W is not None:
                return fa.flash_attention_n_kvcache_fp8_window(q, k8, v8, sl, k_scale, v_scale, W, block_table=table, softmax_n_param=n)
            return fa.flash_attention_n_kvcache_fp8(q, k8, v8, sl, k_scale, v_scale, block_table=table, softmax_n_param=n, is_causal=True)

        def run_b():
            return fa.flash_attention_n_kvcache_fp8_tree(q, k8, v8, sl, k_scale, v_scale, words, block_table=table, softmax_n_param=n, window=W)

        def run_a():
            return fa.flash_attention_n_kvcache_tree(q, pool_k, pool_v, sl, words, block_table=table, softmax_n_param=n, window=W)

        def run_a2():
            deq_k.index_copy_(0, seen, k8[seen].to(dtype) * page_ks[seen][:, None, :, None].to(dtype))
            deq_v.index_copy_(0, seen, v8[seen].to(dtype) * page_vs[seen][:, None, :, None].to(dtype))
            return fa.flash_attention_n_kvcache_tree(q, deq_k, deq_v, sl, words, block_table=table, softmax_n_param=n, window=W)

        with torch.no_grad():
            g0, _o0 = graph_of(run_a0, reps)
            gb, ob = graph_of(run_b, reps)
            ga, oa = graph_of(run_a, reps)
            g2, o2 = graph_of(run_a2, 1)
            t0, tb, ta, t2 = [], [], [], []
            for _ in range(args.rounds):
                t0.append(time_graph(g0, args.iters, reps))
                tb.append(time_graph(gb, args.iters, reps))
                ta.append(time_graph(ga, args.iters, reps))
                if args.a2_inside:
                    t2.append(time_graph(g2, max(2, args.iters // 2), 1))
            while len(t2) < args.rounds:
                t2.append(time_graph(g2, max(2, args.iters // 2), 1))
            torch.cuda.synchronize()
            diff_a = (oa.float() - ob.float()).abs().max().item()
            diff_2 = (o2.float() - ob.float()).abs().max().item()
        med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
        fmt = lambda ts: "/".join(f"{t:.1f}" for t in ts)   # noqa: E731
        say(f"{name:36s} {fmt(t0):>22s} {fmt(tb):>22s} {fmt(ta):>22s} {fmt(t2):>25s} {med(tb) / med(t0):6.3f} {max(t0) / min(t0):9.3f} "
            f"{med(tb) / med(ta):6.3f} {med(tb) / med(t2):6.3f} {diff_a:9.2e} {diff_2:9.2e}")
        del g0, gb, ga, g2, pool_k, pool_v, deq_k, deq_v, pool8_k, pool8_v, k8, v8, ob, oa, o2, _o0
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
