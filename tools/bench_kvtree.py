"""Token-tree attention over the K/V cache (flash_attention_n_kvcache_tree): what the tree costs inside the cache kernels, and what it
saves over the route a caller had. Same box, same process, three shapes on an 8192-key paged cache (bf16, page 256, shuffled block table,
lengths in device memory, per-head n): a 16-node tree on a GQA layer (64 query heads on 8 K/V heads, D = 64), a 64-node tree on an MHA
layer (16 heads, D = 128), and the 16-node tree under window = 128. The nodes are cache rows already (no append in any route).

  B  = flash_attention_n_kvcache_tree with a random tree (ancestor closure plus self per node).
  A0 = the base call on the same shape with no tree - flash_attention_n_kvcache(is_causal=True) at the same Sq, under a window
       flash_attention_n_kvcache_window: the same tiles, the same split plan, another mask on the one or two tiles that hold the nodes.
  A1 = the route the tree call replaces, ALL of it captured: the pages -> dense gather through the block table, the dense boolean mask
       [B, 1, Sq, S] built on the device from the lengths and the words, and flash_attention_n with that mask.

All go through their Python front ends, captured in a HIP graph of REPS calls so that host time is out of the picture; the graphs are
replayed alternating A0 / B / A1 and timed with device events. Reported: microseconds per call for every alternation, B/A0 next to A0's
own spread between its alternations (the margin B is judged against), B/A1 (ratios of medians, < 1 = B is faster) and max |A1 - B|.
usage: python tools/bench_kvtree.py [--rounds N] [--iters N] [--only SUBSTRING] [--out FILE]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256


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
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvtree needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"device: {torch.cuda.get_device_name(0)}; {args.iters} replays per timing, {args.rounds} alternations A0 / B / A1")
    say(f"{'shape (B,H[/Hkv],nodes,S,D)':36s} {'A0 us':>22s} {'B us':>22s} {'A1 us':>25s} {'B/A0':>6s} {'A0 spread':>9s} {'B/A1':>6s} {'max|A1-B|':>9s}")
    gen = torch.Generator().manual_seed(0)
    for name, B, H, Hkv, Sq, S, D, W, reps in shapes():
        if args.only not in name:
            continue
        torch.manual_seed(0)
        max_pages = (S + PAGE - 1) // PAGE
        num_pages = B * max_pages
        q = torch.randn(B, H, Sq, D, device=dev, dtype=dtype) * 0.5
        pool_k = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        pool_v = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        table = torch.randperm(num_pages, device=dev).to(torch.int32).view(B, max_pages)
        tl = table.long()
        sl = torch.full((B,), S, dtype=torch.int32, device=dev)
        n = torch.rand(H, device=dev) + 0.5
        words = random_tree_words(B, Sq, gen).to(dev)
        tbits = torch.arange(64, device=dev).view(1, 1, 64)
        jj = torch.arange(S, device=dev).view(1, 1, S)

        def make_mask():   # the rule of the tree call, from the lengths and the words in device memory
            base = (sl.long() - Sq).view(B, 1, 1)
            bits = ((words.unsqueeze(-1) >> tbits) & 1) != 0                                       # [B, Sq, 64]
            bits = bits & (tbits < Sq)
            p = base + (bits.sum(-1, keepdim=True) - 1).clamp_min(0)
            prefix = jj < base
            if W is not None:
                prefix = prefix & (jj > p - W)
            t = jj - base
            new = (t >= 0) & (t < Sq) & torch.gather(bits, 2, t.clamp(0, 63).expand(B, Sq, S))
            return (prefix | new).view(B, 1, Sq, S)

        def run_a0():
            if W is not None:
                return fa.flash_attention_n_kvcache_window(q, pool_k, pool_v, sl, W, block_table=table, softmax_n_param=n)
            return fa.flash_attention_n_kvcache(q, pool_k, pool_v, sl, block_table=table, softmax_n_param=n, is_causal=True)

        def run_b():
            return fa.flash_attention_n_kvcache_tree(q, pool_k, pool_v, sl, words, block_table=table, softmax_n_param=n, window=W)

        def run_a1():
            kd = pool_k[tl].reshape(B, max_pages * PAGE, Hkv, D)[:, :S].permute(0, 2, 1, 3).contiguous()
            vd = pool_v[tl].reshape(B, max_pages * PAGE, Hkv, D)[:, :S].permute(0, 2, 1, 3).contiguous()
            return fa.flash_attention_n(q, kd, vd, softmax_n_param=n, attn_mask=make_mask())

        with torch.no_grad():
            g0, _o0 = graph_of(run_a0, reps)
            gb, ob = graph_of(run_b, reps)
            g1, o1 = graph_of(run_a1, 1)
            t0, tb, t1 = [], [], []
            for _ in range(args.rounds):
                t0.append(time_graph(g0, args.iters, reps))
                tb.append(time_graph(gb, args.iters, reps))
                t1.append(time_graph(g1, max(2, args.iters // 2), 1))
            torch.cuda.synchronize()
            diff = (o1.float() - ob.float()).abs().max().item()
        med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
        fmt = lambda ts: "/".join(f"{t:.1f}" for t in ts)   # noqa: E731
        say(f"{name:36s} {fmt(t0):>22s} {fmt(tb):>22s} {fmt(t1):>25s} {med(tb) / med(t0):6.3f} {max(t0) / min(t0):9.3f} {med(tb) / med(t1):6.3f} {diff:9.2e}")
        del g0, gb, g1, pool_k, pool_v, ob, o1, _o0
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
