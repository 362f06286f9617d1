"""K/V-cache decode: flash_attention_n_kvcache on a paged cache (B) against the route the package offered before it (A), same box, same process.

  A = flash_attention_n on dense K/V [B, Hkv, S, D] of the same lengths with a key-padding mask (scalar n: the regrouped split-K launch;
      tensor n: the per-query-head launch, which reads K/V once per query head). The gather a paged caller needs first (pages -> dense)
      is timed separately and reported, NOT added to A.
  B = flash_attention_n_kvcache on the paged cache (page 256, shuffled block table, lengths in device memory).

Both go through their Python front ends, captured in a HIP graph of REPS calls so that host time is out of the picture; the graphs are
replayed alternating A / B / A / B and timed with device events. Reported: microseconds per call for every alternation, the K+V bytes
actually visible (sum_b len_b * Hkv * D * 2 tensors * 2 bytes) per second, B's speed-up over A, and A's own spread between its alternations
(the margin B is judged against). usage: python tools/bench_kvcache.py [--rounds N] [--iters N]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256
REPS = 10

# (name, B, H, Hkv, Sq, lengths, D, tensor n)
def shapes():
    out = []
    for B, H, Sq, Sk, D in [(1, 8, 1, 8192, 128), (1, 32, 1, 32768, 128), (8, 16, 1, 4096, 64), (4, 32, 16, 8192, 128), (1, 16, 128, 16384, 64), (64, 16, 1, 8192, 128)]:
        out.append((f"({B},{H},{Sq},{Sk},{D})", B, H, H, Sq, [Sk] * B, D, False))
    out.append(("(4,64/8,1,8192,64) n[H]", 4, 64, 8, 1, [8192] * 4, 64, True))
    ragged = [2048 + (b * (8192 - 2048)) // 31 for b in range(32)]
    out.append(("(32,64/8,1,2048..8192,64) n[H]", 32, 64, 8, 1, ragged, 64, True))
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
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvcache needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    print(f"device: {torch.cuda.get_device_name(0)}; {REPS} calls per graph, {args.iters} replays per timing, {args.rounds} alternations A/B")
    print(f"{'shape (B,H[/Hkv],Sq,S,D)':34s} {'A us':>24s} {'B us':>24s} {'A TB/s':>7s} {'B TB/s':>7s} {'B/A':>6s} {'A spread':>9s} {'gather us':>10s} {'max|A-B|':>9s}")
    for name, B, H, Hkv, Sq, lens, D, tensor_n in shapes():
        torch.manual_seed(0)
        S = max(lens)
        max_pages = (S + PAGE - 1) // PAGE
        q = torch.randn(B, H, Sq, D, device=dev, dtype=dtype) * 0.5
        num_pages = B * max_pages
        pool_k = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        pool_v = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        table = torch.randperm(num_pages, device=dev).to(torch.int32).view(B, max_pages)
        sl = torch.tensor(lens, dtype=torch.int32, device=dev)
        n = (torch.rand(H, device=dev) + 0.5) if tensor_n else 1.0

        def gather():
            kd = pool_k[table.long()].reshape(B, max_pages * PAGE, Hkv, D)[:, :S].permute(0, 2, 1, 3).contiguous()
            vd = pool_v[table.long()].reshape(B, max_pages * PAGE, Hkv, D)[:, :S].permute(0, 2, 1, 3).contiguous()
            return kd, vd

        kd, vd = gather()
        keypad = torch.arange(S, device=dev).view(1, 1, 1, S) < sl.view(B, 1, 1, 1)

        def run_a():
            return fa.flash_attention_n(q, kd, vd, softmax_n_param=n, attn_mask=keypad)

        def run_b():
            return fa.flash_attention_n_kvcache(q, pool_k, pool_v, sl, block_table=table, softmax_n_param=n, is_causal=False)

        with torch.no_grad():
            ga, oa = graph_of(run_a)
            gb, ob = graph_of(run_b)
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(time_graph(ga, args.iters))
                tb.append(time_graph(gb, args.iters))
            torch.cuda.synchronize()
            diff = (oa.float() - ob.float()).abs().max().item()
            for _ in range(2):
                gather()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                gather()
            e1.record()
            torch.cuda.synchronize()
            tg = e0.elapsed_time(e1) * 1e3 / 5
        visible = sum(lens) * Hkv * D * 2 * 2
        a_med, b_med = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
        fmt = lambda ts: "/".join(f"{t:.1f}" for t in ts)   # noqa: E731
        print(f"{name:34s} {fmt(ta):>24s} {fmt(tb):>24s} {visible / a_med / 1e6:7.2f} {visible / b_med / 1e6:7.2f} {a_med / b_med:6.2f} "
              f"{max(ta) / min(ta):9.3f} {tg:10.1f} {diff:9.2e}", flush=True)
        del ga, gb, kd, vd, pool_k, pool_v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
