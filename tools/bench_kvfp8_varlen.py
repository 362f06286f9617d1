"""Continuous-batching steps over an FP8 K/V cache: flash_attention_n_kvcache_fp8_varlen on token-packed queries (B) against the same step
on a bf16 cache (A) and against the route an FP8 cache had for a packed step (A2), same box, same process.

  B  = flash_attention_n_kvcache_fp8_varlen on the packed buffer, over the quantisation of the cache: one scale per (sequence, K/V head)
       = absmax / 448 over the sequence's pages.
  A  = flash_attention_n_kvcache_varlen on the bf16 cache of the same content.
  A2 = pad scatter (token -> [sequence, position], index tensors on the device) into an UNINITIALISED [B, Sq, H, D] buffer, then
       flash_attention_n_kvcache_fp8 with query_seqlens, then the gather back to [T, H, D]. All captured.

Steps (bf16 queries, page 256, per-head n, cache rows already appended; tools/bench_kvvarlen.py's): (a) one chunk of 2048 tokens behind
6144 cached keys plus 255 decode tokens over 2048 .. 8192 keys; (b) 256 decode tokens over 2048 .. 8192 keys; (c) 4 chunks of 2048 tokens
behind 6144 keys. Shapes (64/8, 64) and (16/16, 128).

All go through their Python front ends, captured in a HIP graph of REPS calls; the graphs are replayed alternating A / B / A2 and timed with
device events. Reported: microseconds per call of every alternation, B/A and B/A2 (ratios of medians, < 1 = B is faster), A's and A2's own
spread between their alternations (the margins B is judged against), whether B equals A2 bit for bit, max |B - A| over the real tokens (the
quantisation of the cache) and the peak extra device memory of one eager call of B and of A2 (torch's allocator statistics). The table is
also written to profiles/kvfp8_varlen_<first 8 hex digits of the library's sha256>_summary.txt.
usage: python tools/bench_kvfp8_varlen.py [--rounds N] [--iters N] [--only SUBSTRING] [--out FILE]"""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256
REPS = 4
F8 = torch.float8_e4m3fn


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


def quantise(pool, scale_ph):
    """[pages, PAGE, Hkv, D] 16-bit -> codes, one scale per (page, K/V head): clamp before the cast (torch's cast does not saturate)"""
    return (pool.float() / scale_ph[:, None, :, None]).clamp(-448.0, 448.0).to(F8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvfp8_varlen needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    sha = hashlib.sha256(open(fa._lib.LIB_PATH, "rb").read()).hexdigest()
    out_path = args.out or os.path.join(ROOT, "profiles", f"kvfp8_varlen_{sha[:8]}_summary.txt")
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit(f"device: {torch.cuda.get_device_name(0)}; library sha256 {sha[:8]}; {REPS} calls per graph, {args.iters} replays per timing, "
         f"{args.rounds} alternations A / B / A2")
    emit(f"{'step (H/Hkv,D)':44s} {'A us':>26s} {'B us':>26s} {'A2 us':>26s} {'B/A':>6s} {'B/A2':>6s} {'A spread':>9s} {'A2 spread':>9s} {'B==A2':>6s} "
         f"{'max|B-A|':>9s} {'B MiB':>8s} {'A2 MiB':>8s}")
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
            owner = torch.empty(num_pages, dtype=torch.long)
            for b in range(B):   # shuffled pages; entries beyond a sequence's pages are never read
                mine = [ids.pop() for _ in range(need[b])]
                table[b, :need[b]] = torch.tensor(mine, dtype=torch.int32)
                owner[mine] = b
            table, owner = table.to(dev), owner.to(dev)
            k_scale = torch.zeros(B, Hkv, device=dev).index_reduce_(0, owner, pool_k.float().abs().amax((1, 3)), "amax") / 448.0
            v_scale = torch.zeros(B, Hkv, device=dev).index_reduce_(0, owner, pool_v.float().abs().amax((1, 3)), "amax") / 448.0
            k8, v8 = quantise(pool_k, k_scale[owner]), quantise(pool_v, v_scale[owner])
            sl = torch.tensor(lens, dtype=torch.int32, device=dev)
            ql = torch.tensor(qlens, dtype=torch.int32, device=dev)
            cu = torch.tensor([0] + torch.tensor(qlens).cumsum(0).tolist(), dtype=torch.int32, device=dev)
            b_idx = torch.repeat_interleave(torch.arange(B, device=dev), ql.long())
            i_idx = torch.arange(T, device=dev) - cu[:-1].long()[b_idx]
            n = torch.rand(H, device=dev) + 0.5

            def run_a():
                return fa.flash_attention_n_kvcache_varlen(q, pool_k, pool_v, sl, cu, Sq, block_table=table, softmax_n_param=n)

            def run_b():
                return fa.flash_attention_n_kvcache_fp8_varlen(q, k8, v8, sl, k_scale, v_scale, cu, Sq, block_table=table, softmax_n_param=n)

            def run_a2():
                qp = torch.empty(B, Sq, H, D, device=dev, dtype=dtype)
                qp[b_idx, i_idx] = q
                o = fa.flash_attention_n_kvcache_fp8(qp.transpose(1, 2), k8, v8, sl, k_scale, v_scale, block_table=table, query_seqlens=ql,
                                                     softmax_n_param=n)
                return o.transpose(1, 2)[b_idx, i_idx]

            with torch.no_grad():
                mem_b, mem_a2 = peak_extra(run_b), peak_extra(run_a2)
                ga, oa = graph_of(run_a)
                gb, ob = graph_of(run_b)
                g2, o2 = graph_of(run_a2)
                ta, tb, t2 = [], [], []
                for _ in range(args.rounds):
                    ta.append(time_graph(ga, args.iters))
                    tb.append(time_graph(gb, args.iters))
                    t2.append(time_graph(g2, args.iters))
                torch.cuda.synchronize()
                same = "yes" if torch.equal(ob.view(torch.int16), o2.view(torch.int16)) else f"{(ob.float() - o2.float()).abs().max().item():.0e}"
                diff = (oa.float() - ob.float()).abs().max().item()
            emit(f"{name:44s} {fmt(ta):>26s} {fmt(tb):>26s} {fmt(t2):>26s} {med(tb) / med(ta):6.2f} {med(tb) / med(t2):6.2f} {max(ta) / min(ta):9.3f} "
                 f"{max(t2) / min(t2):9.3f} {same:>6s} {diff:9.2e} {mem_b:8.1f} {mem_a2:8.1f}")
            del ga, gb, g2, pool_k, pool_v, k8, v8, oa, ob, o2
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written to {out_path}")


if __name__ == "__main__":
    main()
