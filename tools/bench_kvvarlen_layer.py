"""One layer step of a served GPT-OSS / Mistral / Llama model on a continuous-batching step: rotate, append, attend (with or without a
sliding window). flash_attention_n_kvcache_varlen_rope on token-packed buffers (B) against the route it replaces (A), same box, same
process.

  A = pad scatter of query, k_new and v_new (token -> [sequence, position], index tensors on the device) into UNINITIALISED
      [B, Sq, heads, D] buffers - the padded call never reads a padding row, so A pays for no zero fill - then
      flash_attention_n_kvcache_rope(..., query_seqlens=, window=), then the gather back to [T, H, D]. All captured.
  B = flash_attention_n_kvcache_varlen_rope(..., window=) on the packed buffers.
  rope = the one launch of fasn_kvvarlen_rope_append alone (B's first launch), through the C ABI.

Steps (bf16, page 256, per-head n, fp32 tables, rotary_dim = D): those of tools/bench_kvvarlen.py, with the step's tokens appended - (a) one
chunk of 2048 tokens behind 6144 cached keys plus 255 decode tokens behind 2047 .. 8191 keys; (b) 256 decode tokens behind 2047 .. 8191
keys; (c) 4 chunks of 2048 tokens behind 6144 keys. Shapes: (H/Hkv, D) = (64/8, 64) with window=128 and window=None, (16/16, 128) with
window=None. Both routes write the same rotated rows to the same cache rows, so they share the pools and every replay finds the same cache.

All go through their Python front ends, captured in a HIP graph of REPS calls; the graphs are replayed alternating and timed with device
events. Reported: microseconds per call of every alternation, B/A (ratio of medians, < 1 = B is faster), A's own spread between its
alternations (max / min: the margin B is judged against), the verdict under that margin, max |A - B| over the real tokens, the peak extra
device memory of one eager call of each route (torch's allocator statistics: outputs, temporaries and workspace), and the rope launch alone.
The table is also written to <--out>/kvvarlen_layer_<first 8 hex of libfasn.so's sha256>_summary.txt.
usage: python tools/bench_kvvarlen_layer.py [--rounds N] [--iters N] [--only SUBSTRING] [--out DIR]"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402
from bench_kvvarlen import REPS, graph_of, peak_extra, time_graph   # noqa: E402

PAGE = 256


def steps():
    spread = [2047 + (b * (8191 - 2047)) // 254 for b in range(255)]
    return [
        ("a mixed 2048@6144 + 255 x 1", [2048] + [1] * 255, [6144] + spread),
        ("b decode 256 x 1", [1] * 256, spread + [8191]),
        ("c chunks 4 x 2048@6144", [2048] * 4, [6144] * 4),
    ]


def tables(rows, rd, dev, base=10000.0):
    inv = base ** (-torch.arange(0, rd, 2, dtype=torch.float64) / rd)
    ang = torch.arange(rows, dtype=torch.float64)[:, None] * inv[None]
    return ang.cos().float().to(dev), ang.sin().float().to(dev)


def rope_alone(q, kn, vn, pool_k, pool_v, sl, cu, Sq, table, cos, sin):
    """a callable that makes the one launch of fasn_kvvarlen_rope_append on the current stream"""
    kc, ffa = fa.kvcache, fa.flash_attn
    fn = "bench_kvvarlen_layer"
    _B, _T, q4 = kc._packed_query(fn, q, pool_k, sl, cu, Sq)
    keep = kc._prepare(fn, "kvvarlen", q4, pool_k, pool_v, sl, table, kn, vn, 1.0, None, True, False, cu_seqlens_q=cu, max_seqlen_q=Sq)
    va, kn4, vn4 = keep.args, keep.k_new, keep.v_new
    rope = kc._rope_operand(cos, sin, False, q)
    q_rot = torch.empty_like(q).unsqueeze(0).transpose(1, 2)
    lib = fa._lib.load()
    views = (ffa._view4(q_rot), ffa._view4(kn4), ffa._view4(vn4))

    def run():
        fa._lib.check(lib.fasn_kvvarlen_rope_append(va, rope, *views, ffa._stream_ptr(q.device)), "fasn_kvvarlen_rope_append")
        return q_rot
    run.keep = (va, rope, keep, kn4, vn4, q4)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="profiles")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvvarlen_layer needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    sha = hashlib.sha256(open(fa._lib.LIB_PATH, "rb").read()).hexdigest()[:8]
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"tools/bench_kvvarlen_layer.py, libfasn.so sha256 {sha}; device: {torch.cuda.get_device_name(0)}; {REPS} calls per graph, "
        f"{args.iters} replays per timing, {args.rounds} alternations A / B")
    say("A = pad scatter + flash_attention_n_kvcache_rope(query_seqlens=, window=) + gather; B = flash_attention_n_kvcache_varlen_rope(window=)")
    say(f"{'step (H/Hkv,D) window':52s} {'A us':>26s} {'B us':>26s} {'B/A':>6s} {'A spread':>9s} {'verdict':>9s} {'max|A-B|':>9s} {'A MiB':>8s} "
        f"{'B MiB':>8s} {'rope us':>8s}")
    med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
    fmt = lambda ts: "/".join(f"{t:.0f}" for t in ts)   # noqa: E731
    for H, Hkv, D, W in ((64, 8, 64, 128), (64, 8, 64, None), (16, 16, 128, None)):
        for name, qlens, lens in steps():
            name = f"{name} ({H}/{Hkv},{D}) window={W}"
            if args.only not in name:
                continue
            torch.manual_seed(0)
            B, T, Sq = len(qlens), sum(qlens), max(qlens)
            total = [ln + ql for ln, ql in zip(lens, qlens)]
            max_pages = (max(total) + PAGE - 1) // PAGE
            need = [(t + PAGE - 1) // PAGE for t in total]
            num_pages = sum(need)
            q = torch.randn(T, H, D, device=dev, dtype=dtype) * 0.5
            kn = torch.randn(T, Hkv, D, device=dev, dtype=dtype) * 0.5
            vn = torch.randn(T, Hkv, D, device=dev, dtype=dtype) * 0.5
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
            cos, sin = tables(PAGE * max_pages, D, dev)

            def run_a():
                qp = torch.empty(B, Sq, H, D, device=dev, dtype=dtype)
                kp = torch.empty(B, Sq, Hkv, D, device=dev, dtype=dtype)
                vp = torch.empty(B, Sq, Hkv, D, device=dev, dtype=dtype)
                qp[b_idx, i_idx], kp[b_idx, i_idx], vp[b_idx, i_idx] = q, kn, vn
                o = fa.flash_attention_n_kvcache_rope(qp.transpose(1, 2), pool_k, pool_v, sl, cos, sin, block_table=table, k_new=kp.transpose(1, 2),
                                                      v_new=vp.transpose(1, 2), query_seqlens=ql, softmax_n_param=n, window=W)
                return o.transpose(1, 2)[b_idx, i_idx]

            def run_b():
                return fa.flash_attention_n_kvcache_varlen_rope(q, pool_k, pool_v, sl, cu, Sq, cos, sin, block_table=table, k_new=kn, v_new=vn,
                                                                softmax_n_param=n, window=W)

            with torch.no_grad():
                run_r = rope_alone(q, kn, vn, pool_k, pool_v, sl, cu, Sq, table, cos, sin)
                mem_a, mem_b = peak_extra(run_a), peak_extra(run_b)
                ga, oa = graph_of(run_a)
                gb, ob = graph_of(run_b)
                gr, _ = graph_of(run_r)
                ta, tb = [], []
                for _ in range(args.rounds):
                    ta.append(time_graph(ga, args.iters))
                    tb.append(time_graph(gb, args.iters))
                tr = time_graph(gr, args.iters)
                torch.cuda.synchronize()
                diff = (oa.float() - ob.float()).abs().max().item()
            spread = max(ta) / min(ta)
            ratio = med(tb) / med(ta)
            verdict = "B faster" if ratio * spread < 1 else "B SLOWER" if ratio > spread else "tie"
            say(f"{name:52s} {fmt(ta):>26s} {fmt(tb):>26s} {ratio:6.2f} {spread:9.3f} {verdict:>9s} {diff:9.2e} {mem_a:8.1f} {mem_b:8.1f} {tr:8.1f}")
            del ga, gb, gr, run_r, pool_k, pool_v, oa, ob
            torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"kvvarlen_layer_{sha}_summary.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written: {path}")


if __name__ == "__main__":
    main()
