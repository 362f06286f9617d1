"""Rotary position embedding on the K/V-cache calls: the fused rotate-and-append against the route it replaces. Same box, same process,
three shapes, bf16: two decode steps on an 8192-key cache and a 2048-position chunk behind 6144 cached keys.

  A = what a caller did before, ALL of it captured: the positions from cache_seqlens with torch ops, the gathered cos / sin rows, the
      Hugging Face rotation (x * cos + rotate_half(x) * sin in fp32, rounded once) of q and k_new, then flash_attention_n_kvcache /
      flash_attention_n_kvcache_prefill with k_new / v_new.
  B = flash_attention_n_kvcache_rope: one rotate-and-append launch, then the same forward.
Both write the same rows of the same paged cache (page 256, shuffled block table, lengths in device memory) with the same bits, so the
results are compared with max |A - B|, which is 0.

Both go through their Python front ends, captured in a HIP graph of REPS calls so that host time is out of the picture; the graphs are
replayed alternating A / B and timed with device events. Reported: microseconds per call for every alternation, B/A (ratio of medians,
< 1 = B is faster) next to A's own spread between its alternations (the margin B is judged against). On the chunk shape the
rotate-and-append launch and the plain append launch are also timed alone (graphs of the C calls), with the bytes each moves per second:
the plain append reads and writes k_new and v_new; the rotary one also reads q, writes q_out and reads the table rows.
The table is printed and written to profiles/kvrope_<first 8 hex digits of libfasn.so's sha256>_summary.txt (--out PATH: elsewhere).
usage: python tools/bench_kvrope.py [--rounds N] [--iters N] [--only SUBSTRING] [--out PATH]"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402
from flash_attention_softmax_n_amd import _lib   # noqa: E402
from flash_attention_softmax_n_amd.flash_attn import _stream_ptr, _view4   # noqa: E402

PAGE = 256


# (name, B, H, Hkv, Sq, keys in the cache before the call, D, calls per graph); n is a tensor [H] everywhere
def shapes():
    return [
        ("decode (64,64/8,1,8192,64)", 64, 64, 8, 1, 8192 - 1, 64, 10),
        ("decode (64,16,1,8192,128)", 64, 16, 16, 1, 8192 - 1, 128, 10),
        ("chunk (4,64/8,2048,6144+2048,64)", 4, 64, 8, 2048, 6144, 64, 4),
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


def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    out_path = args.out or os.path.join("profiles", f"kvrope_{sha[:8]}_summary.txt")
    lines = [f"# Rotary rotate-and-append on the K/V-cache calls (flash_attention_n_kvcache_rope): library sha256 {sha[:8]}..., every line from one",
             "# run of tools/bench_kvrope.py on one MI355X; no clock or power setting was changed",
             "#",
             "# bf16, fp32 tables, rotary_dim = D, per-head n, paged cache (page 256, shuffled block table); A = positions from cache_seqlens, gathered",
             "# cos / sin, Hugging Face rotation of q and k_new in fp32 with torch ops, then the cache call with k_new - all captured; B = the new call;",
             "# 10 (decode) / 4 (chunk) calls per HIP graph; us per call of each alternation; B/A = ratio of medians, < 1 = B is faster; A spread = A's",
             "# max / min between its alternations"]

    def say(text):
        print(text, flush=True)
        lines.append(text)
    assert torch.cuda.is_available(), "bench_kvrope needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
    fmt = lambda ts: "/".join(f"{t:.1f}" for t in ts)   # noqa: E731
    say(f"device: {torch.cuda.get_device_name(0)}; {args.iters} replays per timing, {args.rounds} alternations A / B")
    say(f"{'shape (B,H[/Hkv],Sq,S,D)':36s} {'A us':>24s} {'B us':>24s} {'B/A':>6s} {'A spread':>8s} {'max|A-B|':>9s}")
    for name, B, H, Hkv, Sq, cached, D, reps in shapes():
        if args.only not in name:
            continue
        torch.manual_seed(0)
        S = cached + Sq
        max_pages = (S + PAGE - 1) // PAGE
        num_pages = B * max_pages
        q = torch.randn(B, H, Sq, D, device=dev, dtype=dtype) * 0.5
        kn = torch.randn(B, Hkv, Sq, D, device=dev, dtype=dtype) * 0.5
        vn = torch.randn(B, Hkv, Sq, D, device=dev, dtype=dtype) * 0.5
        pool_k = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        pool_v = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        table = torch.randperm(num_pages, device=dev).to(torch.int32).view(B, max_pages)
        sl = torch.full((B,), cached, dtype=torch.int32, device=dev)
        n = torch.rand(H, device=dev) + 0.5
        rows = max_pages * PAGE
        inv = 10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
        ang = torch.arange(rows, dtype=torch.float64)[:, None] * inv[None]
        cos, sin = ang.cos().float().to(dev), ang.sin().float().to(dev)           # [rows, D / 2]: what B reads
        cos_full, sin_full = torch.cat((cos, cos), -1), torch.cat((sin, sin), -1)   # [rows, D]: the Hugging Face form A gathers from
        steps = torch.arange(Sq, device=dev)
        call = fa.flash_attention_n_kvcache if Sq == 1 else fa.flash_attention_n_kvcache_prefill

        def run_a():
            pos = sl.long()[:, None] + steps                       # [B, Sq], from the lengths in device memory
            c, s = cos_full[pos][:, None], sin_full[pos][:, None]   # [B, 1, Sq, D]
            qf, kf = q.float(), kn.float()
            q_rot = (qf * c + rotate_half(qf) * s).to(dtype)
            k_rot = (kf * c + rotate_half(kf) * s).to(dtype)
            return call(q_rot, pool_k, pool_v, sl, block_table=table, k_new=k_rot, v_new=vn, softmax_n_param=n)

        def run_b():
            return fa.flash_attention_n_kvcache_rope(q, pool_k, pool_v, sl, cos, sin, block_table=table, k_new=kn, v_new=vn, softmax_n_param=n)

        with torch.no_grad():
            ga, oa = graph_of(run_a, reps)
            gb, ob = graph_of(run_b, reps)
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(time_graph(ga, args.iters, reps))
                tb.append(time_graph(gb, args.iters, reps))
            torch.cuda.synchronize()
            diff = (oa.float() - ob.float()).abs().max().item()
        say(f"{name:36s} {fmt(ta):>24s} {fmt(tb):>24s} {med(tb) / med(ta):6.3f} {max(ta) / min(ta):8.3f} {diff:9.2e}")

        if Sq > 1:   # the two append launches alone, through the C ABI
            lib = _lib.load()
            with torch.no_grad():
                _prep = fa.kvcache._prepare("bench_kvrope", "kvprefill", q, pool_k, pool_v, sl, table, kn, vn, n, None, True, False)
            pa = _prep.args
            q_out = torch.empty_like(q)
            rope = _lib.KvRope()
            rope.cos, rope.sin, rope.row_stride, rope.rows = cos.data_ptr(), sin.data_ptr(), cos.stride(0), rows
            rope.rotary_dim, rope.table_dtype, rope.interleaved = D, _lib.FASN_DTYPE_F32, 0

            def plain():
                _lib.check(lib.fasn_kvprefill_append(pa, _view4(kn), _view4(vn), _stream_ptr(dev)), "fasn_kvprefill_append")

            def rotary():
                _lib.check(lib.fasn_kvprefill_rope_append(pa, rope, _view4(q_out), _view4(kn), _view4(vn), _stream_ptr(dev)), "fasn_kvprefill_rope_append")

            with torch.no_grad():
                gp, _ = graph_of(plain, 10)
                gr, _ = graph_of(rotary, 10)
                tp, tr = [], []
                for _ in range(args.rounds):
                    tp.append(time_graph(gp, args.iters, 10))
                    tr.append(time_graph(gr, args.iters, 10))
            kv_bytes = 2 * 2 * B * Hkv * Sq * D * 2                      # k_new and v_new, read and written
            q_bytes = 2 * B * H * Sq * D * 2 + 2 * B * Sq * (D // 2) * 4   # q read, q_out written, the table rows of the call's positions once
            say(f"  append launches alone on this shape, us: plain {fmt(tp)} = {kv_bytes / med(tp) / 1e6:.2f} TB/s of {kv_bytes / 2 ** 20:.0f} MiB; "
                  f"rotate-and-append {fmt(tr)} = {(kv_bytes + q_bytes) / med(tr) / 1e6:.2f} TB/s of {(kv_bytes + q_bytes) / 2 ** 20:.0f} MiB")
            del gp, gr, _prep
        del ga, gb, pool_k, pool_v, oa, ob
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written: {out_path}")


if __name__ == "__main__":
    main()
