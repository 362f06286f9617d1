"""One layer step over an FP8 K/V cache - rotate, quantise, append, attend, with or without a sliding window
(flash_attention_n_kvcache_fp8_rope) - against the same step on a bf16 cache and against the one route an FP8 cache had before, same box,
same process.

  B  = flash_attention_n_kvcache_fp8_rope(..., window=) with k_new / v_new on the quantisation of the cache, one scale per (batch element,
       K/V head).
  A  = flash_attention_n_kvcache_rope(..., window=) with k_new / v_new on a paged bf16 cache of the same content (page 256, shuffled block
       table, lengths in device memory).
  A2 = window=None only: the positions from cache_seqlens, the rotation of query and k_new with torch ops, then
       flash_attention_n_kvcache_fp8(k_new=...) - what a caller with an FP8 cache had to do; all of it captured.

All go through their Python front ends, captured in a HIP graph of REPS calls so that host time is out of the picture; the graphs are
replayed alternating A / B / A2 and timed with device events. Reported: microseconds per call for every alternation, B's median over A's
and over A2's, A's own spread between its alternations (the margin B is judged against), the append launches alone - the 16-bit
rotate-append, the rotate-quantise-append, the plain quantising append - whether B equals A2 bit for bit, and max |B - A| (the
quantisation of the cache). usage: python tools/bench_kvfp8_layer.py [--rounds N] [--iters N]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256
REPS = 10
F8 = torch.float8_e4m3fn


# (name, B, H, Hkv, Sq, lengths the forward sees (the Sq appended rows included), D, tensor n, window)
def shapes():
    ragged = [2048 + (b * (8192 - 2048)) // 31 for b in range(32)]
    return [("decode (64,16,1,8192,128)", 64, 16, 16, 1, [8192] * 64, 128, False, None),
            ("decode (64,64/8,1,8192,64)", 64, 64, 8, 1, [8192] * 64, 64, False, None),
            ("decode (32,64/8,1,2048..8192,64) n[H]", 32, 64, 8, 1, ragged, 64, True, None),
            ("chunk (4,64/8,2048 behind 6144,64)", 4, 64, 8, 2048, [8192] * 4, 64, False, None),
            ("decode (64,64/8,1,8192,64) W=128", 64, 64, 8, 1, [8192] * 64, 64, False, 128)]


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


def quantise(pool, scale_ph):
    """[pages, PAGE, Hkv, D] 16-bit -> codes, one scale per (page, K/V head): clamp before the cast (torch's cast does not saturate)"""
    return (pool.float() / scale_ph[:, None, :, None]).clamp(-448.0, 448.0).to(F8)


def tables(rows, rd, dev, base=10000.0):
    inv = base ** (-torch.arange(0, rd, 2, dtype=torch.float64) / rd)
    ang = torch.arange(rows, dtype=torch.float64)[:, None] * inv[None]
    return ang.cos().float().to(dev), ang.sin().float().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvfp8_layer needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    print(f"device: {torch.cuda.get_device_name(0)}; {REPS} calls per graph, {args.iters} replays per timing, {args.rounds} alternations A/B/A2")
    print(f"{'shape (B,H[/Hkv],Sq,S,D)':40s} {'A us':>24s} {'B us':>24s} {'A2 us':>24s} {'B/A':>6s} {'B/A2':>6s} {'A spread':>9s} "
          f"{'appends 16r/8r/8 us':>20s} {'B==A2':>6s} {'max|B-A|':>9s}")
    for name, B, H, Hkv, Sq, lens, D, tensor_n, window in shapes():
        torch.manual_seed(0)
        S = max(lens)
        max_pages = (S + PAGE - 1) // PAGE
        num_pages = B * max_pages
        half = D // 2
        q = torch.randn(B, H, Sq, D, device=dev, dtype=dtype) * 0.5
        kn = torch.randn(B, Hkv, Sq, D, device=dev, dtype=dtype) * 0.5
        vn = torch.randn(B, Hkv, Sq, D, device=dev, dtype=dtype) * 0.5
        pool_k = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        pool_v = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        table = torch.randperm(num_pages, device=dev).to(torch.int32).view(B, max_pages)
        sl = torch.tensor(lens, dtype=torch.int32, device=dev) - Sq   # the cache before the step: the forward sees `lens`
        n = (torch.rand(H, device=dev) + 0.5) if tensor_n else 1.0
        cos, sin = tables(max_pages * PAGE, D, dev)
        owner = torch.empty(num_pages, dtype=torch.long, device=dev)
        owner[table.long().view(-1)] = torch.arange(B, device=dev).repeat_interleave(max_pages)
        k_scale = torch.zeros(B, Hkv, device=dev).index_reduce_(0, owner, pool_k.float().abs().amax((1, 3)), "amax") / 448.0
        v_scale = torch.zeros(B, Hkv, device=dev).index_reduce_(0, owner, pool_v.float().abs().amax((1, 3)), "amax") / 448.0
        k8, v8 = quantise(pool_k, k_scale[owner]), quantise(pool_v, v_scale[owner])
        steps = torch.arange(Sq, device=dev)

        def run_a():
            return fa.flash_attention_n_kvcache_rope(q, pool_k, pool_v, sl, cos, sin, block_table=table, k_new=kn, v_new=vn, softmax_n_param=n,
                                                     window=window)

        def run_b():
            return fa.flash_attention_n_kvcache_fp8_rope(q, k8, v8, sl, k_scale, v_scale, cos, sin, block_table=table, k_new=kn, v_new=vn,
                                                         softmax_n_param=n, window=window)

        def rotate(x, c, s):
            x1, x2 = x[..., :half].float(), x[..., half:].float()
            return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(dtype)

        def run_a2():
            pos = sl.long()[:, None] + steps[None]            # [B, Sq], from the lengths in device memory
            c, s = cos[pos][:, None], sin[pos][:, None]       # [B, 1, Sq, D / 2]
            return fa.flash_attention_n_kvcache_fp8(rotate(q, c, s), k8, v8, sl, k_scale, v_scale, block_table=table, k_new=rotate(kn, c, s), v_new=vn,
                                                    softmax_n_param=n)

        # the append launches alone (the forward is not part of these graphs)
        lib = fa._lib.load()
        kc = fa.kvcache
        rope = kc._rope_operand(cos, sin, False, q)
        c16 = kc._prepare("bench", "kvprefill", q, pool_k, pool_v, sl, table, kn, vn, 1.0, None, True, False, by_shape=True)
        c8r = kc._prepare("bench", "kvprefill", q, k8, v8, sl, table, kn, vn, 1.0, None, True, False, by_shape=True, fp8=True)
        c8 = kc._prepare("bench", "kvprefill", q, k8, v8, sl, table, kn, vn, 1.0, None, True, False, by_shape=True, fp8=True)
        op = fa._lib.KvFp8(k_scale=k_scale.data_ptr(), v_scale=v_scale.data_ptr(), k_sb=Hkv, k_sh=1, v_sb=Hkv, v_sh=1, reserved=0)
        qr16, qr8 = torch.empty_like(q), torch.empty_like(q)

        def app_16r():
            kc._append(lib, c16, kc._stream_ptr(dev), rope, qr16)

        def app_8r():
            kc._append(lib, c8r, kc._stream_ptr(dev), rope, qr8, fp8=op)

        def app_8():
            kc._append(lib, c8, kc._stream_ptr(dev), fp8=op)

        with torch.no_grad():
            ga, oa = graph_of(run_a)
            gb, ob = graph_of(run_b)
            ga2, oa2 = graph_of(run_a2) if window is None else (None, None)
            ta, tb, ta2 = [], [], []
            for _ in range(args.rounds):
                ta.append(time_graph(ga, args.iters))
                tb.append(time_graph(gb, args.iters))
                if ga2 is not None:
                    ta2.append(time_graph(ga2, args.iters))
            torch.cuda.synchronize()
            same = "-" if oa2 is None else ("yes" if torch.equal(ob.view(torch.int16), oa2.view(torch.int16)) else "NO")
            err = (ob.float() - oa.float()).abs().max().item()
            apps = [time_graph(graph_of(f)[0], args.iters) for f in (app_16r, app_8r, app_8)]
        med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
        fmt = lambda ts: "/".join(f"{t:.1f}" for t in ts) if ts else "-"   # noqa: E731
        ba2 = f"{med(tb) / med(ta2):6.2f}" if ta2 else "     -"
        print(f"{name:40s} {fmt(ta):>24s} {fmt(tb):>24s} {fmt(ta2):>24s} {med(tb) / med(ta):6.2f} {ba2} {max(ta) / min(ta):9.3f} "
              f"{apps[0]:6.1f}/{apps[1]:6.1f}/{apps[2]:6.1f} {same:>6s} {err:9.2e}", flush=True)
        del ga, gb, ga2, pool_k, pool_v, k8, v8
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
