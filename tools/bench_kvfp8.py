"""FP8 K/V cache: flash_attention_n_kvcache_fp8 on a cache of e4m3fn codes (B) against the 16-bit call on a bf16 cache of the same logical
content (A), same box, same process.

  A = flash_attention_n_kvcache / _prefill on a paged bf16 cache (page 256, shuffled block table, lengths in device memory).
  B = flash_attention_n_kvcache_fp8 on the quantisation of that cache, one scale per (batch element, K/V head).

Both go through their Python front ends, captured in a HIP graph of REPS calls so that host time is out of the picture; the graphs are
replayed alternating A / B / A / B and timed with device events. Reported: microseconds per call for every alternation, the K+V bytes
actually visible per second (A: 2 bytes per element, B: 1), B's time over A's (the byte count puts the floor at 0.5), A's own spread between
its alternations (the margin B is judged against), the quantising append alone against the 16-bit append, and max |B - fp32 reference on the
dequantised cache| (on the first batch element). usage: python tools/bench_kvfp8.py [--rounds N] [--iters N]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256
REPS = 10
F8 = torch.float8_e4m3fn


# (name, B, H, Hkv, Sq, cached lengths, D, tensor n)
def shapes():
    ragged = [2048 + (b * (8192 - 2048)) // 31 for b in range(32)]
    return [("decode (64,16,1,8192,128)", 64, 16, 16, 1, [8192] * 64, 128, False),
            ("decode (64,64/8,1,8192,64)", 64, 64, 8, 1, [8192] * 64, 64, False),
            ("decode (32,64/8,1,2048..8192,64) n[H]", 32, 64, 8, 1, ragged, 64, True),
            ("chunk (4,64/8,2048 behind 6144,64)", 4, 64, 8, 2048, [8192] * 4, 64, False)]


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


def reference(q, kd, vd, ln, n, causal):
    """fp32 softmax_n attention of one batch element: q [H, Sq, D], kd / vd [Hkv, S, D] dequantised, the first ln keys"""
    H, Sq, D = q.shape
    G = H // kd.shape[0]
    s = torch.einsum("kgqd,ksd->kgqs", q.float().view(-1, G, Sq, D), kd[:, :ln]) * D ** -0.5
    if causal:
        i, j = torch.arange(Sq, device=q.device)[:, None], torch.arange(ln, device=q.device)[None]
        s = s.masked_fill(j > i + ln - Sq, float("-inf"))
    m = s.amax(-1, keepdim=True).clamp_min(0.0)
    e = torch.exp(s - m)
    z = n.view(-1, G, 1, 1) * torch.exp(-m) + e.sum(-1, keepdim=True)
    return torch.einsum("kgqs,ksd->kgqd", e / z, vd[:, :ln]).reshape(H, Sq, D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvfp8 needs a GPU"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    print(f"device: {torch.cuda.get_device_name(0)}; {REPS} calls per graph, {args.iters} replays per timing, {args.rounds} alternations A/B")
    print(f"{'shape (B,H[/Hkv],Sq,S,D)':40s} {'A us':>24s} {'B us':>24s} {'A TB/s':>7s} {'B TB/s':>7s} {'B/A':>6s} {'A spread':>9s} "
          f"{'append A/B us':>14s} {'max|B-ref|':>10s}")
    for name, B, H, Hkv, Sq, lens, D, tensor_n in shapes():
        torch.manual_seed(0)
        S = max(lens)
        max_pages = (S + PAGE - 1) // PAGE
        num_pages = B * max_pages
        q = torch.randn(B, H, Sq, D, device=dev, dtype=dtype) * 0.5
        pool_k = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        pool_v = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        table = torch.randperm(num_pages, device=dev).to(torch.int32).view(B, max_pages)
        sl = torch.tensor(lens, dtype=torch.int32, device=dev)
        n = (torch.rand(H, device=dev) + 0.5) if tensor_n else 1.0
        # one scale per (batch element, K/V head): absmax / 448 over the element's pages, as a serving stack would calibrate it
        owner = torch.empty(num_pages, dtype=torch.long, device=dev)
        owner[table.long().view(-1)] = torch.arange(B, device=dev).repeat_interleave(max_pages)
        k_scale = torch.zeros(B, Hkv, device=dev).index_reduce_(0, owner, pool_k.float().abs().amax((1, 3)), "amax") / 448.0
        v_scale = torch.zeros(B, Hkv, device=dev).index_reduce_(0, owner, pool_v.float().abs().amax((1, 3)), "amax") / 448.0
        k8, v8 = quantise(pool_k, k_scale[owner]), quantise(pool_v, v_scale[owner])
        causal = Sq > 1
        call16 = fa.flash_attention_n_kvcache_prefill if Sq > 1 else fa.flash_attention_n_kvcache

        def run_a():
            return call16(q, pool_k, pool_v, sl, block_table=table, softmax_n_param=n, is_causal=causal)

        def run_b():
            return fa.flash_attention_n_kvcache_fp8(q, k8, v8, sl, k_scale, v_scale, block_table=table, softmax_n_param=n, is_causal=causal)

        # the appends alone: Sq new rows per batch element behind lengths that leave room for them (the forward is not part of these graphs)
        lib = fa._lib.load()
        sl_app = (sl - Sq).clamp_min(0)
        kn = torch.randn(B, Hkv, Sq, D, device=dev, dtype=dtype) * 0.5
        c16 = fa.kvcache._prepare("bench", "kvprefill", q, pool_k, pool_v, sl_app, table, kn, kn, 1.0, None, causal, False, by_shape=True)
        c8 = fa.kvcache._prepare("bench", "kvprefill", q, k8, v8, sl_app, table, kn, kn, 1.0, None, causal, False, by_shape=True, fp8=True)
        op = fa._lib.KvFp8(k_scale=k_scale.data_ptr(), v_scale=v_scale.data_ptr(), k_sb=Hkv, k_sh=1, v_sb=Hkv, v_sh=1, reserved=0)

        def app_a():
            fa.kvcache._append(lib, c16, fa.kvcache._stream_ptr(dev))

        def app_b():
            fa.kvcache._append(lib, c8, fa.kvcache._stream_ptr(dev), fp8=op)

        with torch.no_grad():
            ga, oa = graph_of(run_a)
            gb, ob = graph_of(run_b)
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(time_graph(ga, args.iters))
                tb.append(time_graph(gb, args.iters))
            torch.cuda.synchronize()
            kd = (k8.view(torch.uint8)[table[0].long()].view(F8).float() * k_scale[0][None, None, :, None]).reshape(-1, Hkv, D).transpose(0, 1)
            vd = (v8.view(torch.uint8)[table[0].long()].view(F8).float() * v_scale[0][None, None, :, None]).reshape(-1, Hkv, D).transpose(0, 1)
            nb = n if tensor_n else torch.full((H,), 1.0, device=dev)
            err = (ob[0].float() - reference(q[0], kd, vd, lens[0], nb, causal)).abs().max().item()
            gaa, _ = graph_of(app_a)
            gab, _ = graph_of(app_b)
            taa, tab = time_graph(gaa, args.iters), time_graph(gab, args.iters)
        a_med, b_med = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
        vis_a = sum(lens) * Hkv * D * 2 * 2
        fmt = lambda ts: "/".join(f"{t:.1f}" for t in ts)   # noqa: E731
        print(f"{name:40s} {fmt(ta):>24s} {fmt(tb):>24s} {vis_a / a_med / 1e6:7.2f} {vis_a / 2 / b_med / 1e6:7.2f} {b_med / a_med:6.2f} "
              f"{max(ta) / min(ta):9.3f} {taa:6.1f}/{tab:6.1f} {err:10.2e}", flush=True)
        del ga, gb, gaa, gab, pool_k, pool_v, k8, v8
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
