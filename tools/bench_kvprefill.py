"""K/V-cache prefill: flash_attention_n_kvcache_prefill on a paged cache (B) against the routes the package offered before it, same box,
same process.

  A   = flash_attention_n(is_causal=True) on dense K/V [B, Hkv, S, D] of the same content (ragged batch: with the [B, 1, Sq, S] visibility
        mask instead, the only way one call serves prompts of different lengths). With a prefix the dense K/V hold prefix + prompt.
  A+g = A plus the pages -> dense gather a paged caller needs first (index through the block table, permute, copy): today's route.
  B   = flash_attention_n_kvcache_prefill on the paged cache (page 256, shuffled block table, lengths in device memory), prompt K/V
        already in the cache (the append is a copy both routes need).

All go through their Python front ends, captured in a HIP graph of REPS calls so that host time is out of the picture; the graphs are
replayed alternating A / A+g / B and timed with device events. Reported: microseconds per call for every alternation, B/A and B/(A+g)
(ratios of medians, < 1 = B is faster), A's own spread between its alternations (the margin B is judged against) and max |A - B|.
usage: python tools/bench_kvprefill.py [--rounds N] [--iters N] [--only SUBSTRING]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256
REPS = 4


# (name, B, H, Hkv, Sq, prefix, D, dtype, tensor n, prompt lengths or None)
def shapes():
    ragged = [256 + (b * (4096 - 256)) // 31 for b in range(32)]
    return [
        ("(8,16/16,4096,0,64) fp16", 8, 16, 16, 4096, 0, 64, torch.float16, False, None),
        ("(4,64/8,2048,0,64) bf16 n[H]", 4, 64, 8, 2048, 0, 64, torch.bfloat16, True, None),
        ("(4,64/8,2048,6144,64) bf16 n[H]", 4, 64, 8, 2048, 6144, 64, torch.bfloat16, True, None),
        ("(4,32/32,2048,6144,128) bf16", 4, 32, 32, 2048, 6144, 128, torch.bfloat16, False, None),
        ("ragged 32 x 256..4096, 64/8, 64 bf16", 32, 64, 8, 4096, 0, 64, torch.bfloat16, True, ragged),
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvprefill needs a GPU"
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; {REPS} calls per graph, {args.iters} replays per timing, {args.rounds} alternations A / A+g / B")
    print(f"{'shape (B,H/Hkv,Sq,prefix,D)':38s} {'A us':>26s} {'A+g us':>26s} {'B us':>26s} {'B/A':>6s} {'B/(A+g)':>8s} {'A spread':>9s} {'max|A-B|':>9s}")
    for name, B, H, Hkv, Sq, prefix, D, dtype, tensor_n, qlens in shapes():
        if args.only not in name:
            continue
        torch.manual_seed(0)
        S = prefix + Sq
        max_pages = (S + PAGE - 1) // PAGE
        num_pages = B * max_pages
        q = torch.randn(B, H, Sq, D, device=dev, dtype=dtype) * 0.5
        pool_k = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        pool_v = torch.randn(num_pages, PAGE, Hkv, D, device=dev, dtype=dtype) * 0.5
        table = torch.randperm(num_pages, device=dev).to(torch.int32).view(B, max_pages)
        tl = table.long()
        n = (torch.rand(H, device=dev) + 0.5) if tensor_n else 1.0
        if qlens is None:
            ql, sl, mask = None, torch.full((B,), S, dtype=torch.int32, device=dev), None
        else:   # prompts of different lengths padded to Sq, no prefix: len_b = qlen_b
            ql = torch.tensor(qlens, dtype=torch.int32, device=dev)
            sl = ql.clone()
            i = torch.arange(Sq, device=dev).view(1, 1, Sq, 1)
            j = torch.arange(S, device=dev).view(1, 1, 1, S)
            mask = (i < ql.view(B, 1, 1, 1)) & (j <= i)

        def gather():
            kd = pool_k[tl].reshape(B, max_pages * PAGE, Hkv, D)[:, :S].permute(0, 2, 1, 3).contiguous()
            vd = pool_v[tl].reshape(B, max_pages * PAGE, Hkv, D)[:, :S].permute(0, 2, 1, 3).contiguous()
            return kd, vd

        kd, vd = gather()

        def attn_a(kd_, vd_):
            if mask is not None:
                return fa.flash_attention_n(q, kd_, vd_, softmax_n_param=n, attn_mask=mask)
            return fa.flash_attention_n(q, kd_, vd_, softmax_n_param=n, is_causal=True)   # bottom-right aligned: the prompt behind its prefix

        def run_a():
            return attn_a(kd, vd)

        def run_ag():
            return attn_a(*gather())

        def run_b():
            return fa.flash_attention_n_kvcache_prefill(q, pool_k, pool_v, sl, block_table=table, query_seqlens=ql, softmax_n_param=n, is_causal=True)

        with torch.no_grad():
            ga, oa = graph_of(run_a)
            gg, og = graph_of(run_ag)
            gb, ob = graph_of(run_b)
            ta, tg, tb = [], [], []
            for _ in range(args.rounds):
                ta.append(time_graph(ga, args.iters))
                tg.append(time_graph(gg, args.iters))
                tb.append(time_graph(gb, args.iters))
            torch.cuda.synchronize()
            real = torch.ones(B, 1, Sq, 1, dtype=torch.bool, device=dev) if ql is None else (torch.arange(Sq, device=dev).view(1, 1, Sq, 1) < ql.view(B, 1, 1, 1))
            diff = ((oa.float() - ob.float()) * real).abs().max().item()
        med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
        fmt = lambda ts: "/".join(f"{t:.0f}" for t in ts)   # noqa: E731
        print(f"{name:38s} {fmt(ta):>26s} {fmt(tg):>26s} {fmt(tb):>26s} {med(tb) / med(ta):6.2f} {med(tb) / med(tg):8.2f} "
              f"{max(ta) / min(ta):9.3f} {diff:9.2e}", flush=True)
        del ga, gg, gb, kd, vd, pool_k, pool_v, oa, og, ob
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
