"""MLA decode over a compressed latent cache: flash_attention_n_mla (B) against the route it replaces (A), same box, same process.

  A = torch ops, fully captured: gather the pages through the block table, torch.matmul(q, rows^T) * scale, the length mask, the sink
      column written by hand, softmax, torch.matmul(p, rows[..., :512]). Sq = 1 shapes need no causal mask beyond the lengths; for Sq = 2
      the causal offset is part of the mask.
  B = flash_attention_n_mla on the same pool and table.

Both are captured in a HIP graph of REPS calls so that host time is out of the picture; the graphs are replayed alternating A / B / A / B
and timed with device events. Reported: microseconds per call for every alternation, A / B, A's own spread between its alternations (the
margin B is judged against), max |A - B| and B's TB/s of VISIBLE cache bytes (B * len * 1152: the cache is read once per 64 rows, so the
bytes moved are ceil(H * Sq / 64) times that).

--fp8: the FP8 latent cache against the 16-bit one, same shapes, lengths and alternation.
  A = flash_attention_n_mla on the pool of bf16 numbers that ARE the codes (pool8.to(bf16)),
  B = flash_attention_n_mla_fp8 on the codes with kv_scale = 1 - so max |A - B| must be 0 - and both columns of TB/s count their own
      visible cache bytes once (B * len * 1152 for A, B * len * 576 for B).

--sparse: flash_attention_n_mla_sparse (B) at topk = 2048 entries per position, sampled without replacement from a context of 32768 that
every position sees, same (B, H, Sq) and alternation A1 / B / A2:
  A1 = flash_attention_n_mla on a dense cache that holds exactly those 2048 rows per (batch element, position), len = topk: the same bytes,
       contiguous - the yardstick for "the gather costs nothing", judged within A1's own spread;
  A2 = the torch route, fully captured: index-gather of the rows through the table, two matmuls, the sink column by hand.

--sparse-fp8: flash_attention_n_mla_sparse_fp8 (B) over 656-byte FP8 rows, the lists and shapes of --sparse, alternation A / B / A2:
  A  = flash_attention_n_mla_sparse on the bf16 pool mla_fp8_rows_unpack gives: the same numbers (max |A - B| must be 0), the yardstick;
  A2 = the route B replaces, fully captured: torch gather of the 656-byte rows, mla_fp8_rows_unpack, flash_attention_n_mla on the compacted rows.
Then the calls with kv_new, A + fasn_mla_append and B + fasn_mla_sparse_fp8_append, and graphs that launch the two append entry points alone.

--index: flash_attention_n_mla_index (B), the indexer that builds such a list: Hi = 64, topk = 2048, context 32768, (B, Sq) = (64, 1), (1, 2), (8, 1).
  A = the torch route, fully captured: gather of the index-key pages through the table, einsum over the 64 heads, relu, the weighted head
      sum, the length and causal mask, torch.topk. Reported beside the times: the share of B's entries that A's list holds too (A's logits
      are sums of bf16 matmul outputs, so the lists differ near the cut) and B's TB/s of key bytes (B * Sq * len * 256: every position
      reads the keys once).
usage: python tools/bench_mla.py [--fp8 | --sparse | --sparse-fp8 | --index] [--rounds N] [--iters N] [--only I]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402

PAGE = 256
REPS = 5
E, EV = 576, 512
SCALE = (128 + 64) ** -0.5
SHAPES = [(64, 128, 1, 8192), (64, 16, 1, 8192), (1, 128, 2, 32768)]   # (B, H, Sq, len); the second is the TP-8 shard


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
    for _ in range(2):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (iters * REPS)   # microseconds per call


TOPK, CONTEXT = 2048, 32768


def sparse_main(args):
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    print(f"A1 = flash_attention_n_mla on the {TOPK} rows made contiguous, B = flash_attention_n_mla_sparse (topk {TOPK} of {CONTEXT}), A2 = torch gather + matmuls")
    print(f"{'shape (B,H,Sq)':16s} {'A1 us':>22s} {'B us':>22s} {'A2 us':>26s} {'A1/B':>6s} {'A2/B':>6s} {'A1 spread':>9s} {'max|A2-B|':>9s} {'max|A1-B|':>9s}")
    for idx, (B, H, Sq, _) in enumerate(SHAPES):
        if args.only is not None and idx != args.only:
            continue
        torch.manual_seed(0)
        max_pages = CONTEXT // PAGE
        q = torch.randn(B, H, Sq, E, device=dev, dtype=dtype) * 0.5
        pool = torch.randn(B * max_pages, PAGE, 1, E, device=dev, dtype=dtype) * 0.5
        table = torch.randperm(B * max_pages, device=dev).to(torch.int32).view(B, max_pages)
        sl = torch.full((B,), CONTEXT, dtype=torch.int32, device=dev)
        # without replacement, from the positions every query position sees (j <= len - Sq)
        ind = torch.stack([torch.randperm(CONTEXT - Sq + 1, device=dev)[:TOPK] for _ in range(B * Sq)]).view(B, Sq, TOPK).to(torch.int32)
        phys = (table.long().gather(1, (ind.long() // PAGE).view(B, -1)) * PAGE + (ind.long() % PAGE).view(B, -1)).view(B, Sq, TOPK)
        flat = pool.view(-1, E)
        compact = flat[phys.view(B * Sq, TOPK)].view(B * Sq, TOPK, 1, E).contiguous()    # A1's cache: the same rows, contiguous
        q1 = q.transpose(1, 2).reshape(B * Sq, H, 1, E)
        sl1 = torch.full((B * Sq,), TOPK, dtype=torch.int32, device=dev)

        def run_a1():
            return fa.flash_attention_n_mla(q1, compact, sl1, SCALE).view(B, Sq, H, EV).transpose(1, 2)

        def run_a2():
            rows = flat[phys]                                                             # [B, Sq, topk, 576]: the gather
            x = torch.matmul(q.transpose(1, 2), rows.transpose(2, 3)).float() * SCALE      # [B, Sq, H, topk]
            x = torch.cat([torch.zeros(B, Sq, H, 1, device=dev), x], -1)                   # the sink column: logit 0, weight n = 1
            p = torch.softmax(x, -1)[..., 1:].to(dtype)
            return torch.matmul(p, rows[..., :EV]).transpose(1, 2)

        def run_b():
            return fa.flash_attention_n_mla_sparse(q, pool, ind, sl, SCALE, block_table=table)

        with torch.no_grad():
            (g1, o1), (gb, ob), (g2, o2) = graph_of(run_a1), graph_of(run_b), graph_of(run_a2)
            t1, tb, t2 = [], [], []
            for _ in range(args.rounds):
                t1.append(time_graph(g1, args.iters))
                tb.append(time_graph(gb, args.iters))
                t2.append(time_graph(g2, args.iters))
            d2, d1 = (o2.float() - ob.float()).abs().max().item(), (o1.float() - ob.float()).abs().max().item()
        med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
        fmt = lambda ts: "/".join(f"{t:.1f}" for t in ts)   # noqa: E731
        print(f"{str((B, H, Sq)):16s} {fmt(t1):>22s} {fmt(tb):>22s} {fmt(t2):>26s} {med(t1) / med(tb):6.2f} {med(t2) / med(tb):6.2f} "
              f"{max(t1) / min(t1):9.3f} {d2:9.2e} {d1:9.2e}", flush=True)
        del g1, gb, g2, pool, compact
        torch.cuda.empty_cache()


INDEX_SHAPES = [(64, 1), (1, 2), (8, 1)]   # (B, Sq)
INDEX_HEADS, INDEX_D = 64, 128


def index_main(args):
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    print(f"A = torch gather + einsum + relu + weighted sum + mask + topk, B = flash_attention_n_mla_index (Hi {INDEX_HEADS}, topk {TOPK} of {CONTEXT})")
    print(f"{'shape (B,Sq)':14s} {'A us':>26s} {'B us':>26s} {'A/B':>6s} {'A spread':>9s} {'B entries in A list':>20s} {'B TB/s of key bytes':>20s}")
    for idx, (B, Sq) in enumerate(INDEX_SHAPES):
        if args.only is not None and idx != args.only:
            continue
        torch.manual_seed(0)
        max_pages = CONTEXT // PAGE
        q = torch.randn(B, INDEX_HEADS, Sq, INDEX_D, device=dev, dtype=dtype)
        w = (torch.randn(B, Sq, INDEX_HEADS, device=dev) * INDEX_HEADS ** -0.5).transpose(1, 2)   # the model's [B, Sq, Hi], transposed
        pool = torch.randn(B * max_pages, PAGE, 1, INDEX_D, device=dev, dtype=dtype)
        table = torch.randperm(B * max_pages, device=dev).to(torch.int32).view(B, max_pages)
        sl = torch.full((B,), CONTEXT, dtype=torch.int32, device=dev)
        pos = torch.arange(CONTEXT, device=dev).view(1, 1, -1)
        qi = torch.arange(Sq, device=dev).view(1, Sq, 1)

        def run_a():
            rows = pool[table.long()].view(B, CONTEXT, INDEX_D)                                        # gather the pages
            s = torch.relu(torch.einsum("bhqd,bsd->bhqs", q, rows).float())
            lg = (w[..., None] * s).sum(1).masked_fill(pos > qi + sl.view(B, 1, 1) - Sq, float("-inf"))
            return lg.topk(TOPK, -1).indices

        def run_b():
            return fa.flash_attention_n_mla_index(q, w, pool, sl, TOPK, block_table=table)

        with torch.no_grad():
            (ga, oa), (gb, ob) = graph_of(run_a), graph_of(run_b)
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(time_graph(ga, args.iters))
                tb.append(time_graph(gb, args.iters))
            same = sum(int(torch.isin(b, a).sum()) for a, b in zip(oa.view(-1, TOPK), ob.view(-1, TOPK))) / (B * Sq * TOPK)
        a_med, b_med = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
        fmt = lambda ts: "/".join(f"{t:.1f}" for t in ts)   # noqa: E731
        tbs = B * Sq * CONTEXT * INDEX_D * 2 / (b_med * 1e-6) / 1e12
        print(f"{str((B, Sq)):14s} {fmt(ta):>26s} {fmt(tb):>26s} {a_med / b_med:6.2f} {max(ta) / min(ta):9.3f} {same:20.4f} {tbs:20.2f}", flush=True)
        del ga, gb, pool
        torch.cuda.empty_cache()


def append_graph(name, q, pool, table, sl, kv_new):
    """a captured graph that launches nothing but the append entry point `name` on the call's block (pool: 16-bit or 656-byte rows)"""
    from flash_attention_softmax_n_amd import _lib
    from flash_attention_softmax_n_amd.flash_attn import _stream_ptr, _view4
    (B, H, Sq, _), lib = q.shape, _lib.load()
    out = torch.empty(B, H, Sq, EV, device=q.device, dtype=q.dtype)
    a = _lib.MlaArgs()
    a.q, a.o, a.kv_cache, a.seqlens = _view4(q), _view4(out), pool.data_ptr(), sl.data_ptr()
    a.kv_stride[0], a.kv_stride[1] = pool.stride(0), pool.stride(1)
    a.block_table, a.block_table_stride, a.max_pages, a.page_size = table.data_ptr(), table.stride(0), table.shape[1], PAGE
    a.B, a.H, a.Sq, a.D, a.Dv, a.dtype = B, H, Sq, E, EV, _lib.FASN_DTYPE_BF16
    a.scale, a.softmax_n, a.causal = SCALE, 1.0, 1
    view = _view4(kv_new)
    return graph_of(lambda: _lib.check(getattr(lib, name)(a, view, _stream_ptr(q.device)), name))[0], (a, out, view)


def sparse_fp8_main(args):
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    print(f"A = flash_attention_n_mla_sparse on the unpacked bf16 pool, B = flash_attention_n_mla_sparse_fp8 (topk {TOPK} of {CONTEXT}), "
          "A2 = torch gather + unpack + flash_attention_n_mla; +new: the same call with kv_new")
    print(f"{'shape (B,H,Sq)':16s} {'A us':>22s} {'B us':>22s} {'A2 us':>26s} {'B/A':>6s} {'B/A2':>6s} {'A spread':>9s} {'max|A-B|':>9s} {'max|A2-B|':>9s} "
          f"{'A+new us':>9s} {'B+new us':>9s} {'append16':>9s} {'append8':>9s}")
    for idx, (B, H, Sq, _) in enumerate(SHAPES):
        if args.only is not None and idx != args.only:
            continue
        torch.manual_seed(0)
        max_pages = CONTEXT // PAGE
        q = torch.randn(B, H, Sq, E, device=dev, dtype=dtype) * 0.5
        pool8 = torch.cat([fa.mla_fp8_rows_pack(torch.randn(max_pages, PAGE, 1, E, device=dev, dtype=dtype) * 0.5) for _ in range(B)])
        pool = torch.cat([fa.mla_fp8_rows_unpack(pool8[b * max_pages:(b + 1) * max_pages], dtype) for b in range(B)])
        table = torch.randperm(B * max_pages, device=dev).to(torch.int32).view(B, max_pages)
        sl = torch.full((B,), CONTEXT, dtype=torch.int32, device=dev)
        sl_new = sl - Sq   # with kv_new the same context, its last Sq rows rewritten every call
        kv_new = torch.randn(B, Sq, 1, E, device=dev, dtype=dtype) * 0.5
        ind = torch.stack([torch.randperm(CONTEXT - Sq + 1, device=dev)[:TOPK] for _ in range(B * Sq)]).view(B, Sq, TOPK).to(torch.int32)
        phys = (table.long().gather(1, (ind.long() // PAGE).view(B, -1)) * PAGE + (ind.long() % PAGE).view(B, -1)).view(B * Sq, TOPK)
        flat8 = pool8.view(-1, 656)
        q1 = q.transpose(1, 2).reshape(B * Sq, H, 1, E)
        sl1 = torch.full((B * Sq,), TOPK, dtype=torch.int32, device=dev)

        def run_a(**kw):
            return fa.flash_attention_n_mla_sparse(q, pool, ind, sl_new if kw else sl, SCALE, block_table=table, **kw)

        def run_b(**kw):
            return fa.flash_attention_n_mla_sparse_fp8(q, pool8, ind, sl_new if kw else sl, SCALE, block_table=table, **kw)

        def run_a2():
            rows = fa.mla_fp8_rows_unpack(flat8[phys], dtype).view(B * Sq, TOPK, 1, E)
            return fa.flash_attention_n_mla(q1, rows, sl1, SCALE).view(B, Sq, H, EV).transpose(1, 2)

        with torch.no_grad():
            (ga, oa), (gb, ob), (g2, o2) = graph_of(run_a), graph_of(run_b), graph_of(run_a2)
            ta, tb, t2 = [], [], []
            for _ in range(args.rounds):
                ta.append(time_graph(ga, args.iters))
                tb.append(time_graph(gb, args.iters))
                t2.append(time_graph(g2, args.iters))
            da, d2 = (oa.float() - ob.float()).abs().max().item(), (o2.float() - ob.float()).abs().max().item()
            del ga, gb, g2
            gan, gbn = graph_of(lambda: run_a(kv_new=kv_new))[0], graph_of(lambda: run_b(kv_new=kv_new))[0]
            (g16, keep16), (g8, keep8) = (append_graph("fasn_mla_append", q, pool, table, sl_new, kv_new),
                                          append_graph("fasn_mla_sparse_fp8_append", q, pool8, table, sl_new, kv_new))   # the appends alone
            tan, tbn, t16, t8 = [], [], [], []
            for _ in range(args.rounds):
                tan.append(time_graph(gan, args.iters))
                tbn.append(time_graph(gbn, args.iters))
                t16.append(time_graph(g16, args.iters))
                t8.append(time_graph(g8, args.iters))
        med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
        fmt = lambda ts: "/".join(f"{t:.1f}" for t in ts)   # noqa: E731
        print(f"{str((B, H, Sq)):16s} {fmt(ta):>22s} {fmt(tb):>22s} {fmt(t2):>26s} {med(tb) / med(ta):6.2f} {med(tb) / med(t2):6.2f} "
              f"{max(ta) / min(ta):9.3f} {da:9.2e} {d2:9.2e} {med(tan):9.1f} {med(tbn):9.1f} {med(t16):9.2f} {med(t8):9.2f}", flush=True)
        del gan, gbn, g16, g8, pool, pool8, flat8
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--fp8", action="store_true")
    ap.add_argument("--sparse", action="store_true")
    ap.add_argument("--sparse-fp8", action="store_true")
    ap.add_argument("--index", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mla needs a GPU"
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    print(f"device: {torch.cuda.get_device_name(0)}; {REPS} calls per graph, {args.iters} replays per timing, {args.rounds} alternations A/B; bf16, page {PAGE}, n = 1")
    if args.sparse:
        return sparse_main(args)
    if args.sparse_fp8:
        return sparse_fp8_main(args)
    if args.index:
        return index_main(args)
    if args.fp8:
        print("A = flash_attention_n_mla (bf16 cache), B = flash_attention_n_mla_fp8 (e4m3fn cache, kv_scale = 1)")
    print(f"{'shape (B,H,Sq,len)':24s} {'A us':>26s} {'B us':>26s} {'A/B':>6s} {'A spread':>9s} {'max|A-B|':>9s} "
          + (f"{'A TB/s visible':>15s} " if args.fp8 else "") + f"{'B TB/s visible':>15s}")
    for idx, (B, H, Sq, ln) in enumerate(SHAPES):
        if args.only is not None and idx != args.only:
            continue
        torch.manual_seed(0)
        max_pages = (ln + PAGE - 1) // PAGE
        q = torch.randn(B, H, Sq, E, device=dev, dtype=dtype) * 0.5
        pool = torch.randn(B * max_pages, PAGE, 1, E, device=dev, dtype=dtype) * 0.5
        if args.fp8:   # the codes nearest to the same values, and the 16-bit pool of exactly those numbers
            pool8 = pool.to(torch.float8_e4m3fn)
            pool = pool8.to(dtype)
        table = torch.randperm(B * max_pages, device=dev).to(torch.int32).view(B, max_pages)
        sl = torch.full((B,), ln, dtype=torch.int32, device=dev)
        pos = torch.arange(max_pages * PAGE, device=dev).view(1, 1, 1, -1)
        qi = torch.arange(Sq, device=dev).view(1, 1, Sq, 1)

        def run_a():
            rows = pool[table.long()].view(B, max_pages * PAGE, E)                       # gather the pages
            x = torch.matmul(q.view(B, H * Sq, E), rows.transpose(1, 2)).view(B, H, Sq, -1).float() * SCALE
            x = x.masked_fill(pos > qi + sl.view(B, 1, 1, 1) - Sq, float("-inf"))
            x = torch.cat([torch.zeros(B, H, Sq, 1, device=dev), x], -1)                  # the sink column: logit 0, weight n = 1
            p = torch.softmax(x, -1)[..., 1:].to(dtype)
            return torch.matmul(p.view(B, H * Sq, -1), rows[..., :EV]).view(B, H, Sq, EV)

        def run_b():
            return fa.flash_attention_n_mla(q, pool, sl, SCALE, block_table=table)

        def run_b8():
            return fa.flash_attention_n_mla_fp8(q, pool8, sl, SCALE, 1.0, block_table=table)

        with torch.no_grad():
            ga, oa = graph_of(run_b if args.fp8 else run_a)
            gb, ob = graph_of(run_b8 if args.fp8 else run_b)
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(time_graph(ga, args.iters))
                tb.append(time_graph(gb, args.iters))
            diff = (oa.float() - ob.float()).abs().max().item()
        a_med, b_med = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
        fmt = lambda ts: "/".join(f"{t:.1f}" for t in ts)   # noqa: E731
        tbs = B * ln * E * (1 if args.fp8 else 2) / (b_med * 1e-6) / 1e12
        tas = f"{B * ln * E * 2 / (a_med * 1e-6) / 1e12:15.2f} " if args.fp8 else ""
        print(f"{str((B, H, Sq, ln)):24s} {fmt(ta):>26s} {fmt(tb):>26s} {a_med / b_med:6.2f} {max(ta) / min(ta):9.3f} {diff:9.2e} {tas}{tbs:15.2f}", flush=True)
        del ga, gb, pool
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
