"""Padding-free batches through transformers: the packed route of surgery._hf_attention (B) against the only correct route the library
offered before it (A), same box, same process.

The model is a two-layer GPT-OSS-shaped GptOssForCausalLM - a sliding layer (window 128) and a full one, 64 query / 8 K/V heads, head dim
64, attention sinks, four small experts - in bf16 with attn_implementation = surgery.HF_ATTENTION_NAME, on a flattened [1, T] batch of
T = 16384 tokens with restarting position_ids, in two packs: 16 x 1024 and 8192 + 8 x 1024. Every token uses all four experts
(num_experts_per_tok = num_local_experts): with top-1 routing of random weights, one bf16 rounding of an attention output flips the
expert of about 1 token in 120 and moves that token's logits by their own size, so max |A - B| would measure the router's
discontinuity, not the routes; with all experts weighted the model is continuous and the figure is the routes' difference.

  B   the packed route: the keywords of DataCollatorWithFlattening(return_flash_attn_kwargs=True) (cu_seq_lens_q / _k, max_length_q / _k)
      reach flash_attention_n_varlen in every layer. transformers still builds its dense masks before the layers run; they are not read.
  B0  B with the mask construction switched off (attention_mask = {"full_attention": None, "sliding_attention": None}): B - B0 is the
      time, and the difference of the peaks the memory, of building masks that nobody reads.
  A   GPT-OSS's own masks carry no document boundaries, so the correct dense route is the caller's: block-diagonal causal and band boolean
      masks [1, 1, T, T], built OUTSIDE the timed region, passed as the {"full_attention", "sliding_attention"} mapping, keywords withheld;
      flash_attention_n runs under the dense mask.

The routes alternate (A, B, B0, A, B, B0, ...); each timing is `iters` eager model calls between two device events after a warm-up.
Reported per pack, for the model's forward and forward + backward: milliseconds of every alternation, B / A (ratio of medians, < 1 = B is
faster), A's own spread between its alternations (the margin B is judged against), the peak extra device memory of one call of each route
(torch's allocator statistics; A's prebuilt masks are reported apart), B - B0, and max |A - B| over the logits.
usage: python tools/bench_hf_packed.py [--rounds N] [--iters N] [--only SUBSTRING]"""
import argparse
import hashlib
import sys

import torch

sys.path.insert(0, ".")
import flash_attention_softmax_n_amd as fa   # noqa: E402
from flash_attention_softmax_n_amd import surgery   # noqa: E402

WINDOW = 128


def packs():
    return [("16 x 1024", [1024] * 16), ("8192 + 8 x 1024", [8192] + [1024] * 8)]


def timed(fn, iters):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters   # milliseconds per call


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


def build_model(dev, T):
    from transformers import GptOssConfig, GptOssForCausalLM
    cfg = GptOssConfig(vocab_size=1024, hidden_size=1024, intermediate_size=256, num_hidden_layers=2, num_attention_heads=64, num_key_value_heads=8,
                       head_dim=64, num_local_experts=4, num_experts_per_tok=4, layer_types=["sliding_attention", "full_attention"],
                       sliding_window=WINDOW, max_position_embeddings=T, attention_dropout=0.0, use_cache=False)
    torch.manual_seed(0)
    model = GptOssForCausalLM(cfg).eval()
    with torch.no_grad():
        for layer in model.model.layers:
            layer.self_attn.sinks.copy_(torch.randn(cfg.num_attention_heads))
    model = model.to(torch.bfloat16).to(dev)
    model.config._attn_implementation = surgery.HF_ATTENTION_NAME
    return cfg, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_hf_packed needs a GPU"
    assert surgery.register_hf_attention(), "bench_hf_packed needs transformers with AttentionInterface"
    import transformers
    dev = torch.device("cuda:0")
    sha = hashlib.sha256(open(fa._lib.LIB_PATH, "rb").read()).hexdigest()[:12]
    print(f"device: {torch.cuda.get_device_name(0)}; libfasn.so {sha}; transformers {transformers.__version__}; bf16 GPT-OSS-shaped model, 2 layers "
          f"(sliding {WINDOW} + full), 64 / 8 heads, head dim 64; {args.iters} calls per timing, {args.rounds} alternations A / B / B0")
    med = lambda ts: sorted(ts)[len(ts) // 2]   # noqa: E731
    fmt = lambda ts: "/".join(f"{t:.2f}" for t in ts)   # noqa: E731
    T = 16384
    cfg, model = build_model(dev, T)
    calls = {"varlen": 0, "dense": 0}
    real_v, real_d = fa.flash_attn.flash_attention_n_varlen, fa.flash_attn.flash_attention_n

    def spy_v(*a, **kw):
        calls["varlen"] += 1
        return real_v(*a, **kw)

    def spy_d(*a, **kw):
        calls["dense"] += 1
        return real_d(*a, **kw)

    fa.flash_attn.flash_attention_n_varlen, fa.flash_attn.flash_attention_n = spy_v, spy_d
    for name, lens in packs():
        if args.only not in name:
            continue
        assert sum(lens) == T
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(0, cfg.vocab_size, (1, T), generator=g).to(dev)
        pos = torch.cat([torch.arange(n) for n in lens]).view(1, T).to(dev)
        cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)
        kw = dict(cu_seq_lens_q=cu, cu_seq_lens_k=cu.clone(), max_length_q=max(lens), max_length_k=max(lens))
        dlogits = (torch.randn(1, T, cfg.vocab_size, generator=g) / T).to(torch.bfloat16).to(dev)
        # route A's masks, outside the timed region: same document, key not behind the row (and within the window)
        base = torch.cuda.memory_allocated()
        doc = torch.repeat_interleave(torch.arange(len(lens), device=dev), torch.tensor(lens, device=dev))
        at = torch.arange(T, device=dev)
        full = ((doc[:, None] == doc[None, :]) & (at[None, :] <= at[:, None])).view(1, 1, T, T)
        band = full & (at[None, :] > at[:, None] - WINDOW).view(1, 1, T, T)
        torch.cuda.synchronize()
        masks_mib = (torch.cuda.memory_allocated() - base) / 2 ** 20
        mapping = {"full_attention": full, "sliding_attention": band}
        none = {"full_attention": None, "sliding_attention": None}

        fwd = {"A": lambda: model(input_ids=ids, position_ids=pos, attention_mask=mapping).logits,
               "B": lambda: model(input_ids=ids, position_ids=pos, **kw).logits,
               "B0": lambda: model(input_ids=ids, position_ids=pos, attention_mask=none, **kw).logits}

        def train(f):
            def step():
                f().backward(dlogits)
                model.zero_grad(set_to_none=True)
            return step

        def infer(f):
            def step():
                with torch.no_grad():
                    return f()
            return step

        outs = {}
        for r, f in fwd.items():   # which function answers on which route, and the results
            calls["varlen"] = calls["dense"] = 0
            outs[r] = infer(f)().float()
            want = (0, cfg.num_hidden_layers) if r == "A" else (cfg.num_hidden_layers, 0)
            assert (calls["varlen"], calls["dense"]) == want, f"route {r}: {calls}"
        diff = (outs["A"] - outs["B"]).abs().max().item()
        top = outs["A"].abs().max().item()
        assert torch.equal(outs["B"], outs["B0"]), "the masks transformers builds must not change the packed route's result"
        del outs
        for what, wrap in (("forward", infer), ("forward + backward", train)):
            fns = {r: wrap(f) for r, f in fwd.items()}
            mem = {r: peak_extra(fn) for r, fn in fns.items()}
            ts = {r: [] for r in fns}
            for _ in range(args.rounds):
                for r, fn in fns.items():
                    ts[r].append(timed(fn, args.iters))
            ratio, spread = med(ts["B"]) / med(ts["A"]), max(ts["A"]) / min(ts["A"])
            print(f"{name:16s} {what:19s} A ms {fmt(ts['A'])}  B ms {fmt(ts['B'])}  B0 ms {fmt(ts['B0'])}  B/A {ratio:.3f}  A spread {spread:.3f}  "
                  f"B ahead of A by more than A's spread: {'yes' if ratio * spread < 1.0 else 'NO'}  "
                  f"extra MiB A {mem['A']:.0f} (+ {masks_mib:.0f} of prebuilt masks) B {mem['B']:.0f} B0 {mem['B0']:.0f}  "
                  f"unread masks: {med(ts['B']) - med(ts['B0']):.2f} ms, {mem['B'] - mem['B0']:.0f} MiB  max|A-B| {diff:.2e} (max |logit| {top:.2e})", flush=True)
        del full, band, mapping
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
