"""What the tests of the packed route of surgery._hf_attention share (tests/test_hfpacked_cpu.py, tests/test_gpu_hfpacked.py).
A plain module: no tests, importable without a GPU.

  LENS / flat_batch   the documents (40, 1, 23, 64) as the flattened [1, T] batch DataCollatorWithFlattening(return_flash_attn_kwargs=True)
                      produces: input_ids, restarting position_ids, int32 cu_seq_lens_q / _k and the Python-int max_length_q / _k
  tiny_gpt_oss        the config of tests/test_gpu_sinks.py (sliding_window = 16, layers sliding + full, 4 / 2 heads, head dim 64, sinks)
  tiny_llama          LlamaConfig with 4 query / 2 K/V heads and 2 layers at a given head dim; use_cache=False, the training setup in which
                      transformers' mask builders look for restarting position_ids (they do not next to a K/V cache)
  varlen_restated / dense_restated   flash_attention_n_varlen and flash_attention_n in fp32 torch, in the manner of tests/test_sinks_cpu.py
  Recorder            replaces (or spies on) the two functions in flash_attn and keeps every call's arguments
  per_doc             logits, sink gradients and embedding gradient of one document under the loss of tests/test_gpu_sinks.py
  gate                max |B - ref| <= 2 max |A - ref|, the figures printed before the assertion"""
import copy

import torch

LENS = (40, 1, 23, 64)


def flat_batch(vocab, dev="cpu", lens=LENS, seed=0):
    """(model inputs, packed keywords, per-document input_ids) - the keywords exactly as the collator builds them"""
    g = torch.Generator().manual_seed(seed)
    docs = [torch.randint(0, vocab, (n,), generator=g) for n in lens]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    inputs = dict(input_ids=torch.cat(docs).view(1, -1).to(dev), position_ids=torch.cat([torch.arange(n) for n in lens]).view(1, -1).to(dev))
    kw = dict(cu_seq_lens_q=torch.tensor(cu, dtype=torch.int32, device=dev), cu_seq_lens_k=torch.tensor(cu, dtype=torch.int32, device=dev),
              max_length_q=max(lens), max_length_k=max(lens))
    return inputs, kw, [d.view(1, -1).to(dev) for d in docs]


def rows(lens=LENS):
    out, at = [], 0
    for n in lens:
        out.append(slice(at, at + n))
        at += n
    return out


def tiny_gpt_oss(dtype, dev="cpu", sliding_window=16):
    from transformers import GptOssConfig, GptOssForCausalLM
    cfg = GptOssConfig(vocab_size=128, hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                       head_dim=64, num_local_experts=2, num_experts_per_tok=1, layer_types=["sliding_attention", "full_attention"],
                       sliding_window=sliding_window, max_position_embeddings=256, attention_dropout=0.0)
    torch.manual_seed(0)
    model = GptOssForCausalLM(cfg).eval()
    with torch.no_grad():
        for layer in model.model.layers:
            layer.self_attn.sinks.copy_(torch.randn(cfg.num_attention_heads))
    return cfg, model.to(dtype).to(dev)


def tiny_llama(dtype, dev="cpu", head_dim=64):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      head_dim=head_dim, max_position_embeddings=256, attention_dropout=0.0, use_cache=False)
    torch.manual_seed(0)
    return cfg, LlamaForCausalLM(cfg).eval().to(dtype).to(dev)


def fp32_copy(model):
    return copy.deepcopy(model).float()


# ---------------------------------------------------------------- the two calls in fp32 torch
def _softmax_n(s, n):
    """rows of s [H, L, S] with the sink n ([H, 1, 1] or a float): exp(s) / (n + sum exp(s))"""
    m = s.amax(-1, keepdim=True).clamp_min(0.0).detach()
    e = torch.exp(s - m)
    return e / (n * torch.exp(-m) + e.sum(-1, keepdim=True))


def varlen_restated(query, key, value, cu_seqlens_q, max_seqlen_q, cu_seqlens_k=None, max_seqlen_k=None, softmax_n_param=1, scale=None,
                    is_causal=False, return_lse=False, window=None):
    """flash_attention_n_varlen sequence by sequence in fp32 (self-attention packs whose every row sees a key): [T, H, E] in query's dtype,
    rows behind cu[B] 0"""
    assert not return_lse
    T, H, E = query.shape
    G = H // key.shape[1]
    cu_q = cu_seqlens_q.tolist()
    cu_k = cu_q if cu_seqlens_k is None else cu_seqlens_k.tolist()
    assert max(b - a for a, b in zip(cu_q, cu_q[1:])) <= max_seqlen_q and (max_seqlen_k is None or max(b - a for a, b in zip(cu_k, cu_k[1:])) <= max_seqlen_k)
    n = softmax_n_param
    if torch.is_tensor(n):
        n = n.float().reshape(-1).expand(H).view(H, 1, 1)
    scale = E ** -0.5 if scale is None else scale
    pieces = []
    for b in range(len(cu_q) - 1):
        q = query[cu_q[b]:cu_q[b + 1]].float().transpose(0, 1)
        k = key[cu_k[b]:cu_k[b + 1]].float().transpose(0, 1).repeat_interleave(G, 0)
        v = value[cu_k[b]:cu_k[b + 1]].float().transpose(0, 1).repeat_interleave(G, 0)
        sq, sk = q.shape[1], k.shape[1]
        s = q @ k.transpose(-1, -2) * scale
        if is_causal:
            p = torch.arange(sq).view(sq, 1) + (sk - sq)
            j = torch.arange(sk).view(1, sk)
            hide = j > p
            if window is not None:
                hide = hide | (j <= p - window)
            s = s.masked_fill(hide, float("-inf"))
        pieces.append((_softmax_n(s, n) @ v).transpose(0, 1))
    pieces.append(torch.zeros(T - cu_q[-1], H, E))
    return torch.cat(pieces).to(query.dtype)


def dense_restated(query, key, value, softmax_n_param=None, scale=None, dropout_p=0.0, attn_mask=None, attn_bias=None, is_causal=False):
    """flash_attention_n in fp32 torch: [B, H, L, Ev] in query's dtype"""
    B, H, L, E = query.shape
    S = key.shape[2]
    G = H // key.shape[1]
    k, v = key.float().repeat_interleave(G, 1), value.float().repeat_interleave(G, 1)
    s = query.float() @ k.transpose(-1, -2) * (E ** -0.5 if scale is None else scale)
    if attn_bias is not None:
        s = s + attn_bias.float()
    if is_causal:
        i, j = torch.arange(L).view(L, 1), torch.arange(S).view(1, S)
        s = s.masked_fill(j > i + S - L, float("-inf"))
    if attn_mask is not None:
        s = s.masked_fill(~attn_mask, float("-inf"))
    n = 0.0 if softmax_n_param is None else softmax_n_param
    if torch.is_tensor(n):
        n = n.float().reshape((1,) * (2 - n.dim()) + tuple(n.shape)).expand(B, H)[..., None, None]
    return (_softmax_n(s, n) @ v).to(query.dtype)


class Recorder:
    """flash_attn.flash_attention_n_varlen and flash_attn.flash_attention_n replaced for the test's duration: by the restatements above
    (`stub=True`, the CPU suite) or by spies around the real functions. Every call is kept as (positional arguments, keywords)."""

    def __init__(self, monkeypatch, stub):
        import flash_attention_softmax_n_amd.flash_attn as fa
        self.varlen, self.dense = [], []
        real_v, real_d = (varlen_restated, dense_restated) if stub else (fa.flash_attention_n_varlen, fa.flash_attention_n)

        def varlen(*a, **kw):
            self.varlen.append((a, kw))
            return real_v(*a, **kw)

        def dense(*a, **kw):
            self.dense.append((a, kw))
            return real_d(*a, **kw)

        monkeypatch.setattr(fa, "flash_attention_n_varlen", varlen)
        monkeypatch.setattr(fa, "flash_attention_n", dense)

    def clear(self):
        self.varlen.clear()
        self.dense.clear()


class Counter:
    """counts the calls of surgery._offsets_from_position_ids"""

    def __init__(self, monkeypatch, surgery):
        self.calls = 0
        real = surgery._offsets_from_position_ids

        def counted(position_ids):
            self.calls += 1
            return real(position_ids)

        monkeypatch.setattr(surgery, "_offsets_from_position_ids", counted)


# ---------------------------------------------------------------- model-level quantities and the gate
def sinks_of(model):
    return [layer.self_attn.sinks for layer in model.model.layers if hasattr(layer.self_attn, "sinks")]


def per_doc(model, impl, batches, doc_rows=None):
    """Per document d: (logits [n_d, V], [sink gradient per layer], embedding gradient), fp32 on the CPU, under the loss of
    tests/test_gpu_sinks.py restricted to the document: sum of its squared logits. `batches`: a list of (model inputs, keywords) - one
    entry per document (doc_rows None), or one packed entry whose documents are the slices doc_rows."""
    model.config._attn_implementation = impl
    params = sinks_of(model) + [model.get_input_embeddings().weight]
    out = []
    for inputs, kw in batches:
        logits = model(**inputs, **kw).logits
        for r in ([slice(0, logits.shape[1])] if doc_rows is None else doc_rows):
            mine = logits[0, r]
            grads = torch.autograd.grad(mine.float().square().sum(), params, retain_graph=True)
            grads = [g.detach().float().cpu() for g in grads]
            out.append((mine.detach().float().cpu(), grads[:-1], grads[-1]))
    return out


def errors(got, ref):
    """max |got - ref| over the documents for (logits, sink gradients, embedding gradient); the per-document figures are printed"""
    worst = [0.0, 0.0, 0.0]
    for d, ((lg, sg, eg), (lr, sr, er)) in enumerate(zip(got, ref)):
        e = [(lg - lr).abs().max().item(), max([(a - b).abs().max().item() for a, b in zip(sg, sr)], default=0.0), (eg - er).abs().max().item()]
        print(f"  document {d}: max-abs error logits {e[0]:.3e}  sink gradients {e[1]:.3e}  embedding gradient {e[2]:.3e}")
        worst = [max(a, b) for a, b in zip(worst, e)]
    return worst


def gate(err_b, err_a, what, names=("logits", "sink gradients", "embedding gradient")):
    """max |B - ref| <= 2 max |A - ref| for every quantity: B's attention differs from A's only in which instantiation of the same kernel
    text runs and in the order of its sums, the rest of the model is per-token math - a factor of 2 covers the reordering, whereas a leak
    across documents moves the logits by their own size"""
    for nm, b, a in zip(names, err_b, err_a):
        print(f"{what} {nm}: max|B - ref| {b:.3e}  max|A - ref| {a:.3e}  ratio {b / a if a else float('inf'):.3f}")
    for nm, b, a in zip(names, err_b, err_a):
        assert b <= 2.0 * a, f"{what} {nm}: max|B - ref| {b:.3e} > 2 x max|A - ref| {a:.3e}"
