"""Per-(batch, head) softmax_n without a GPU: the new C entry points (fasn_fwd_n, fasn_bwd_dn, fasn_bwd_dn_workspace_bytes) are exported and
refuse bad arguments with the documented FASN_E* codes before any launch; the front end's tensor-n normalisation; and the Hugging Face route of
a model with attention sinks (GPT-OSS: `s_aux`, causality from the module) with the kernel call replaced by a torch restatement."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEW = ("fasn_fwd_n", "fasn_bwd_dn_workspace_bytes", "fasn_bwd_dn")


def _buf(nbytes=1 << 16):
    buf = (ctypes.c_char * (nbytes + 16))()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _fwd_args(pkg, base, **over):
    a = pkg._lib.FwdArgs()
    for v in (a.q, a.k, a.v, a.o):
        v.ptr = base
        v.stride[0], v.stride[1], v.stride[2], v.stride[3] = 64 * 8, 64 * 8, 64, 1
    a.dtype, a.B, a.H, a.Sq, a.Sk, a.D, a.Dv = 1, 1, 1, 8, 8, 64, 64
    a.scale, a.softmax_n = 0.125, 1.0
    for k_, v_ in over.items():
        setattr(a, k_, v_)
    return a


def _bwd_args(pkg, base, **over):
    b = pkg._lib.BwdArgs()
    b.fwd = _fwd_args(pkg, base, **over)
    b.fwd.lse = base
    b.dout.ptr = base
    b.dout.stride[0], b.dout.stride[1], b.dout.stride[2], b.dout.stride[3] = 64 * 8, 64 * 8, 64, 1
    return b


def test_new_entry_points_are_exported_and_declared(pkg):
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fasn.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in pkg._lib.EXPORTS
        assert f"{name}(" in header
    assert pkg._lib.load().fasn_abi_version() == 6   # added entry points, no struct changed


def test_fwd_n_validation_codes(pkg):
    """fasn_fwd_n refuses before any launch: NULL args, a misaligned n, negative strides or strides that leave 32-bit offsets; a NULL n is
    fasn_fwd_ws (its codes); the ignored scalar softmax_n is not checked when n is given."""
    lib = pkg._lib.load()
    buf, base = _buf()
    n = base + 4096
    assert lib.fasn_fwd_n(None, n, 0, 1, None, 0, None) == -1
    assert lib.fasn_fwd_n(_fwd_args(pkg, base), n + 2, 0, 1, None, 0, None) == -4
    assert lib.fasn_fwd_n(_fwd_args(pkg, base), n, -1, 1, None, 0, None) == -1
    assert lib.fasn_fwd_n(_fwd_args(pkg, base, B=2, H=2), n, 1 << 31, 1, None, 0, None) == -1
    assert lib.fasn_fwd_n(_fwd_args(pkg, base, B=0), n, 0, 1, None, 0, None) == -1
    assert lib.fasn_fwd_n(_fwd_args(pkg, base, dtype=3), n, 0, 1, None, 0, None) == -2
    assert lib.fasn_fwd_n(_fwd_args(pkg, base, D=96, Dv=96), n, 0, 1, None, 0, None) == -3
    a = _fwd_args(pkg, base, softmax_n=-1.0)
    a.q.ptr = base + 2
    assert lib.fasn_fwd_n(a, n, 0, 1, None, 0, None) == -4          # the negative scalar is ignored, the bad view is not
    assert lib.fasn_fwd_n(_fwd_args(pkg, base, softmax_n=-1.0), None, 0, 1, None, 0, None) == -1   # n NULL: fasn_fwd_ws checks the scalar
    a = _fwd_args(pkg, base)
    a.v.stride[3] = 2
    assert lib.fasn_fwd_n(a, n, 0, 1, None, 0, None) == -5
    del buf


def test_bwd_dn_validation_codes_and_workspace(pkg):
    lib = pkg._lib.load()
    buf, base = _buf()
    dn, ws = base + 8192, base + 16384
    assert lib.fasn_bwd_dn(None, dn, 0, 1, ws, 1 << 12, None) == -1
    assert lib.fasn_bwd_dn_workspace_bytes(None) == 0
    b = _bwd_args(pkg, base)
    b.fwd.lse = None
    assert lib.fasn_bwd_dn(b, dn, 0, 1, ws, 1 << 12, None) == -1                 # lse missing
    assert lib.fasn_bwd_dn_workspace_bytes(b) == 0
    assert lib.fasn_bwd_dn(_bwd_args(pkg, base), None, 0, 1, ws, 1 << 12, None) == -1   # dn missing
    assert lib.fasn_bwd_dn(_bwd_args(pkg, base), dn + 2, 0, 1, ws, 1 << 12, None) == -4
    assert lib.fasn_bwd_dn(_bwd_args(pkg, base), dn, -1, 1, ws, 1 << 12, None) == -1
    assert lib.fasn_bwd_dn(_bwd_args(pkg, base), dn, 0, 1, None, 0, None) == -8     # workspace missing
    need = lib.fasn_bwd_dn_workspace_bytes(_bwd_args(pkg, base))
    assert need > 0 and need % 4 == 0
    assert lib.fasn_bwd_dn(_bwd_args(pkg, base), dn, 0, 1, ws, need - 4, None) == -8   # too small
    assert lib.fasn_bwd_dn(_bwd_args(pkg, base), dn, 0, 1, ws + 4, need, None) == -4   # misaligned
    b = _bwd_args(pkg, base)
    b.dout.ptr = base + 2
    assert lib.fasn_bwd_dn(b, dn, 0, 1, ws, need, None) == -4
    b = _bwd_args(pkg, base)
    b.dout.stride[3] = 2
    assert lib.fasn_bwd_dn(b, dn, 0, 1, ws, need, None) == -5
    assert lib.fasn_bwd_dn(_bwd_args(pkg, base, dtype=3), dn, 0, 1, ws, need, None) == -2
    # one fp32 partial sum per (b, h, chunk of rows): grows with B * H and with Sq
    big = lib.fasn_bwd_dn_workspace_bytes(_bwd_args(pkg, base, B=4, H=8, Sq=4096))
    assert big >= 4 * 8 * 4 and big % (4 * 8 * 4) == 0 and big > need
    del buf


def test_tensor_n_normalisation(pkg):
    """[H], [1, H], [B, 1], [B, H] and 0-d become the fp32 [1 or B, 1 or H] view the kernels read; anything else is refused; gradients reach
    the caller's tensor in its own shape and dtype."""
    from flash_attention_softmax_n_amd.flash_attn import _n_strides, _n_tensor
    q = torch.zeros(3, 4, 5, 64)
    for shape, want in (((4,), (1, 4)), ((1, 4), (1, 4)), ((3, 1), (3, 1)), ((3, 4), (3, 4)), ((), (1, 1))):
        nt = _n_tensor(torch.ones(shape), q)
        assert nt.shape == want and nt.dtype == torch.float32
    assert _n_strides(_n_tensor(torch.ones(4), q)) == (0, 1)
    assert _n_strides(_n_tensor(torch.ones(3, 4), q)) == (4, 1)
    assert _n_strides(_n_tensor(torch.ones(3, 1), q)) == (1, 0)
    assert _n_strides(_n_tensor(torch.ones(()), q)) == (0, 0)
    for bad in (torch.ones(5), torch.ones(2, 4), torch.ones(3, 4, 1), torch.ones(4, dtype=torch.int32)):
        with pytest.raises((ValueError, TypeError)):
            _n_tensor(bad, q)
    s = torch.zeros(4, dtype=torch.bfloat16, requires_grad=True)
    _n_tensor(torch.exp(s.float()), q).sum().backward()
    assert s.grad.dtype == torch.bfloat16 and s.grad.shape == (4,)


def _torch_attention(query, key, value, softmax_n_param=None, scale=None, dropout_p=0.0, attn_mask=None, attn_bias=None, is_causal=False):
    """flash_attention_n restated in fp32 torch (float or [H] / [B, H] tensor n, grouped K/V, bool mask, additive bias, bottom-right causal)"""
    B, H, L, E = query.shape
    S = key.shape[2]
    G = H // key.shape[1]
    k, v = key.repeat_interleave(G, 1), value.repeat_interleave(G, 1)
    s = query @ k.transpose(-1, -2) * (E ** -0.5 if scale is None else scale)
    if attn_bias is not None:
        s = s + attn_bias
    if is_causal:
        i, j = torch.arange(L).view(L, 1), torch.arange(S).view(1, S)
        s = s.masked_fill(j > i + S - L, float("-inf"))
    if attn_mask is not None:
        s = s.masked_fill(~attn_mask, float("-inf"))
    n = 0.0 if softmax_n_param is None else softmax_n_param
    if torch.is_tensor(n):
        n = n.reshape((1,) * (2 - n.dim()) + tuple(n.shape)).expand(B, H)[..., None, None]
    m = s.amax(-1, keepdim=True).clamp_min(0.0).detach()
    e = torch.exp(s - m)
    return (e / (n * torch.exp(-m) + e.sum(-1, keepdim=True))) @ v


def _tiny_gpt_oss():
    from transformers import GptOssConfig, GptOssForCausalLM
    cfg = GptOssConfig(vocab_size=128, hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                       head_dim=64, num_local_experts=2, num_experts_per_tok=1, layer_types=["sliding_attention", "full_attention"],
                       sliding_window=8, max_position_embeddings=256, attention_dropout=0.0)
    torch.manual_seed(0)
    model = GptOssForCausalLM(cfg).eval()
    with torch.no_grad():
        for layer in model.model.layers:
            layer.self_attn.sinks.copy_(torch.randn(cfg.num_attention_heads))
    return cfg, model


def test_gpt_oss_sinks_and_causality_reach_the_attention_function(monkeypatch):
    """GPT-OSS hands its sink logits as `s_aux` and, in a full-attention layer of an unpadded batch, no mask and no `is_causal`: the attention
    function must pass n_h = softmax_n_param + exp(s_h) per head and take the causality from the module. Logits and the sink gradients then
    equal eager's, with and without a padded row (the kernel call replaced by a torch restatement)."""
    pytest.importorskip("transformers")
    from flash_attention_softmax_n_amd import surgery
    if not surgery.register_hf_attention():
        pytest.skip("transformers without AttentionInterface")
    pytest.importorskip("transformers.models.gpt_oss")
    import flash_attention_softmax_n_amd.flash_attn as fa
    seen = []

    def recording(query, key, value, **kw):
        seen.append((torch.is_tensor(kw.get("softmax_n_param")), kw.get("is_causal"), kw.get("attn_mask") is not None))
        return _torch_attention(query, key, value, **kw)

    monkeypatch.setattr(fa, "flash_attention_n", recording)
    cfg, model = _tiny_gpt_oss()
    ids = torch.randint(0, cfg.vocab_size, (2, 24))
    att = torch.ones(2, 24, dtype=torch.long)
    att[1, :5] = 0

    def run(impl, mask):
        model.config._attn_implementation = impl
        model.zero_grad()
        out = model(input_ids=ids, attention_mask=mask).logits
        valid = torch.ones_like(out[..., :1]) if mask is None else mask[..., None].float()
        (out * valid).square().sum().backward()
        return out.detach() * valid, [l.self_attn.sinks.grad.clone() for l in model.model.layers]

    for mask in (None, att):
        want, gwant = run("eager", mask)
        seen.clear()
        got, ggot = run(surgery.HF_ATTENTION_NAME, mask)
        assert len(seen) == cfg.num_hidden_layers and all(t for t, _, _ in seen)   # the sinks arrive as a tensor n
        if mask is None:   # the full-attention layer: no mask, causal from the module
            assert (False, True) in [(m, c) for _, c, m in seen]
        assert (got - want).abs().max().item() <= 1e-4 * want.abs().max().item()
        for a, b in zip(ggot, gwant):
            assert (a - b).abs().max().item() <= 1e-4 * max(b.abs().max().item(), 1e-6)


def test_hf_attention_causality_rule():
    """transformers' SDPA rule: the `is_causal` kwarg, else the module's attribute; never with one query row or a mask."""
    import flash_attention_softmax_n_amd.flash_attn as fa
    from flash_attention_softmax_n_amd import surgery
    got = []

    def recording(query, key, value, **kw):
        got.append(kw["is_causal"])
        return torch.zeros_like(query)

    mp = pytest.MonkeyPatch()
    mp.setattr(fa, "flash_attention_n", recording)
    try:
        q = torch.zeros(1, 2, 4, 64)
        q1 = torch.zeros(1, 2, 1, 64)
        mask = torch.ones(1, 1, 4, 4, dtype=torch.bool)
        dec, enc, bare = torch.nn.Module(), torch.nn.Module(), torch.nn.Module()
        dec.is_causal, enc.is_causal = True, False
        for module, query, m, kw, want in ((dec, q, None, {}, True), (enc, q, None, {}, False), (bare, q, None, {}, False),
                                           (dec, q1, None, {}, False), (dec, q, mask, {}, False), (enc, q, None, {"is_causal": True}, True),
                                           (dec, q, None, {"is_causal": False}, False)):
            got.clear()
            surgery._hf_attention(module, query, q, q, m, **kw)
            assert got == [want], (module.__dict__.get("is_causal"), query.shape, m is not None, kw)
    finally:
        mp.undo()
