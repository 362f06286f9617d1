"""Per-(batch, head) softmax_n as a tensor with a gradient (learned attention sinks, n_h = exp(s_h)) on the GPU: forward and dq / dk / dv / dn
against an fp32 torch restatement with one n per head (the explicit sink column), bit-identity with the scalar-n launches where n is constant,
launches big enough for head groups, paired causal blocks, the folded causal kernel and the dynamic deal across XCDs, determinism and shapes of
dn, HIP-graph replay with n changed in place, and GPT-OSS through transformers."""
import pytest
import torch

import flash_attention_softmax_n_amd.synth as synth

pytestmark = pytest.mark.gpu

# the gates of tests/test_gpu_parity.py::_check: the reference's own atol (O(1) tensors, scaled for larger ones) and a relative gate
REF_ATOL = {torch.float16: 1e-2, torch.bfloat16: 5e-2, torch.float32: 1e-3}
REL_TRUE = {torch.float16: 2.0 ** -9, torch.bfloat16: 2.0 ** -6, torch.float32: 2e-5}


def _check(got, want, dtype, what):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - want).abs().max().item()
    atol = REF_ATOL[dtype] * max(1.0, want.abs().max().item())
    assert err <= atol, f"{what}: max-abs {err:.3e} > reference atol {atol:.3e}"
    lim = REL_TRUE[dtype] * max(want.abs().max().item(), 1e-2)
    assert err <= lim, f"{what}: max-abs {err:.3e} > {lim:.3e} (relative gate)"


def _rand(shape, dtype, dev, seed, std=0.5):
    return synth.counter_normal(shape, seed, std=std, dtype=dtype, device=dev)


def _n_values(shape, dev, seed, zeros=True):
    """n in [0.2, 3] with exact zeros next to positive entries"""
    g = torch.Generator().manual_seed(seed)
    n = 0.2 + 2.8 * torch.rand(shape, generator=g)
    if zeros and n.numel() > 1:
        n.view(-1)[::3] = 0.0
    return n.to(dev)


def _reference(q, k, v, do, n, causal=False, mask=None, bias=None, keep=None, p_eff=0.0, scale=None):
    """fp32 torch on the device, one n per (batch, head): Z_i = n + sum_j exp(x_ij) (the sink column: logit 0, weight n, value 0).
    Returns (o, dq, dk, dv, dn in n's shape, dbias in bias's shape or None)."""
    B, H, L, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    qf, kf, vf = (t.detach().float().requires_grad_() for t in (q, k, v))
    nf = n.detach().float().clone().requires_grad_()
    bf = None if bias is None else bias.detach().float().requires_grad_()
    kx, vx = (t.repeat_interleave(H // Hkv, dim=1) for t in (kf, vf))
    s = (qf @ kx.transpose(-1, -2)) * (D ** -0.5 if scale is None else scale)
    if bf is not None:
        s = s + bf
    hide = torch.zeros(1, 1, L, S, dtype=torch.bool, device=q.device)
    if causal:
        i = torch.arange(L, device=q.device).view(L, 1)
        j = torch.arange(S, device=q.device).view(1, S)
        hide = hide | (j > i + S - L)
    if mask is not None:
        hide = hide | ~mask
    s = s.masked_fill(hide, float("-inf"))
    nb = nf.reshape((1,) * (2 - nf.dim()) + tuple(nf.shape)).expand(B, H)[..., None, None]
    with torch.no_grad():
        m = s.amax(-1, keepdim=True)
        m = torch.where(nb > 0, m.clamp_min(0.0), m)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    z = nb * torch.exp(-m) + e.sum(-1, keepdim=True)
    p = e / torch.where(z > 0, z, torch.ones_like(z))   # no visible key and n = 0: the row is 0 (and adds nothing to dn)
    if keep is not None:
        p = p * keep / (1.0 - p_eff)
    o = p @ vx
    o.backward(do.float())
    return o, qf.grad, kf.grad, vf.grad, nf.grad, (None if bf is None else bf.grad)


def _run(pkg, q, k, v, do, n, **kw):
    """the library: out, dq, dk, dv, dn (n is a leaf tensor that requires grad)"""
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    n = n.detach().clone().requires_grad_()
    out = pkg.flash_attention_n(q, k, v, softmax_n_param=n, **kw)
    out.backward(do)
    return out, q.grad, k.grad, v.grad, n.grad


def _compare(got, want, dtype, what):
    for g, w, nm in zip(got, want, ("out", "dq", "dk", "dv", "dn")):
        _check(g, w, dtype, f"{what} {nm}")


# ---------------------------------------------------------------- every head dim and dtype
@pytest.mark.parametrize("dtype,D", [(dt, d) for dt in (torch.float16, torch.bfloat16, torch.float32) for d in (32, 64, 128, 256)
                                     if not (dt == torch.float32 and d == 256)])
def test_tensor_n_matches_the_per_head_reference(pkg, dev, dtype, D):
    """n of shape [B, H] with exact zeros next to positive entries: forward and dq / dk / dv / dn of every head against the per-head fp32
    reference (the kernels before this change read one n per launch)."""
    B, H, L, S = 2, 6, 150, 230
    q = _rand((B, H, L, D), dtype, dev, 1)
    k, v = (_rand((B, H, S, D), dtype, dev, s) for s in (2, 3))
    do = _rand((B, H, L, D), dtype, dev, 4, std=1.0)
    n = _n_values((B, H), dev, 5)
    got = _run(pkg, q, k, v, do, n)
    want = _reference(q, k, v, do, n)[:5]
    _compare(got, want, dtype, f"D={D} {dtype}")


# ---------------------------------------------------------------- the modes
@pytest.mark.parametrize("kind", ["causal", "causal_fp16", "keypad", "mask", "bias", "dropout", "gqa", "decode_splitk"])
def test_tensor_n_in_every_mode(pkg, dev, kind):
    """causal with L > S (rows without a visible key, some with n = 0: lse = -inf, dn finite) and L < S, key padding, a dense mask, a
    batch-broadcast bias with its reduced gradient, dropout against the explicit keep mask, grouped K/V with n of shape [H], and a decode shape
    that splits its keys over workgroups (split 0 carries the sink, the combine kernel merges it)."""
    from flash_attention_softmax_n_amd import dropout as dmod, flash_attn
    dtype = torch.float16 if kind == "causal_fp16" else torch.bfloat16
    B, H, Hkv, L, S, D = 2, 4, 4, 200, 160, 64
    kw, ref = {}, {}
    nshape = (B, H)
    if kind == "causal_fp16":
        L, S = 160, 300
    if kind.startswith("causal"):
        kw["is_causal"] = ref["causal"] = True
    if kind == "gqa":
        H, Hkv, nshape = 8, 2, (8,)
    if kind == "decode_splitk":
        L, S, nshape = 2, 8192, (B, 1)
    q = _rand((B, H, L, D), dtype, dev, 11)
    k, v = (_rand((B, Hkv, S, D), dtype, dev, s) for s in (12, 13))
    do = _rand((B, H, L, D), dtype, dev, 14, std=1.0)
    n = _n_values(nshape, dev, 15)
    if kind == "keypad":
        mask = torch.ones(B, 1, 1, S, dtype=torch.bool, device=dev)
        mask[1, ..., 100:] = False
        kw["attn_mask"] = ref["mask"] = mask
    if kind == "mask":
        g = torch.Generator().manual_seed(16)
        mask = (torch.rand(B, H, L, S, generator=g) < 0.7).to(dev)
        mask[0, 0, 3] = False   # a fully hidden row with n = 0 (n[0, 0] is one of the zeros)
        kw["attn_mask"] = ref["mask"] = mask
    if kind == "bias":
        bias = _rand((1, H, L, S), dtype, dev, 17, std=1.0).requires_grad_()
        kw["attn_bias"] = bias
        ref["bias"] = bias
    if kind == "decode_splitk":
        pl = flash_attn._plan_for(q, k, v, None, None, n, D ** -0.5, False, 0.0)
        assert pl.fwd_ws > 64, "the decode shape must take the split-K plan"
    if kind == "dropout":
        kw["dropout_p"] = 0.2
    got = list(_run(pkg, q, k, v, do, n, **kw))
    if kind == "dropout":
        seed, off = flash_attn.last_dropout_state()
        keep = torch.from_numpy(dmod.keep_mask(seed, off, B, H, L, S, 0.2)).to(dev)
        ref["keep"], ref["p_eff"] = keep, dmod.effective_p(0.2)
    want = _reference(q, k, v, do, n, **ref)
    _compare(got, want[:5], dtype, kind)
    if kind == "bias":   # the reduced (batch-broadcast) bias gradient next to a tensor n
        bias.grad = None
        out = pkg.flash_attention_n(q, k, v, softmax_n_param=n, attn_bias=bias)
        out.backward(do)
        _check(bias.grad, want[5], dtype, "bias dbias")


# ---------------------------------------------------------------- big launches: bit for bit the scalar launches of each head's n
def _n_grouped(B, H, Hkv, vals, dev):
    """n[b, h] = vals[(b Hkv + h // G) % len(vals)]: constant within a K/V group, different between neighbouring items"""
    G = H // Hkv
    idx = (torch.arange(B).view(B, 1) * Hkv + torch.arange(H).view(1, H) // G) % len(vals)
    return torch.tensor(vals, dtype=torch.float32)[idx].to(dev)


@pytest.mark.parametrize("case", ["groups_d128", "groups_d256", "paired_causal", "fold_dynamic_deal", "plain_dynamic_deal", "bias_keypad_pairs"])
def test_big_launches_equal_the_scalar_launch_of_each_items_n(pkg, dev, case):
    """Launch shapes of the head-group hand-out (two-wave kernels, D = 128 / 256, grouped K/V), the paired causal blocks, the folded causal
    kernel with the dynamic deal across XCDs, the plain dynamic deal, and length-paired batches under a batch-broadcast bias (two (b, h) per
    workgroup): with n varying from item to item, every head's O, lse and dq / dk / dv must equal BIT FOR BIT those of the scalar launch with
    that head's n (the same kernels; only where n is read differs) - a kernel reading n once per launch, or per workgroup instead of per item,
    fails. dn against -sum_i delta_i exp(-lse_i) from the kernel's own O and lse."""
    from flash_attention_softmax_n_amd import flash_attn
    causal, mask, bias = True, None, None
    dtype = torch.bfloat16
    if case == "groups_d128":
        B, H, Hkv, L, S, D = 2, 32, 8, 512, 512, 128
    elif case == "groups_d256":
        B, H, Hkv, L, S, D = 2, 16, 16, 384, 640, 256
    elif case == "paired_causal":
        B, H, Hkv, L, S, D = 13, 32, 32, 1152, 1408, 64
        dtype = torch.float16
    elif case == "fold_dynamic_deal":
        B, H, Hkv, L, S, D = 32, 32, 32, 2000, 2024, 64
    elif case == "plain_dynamic_deal":
        B, H, Hkv, L, S, D = 32, 32, 32, 1000, 1000, 64
        causal = False
    else:
        B, H, Hkv, L, S, D = 8, 16, 16, 512, 512, 64
        causal = False
        lens = [512, 64, 448, 96, 384, 128, 320, 160]
        mask = torch.zeros(B, 1, 1, S, dtype=torch.bool, device=dev)
        for b_, l_ in enumerate(lens):
            mask[b_, ..., :l_] = True
        bias = _rand((1, H, L, S), dtype, dev, 47, std=1.0)
    q = _rand((B, H, L, D), dtype, dev, 41)
    k, v = (_rand((B, Hkv, S, D), dtype, dev, s) for s in (42, 43))
    do = _rand((B, H, L, D), dtype, dev, 44, std=1.0)
    vals = [0.0, 0.75, 2.5]
    nt = _n_grouped(B, H, Hkv, vals, dev)
    scale = D ** -0.5
    m_k = None if mask is None else mask.expand(B, H, L, S).view(torch.uint8)
    b_k = None if bias is None else bias.expand(B, H, L, S)

    def run(n):
        o, lse = flash_attn._launch_fwd(q, k, v, m_k, b_k, n, scale, causal, 0.0, None)
        qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
        nn = n.detach().clone().requires_grad_() if torch.is_tensor(n) else n
        out = pkg.flash_attention_n(qq, kk, vv, softmax_n_param=nn, is_causal=causal, attn_mask=mask, attn_bias=bias)
        out.backward(do)
        return o, lse, out.detach(), qq.grad, kk.grad, vv.grad, (nn.grad if torch.is_tensor(nn) else None)

    o_t, lse_t, out_t, dq_t, dk_t, dv_t, dn_t = run(nt)
    assert torch.equal(o_t, out_t)
    G = H // Hkv
    for c in vals:
        sel = nt == c                    # [B, H]
        selk = sel[:, ::G]               # [B, Hkv]: n is constant within a group
        o_c, lse_c, _, dq_c, dk_c, dv_c, _ = run(c)
        for got, want, s_, nm in ((o_t, o_c, sel, "out"), (lse_t, lse_c, sel, "lse"), (dq_t, dq_c, sel, "dq"), (dk_t, dk_c, selk, "dk"),
                                  (dv_t, dv_c, selk, "dv")):
            assert torch.equal(got[s_], want[s_]), f"{case}: {nm} of the heads with n = {c} differs from the scalar launch"
    # dn from the kernel's own O and lse (fp64 on the device)
    delta = (do.double() * o_t.double()).sum(-1)
    w = torch.where(torch.isfinite(lse_t), torch.exp(-lse_t.double()), torch.zeros_like(delta))
    dn_ref = -(delta * w).sum(-1)
    assert torch.isfinite(dn_t).all()
    err = (dn_t.double() - dn_ref).abs().max().item()
    assert err <= 1e-4 * max(dn_ref.abs().max().item(), 1e-3), f"{case}: dn off by {err:.3e}"


# ---------------------------------------------------------------- constant tensor == float
@pytest.mark.parametrize("dtype,D,causal,p", [(torch.bfloat16, 64, True, 0.0), (torch.float16, 128, False, 0.1), (torch.float32, 64, True, 0.0),
                                              (torch.bfloat16, 256, False, 0.0)])
def test_constant_tensor_n_is_the_float_bit_for_bit(pkg, dev, dtype, D, causal, p):
    """A tensor filled with c ([H], 0-d) gives O, lse (through the C ABI) and dq / dk / dv bit-identical to softmax_n_param = c."""
    from flash_attention_softmax_n_amd import flash_attn
    B, H, L, S = 2, 8, 300, 333
    q = _rand((B, H, L, D), dtype, dev, 51)
    k, v = (_rand((B, H, S, D), dtype, dev, s) for s in (52, 53))
    do = _rand((B, H, L, D), dtype, dev, 54, std=1.0)
    c = 1.75
    for n in (torch.full((H,), c, device=dev), torch.tensor(c, device=dev)):
        nt = flash_attn._n_tensor(n, q)
        rng = (1234, 8)
        o1, l1 = flash_attn._launch_fwd(q, k, v, None, None, c, D ** -0.5, causal, p, rng if p else None)
        o2, l2 = flash_attn._launch_fwd(q, k, v, None, None, nt, D ** -0.5, causal, p, rng if p else None)
        assert torch.equal(o1, o2) and torch.equal(l1, l2)
        grads = []
        for nn in (c, n):
            qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
            torch.manual_seed(7)
            out = pkg.flash_attention_n(qq, kk, vv, softmax_n_param=nn, is_causal=causal, dropout_p=p)
            out.backward(do)
            grads.append((out, qq.grad, kk.grad, vv.grad))
        for a, b_, nm in zip(grads[0], grads[1], ("out", "dq", "dk", "dv")):
            assert torch.equal(a, b_), f"{nm}: constant tensor n differs from the float"


# ---------------------------------------------------------------- dn: shapes, reductions, determinism
def test_dn_follows_the_shape_of_n_and_is_deterministic(pkg, dev):
    """dn comes back in n's shape ([H], [B, H], [B, 1], 0-d, a bf16 parameter through .float()); the zero-strided reductions equal the sums of
    the [B, H] result; two runs give the same bits."""
    dtype = torch.bfloat16
    B, H, L, S, D = 3, 8, 257, 300, 64
    q = _rand((B, H, L, D), dtype, dev, 61)
    k, v = (_rand((B, H, S, D), dtype, dev, s) for s in (62, 63))
    do = _rand((B, H, L, D), dtype, dev, 64, std=1.0)
    base = _n_values((B, H), dev, 65, zeros=False)
    full = _run(pkg, q, k, v, do, base)[4]
    again = _run(pkg, q, k, v, do, base)[4]
    assert full.shape == (B, H) and torch.equal(full, again)
    const = 1.25
    dn_bh = _run(pkg, q, k, v, do, torch.full((B, H), const, device=dev))[4]
    for shape, want in (((H,), dn_bh.sum(0)), ((B, 1), dn_bh.sum(1, keepdim=True)), ((1, H), dn_bh.sum(0, keepdim=True)), ((), dn_bh.sum())):
        dn = _run(pkg, q, k, v, do, torch.full(shape, const, device=dev))[4]
        assert dn.shape == torch.Size(shape)
        assert torch.allclose(dn, want, rtol=1e-4, atol=1e-5 * want.abs().max().item()), (shape, dn, want)
    s = torch.zeros(H, dtype=torch.bfloat16, device=dev, requires_grad=True)   # a bf16 sink logit: n = exp(s)
    out = pkg.flash_attention_n(q, k, v, softmax_n_param=torch.exp(s.float()))
    out.backward(do)
    assert s.grad is not None and s.grad.dtype == torch.bfloat16 and s.grad.shape == (H,)
    ref = _reference(q, k, v, do, torch.ones(H, device=dev))[4]   # dL/ds = dL/dn * exp(s) = dL/dn at s = 0
    _check(s.grad, ref, dtype, "bf16 sink logit gradient")


# ---------------------------------------------------------------- HIP graph
def test_graph_replay_follows_n_changed_in_place(pkg, dev):
    """Capture forward + backward with a tensor n, change n in place, replay: outputs and gradients are those of an eager run with the new
    values (the pointer is passed per call, never cached with the argument block)."""
    dtype = torch.bfloat16
    B, H, L, S, D = 2, 4, 256, 256, 64
    q, k, v = (_rand((B, H, L, D), dtype, dev, s).requires_grad_() for s in (71, 72, 73))
    do = _rand((B, H, L, D), dtype, dev, 74, std=1.0)
    n = _n_values((H,), dev, 75, zeros=False).requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            pkg.flash_attention_n(q, k, v, softmax_n_param=n, is_causal=True).backward(do)
            q.grad = k.grad = v.grad = n.grad = None
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        go = pkg.flash_attention_n(q, k, v, softmax_n_param=n, is_causal=True)
        go.backward(do)
    for vals in ([0.5, 1.0, 2.0, 4.0], [3.0, 0.0, 0.25, 1.5]):
        with torch.no_grad():
            n.copy_(torch.tensor(vals, device=dev))
        g.replay()
        torch.cuda.synchronize()
        got = (go.detach().clone(), q.grad.clone(), k.grad.clone(), v.grad.clone(), n.grad.clone())
        want = _run(pkg, q, k, v, do, torch.tensor(vals, device=dev), is_causal=True)
        for a, b_, nm in zip(got, want, ("out", "dq", "dk", "dv", "dn")):
            assert torch.equal(a, b_), f"graph replay with n = {vals}: {nm} differs from the eager run"


# ---------------------------------------------------------------- GPT-OSS
def test_gpt_oss_through_transformers_matches_eager(pkg, dev):
    """A tiny random GPT-OSS (sliding + full attention layers, head dim 64, 4 query / 2 K/V heads, attention sinks) loaded with the package's
    attention implementation: logits equal eager's (without and with a padded row) and so do the gradients of the sink logits."""
    pytest.importorskip("transformers")
    from flash_attention_softmax_n_amd import surgery
    if not surgery.register_hf_attention():
        pytest.skip("transformers without AttentionInterface")
    from transformers import GptOssConfig, GptOssForCausalLM
    cfg = GptOssConfig(vocab_size=128, hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                       head_dim=64, num_local_experts=2, num_experts_per_tok=1, layer_types=["sliding_attention", "full_attention"],
                       sliding_window=16, max_position_embeddings=256, attention_dropout=0.0)
    torch.manual_seed(0)
    model = GptOssForCausalLM(cfg).to(dev).float().eval()
    with torch.no_grad():
        for layer in model.model.layers:
            layer.self_attn.sinks.copy_(torch.randn(cfg.num_attention_heads))
    ids = torch.randint(0, cfg.vocab_size, (2, 40), device=dev)
    att = torch.ones(2, 40, dtype=torch.long, device=dev)
    att[1, :9] = 0   # a left-padded row

    def logits_and_sink_grads(impl, mask):
        model.config._attn_implementation = impl
        model.zero_grad()
        out = model(input_ids=ids, attention_mask=mask).logits
        valid = torch.ones_like(out[..., :1]) if mask is None else mask[..., None].float()
        (out * valid).square().sum().backward()
        return out.detach() * valid, [l.self_attn.sinks.grad.clone() for l in model.model.layers]

    for mask in (None, att):
        want, gwant = logits_and_sink_grads("eager", mask)
        got, ggot = logits_and_sink_grads(surgery.HF_ATTENTION_NAME, mask)
        what = "padded" if mask is not None else "unpadded"
        _check(got, want, torch.float32, f"GPT-OSS logits ({what})")
        for i, (a, b_) in enumerate(zip(ggot, gwant)):
            _check(a, b_, torch.float32, f"GPT-OSS layer {i} sink gradient ({what})")
