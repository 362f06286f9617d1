"""The packed route of surgery._hf_attention without a GPU: flash_attn.flash_attention_n_varlen and flash_attn.flash_attention_n
are replaced by recording fp32 torch restatements (tests/hf_packed.py). The routing table - which function answers and with which
arguments, for every condition of the route -, the opt-in switch with its one-entry cache, and a tiny GPT-OSS on a flattened batch."""
import logging
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hf_packed as hp   # noqa: E402

H, HKV, E = 4, 2, 64
T = sum(hp.LENS)


@pytest.fixture
def surgery(pkg, monkeypatch):
    from flash_attention_softmax_n_amd import surgery as s
    monkeypatch.setattr(s, "_PACKED_WARNED", set(), raising=False)
    monkeypatch.setattr(s, "_POSITION_IDS_CACHE", None, raising=False)
    monkeypatch.setattr(s, "HF_PACKED_FROM_POSITION_IDS", False, raising=False)
    return s


@pytest.fixture
def rec(pkg, monkeypatch):
    return hp.Recorder(monkeypatch, stub=True)


def _module(causal=True, n=None, training=True):
    m = torch.nn.Module()
    m.is_causal = causal
    if n is not None:
        m.softmax_n_param = n
    return m.train(training)


def _qkv(dtype=torch.bfloat16, batch=1, e=E, ev=E, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda heads, d: (0.5 * torch.randn(batch, heads, T, d, generator=g)).to(dtype)   # noqa: E731
    return mk(H, e), mk(HKV, e), mk(HKV, ev)


def _keywords():
    return hp.flat_batch(128)[1]


def _same(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    return a == b and type(a) is type(b)


# ---------------------------------------------------------------- the routing table: what is routed, and how
def test_collator_keywords_are_what_flat_batch_builds():
    transformers = pytest.importorskip("transformers")
    inputs, kw, docs = hp.flat_batch(128)
    got = transformers.DataCollatorWithFlattening(return_flash_attn_kwargs=True, return_tensors="pt")([{"input_ids": d[0].tolist()} for d in docs])
    assert torch.equal(got["input_ids"], inputs["input_ids"]) and torch.equal(got["position_ids"], inputs["position_ids"])
    for name in ("cu_seq_lens_q", "cu_seq_lens_k"):
        assert got[name].dtype == torch.int32 and torch.equal(got[name], kw[name])
    assert got["max_length_q"] == kw["max_length_q"] == 64 and type(got["max_length_q"]) is int and got["max_length_k"] == 64


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_packed_keywords_reach_the_packed_call(surgery, rec, dtype):
    """int32 offsets as the same objects, Python-int bounds as they are, the [T, H, E] views of the operands without a copy, scale, the
    window, causality from the module, n = softmax_n_param + exp(s_aux) with the gradient reaching s_aux, and the [1, T, H, E] result"""
    q, k, v = _qkv(dtype)
    kw = _keywords()
    s_aux = torch.linspace(-1.0, 1.0, H).to(dtype).requires_grad_()
    out, weights = surgery._hf_attention(_module(n=0.5), q, k, v, torch.ones(1, 1, T, T, dtype=torch.bool), scaling=0.2, dropout=0.0,
                                         s_aux=s_aux, sliding_window=16, position_ids=torch.zeros(1, T, dtype=torch.long), **kw)
    assert weights is None and not rec.dense and len(rec.varlen) == 1
    a, c = rec.varlen[0]
    assert a[3] is kw["cu_seq_lens_q"] and a[5] is kw["cu_seq_lens_k"] and a[4] == 64 and type(a[4]) is int and a[6] == 64 and type(a[6]) is int
    for got, src, heads in zip(a[:3], (q, k, v), (H, HKV, HKV)):
        assert got.data_ptr() == src.data_ptr() and got.shape == (T, heads, E) and got.stride() == (E, T * E, 1)
    assert c["scale"] == 0.2 and c["window"] == 16 and type(c["window"]) is int and c["is_causal"] is True
    assert torch.equal(c["softmax_n_param"], torch.exp(s_aux.float()) + 0.5) and c["softmax_n_param"].shape == (H,)
    assert out.shape == (1, T, H, E) and out.dtype == dtype
    assert torch.equal(out[0], hp.varlen_restated(*a, **c))
    out.float().sum().backward()
    assert s_aux.grad is not None and s_aux.grad.abs().max() > 0


def test_offset_and_bound_forms_are_converted(surgery, rec):
    """int64 offsets become int32, 0-d tensor bounds Python ints, a missing cu_seq_lens_k / max_length_k the query side's; without s_aux
    n is the module's float; the `is_causal` keyword wins over the module; eval() switches dropout off"""
    q, k, v = _qkv()
    kw = _keywords()
    cu64 = kw["cu_seq_lens_q"].long()
    surgery._hf_attention(_module(causal=False, n=1.5, training=False), q, k, v, None, dropout=0.1, cu_seq_lens_q=cu64, cu_seq_lens_k=None,
                          max_length_q=torch.tensor(64), is_causal=True)
    assert not rec.dense and len(rec.varlen) == 1
    a, c = rec.varlen[0]
    assert a[3].dtype == torch.int32 and torch.equal(a[3], kw["cu_seq_lens_q"]) and a[5] is a[3]
    assert type(a[4]) is int and a[4] == 64 and type(a[6]) is int and a[6] == 64
    assert c["softmax_n_param"] == 1.5 and c["is_causal"] is True and c["window"] is None and c["scale"] is None
    rec.clear()
    surgery._hf_attention(_module(causal=False), q, k, v, None, cu_seq_lens_q=kw["cu_seq_lens_q"], cu_seq_lens_k=cu64, max_length_q=64,
                          max_length_k=torch.tensor(70))
    a, c = rec.varlen[0]
    assert a[3] is kw["cu_seq_lens_q"] and a[5].dtype == torch.int32 and a[6] == 70 and type(a[6]) is int
    assert c["is_causal"] is False and c["softmax_n_param"] == 0.0
    with pytest.raises(ValueError, match="max_length_q"):   # offsets without a bound: an error, not a guess and not the dense route
        surgery._hf_attention(_module(), q, k, v, None, cu_seq_lens_q=kw["cu_seq_lens_q"])


def test_float16_scale_limit(surgery, rec, caplog):
    """float16 serves |scaling| * log2(e) <= 8: 5.5 is routed, -6 (8.66) takes the dense route; bfloat16 has no such limit"""
    kw = _keywords()
    q, k, v = _qkv(torch.float16)
    surgery._hf_attention(_module(), q, k, v, None, scaling=5.5, **kw)
    assert len(rec.varlen) == 1 and not rec.dense
    with caplog.at_level(logging.WARNING):
        surgery._hf_attention(_module(), q, k, v, None, scaling=-6.0, **kw)
    assert len(rec.varlen) == 1 and len(rec.dense) == 1 and "float16" in caplog.text
    q, k, v = _qkv(torch.bfloat16)
    surgery._hf_attention(_module(), q, k, v, None, scaling=-6.0, **kw)
    assert len(rec.varlen) == 2


FALLBACKS = {
    "batch_2": dict(qkv=dict(batch=2)),
    "float32": dict(qkv=dict(dtype=torch.float32)),
    "head_dim_32": dict(qkv=dict(e=32, ev=32)),
    "e_ne_ev": dict(qkv=dict(ev=32)),
    "dropout_training": dict(call=dict(dropout=0.1)),
    "window_zero": dict(kw=dict(sliding_window=0)),
    "window_bool": dict(kw=dict(sliding_window=True)),
    "window_not_causal": dict(kw=dict(sliding_window=16), causal=False),
    "window_kwarg_not_causal": dict(kw=dict(sliding_window=16, is_causal=False)),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_fallbacks_make_the_keywordless_call_and_warn_once(surgery, rec, caplog, name):
    """a packed batch that misses one condition of the route: exactly the flash_attention_n call the same arguments make without the
    packed keywords (the same operand objects, mask and keywords) and one warning per reason, however many layers ask"""
    case = FALLBACKS[name]
    q, k, v = _qkv(**case.get("qkv", {}))
    module = _module(causal=case.get("causal", True), n=0.25)
    mask = torch.ones(q.shape[0], 1, T, T, dtype=torch.bool).tril()
    s_aux = torch.linspace(-1.0, 1.0, H)
    extra = dict(s_aux=s_aux, **case.get("kw", {}))
    call = case.get("call", {})
    torch.manual_seed(3)
    want = surgery._hf_attention(module, q, k, v, mask, **call, **extra)[0]
    assert len(rec.dense) == 1 and not rec.varlen
    with caplog.at_level(logging.WARNING):
        for _ in range(3):
            torch.manual_seed(3)
            got = surgery._hf_attention(module, q, k, v, mask, **call, **extra, **_keywords())[0]
    assert not rec.varlen and len(rec.dense) == 4
    (a0, c0) = rec.dense[0]
    for a1, c1 in rec.dense[1:]:
        assert all(x is y for x, y in zip(a0, a1)) and len(a0) == len(a1) and sorted(c0) == sorted(c1)
        assert all(_same(c0[key], c1[key]) for key in c0), (c0, c1)
    assert torch.equal(got, want)
    lines = [r for r in caplog.records if "not routed" in r.getMessage()]
    assert len(lines) == 1, [r.getMessage() for r in lines]


def test_head_mask_stays_the_dense_routes_refusal(surgery, rec, caplog):
    q, k, v = _qkv()
    with caplog.at_level(logging.WARNING), pytest.raises(NotImplementedError, match="head_mask"):
        surgery._hf_attention(_module(), q, k, v, None, head_mask=torch.ones(H), **_keywords())
    assert not rec.varlen and not rec.dense and "head_mask" in caplog.text


def test_one_warning_per_distinct_reason(surgery, rec, caplog):
    kw = _keywords()
    with caplog.at_level(logging.WARNING):
        for _ in range(2):
            surgery._hf_attention(_module(), *_qkv(torch.float32), None, **kw)
            surgery._hf_attention(_module(), *_qkv(e=32, ev=32), None, **kw)
    lines = [r.getMessage() for r in caplog.records if "not routed" in r.getMessage()]
    assert len(lines) == 2 and "float32" in lines[0] and "head dim 32" in lines[1]


# ---------------------------------------------------------------- offsets from position_ids: the switch and its cache
def test_position_ids_route_only_with_the_switch(surgery, rec, monkeypatch):
    """switch off: position_ids alone never route (the call is the one without them). Switch on: the derived offsets are the collator's,
    int32, the bound the longest length; position_ids of another shape, or next to cu_seq_lens_q, are not looked at."""
    q, k, v = _qkv()
    inputs, kw, _ = hp.flat_batch(128)
    pos = inputs["position_ids"]
    count = hp.Counter(monkeypatch, surgery)
    surgery._hf_attention(_module(), q, k, v, None, position_ids=pos)
    assert len(rec.dense) == 1 and not rec.varlen and count.calls == 0
    monkeypatch.setattr(surgery, "HF_PACKED_FROM_POSITION_IDS", True)
    out = surgery._hf_attention(_module(), q, k, v, None, position_ids=pos, sliding_window=16)[0]
    assert len(rec.varlen) == 1 and count.calls == 1
    a, c = rec.varlen[0]
    assert a[3].dtype == torch.int32 and torch.equal(a[3], kw["cu_seq_lens_q"]) and a[5] is a[3] and a[4] == a[6] == 64 and type(a[4]) is int
    assert c["window"] == 16 and c["is_causal"] is True
    assert torch.equal(out, surgery._hf_attention(_module(), q, k, v, None, sliding_window=16, **kw)[0])
    rec.clear()
    surgery._hf_attention(_module(), q, k, v, None, position_ids=pos[:, :-1])                 # not [1, T]
    surgery._hf_attention(_module(), q, k, v, None, position_ids=pos.expand(3, 1, T))         # rotary sections
    surgery._hf_attention(_module(), *_qkv(batch=2), None, position_ids=pos.expand(2, T))    # an ordinary batch: no warning either
    assert len(rec.dense) == 3 and not rec.varlen and count.calls == 1 and not surgery._PACKED_WARNED
    surgery._hf_attention(_module(), q, k, v, None, position_ids=torch.zeros(1, T, dtype=torch.long), **kw)   # the keywords win
    assert len(rec.varlen) == 1 and rec.varlen[0][0][3] is kw["cu_seq_lens_q"] and count.calls == 1


def test_boundary_rule_of_the_derivation(surgery):
    """a sequence starts at token 0 and wherever a position is not its predecessor's plus one - whatever the first position is"""
    f = surgery._offsets_from_position_ids
    for pos, cu in (([0, 1, 2, 0, 0, 1], [0, 3, 4, 6]), ([5, 6, 7, 8], [0, 4]), ([2, 3, 2, 3, 4, 9], [0, 2, 5, 6]), ([0], [0, 1]), ([0, 0, 0], [0, 1, 2, 3]),
                    ([3, 2, 1], [0, 1, 2, 3])):
        got, longest = f(torch.tensor([pos]))
        assert got.dtype == torch.int32 and got.tolist() == cu and got.is_contiguous()
        assert longest == max(b - a for a, b in zip(cu, cu[1:])) and type(longest) is int


def test_derivation_is_shared_by_the_layers_of_a_forward(surgery, rec, monkeypatch):
    """one derivation for the two layers of a forward (the same position_ids object); again after the tensor is replaced - by an equal one
    too - or modified in place"""
    monkeypatch.setattr(surgery, "HF_PACKED_FROM_POSITION_IDS", True)
    count = hp.Counter(monkeypatch, surgery)
    q, k, v = _qkv()
    inputs, kw, _ = hp.flat_batch(128)
    pos = inputs["position_ids"]
    for _ in range(2):
        surgery._hf_attention(_module(), q, k, v, None, position_ids=pos)
    assert count.calls == 1 and rec.varlen[0][0][3] is rec.varlen[1][0][3]
    surgery._hf_attention(_module(), q, k, v, None, position_ids=pos.clone())
    assert count.calls == 2
    surgery._hf_attention(_module(), q, k, v, None, position_ids=pos)
    assert count.calls == 3
    pos[0, 10:] = torch.arange(T - 10)   # in place: documents (10, T - 10)
    surgery._hf_attention(_module(), q, k, v, None, position_ids=pos)
    assert count.calls == 4 and rec.varlen[-1][0][3].tolist() == [0, 10, T] and rec.varlen[-1][0][4] == T - 10


# ---------------------------------------------------------------- GPT-OSS on a flattened batch
def test_gpt_oss_flattened_batch_takes_the_packed_route(surgery, rec, monkeypatch):
    """A tiny bf16 GptOssForCausalLM on the CPU (bfloat16 applied: the MoE block runs in it here), documents (40, 1, 23, 64) flattened
    with the collator's keywords: the packed call answers once per layer - window 16 on the sliding layer, None on the full one, causal,
    the sinks as a tensor n -, flash_attention_n never, and the logits pass the model-level gate max |B - ref| <= 2 max |A' - ref| against
    the fp32 copy run with `eager` one document per call (A': the same bf16 model through this library, one document per call). GPT-OSS
    builds its masks without the documents' boundaries, so ignoring the keywords fails the gate by the logits' own size. With the
    opt-in switch and position_ids alone: the same bits, one derivation per forward."""
    pytest.importorskip("transformers")
    if not surgery.register_hf_attention():
        pytest.skip("transformers without AttentionInterface")
    pytest.importorskip("transformers.models.gpt_oss")
    cfg, model = hp.tiny_gpt_oss(torch.bfloat16)
    inputs, kw, docs = hp.flat_batch(cfg.vocab_size)
    with torch.no_grad():
        ref = [hp.fp32_copy(model)(input_ids=d).logits[0] for d in docs]
        model.config._attn_implementation = surgery.HF_ATTENTION_NAME
        a = [model(input_ids=d).logits[0].float() for d in docs]
        assert not rec.varlen and len(rec.dense) == 2 * len(docs)
        rec.clear()
        b = model(**inputs, **kw).logits[0].float()
    assert not rec.dense and len(rec.varlen) == cfg.num_hidden_layers
    assert [c["window"] for _, c in rec.varlen] == [16, None]
    for args, c in rec.varlen:
        assert c["is_causal"] is True and torch.is_tensor(c["softmax_n_param"]) and c["softmax_n_param"].shape == (4,)
        assert args[3] is kw["cu_seq_lens_q"] and args[4] == 64
    err_b = max((b[r] - w).abs().max().item() for r, w in zip(hp.rows(), ref))
    err_a = max((g - w).abs().max().item() for g, w in zip(a, ref))
    hp.gate([err_b], [err_a], "GPT-OSS on the CPU", names=("logits",))
    monkeypatch.setattr(surgery, "HF_PACKED_FROM_POSITION_IDS", True)
    count = hp.Counter(monkeypatch, surgery)
    rec.clear()
    with torch.no_grad():
        b2 = model(**inputs).logits[0].float()
    assert count.calls == 1 and len(rec.varlen) == 2 and not rec.dense and torch.equal(b2, b)
