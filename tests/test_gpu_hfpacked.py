"""The packed route of surgery._hf_attention on the GPU: transformers' padding-free keywords (cu_seq_lens_q / _k, max_length_q /
_k, sliding_window) reach flash_attention_n_varlen. Function level - the bits of the direct packed call on the transposed views, judged per
sequence against the fp32 references of tests/attn_varlen.py and tests/attn_varlen_window.py -, the offset forms, GPT-OSS and a Llama at
model level against fp32 `eager`, the fallbacks and the opt-in switch that derives the offsets from position_ids."""
import logging
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_varlen as av            # noqa: E402
import attn_varlen_window as aww    # noqa: E402
import hf_packed as hp              # noqa: E402

pytestmark = pytest.mark.gpu

D = 64
SCALE = 0.125   # 64 ** -0.5, what transformers passes as `scaling` at head dim 64 and what the references use


@pytest.fixture
def surgery(pkg, monkeypatch):
    pytest.importorskip("transformers")
    from flash_attention_softmax_n_amd import surgery as s
    if not s.register_hf_attention():
        pytest.skip("transformers without AttentionInterface")
    monkeypatch.setattr(s, "_PACKED_WARNED", set(), raising=False)
    monkeypatch.setattr(s, "_POSITION_IDS_CACHE", None, raising=False)
    monkeypatch.setattr(s, "HF_PACKED_FROM_POSITION_IDS", False, raising=False)
    return s


# ---------------------------------------------------------------- 1. function level, bit for bit
def _stub(causal):
    m = torch.nn.Module()
    m.is_causal = causal
    return m


def _operands(inp, dev):
    """query [1, H, T, 64], key, value [1, Hkv, T, 64] contiguous as transformers hands them, s_aux [H] and dO [1, T, H, 64]: fresh leaves"""
    query, key, value = (inp[x].to(dev).transpose(0, 1).unsqueeze(0).contiguous().requires_grad_() for x in ("q", "k", "v"))
    s = torch.linspace(-1.0, 1.0, av.H, device=dev).requires_grad_()
    return query, key, value, s, inp["do"].to(dev).unsqueeze(0)


def _through_hf(surgery, inp, dev, causal, window, forms=lambda kw: kw):
    pack = av.SEAMS
    query, key, value, s, do = _operands(inp, dev)
    cu = torch.tensor(pack.cu_q, dtype=torch.int32, device=dev)
    kw = forms(dict(cu_seq_lens_q=cu, cu_seq_lens_k=cu.clone(), max_length_q=pack.max_q, max_length_k=pack.max_k))
    if window is not None:
        kw["sliding_window"] = window
    out, weights = surgery._hf_attention(_stub(causal), query, key, value, None, scaling=SCALE, dropout=0.0, s_aux=s, **kw)
    assert weights is None and out.shape == (1, pack.Tq, av.H, D) and out.is_contiguous()
    out.backward(do)
    torch.cuda.synchronize()
    return out.detach(), query.grad, key.grad, value.grad, s.grad


def _direct(pkg, inp, dev, causal, window):
    pack = av.SEAMS
    query, key, value, s, do = _operands(inp, dev)
    cu = torch.tensor(pack.cu_q, dtype=torch.int32, device=dev)
    out = pkg.flash_attention_n_varlen(query[0].transpose(0, 1), key[0].transpose(0, 1), value[0].transpose(0, 1), cu, pack.max_q, cu, pack.max_k,
                                       softmax_n_param=torch.exp(s.float()) + 0.0, scale=SCALE, is_causal=causal, window=window)
    out.backward(do[0])
    torch.cuda.synchronize()
    return out.detach().unsqueeze(0), query.grad, key.grad, value.grad, s.grad


NAMES = ("out", "d query", "d key", "d value", "d s_aux")
MODES = {"causal": (True, None), "window16": (True, 16), "window100": (True, 100), "plain": (False, None)}
FUNCTION_CASES = [(dt, hkv, m) for dt in (torch.float16, torch.bfloat16) for hkv in (4, 2) for m in ("causal", "window16", "window100")]
FUNCTION_CASES.append((torch.bfloat16, 2, "plain"))   # module.is_causal = False


@pytest.mark.parametrize("dtype,Hkv,mode", FUNCTION_CASES, ids=lambda x: str(x).replace("torch.", ""))
def test_function_level_is_the_direct_packed_call(pkg, dev, surgery, dtype, Hkv, mode):
    """_hf_attention on a stub module over av.SEAMS (lengths that straddle every tile edge, 40 token rows behind cu[B]), s_aux requiring
    grad: out and the gradients of query, key, value and s_aux are, by torch.equal, those of flash_attention_n_varlen on the transposed
    views; out is judged per sequence against the fp32 reference (under the band where a window is set); the rows behind cu[B] are 0."""
    causal, window = MODES[mode]
    pack = av.SEAMS
    inp = av.inputs(pack, Hkv, D, dtype, seed=2801 + Hkv)
    got = _through_hf(surgery, inp, dev, causal, window)
    want = _direct(pkg, inp, dev, causal, window)
    for g, w, nm in zip(got, want, NAMES):
        assert g.shape == w.shape and torch.equal(g, w), f"{nm}: differs from the direct flash_attention_n_varlen call"
    s = torch.linspace(-1.0, 1.0, av.H)
    key = ("hfpacked", dtype, Hkv, mode)
    ref = av.reference(key, pack, inp, None, causal, log_n=s) if window is None else aww.reference(key, pack, inp, None, window, log_n=s)
    out = got[0][0]
    for b in range(pack.B):
        r = av.seq_rows(pack, "q", b)
        if r.stop > r.start:
            av.check(out[r], ref["out"][r], dtype, f"{mode} Hkv={Hkv} sequence {b} ({pack.lens_q[b]} tokens) out")
    assert pack.Tq > pack.cu_q[-1] and not out[pack.cu_q[-1]:].any(), "rows behind cu[B] must be exactly 0"


# ---------------------------------------------------------------- 2. offset forms
@pytest.mark.parametrize("form", ["int64", "cpu", "cpu_int64", "tensor_maxima", "no_k_side"])
def test_offset_forms_give_the_same_bits(dev, surgery, form):
    """int64 offsets, CPU-resident offsets, 0-d tensor maxima and a missing key side: the bits of the int32 / Python-int call"""
    inp = av.inputs(av.SEAMS, 2, D, torch.bfloat16, seed=2803)

    def forms(kw):
        if form in ("int64", "cpu_int64"):
            kw["cu_seq_lens_q"], kw["cu_seq_lens_k"] = kw["cu_seq_lens_q"].long(), kw["cu_seq_lens_k"].long()
        if form in ("cpu", "cpu_int64"):
            kw["cu_seq_lens_q"], kw["cu_seq_lens_k"] = kw["cu_seq_lens_q"].cpu(), kw["cu_seq_lens_k"].cpu()
        if form == "tensor_maxima":
            kw["max_length_q"], kw["max_length_k"] = torch.tensor(kw["max_length_q"], device=dev), torch.tensor(kw["max_length_k"])
        if form == "no_k_side":
            kw["cu_seq_lens_k"] = kw["max_length_k"] = None
        return kw

    want = _through_hf(surgery, inp, dev, True, 16)
    got = _through_hf(surgery, inp, dev, True, 16, forms)
    for g, w, nm in zip(got, want, NAMES):
        assert torch.equal(g, w), f"{form}: {nm} differs"


# ---------------------------------------------------------------- 3. GPT-OSS at model level
@pytest.fixture(scope="module")
def gpt(dev):
    pytest.importorskip("transformers")
    cfg, model = hp.tiny_gpt_oss(torch.bfloat16, dev)
    inputs, kw, docs = hp.flat_batch(cfg.vocab_size, dev)
    return cfg, model, inputs, kw, docs


def test_gpt_oss_packed_batch_against_fp32_eager(dev, surgery, gpt, monkeypatch):
    """Tiny bf16 GPT-OSS (sliding 16 + full, 4 / 2 heads, head dim 64, random sinks), documents (40, 1, 23, 64). ref: the fp32 copy with
    `eager`, one document per call. B: the flattened batch through this library with the collator's keywords. A': the same bf16 model
    through this library one document per call. Per document the logits, the sink gradients and the embedding gradient under the loss of
    tests/test_gpu_sinks.py (the document's squared logits); gate max |B - ref| <= 2 max |A' - ref| for each of the three. The packed
    call answers once per layer with window 16 / None. Without the route GPT-OSS's masks carry no boundaries and the gate fails."""
    cfg, model, inputs, kw, docs = gpt
    spy = hp.Recorder(monkeypatch, stub=False)
    print("ref (fp32 eager, per document) against itself: the per-document errors below are A' and B")
    ref = hp.per_doc(hp.fp32_copy(model), "eager", [(dict(input_ids=d), {}) for d in docs])
    a = hp.per_doc(model, surgery.HF_ATTENTION_NAME, [(dict(input_ids=d), {}) for d in docs])
    assert not spy.varlen and len(spy.dense) == cfg.num_hidden_layers * len(docs)
    spy.clear()
    b = hp.per_doc(model, surgery.HF_ATTENTION_NAME, [(inputs, kw)], doc_rows=hp.rows())
    print("A' (one document per call):")
    err_a = hp.errors(a, ref)
    print("B (packed):")
    err_b = hp.errors(b, ref)
    hp.gate(err_b, err_a, "GPT-OSS")
    assert not spy.dense and [c["window"] for _, c in spy.varlen] == [16, None]


# ---------------------------------------------------------------- 4. Llama at model level
def test_llama_packed_batch_against_dense_masks(dev, surgery, monkeypatch):
    """LlamaConfig with head_dim 64, 4 / 2 heads, 2 layers, bf16. A: the dense block-diagonal masks transformers builds from
    position_ids (the keywords withheld: flash_attention_n answers). B: the packed route with the collator's keywords
    (flash_attention_n_varlen once per layer, flash_attention_n never). ref: fp32 `eager` on the same flattened batch - which itself
    must equal its one-document-per-call runs. Gate on the logits: max |B - ref| <= 2 max |A - ref|."""
    cfg, model = hp.tiny_llama(torch.bfloat16, dev)
    inputs, kw, docs = hp.flat_batch(cfg.vocab_size, dev)
    spy = hp.Recorder(monkeypatch, stub=False)
    with torch.no_grad():
        ref_model = hp.fp32_copy(model)
        ref_model.config._attn_implementation = "eager"
        ref = ref_model(**inputs).logits[0]
        alone = torch.cat([ref_model(input_ids=d).logits[0] for d in docs])
        assert (ref - alone).abs().max().item() <= 1e-4 * alone.abs().max().item(), "the reference must separate the documents"
        model.config._attn_implementation = surgery.HF_ATTENTION_NAME
        a = model(**inputs).logits[0].float()
        assert len(spy.dense) == cfg.num_hidden_layers and not spy.varlen
        assert all(c.get("attn_mask") is not None for _, c in spy.dense)
        spy.clear()
        b = model(**inputs, **kw).logits[0].float()
    err_a, err_b = (a - ref).abs().max().item(), (b - ref).abs().max().item()
    hp.gate([err_b], [err_a], "Llama", names=("logits",))
    assert len(spy.varlen) == cfg.num_hidden_layers and not spy.dense
    assert all(c["window"] is None and c["is_causal"] is True for _, c in spy.varlen)


# ---------------------------------------------------------------- 5. fallbacks
@pytest.mark.parametrize("which", ["gpt_oss_fp32", "llama_head_dim_32"])
def test_fallbacks_give_the_keywordless_bits_and_warn_once(dev, surgery, monkeypatch, caplog, which):
    """a packed batch the packed kernels do not serve (fp32; head dim 32): the bits of the same run with the keywords withheld, the packed
    call never made, one warning for all the layers"""
    if which == "gpt_oss_fp32":
        cfg, model = hp.tiny_gpt_oss(torch.float32, dev)
    else:
        cfg, model = hp.tiny_llama(torch.bfloat16, dev, head_dim=32)
    inputs, kw, _ = hp.flat_batch(cfg.vocab_size, dev)
    model.config._attn_implementation = surgery.HF_ATTENTION_NAME
    spy = hp.Recorder(monkeypatch, stub=False)
    with torch.no_grad(), caplog.at_level(logging.WARNING):
        want = model(**inputs).logits
        assert not [r for r in caplog.records if "not routed" in r.getMessage()]
        got = model(**inputs, **kw).logits
        again = model(**inputs, **kw).logits
    assert torch.equal(got, want) and torch.equal(again, want)
    assert not spy.varlen and len(spy.dense) == 3 * cfg.num_hidden_layers
    lines = [r.getMessage() for r in caplog.records if "not routed" in r.getMessage()]
    assert len(lines) == 1 and ("float32" if which == "gpt_oss_fp32" else "head dim 32") in lines[0], lines


# ---------------------------------------------------------------- 6. the opt-in switch
def test_position_ids_route_is_opt_in(dev, surgery, gpt, monkeypatch):
    """switch on, position_ids alone: the bits of the keyword route (case 3's B) with one derivation per forward; switch off: the bits of
    the run without the keywords, flash_attention_n answering"""
    cfg, model, inputs, kw, _ = gpt
    model.config._attn_implementation = surgery.HF_ATTENTION_NAME
    spy = hp.Recorder(monkeypatch, stub=False)
    count = hp.Counter(monkeypatch, surgery)
    with torch.no_grad():
        b = model(**inputs, **kw).logits
        assert len(spy.varlen) == cfg.num_hidden_layers and not spy.dense
        off = model(**inputs).logits
        assert len(spy.varlen) == cfg.num_hidden_layers and len(spy.dense) == cfg.num_hidden_layers and count.calls == 0
        monkeypatch.setattr(surgery, "HF_PACKED_FROM_POSITION_IDS", True)
        on = model(**inputs).logits
        assert count.calls == 1 and len(spy.varlen) == 2 * cfg.num_hidden_layers
        on2 = model(input_ids=inputs["input_ids"], position_ids=inputs["position_ids"].clone()).logits
        assert count.calls == 2 and len(spy.dense) == cfg.num_hidden_layers
        monkeypatch.setattr(surgery, "HF_PACKED_FROM_POSITION_IDS", False)
        off2 = model(**inputs).logits   # (the switch and its cache leave nothing behind)
        assert count.calls == 2 and len(spy.dense) == 2 * cfg.num_hidden_layers
    assert torch.equal(on, b) and torch.equal(on2, b) and torch.equal(off2, off)
    assert not torch.equal(off, b)   # (GPT-OSS's own masks carry no boundaries: the keyword-less run attends across the documents)
