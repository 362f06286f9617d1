"""Model surgery: put softmax_n attention (the HIP kernel) into existing models.

Mirrors the reference's surgery interface without its MosaicML-composer dependency:
    policy_registry / PolicyRegistry.register   surgery/surgery_functions/utils.py:12-97   (same signature rules and errors)
    apply_attention_softmax_n(model, n, opts)    surgery/attention_softmax_n.py:19-63       (module replacement by policy)
A surgery function has the signature `(module: torch.nn.Module, module_index: int, softmax_n_param: float)` and returns the
module to keep in the model (the same object, modified in place, or a new one) or None to leave it alone.

Built-in policy: Hugging Face self-attention modules that dispatch through `transformers.AttentionInterface`
(transformers >= 4.48; BERT / RoBERTa here). The reference re-implements `BertSelfAttention.forward` around its eager
`softmax_n` (surgery_functions/_bert.py:24-121, pinned to transformers < 4.33); here the module keeps its own forward and its
attention function becomes `flash_attention_n` — fused, no [B,H,L,S] score tensor. XLNet (surgery_functions/_xlnet.py:25-75
re-implements `rel_attn_core` around the eager softmax_n): here `rel_attn_core` keeps computing the position and segment
scores, which become the `attn_bias` of one fused `flash_attention_n` call for content score, softmax_n, dropout and PV.
"""
from __future__ import annotations

import inspect
import logging
from typing import Callable, Dict, Optional, Sequence, Type, Union

import torch
from torch.nn import Module
from torch.optim import Optimizer

log = logging.getLogger(__name__)

AttentionSoftmaxNReplacementFunction = Callable[[Module, int, float], Optional[Module]]
HF_ATTENTION_NAME = "softmax_n_hip"   # key under which the attention function is registered with transformers

__all__ = ["PolicyRegistry", "policy_registry", "apply_attention_softmax_n", "register_hf_attention", "HF_ATTENTION_NAME"]



class PolicyRegistry(Dict[Type[Module], AttentionSoftmaxNReplacementFunction]):
    """module class -> surgery function (reference surgery_functions/utils.py:12-93)."""

    def register(self, *modules: Type[Module]):
        if len(modules) == 0:
            raise ValueError("register() needs at least one torch.nn.Module class to attach the surgery function to")

        def check_signature(func: Callable) -> None:
            params = list(inspect.signature(func).parameters.items())
            if len(params) != 3:
                raise ValueError(f"a surgery function takes (module, module_index, softmax_n_param); {func} takes {len(params)} arguments")
            (_, p_module), (_, p_index), (n_name, p_n) = params
            # annotations may be strings under `from __future__ import annotations`
            def is_(annotation, typ, name):
                return annotation is typ or annotation == name or annotation == f"torch.nn.{name}" or annotation == f"nn.{name}"
            if not is_(p_module.annotation, Module, "Module"):
                raise TypeError(f'the first argument of surgery function {func} must be annotated "torch.nn.Module"')
            if not is_(p_index.annotation, int, "int"):
                raise TypeError(f'the second argument of surgery function {func} must be annotated "int"')
            if not is_(p_n.annotation, float, "float"):
                raise TypeError(f'the third argument of surgery function {func} must be annotated "float"')
            if n_name != "softmax_n_param":
                raise NameError(f'the third argument of surgery function {func} must be named "softmax_n_param"')

        def wrapper(func: AttentionSoftmaxNReplacementFunction) -> AttentionSoftmaxNReplacementFunction:
            check_signature(func)
            for m in modules:
                if not (isinstance(m, type) and issubclass(m, Module)):
                    raise TypeError(f"{getattr(m, '__name__', m)} is not a subclass of torch.nn.Module")
                if m in self:
                    raise ValueError(f"a surgery function is already registered for {m.__name__}")
                self[m] = func
            return func

        return wrapper


policy_registry = PolicyRegistry()


def _swap_optimizer_params(optimizers, old: Module, new: Module) -> None:
    """keep optimizers that were built on `model.parameters()` pointing at the parameters of the replacement module"""
    if optimizers is None:
        return
    if isinstance(optimizers, Optimizer):
        optimizers = [optimizers]
    old_params = list(old.parameters())
    new_params = list(new.parameters())
    if {id(p) for p in old_params} == {id(p) for p in new_params}:
        return
    for opt in optimizers:
        for group in opt.param_groups:
            kept = [p for p in group["params"] if all(p is not q for q in old_params)]
            if len(kept) != len(group["params"]):     # this group held the old module's parameters
                for p in old_params:
                    opt.state.pop(p, None)
                group["params"] = kept + [p for p in new_params if all(p is not q for q in kept)]
                new_params = []


def apply_attention_softmax_n(model: Module, softmax_n_param: float,
                              optimizers: Optional[Union[Optimizer, Sequence[Optimizer]]] = None) -> int:
    """Run every registered surgery function over the matching sub-modules of `model` (reference
    surgery/attention_softmax_n.py:19-63). Returns the number of modules converted; logs a warning when it is 0."""
    replaced = 0
    index = 0
    # parents first, children collected before any replacement so a replacement's own sub-modules are not revisited
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            func = next((f for cls, f in policy_registry.items() if type(child) is cls), None)
            if func is None:
                func = next((f for cls, f in policy_registry.items() if isinstance(child, cls)), None)
            if func is None:
                continue
            new = func(child, index, softmax_n_param=float(softmax_n_param))
            index += 1
            if new is None:
                continue
            if new is not child:
                setattr(parent, name, new)
                _swap_optimizer_params(optimizers, child, new)
            replaced += 1
    if replaced == 0:
        supported = "".join(sorted("\n\t" + c.__module__ + "." + c.__name__ for c in policy_registry))
        log.warning("AttentionSoftmaxN had no effect on the model! Supported module classes: %s", supported)
    else:
        log.info("%d instances of AttentionSoftmaxN added", replaced)
    return replaced


# ------------------------------------------------------------------------------------------- Hugging Face transformers
def _hf_attention(module: Module, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                  attention_mask: Optional[torch.Tensor], scaling: Optional[float] = None, dropout: float = 0.0, **kwargs):
    """`transformers` attention-interface function: [B,H,L,E] in, ([B,L,H,Ev], None) out. The additive float mask HF builds
    ([B,1,L,S], finfo.min where hidden) is passed as `attn_bias` through its broadcast strides.
    Attention sinks (`s_aux`, GPT-OSS: one learned logit s_h per query head, a softmax column that is dropped after the softmax) are
    softmax_n with n_h = exp(s_h): they add to a surgery n (n_h = softmax_n_param + exp(s_h)) and their gradient reaches the sink
    parameter. Causality follows transformers' SDPA integration: the `is_causal` kwarg, else the module's `is_causal` attribute, and
    only for more than one query row and no mask (a mask, when given, already holds the causal pattern).

    Padding-free batches: with `cu_seq_lens_q` among the keywords - what `DataCollatorWithFlattening(
    return_flash_attn_kwargs=True)` adds to a flattened [1, T] batch - the call goes to `flash_attention_n_varlen` on the
    [T, H, E] views of query, key and value (no copy, no repeat_kv): `cu_seq_lens_q / _k` are the offsets (int32 on the query's device
    goes in as the same object; int64 or CPU offsets are converted on the way), `max_length_q / _k` the bounds (Python ints as they are;
    a 0-d tensor becomes int(x), ONE HOST READ per call - pass ints), `sliding_window` the call's `window`, causality the `is_causal`
    kwarg, else the module's attribute (the conditions "more than one row" and "no mask" do not apply: the offsets replace the mask).
    `attention_mask` is NOT READ on this route: the offsets must describe every token, which is the contract of transformers' own
    flash-attention path. The result is the packed call's [T, H, E] output as [1, T, H, E], no transpose and no copy. The route needs
    batch 1, fp16 / bf16, E == Ev in flash_attn._VARLEN_D, no active dropout, no head_mask, a sliding window only on a causal call
    and, for fp16, |scaling| * log2(e) <= 8; anything else takes the dense route below exactly as without the packed keywords, after
    one warning per reason and process. The device is not tested: on CPU tensors flash_attention_n_varlen raises its own error.
    With HF_PACKED_FROM_POSITION_IDS set and no `cu_seq_lens_q`, the offsets are derived from a [1, T] `position_ids`
    (_offsets_from_position_ids: one host read per forward, shared by the layers)."""
    packed = _hf_packed_operands(module, query, key, value, scaling, dropout, kwargs)
    if packed is not None:
        from .flash_attn import flash_attention_n_varlen
        cu_q, cu_k, max_q, max_k, n, is_causal, window = packed
        out = flash_attention_n_varlen(query[0].transpose(0, 1), key[0].transpose(0, 1), value[0].transpose(0, 1), cu_q, max_q, cu_k, max_k,
                                       softmax_n_param=n, scale=scaling, is_causal=is_causal, window=window)
        return out.unsqueeze(0), None
    from .flash_attn import flash_attention_n
    n = float(getattr(module, "softmax_n_param", 0.0))
    s_aux = kwargs.get("s_aux")
    if s_aux is not None:
        n = torch.exp(s_aux.float()) + n   # [H]: one n per query head
    is_causal = kwargs.get("is_causal")
    if is_causal is None:
        is_causal = getattr(module, "is_causal", False)
    is_causal = bool(is_causal) and query.shape[2] > 1 and attention_mask is None
    if kwargs.get("head_mask") is not None:
        raise NotImplementedError("head_mask multiplies the attention probabilities, which the fused kernel never materialises")
    bias = mask = None
    if attention_mask is not None:
        if attention_mask.dtype == torch.bool:
            mask = attention_mask[..., : key.shape[-2]]   # row stride 0 (from _hf_mask) -> the key-padding kernels
        else:
            bias = attention_mask[..., : key.shape[-2]]
            keymask = _as_key_padding_mask(bias)
            if keymask is not None:
                # row-broadcast additive mask: its hidden keys as the kernels' key-padding mask (padded tiles skipped). HF builds
                # these as 0 / finfo.min from a binary mask, so the visible entries add nothing and the bias is dropped - unless
                # ADDITIVE_KEY_MASKS_MAY_BE_SOFT says a caller feeds non-binary masks: then the finite entries stay a [B,1,1,S] bias
                mask = keymask
                bias = torch.where(keymask, bias[..., :1, :], torch.zeros((), dtype=bias.dtype, device=bias.device)) if ADDITIVE_KEY_MASKS_MAY_BE_SOFT else None
    out = flash_attention_n(query, key, value, softmax_n_param=n, scale=scaling, dropout_p=dropout if module.training else 0.0,
                            attn_mask=mask, attn_bias=bias, is_causal=is_causal)
    return out.transpose(1, 2).contiguous(), None


# ---- padding-free (packed) batches: transformers' flash-attention keywords -> flash_attention_n_varlen
# transformers hands every layer `position_ids`, so deriving the offsets from them cannot be automatic: it would change the bits of
# every existing batch-1 call and add a host read. Set this to True to route a [1, T] batch whose `position_ids` restart (and that comes
# without `cu_seq_lens_q`) through the packed call: a sequence starts at token 0 and wherever a position is not its predecessor's + 1.
HF_PACKED_FROM_POSITION_IDS = False

_PACKED_WARNED = set()      # the reasons a packed batch took the dense route, each logged once per process
_POSITION_IDS_CACHE = None  # (weakref of the position_ids tensor, its _version, device, (cu, max_len)): the layers of one forward share it


def _packed_fallback(reason: str) -> None:
    if reason not in _PACKED_WARNED:
        _PACKED_WARNED.add(reason)
        log.warning("packed-batch keywords (cu_seq_lens_q / position_ids) are not routed to flash_attention_n_varlen: %s; the call takes "
                    "the dense route, where only attention_mask separates the documents", reason)


def _packed_refusal(module, query, key, value, scaling, dropout, kwargs) -> Optional[str]:
    """why this call cannot go to flash_attention_n_varlen, or None (the conditions of the packed route, nothing read on the host)"""
    from . import flash_attn
    if query.dim() != 4 or query.shape[0] != 1:
        return "query is not [1, H, T, E] (batch greater than 1)"
    if key.dim() != 4 or value.dim() != 4 or key.shape[0] != 1 or value.shape[0] != 1:
        return "key / value are not [1, Hkv, T, E] (batch greater than 1)"
    if query.dtype not in (torch.float16, torch.bfloat16):
        return f"dtype {query.dtype} (the packed kernels serve float16 and bfloat16)"
    E, Ev = query.shape[-1], value.shape[-1]
    if E != Ev or key.shape[-1] != E or E not in flash_attn._VARLEN_D:
        return f"head dim {E} / {Ev} (the packed kernels serve E == Ev in {list(flash_attn._VARLEN_D)})"
    if dropout and module.training:
        return "attention dropout in training (there is no dropout on packed operands)"
    if kwargs.get("head_mask") is not None:
        return "head_mask is given"
    window = kwargs.get("sliding_window")
    if window is not None:
        if isinstance(window, bool) or not isinstance(window, int) or window < 1:
            return f"sliding_window {window!r} is not an int >= 1"
        if not _packed_is_causal(module, kwargs):
            return "sliding_window on a call that is not causal (the packed window is causal)"
    if query.dtype == torch.float16:
        scale = E ** -0.5 if scaling is None else abs(float(scaling))
        # (in fp32, as flash_attention_n_varlen forms it: a scale within a rounding of the limit gets the same answer here and there)
        if float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(flash_attn._VARLEN_LOG2E, dtype=torch.float32)) > flash_attn._VARLEN_F16_MAX_PRESCALE:
            return f"float16 with |scaling| = {scale:g} (|scaling| * log2(e) must be <= {flash_attn._VARLEN_F16_MAX_PRESCALE:g})"
    return None


def _packed_is_causal(module, kwargs) -> bool:
    is_causal = kwargs.get("is_causal")
    return bool(getattr(module, "is_causal", False) if is_causal is None else is_causal)


def _packed_offsets(cu: torch.Tensor, device) -> torch.Tensor:
    """an offset table as the packed call reads it: int32 on the query's device (such a tensor is returned as it is)"""
    if cu.device != device:
        cu = cu.to(device)
    return cu if cu.dtype == torch.int32 else cu.to(torch.int32)


def _offsets_from_position_ids(position_ids: torch.Tensor):
    """(cu_seqlens int32 [B + 1] on position_ids' device, longest length as a Python int) of a flattened [1, T] batch, by the boundary
    rule of transformers' packed masks: a sequence starts at token 0 and wherever a position is not its predecessor's plus one.
    Torch ops on the device and ONE host read (B and the longest length together)."""
    pos = position_ids.reshape(-1)
    T = pos.numel()
    start = torch.ones(T, dtype=torch.bool, device=pos.device)
    start[1:] = pos[1:] != pos[:-1] + 1
    at = torch.arange(T + 1, device=pos.device)
    # the starts in order, then T for every token that starts nothing and once more as cu[B]: no nonzero(), whose size is a host read
    table = torch.where(torch.cat([start, start.new_zeros(1)]), at, at.new_full((), T)).sort().values
    B, longest = torch.stack([start.sum(), (table[1:] - table[:-1]).max()]).tolist()
    return table[:B + 1].to(torch.int32), int(longest)


def _cached_offsets_from_position_ids(position_ids: torch.Tensor, device):
    """_offsets_from_position_ids once per tensor OBJECT and version (a weakref compared with `is`, plus `_version`; never an address -
    see _as_key_padding_mask): the layers of one forward get the same position_ids and share the derivation and its host read."""
    global _POSITION_IDS_CACHE
    import weakref
    c = _POSITION_IDS_CACHE
    if c is not None and c[0]() is position_ids and c[1] == position_ids._version and c[2] == device:
        return c[3]
    cu, longest = _offsets_from_position_ids(position_ids)
    got = (_packed_offsets(cu, device), longest)
    _POSITION_IDS_CACHE = (weakref.ref(position_ids), position_ids._version, device, got)
    return got


def _hf_packed_operands(module, query, key, value, scaling, dropout, kwargs):
    """(cu_q, cu_k, max_q, max_k, n, is_causal, window) of the packed route of _hf_attention, or None: not a packed batch, or one of the
    route's conditions fails (logged once per reason)."""
    cu_q = kwargs.get("cu_seq_lens_q")
    position_ids = None
    if cu_q is None:
        position_ids = kwargs.get("position_ids") if HF_PACKED_FROM_POSITION_IDS else None
        if (not torch.is_tensor(position_ids) or query.dim() != 4 or key.dim() != 4
                or tuple(position_ids.shape) != (1, query.shape[2]) or key.shape[2] != query.shape[2]):
            return None
    reason = _packed_refusal(module, query, key, value, scaling, dropout, kwargs)
    if reason is not None:
        _packed_fallback(reason)
        return None
    if cu_q is None:
        cu_q, max_q = _cached_offsets_from_position_ids(position_ids, query.device)
        cu_k, max_k = cu_q, max_q
    else:
        given_k = kwargs.get("cu_seq_lens_k")
        cu_q_in, cu_q = cu_q, _packed_offsets(cu_q, query.device)
        cu_k = cu_q if given_k is None or given_k is cu_q_in else _packed_offsets(given_k, query.device)
        max_q, max_k = kwargs.get("max_length_q"), kwargs.get("max_length_k")
        if max_q is None:
            raise ValueError("cu_seq_lens_q came without max_length_q: the packed call needs a bound of the sequence lengths (the collator "
                             "passes both, as transformers' flash-attention path requires)")
        max_q = int(max_q)   # a Python int as it is; a 0-d tensor: one host read
        max_k = max_q if max_k is None else int(max_k)
    n = float(getattr(module, "softmax_n_param", 0.0))
    s_aux = kwargs.get("s_aux")
    if s_aux is not None:
        n = torch.exp(s_aux.float()) + n   # [H]: one n per query head
    window = kwargs.get("sliding_window")
    return cu_q, cu_k, max_q, max_k, n, _packed_is_causal(module, kwargs), None if window is None else int(window)


# transformers' extended attention mask is (1 - mask) * finfo.min: 0 / min for the binary masks tokenizers produce. A float mask
# with values strictly between 0 and 1 ("soft" masking) gives finite non-zero additive entries; set this to True to keep them as
# an additive key bias next to the key-padding mask (the bias + key-padding kernels instead of the plain key-padding ones).
ADDITIVE_KEY_MASKS_MAY_BE_SOFT = False


def _as_key_padding_mask(additive: torch.Tensor) -> Optional[torch.Tensor]:
    """Older `transformers` versions (and direct callers) hand every layer an ADDITIVE mask, [B,1,1,S] (or a row-broadcast
    expansion of it) with 0 for real tokens and a huge negative number for padding. A row-broadcast additive mask yields the
    boolean key mask `additive > -1e4` WITHOUT inspecting its values on the host (no device synchronisation, nothing cached -
    a cache keyed on the tensor's address would return a previous batch's mask once the allocator reuses the address):
    entries at or below the threshold (finfo.min, -inf, -1e9, -1e4) are hidden keys - the kernels skip their tiles.
    The VALUES above the threshold are not looked at here: `_hf_attention` drops them (0 by HF's construction) unless
    ADDITIVE_KEY_MASKS_MAY_BE_SOFT is set, in which case it keeps them as an additive key bias next to this mask.
    Anything with a real row dimension (e.g. causal) returns None and stays an additive bias only."""
    if additive.dim() != 4 or additive.shape[1] != 1:
        return None
    if additive.shape[-2] != 1:
        if additive.stride(-2) != 0:
            return None
        additive = additive[..., :1, :]   # expanded view of a row-broadcast mask
    return additive > -1e4


def _hf_mask(batch_size: int, cache_position: Optional[torch.Tensor] = None, kv_length: Optional[int] = None, kv_offset: int = 0,
             mask_function=None, attention_mask: Optional[torch.Tensor] = None, q_length: Optional[int] = None, q_offset: int = 0,
             **kwargs):
    """`transformers.AttentionMaskInterface` function for HF_ATTENTION_NAME. Without a registered mask function transformers
    hands a custom attention function `attention_mask=None` - every layer would silently attend to padding tokens.
    Both calling conventions are served: transformers 4.53 - 4.5x pass `cache_position` (the query positions), newer versions
    `q_length` / `q_offset`; whatever was received is forwarded to transformers' own `sdpa_mask`.
    Bidirectional models with a 2-D padding mask get it back as a boolean [B,1,L,S] view with ROW STRIDE 0 (True = attend),
    which is exactly the kernels' key-padding form (one byte per key, padded tiles skipped); everything else (causal,
    sliding window, packed sequences, or/and-mask functions) is built by transformers' own boolean `sdpa_mask`."""
    import inspect
    from transformers import masking_utils as mu
    if q_length is None and cache_position is not None:
        q_length = int(cache_position.shape[0])
    if (attention_mask is not None and attention_mask.dim() == 2 and kv_length is not None and q_length is not None
            and mask_function is getattr(mu, "bidirectional_mask_function", object())
            and attention_mask.shape[-1] >= kv_offset + kv_length):
        keys = attention_mask[:, kv_offset:kv_offset + kv_length].to(torch.bool)
        return keys[:, None, None, :].expand(batch_size, 1, q_length, kv_length)
    kwargs.pop("allow_is_bidirectional_skip", None)
    # never "skip" to None for a padded batch; an all-True mask may still come back as None, which means "no mask"
    have = dict(batch_size=batch_size, cache_position=cache_position, kv_length=kv_length, kv_offset=kv_offset,
                mask_function=mask_function, attention_mask=attention_mask, q_length=q_length, q_offset=q_offset, **kwargs)
    params = inspect.signature(mu.sdpa_mask).parameters
    if not any(prm.kind is inspect.Parameter.VAR_KEYWORD for prm in params.values()):
        have = {k_: v_ for k_, v_ in have.items() if k_ in params}   # this version's sdpa_mask takes only what it names
    elif "cache_position" not in params:
        have.pop("cache_position", None)
    if mask_function is None:
        have.pop("mask_function", None)   # sdpa_mask's own default (causal)
    return mu.sdpa_mask(**have)


def register_hf_attention() -> bool:
    """Register the attention function with transformers (once) and the built-in surgery policy for the self-attention
    classes of the installed version. Returns False when transformers has no AttentionInterface."""
    try:
        from transformers import AttentionInterface
    except Exception:   # transformers missing or too old
        return False
    if HF_ATTENTION_NAME not in AttentionInterface._global_mapping:
        AttentionInterface.register(HF_ATTENTION_NAME, _hf_attention)
    try:   # the padding mask only reaches a custom attention function whose name also has a mask function
        from transformers import AttentionMaskInterface
        if HF_ATTENTION_NAME not in AttentionMaskInterface._global_mapping:
            AttentionMaskInterface.register(HF_ATTENTION_NAME, _hf_mask)
    except ImportError:   # transformers 4.48 - 4.52: the model builds the additive mask itself and passes it on
        pass
    classes = []
    for mod_name, cls_names in (("transformers.models.bert.modeling_bert", ("BertSelfAttention", "BertCrossAttention")),
                                ("transformers.models.roberta.modeling_roberta", ("RobertaSelfAttention", "RobertaCrossAttention"))):
        try:
            mod = __import__(mod_name, fromlist=list(cls_names))
        except Exception:
            continue
        classes += [getattr(mod, c) for c in cls_names if hasattr(mod, c)]
    classes = [c for c in classes if c not in policy_registry]
    if classes:
        policy_registry.register(*classes)(hf_self_attention_surgery)
    try:
        from transformers.models.xlnet.modeling_xlnet import XLNetRelativeAttention
        if XLNetRelativeAttention not in policy_registry:
            policy_registry.register(XLNetRelativeAttention)(xlnet_relative_attention_surgery)
    except Exception:
        pass
    return True


def hf_self_attention_surgery(module: Module, module_index: int, softmax_n_param: float) -> Optional[Module]:
    """Built-in policy for HF self-attention modules: remember n on the module and route its attention call to the HIP
    kernel (the module's projections, cache handling and output reshaping stay its own)."""
    del module_index
    config = getattr(module, "config", None)
    if config is None or not hasattr(config, "_attn_implementation"):
        return None
    module.softmax_n_param = float(softmax_n_param)
    config._attn_implementation = HF_ATTENTION_NAME   # the config object is shared by all layers of the model
    return module


# ------------------------------------------------------------------------------------------------------------ XLNet
def _xlnet_rel_attn_core(self, q_head, k_head_h, v_head_h, k_head_r, seg_mat=None, attn_mask=None, head_mask=None,
                         output_attentions=False, **kwargs):
    """Replacement for `XLNetRelativeAttention.rel_attn_core` (same arguments and return value; tensors are [len, batch,
    head, dim]). Position (bd) and segment (ef) scores are computed as the module always did and enter one fused
    `flash_attention_n` call as the additive bias; the content score, softmax_n, dropout and the weighted sum happen in the
    kernel. With `output_attentions=True` the probabilities must be returned, so that case takes the module's own einsum
    route with the softmax_n row kernel."""
    from .flash_attn import flash_attention_n
    from .softmax import softmax_n
    n = float(getattr(self, "softmax_n_param", 0.0))
    bd = torch.einsum("ibnd,jbnd->bnij", q_head + self.r_r_bias, k_head_r)
    bd = self.rel_shift_bnij(bd, klen=k_head_h.shape[0])
    if seg_mat is None:
        extra = bd
    else:
        ef = torch.einsum("ibnd,snd->ibns", q_head + self.r_s_bias, self.seg_embed)
        extra = bd + torch.einsum("ijbs,ibns->bnij", seg_mat, ef)
    visible = None
    if attn_mask is not None:          # [i, j, b, n] (n may be 1), 1 = masked
        # (contiguous: the comparison keeps the permuted memory order of its input, whose key stride is not 1 - such a mask takes the
        # element-load kernels; [b, n or 1, i, j] with unit key stride takes the vector path, the head broadcast stays a stride 0)
        visible = (torch.einsum("ijbn->bnij", attn_mask) == 0).contiguous()
    if output_attentions or head_mask is not None:
        # the probabilities themselves are wanted (or multiplied by head_mask, as transformers 4.x passes it and the reference's
        # rel_attn_core applies it, surgery_functions/_xlnet.py:66-67): the module's einsum route with the softmax_n row kernel
        ac = torch.einsum("ibnd,jbnd->bnij", q_head + self.r_w_bias, k_head_h)
        score = (ac + extra) * self.scale
        if visible is not None:
            score = score.masked_fill(~visible, float("-inf"))
        prob = self.dropout(softmax_n(score, n=n, dim=3))
        if head_mask is not None:
            prob = prob * torch.einsum("ijbn->bnij", head_mask)
        if not output_attentions:
            return torch.einsum("bnij,jbnd->ibnd", prob, v_head_h)
        return torch.einsum("bnij,jbnd->ibnd", prob, v_head_h), torch.einsum("bnij->ijbn", prob)
    q = (q_head + self.r_w_bias).permute(1, 2, 0, 3)      # [b, n, i, d]
    k = k_head_h.permute(1, 2, 0, 3)
    v = v_head_h.permute(1, 2, 0, 3)
    out = flash_attention_n(q, k, v, softmax_n_param=n, scale=self.scale, attn_bias=extra * self.scale, attn_mask=visible,
                            dropout_p=self.dropout.p if self.training else 0.0)
    return out.permute(2, 0, 1, 3)                          # [i, b, n, d]


def xlnet_relative_attention_surgery(module: Module, module_index: int, softmax_n_param: float) -> Optional[Module]:
    """Built-in policy for `transformers` XLNetRelativeAttention (reference surgery_functions/_xlnet.py:11-22)."""
    from types import MethodType
    del module_index
    if not hasattr(module, "rel_attn_core") or not hasattr(module, "rel_shift_bnij"):
        return None
    module.softmax_n_param = float(softmax_n_param)
    module.rel_attn_core = MethodType(_xlnet_rel_attn_core, module)
    return module
