// The K/V-cache calls by operand set (include/fasn.h: fasn_kv_forward_workspace_bytes, fasn_kv_forward, fasn_kv_forward_plan, fasn_kv_append,
// fasn_kv_append_plan): the family's one host path (fasn_kv_host.h: kv_forward, kv_forward_plan, kv_workspace_bytes, the appends) with the
// operand set taken as data - a fasn_kv_call names the block and the operands present. Nothing is checked here but the call itself; a
// named entry point and the call of its set run the same functions, so they agree on every code, byte count and plan line.
#include "fasn_kv_host.h"

namespace fasn {

namespace {

// the call itself: a block of the kind it names, nothing reserved
bool kvc_ok(const fasn_kv_call* c) {
    return c != nullptr && c->block != nullptr && c->kind >= FASN_KV_CALL_DECODE && c->kind <= FASN_KV_CALL_PACKED && c->reserved == 0;
}
KvArgs kvc_args(const fasn_kv_call* c) {
    if (c->kind == FASN_KV_CALL_PACKED) return kv_args(static_cast<const fasn_kvvarlen_args*>(c->block));
    if (c->kind == FASN_KV_CALL_PREFILL) return kv_args(static_cast<const fasn_kvprefill_args*>(c->block));
    return kv_args(static_cast<const fasn_kvcache_args*>(c->block));
}
// the operand set of a forward: the non-NULL pointers
KvOps kvc_ops(const fasn_kv_call* c) {
    KvOps o{};
    if (c->fp8 != nullptr) kv_op(o, c->fp8);
    if (c->tree != nullptr) kv_op(o, c->tree);
    if (c->window != nullptr) kv_op(o, c->window);
    if (c->alibi != nullptr) kv_op(o, c->alibi);
    return o;
}
// ... and of an append: the FP8 operand, the tree under a rope operand only; the window and the slopes take no part
KvOps kvc_append_ops(const fasn_kv_call* c, const fasn_kv_rope* rope) {
    KvOps o{};
    if (c->fp8 != nullptr) kv_op(o, c->fp8);
    if (rope != nullptr && c->tree != nullptr) kv_op(o, c->tree);
    return o;
}

// the append of the call's set, as the named entry points pick it: with `rope` the rotary path, without it the quantising append when the
// FP8 operand is there, the block's plain append otherwise
int kvc_append(const fasn_kv_call* c, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new,
               fasn_stream_t stream) {
    const KvArgs in = kvc_args(c);
    const KvOps ops = kvc_append_ops(c, rope);
    if (rope != nullptr) return kvr_call(in, ops, rope, q_out, k_new, v_new, stream);
    if (ops.takes & KV_OP_FP8) return kv8_append(in, ops.fp8, k_new, v_new, stream);
    if (c->kind == FASN_KV_CALL_PACKED) return kvv_append(static_cast<const fasn_kvvarlen_args*>(c->block), k_new, v_new, stream);
    if (c->kind == FASN_KV_CALL_PREFILL) return kvp_append(static_cast<const fasn_kvprefill_args*>(c->block), k_new, v_new, stream);
    return kv_append(static_cast<const fasn_kvcache_args*>(c->block), k_new, v_new, stream);
}

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_kv_forward_workspace_bytes(const fasn_kv_call* call) {
    if (!kvc_ok(call)) return 0;
    return kv_workspace_bytes(kvc_args(call), kvc_ops(call));
}

int fasn_kv_forward(const fasn_kv_call* call, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    if (!kvc_ok(call)) return FASN_EINVAL;
    return kv_forward(kvc_args(call), kvc_ops(call), workspace, workspace_bytes, stream);
}

int fasn_kv_forward_plan(const fasn_kv_call* call, char* buf, size_t cap) {
    if (!kvc_ok(call)) return FASN_EINVAL;
    return kv_forward_plan(kvc_args(call), kvc_ops(call), buf, cap);
}

int fasn_kv_append(const fasn_kv_call* call, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new,
                   fasn_stream_t stream) {
    if (!kvc_ok(call)) return FASN_EINVAL;
    return kvc_append(call, rope, q_out, k_new, v_new, stream);
}

int fasn_kv_append_plan(const fasn_kv_call* call, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                        const fasn_view4* v_new, char* buf, size_t cap) {
    if (!kvc_ok(call)) return FASN_EINVAL;
    return record_plan(buf, cap, [&] { return kvc_append(call, rope, q_out, k_new, v_new, nullptr); });
}

}  // extern "C"
