// fasn_kv_host.h — the ONE host layer of the K/V-cache family (decode, prefill, packed prefill, rotary append): argument checks, parameter
// packing, the operand set of a call (KvOps) with its one check order and its table of supported sets, the launch plan, the workspace
// rule, the one forward / plan / workspace path, the token-tree commit and the dtype x head-dim dispatch.
// fasn_kvcache.hip defines what is declared here, but for the forward launchers: fasn_kvcache.hip, fasn_kvprefill.hip, fasn_kvvarlen.hip
// and fasn_kvfp8.hip each define the launcher of the kernels they instantiate (fasn_kvrope.hip: the rotary appends of every call).
#pragma once
#include <type_traits>
#include "fasn.h"
#include "fasn_kvvarlen.h"
#include "fasn_plan.h"

namespace fasn {

// Which call an argument block belongs to. Decode is the one-row-block case of prefill - the Sq positions of a K/V head are ONE block
// (PB = Sq, nrb = 1, R = G * Sq rows) - so both fill a KvPrefillParams and the decode kernels take its .kv. Where the checks differ,
// kv_build names the call. The packed call is a prefill whose row blocks come from an item table (fasn_kvvarlen.h): B sequences of up
// to Sq positions each, `packed` carries the offsets and the size of the token buffer.
enum KvCall { KV_DECODE, KV_PREFILL, KV_VARLEN };
struct KvArgs {
    const fasn_kvcache_args* a;   // nullptr: refused first, as a NULL block
    const int32_t* q_seqlens;     // the prefill block's; decode has none
    KvCall call;
    const fasn_kvvarlen_args* packed;   // KV_VARLEN only
};
inline KvArgs kv_args(const fasn_kvcache_args* a) { return {a, nullptr, KV_DECODE, nullptr}; }
inline KvArgs kv_args(const fasn_kvprefill_args* pa) { return {pa != nullptr ? &pa->kv : nullptr, pa != nullptr ? pa->q_seqlens : nullptr, KV_PREFILL, nullptr}; }
inline KvArgs kv_args(const fasn_kvvarlen_args* va) { return {va != nullptr ? &va->pf.kv : nullptr, va != nullptr ? va->pf.q_seqlens : nullptr, KV_VARLEN, va}; }

// The operands of a call beside its block, as a set. `takes` says which operands the entry point HAS; a NULL pointer of an operand it
// takes is refused by that operand's own rule, never read as "none". kv_ops(typed pointers...) builds one from what an entry point got.
enum : unsigned { KV_OP_ALIBI = 1, KV_OP_WINDOW = 2, KV_OP_TREE = 4, KV_OP_FP8 = 8 };
struct KvOps {
    unsigned takes;
    const fasn_alibi_slopes* alibi;
    const fasn_kv_window* window;
    const fasn_kv_tree* tree;
    const fasn_kv_fp8* fp8;
};
inline void kv_op(KvOps& o, const fasn_alibi_slopes* p) { o.takes |= KV_OP_ALIBI, o.alibi = p; }
inline void kv_op(KvOps& o, const fasn_kv_window* p) { o.takes |= KV_OP_WINDOW, o.window = p; }
inline void kv_op(KvOps& o, const fasn_kv_tree* p) { o.takes |= KV_OP_TREE, o.tree = p; }
inline void kv_op(KvOps& o, const fasn_kv_fp8* p) { o.takes |= KV_OP_FP8, o.fp8 = p; }
template <typename... P>
KvOps kv_ops(const P*... p) {
    KvOps o{};
    (kv_op(o, p), ...);
    return o;
}

// The operand sets a forward has kernels for, stated once: every other set is FASN_EUNSUPPORTED, behind the base checks. Decode and
// prefill have the sets of kKvOpSets; the packed call (KV_VARLEN) has the base and the window kernels, over a 16-bit and an FP8 cache.
constexpr unsigned kKvOpSets[] = {0, KV_OP_ALIBI, KV_OP_WINDOW, KV_OP_TREE, KV_OP_FP8, KV_OP_FP8 | KV_OP_WINDOW, KV_OP_FP8 | KV_OP_TREE};
constexpr bool kv_ops_supported(KvCall call, unsigned takes) {
    if (call == KV_VARLEN) return (takes & ~(KV_OP_FP8 | KV_OP_WINDOW)) == 0;
    for (unsigned s : kKvOpSets)
        if (s == takes) return true;
    return false;
}

// what a forward launches with: the parameters, the operand set (KvOps::takes) and the operands as the kernels take them
struct KvFwd {
    KvPrefillParams pp;
    unsigned ops;
    int dtype, D;         // the block's: what the launchers dispatch on
    KvAlibi al;           // KV_OP_ALIBI
    KvWindow kw;          // KV_OP_WINDOW
    KvPacked pk;          // KV_VARLEN only
    KvTree kt;            // KV_OP_TREE
    KvFp8 f8;             // KV_OP_FP8
};

inline bool kv_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int kv_check_view(const fasn_view4& v);                                     // the rules of q: o, q_out, k_new, v_new
// the base checks (no HIP call), the parameters, the plan; the packed call: then the checks of its own operands, and `pk`
int kv_build(const KvArgs& in, KvPrefillParams& pp, KvPacked* pk = nullptr);
int kv_pack_new(const fasn_view4& k_new, const fasn_view4& v_new, KvParams& p);   // the views' checks, then p.kn / vn / kns / vns
int kv_build_append(const KvArgs& in, const fasn_view4* k_new, const fasn_view4* v_new, KvPrefillParams& pp, KvPacked* pk = nullptr);
// the token-tree operand's checks, behind the base arguments' (the tree forwards and the tree rotary appends share them): `kt` with the
// window as the kernels take it - capacity + 1 when there is none
int kv_check_tree(const fasn_kvcache_args* a, const fasn_kv_tree* t, int capacity, KvTree& kt);
// the FP8 operand's checks, behind the base arguments' (the FP8 forwards and the quantising appends share them): the scales, and the rules
// of a cache whose strides count bytes
int kv_check_fp8(const fasn_kvcache_args* a, const fasn_kv_fp8* o, KvFp8& f8);
// the checks of a fasn_kv_tree_commit block and the kernel's parameters (no HIP call). `fp8`: the cache holds codes - strides count bytes
// and follow the FP8 calls' 16-byte rule, D is 64 or 128
int kv_build_commit(const fasn_kv_tree_commit* a, bool fp8, KvCommit& c);
// The one forward path. Behind the base checks the operands are checked in ONE order, each at most once - FP8, tree, window, ALiBi - then
// the workspace; then the launcher of the call's translation unit runs. kv_forward_plan is the same call under the launch recorder
// (record_plan, fasn_plan.h), with plan_workspace() and a size of ~size_t(0) standing for the workspace.
size_t kv_workspace_bytes(const KvArgs& in, const KvOps& ops);
int kv_forward(const KvArgs& in, const KvOps& ops, void* workspace, size_t workspace_bytes, fasn_stream_t stream);
int kv_forward_plan(const KvArgs& in, const KvOps& ops, char* buf, size_t cap);
// The launchers, each defined beside the kernels it instantiates: it picks the kernel of f.ops among those its translation unit holds
// and adds the combine (decode: always; prefill and packed: when there is more than one split).
int kv_launch_decode(const KvFwd& f, hipStream_t s);        // fasn_kvcache.hip
int kv_launch_prefill(const KvFwd& f, hipStream_t s);       // fasn_kvprefill.hip
int kv_launch_packed(const KvFwd& f, hipStream_t s);        // fasn_kvvarlen.hip
int kv_launch_fp8_decode(const KvFwd& f, hipStream_t s);    // fasn_kvfp8.hip
int kv_launch_fp8_prefill(const KvFwd& f, hipStream_t s);   // fasn_kvfp8.hip
int kv_launch_fp8_packed(const KvFwd& f, hipStream_t s);    // fasn_kvfp8.hip
// The appends, each defined beside the kernels it launches: the plain appends of the three blocks, the quantising append of any block
// (base checks, the new rows' views, then kv_check_fp8) and the one path of every rotary append - `ops`: FP8 and / or tree (fasn_kvrope.hip).
// fasn_kv_append (fasn_kvcall.hip) picks among them as the named entry points do.
int kv_append(const fasn_kvcache_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);      // fasn_kvcache.hip
int kvp_append(const fasn_kvprefill_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);   // fasn_kvprefill.hip
int kvv_append(const fasn_kvvarlen_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);    // fasn_kvvarlen.hip
int kv8_append(const KvArgs& in, const fasn_kv_fp8* fp8, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream);   // fasn_kvfp8.hip
int kvr_call(const KvArgs& in, const KvOps& ops, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new,
             fasn_stream_t stream);
// fasn_kvcache_tree_commit / fasn_kvcache_fp8_tree_commit: kv_build_commit, the grid (a thread per 16-byte chunk of a row: D / 8 elements,
// D / 16 codes), then the one launch from the kernel's translation unit
int kv_commit(const fasn_kv_tree_commit* a, bool fp8, fasn_stream_t stream);
int kv_launch_commit(const KvCommit& c, int D, unsigned grid, hipStream_t s);       // fasn_kvcache.hip
int kv_launch_fp8_commit(const KvCommit& c, int D, unsigned grid, hipStream_t s);   // fasn_kvfp8.hip

// dtype x head dim -> f(tag, std::integral_constant<int, D>) (kv_build let only these four head dims through)
template <typename F>
int kv_dispatch_d(int D, F f) {
    switch (D) {
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        default: return f(std::integral_constant<int, 256>{});
    }
}
template <typename F>
int kv_dispatch(int dtype, int D, F f) {
    if (dtype == FASN_DTYPE_BF16) return kv_dispatch_d(D, [&](auto d) { return f(bf16_tag{}, d); });
    return kv_dispatch_d(D, [&](auto d) { return f(f16_tag{}, d); });
}

// dtype x the two head dims the FP8 kernels and the kernels behind shared prefixes (fasn_kvprefix.hip) are built for (kv_check_fp8 and
// the prefix calls' builder let only these through)
template <typename F>
int kv8_dispatch(int dtype, int D, F f) {
    if (dtype == FASN_DTYPE_BF16) return D == 64 ? f(bf16_tag{}, std::integral_constant<int, 64>{}) : f(bf16_tag{}, std::integral_constant<int, 128>{});
    return D == 64 ? f(f16_tag{}, std::integral_constant<int, 64>{}) : f(f16_tag{}, std::integral_constant<int, 128>{});
}

// the one launch of the family's kernels with their trailing arguments: workgroups of 256, the dynamic-LDS attribute where it is needed
template <auto Kern, typename... A>
void kv_launch(unsigned grid, int smem, hipStream_t s, const A&... a) {
    ensure_smem<Kern>(smem);
    FASN_LAUNCH(Kern, dim3(grid), dim3(256), smem, s, a...);
}

}  // namespace fasn
