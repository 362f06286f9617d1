// fasn_kv_host.h — the ONE host layer of the K/V-cache family (decode, prefill, packed prefill, rotary append): argument checks, parameter
// packing, the launch plan, the workspace rule, the launch recorder and the dtype x head-dim dispatch. fasn_kvcache.hip defines what is
// declared here; fasn_kvcache.hip, fasn_kvprefill.hip, fasn_kvvarlen.hip, fasn_kvrope.hip and fasn_kvfp8.hip each instantiate and launch the
// kernels of their own header (fasn_kvrope.hip: also the packed rotary append, fasn_kvvarlen.hip: also the packed window forward,
// fasn_kvfp8.hip: the decode and the prefill call over an FP8 cache).
#pragma once
#include <type_traits>
#include "fasn.h"
#include "fasn_kvvarlen.h"
#include "fasn_launch.h"

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

// what a forward launches with: the parameters, the variant and its operand
struct KvFwd {
    KvPrefillParams pp;
    KvVariant variant;
    KvAlibi al;
    KvWindow kw;
    KvPacked pk;          // KV_VARLEN only
    KvTree kt;            // KV_TREE and KV_FP8_TREE
    KvFp8 f8;             // KV_FP8, KV_FP8_WINDOW (which fills kw too) and KV_FP8_TREE (which fills kt too)
};
// the operand of KV_FP8_WINDOW: the two operands its entry points take, checked in this order
struct KvFp8Window {
    const fasn_kv_fp8* fp8;
    const fasn_kv_window* window;
};

// the operand of KV_FP8_TREE, likewise: the FP8 operand's checks, then the tree operand's
struct KvFp8Tree {
    const fasn_kv_fp8* fp8;
    const fasn_kv_tree* tree;
};

inline bool kv_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int kv_check_view(const fasn_view4& v);                                     // the rules of q: o, q_out, k_new, v_new
// the base checks (no HIP call), the parameters, the plan; the packed call: then the checks of its own operands, and `pk`
int kv_build(const KvArgs& in, KvPrefillParams& pp, KvPacked* pk = nullptr);
int kv_pack_new(const fasn_view4& k_new, const fasn_view4& v_new, KvParams& p);   // the views' checks, then p.kn / vn / kns / vns
int kv_build_append(const KvArgs& in, const fasn_view4* k_new, const fasn_view4* v_new, KvPrefillParams& pp, KvPacked* pk = nullptr);
size_t kv_workspace_bytes(const KvArgs& in, KvVariant variant, const void* operand);
// the token-tree operand's checks, behind the base arguments' (the tree forwards and the tree rotary appends share them): `kt` with the
// window as the kernels take it - capacity + 1 when there is none
int kv_check_tree(const fasn_kvcache_args* a, const fasn_kv_tree* t, int capacity, KvTree& kt);
// the FP8 operand's checks, behind the base arguments' (the FP8 forwards and the quantising appends share them): the scales, and the rules
// of a cache whose strides count bytes
int kv_check_fp8(const fasn_kvcache_args* a, const fasn_kv_fp8* o, KvFp8& f8);
// the checks of a fasn_kv_tree_commit block and the kernel's parameters (no HIP call). `fp8`: the cache holds codes - strides count bytes
// and follow the FP8 calls' 16-byte rule, D is 64 or 128
int kv_build_commit(const fasn_kv_tree_commit* a, bool fp8, KvCommit& c);
// everything a forward does before its launches: base checks, the variant's operand (nothing, a fasn_alibi_slopes, a fasn_kv_window, a
// fasn_kv_tree, a fasn_kv_fp8), then the workspace
int kv_build_forward(const KvArgs& in, KvVariant variant, const void* operand, void* workspace, size_t workspace_bytes, KvFwd& f);

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

// The forward kernel of f.variant - the base kernel, or its ALiBi or window sibling on the same grid and LDS. `p` is what the kernels
// take first: f.pp.kv (decode) or f.pp (prefill).
template <auto Base, auto Alibi, auto Window, typename P>
void kv_launch_variant(const KvFwd& f, const P& p, unsigned grid, int smem, hipStream_t s) {
    if (f.variant == KV_WINDOW) {
        ensure_smem<Window>(smem);
        FASN_LAUNCH(Window, dim3(grid), dim3(256), smem, s, p, f.kw);
    } else if (f.variant == KV_ALIBI) {
        ensure_smem<Alibi>(smem);
        FASN_LAUNCH(Alibi, dim3(grid), dim3(256), smem, s, p, f.al);
    } else {
        ensure_smem<Base>(smem);
        FASN_LAUNCH(Base, dim3(grid), dim3(256), smem, s, p);
    }
}

// ... and its token-tree sibling (KV_TREE), on the same grid and LDS: no packed call has one, so it stays out of the list above
template <auto Tree, typename P>
void kv_launch_tree(const KvFwd& f, const P& p, unsigned grid, int smem, hipStream_t s) {
    ensure_smem<Tree>(smem);
    FASN_LAUNCH(Tree, dim3(grid), dim3(256), smem, s, p, f.kt);
}

// A call's launches as text: the call itself under the launch recorder (nothing is launched, no device is touched). The forwards are
// recorded with kv_plan_workspace() and a size of ~size_t(0) standing for the workspace: any aligned address will do.
inline void* kv_plan_workspace() { return reinterpret_cast<void*>(uintptr_t(256)); }
template <typename Call>
int kv_plan(char* buf, size_t cap, Call call) {
    if (buf == nullptr || cap == 0) return FASN_EINVAL;
    LaunchLog log{buf, cap, 0};
    buf[0] = 0;
    LaunchLog* const outer = t_launch_log;
    t_launch_log = &log;
    const int rc = call();
    t_launch_log = outer;
    if (rc) return rc;
    return log.len > cap ? FASN_EINVAL : (int)log.len;
}

}  // namespace fasn
