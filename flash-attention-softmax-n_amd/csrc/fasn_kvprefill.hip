// K/V-cache prefill (include/fasn.h: fasn_fwd_kvprefill[_alibi|_window], fasn_kvprefill_append, fasn_kvprefill[_alibi|_window]_plan): argument checks, the launch plan -
// which depends on shapes and capacity only, never on the lengths in device memory - and the launches of fasn_kvprefill.h.
#include <limits.h>
#include <math.h>
#include "fasn.h"
#include "fasn_kvprefill.h"
#include "fasn_launch.h"

namespace fasn {
namespace {

bool kvp_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int kvp_check_view(const fasn_view4& v) {
    if (v.ptr == nullptr) return FASN_EINVAL;
    if (v.stride[3] != 1) return FASN_ESTRIDE;
    if (!kvp_aligned16(v.ptr)) return FASN_EALIGN;
    for (int i = 0; i < 3; ++i)
        if (v.stride[i] % 8 != 0) return FASN_EALIGN;
    return FASN_OK;
}

// Validation (no HIP call) + the kernel parameters: the rules of fasn_fwd_kvcache without its row limit. The plan: one workgroup per
// (batch element, K/V head, row block, split); splits by the decode rule with base = B * Hkv * row blocks, so a prefill whose row
// blocks fill the chip has one split, no partials and no combine launch.
int kvp_build(const fasn_kvprefill_args* pa, KvPrefillParams& pp) {
    if (pa == nullptr) return FASN_EINVAL;
    const fasn_kvcache_args* a = &pa->kv;
    if (a->B <= 0 || a->H <= 0 || a->Sq <= 0 || a->D <= 0 || a->page_size <= 0) return FASN_EINVAL;
    if (a->dtype != FASN_DTYPE_F16 && a->dtype != FASN_DTYPE_BF16) return FASN_EDTYPE;
    if (!kv_head_dim_ok(a->D)) return FASN_EHEADDIM;
    const int G = a->kv_group <= 1 ? 1 : a->kv_group;
    if (a->H % G != 0) return FASN_EINVAL;
    if (!(a->softmax_n >= 0.f) || !isfinite(a->scale)) return FASN_EINVAL;
    if (a->seqlens == nullptr || a->k_cache == nullptr || a->v_cache == nullptr) return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(a->seqlens) % 4 || reinterpret_cast<uintptr_t>(a->block_table) % 4 || reinterpret_cast<uintptr_t>(pa->q_seqlens) % 4) return FASN_EALIGN;
    if (a->seqlen_add != 0 && a->seqlen_add != a->Sq) return FASN_EINVAL;   // 0: the cache as it is; Sq: plus the qlen_b appended rows
    int rc;
    if ((rc = kvp_check_view(a->q))) return rc;
    if ((rc = kvp_check_view(a->o))) return rc;
    if (!kvp_aligned16(a->k_cache) || !kvp_aligned16(a->v_cache)) return FASN_EALIGN;
    for (int i = 0; i < 3; ++i)
        if (a->k_stride[i] % 8 != 0 || a->v_stride[i] % 8 != 0 || a->k_stride[i] < 0 || a->v_stride[i] < 0) return FASN_EALIGN;
    const bool paged = a->block_table != nullptr;
    if (paged && (a->max_pages <= 0 || a->block_table_stride < a->max_pages)) return FASN_EINVAL;
    if (paged && a->page_size % KV_KT != 0) return FASN_EUNSUPPORTED;   // a 64-key tile never straddles a page
    if (G > KVP_ROWS) return FASN_EUNSUPPORTED;                            // the query heads of a K/V head share one workgroup
    const int64_t capacity = paged ? (int64_t)a->max_pages * a->page_size : (int64_t)a->page_size;
    if (capacity > INT_MAX - 2 * KV_KT || (int64_t)a->Sq + capacity > INT_MAX) return FASN_EINVAL;
    // a tile's descriptor range and the lanes' offsets into it are 32-bit
    if ((int64_t)KV_KT * a->k_stride[1] * 2 >= (1ll << 31) || (int64_t)KV_KT * a->v_stride[1] * 2 >= (1ll << 31)) return FASN_EUNSUPPORTED;
    if (a->k_stride[1] < a->D || a->v_stride[1] < a->D) return FASN_EINVAL;
    if (a->n != nullptr) {
        if (reinterpret_cast<uintptr_t>(a->n) % 4) return FASN_EALIGN;
        if (a->n_stride_b < 0 || a->n_stride_h < 0 || (a->B - 1) * a->n_stride_b + (a->H - 1) * a->n_stride_h >= (1ll << 31)) return FASN_EINVAL;
    }
    pp = KvPrefillParams{};
    KvParams& p = pp.kv;
    p.q = static_cast<const char*>(a->q.ptr);
    p.o = static_cast<char*>(a->o.ptr);
    p.lse = a->lse;
    p.k = static_cast<char*>(a->k_cache);
    p.v = static_cast<char*>(a->v_cache);
    for (int i = 0; i < 3; ++i) {
        p.qs[i] = a->q.stride[i];
        p.os[i] = a->o.stride[i];
    }
    p.kps = a->k_stride[0], p.krs = a->k_stride[1], p.khs = a->k_stride[2];
    p.vps = a->v_stride[0], p.vrs = a->v_stride[1], p.vhs = a->v_stride[2];
    p.bt = a->block_table;
    p.bts = a->block_table_stride;
    p.seqlens = a->seqlens;
    p.seqlen_add = a->seqlen_add;
    p.page_size = a->page_size;
    p.tpp = paged ? a->page_size / KV_KT : INT_MAX;
    p.capacity = (int)capacity;
    p.B = a->B, p.H = a->H, p.G = G, p.Hkv = a->H / G, p.Sq = a->Sq, p.R = KVP_ROWS;
    p.causal = a->causal ? 1 : 0;
    p.c = a->scale * kLog2e;
    p.n = a->softmax_n;
    p.nt = a->n;
    p.nsb = (int)a->n_stride_b, p.nsh = (int)a->n_stride_h;
    pp.qlens = pa->q_seqlens;
    pp.PB = KVP_ROWS / G;
    pp.nrb = (a->Sq + pp.PB - 1) / pp.PB;
    const int64_t base = (int64_t)p.B * p.Hkv * pp.nrb;
    const int64_t cap_tiles = (capacity + KV_KT - 1) / KV_KT;
    // a split costs its partial (128 row slots of D + 2 floats, written and read back: what 4 tiles move) next to its tiles: at least
    // 16 tiles per split of a full cache (the decode rule at 128 rows)
    p.nsplit = (int)kv_nsplit(a->D, base, cap_tiles, KVP_ROWS / 8);
    if (base * p.nsplit > INT_MAX / KVP_ROWS) return FASN_EINVAL;
    return FASN_OK;
}
size_t kvp_ws_bytes(const KvPrefillParams& pp, int D) {
    if (pp.kv.nsplit <= 1) return 0;
    return (size_t)pp.kv.B * pp.kv.Hkv * pp.nrb * pp.kv.nsplit * KVP_ROWS * (size_t)(D + 2) * sizeof(float);
}

// The ALiBi operand of the *_alibi entry points (checked after the base arguments, before any HIP call): the rules of `n`
int kvp_build_alibi(const fasn_kvcache_args* a, const fasn_alibi_slopes* s, KvAlibi& al) {
    if (s == nullptr || s->slopes == nullptr) return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(s->slopes) % 4) return FASN_EALIGN;
    if (s->stride_b < 0 || s->stride_h < 0 || (a->B - 1) * s->stride_b + (a->H - 1) * s->stride_h >= (1ll << 31)) return FASN_EINVAL;
    al = KvAlibi{s->slopes, (int)s->stride_b, (int)s->stride_h};
    return FASN_OK;
}

// The window operand of the *_window entry points (checked after the base arguments, before any HIP call), and the plan under it: the
// base rule over the tiles a row block's window can touch, never more splits than the base plan has.
int kvp_build_window(const fasn_kvcache_args* a, const fasn_kv_window* w, KvPrefillParams& pp, KvWindow& kw) {
    KvParams& p = pp.kv;
    if (w == nullptr || w->window < 1 || w->reserved != 0) return FASN_EINVAL;
    if (!a->causal) return FASN_EUNSUPPORTED;
    kw = KvWindow{w->window < p.capacity ? w->window : p.capacity};
    const int64_t cap_tiles = ((int64_t)p.capacity + KV_KT - 1) / KV_KT;
    p.nsplit = (int)kv_nsplit(a->D, (int64_t)p.B * p.Hkv * pp.nrb, kv_window_tiles(cap_tiles, w->window, pp.PB), KVP_ROWS / 8);
    return FASN_OK;
}

// (al == kw == nullptr: the base kernel; otherwise its ALiBi sibling on the same grid, LDS and workspace, or its window sibling)
template <typename Tag, int D>
int kvp_launch_fwd(const KvPrefillParams& pp, const KvAlibi* al, const KvWindow* kw, hipStream_t s) {
    const KvParams& p = pp.kv;
    constexpr int smem = kv_smem(D);
    if (kw != nullptr) {
        constexpr auto kern = &fasn_kvprefill_fwd_window_kernel<Tag, D>;
        ensure_smem<kern>(smem);
        FASN_LAUNCH(kern, dim3((unsigned)(p.B * p.Hkv * pp.nrb * p.nsplit)), dim3(256), smem, s, pp, *kw);
    } else if (al == nullptr) {
        constexpr auto kern = &fasn_kvprefill_fwd_kernel<Tag, D>;
        ensure_smem<kern>(smem);
        FASN_LAUNCH(kern, dim3((unsigned)(p.B * p.Hkv * pp.nrb * p.nsplit)), dim3(256), smem, s, pp);
    } else {
        constexpr auto kern = &fasn_kvprefill_fwd_alibi_kernel<Tag, D>;
        ensure_smem<kern>(smem);
        FASN_LAUNCH(kern, dim3((unsigned)(p.B * p.Hkv * pp.nrb * p.nsplit)), dim3(256), smem, s, pp, *al);
    }
    if (p.nsplit > 1) {
        const int64_t nthr = (int64_t)p.B * p.Hkv * pp.nrb * KVP_ROWS * (D / 4);
        FASN_LAUNCH((fasn_kvprefill_combine_kernel<Tag, D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, pp);
    }
    return launch_rc();
}
template <int D>
int kvp_launch_append(const KvPrefillParams& pp, hipStream_t s) {
    const int64_t nthr = (int64_t)pp.kv.B * pp.kv.Hkv * pp.kv.Sq * (D / 8);
    if ((nthr + 255) / 256 > INT_MAX) return FASN_EINVAL;
    FASN_LAUNCH((fasn_kvprefill_append_kernel<D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, pp);
    return launch_rc();
}

template <typename Tag>
int kvp_launch_fwd_d(int D, const KvPrefillParams& pp, const KvAlibi* al, const KvWindow* kw, hipStream_t s) {   // (kvp_build let only these four through)
    switch (D) {
        case 32: return kvp_launch_fwd<Tag, 32>(pp, al, kw, s);
        case 64: return kvp_launch_fwd<Tag, 64>(pp, al, kw, s);
        case 128: return kvp_launch_fwd<Tag, 128>(pp, al, kw, s);
        default: return kvp_launch_fwd<Tag, 256>(pp, al, kw, s);
    }
}

int kvp_forward(const fasn_kvprefill_args* args, KvVariant variant, const void* operand, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    KvPrefillParams pp;
    int rc = kvp_build(args, pp);
    if (rc) return rc;
    KvAlibi al{};
    KvWindow kw{};
    if (variant == KV_ALIBI && (rc = kvp_build_alibi(&args->kv, static_cast<const fasn_alibi_slopes*>(operand), al))) return rc;
    if (variant == KV_WINDOW && (rc = kvp_build_window(&args->kv, static_cast<const fasn_kv_window*>(operand), pp, kw))) return rc;
    const int D = args->kv.D;
    const size_t need = kvp_ws_bytes(pp, D);
    if (need > 0) {   // (one split: nothing is written beside o / lse, a NULL workspace is fine)
        if (workspace == nullptr || workspace_bytes < need) return FASN_EWORKSPACE;
        if (!kvp_aligned16(workspace)) return FASN_EALIGN;
        pp.kv.part_o = static_cast<float*>(workspace);
        pp.kv.part_ml = pp.kv.part_o + (size_t)pp.kv.B * pp.kv.Hkv * pp.nrb * pp.kv.nsplit * KVP_ROWS * D;
    }
    hipStream_t s = (hipStream_t)stream;
    const KvAlibi* const alp = variant == KV_ALIBI ? &al : nullptr;
    const KvWindow* const kwp = variant == KV_WINDOW ? &kw : nullptr;
    if (args->kv.dtype == FASN_DTYPE_BF16) return kvp_launch_fwd_d<bf16_tag>(D, pp, alp, kwp, s);
    return kvp_launch_fwd_d<f16_tag>(D, pp, alp, kwp, s);
}

int kvp_plan(const fasn_kvprefill_args* args, KvVariant variant, const void* operand, char* buf, size_t cap) {
    if (args == nullptr || buf == nullptr || cap == 0) return FASN_EINVAL;
    LaunchLog log{buf, cap, 0};
    buf[0] = 0;
    LaunchLog* const outer = t_launch_log;
    t_launch_log = &log;
    const int rc = kvp_forward(args, variant, operand, reinterpret_cast<void*>(uintptr_t(256)), ~size_t(0), nullptr);   // (nothing is launched: any aligned address stands for the workspace)
    t_launch_log = outer;
    if (rc) return rc;
    return log.len > cap ? FASN_EINVAL : (int)log.len;
}

}  // namespace

// the validation and parameter packing above, for the rotary rotate-and-append call (fasn_kvrope.h declares it, fasn_kvrope.hip calls it)
int kvp_build_params(const fasn_kvprefill_args* pa, KvPrefillParams& pp) { return kvp_build(pa, pp); }

}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_fwd_kvprefill_workspace_bytes(const fasn_kvprefill_args* args) {
    KvPrefillParams pp;
    if (kvp_build(args, pp) != FASN_OK) return 0;
    return kvp_ws_bytes(pp, args->kv.D);
}

int fasn_fwd_kvprefill(const fasn_kvprefill_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kvp_forward(args, KV_BASE, nullptr, workspace, workspace_bytes, stream);
}

int fasn_fwd_kvprefill_alibi(const fasn_kvprefill_args* args, const fasn_alibi_slopes* alibi, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kvp_forward(args, KV_ALIBI, alibi, workspace, workspace_bytes, stream);
}

size_t fasn_fwd_kvprefill_window_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_window* window) {
    KvPrefillParams pp;
    KvWindow kw;
    if (kvp_build(args, pp) != FASN_OK || kvp_build_window(&args->kv, window, pp, kw) != FASN_OK) return 0;
    return kvp_ws_bytes(pp, args->kv.D);
}

int fasn_fwd_kvprefill_window(const fasn_kvprefill_args* args, const fasn_kv_window* window, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kvp_forward(args, KV_WINDOW, window, workspace, workspace_bytes, stream);
}

int fasn_kvprefill_append(const fasn_kvprefill_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    KvPrefillParams pp;
    int rc = kvp_build(args, pp);
    if (rc) return rc;
    if (k_new == nullptr || v_new == nullptr) return FASN_EINVAL;
    if ((rc = kvp_check_view(*k_new))) return rc;
    if ((rc = kvp_check_view(*v_new))) return rc;
    pp.kv.kn = static_cast<const char*>(k_new->ptr);
    pp.kv.vn = static_cast<const char*>(v_new->ptr);
    for (int i = 0; i < 3; ++i) {
        pp.kv.kns[i] = k_new->stride[i];
        pp.kv.vns[i] = v_new->stride[i];
    }
    hipStream_t s = (hipStream_t)stream;
    switch (args->kv.D) {
        case 32: return kvp_launch_append<32>(pp, s);
        case 64: return kvp_launch_append<64>(pp, s);
        case 128: return kvp_launch_append<128>(pp, s);
        default: return kvp_launch_append<256>(pp, s);
    }
}

int fasn_kvprefill_plan(const fasn_kvprefill_args* args, char* buf, size_t cap) { return kvp_plan(args, KV_BASE, nullptr, buf, cap); }

int fasn_kvprefill_alibi_plan(const fasn_kvprefill_args* args, const fasn_alibi_slopes* alibi, char* buf, size_t cap) {
    return kvp_plan(args, KV_ALIBI, alibi, buf, cap);
}

int fasn_kvprefill_window_plan(const fasn_kvprefill_args* args, const fasn_kv_window* window, char* buf, size_t cap) {
    return kvp_plan(args, KV_WINDOW, window, buf, cap);
}

}  // extern "C"
