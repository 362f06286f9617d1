// K/V-cache forward (include/fasn.h: fasn_fwd_kvcache[_alibi|_window], fasn_kvcache_append, fasn_kvcache[_alibi|_window]_plan): argument checks, the launch plan -
// which depends on shapes and capacity only, never on the lengths in device memory - and the three launches of fasn_kvcache.h.
#include <limits.h>
#include <math.h>
#include "fasn.h"
#include "fasn_kvcache.h"
#include "fasn_launch.h"

namespace fasn {
namespace {

bool kv_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int kv_check_view(const fasn_view4& v) {
    if (v.ptr == nullptr) return FASN_EINVAL;
    if (v.stride[3] != 1) return FASN_ESTRIDE;
    if (!kv_aligned16(v.ptr)) return FASN_EALIGN;
    for (int i = 0; i < 3; ++i)
        if (v.stride[i] % 8 != 0) return FASN_EALIGN;
    return FASN_OK;
}

// Validation (no HIP call) + the kernel parameters. The plan: one workgroup per (batch element, K/V head, split); as many splits as
// bring the grid to ~1024 workgroups (the split-K forward's target; ~512 at D = 256, kv_split_target), each with enough tiles of a FULL
// cache to pay for its partial. Head dims: 32, 64, 128, 256 (kv_head_dim_ok).
// a split costs its partial (R rows of D + 2 floats, written and read back) next to its tiles (64 keys of K and V): at least 4 tiles
// per split of a full cache, R / 8 when there are many rows (128 rows: the partial moves what 4 tiles do)
int64_t kv_min_tps(int R) { return R / 8 > 4 ? R / 8 : 4; }

int kv_build(const fasn_kvcache_args* a, KvParams& p) {
    if (a == nullptr) return FASN_EINVAL;
    if (a->B <= 0 || a->H <= 0 || a->Sq <= 0 || a->D <= 0 || a->page_size <= 0) return FASN_EINVAL;
    if (a->dtype != FASN_DTYPE_F16 && a->dtype != FASN_DTYPE_BF16) return FASN_EDTYPE;
    if (!kv_head_dim_ok(a->D)) return FASN_EHEADDIM;
    const int G = a->kv_group <= 1 ? 1 : a->kv_group;
    if (a->H % G != 0) return FASN_EINVAL;
    if (!(a->softmax_n >= 0.f) || !isfinite(a->scale)) return FASN_EINVAL;
    if (a->seqlens == nullptr || a->k_cache == nullptr || a->v_cache == nullptr) return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(a->seqlens) % 4 || reinterpret_cast<uintptr_t>(a->block_table) % 4) return FASN_EALIGN;
    int rc;
    if ((rc = kv_check_view(a->q))) return rc;
    if ((rc = kv_check_view(a->o))) return rc;
    if (!kv_aligned16(a->k_cache) || !kv_aligned16(a->v_cache)) return FASN_EALIGN;
    for (int i = 0; i < 3; ++i)
        if (a->k_stride[i] % 8 != 0 || a->v_stride[i] % 8 != 0 || a->k_stride[i] < 0 || a->v_stride[i] < 0) return FASN_EALIGN;
    const bool paged = a->block_table != nullptr;
    if (paged && (a->max_pages <= 0 || a->block_table_stride < a->max_pages)) return FASN_EINVAL;
    if (paged && a->page_size % KV_KT != 0) return FASN_EUNSUPPORTED;   // a 64-key tile never straddles a page
    if ((int64_t)G * a->Sq > 128) return FASN_EUNSUPPORTED;               // the rows of a K/V head are one pass of one workgroup
    const int64_t capacity = paged ? (int64_t)a->max_pages * a->page_size : (int64_t)a->page_size;
    if (capacity > INT_MAX - 2 * KV_KT || (int64_t)a->seqlen_add + capacity > INT_MAX) return FASN_EINVAL;
    // a tile's descriptor range and the lanes' offsets into it are 32-bit
    if ((int64_t)KV_KT * a->k_stride[1] * 2 >= (1ll << 31) || (int64_t)KV_KT * a->v_stride[1] * 2 >= (1ll << 31)) return FASN_EUNSUPPORTED;
    if (a->k_stride[1] < a->D || a->v_stride[1] < a->D) return FASN_EINVAL;
    if (a->n != nullptr) {
        if (reinterpret_cast<uintptr_t>(a->n) % 4) return FASN_EALIGN;
        if (a->n_stride_b < 0 || a->n_stride_h < 0 || (a->B - 1) * a->n_stride_b + (a->H - 1) * a->n_stride_h >= (1ll << 31)) return FASN_EINVAL;
    }
    p = KvParams{};
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
    p.B = a->B, p.H = a->H, p.G = G, p.Hkv = a->H / G, p.Sq = a->Sq, p.R = G * a->Sq;
    p.causal = a->causal ? 1 : 0;
    p.c = a->scale * kLog2e;
    p.n = a->softmax_n;
    p.nt = a->n;
    p.nsb = (int)a->n_stride_b, p.nsh = (int)a->n_stride_h;
    const int64_t base = (int64_t)p.B * p.Hkv;
    const int64_t cap_tiles = (capacity + KV_KT - 1) / KV_KT;
    p.nsplit = (int)kv_nsplit(a->D, base, cap_tiles, kv_min_tps(p.R));
    if (base * p.nsplit > INT_MAX) return FASN_EINVAL;
    return FASN_OK;
}
size_t kv_ws_bytes(const KvParams& p, int D) { return (size_t)p.B * p.Hkv * p.nsplit * p.R * (size_t)(D + 2) * sizeof(float); }

// The ALiBi operand of the *_alibi entry points (checked after the base arguments, before any HIP call): the rules of `n`
int kv_build_alibi(const fasn_kvcache_args* a, const fasn_alibi_slopes* s, KvAlibi& al) {
    if (s == nullptr || s->slopes == nullptr) return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(s->slopes) % 4) return FASN_EALIGN;
    if (s->stride_b < 0 || s->stride_h < 0 || (a->B - 1) * s->stride_b + (a->H - 1) * s->stride_h >= (1ll << 31)) return FASN_EINVAL;
    al = KvAlibi{s->slopes, (int)s->stride_b, (int)s->stride_h};
    return FASN_OK;
}

// The window operand of the *_window entry points (checked after the base arguments, before any HIP call), and the plan under it: the
// base rule over the tiles a workgroup's window can touch, never more splits than the base plan has.
int kv_build_window(const fasn_kvcache_args* a, const fasn_kv_window* w, KvParams& p, KvWindow& kw) {
    if (w == nullptr || w->window < 1 || w->reserved != 0) return FASN_EINVAL;
    if (!a->causal) return FASN_EUNSUPPORTED;
    kw = KvWindow{w->window < p.capacity ? w->window : p.capacity};
    const int64_t cap_tiles = ((int64_t)p.capacity + KV_KT - 1) / KV_KT;
    p.nsplit = (int)kv_nsplit(a->D, (int64_t)p.B * p.Hkv, kv_window_tiles(cap_tiles, w->window, p.Sq), kv_min_tps(p.R));
    return FASN_OK;
}

// (al == kw == nullptr: the base kernel; otherwise its ALiBi sibling on the same grid, LDS and workspace, or its window sibling)
template <typename Tag, int D>
int kv_launch_fwd(const KvParams& p, const KvAlibi* al, const KvWindow* kw, hipStream_t s) {
    constexpr int smem = kv_smem(D);
    if (kw != nullptr) {
        constexpr auto kern = &fasn_kvcache_fwd_window_kernel<Tag, D>;
        ensure_smem<kern>(smem);
        FASN_LAUNCH(kern, dim3((unsigned)(p.B * p.Hkv * p.nsplit)), dim3(256), smem, s, p, *kw);
    } else if (al == nullptr) {
        constexpr auto kern = &fasn_kvcache_fwd_kernel<Tag, D>;
        ensure_smem<kern>(smem);
        FASN_LAUNCH(kern, dim3((unsigned)(p.B * p.Hkv * p.nsplit)), dim3(256), smem, s, p);
    } else {
        constexpr auto kern = &fasn_kvcache_fwd_alibi_kernel<Tag, D>;
        ensure_smem<kern>(smem);
        FASN_LAUNCH(kern, dim3((unsigned)(p.B * p.Hkv * p.nsplit)), dim3(256), smem, s, p, *al);
    }
    const int64_t nthr = (int64_t)p.B * p.Hkv * p.R * (D / 4);
    FASN_LAUNCH((fasn_kvcache_combine_kernel<Tag, D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, p);
    return launch_rc();
}
template <int D>
int kv_launch_append(const KvParams& p, hipStream_t s) {
    const int64_t nthr = (int64_t)p.B * p.Hkv * p.Sq * (D / 8);
    FASN_LAUNCH((fasn_kvcache_append_kernel<D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, p);
    return launch_rc();
}

template <typename Tag>
int kv_launch_fwd_d(int D, const KvParams& p, const KvAlibi* al, const KvWindow* kw, hipStream_t s) {   // (kv_build let only these four through)
    switch (D) {
        case 32: return kv_launch_fwd<Tag, 32>(p, al, kw, s);
        case 64: return kv_launch_fwd<Tag, 64>(p, al, kw, s);
        case 128: return kv_launch_fwd<Tag, 128>(p, al, kw, s);
        default: return kv_launch_fwd<Tag, 256>(p, al, kw, s);
    }
}

int kv_forward(const fasn_kvcache_args* args, KvVariant variant, const void* operand, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    KvParams p;
    int rc = kv_build(args, p);
    if (rc) return rc;
    KvAlibi al{};
    KvWindow kw{};
    if (variant == KV_ALIBI && (rc = kv_build_alibi(args, static_cast<const fasn_alibi_slopes*>(operand), al))) return rc;
    if (variant == KV_WINDOW && (rc = kv_build_window(args, static_cast<const fasn_kv_window*>(operand), p, kw))) return rc;
    if (workspace == nullptr || workspace_bytes < kv_ws_bytes(p, args->D)) return FASN_EWORKSPACE;
    if (!kv_aligned16(workspace)) return FASN_EALIGN;
    p.part_o = static_cast<float*>(workspace);
    p.part_ml = p.part_o + (size_t)p.B * p.Hkv * p.nsplit * p.R * args->D;
    hipStream_t s = (hipStream_t)stream;
    const KvAlibi* const alp = variant == KV_ALIBI ? &al : nullptr;
    const KvWindow* const kwp = variant == KV_WINDOW ? &kw : nullptr;
    if (args->dtype == FASN_DTYPE_BF16) return kv_launch_fwd_d<bf16_tag>(args->D, p, alp, kwp, s);
    return kv_launch_fwd_d<f16_tag>(args->D, p, alp, kwp, s);
}

int kv_plan(const fasn_kvcache_args* args, KvVariant variant, const void* operand, char* buf, size_t cap) {
    if (args == nullptr || buf == nullptr || cap == 0) return FASN_EINVAL;
    LaunchLog log{buf, cap, 0};
    buf[0] = 0;
    LaunchLog* const outer = t_launch_log;
    t_launch_log = &log;
    const int rc = kv_forward(args, variant, operand, reinterpret_cast<void*>(uintptr_t(256)), ~size_t(0), nullptr);   // (nothing is launched: any aligned address stands for the workspace)
    t_launch_log = outer;
    if (rc) return rc;
    return log.len > cap ? FASN_EINVAL : (int)log.len;
}

}  // namespace

// the validation and parameter packing above, for the rotary rotate-and-append call (fasn_kvrope.h declares it, fasn_kvrope.hip calls it)
int kv_build_params(const fasn_kvcache_args* a, KvParams& p) { return kv_build(a, p); }

}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_fwd_kvcache_workspace_bytes(const fasn_kvcache_args* args) {
    KvParams p;
    if (kv_build(args, p) != FASN_OK) return 0;
    return kv_ws_bytes(p, args->D);
}

int fasn_fwd_kvcache(const fasn_kvcache_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(args, KV_BASE, nullptr, workspace, workspace_bytes, stream);
}

int fasn_fwd_kvcache_alibi(const fasn_kvcache_args* args, const fasn_alibi_slopes* alibi, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(args, KV_ALIBI, alibi, workspace, workspace_bytes, stream);
}

size_t fasn_fwd_kvcache_window_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_window* window) {
    KvParams p;
    KvWindow kw;
    if (kv_build(args, p) != FASN_OK || kv_build_window(args, window, p, kw) != FASN_OK) return 0;
    return kv_ws_bytes(p, args->D);
}

int fasn_fwd_kvcache_window(const fasn_kvcache_args* args, const fasn_kv_window* window, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(args, KV_WINDOW, window, workspace, workspace_bytes, stream);
}

int fasn_kvcache_append(const fasn_kvcache_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    KvParams p;
    int rc = kv_build(args, p);
    if (rc) return rc;
    if (k_new == nullptr || v_new == nullptr) return FASN_EINVAL;
    if ((rc = kv_check_view(*k_new))) return rc;
    if ((rc = kv_check_view(*v_new))) return rc;
    p.kn = static_cast<const char*>(k_new->ptr);
    p.vn = static_cast<const char*>(v_new->ptr);
    for (int i = 0; i < 3; ++i) {
        p.kns[i] = k_new->stride[i];
        p.vns[i] = v_new->stride[i];
    }
    hipStream_t s = (hipStream_t)stream;
    switch (args->D) {
        case 32: return kv_launch_append<32>(p, s);
        case 64: return kv_launch_append<64>(p, s);
        case 128: return kv_launch_append<128>(p, s);
        default: return kv_launch_append<256>(p, s);
    }
}

int fasn_kvcache_plan(const fasn_kvcache_args* args, char* buf, size_t cap) { return kv_plan(args, KV_BASE, nullptr, buf, cap); }

int fasn_kvcache_alibi_plan(const fasn_kvcache_args* args, const fasn_alibi_slopes* alibi, char* buf, size_t cap) {
    return kv_plan(args, KV_ALIBI, alibi, buf, cap);
}

int fasn_kvcache_window_plan(const fasn_kvcache_args* args, const fasn_kv_window* window, char* buf, size_t cap) {
    return kv_plan(args, KV_WINDOW, window, buf, cap);
}

}  // extern "C"
