// MLA decode over a compressed latent K/V cache (include/fasn.h: fasn_fwd_mla, fasn_mla_append, fasn_mla_workspace_bytes, fasn_mla_plan):
// the argument checks - all of them in front of any HIP call -, the launch plan, which depends on shapes and capacity only, and the
// launches of fasn_mla.h. The call sits beside the K/V-cache family and is no operand set of it: a block of its own, kernels of its own.
// The same block over a latent cache of e4m3fn codes (fasn_fwd_mla_fp8, fasn_mla_fp8_append, fasn_mla_fp8_workspace_bytes, fasn_mla_fp8_plan;
// kernels in fasn_mla_fp8.h) goes through the same checks with the cache's element size at 1 and the operand's checks behind them.
// The sparse decode over 656-byte FP8 rows (fasn_fwd_mla_sparse_fp8, fasn_mla_sparse_fp8_append, fasn_mla_sparse_fp8_workspace_bytes,
// fasn_mla_sparse_fp8_plan; kernels in fasn_mla_sparse_fp8.h) is the sparse block with the element size at 1 and the row's bytes at 656.
#include <limits.h>
#include <math.h>
#include "fasn_kv_host.h"
#include "fasn_mla.h"
#include "fasn_mla_fp8.h"
#include "fasn_mla_sparse.h"
#include "fasn_mla_sparse_fp8.h"

namespace fasn {
namespace {

// Check order: sizes, enums and NULL members; what this build does not serve; the views; the remaining alignment rules. `eb`: bytes of a
// cache element (2; 1 for the cache of codes), which enters the 32-bit range of a tile and the 16-byte rule of the cache strides; `rowe`:
// elements of a cache row (576; 656 bytes for the FP8 rows behind an index list), the least row stride.
int mla_build(const fasn_mla_args* a, MlaParams& p, int eb = 2, int rowe = MLA_E) {
    if (a == nullptr) return FASN_EINVAL;
    if (a->B <= 0 || a->H <= 0 || a->Sq <= 0 || a->D <= 0 || a->Dv <= 0 || a->page_size <= 0 || a->reserved != 0) return FASN_EINVAL;
    if (a->dtype != FASN_DTYPE_F16 && a->dtype != FASN_DTYPE_BF16) return FASN_EDTYPE;
    if (a->D != MLA_E || a->Dv != MLA_EV) return FASN_EHEADDIM;
    if (!(a->softmax_n >= 0.f) || !isfinite(a->scale)) return FASN_EINVAL;
    if (a->seqlens == nullptr || a->kv_cache == nullptr) return FASN_EINVAL;
    const bool paged = a->block_table != nullptr;
    if (paged && (a->max_pages <= 0 || a->block_table_stride < a->max_pages)) return FASN_EINVAL;
    const int64_t capacity = paged ? (int64_t)a->max_pages * a->page_size : (int64_t)a->page_size;
    if (capacity > INT_MAX - 2 * KV_KT || (int64_t)a->seqlen_add + capacity > INT_MAX || a->seqlen_add < 0) return FASN_EINVAL;
    if (a->kv_stride[0] < 0 || a->kv_stride[1] < rowe) return FASN_EINVAL;
    if (a->n != nullptr && (a->n_stride_b < 0 || a->n_stride_h < 0 || (a->B - 1) * a->n_stride_b + (a->H - 1) * a->n_stride_h >= (1ll << 31))) return FASN_EINVAL;
    // served: H * Sq <= 256 rows, pages of whole 64-key tiles, a tile whose descriptor range and lane offsets are 32-bit, and - the queries are
    // prescaled by scale * log2(e) in the element type - |scale * log2(e)| <= 8 in fp16
    if ((int64_t)a->H * a->Sq > MLA_MAX_ROWS) return FASN_EUNSUPPORTED;
    if (paged && a->page_size % KV_KT != 0) return FASN_EUNSUPPORTED;
    if ((int64_t)KV_KT * a->kv_stride[1] * eb >= (1ll << 31)) return FASN_EUNSUPPORTED;
    if (a->dtype == FASN_DTYPE_F16 && !(fabsf(a->scale * kLog2e) <= 8.0f)) return FASN_EUNSUPPORTED;
    int rc;
    if ((rc = kv_check_view(a->q))) return rc;
    if ((rc = kv_check_view(a->o))) return rc;
    if (!kv_aligned16(a->kv_cache) || a->kv_stride[0] % (16 / eb) != 0 || a->kv_stride[1] % (16 / eb) != 0) return FASN_EALIGN;
    if (reinterpret_cast<uintptr_t>(a->seqlens) % 4 || reinterpret_cast<uintptr_t>(a->block_table) % 4 || reinterpret_cast<uintptr_t>(a->n) % 4) return FASN_EALIGN;
    p = MlaParams{};
    p.q = static_cast<const char*>(a->q.ptr);
    p.o = static_cast<char*>(a->o.ptr);
    p.lse = a->lse;
    p.kv = static_cast<char*>(a->kv_cache);
    for (int i = 0; i < 3; ++i) {
        p.qs[i] = a->q.stride[i];
        p.os[i] = a->o.stride[i];
    }
    p.kps = a->kv_stride[0], p.krs = a->kv_stride[1];
    p.bt = a->block_table;
    p.bts = a->block_table_stride;
    p.seqlens = a->seqlens;
    p.seqlen_add = a->seqlen_add;
    p.page_size = a->page_size;
    p.tpp = paged ? a->page_size / KV_KT : INT_MAX;
    p.capacity = (int)capacity;
    p.B = a->B, p.H = a->H, p.Sq = a->Sq;
    p.R = a->H * a->Sq;
    p.nrb = (p.R + MLA_RB - 1) / MLA_RB;
    p.causal = a->causal ? 1 : 0;
    p.c = a->scale * kLog2e;
    p.n = a->softmax_n;
    p.nt = a->n;
    p.nsb = (int)a->n_stride_b, p.nsh = (int)a->n_stride_h;
    // the plan: one workgroup per (batch element, 64-row block, split)
    const int64_t base = (int64_t)p.B * p.nrb;
    p.nsplit = (int)mla_nsplit(base, (capacity + KV_KT - 1) / KV_KT, p.R);
    if (base * p.nsplit > INT_MAX / MLA_MAX_ROWS) return FASN_EINVAL;
    return FASN_OK;
}

size_t mla_ws_bytes(const MlaParams& p) { return (size_t)p.B * p.nsplit * p.R * (size_t)(MLA_EV + 2) * sizeof(float); }

// the FP8 operand behind the block's checks: NULL, a NULL scale, reserved, a stride that is negative or leaves the 32-bit range
// (FASN_EINVAL); a scale pointer off 4 bytes (FASN_EALIGN)
int mla_build_fp8(const fasn_mla_args* a, const fasn_mla_fp8* f, MlaParams& p, MlaFp8& f8) {
    const int rc = mla_build(a, p, 1);
    if (rc) return rc;
    if (f == nullptr || f->kv_scale == nullptr || f->reserved != 0 || f->sb < 0 || f->sb >= (1ll << 31) || (a->B - 1) * f->sb >= (1ll << 31))
        return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(f->kv_scale) % 4) return FASN_EALIGN;
    f8 = MlaFp8{f->kv_scale, f->sb};
    return FASN_OK;
}

// the index list behind the block's checks: NULL, a NULL list, reserved, topk <= 0, a stride that is negative or leaves the 32-bit range
// (FASN_EINVAL); a topk that is no multiple of the 64-key tile (FASN_EUNSUPPORTED); a list off 4 bytes (FASN_EALIGN). The plan: one
// workgroup per (batch element, position, 64-head block, split), split s over the index tiles [s * tps, (s + 1) * tps). rows8: the cache
// holds 656-byte FP8 rows - the same checks on bytes, the same plan.
int mla_build_sparse(const fasn_mla_args* a, const fasn_mla_sparse* x, MlaParams& p, MlaSparse& sp, bool rows8 = false) {
    const int rc = rows8 ? mla_build(a, p, 1, MLA8S_ROWB) : mla_build(a, p);
    if (rc) return rc;
    if (x == nullptr || x->indices == nullptr || x->reserved != 0 || x->topk <= 0 || x->stride_b < 0 || x->stride_q < 0 ||
        x->stride_b >= (1ll << 31) || x->stride_q >= (1ll << 31) || (a->B - 1) * x->stride_b + (a->Sq - 1) * x->stride_q + x->topk >= (1ll << 31))
        return FASN_EINVAL;
    if (x->topk % KV_KT != 0) return FASN_EUNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(x->indices) % 4) return FASN_EALIGN;
    sp = MlaSparse{};
    sp.idx = x->indices;
    sp.sb = x->stride_b, sp.sq = x->stride_q;
    sp.ntiles = x->topk / KV_KT;
    sp.nhb = (p.H + MLA_RB - 1) / MLA_RB;
    sp.ps_magic = (uint32_t)((1ull << 32) / (uint64_t)p.page_size);   // (a paged cache has page_size >= 64; a dense one does not divide)
    const int64_t base = (int64_t)p.B * p.Sq * sp.nhb;
    p.nsplit = (int)mla_nsplit(base, sp.ntiles, p.H < MLA_RB ? p.H : MLA_RB);
    sp.tps = (sp.ntiles + p.nsplit - 1) / p.nsplit;
    if (base * p.nsplit > INT_MAX / MLA_MAX_ROWS) return FASN_EINVAL;
    return FASN_OK;
}

// f8 == nullptr: the 16-bit cache; sp != nullptr: behind an index list, rows8: over 656-byte FP8 rows
template <typename Tag>
int mla_launch_as(const MlaParams& p, const MlaFp8* f8, const MlaSparse* sp, hipStream_t s, bool rows8 = false) {
    const int64_t nthr = (int64_t)p.B * p.R * (MLA_EV / 4);
    if (sp != nullptr) {
        const unsigned grid = (unsigned)(p.B * p.Sq * sp->nhb * p.nsplit);
        if (rows8) kv_launch<&fasn_mla_sparse_fp8_fwd_kernel<Tag>>(grid, MLA8S_SMEM, s, p, *sp);
        else kv_launch<&fasn_mla_sparse_fwd_kernel<Tag>>(grid, MLA_SMEM, s, p, *sp);
        FASN_LAUNCH((fasn_mla_combine_kernel<Tag>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, p);
        return launch_rc();
    }
    if (f8 != nullptr) {
        kv_launch<&fasn_mla_fwd_fp8_kernel<Tag>>((unsigned)(p.B * p.nrb * p.nsplit), MLA8_SMEM, s, p, *f8);
        FASN_LAUNCH((fasn_mla_fp8_combine_kernel<Tag>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, p, *f8);
        return launch_rc();
    }
    kv_launch<&fasn_mla_fwd_kernel<Tag>>((unsigned)(p.B * p.nrb * p.nsplit), MLA_SMEM, s, p);
    FASN_LAUNCH((fasn_mla_combine_kernel<Tag>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, p);
    return launch_rc();
}

// f == nullptr with fp8 == false: fasn_fwd_mla; fp8: fasn_fwd_mla_fp8, whose operand may be NULL only to be refused; sparse: fasn_fwd_mla_sparse,
// likewise with x; sparse and fp8: fasn_fwd_mla_sparse_fp8 (the rows carry their scales: f is not looked at)
int mla_forward(const fasn_mla_args* a, bool fp8, const fasn_mla_fp8* f, void* workspace, size_t workspace_bytes, hipStream_t s,
                bool sparse = false, const fasn_mla_sparse* x = nullptr) {
    MlaParams p;
    MlaFp8 f8;
    MlaSparse sp;
    const bool rows8 = sparse && fp8;
    const int rc = sparse ? mla_build_sparse(a, x, p, sp, rows8) : fp8 ? mla_build_fp8(a, f, p, f8) : mla_build(a, p);
    if (rc) return rc;
    if (workspace == nullptr || workspace_bytes < mla_ws_bytes(p)) return FASN_EWORKSPACE;
    if (!kv_aligned16(workspace)) return FASN_EALIGN;
    p.part_o = static_cast<float*>(workspace);
    p.part_ml = p.part_o + (size_t)p.B * p.nsplit * p.R * MLA_EV;
    const MlaFp8* const f8p = fp8 && !sparse ? &f8 : nullptr;
    const MlaSparse* const spp = sparse ? &sp : nullptr;
    return a->dtype == FASN_DTYPE_BF16 ? mla_launch_as<bf16_tag>(p, f8p, spp, s, rows8) : mla_launch_as<f16_tag>(p, f8p, spp, s, rows8);
}

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_mla_workspace_bytes(const fasn_mla_args* args) {
    MlaParams p;
    return mla_build(args, p) == FASN_OK ? mla_ws_bytes(p) : 0;
}

int fasn_fwd_mla(const fasn_mla_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return mla_forward(args, false, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

int fasn_mla_append(const fasn_mla_args* args, const fasn_view4* kv_new, fasn_stream_t stream) {
    MlaParams p;
    int rc = mla_build(args, p);
    if (rc) return rc;
    if (kv_new == nullptr) return FASN_EINVAL;
    if ((rc = kv_check_view(*kv_new))) return rc;
    p.kn = static_cast<const char*>(kv_new->ptr);
    p.kns[0] = kv_new->stride[0], p.kns[1] = kv_new->stride[1];
    const int64_t nthr = (int64_t)p.B * p.Sq * MLA_CPR;   // (at most 256 rows per batch element: the grid fits)
    FASN_LAUNCH(fasn_mla_append_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return launch_rc();
}

int fasn_mla_plan(const fasn_mla_args* args, char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return mla_forward(args, false, nullptr, plan_workspace(), ~size_t(0), nullptr); });
}

size_t fasn_mla_fp8_workspace_bytes(const fasn_mla_args* args, const fasn_mla_fp8* fp8) {
    MlaParams p;
    MlaFp8 f8;
    return mla_build_fp8(args, fp8, p, f8) == FASN_OK ? mla_ws_bytes(p) : 0;
}

int fasn_fwd_mla_fp8(const fasn_mla_args* args, const fasn_mla_fp8* fp8, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return mla_forward(args, true, fp8, workspace, workspace_bytes, (hipStream_t)stream);
}

int fasn_mla_fp8_append(const fasn_mla_args* args, const fasn_mla_fp8* fp8, const fasn_view4* kv_new, fasn_stream_t stream) {
    MlaParams p;
    MlaFp8 f8;
    int rc = mla_build_fp8(args, fp8, p, f8);
    if (rc) return rc;
    if (kv_new == nullptr) return FASN_EINVAL;
    if ((rc = kv_check_view(*kv_new))) return rc;
    p.kn = static_cast<const char*>(kv_new->ptr);
    p.kns[0] = kv_new->stride[0], p.kns[1] = kv_new->stride[1];
    const int64_t nthr = (int64_t)p.B * p.Sq * (MLA_E / 16);
    const dim3 grid((unsigned)((nthr + 255) / 256));
    if (args->dtype == FASN_DTYPE_BF16) FASN_LAUNCH((fasn_mla_fp8_append_kernel<bf16_tag>), grid, dim3(256), 0, (hipStream_t)stream, p, f8);
    else FASN_LAUNCH((fasn_mla_fp8_append_kernel<f16_tag>), grid, dim3(256), 0, (hipStream_t)stream, p, f8);
    return launch_rc();
}

int fasn_mla_fp8_plan(const fasn_mla_args* args, const fasn_mla_fp8* fp8, char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return mla_forward(args, true, fp8, plan_workspace(), ~size_t(0), nullptr); });
}

size_t fasn_mla_sparse_workspace_bytes(const fasn_mla_args* args, const fasn_mla_sparse* sparse) {
    MlaParams p;
    MlaSparse sp;
    return mla_build_sparse(args, sparse, p, sp) == FASN_OK ? mla_ws_bytes(p) : 0;
}

int fasn_fwd_mla_sparse(const fasn_mla_args* args, const fasn_mla_sparse* sparse, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return mla_forward(args, false, nullptr, workspace, workspace_bytes, (hipStream_t)stream, true, sparse);
}

int fasn_mla_sparse_plan(const fasn_mla_args* args, const fasn_mla_sparse* sparse, char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return mla_forward(args, false, nullptr, plan_workspace(), ~size_t(0), nullptr, true, sparse); });
}

size_t fasn_mla_sparse_fp8_workspace_bytes(const fasn_mla_args* args, const fasn_mla_sparse* sparse) {
    MlaParams p;
    MlaSparse sp;
    return mla_build_sparse(args, sparse, p, sp, true) == FASN_OK ? mla_ws_bytes(p) : 0;
}

int fasn_fwd_mla_sparse_fp8(const fasn_mla_args* args, const fasn_mla_sparse* sparse, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return mla_forward(args, true, nullptr, workspace, workspace_bytes, (hipStream_t)stream, true, sparse);
}

int fasn_mla_sparse_fp8_append(const fasn_mla_args* args, const fasn_view4* kv_new, fasn_stream_t stream) {
    MlaParams p;
    int rc = mla_build(args, p, 1, MLA8S_ROWB);
    if (rc) return rc;
    if (kv_new == nullptr) return FASN_EINVAL;
    if ((rc = kv_check_view(*kv_new))) return rc;
    p.kn = static_cast<const char*>(kv_new->ptr);
    p.kns[0] = kv_new->stride[0], p.kns[1] = kv_new->stride[1];
    const dim3 grid((unsigned)(((int64_t)p.B * p.Sq + 3) / 4));   // one wave per row
    if (args->dtype == FASN_DTYPE_BF16) FASN_LAUNCH((fasn_mla_sparse_fp8_append_kernel<bf16_tag>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else FASN_LAUNCH((fasn_mla_sparse_fp8_append_kernel<f16_tag>), grid, dim3(256), 0, (hipStream_t)stream, p);
    return launch_rc();
}

int fasn_mla_sparse_fp8_plan(const fasn_mla_args* args, const fasn_mla_sparse* sparse, char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return mla_forward(args, true, nullptr, plan_workspace(), ~size_t(0), nullptr, true, sparse); });
}

}  // extern "C"
