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

// what the checks leave to the launches: the parameters, and the operand (MLA_FP8, MLA_SPARSE) as the kernels take it
struct MlaRun { MlaParams p; MlaFp8 f8; MlaSparse sp; };

// A variant of the decode, stated once: what its cache holds, which operand stands behind the block, and its launches by dtype (f16,
// bf16). An index list is the forward's operand alone, so the variants behind one have no append: their rows' own serves them (kMla's
// for the 16-bit rows, kMlaRows8's for the 656-byte rows, which in turn have no forward without a list).
enum MlaOperand { MLA_NONE, MLA_FP8, MLA_SPARSE };
using MlaLaunch = void (*)(const MlaRun&, hipStream_t);
struct MlaVariant {
    int eb;     // bytes of a cache element: enters the 32-bit range of a tile and the 16-byte rule of the cache strides
    int rowe;   // elements of a cache row, the least row stride
    MlaOperand takes;
    MlaLaunch forward[2], append[2];
};

// One call: the variant, the block, and the operand its entry point got - a NULL one is refused by the operand's rule, never read as "none".
struct MlaCall {
    const MlaVariant& v;
    const fasn_mla_args* a;
    const fasn_mla_fp8* f = nullptr;
    const fasn_mla_sparse* x = nullptr;
    MlaCall(const MlaVariant& v, const fasn_mla_args* a) : v(v), a(a) {}
    MlaCall(const MlaVariant& v, const fasn_mla_args* a, const fasn_mla_fp8* f) : v(v), a(a), f(f) {}
    MlaCall(const MlaVariant& v, const fasn_mla_args* a, const fasn_mla_sparse* x) : v(v), a(a), x(x) {}
};

// the FP8 operand: NULL, a NULL scale, reserved, a stride that is negative or leaves the 32-bit range (FASN_EINVAL); a scale pointer off
// 4 bytes (FASN_EALIGN)
int mla_check_fp8(const fasn_mla_args* a, const fasn_mla_fp8* f, MlaFp8& f8) {
    if (f == nullptr || f->kv_scale == nullptr || f->reserved != 0 || f->sb < 0 || f->sb >= (1ll << 31) || (a->B - 1) * f->sb >= (1ll << 31))
        return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(f->kv_scale) % 4) return FASN_EALIGN;
    f8 = MlaFp8{f->kv_scale, f->sb};
    return FASN_OK;
}

// the index list: NULL, a NULL list, reserved, topk <= 0, a stride that is negative or leaves the 32-bit range (FASN_EINVAL); a topk that
// is no multiple of the 64-key tile (FASN_EUNSUPPORTED); a list off 4 bytes (FASN_EALIGN). The plan: one workgroup per (batch element,
// position, 64-head block, split), split s over the index tiles [s * tps, (s + 1) * tps) - the same over either row format.
int mla_check_sparse(const fasn_mla_sparse* x, MlaParams& p, MlaSparse& sp) {
    if (x == nullptr || x->indices == nullptr || x->reserved != 0 || x->topk <= 0 || x->stride_b < 0 || x->stride_q < 0 ||
        x->stride_b >= (1ll << 31) || x->stride_q >= (1ll << 31) || (p.B - 1) * x->stride_b + (p.Sq - 1) * x->stride_q + x->topk >= (1ll << 31))
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

// The one build path: the block's checks, then the variant's operand's. Order of the block's: sizes, enums and NULL members; what this
// build does not serve; the views; the remaining alignment rules.
int mla_build(const MlaCall& c, MlaRun& r) {
    const fasn_mla_args* const a = c.a;
    const int eb = c.v.eb;
    MlaParams& p = r.p;
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
    if (a->kv_stride[0] < 0 || a->kv_stride[1] < c.v.rowe) return FASN_EINVAL;
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
    if (c.v.takes == MLA_FP8) return mla_check_fp8(a, c.f, r.f8);
    if (c.v.takes == MLA_SPARSE) return mla_check_sparse(c.x, p, r.sp);
    return FASN_OK;
}

size_t mla_ws_bytes(const MlaParams& p) { return (size_t)p.B * p.nsplit * p.R * (size_t)(MLA_EV + 2) * sizeof(float); }
size_t mla_workspace_bytes(const MlaCall& c) {
    MlaRun r;
    return mla_build(c, r) == FASN_OK ? mla_ws_bytes(r.p) : 0;
}

int mla_forward(const MlaCall& c, void* workspace, size_t workspace_bytes, hipStream_t s) {
    MlaRun r;
    const int rc = mla_build(c, r);
    if (rc) return rc;
    if (workspace == nullptr || workspace_bytes < mla_ws_bytes(r.p)) return FASN_EWORKSPACE;
    if (!kv_aligned16(workspace)) return FASN_EALIGN;
    r.p.part_o = static_cast<float*>(workspace);
    r.p.part_ml = r.p.part_o + (size_t)r.p.B * r.p.nsplit * r.p.R * MLA_EV;
    const MlaLaunch launch = c.v.forward[c.a->dtype == FASN_DTYPE_BF16];
    if (launch == nullptr) return FASN_EUNSUPPORTED;   // (a record without a forward, kMlaRows8: no entry point hands one in)
    launch(r, s);
    return launch_rc();
}

int mla_plan(const MlaCall& c, char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return mla_forward(c, plan_workspace(), ~size_t(0), nullptr); });
}

// The one append path: the build, the new rows' view, then the variant's launch.
int mla_append(const MlaCall& c, const fasn_view4* kv_new, hipStream_t s) {
    MlaRun r;
    int rc = mla_build(c, r);
    if (rc) return rc;
    if (kv_new == nullptr) return FASN_EINVAL;
    if ((rc = kv_check_view(*kv_new))) return rc;
    r.p.kn = static_cast<const char*>(kv_new->ptr);
    r.p.kns[0] = kv_new->stride[0], r.p.kns[1] = kv_new->stride[1];
    const MlaLaunch launch = c.v.append[c.a->dtype == FASN_DTYPE_BF16];
    if (launch == nullptr) return FASN_EUNSUPPORTED;   // (a record behind an index list: its rows' own record has the append)
    launch(r, s);
    return launch_rc();
}

// ---- the launches: each forward with its combine, each append on its grid
dim3 mla_threads(int64_t nthr) { return dim3((unsigned)((nthr + 255) / 256)); }   // a grid of 256-thread workgroups over nthr threads
dim3 mla_combine_grid(const MlaParams& p) { return mla_threads((int64_t)p.B * p.R * (MLA_EV / 4)); }

template <typename Tag>
void mla_fwd_16(const MlaRun& r, hipStream_t s) {
    kv_launch<&fasn_mla_fwd_kernel<Tag>>((unsigned)(r.p.B * r.p.nrb * r.p.nsplit), MLA_SMEM, s, r.p);
    FASN_LAUNCH((fasn_mla_combine_kernel<Tag>), mla_combine_grid(r.p), dim3(256), 0, s, r.p);
}
template <typename Tag>
void mla_fwd_fp8(const MlaRun& r, hipStream_t s) {
    kv_launch<&fasn_mla_fwd_fp8_kernel<Tag>>((unsigned)(r.p.B * r.p.nrb * r.p.nsplit), MLA8_SMEM, s, r.p, r.f8);
    FASN_LAUNCH((fasn_mla_fp8_combine_kernel<Tag>), mla_combine_grid(r.p), dim3(256), 0, s, r.p, r.f8);
}
template <typename Tag>
void mla_fwd_sparse(const MlaRun& r, hipStream_t s) {
    kv_launch<&fasn_mla_sparse_fwd_kernel<Tag>>((unsigned)(r.p.B * r.p.Sq * r.sp.nhb * r.p.nsplit), MLA_SMEM, s, r.p, r.sp);
    FASN_LAUNCH((fasn_mla_combine_kernel<Tag>), mla_combine_grid(r.p), dim3(256), 0, s, r.p);
}
template <typename Tag>
void mla_fwd_sparse_fp8(const MlaRun& r, hipStream_t s) {
    kv_launch<&fasn_mla_sparse_fp8_fwd_kernel<Tag>>((unsigned)(r.p.B * r.p.Sq * r.sp.nhb * r.p.nsplit), MLA8S_SMEM, s, r.p, r.sp);
    FASN_LAUNCH((fasn_mla_combine_kernel<Tag>), mla_combine_grid(r.p), dim3(256), 0, s, r.p);
}
void mla_append_16(const MlaRun& r, hipStream_t s) {   // (a copy: either dtype; at most 256 rows per batch element: the grid fits)
    FASN_LAUNCH(fasn_mla_append_kernel, mla_threads((int64_t)r.p.B * r.p.Sq * MLA_CPR), dim3(256), 0, s, r.p);
}
template <typename Tag>
void mla_append_fp8(const MlaRun& r, hipStream_t s) {
    FASN_LAUNCH((fasn_mla_fp8_append_kernel<Tag>), mla_threads((int64_t)r.p.B * r.p.Sq * (MLA_E / 16)), dim3(256), 0, s, r.p, r.f8);
}
template <typename Tag>
void mla_append_rows8(const MlaRun& r, hipStream_t s) {   // one wave per row
    FASN_LAUNCH((fasn_mla_sparse_fp8_append_kernel<Tag>), dim3((unsigned)(((int64_t)r.p.B * r.p.Sq + 3) / 4)), dim3(256), 0, s, r.p);
}

constexpr MlaVariant kMla = {2, MLA_E, MLA_NONE, {mla_fwd_16<f16_tag>, mla_fwd_16<bf16_tag>}, {mla_append_16, mla_append_16}};
constexpr MlaVariant kMlaFp8 = {1, MLA_E, MLA_FP8, {mla_fwd_fp8<f16_tag>, mla_fwd_fp8<bf16_tag>}, {mla_append_fp8<f16_tag>, mla_append_fp8<bf16_tag>}};
constexpr MlaVariant kMlaSparse = {2, MLA_E, MLA_SPARSE, {mla_fwd_sparse<f16_tag>, mla_fwd_sparse<bf16_tag>}, {}};
constexpr MlaVariant kMlaRows8 = {1, MLA8S_ROWB, MLA_NONE, {}, {mla_append_rows8<f16_tag>, mla_append_rows8<bf16_tag>}};
constexpr MlaVariant kMlaSparseFp8 = {1, MLA8S_ROWB, MLA_SPARSE, {mla_fwd_sparse_fp8<f16_tag>, mla_fwd_sparse_fp8<bf16_tag>}, {}};

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_mla_workspace_bytes(const fasn_mla_args* args) { return mla_workspace_bytes({kMla, args}); }
int fasn_fwd_mla(const fasn_mla_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream) { return mla_forward({kMla, args}, workspace, workspace_bytes, (hipStream_t)stream); }
int fasn_mla_append(const fasn_mla_args* args, const fasn_view4* kv_new, fasn_stream_t stream) { return mla_append({kMla, args}, kv_new, (hipStream_t)stream); }
int fasn_mla_plan(const fasn_mla_args* args, char* buf, size_t cap) { return mla_plan({kMla, args}, buf, cap); }

size_t fasn_mla_fp8_workspace_bytes(const fasn_mla_args* args, const fasn_mla_fp8* fp8) { return mla_workspace_bytes({kMlaFp8, args, fp8}); }
int fasn_fwd_mla_fp8(const fasn_mla_args* args, const fasn_mla_fp8* fp8, void* workspace, size_t workspace_bytes, fasn_stream_t stream) { return mla_forward({kMlaFp8, args, fp8}, workspace, workspace_bytes, (hipStream_t)stream); }
int fasn_mla_fp8_append(const fasn_mla_args* args, const fasn_mla_fp8* fp8, const fasn_view4* kv_new, fasn_stream_t stream) { return mla_append({kMlaFp8, args, fp8}, kv_new, (hipStream_t)stream); }
int fasn_mla_fp8_plan(const fasn_mla_args* args, const fasn_mla_fp8* fp8, char* buf, size_t cap) { return mla_plan({kMlaFp8, args, fp8}, buf, cap); }

size_t fasn_mla_sparse_workspace_bytes(const fasn_mla_args* args, const fasn_mla_sparse* sparse) { return mla_workspace_bytes({kMlaSparse, args, sparse}); }
int fasn_fwd_mla_sparse(const fasn_mla_args* args, const fasn_mla_sparse* sparse, void* workspace, size_t workspace_bytes, fasn_stream_t stream) { return mla_forward({kMlaSparse, args, sparse}, workspace, workspace_bytes, (hipStream_t)stream); }
int fasn_mla_sparse_plan(const fasn_mla_args* args, const fasn_mla_sparse* sparse, char* buf, size_t cap) { return mla_plan({kMlaSparse, args, sparse}, buf, cap); }

size_t fasn_mla_sparse_fp8_workspace_bytes(const fasn_mla_args* args, const fasn_mla_sparse* sparse) { return mla_workspace_bytes({kMlaSparseFp8, args, sparse}); }
int fasn_fwd_mla_sparse_fp8(const fasn_mla_args* args, const fasn_mla_sparse* sparse, void* workspace, size_t workspace_bytes, fasn_stream_t stream) { return mla_forward({kMlaSparseFp8, args, sparse}, workspace, workspace_bytes, (hipStream_t)stream); }
int fasn_mla_sparse_fp8_append(const fasn_mla_args* args, const fasn_view4* kv_new, fasn_stream_t stream) { return mla_append({kMlaRows8, args}, kv_new, (hipStream_t)stream); }
int fasn_mla_sparse_fp8_plan(const fasn_mla_args* args, const fasn_mla_sparse* sparse, char* buf, size_t cap) { return mla_plan({kMlaSparseFp8, args, sparse}, buf, cap); }

}  // extern "C"
