// The lightning indexer in front of the sparse MLA decode (include/fasn.h: fasn_mla_index, fasn_mla_index_append,
// fasn_mla_index_workspace_bytes, fasn_mla_index_plan): the argument checks - all of them in front of any HIP call -, the launch plan, which
// depends on shapes and capacity only, and the launches of fasn_mla_index.h. A block of its own beside the MLA decode's (fasn_mla.hip).
#include <limits.h>
#include "fasn_kv_host.h"
#include "fasn_mla_index.h"

namespace fasn {
namespace {

// The logits kernel's plan: runs of `tpw` 64-key tiles, tpw even (a workgroup steps through 128-key units), as many as bring the grid to
// ~2048 workgroups - eight per CU, of which two are resident - and never fewer than one unit per workgroup.
constexpr int64_t kIndexTargetWgs = 2048;

// Check order: sizes, enums and NULL members; what this build does not serve; the view; the remaining alignment rules.
int index_build(const fasn_mla_index_args* a, MlaIndexParams& p) {
    if (a == nullptr) return FASN_EINVAL;
    if (a->B <= 0 || a->Hi <= 0 || a->Sq <= 0 || a->D <= 0 || a->page_size <= 0 || a->topk <= 0 || a->reserved != 0) return FASN_EINVAL;
    if (a->dtype != FASN_DTYPE_F16 && a->dtype != FASN_DTYPE_BF16) return FASN_EDTYPE;
    if (a->D != MLI_D) return FASN_EHEADDIM;
    if (a->seqlens == nullptr || a->k_cache == nullptr || a->w == nullptr || a->indices == nullptr) return FASN_EINVAL;
    const bool paged = a->block_table != nullptr;
    if (paged && (a->max_pages <= 0 || a->block_table_stride < a->max_pages)) return FASN_EINVAL;
    const int64_t capacity = paged ? (int64_t)a->max_pages * a->page_size : (int64_t)a->page_size;
    if (capacity > (1 << 30) || a->seqlen_add < 0) return FASN_EINVAL;   // (key offsets of a run and capacity + seqlen_add stay 32-bit)
    if (a->k_stride[0] < 0 || a->k_stride[1] < MLI_D) return FASN_EINVAL;
    if (a->w_stride[0] < 0 || a->w_stride[1] < 0 || a->w_stride[2] < 0) return FASN_EINVAL;
    if (a->indices_stride[0] < 0 || a->indices_stride[1] < 0 || (a->Sq > 1 && a->indices_stride[1] < a->topk)) return FASN_EINVAL;
    if (a->logits != nullptr && (a->logits_stride[0] < 0 || a->logits_stride[1] < 0 || (a->Sq > 1 && a->logits_stride[1] < capacity))) return FASN_EINVAL;
    // served: 32 or 64 index heads, a list of whole 64-entry tiles, pages of whole 64-key tiles
    if (a->Hi != 32 && a->Hi != 64) return FASN_EUNSUPPORTED;
    if (a->topk % 64 != 0) return FASN_EUNSUPPORTED;
    if (paged && a->page_size % 64 != 0) return FASN_EUNSUPPORTED;
    int rc;
    if ((rc = kv_check_view(a->q))) return rc;
    if (!kv_aligned16(a->k_cache) || a->k_stride[0] % 8 != 0 || a->k_stride[1] % 8 != 0) return FASN_EALIGN;
    if (reinterpret_cast<uintptr_t>(a->seqlens) % 4 || reinterpret_cast<uintptr_t>(a->block_table) % 4 || reinterpret_cast<uintptr_t>(a->w) % 4 ||
        reinterpret_cast<uintptr_t>(a->indices) % 4 || reinterpret_cast<uintptr_t>(a->logits) % 4)
        return FASN_EALIGN;
    p = MlaIndexParams{};
    p.q = static_cast<const char*>(a->q.ptr);
    p.w = a->w;
    for (int i = 0; i < 3; ++i) p.qs[i] = a->q.stride[i], p.ws[i] = a->w_stride[i];
    p.kc = static_cast<char*>(a->k_cache);
    p.kps = a->k_stride[0], p.krs = a->k_stride[1];
    p.bt = a->block_table;
    p.bts = a->block_table_stride;
    p.seqlens = a->seqlens;
    p.seqlen_add = a->seqlen_add;
    p.page_size = a->page_size;
    p.capacity = (int)capacity;
    p.B = a->B, p.Sq = a->Sq;
    p.causal = a->causal ? 1 : 0;
    p.topk = a->topk;
    p.idx = a->indices;
    p.is[0] = a->indices_stride[0], p.is[1] = a->indices_stride[1];
    // the plan
    const int64_t rows = (int64_t)p.B * p.Sq, cap_tiles = (capacity + 63) / 64;
    int64_t tpw = (rows * cap_tiles + kIndexTargetWgs - 1) / kIndexTargetWgs;
    if (tpw > cap_tiles) tpw = cap_tiles;
    tpw = tpw < 2 ? 2 : (tpw + 1) & ~int64_t(1);
    p.tpw = (int)tpw;
    p.nrun = (int)((cap_tiles + tpw - 1) / tpw);
    if (rows * p.nrun > INT_MAX) return FASN_EINVAL;
    // the logits: the caller's buffer, or rows of whole tiles in the workspace
    p.lg = a->logits;
    p.ls[0] = a->logits_stride[0], p.ls[1] = a->logits_stride[1];
    p.lcols = (int)capacity;
    if (a->logits == nullptr) {
        p.lcols = (int)(cap_tiles * 64);
        p.ls[1] = p.lcols, p.ls[0] = (int64_t)p.Sq * p.lcols;
    }
    return FASN_OK;
}

size_t index_ws_bytes(const fasn_mla_index_args* a, const MlaIndexParams& p) {
    return a->logits != nullptr ? 0 : (size_t)p.B * p.Sq * (size_t)p.lcols * sizeof(float);
}

template <typename Tag>
void index_launch_as(const MlaIndexParams& p, int Hi, hipStream_t s) {
    const unsigned grid = (unsigned)(p.B * p.Sq * p.nrun);
    if (Hi == 64) kv_launch<&fasn_mla_index_logits_kernel<Tag, 64>>(grid, 0, s, p);
    else kv_launch<&fasn_mla_index_logits_kernel<Tag, 32>>(grid, 0, s, p);
}

int index_forward(const fasn_mla_index_args* a, void* workspace, size_t workspace_bytes, hipStream_t s) {
    MlaIndexParams p;
    const int rc = index_build(a, p);
    if (rc) return rc;
    const size_t need = index_ws_bytes(a, p);
    if (need > 0) {
        if (workspace == nullptr || workspace_bytes < need) return FASN_EWORKSPACE;
        if (!kv_aligned16(workspace)) return FASN_EALIGN;
        p.lg = static_cast<float*>(workspace);
    }
    if (a->dtype == FASN_DTYPE_BF16) index_launch_as<bf16_tag>(p, a->Hi, s);
    else index_launch_as<f16_tag>(p, a->Hi, s);
    FASN_LAUNCH(fasn_mla_index_select_kernel<MLI_SEL_NT>, dim3((unsigned)(p.B * p.Sq)), dim3(MLI_SEL_NT), 0, s, p);
    return launch_rc();
}

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_mla_index_workspace_bytes(const fasn_mla_index_args* args) {
    MlaIndexParams p;
    return index_build(args, p) == FASN_OK ? index_ws_bytes(args, p) : 0;
}

int fasn_mla_index(const fasn_mla_index_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return index_forward(args, workspace, workspace_bytes, (hipStream_t)stream);
}

int fasn_mla_index_append(const fasn_mla_index_args* args, const fasn_view4* k_new, fasn_stream_t stream) {
    MlaIndexParams p;
    int rc = index_build(args, p);
    if (rc) return rc;
    if (k_new == nullptr) return FASN_EINVAL;
    if ((rc = kv_check_view(*k_new))) return rc;
    p.kn = static_cast<const char*>(k_new->ptr);
    p.kns[0] = k_new->stride[0], p.kns[1] = k_new->stride[1];
    const int64_t nthr = (int64_t)p.B * p.Sq * (MLI_ROWB / 16);
    if ((nthr + 255) / 256 > INT_MAX) return FASN_EINVAL;
    FASN_LAUNCH(fasn_mla_index_append_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return launch_rc();
}

int fasn_mla_index_plan(const fasn_mla_index_args* args, char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return index_forward(args, plan_workspace(), ~size_t(0), nullptr); });
}

}  // extern "C"
