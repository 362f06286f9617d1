// Shared-prefix decode over a paged K/V cache (include/fasn.h: fasn_fwd_shared_prefix, fasn_fwd_shared_prefix_workspace_bytes,
// fasn_shared_prefix_plan): the checks of the prefix operand behind the family's base checks (kv_build, fasn_kv_host.h), the plan of the
// two passes, the workspace and the three launches of fasn_kvshared.h. The operand is not part of the operand sets of fasn_kv_host.h: the
// call has these entry points alone.
#include <limits.h>
#include "fasn_kv_host.h"
#include "fasn_kvshared.h"

namespace fasn {
namespace {

// what the call launches with: the decode parameters (the suffix pass's plan is the decode call's), the prefix operand and pass
struct KvSharedFwd {
    KvPrefillParams pp;
    KvShared sh;
    size_t suffix_elems, prefix_elems;   // partial rows of the two passes
};

// a prefix split's partial is 128 rows of D + 2 floats: what kv_build's rule asks of a 128-row block, 16 tiles of a full prefix
constexpr int64_t KVS_MIN_TPS = KVS_ROWS / 8;

// The base block's rules with their codes and their order (kv_build), then the call's own: paged only, D of 64 / 128, the operand, its
// alignment. The plan follows from shapes, max_prefix_pages and capacity alone.
int kvs_build(const fasn_kvcache_args* a, const fasn_shared_prefix* sp, KvSharedFwd& f) {
    const int rc = kv_build(kv_args(a), f.pp);
    if (rc) return rc;
    if (a->block_table == nullptr) return FASN_EUNSUPPORTED;    // a shared prefix is a set of pages
    if (a->D != 64 && a->D != 128) return FASN_EUNSUPPORTED;
    if (sp == nullptr || sp->prefix_len == nullptr || sp->prefix_table == nullptr || sp->max_prefix_pages < 1 || sp->reserved != 0) return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(sp->prefix_len) % 4 || reinterpret_cast<uintptr_t>(sp->prefix_table) % 4) return FASN_EALIGN;
    const KvParams& p = f.pp.kv;
    const int64_t rows_all = (int64_t)p.B * p.R;
    if (rows_all > INT_MAX / 4) return FASN_EINVAL;   // (a row of the row space and twice its index are 32-bit in the prefix pass)
    const int64_t pkeys = (int64_t)sp->max_prefix_pages * a->page_size;
    const int64_t pcap = pkeys < p.capacity ? pkeys : p.capacity;
    const int64_t nrb = (rows_all + KVS_ROWS - 1) / KVS_ROWS;
    f.sh = KvShared{};
    f.sh.plen = sp->prefix_len;
    f.sh.ptab = sp->prefix_table;
    f.sh.pcap = (int)pcap;
    f.sh.nrb = (int)nrb;
    f.sh.nsplit = (int)kv_nsplit(a->D, p.Hkv * nrb, (pcap + KV_KT - 1) / KV_KT, KVS_MIN_TPS);
    f.suffix_elems = (size_t)p.B * p.Hkv * p.nsplit * p.R;
    f.prefix_elems = (size_t)p.Hkv * f.sh.nsplit * (size_t)rows_all;
    return FASN_OK;
}

// [suffix acc][prefix acc][suffix (m, l)][prefix (m, l)]: the accumulators first, so that every row of D floats is 16-byte aligned
size_t kvs_ws_bytes(const KvSharedFwd& f, int D) { return (f.suffix_elems + f.prefix_elems) * (size_t)(D + 2) * sizeof(float); }

template <typename Tag, int D>
int kvs_launch_as(const KvSharedFwd& f, hipStream_t s) {
    const KvParams& p = f.pp.kv;
    kv_launch<&fasn_kvshared_prefix_kernel<Tag, D>>((unsigned)(p.Hkv * f.sh.nrb * f.sh.nsplit), kv_smem(D), s, p, f.sh);
    kv_launch<&fasn_kvshared_suffix_kernel<Tag, D>>((unsigned)(p.B * p.Hkv * p.nsplit), kv_smem(D), s, p, f.sh);
    const int64_t nthr = (int64_t)p.B * p.Hkv * p.R * (D / 4);
    FASN_LAUNCH((fasn_kvshared_combine_kernel<Tag, D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, p, f.sh);
    return launch_rc();
}

int kvs_forward(const fasn_kvcache_args* a, const fasn_shared_prefix* sp, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    KvSharedFwd f;
    const int rc = kvs_build(a, sp, f);
    if (rc) return rc;
    if (workspace == nullptr || workspace_bytes < kvs_ws_bytes(f, a->D)) return FASN_EWORKSPACE;
    if (!kv_aligned16(workspace)) return FASN_EALIGN;
    float* const w = static_cast<float*>(workspace);
    f.pp.kv.part_o = w;
    f.sh.part_o = w + f.suffix_elems * a->D;
    f.pp.kv.part_ml = f.sh.part_o + f.prefix_elems * a->D;
    f.sh.part_ml = f.pp.kv.part_ml + f.suffix_elems * 2;
    const hipStream_t s = (hipStream_t)stream;
    if (a->dtype == FASN_DTYPE_BF16) return a->D == 64 ? kvs_launch_as<bf16_tag, 64>(f, s) : kvs_launch_as<bf16_tag, 128>(f, s);
    return a->D == 64 ? kvs_launch_as<f16_tag, 64>(f, s) : kvs_launch_as<f16_tag, 128>(f, s);
}

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_fwd_shared_prefix_workspace_bytes(const fasn_kvcache_args* args, const fasn_shared_prefix* prefix) {
    KvSharedFwd f;
    if (kvs_build(args, prefix, f) != FASN_OK) return 0;
    return kvs_ws_bytes(f, args->D);
}

int fasn_fwd_shared_prefix(const fasn_kvcache_args* args, const fasn_shared_prefix* prefix, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kvs_forward(args, prefix, workspace, workspace_bytes, stream);
}

int fasn_shared_prefix_plan(const fasn_kvcache_args* args, const fasn_shared_prefix* prefix, char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return kvs_forward(args, prefix, plan_workspace(), ~size_t(0), nullptr); });
}

}  // extern "C"
