// Decode behind several shared prefixes in one call (include/fasn.h: fasn_fwd_prefix_groups, fasn_fwd_prefix_groups_workspace_bytes,
// fasn_prefix_groups_plan): the checks of the operand behind the family's base checks (kv_build, fasn_kv_host.h), the plan of the two
// passes, the workspace with the schedule table behind the partials, and the four launches of fasn_kvgroups.h. Like the shared-prefix
// operand, this one is not part of the operand sets of fasn_kv_host.h: the call has these entry points alone.
#include <limits.h>
#include "fasn_kv_host.h"
#include "fasn_kvgroups.h"

namespace fasn {
namespace {

struct KvGroupsFwd {
    KvPrefillParams pp;
    KvGroups gr;
    size_t suffix_elems, prefix_elems;   // partial rows of the two passes
};

constexpr int64_t KVG_MIN_TPS = KVS_ROWS / 8;   // the shared-prefix call's: 16 tiles of a full prefix per split
static_assert(KVG_MAX_GROUPS == FASN_PREFIX_GROUPS_MAX, "the schedule kernel's LDS counters hold the documented limit");

// kvs_build's rules with its codes and its order. The plan follows from shapes, num_groups, max_prefix_pages and capacity alone.
int kvg_build(const fasn_kvcache_args* a, const fasn_prefix_groups* pg, KvGroupsFwd& f) {
    const int rc = kv_build(kv_args(a), f.pp);
    if (rc) return rc;
    if (a->block_table == nullptr) return FASN_EUNSUPPORTED;    // a shared prefix is a set of pages
    if (a->D != 64 && a->D != 128) return FASN_EUNSUPPORTED;
    if (pg == nullptr || pg->prefix_lens == nullptr || pg->prefix_tables == nullptr || pg->prefix_group == nullptr || pg->num_groups < 1 ||
        pg->num_groups > FASN_PREFIX_GROUPS_MAX || pg->max_prefix_pages < 1 || pg->reserved != 0)
        return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(pg->prefix_lens) % 4 || reinterpret_cast<uintptr_t>(pg->prefix_tables) % 4 ||
        reinterpret_cast<uintptr_t>(pg->prefix_group) % 4)
        return FASN_EALIGN;
    const KvParams& p = f.pp.kv;
    const int64_t rows_all = (int64_t)p.B * p.R;
    if (rows_all > INT_MAX / 4) return FASN_EINVAL;   // (a row of the row space and twice its index are 32-bit in the prefix pass)
    const int64_t pkeys = (int64_t)pg->max_prefix_pages * a->page_size;
    const int64_t pcap = pkeys < p.capacity ? pkeys : p.capacity;
    const int64_t items_max = kvg_items_max(p.B, p.R, pg->num_groups);
    f.gr = KvGroups{};
    f.gr.plens = pg->prefix_lens;
    f.gr.ptabs = pg->prefix_tables;
    f.gr.pgroup = pg->prefix_group;
    f.gr.G = pg->num_groups;
    f.gr.mpp = pg->max_prefix_pages;
    f.gr.pcap = (int)pcap;
    f.gr.items_max = (int)items_max;
    f.gr.nsplit = (int)kv_nsplit(a->D, p.Hkv * items_max, (pcap + KV_KT - 1) / KV_KT, KVG_MIN_TPS);
    if ((int64_t)p.Hkv * items_max * f.gr.nsplit > INT_MAX) return FASN_EINVAL;
    f.suffix_elems = (size_t)p.B * p.Hkv * p.nsplit * p.R;
    f.prefix_elems = (size_t)p.Hkv * f.gr.nsplit * (size_t)rows_all;
    return FASN_OK;
}

// [suffix acc][prefix acc][suffix (m, l)][prefix (m, l)] as in the shared-prefix call - the accumulators first, so that every row of D
// floats is 16-byte aligned - then, at the next multiple of 16 bytes, the table
size_t kvg_table_offset(const KvGroupsFwd& f, int D) { return ((f.suffix_elems + f.prefix_elems) * (size_t)(D + 2) * sizeof(float) + 15) / 16 * 16; }
size_t kvg_ws_bytes(const KvGroupsFwd& f, int D) {
    return kvg_table_offset(f, D) + (size_t)kvg_table_ints(f.pp.kv.B, f.gr.items_max) * sizeof(int);
}

template <typename Tag, int D>
int kvg_launch_as(const KvGroupsFwd& f, hipStream_t s) {
    const KvParams& p = f.pp.kv;
    FASN_LAUNCH(fasn_kvgroups_schedule_kernel<256>, dim3(1), dim3(256), 0, s, p, f.gr);
    kv_launch<&fasn_kvgroups_prefix_kernel<Tag, D>>((unsigned)(p.Hkv * f.gr.items_max * f.gr.nsplit), kv_smem(D), s, p, f.gr);
    kv_launch<&fasn_kvgroups_suffix_kernel<Tag, D>>((unsigned)(p.B * p.Hkv * p.nsplit), kv_smem(D), s, p, f.gr);
    const int64_t nthr = (int64_t)p.B * p.Hkv * p.R * (D / 4);
    FASN_LAUNCH((fasn_kvgroups_combine_kernel<Tag, D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, p, f.gr);
    return launch_rc();
}

int kvg_forward(const fasn_kvcache_args* a, const fasn_prefix_groups* pg, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    KvGroupsFwd f;
    const int rc = kvg_build(a, pg, f);
    if (rc) return rc;
    if (workspace == nullptr || workspace_bytes < kvg_ws_bytes(f, a->D)) return FASN_EWORKSPACE;
    if (!kv_aligned16(workspace)) return FASN_EALIGN;
    float* const w = static_cast<float*>(workspace);
    f.pp.kv.part_o = w;
    f.gr.part_o = w + f.suffix_elems * a->D;
    f.pp.kv.part_ml = f.gr.part_o + f.prefix_elems * a->D;
    f.gr.part_ml = f.pp.kv.part_ml + f.suffix_elems * 2;
    f.gr.tab = reinterpret_cast<int*>(static_cast<char*>(workspace) + kvg_table_offset(f, a->D));
    const hipStream_t s = (hipStream_t)stream;
    if (a->dtype == FASN_DTYPE_BF16) return a->D == 64 ? kvg_launch_as<bf16_tag, 64>(f, s) : kvg_launch_as<bf16_tag, 128>(f, s);
    return a->D == 64 ? kvg_launch_as<f16_tag, 64>(f, s) : kvg_launch_as<f16_tag, 128>(f, s);
}

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_fwd_prefix_groups_workspace_bytes(const fasn_kvcache_args* args, const fasn_prefix_groups* groups) {
    KvGroupsFwd f;
    if (kvg_build(args, groups, f) != FASN_OK) return 0;
    return kvg_ws_bytes(f, args->D);
}

int fasn_fwd_prefix_groups(const fasn_kvcache_args* args, const fasn_prefix_groups* groups, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kvg_forward(args, groups, workspace, workspace_bytes, stream);
}

int fasn_prefix_groups_plan(const fasn_kvcache_args* args, const fasn_prefix_groups* groups, char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return kvg_forward(args, groups, plan_workspace(), ~size_t(0), nullptr); });
}

}  // extern "C"
