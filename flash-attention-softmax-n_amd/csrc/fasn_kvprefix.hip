// Decode over a paged K/V cache behind shared prefixes (include/fasn.h: fasn_fwd_shared_prefix, fasn_fwd_prefix_groups and the
// _workspace_bytes / _plan entry points of both): the checks of the prefix operand behind the family's base checks (kv_build,
// fasn_kv_host.h), the plan of the two passes, the workspace - for prefix groups with the schedule table behind the partials - and the
// launches of fasn_kvprefix.h. The two operands are not part of the operand sets of fasn_kv_host.h: the calls have these entry points alone.
#include <limits.h>
#include "fasn_kv_host.h"
#include "fasn_kvprefix.h"

namespace fasn {
namespace {

// what a call launches with: the decode parameters (the suffix pass's plan is the decode call's), the prefix operand as the kernels take
// it (Dev: KvShared or KvGroups) and the sizes the workspace is carved by
template <typename Dev>
struct KvPrefixFwd {
    KvPrefillParams pp;
    Dev x;
    size_t suffix_elems, prefix_elems;   // partial rows of the two passes
    size_t table_ints;                   // the schedule table behind the partials (one prefix: none)
};

// a prefix split's partial is 128 rows of D + 2 floats: what kv_build's rule asks of a 128-row block, 16 tiles of a full prefix
constexpr int64_t KVS_MIN_TPS = KVS_ROWS / 8;
static_assert(KVG_MAX_GROUPS == FASN_PREFIX_GROUPS_MAX, "the schedule kernel's LDS counters hold the documented limit");

// ---- what the two operands do not share. The operand's own rules - NULL / range / `reserved`, then alignment - and its pointers ...
int kvx_operand(const fasn_shared_prefix* sp, KvShared& sh) {
    if (sp == nullptr || sp->prefix_len == nullptr || sp->prefix_table == nullptr || sp->max_prefix_pages < 1 || sp->reserved != 0) return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(sp->prefix_len) % 4 || reinterpret_cast<uintptr_t>(sp->prefix_table) % 4) return FASN_EALIGN;
    sh.plen = sp->prefix_len;
    sh.ptab = sp->prefix_table;
    return FASN_OK;
}
int kvx_operand(const fasn_prefix_groups* pg, KvGroups& gr) {
    if (pg == nullptr || pg->prefix_lens == nullptr || pg->prefix_tables == nullptr || pg->prefix_group == nullptr || pg->num_groups < 1 ||
        pg->num_groups > FASN_PREFIX_GROUPS_MAX || pg->max_prefix_pages < 1 || pg->reserved != 0)
        return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(pg->prefix_lens) % 4 || reinterpret_cast<uintptr_t>(pg->prefix_tables) % 4 ||
        reinterpret_cast<uintptr_t>(pg->prefix_group) % 4)
        return FASN_EALIGN;
    gr.plens = pg->prefix_lens;
    gr.ptabs = pg->prefix_tables;
    gr.pgroup = pg->prefix_group;
    gr.G = pg->num_groups;
    gr.mpp = pg->max_prefix_pages;
    return FASN_OK;
}
// ... and the units of 128 rows the prefix pass has workgroups for: the blocks of the row space, the most items a table can hold
int64_t kvx_units(KvShared& sh, int64_t B, int64_t R) { return sh.nrb = (int)((B * R + KVS_ROWS - 1) / KVS_ROWS); }
int64_t kvx_units(KvGroups& gr, int64_t B, int64_t R) { return gr.items_max = (int)kvg_items_max(B, R, gr.G); }

// The base block's rules with their codes and their order (kv_build), then the calls' own: paged only, D of 64 / 128, the operand, its
// alignment, the size of the row space; prefix groups: the prefix pass's grid. The plan follows from shapes, max_prefix_pages, capacity
// and (prefix groups) num_groups alone.
template <typename Op, typename Dev>
int kvx_build(const fasn_kvcache_args* a, const Op* op, KvPrefixFwd<Dev>& f) {
    const int rc = kv_build(kv_args(a), f.pp);
    if (rc) return rc;
    if (a->block_table == nullptr) return FASN_EUNSUPPORTED;    // a shared prefix is a set of pages
    if (a->D != 64 && a->D != 128) return FASN_EUNSUPPORTED;
    f.x = Dev{};
    const int rc_op = kvx_operand(op, f.x);
    if (rc_op) return rc_op;
    const KvParams& p = f.pp.kv;
    const int64_t rows_all = (int64_t)p.B * p.R;
    if (rows_all > INT_MAX / 4) return FASN_EINVAL;   // (a row of the row space and twice its index are 32-bit in the prefix pass)
    const int64_t pkeys = (int64_t)op->max_prefix_pages * a->page_size;
    const int64_t pcap = pkeys < p.capacity ? pkeys : p.capacity;
    const int64_t units = kvx_units(f.x, p.B, p.R);
    f.x.pcap = (int)pcap;
    f.x.nsplit = (int)kv_nsplit(a->D, p.Hkv * units, (pcap + KV_KT - 1) / KV_KT, KVS_MIN_TPS);
    f.table_ints = 0;
    if constexpr (std::is_same_v<Dev, KvGroups>) {
        if ((int64_t)p.Hkv * units * f.x.nsplit > INT_MAX) return FASN_EINVAL;
        f.table_ints = (size_t)kvg_table_ints(p.B, units);
    }
    f.suffix_elems = (size_t)p.B * p.Hkv * p.nsplit * p.R;
    f.prefix_elems = (size_t)p.Hkv * f.x.nsplit * (size_t)rows_all;
    return FASN_OK;
}

// [suffix acc][prefix acc][suffix (m, l)][prefix (m, l)]: the accumulators first, so that every row of D floats is 16-byte aligned;
// then, where there is one, the table at the next multiple of 16 bytes
template <typename Dev>
size_t kvx_partial_bytes(const KvPrefixFwd<Dev>& f, int D) { return (f.suffix_elems + f.prefix_elems) * (size_t)(D + 2) * sizeof(float); }
template <typename Dev>
size_t kvx_table_offset(const KvPrefixFwd<Dev>& f, int D) { return (kvx_partial_bytes(f, D) + 15) / 16 * 16; }
template <typename Dev>
size_t kvx_ws_bytes(const KvPrefixFwd<Dev>& f, int D) {
    return f.table_ints == 0 ? kvx_partial_bytes(f, D) : kvx_table_offset(f, D) + f.table_ints * sizeof(int);
}

// the combine of both calls: one thread per (row, 4 features)
unsigned kvx_combine_grid(const KvParams& p, int D) { return (unsigned)(((int64_t)p.B * p.Hkv * p.R * (D / 4) + 255) / 256); }

template <typename Tag, int D>
int kvx_launch(const KvPrefixFwd<KvShared>& f, hipStream_t s) {
    const KvParams& p = f.pp.kv;
    kv_launch<&fasn_kvshared_prefix_kernel<Tag, D>>((unsigned)(p.Hkv * f.x.nrb * f.x.nsplit), kv_smem(D), s, p, f.x);
    kv_launch<&fasn_kvshared_suffix_kernel<Tag, D>>((unsigned)(p.B * p.Hkv * p.nsplit), kv_smem(D), s, p, f.x);
    FASN_LAUNCH((fasn_kvshared_combine_kernel<Tag, D>), dim3(kvx_combine_grid(p, D)), dim3(256), 0, s, p, f.x);
    return launch_rc();
}
template <typename Tag, int D>
int kvx_launch(const KvPrefixFwd<KvGroups>& f, hipStream_t s) {
    const KvParams& p = f.pp.kv;
    FASN_LAUNCH(fasn_kvgroups_schedule_kernel<256>, dim3(1), dim3(256), 0, s, p, f.x);
    kv_launch<&fasn_kvgroups_prefix_kernel<Tag, D>>((unsigned)(p.Hkv * f.x.items_max * f.x.nsplit), kv_smem(D), s, p, f.x);
    kv_launch<&fasn_kvgroups_suffix_kernel<Tag, D>>((unsigned)(p.B * p.Hkv * p.nsplit), kv_smem(D), s, p, f.x);
    FASN_LAUNCH((fasn_kvgroups_combine_kernel<Tag, D>), dim3(kvx_combine_grid(p, D)), dim3(256), 0, s, p, f.x);
    return launch_rc();
}

template <typename Dev, typename Op>
int kvx_forward(const fasn_kvcache_args* a, const Op* op, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    KvPrefixFwd<Dev> f;
    const int rc = kvx_build(a, op, f);
    if (rc) return rc;
    if (workspace == nullptr || workspace_bytes < kvx_ws_bytes(f, a->D)) return FASN_EWORKSPACE;
    if (!kv_aligned16(workspace)) return FASN_EALIGN;
    float* const w = static_cast<float*>(workspace);
    f.pp.kv.part_o = w;
    f.x.part_o = w + f.suffix_elems * a->D;
    f.pp.kv.part_ml = f.x.part_o + f.prefix_elems * a->D;
    f.x.part_ml = f.pp.kv.part_ml + f.suffix_elems * 2;
    if constexpr (std::is_same_v<Dev, KvGroups>) f.x.tab = reinterpret_cast<int*>(static_cast<char*>(workspace) + kvx_table_offset(f, a->D));
    return kv8_dispatch(a->dtype, a->D, [&](auto tag, auto d) { return kvx_launch<decltype(tag), decltype(d)::value>(f, (hipStream_t)stream); });
}
template <typename Dev, typename Op>
size_t kvx_workspace_bytes(const fasn_kvcache_args* a, const Op* op) {
    KvPrefixFwd<Dev> f;
    return kvx_build(a, op, f) == FASN_OK ? kvx_ws_bytes(f, a->D) : 0;
}

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_fwd_shared_prefix_workspace_bytes(const fasn_kvcache_args* args, const fasn_shared_prefix* prefix) {
    return kvx_workspace_bytes<KvShared>(args, prefix);
}

int fasn_fwd_shared_prefix(const fasn_kvcache_args* args, const fasn_shared_prefix* prefix, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kvx_forward<KvShared>(args, prefix, workspace, workspace_bytes, stream);
}

int fasn_shared_prefix_plan(const fasn_kvcache_args* args, const fasn_shared_prefix* prefix, char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return kvx_forward<KvShared>(args, prefix, plan_workspace(), ~size_t(0), nullptr); });
}

size_t fasn_fwd_prefix_groups_workspace_bytes(const fasn_kvcache_args* args, const fasn_prefix_groups* groups) {
    return kvx_workspace_bytes<KvGroups>(args, groups);
}

int fasn_fwd_prefix_groups(const fasn_kvcache_args* args, const fasn_prefix_groups* groups, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kvx_forward<KvGroups>(args, groups, workspace, workspace_bytes, stream);
}

int fasn_prefix_groups_plan(const fasn_kvcache_args* args, const fasn_prefix_groups* groups, char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return kvx_forward<KvGroups>(args, groups, plan_workspace(), ~size_t(0), nullptr); });
}

}  // extern "C"
