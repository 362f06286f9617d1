// fasn_kvprefill.h — PREFILL over a K/V cache: any number of new query positions per batch element against a paged or dense cache,
// cache lengths AND query lengths in device memory. The decode kernels of fasn_kvcache.h are not touched; these are their row-block
// siblings and share the header's parameter block, tile geometry (KV_KT, kv_nbuf, kv_smem), kv_dma16 and nothing else.
//
//   fasn_kvprefill_append_kernel   rows i < qlen_b of k_new / v_new -> cache rows seqlens[b] + i (dropped beyond the capacity)
//   fasn_kvprefill_fwd_kernel      one workgroup per (batch element, K/V head, row block, split); with one split it normalises and stores
//                                  o / lse itself, with several it writes un-normalised partials
//   fasn_kvprefill_fwd_alibi_kernel  the same kernel with the ALiBi term -slope_h |j - p_i| in the scores (fasn_kvprefill_fwd.inc holds both)
//   fasn_kvprefill_fwd_window_kernel  the same kernel over the tiles of a sliding window only (fasn_kvcache.h: KvWindow)
//   fasn_kvprefill_fwd_tree_kernel  the same kernel on the nodes of a token tree (fasn_kvcache.h: KvTree): every row block walks to len_b
//   fasn_kvprefill_combine_kernel  (several splits only) merges the partials and scatters the rows of the block map
//
// Row blocks. A workgroup owns KVP_ROWS = 128 row slots: the G query heads of one K/V head times PB = 128 / G consecutive positions,
//   slot r = g * PB + pl,   position pos = rb * PB + pl,   query head h = hkv * G + g      (slots with g >= G or pos >= Sq are idle)
// so every K/V tile a workgroup stages serves all G heads and the cache is read once per K/V head and row block. One lane owns one slot
// exactly as in fasn_kvcache_fwd_kernel (S^T = K Q^T, O^T += V^T P^T, same LDS tile image and fragment reads).
//
// Lengths. qlen_b = clamp(q_seqlens[b], 0, Sq) (no q_seqlens: Sq), len_b = clamp(seqlens[b] + (seqlen_add ? qlen_b : 0), 0, capacity).
// Position i < qlen_b sees key j iff j < len_b and (causal) j <= i + len_b - qlen_b. Positions i >= qlen_b are padding: o = 0,
// lse = -inf. A block's tiles end at ceil(min(len_b, pos_hi + len_b - qlen_b + 1) / 64) (pos_hi: its last real position); the per-row
// mask branch runs only on tiles that reach beyond the limit of the block's FIRST position. A block whose first position is >= qlen_b
// stores its neutral result and leaves before it reads a table entry. The grid depends on shapes and capacity only.
//
// Order. Later row blocks see more keys and the dispatcher hands workgroups out in order: the LAST row block comes first in the grid.
// Stale memory: the rules of fasn_kvcache.h, unchanged (per-tile descriptor ranges, zero-range descriptors past the block's range, LDS
// zeroed before first use, vmcnt(0) before the workgroup ends, unneeded table entries never read).
#pragma once
#include "fasn_kvcache.h"

namespace fasn {

constexpr int KVP_ROWS = 128;   // row slots of a workgroup

struct KvPrefillParams {
    KvParams kv;          // part_o / part_ml: [B * Hkv * nrb][nsplit][KVP_ROWS][D] and [...][KVP_ROWS][2]; kv.R is not used
    const int* qlens;     // [B], device, or nullptr (every batch element has Sq positions)
    int PB;               // positions per row block = KVP_ROWS / G
    int nrb;              // row blocks = ceil(Sq / PB)
};

FASN_DEV int kvp_qlen(const KvPrefillParams& pp, int b) {
    if (pp.qlens == nullptr) return pp.kv.Sq;
    return min(max(__builtin_amdgcn_readfirstlane(pp.qlens[b]), 0), pp.kv.Sq);
}
FASN_DEV int kvp_len(const KvPrefillParams& pp, int b, int qlen) {
    const int64_t len = (int64_t)__builtin_amdgcn_readfirstlane(pp.kv.seqlens[b]) + (pp.kv.seqlen_add ? qlen : 0);
    return (int)min(max(len, (int64_t)0), (int64_t)pp.kv.capacity);
}

// fasn_kvprefill_fwd_kernel<Tag, D>(KvPrefillParams), fasn_kvprefill_fwd_alibi_kernel<Tag, D>(KvPrefillParams, KvAlibi) and
// fasn_kvprefill_fwd_window_kernel<Tag, D>(KvPrefillParams, KvWindow): one text, compiled three times, for the reason fasn_kvcache.h gives.
// (FASN_KV_PACKED: the token-packed siblings of fasn_kvvarlen.h, a fourth and - under a window - a fifth compilation of the same text.)
// (FASN_KV_TREE: fasn_kvprefill_fwd_tree_kernel<Tag, D>(KvPrefillParams, KvTree), the token-tree sibling, one more compilation.)
#define FASN_KV_PACKED 0
#define FASN_KV_TREE 0
#define FASN_KV_WINDOW 0
#define FASN_KV_ALIBI 0
#include "fasn_kvprefill_fwd.inc"
#undef FASN_KV_ALIBI
#define FASN_KV_ALIBI 1
#include "fasn_kvprefill_fwd.inc"
#undef FASN_KV_ALIBI
#undef FASN_KV_WINDOW
#define FASN_KV_ALIBI 0
#define FASN_KV_WINDOW 1
#include "fasn_kvprefill_fwd.inc"
#undef FASN_KV_WINDOW
#undef FASN_KV_TREE
#define FASN_KV_WINDOW 0
#define FASN_KV_TREE 1
#include "fasn_kvprefill_fwd.inc"
#undef FASN_KV_TREE
#undef FASN_KV_WINDOW
#undef FASN_KV_ALIBI
#undef FASN_KV_PACKED

// Merge the partials of a row slot (the arithmetic of fasn_kvcache_combine_kernel) and scatter it through the block map: slot r of
// (b, hkv, rb) is o[b, hkv * G + r / PB, rb * PB + r % PB, :]. Padding positions get zeros / -inf here; their partials are never read.
// One thread per (row slot, 4 features).
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvprefill_combine_kernel(const KvPrefillParams pp) {
    using E = ET<Tag>;
    const KvParams& p = pp.kv;
    constexpr int TPR = D / 4;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t slot = gid / TPR;   // ((b * Hkv + hkv) * nrb + rb, r)
    const int c4 = (int)(gid % TPR) * 4;
    if (slot >= (int64_t)p.B * p.Hkv * pp.nrb * KVP_ROWS) return;
    const int64_t blk = slot / KVP_ROWS;
    const int r = (int)(slot % KVP_ROWS);
    const int rb = (int)(blk % pp.nrb), bk = (int)(blk / pp.nrb);
    const int g = r / pp.PB, pos = rb * pp.PB + r % pp.PB;
    if (g >= p.G || pos >= p.Sq) return;
    const int b = bk / p.Hkv, h = (bk % p.Hkv) * p.G + g;
    char* const oat = p.o + (b * p.os[0] + h * p.os[1] + (int64_t)pos * p.os[2] + c4) * 2;
    float* const lat = p.lse != nullptr && c4 == 0 ? p.lse + ((int64_t)b * p.H + h) * p.Sq + pos : nullptr;
    int qlen = p.Sq;
    if (pp.qlens != nullptr) qlen = min(max(pp.qlens[b], 0), p.Sq);
    if (pos >= qlen) {
        gstore8(oat, u32x2{0u, 0u});
        if (lat != nullptr) *lat = -INFINITY;
        return;
    }
    const KvMerged m = kv_merge<D>(c4, p.part_o, p.part_ml, p.nsplit, [&](int s) { return (blk * p.nsplit + s) * KVP_ROWS + r; });
    kv_store_row<E>(oat, m);
    if (lat != nullptr) *lat = kv_lse(m);
}

// fasn_kvcache_append_kernel plus the i < qlen_b test: padding rows of k_new / v_new are neither read nor written.
template <int D>
__global__ void __launch_bounds__(256) fasn_kvprefill_append_kernel(const KvPrefillParams pp) {
    const KvParams& p = pp.kv;
    constexpr int CPR = D / 8;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)p.B * p.Hkv * p.Sq * CPR) return;
    const int ch = (int)(gid % CPR);
    int64_t rest = gid / CPR;
    const int i = (int)(rest % p.Sq);
    rest /= p.Sq;
    const int hkv = (int)(rest % p.Hkv), b = (int)(rest / p.Hkv);
    if (pp.qlens != nullptr && i >= pp.qlens[b]) return;
    const int64_t key = (int64_t)p.seqlens[b] + i;
    if (key < 0 || key >= p.capacity) return;
    const int slot = (int)(key / p.page_size), rip = (int)(key % p.page_size);
    const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
    const u32x4 kx = gload16(p.kn + (b * p.kns[0] + hkv * p.kns[1] + (int64_t)i * p.kns[2]) * 2 + ch * 16);
    const u32x4 vx = gload16(p.vn + (b * p.vns[0] + hkv * p.vns[1] + (int64_t)i * p.vns[2]) * 2 + ch * 16);
    gstore16(p.k + (page * p.kps + (int64_t)rip * p.krs + (int64_t)hkv * p.khs) * 2 + ch * 16, kx);
    gstore16(p.v + (page * p.vps + (int64_t)rip * p.vrs + (int64_t)hkv * p.vhs) * 2 + ch * 16, vx);
}

}  // namespace fasn
