// fasn_kvvarlen.h — the prefill kernels of fasn_kvprefill.h on TOKEN-PACKED queries (continuous batching): the query positions of all
// sequences lie behind each other in one [T, H, D] buffer, cu[b] .. cu[b + 1] - 1 are the tokens of sequence b, cu in device memory.
// The existing kernels are not touched; these are their packed siblings.
//
//   fasn_kvvarlen_schedule_kernel  cu -> the item table: one item per (sequence, row block) that holds a token
//   fasn_kvvarlen_fwd_kernel       fasn_kvprefill_fwd.inc under FASN_KV_PACKED: one workgroup per (item, K/V head, split)
//   fasn_kvvarlen_fwd_window_kernel  the same kernel over the tiles of a sliding window only (FASN_KV_PACKED and FASN_KV_WINDOW)
//   fasn_kvvarlen_combine_kernel   (several splits only) merges the partials and scatters the rows through the item table
//   fasn_kvvarlen_append_kernel    k_new / v_new row t -> cache row seqlens[b] + (t - cu[b]) of the token's sequence
//
// Why a table. The padded call's grid is B * Hkv * ceil(Sq / PB) * nsplit: a step of many one-token sequences and one long chunk is
// nearly all workgroups that leave at once. Here the grid is items_max * Hkv * nsplit with
//   items_max = min(B * ceil(Sq / PB), T / PB + B)      (Sq = max_seqlen_q; sum_b ceil(qlen_b / PB) <= floor(sum_b qlen_b / PB) + B)
// - a bound from shapes alone, so the launches still do not depend on anything in device memory - and the table says which
// (sequence, row block) a workgroup owns. Items beyond the count leave before they read anything else.
//
// The table: sched[0] = the item count, sched[KVV_HEAD + KVV_ITEM * i ..] = (b, rb, token0, qlen) of item i with
//   token0 = clamp(cu[b], 0, T),  qlen = min(clamp(cu[b + 1] - cu[b], 0, Sq), T - token0),  0 <= rb < ceil(qlen / PB).
// Every clamp that keeps a token index inside [0, T) is made ONCE, by the schedule kernel; the forward and combine kernels take the
// table as it is (it lives in the call's workspace, nobody else writes it). Whatever cu holds, token0 + pos < T for every pos < qlen,
// b is a sequence index and the item count is at most items_max: a malformed cu gives unspecified values, never an access outside
// the buffers. Order: sequences in order, within a sequence the LAST row block first (fasn_kvprefill.h: later blocks see more keys).
//
// Rows. slot r = g * PB + pl of item (b, rb) is token token0 + rb * PB + pl of query head hkv * G + g, live iff g < G and
// rb * PB + pl < qlen: a packed buffer has no padding rows, so a slot beyond qlen is some other sequence's token and is neither read
// nor written. lse is [H, T]. Lengths, visibility, stale memory: fasn_kvprefill.h, unchanged.
#pragma once
#include "fasn_kvprefill.h"

namespace fasn {

constexpr int KVV_HEAD = 4;   // ints in front of the items (16 bytes): [0] the item count
constexpr int KVV_ITEM = 4;   // ints per item: b, rb, token0, qlen

struct KvPacked {
    const int* cu;       // [B + 1], device
    int* sched;          // the item table, in the workspace
    int T;               // tokens the buffers hold
    int items_max;
};

constexpr int64_t kvv_items_max(int64_t B, int64_t Sq, int64_t T, int64_t PB) {
    const int64_t by_len = B * ((Sq + PB - 1) / PB), by_tokens = T / PB + B;
    return by_len < by_tokens ? by_len : by_tokens;
}

// One workgroup of NT threads: NT sequences per round, their row-block counts scanned inside the waves and across them, every thread
// writes the items of its own sequence (a chunk of 2048 tokens at PB = 16 is 128 stores of 16 bytes).
template <int NT>
__global__ void __launch_bounds__(NT) fasn_kvvarlen_schedule_kernel(const KvPrefillParams pp, const KvPacked pk) {
    const KvParams& p = pp.kv;
    __shared__ int wsum[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;   // items of the sequences of earlier rounds
    for (int base = 0; base < p.B; base += NT) {
        const int b = base + tid;
        int token0 = 0, qlen = 0, nblk = 0;
        if (b < p.B) {
            const int c0 = pk.cu[b];
            token0 = min(max(c0, 0), pk.T);
            qlen = (int)min(max((int64_t)pk.cu[b + 1] - c0, (int64_t)0), (int64_t)p.Sq);
            qlen = min(qlen, pk.T - token0);
            nblk = (qlen + pp.PB - 1) / pp.PB;
        }
        int x = nblk;   // inclusive prefix inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) {
            const int s = wsum[w];
            before += w < wave ? s : 0;
            total += s;
        }
        __syncthreads();   // (wsum is written again in the next round)
        const int first = carry + before + x - nblk;
        for (int j = 0; j < nblk && first + j < pk.items_max; ++j)
            *reinterpret_cast<int4*>(pk.sched + KVV_HEAD + (int64_t)(first + j) * KVV_ITEM) = make_int4(b, nblk - 1 - j, token0, qlen);
        carry += total;
    }
    if (tid == 0) pk.sched[0] = min(carry, pk.items_max);
}

// fasn_kvvarlen_fwd_kernel<Tag, D>(KvPrefillParams, KvPacked): the text of the prefill forward, compiled a fourth time.
#define FASN_KV_PACKED 1
#define FASN_KV_WINDOW 0
#define FASN_KV_ALIBI 0
#include "fasn_kvprefill_fwd.inc"
#undef FASN_KV_WINDOW
// fasn_kvvarlen_fwd_window_kernel<Tag, D>(KvPrefillParams, KvPacked, KvWindow): a fifth time, the item's rows under a sliding window.
// Schedule and combine kernels are the ones above: the window changes which tiles a workgroup walks, not what an item or a partial is.
#define FASN_KV_WINDOW 1
#include "fasn_kvprefill_fwd.inc"
#undef FASN_KV_ALIBI
#undef FASN_KV_WINDOW
#undef FASN_KV_PACKED

// The arithmetic of fasn_kvprefill_combine_kernel, scattered through the item table: slot r of (item, hkv) is token
// token0 + rb * PB + r % PB of query head hkv * G + r / PB. One thread per (row slot, 4 features).
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvvarlen_combine_kernel(const KvPrefillParams pp, const KvPacked pk) {
    using E = ET<Tag>;
    const KvParams& p = pp.kv;
    constexpr int TPR = D / 4;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t slot = gid / TPR;   // ((item * Hkv + hkv), r)
    const int c4 = (int)(gid % TPR) * 4;
    if (slot >= (int64_t)pk.items_max * p.Hkv * KVP_ROWS) return;
    const int64_t blk = slot / KVP_ROWS;
    const int r = (int)(slot % KVP_ROWS);
    const int item = (int)(blk / p.Hkv), hkv = (int)(blk % p.Hkv);
    if (item >= pk.sched[0]) return;
    const int4 it = *reinterpret_cast<const int4*>(pk.sched + KVV_HEAD + (int64_t)item * KVV_ITEM);   // b, rb, token0, qlen
    const int g = r / pp.PB, pos = it.y * pp.PB + r % pp.PB;
    if (g >= p.G || pos >= it.w) return;
    const int h = hkv * p.G + g;
    const int64_t tok = (int64_t)it.z + pos;
    char* const oat = p.o + (h * p.os[1] + tok * p.os[2] + c4) * 2;
    const KvMerged m = kv_merge<D>(c4, p.part_o, p.part_ml, p.nsplit, [&](int s) { return (blk * p.nsplit + s) * KVP_ROWS + r; });
    kv_store_row<E>(oat, m);
    if (p.lse != nullptr && c4 == 0) p.lse[(int64_t)h * pk.T + tok] = kv_lse(m);
}

// fasn_kvprefill_append_kernel on packed rows: one thread per (token, K/V head, 16-byte chunk). The token's sequence is found by a
// binary search in cu (the first offset beyond t, minus one) rather than in a token map of the schedule kernel: the append is a call of
// its own, in front of the forward and without a workspace, and cu - B + 1 words that every thread reads - stays in the caches. Under a
// malformed cu the search still ends at some index; the tests below keep the row inside its sequence, the buffers and the capacity.
template <int D>
__global__ void __launch_bounds__(256) fasn_kvvarlen_append_kernel(const KvPrefillParams pp, const KvPacked pk) {
    const KvParams& p = pp.kv;
    constexpr int CPR = D / 8;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)pk.T * p.Hkv * CPR) return;
    const int ch = (int)(gid % CPR);
    const int64_t rest = gid / CPR;
    const int hkv = (int)(rest % p.Hkv), t = (int)(rest / p.Hkv);
    int lo = 0, hi = p.B + 1;   // the first index of cu[0 .. B] whose offset is beyond t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pk.cu[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    const int b = lo - 1;
    if (b < 0 || b >= p.B) return;   // a token at or beyond cu[B] (or in front of cu[0])
    const int64_t c0 = pk.cu[b];
    const int64_t i = t - c0;        // >= 0: cu[b] <= t
    if (i >= min(max((int64_t)pk.cu[b + 1] - c0, (int64_t)0), (int64_t)p.Sq)) return;
    const int64_t key = (int64_t)p.seqlens[b] + i;
    if (key < 0 || key >= p.capacity) return;
    const int slot = (int)(key / p.page_size), rip = (int)(key % p.page_size);
    const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
    const u32x4 kx = gload16(p.kn + (hkv * p.kns[1] + (int64_t)t * p.kns[2]) * 2 + ch * 16);
    const u32x4 vx = gload16(p.vn + (hkv * p.vns[1] + (int64_t)t * p.vns[2]) * 2 + ch * 16);
    gstore16(p.k + (page * p.kps + (int64_t)rip * p.krs + (int64_t)hkv * p.khs) * 2 + ch * 16, kx);
    gstore16(p.v + (page * p.vps + (int64_t)rip * p.vrs + (int64_t)hkv * p.vhs) * 2 + ch * 16, vx);
}

}  // namespace fasn
