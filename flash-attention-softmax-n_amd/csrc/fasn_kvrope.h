// fasn_kvrope.h — rotary position embedding (RoPE) on the append side of the K/V-cache calls: ONE launch in front of the forward that
//   1. rotates row i of k_new[b, hkv] at position seqlens[b] + i and writes it to that cache row (paged or dense, addressed exactly as
//      fasn_kvcache_append_kernel / fasn_kvprefill_append_kernel address it; rows at a negative position or at / beyond the capacity
//      are dropped here, rows i >= qlen_b are neither read nor written),
//   2. copies row i of v_new to the same position, unrotated,
//   3. rotates row i of q[b, h] at p_i = i + len_b - qlen_b into q_out - len_b / qlen_b exactly as the forward kernels compute them
//      (kv_len, kvp_qlen / kvp_len), so p_i is the position of the ALiBi and window calls; rows i >= qlen_b are not read and not written.
// Without k_new / v_new only step 3 runs. The attention kernels and the append kernels are not touched: the forward that follows reads
// q_out in the place of q.
//
// Positions come from the lengths in device memory: a captured graph follows `seqlens` / `q_seqlens`. The table row is
// clamp(pos, 0, rows - 1) with rows >= capacity (host rule), so the clamp acts only on the negative p_i of causal rows that see no key
// and never reads out of bounds.
//
// Layouts (run-time flag). Features d < rotary_dim are rotated, the others copied. With c = cos[pos, d], s = sin[pos, d]:
//   half-split  (GPT-NeoX / Llama / GPT-OSS, rotate_half): x1 = x[d], x2 = x[d + rotary_dim / 2], d < rotary_dim / 2
//   interleaved (GPT-J):                                   x1 = x[2 d], x2 = x[2 d + 1]
//   y1 = x1 c - x2 s,   y2 = x2 c + x1 s   written where x1 / x2 came from.
// Arithmetic, pinned: operands widened to fp32, every product rounded to fp32 on its own, the sum / difference rounded to fp32 on its
// own (no fused multiply-add: contraction is off around the rotation), ONE rounding to the 16-bit type, to nearest even - bit for bit
// what eager torch gives for (x1.float() * c.float() - x2.float() * s.float()).to(dtype). The kernel is bound by memory, the four extra
// VALU operations per pair cost nothing.
//
// Work. One lane owns a UNIT of a row: two 16-byte chunks. Unit u < rotary_dim / 16 owns the chunks of the pairs d = 8 u .. 8 u + 7 -
// chunks u and u + rotary_dim / 16 (half-split) or 2 u and 2 u + 1 (interleaved) - and reads cos / sin[pos, 8 u .. 8 u + 7] as one
// (16-bit tables) or two (fp32 tables) 16-byte vectors each; the units beyond copy chunks 2 u and 2 u + 1. A K/V unit also copies chunks
// 2 u and 2 u + 1 of the v_new row. Lanes [0, nkv) are the K/V units (b, hkv, i, u), lanes [nkv, nkv + nq) the query units (b, h, i, u):
// the grid depends on shapes only. Plain 16-byte vector loads and stores, nothing else.
//
// fasn_kvvarlen_rope_kernel is the same launch on token-packed rows (fasn_kvvarlen.h): lanes (t, hkv, u) then (t, h, u) over the T tokens
// of the buffers, the sequence and position of a token from cu_seqlens_q in device memory.
#pragma once
#include "fasn_kvvarlen.h"

namespace fasn {

struct KvRopeParams {
    KvParams kv;          // q: the queries to rotate; kn / vn / kns / vns: the new rows (kn == nullptr: queries only); k / v: the cache
    const int* qlens;     // [B], device, or nullptr (every batch element has Sq positions)
    char* qo;             // q_out
    int64_t qos[3];       // element strides (batch, head, row)
    const char* cos;      // [rows][rd / 2]
    const char* sin;
    int64_t trs;          // table row stride, elements
    int rows;             // table rows, >= capacity
    int rd;               // rotary_dim
    int tf32;             // tables are fp32 (otherwise the 16-bit type of the call)
    int interleaved;
    int add_qlen;         // the prefill rule (kvp_len): len_b = seqlens[b] + (add_qlen ? qlen_b : 0), add_qlen = 0 / 1; -1: the decode rule (kv_len), seqlens[b] + seqlen_add
    int64_t nkv, nq;      // K/V units, query units
};

template <typename Tag>
FASN_DEV void kvrope_widen(u32x4 raw, float (&x)[8]) {
    uint16_t h[8];
    __builtin_memcpy(h, &raw, 16);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = ET<Tag>::to_f32(h[j]);
}
template <typename Tag>
FASN_DEV u32x4 kvrope_round(const float (&y)[8]) {
    f32x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = y[j];
    typename ET<Tag>::vec8 r = ET<Tag>::cvt8(v);   // one rounding, to nearest even
    u32x4 raw;
    __builtin_memcpy(&raw, &r, 16);
    return raw;
}
// 8 table values of one row from column c0 (a multiple of 8), widened to fp32
template <typename Tag>
FASN_DEV void kvrope_table(const char* t, int64_t elem, int tf32, float (&c)[8]) {
    if (tf32) {
        const u32x4 lo = gload16(t + elem * 4), hi = gload16(t + elem * 4 + 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = __uint_as_float(lo[j]), c[4 + j] = __uint_as_float(hi[j]);
    } else {
        kvrope_widen<Tag>(gload16(t + elem * 2), c);
    }
}

template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvrope_kernel(const KvRopeParams rp) {
    const KvParams& p = rp.kv;
    constexpr int UPR = D / 16;   // units per row
    int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= rp.nkv + rp.nq) return;
    const bool isq = gid >= rp.nkv;
    if (isq) gid -= rp.nkv;
    const int u = (int)(gid % UPR);
    int64_t rest = gid / UPR;
    const int i = (int)(rest % p.Sq);
    rest /= p.Sq;
    const int heads = isq ? p.H : p.Hkv;
    const int h = (int)(rest % heads), b = (int)(rest / heads);
    int qlen = p.Sq;
    if (rp.qlens != nullptr) qlen = min(max(rp.qlens[b], 0), p.Sq);
    if (i >= qlen) return;   // padding rows: neither read nor written
    int64_t pos;
    const char* src;
    char* dst;
    if (!isq) {
        pos = (int64_t)p.seqlens[b] + i;
        if (pos < 0 || pos >= p.capacity) return;   // dropped: the host does not know the lengths
        const int slot = (int)(pos / p.page_size), rip = (int)(pos % p.page_size);
        const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
        src = p.kn + (b * p.kns[0] + h * p.kns[1] + (int64_t)i * p.kns[2]) * 2;
        dst = p.k + (page * p.kps + (int64_t)rip * p.krs + (int64_t)h * p.khs) * 2;
        const char* const vsrc = p.vn + (b * p.vns[0] + h * p.vns[1] + (int64_t)i * p.vns[2]) * 2 + u * 32;
        char* const vdst = p.v + (page * p.vps + (int64_t)rip * p.vrs + (int64_t)h * p.vhs) * 2 + u * 32;
        const u32x4 v0 = gload16(vsrc), v1 = gload16(vsrc + 16);
        gstore16(vdst, v0);
        gstore16(vdst + 16, v1);
    } else {
        // len_b with the operand types of kv_len (decode: 32-bit sum) and kvp_len (prefill: 64-bit sum), restated because those helpers
        // broadcast the length of a wave-uniform b through readfirstlane and the lanes of a wave here belong to several batch elements
        int len;
        if (rp.add_qlen < 0) len = min(max(p.seqlens[b] + p.seqlen_add, 0), p.capacity);
        else len = (int)min(max((int64_t)p.seqlens[b] + (rp.add_qlen ? qlen : 0), (int64_t)0), (int64_t)p.capacity);
        pos = (int64_t)i + len - qlen;
        src = p.q + (b * p.qs[0] + h * p.qs[1] + (int64_t)i * p.qs[2]) * 2;
        dst = rp.qo + (b * rp.qos[0] + h * rp.qos[1] + (int64_t)i * rp.qos[2]) * 2;
    }
#include "fasn_kvrope_unit.inc"
}

// fasn_kvrope_kernel at DEPTH positions (fasn_kvcache.h: KvTree): the new rows are the nodes of a token tree. Node i of k_new / v_new is
// still WRITTEN to cache row seqlens[b] + i, but rotated at seqlens[b] + d_i, and the query at p_i = len_b - qlen_b + d_i, with
// d_i = max(popcount(mask[b, i] & the low qlen_b bits) - 1, 0). Everything else - the v_new copy, the dropped rows at or beyond the
// capacity, the untouched padding rows, the table-row clamp, layouts, table types, arithmetic - is the kernel's above: same lanes, same
// grid, the same unit text. The window member of the operand takes no part here.
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvrope_tree_kernel(const KvRopeParams rp, const KvTree tree) {
    const KvParams& p = rp.kv;
    constexpr int UPR = D / 16;   // units per row
    int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= rp.nkv + rp.nq) return;
    const bool isq = gid >= rp.nkv;
    if (isq) gid -= rp.nkv;
    const int u = (int)(gid % UPR);
    int64_t rest = gid / UPR;
    const int i = (int)(rest % p.Sq);
    rest /= p.Sq;
    const int heads = isq ? p.H : p.Hkv;
    const int h = (int)(rest % heads), b = (int)(rest / heads);
    int qlen = p.Sq;
    if (rp.qlens != nullptr) qlen = min(max(rp.qlens[b], 0), p.Sq);
    if (i >= qlen) return;   // padding rows: neither read nor written (qlen >= 1 from here on)
    const unsigned long long word = (unsigned long long)tree.mask[b * tree.sb + i] & (~0ull >> (64 - qlen));
    const int depth = max(__builtin_popcountll(word) - 1, 0);
    int64_t pos;
    const char* src;
    char* dst;
    if (!isq) {
        const int64_t at = (int64_t)p.seqlens[b] + i;   // the row written
        if (at < 0 || at >= p.capacity) return;         // dropped: the host does not know the lengths
        pos = (int64_t)p.seqlens[b] + depth;            // the position rotated at
        const int slot = (int)(at / p.page_size), rip = (int)(at % p.page_size);
        const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
        src = p.kn + (b * p.kns[0] + h * p.kns[1] + (int64_t)i * p.kns[2]) * 2;
        dst = p.k + (page * p.kps + (int64_t)rip * p.krs + (int64_t)h * p.khs) * 2;
        const char* const vsrc = p.vn + (b * p.vns[0] + h * p.vns[1] + (int64_t)i * p.vns[2]) * 2 + u * 32;
        char* const vdst = p.v + (page * p.vps + (int64_t)rip * p.vrs + (int64_t)h * p.vhs) * 2 + u * 32;
        const u32x4 v0 = gload16(vsrc), v1 = gload16(vsrc + 16);
        gstore16(vdst, v0);
        gstore16(vdst + 16, v1);
    } else {
        // len_b per lane, as in fasn_kvrope_kernel
        int len;
        if (rp.add_qlen < 0) len = min(max(p.seqlens[b] + p.seqlen_add, 0), p.capacity);
        else len = (int)min(max((int64_t)p.seqlens[b] + (rp.add_qlen ? qlen : 0), (int64_t)0), (int64_t)p.capacity);
        pos = (int64_t)depth + len - qlen;
        src = p.q + (b * p.qs[0] + h * p.qs[1] + (int64_t)i * p.qs[2]) * 2;
        dst = rp.qo + (b * rp.qos[0] + h * rp.qos[1] + (int64_t)i * rp.qos[2]) * 2;
    }
#include "fasn_kvrope_unit.inc"
}

// fasn_kvrope_kernel on TOKEN-PACKED rows (fasn_kvvarlen.h): one lane per (token t < T, head, unit), the K/V units first. The token's
// sequence is found as fasn_kvvarlen_append_kernel finds it - a binary search in cu - and a token of no sequence (at or beyond cu[B])
// or beyond its sequence's clamped length leaves before it reads a row. qlen_b is the schedule kernel's, the T - token0 clamp included:
// every row of q_out the forward reads through the item table was written here. len_b: kvp_len's rule, restated per lane as above.
// Under a malformed cu the search still ends at some index; t < T by the grid, b is a sequence index, the cache row lies below the
// capacity and the table row inside the tables: unspecified values, never an access outside the buffers.
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvvarlen_rope_kernel(const KvRopeParams rp, const KvPacked pk) {
    const KvParams& p = rp.kv;
    constexpr int UPR = D / 16;   // units per row
    int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= rp.nkv + rp.nq) return;
    const bool isq = gid >= rp.nkv;
    if (isq) gid -= rp.nkv;
    const int u = (int)(gid % UPR);
    const int64_t rest = gid / UPR;
    const int heads = isq ? p.H : p.Hkv;
    const int h = (int)(rest % heads), t = (int)(rest / heads);   // t < T: nkv / nq count T tokens
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
    const int token0 = (int)min(max(c0, (int64_t)0), (int64_t)pk.T);
    int qlen = (int)min(max((int64_t)pk.cu[b + 1] - c0, (int64_t)0), (int64_t)p.Sq);
    qlen = min(qlen, pk.T - token0);
    if (i >= qlen) return;
    int64_t pos;
    const char* src;
    char* dst;
    if (!isq) {
        pos = (int64_t)p.seqlens[b] + i;
        if (pos < 0 || pos >= p.capacity) return;   // dropped: the host does not know the lengths
        const int slot = (int)(pos / p.page_size), rip = (int)(pos % p.page_size);
        const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
        src = p.kn + (h * p.kns[1] + (int64_t)t * p.kns[2]) * 2;
        dst = p.k + (page * p.kps + (int64_t)rip * p.krs + (int64_t)h * p.khs) * 2;
        const char* const vsrc = p.vn + (h * p.vns[1] + (int64_t)t * p.vns[2]) * 2 + u * 32;
        char* const vdst = p.v + (page * p.vps + (int64_t)rip * p.vrs + (int64_t)h * p.vhs) * 2 + u * 32;
        const u32x4 v0 = gload16(vsrc), v1 = gload16(vsrc + 16);
        gstore16(vdst, v0);
        gstore16(vdst + 16, v1);
    } else {
        const int len = (int)min(max((int64_t)p.seqlens[b] + (rp.add_qlen ? qlen : 0), (int64_t)0), (int64_t)p.capacity);
        pos = i + len - qlen;
        src = p.q + (h * p.qs[1] + (int64_t)t * p.qs[2]) * 2;
        dst = rp.qo + (h * rp.qos[1] + (int64_t)t * rp.qos[2]) * 2;
    }
#include "fasn_kvrope_unit.inc"
}

}  // namespace fasn
