// fasn_kvcache.h — forward over a K/V CACHE (inference): paged or dense cache, lengths in device memory, grouped-query rows.
//
// Three kernels beside the training / prefill kernels (none of which changes):
//   fasn_kvcache_append_kernel   k_new / v_new rows -> cache rows len_b .. len_b + Sq - 1 (dropped beyond the capacity)
//   fasn_kvcache_fwd_kernel      split-K walk over the pages of one (batch element, K/V head): un-normalised partials
//   fasn_kvcache_combine_kernel  merges the partials and scatters the rows back to o[b, h, pos, :] / lse[b, h, pos]
//
// Rows. The G = H / Hkv query heads that share a K/V head times the Sq query positions are the rows of ONE problem:
//   row r = g * Sq + pos   (g = query head of the group, pos = query position),   query head h = hkv * G + g,   R = G * Sq <= 128
// so a K/V tile is read once per K/V head whatever G is. One lane owns one row (S^T = K Q^T, O^T += V^T P^T as in fasn_fwd_kernel.h:
// same LDS tile image, same fragment reads); every row carries the softmax_n of its own query head (lane-private, read once in front
// of the tile loop) and its own causal limit: key j is visible to row r iff j <= pos(r) + len_b - Sq.
//
// Lengths. len_b = clamp(seqlens[b] + seqlen_add, 0, capacity) is read INSIDE the kernels. The grid depends on shapes and capacity
// only: split s of nsplit owns the tiles [s * tps_b, (s + 1) * tps_b) with tps_b = ceil(ceil(len_b / 64) / nsplit), a workgroup whose
// range is empty writes the neutral partial (m = -inf, l = 0; split 0: the sink state m = 0, l = n) and leaves.
//
// Stale memory. A K/V tile is fetched through a buffer descriptor of its own: base = the tile's first row, range = up to the last
// row below len_b. Rows at or beyond len_b are out of range for it and arrive as zeros (the V operand of an MFMA must not carry a
// stale NaN even under weight 0), tiles beyond the split's range get a zero-range descriptor and no block-table entry is read for
// them. The whole per-lane offset sits in the instruction's VGPR offset (the scalar offset takes no part in the range check).
#pragma once
#include "fasn_common.h"

namespace fasn {

struct KvParams {
    const char* q;
    char* o;
    float* lse;          // [B, H, Sq] or nullptr
    char* k;             // cache pools
    char* v;
    int64_t qs[3], os[3];             // element strides (batch, head, row)
    int64_t kps, krs, khs;            // K cache element strides (page, row, head)
    int64_t vps, vrs, vhs;
    const int* bt;       // block table [B][bts] or nullptr (dense: page = batch element)
    int64_t bts;
    const int* seqlens;  // [B], device
    int seqlen_add;
    int tpp;             // 64-key tiles per page (dense: no page ever ends)
    int page_size;
    int capacity;        // keys a batch element can hold
    int B, H, Hkv, G, Sq, R;
    int causal;
    float c;             // scale * log2(e)
    float n;
    const float* nt;     // per-(batch, query head) softmax_n or nullptr
    int nsb, nsh;
    int nsplit;
    float* part_o;       // [B * Hkv][nsplit][R][D]
    float* part_ml;      // [B * Hkv][nsplit][R][2]
    // append
    const char* kn;
    const char* vn;
    int64_t kns[3], vns[3];           // k_new / v_new element strides (batch, K/V head, row)
};

constexpr int KV_KT = 64;   // keys per tile
constexpr int kv_nbuf(int D) { return D <= 64 ? 3 : 2; }                        // LDS tile buffers per operand (48 KiB / 64 KiB: three / two workgroups per CU)
constexpr int kv_smem(int D) { return 2 * kv_nbuf(D) * KV_KT * D * 2; }

FASN_DEV int kv_len(const KvParams& p, int b) {
    const int len = __builtin_amdgcn_readfirstlane(p.seqlens[b]) + p.seqlen_add;
    return min(max(len, 0), p.capacity);
}

// 16 bytes per lane into LDS through a descriptor that was just built in SGPRs: as lds_dma16, with the wait states an SGPR written by
// the scalar or vector unit needs before a memory instruction reads it as a descriptor (cdna_hip_programming.md, inline-asm rule 2)
FASN_DEV void kv_dma16(u32x4 rsrc, uint32_t lds_base, uint32_t voff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lds_base), "v"(voff), "s"(rsrc) : "memory", "m0");
}

template <typename Tag, int D>
__global__ void __launch_bounds__(256, 2) fasn_kvcache_fwd_kernel(const KvParams p) {
    using E = ET<Tag>;
    using vec8 = typename E::vec8;
    constexpr int NT = 256;
    constexpr int NBUF = kv_nbuf(D);
    constexpr int ROWB = D * 2;
    constexpr int TILEB = KV_KT * ROWB;
    constexpr int KS = D / 16;
    constexpr int DB = D / 32;
    constexpr int CPR = D / 8;
    constexpr int NLD = (KV_KT * CPR) / NT;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const ldsK = smem;
    char* const ldsV = smem + NBUF * TILEB;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int hi = lane >> 5;

    const int wg = (int)blockIdx.x;
    const int split = wg % p.nsplit;
    const int bk = wg / p.nsplit;          // b * Hkv + hkv
    const int b = bk / p.Hkv, hkv = bk % p.Hkv;

    // ---- this split's tile range, from the length in device memory
    const int len = kv_len(p, b);
    const int tiles_b = (len + KV_KT - 1) / KV_KT;
    const int tps = (tiles_b + p.nsplit - 1) / p.nsplit;
    const int t0 = min(split * tps, tiles_b);
    const int t1 = min(t0 + tps, tiles_b);

    // ---- the lane's row: query head of the group, position, softmax_n, causal limit
    const int row = wave * 32 + l31;
    const bool row_ok = row < p.R;
    const int g = row_ok ? row / p.Sq : 0;
    const int pos = row_ok ? row - g * p.Sq : 0;
    const int h = hkv * p.G + g;
    float n_row = p.n;
    if (p.nt != nullptr) n_row = p.nt[b * p.nsb + h * p.nsh];
    const bool wave_rows = wave * 32 < p.R;   // a wave without rows only helps staging

    vec8 qf[KS];
    {
        const char* rp = p.q + (b * p.qs[0] + h * p.qs[1] + (int64_t)pos * p.qs[2]) * 2 + hi * 16;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            u32x4 raw = {0u, 0u, 0u, 0u};
            if (row_ok) raw = gload16(rp + s * 32);
            __builtin_memcpy(&qf[s], &raw, 16);
        }
    }

    // ---- staging: thread tid fills slots tid + i * 256 of the tile image (slot = 16 bytes; the chunk that belongs there after the swizzle)
    unsigned kvoff[NLD], vvoff[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int ci = tid + i * NT;
        const int r = ci / CPR, ch = (ci % CPR) ^ swz_f<D>(r);
        kvoff[i] = (unsigned)(r * (int)p.krs * 2 + ch * 16);
        vvoff[i] = (unsigned)(r * (int)p.vrs * 2 + ch * 16);
    }
    const uint32_t ldsK_w = lds_addr(ldsK) + wave * 1024, ldsV_w = lds_addr(ldsV) + wave * 1024;
    const char* const kpool = p.k + (int64_t)hkv * p.khs * 2;
    const char* const vpool = p.v + (int64_t)hkv * p.vhs * 2;

    // the tile that is requested next: its index, page slot and tile inside the page advance together (no division in the loop)
    int u = t0;
    int u_slot = t0 / p.tpp;
    int u_tip = t0 - u_slot * p.tpp;
    // Page ids are wave-uniform and the table does not change while the kernel runs: read through the constant address space they are
    // scalar loads whose wait the compiler places at the first use - the NEXT tile's request - instead of vector loads whose wait
    // would drain the K/V requests just issued. Entries of tiles outside the range are never read.
    const __attribute__((address_space(4))) int* const bt_row = (const __attribute__((address_space(4))) int*)(p.bt + (int64_t)b * p.bts);
    const bool paged = p.bt != nullptr;
    auto page_of = [&](int tile, int slot) -> int {
        if (tile >= t1) return 0;
        return paged ? bt_row[slot] : b;
    };
    int u_page = page_of(u, u_slot);
    auto request_next = [&](int buf) {
        const int nvis = u < t1 ? min(KV_KT, len - u * KV_KT) : 0;   // rows of the tile below len_b (>= 1 inside the range)
        const int64_t koff = ((int64_t)u_page * p.kps + (int64_t)u_tip * KV_KT * p.krs) * 2;
        const int64_t voff = ((int64_t)u_page * p.vps + (int64_t)u_tip * KV_KT * p.vrs) * 2;
        const uint32_t kbytes = nvis > 0 ? (uint32_t)((nvis - 1) * (int)p.krs * 2 + ROWB) : 0u;
        const uint32_t vbytes = nvis > 0 ? (uint32_t)((nvis - 1) * (int)p.vrs * 2 + ROWB) : 0u;
        const u32x4 krw = make_rsrc_words(kpool + koff, kbytes), vrw = make_rsrc_words(vpool + voff, vbytes);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            kv_dma16(krw, __builtin_amdgcn_readfirstlane(ldsK_w + buf * TILEB + i * NT * 16), kvoff[i]);
            kv_dma16(vrw, __builtin_amdgcn_readfirstlane(ldsV_w + buf * TILEB + i * NT * 16), vvoff[i]);
        }
        ++u;
        if (++u_tip == p.tpp) {
            u_tip = 0;
            ++u_slot;
        }
        u_page = page_of(u, u_slot);   // the next tile's page id is on its way while this one's data is
    };

    // ---- online-softmax state of the row (log2 domain); the sink (+n) belongs to split 0
    const bool sink = n_row > 0.f && split == 0;
    float m_run = sink ? 0.f : -INFINITY;
    float l_run = (sink && hi == 0) ? n_row : 0.f;   // the two half-lanes' partial sums are added at the end
    f32x16 oacc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
    const int vis = !row_ok ? -1 : (p.causal ? pos + len - p.Sq : len - 1);   // last visible key of the row
    const int all_vis = p.causal ? len - p.Sq : len - 1;                          // every row sees the keys up to here

#pragma unroll
    for (int s = 0; s < KS; ++s) retire_loads(qf[s]);
    retire_loads(n_row);

    // ---- the tile buffers start as zeros: a request that is out of range for its descriptor must leave nothing behind that is not
    // a finite number, whether the hardware fills the slot with zeros or leaves it alone (afterwards a slot holds zeros or visible rows)
    for (int i = tid; i < 2 * NBUF * TILEB / 16; i += NT) *LDS_PTR(u32x4, smem + i * 16) = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    // ---- prologue: NBUF - 1 tiles in flight
#pragma unroll
    for (int i = 0; i < NBUF - 1; ++i) request_next(i);

    int buf = 0;
    for (int t = t0; t < t1; ++t) {
        // tile t has landed (this wave's share: the NBUF - 2 younger tiles may still be in flight), then everybody's share has, and
        // everybody is done with tile t - 1, whose buffer takes the next request
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NBUF - 2) * 2 * NLD) : "memory");
        __syncthreads();
        request_next(buf == 0 ? NBUF - 1 : buf - 1);
        if (wave_rows) {
            const char* tK = ldsK + buf * TILEB;
            const char* tV = ldsV + buf * TILEB;
            const int k0 = t * KV_KT;
            f32x16 sacc[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[kb][r] = 0.f;
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const vec8 kf = lds_read_rowfrag<E, D>(tK, kb * 32 + l31, s, hi);
                    sacc[kb] = E::mfma(kf, qf[s], sacc[kb]);
                }
            }
            // scores in the log2 domain; hidden keys (beyond the row's causal limit, which is below len_b) at -inf
            float mx = -INFINITY;
            if (k0 + KV_KT - 1 <= all_vis) {   // wave-uniform (lanes without a row carry zero queries; their state is never stored)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        sacc[kb][r] *= p.c;
                        mx = fmaxf(mx, sacc[kb][r]);
                    }
            } else {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = k0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                        const float y = key <= vis ? sacc[kb][r] * p.c : -INFINITY;
                        sacc[kb][r] = y;
                        mx = fmaxf(mx, y);
                    }
            }
            mx = max_across_halves(mx);
            const float m_new = fmaxf(m_run, mx);
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;   // nothing visible so far
            const float alpha = fast_exp2(m_run - m_use);
            float rs = 0.f;
            vec8 pf[2][2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    f32x8 x;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        x[e] = fast_exp2(sacc[kb][8 * t2 + e] - m_use);
                        rs += x[e];
                    }
                    pf[kb][t2] = E::cvt8(x);
                }
            l_run = l_run * alpha + rs;
            m_run = m_new;
            if (!__all(alpha == 1.0f)) {
#pragma unroll
                for (int d = 0; d < DB; ++d)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[d][r] *= alpha;
            }
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                    for (int d = 0; d < DB; ++d) {
                        const vec8 vf = lds_read_trfrag<E, D>(tV, kb * 32 + 16 * t2, d, lane);
                        oacc[d] = E::mfma(vf, pf[kb][t2], oacc[d]);
                    }
        }
        buf = buf == NBUF - 1 ? 0 : buf + 1;
    }
    // requests for tiles past the end (zero range) must land before the LDS can go to another workgroup
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- partial result of this key range: un-normalised accumulator + (m, l) per row
    float* po = p.part_o + ((int64_t)bk * p.nsplit + split) * p.R * D;
    float* pml = p.part_ml + ((int64_t)bk * p.nsplit + split) * p.R * 2;
    const float l_tot = sum_across_halves(l_run);
    if (row_ok) {
        if (hi == 0) {
            pml[row * 2] = m_run;
            pml[row * 2 + 1] = l_tot;
        }
#pragma unroll
        for (int d = 0; d < DB; ++d)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                f32x4 x;
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = oacc[d][4 * gq + e];
                *reinterpret_cast<f32x4*>(po + (int64_t)row * D + d * 32 + 8 * gq + 4 * hi) = x;
            }
    }
}

// Merge the partials of a row (the arithmetic of fasn_fwd_combine_kernel: m* = max_s m_s, l = sum_s l_s 2^(m_s - m*),
// O = sum_s acc_s 2^(m_s - m*) / l) and scatter it: row r of (b, hkv) is o[b, hkv * G + r / Sq, r % Sq, :]. One thread per (row, 4 features).
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvcache_combine_kernel(const KvParams p) {
    using E = ET<Tag>;
    constexpr int TPR = D / 4;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rowg = gid / TPR;   // (b * Hkv + hkv, r)
    const int c4 = (int)(gid % TPR) * 4;
    if (rowg >= (int64_t)p.B * p.Hkv * p.R) return;
    const int bk = (int)(rowg / p.R), r = (int)(rowg % p.R);
    const int b = bk / p.Hkv, h = (bk % p.Hkv) * p.G + r / p.Sq, pos = r % p.Sq;
    float mstar = -INFINITY;
    for (int s = 0; s < p.nsplit; ++s) mstar = fmaxf(mstar, p.part_ml[(((int64_t)bk * p.nsplit + s) * p.R + r) * 2]);
    const float m_use = (mstar == -INFINITY) ? 0.f : mstar;
    float l = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < p.nsplit; ++s) {
        const int64_t base = ((int64_t)bk * p.nsplit + s) * p.R + r;
        const float ms = p.part_ml[base * 2], ls = p.part_ml[base * 2 + 1];
        if (ms == -INFINITY) continue;   // an empty or fully hidden range: nothing to add
        const float w = fast_exp2(ms - m_use);
        l += ls * w;
        const f32x4 a = *reinterpret_cast<const f32x4*>(p.part_o + base * D + c4);
        acc += a * w;
    }
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    typename E::vec4 y = E::cvt4(acc * inv);
    u32x2 raw;
    __builtin_memcpy(&raw, &y, 8);
    gstore8(p.o + (b * p.os[0] + h * p.os[1] + (int64_t)pos * p.os[2] + c4) * 2, raw);
    if (p.lse != nullptr && c4 == 0) p.lse[((int64_t)b * p.H + h) * p.Sq + pos] = l > 0.f ? (m_use + __builtin_log2f(l)) * kLn2 : -INFINITY;
}

// k_new / v_new row i of (b, hkv) -> cache row seqlens[b] + i, 16 bytes per thread and tensor. Rows that would land at or beyond the
// capacity (or at a negative position) are dropped here: the host does not know the lengths.
template <int D>
__global__ void __launch_bounds__(256) fasn_kvcache_append_kernel(const KvParams p) {
    constexpr int CPR = D / 8;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)p.B * p.Hkv * p.Sq * CPR) return;
    const int ch = (int)(gid % CPR);
    int64_t rest = gid / CPR;
    const int i = (int)(rest % p.Sq);
    rest /= p.Sq;
    const int hkv = (int)(rest % p.Hkv), b = (int)(rest / p.Hkv);
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
