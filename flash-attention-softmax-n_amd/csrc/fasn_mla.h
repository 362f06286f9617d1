// fasn_mla.h — decode over a compressed latent K/V cache (multi-head latent attention in its absorbed form: DeepSeek-V2 / V3 / R1, Kimi K2).
//
// One cache row per token, shared by every query head: 576 features = a 512-wide latent and a 64-wide rotated key part. The logit of head
// h is q_h[0:576] . row[0:576], the value is the latent itself: out_h = sum_j p_hj row_j[0:512] - multi-query attention with one K/V head,
// E = 576, Ev = 512 and V aliased onto K's first 512 features. Three kernels, none shared with the K/V-cache family's texts:
//   fasn_mla_append_kernel    kv_new rows -> cache rows len_b .. len_b + Sq - 1 (dropped beyond the capacity)
//   fasn_mla_fwd_kernel       split-K walk over the pages of one (batch element, 64-row block): un-normalised partials
//   fasn_mla_combine_kernel   kv_merge / kv_store_row / kv_lse of fasn_kvcache.h over the partials, rows back to o[b, h, pos, :]
//
// Rows. R = H * Sq rows, row r = h * Sq + pos; a work item is (batch element, 64-row block, key split), a workgroup of four waves.
//
// ONE LDS image per 64-key tile serves both products: [64][576] 16-bit rows = 72 KiB, two buffers (144 KiB of the CU's 160), filled by
// buffer_load_dwordx4 ... lds one tile ahead, one barrier per tile. The cache row is read from HBM once and from LDS in two patterns:
// ds_read_b128 along the features for S^T = K Q^T (all 576), ds_read_b64_tr_b16 along the keys for O^T += V^T P^T (features 0 .. 511 only:
// the rotated part never reaches a value).
//
// The image's swizzle. A row is 72 chunks of 16 bytes - 4.5 bank rows, so row r starts at bank 32 (r & 1) - and 72 is no power of two:
// chunk' = chunk ^ f(row) with f < 8 stays inside a group of 8 chunks (72 = 9 groups). f(row) = (bit1(row) << 2) | bits 3:2 of row:
//   (1) ds_read_b128, one chunk index, 16 rows per service group (lanes {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}): the 16-byte bank slot
//       is (8 (r & 1) + (c & 8)) mod 16 + ((c & 7) ^ f(r)); (r & 1, f(r)) is r mod 16 bit by bit, and a service group's rows are distinct
//       mod 16: 16 slots, 64 banks;
//   (2) ds_read_b64_tr_b16, 4 consecutive rows x 4 consecutive chunks (aligned) per half-wave: bits 3:2 of the row are common, rows 0 / 1
//       and 2 / 3 differ in the slot's bit 3, rows {0, 1} and {2, 3} in bit 2 (through f): 16 slots, 64 banks.
// This is the bank model the family's tile image is built on (fasn_common.h); no bank-conflict counter was read for this image.
//
// The four waves. Wave w takes row half w & 1 (32 rows, one lane per row: the online softmax stays in the lane, as in fasn_kvcache.h) and
// value-feature half w >> 1 (256 of the 512 output features). Both waves of a row half compute the same S^T over the whole tile from the
// same Q^T fragments - 36 k-steps, 144 registers; in fp16 prescaled by scale * log2(e) and rounded once - so their (m, l)
// agree bit for bit with no exchange; P stays in registers as the B operand; each wave accumulates its 8 of the 16 O^T feature blocks
// (128 accumulator registers). The duplicated S^T makes the MFMA work (2 * 576 + 512) / (576 + 512) = 1.53 x the minimum.
//
// Lengths, splits and stale memory are the decode kernel's (fasn_kvcache.h): len_b is read in the kernel, split s walks the tiles
// [s * tps_b, (s + 1) * tps_b), an empty range writes the neutral partial (split 0: the sink state m = 0, l = n) and leaves before it
// touches LDS, page ids come by scalar loads, every tile has a buffer descriptor of its own that ends at len_b.
#pragma once
#include <type_traits>
#include "fasn_kvcache.h"

namespace fasn {

constexpr int MLA_E = 576;                    // features of a cache row and of a query
constexpr int MLA_EV = 512;                   // ... of which the first 512 are the value
constexpr int MLA_RB = 64;                    // rows of a workgroup
constexpr int MLA_MAX_ROWS = 256;             // H * Sq of a call
constexpr int MLA_ROWB = MLA_E * 2;           // bytes of a row of the tile image
constexpr int MLA_CPR = MLA_E / 8;            // its 16-byte chunks: 72
constexpr int MLA_TILEB = KV_KT * MLA_ROWB;   // 72 KiB
constexpr int MLA_SMEM = 2 * MLA_TILEB;
// The split rule is the decode plan's at one workgroup per CU (kv_split_target(256): ~512 workgroups). A split costs its partial - up to 64
// rows of 514 floats, written and read back: what 3.6 tiles move - next to its tiles: at least 8 tiles per split of a full cache when the
// row block is full, 4 below that.
constexpr int64_t mla_min_tps(int R) { return R >= MLA_RB ? 8 : 4; }
constexpr int64_t mla_nsplit(int64_t base, int64_t cap_tiles, int R) { return kv_nsplit(256, base, cap_tiles, mla_min_tps(R)); }

struct MlaParams {
    const char* q;
    char* o;
    float* lse;          // [B, H, Sq] or nullptr
    char* kv;            // the cache pool
    int64_t qs[3], os[3];             // element strides (batch, head, row)
    int64_t kps, krs;                 // cache element strides (page, row)
    const int* bt;       // block table [B][bts] or nullptr (dense: page = batch element)
    int64_t bts;
    const int* seqlens;  // [B], device
    int seqlen_add;
    int tpp;             // 64-key tiles per page (dense: no page ever ends)
    int page_size;
    int capacity;
    int B, H, Sq, R, nrb;             // R = H * Sq rows in nrb blocks of 64
    int causal;
    float c;             // scale * log2(e)
    float n;
    const float* nt;     // per-(batch, query head) softmax_n or nullptr
    int nsb, nsh;
    int nsplit;
    float* part_o;       // [B][nsplit][R][512]
    float* part_ml;      // [B][nsplit][R][2]
    // append
    const char* kn;
    int64_t kns[2];      // kv_new element strides (batch, row)
};

FASN_DEV int mla_len(const MlaParams& p, int b) {
    const int len = __builtin_amdgcn_readfirstlane(p.seqlens[b]) + p.seqlen_add;
    return min(max(len, 0), p.capacity);
}
FASN_DEV int mla_swz(int row) { return ((row & 2) << 1) | ((row >> 2) & 3); }
// byte offset of (row, 16-byte chunk) inside a tile image
FASN_DEV int mla_tile_off(int row, int chunk) { return row * MLA_ROWB + ((chunk ^ mla_swz(row)) << 4); }

// The fragment reads take their LDS address as lane part + compile-time literal, so that the literal rides in the instruction's offset field
// and the unrolled tile body keeps 8 address registers, not one per read. The XOR stays inside a group of 8 chunks (128 bytes) and rows
// are 9 groups long, so the group of a chunk and the row block of a read are plain byte offsets:
//   S^T  k-step s of key block kb reads chunk 2 s + hi of row kb * 32 + l31: lane part of (s & 3), literal kb * 32 rows + (s >> 2) groups;
//   O^T  feature block c of tile rows rbase + {4 hi + 0 .. 3} and those + 8 (lds_read_trfrag's lane map): lane part of (c & 1), literal
//        rbase rows + (c >> 1) groups; row + 8 flips bit 1 of f, which is bit 5 of an address whose other terms are multiples of 128.
template <typename V>
FASN_DEV V mla_lds_read16(uint32_t addr) {
    const u32x4 raw = *LDS_PTR(const u32x4, (uintptr_t)addr);
    V r;
    __builtin_memcpy(&r, &raw, 16);
    return r;
}
template <typename V>
FASN_DEV V mla_lds_read_tr(uint32_t a0, uint32_t a1) {
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, (uintptr_t)a0));
    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, (uintptr_t)a1));
    const s16x8 ab = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    V r;
    __builtin_memcpy(&r, &ab, 16);
    return r;
}

template <typename Tag>
__global__ void __launch_bounds__(256, 1) fasn_mla_fwd_kernel(const MlaParams p) {
    using E = ET<Tag>;
    using vec8 = typename E::vec8;
    constexpr bool PRESCALE = std::is_same<Tag, f16_tag>::value;
    constexpr int NT = 256;
    constexpr int KS = MLA_E / 16;                  // 36 k-steps of S^T
    constexpr int DBW = MLA_EV / 32 / 2;            // 8 feature blocks of O^T per wave
    constexpr int NLD = (KV_KT * MLA_CPR) / NT;     // 18 requests of 16 bytes per thread and tile

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int hi = lane >> 5;
    const int rh = wave & 1, fh = wave >> 1;   // row half, value-feature half

    const int wg = (int)blockIdx.x;
    const int split = wg % p.nsplit;
    const int bk = wg / p.nsplit;              // b * nrb + row block
    const int b = bk / p.nrb, rb = bk - b * p.nrb;

    // ---- this split's tile range, from the length in device memory
    const int len = mla_len(p, b);
    const int tiles_b = (len + KV_KT - 1) / KV_KT;
    const int tps = (tiles_b + p.nsplit - 1) / p.nsplit;
    const int t0 = min(split * tps, tiles_b);
    const int t1 = min(t0 + tps, tiles_b);

    // ---- the lane's row: query head, position, softmax_n, causal limit
    const int row = rb * MLA_RB + rh * 32 + l31;
    const bool row_ok = row < p.R;
    const int h = row_ok ? row / p.Sq : 0;
    const int pos = row_ok ? row - h * p.Sq : 0;
    float n_row = p.n;
    if (p.nt != nullptr) n_row = p.nt[b * p.nsb + h * p.nsh];
    const bool wave_rows = rb * MLA_RB + rh * 32 < p.R;   // a wave without rows only helps staging

    // ---- online-softmax state of the row (log2 domain); the sink (+n) belongs to split 0
    const bool sink = n_row > 0.f && split == 0;
    float m_run = sink ? 0.f : -INFINITY;
    float l_run = (sink && hi == 0) ? n_row : 0.f;   // the two half-lanes' partial sums are added at the end
    f32x16 oacc[DBW];
#pragma unroll
    for (int d = 0; d < DBW; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;

    if (t0 < t1) {   // (uniform over the workgroup)
        // Q^T of the lane's row. fp16: prescaled by scale * log2(e) and rounded once, so that the scores leave the MFMAs in the log2 domain
        // (the host refuses |scale * log2(e)| > 8 there). bf16: as it is - eight bits of mantissa under the factor cost the lse 1e-3 - and
        // the scores are scaled in fp32 behind the MFMAs, as in fasn_kvcache.h.
        vec8 qf[KS];
        {
            // (a lane without a row reads row (b, 0, 0) and drops it: 36 loads in flight, no branch between them)
            const char* rp = p.q + (b * p.qs[0] + h * p.qs[1] + (int64_t)pos * p.qs[2]) * 2 + hi * 16;
            u32x4 raw[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) raw[s] = gload16(rp + s * 32);
            const float cq = row_ok ? p.c : 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if (!row_ok) raw[s] = u32x4{0u, 0u, 0u, 0u};
                vec8 x;
                __builtin_memcpy(&x, &raw[s], 16);
                if constexpr (PRESCALE) qf[s] = E::cvt8(__builtin_convertvector(x, f32x8) * cq);
                else qf[s] = x;
            }
            // 144 query registers, 48 of scores and weights and the reads in flight do not fit the 256 vector registers: the last 24
            // fragments are handed over in accumulation registers, where an MFMA reads its B operand just as well (128 of the 256 hold O^T)
#pragma unroll
            for (int s = KS - 24; s < KS; ++s) asm volatile("" : "+a"(qf[s]));
        }

        // ---- staging: thread tid fills slots tid + i * 256 of the tile image (slot = 16 bytes; the chunk that belongs there after the swizzle).
        // The 18 offsets of a thread are recomputed per tile from an opaque copy of tid - a few VALU instructions under 104 MFMAs - because
        // kept across the loop they are 18 registers that the query fragments need.
        const int krs2 = (int)p.krs * 2;
        const uint32_t lds_w = lds_addr(smem) + wave * 1024;
        // the lane parts of the fragment addresses (mla_lds_read16 / mla_lds_read_tr)
        uint32_t ka[4], va[2][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) ka[j] = lds_addr(smem) + mla_tile_off(l31, 2 * j + hi);
        {
            const int i = lane & 15, g1 = (lane >> 4) & 1;
            const int r0 = 4 * hi + (i >> 2), sub = ((4 * (i & 3)) & 7) * 2;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                va[e][0] = lds_addr(smem) + mla_tile_off(r0, e * 4 + g1 * 2 + ((i & 3) >> 1)) + sub + fh * (DBW / 2) * 128;
                va[e][1] = (va[e][0] ^ 32u) + 8 * MLA_ROWB;
            }
        }

        // the tile that is requested next: its index, page slot and tile inside the page advance together (no division in the loop)
        int u = t0;
        int u_slot = t0 / p.tpp;
        int u_tip = t0 - u_slot * p.tpp;
        // page ids are wave-uniform and the table does not change while the kernel runs: scalar loads through the constant address space,
        // whose wait the compiler places at the next tile's request. Entries of tiles outside the range are never read.
        const __attribute__((address_space(4))) int* const bt_row = (const __attribute__((address_space(4))) int*)(p.bt + (int64_t)b * p.bts);
        const bool paged = p.bt != nullptr;
        auto page_of = [&](int tile, int slot) -> int {
            if (tile >= t1) return 0;
            return paged ? bt_row[slot] : b;
        };
        int u_page = page_of(u, u_slot);
        auto request_next = [&](int buf) {
            const int nvis = u < t1 ? min(KV_KT, len - u * KV_KT) : 0;   // rows of the tile below len_b (>= 1 inside the range)
            const int64_t off = ((int64_t)u_page * p.kps + (int64_t)u_tip * KV_KT * p.krs) * 2;
            const uint32_t bytes = nvis > 0 ? (uint32_t)((nvis - 1) * (int)p.krs * 2 + MLA_ROWB) : 0u;
            const u32x4 rw = make_rsrc_words(p.kv + off, bytes);
            int tid_o = tid;
            asm volatile("" : "+v"(tid_o));
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int ci = tid_o + i * NT;
                const int r = ci / MLA_CPR, ch = (ci - r * MLA_CPR) ^ mla_swz(r);
                kv_dma16(rw, __builtin_amdgcn_readfirstlane(lds_w + buf * MLA_TILEB + i * NT * 16), (unsigned)(r * krs2 + ch * 16));
            }
            ++u;
            if (++u_tip == p.tpp) {
                u_tip = 0;
                ++u_slot;
            }
            u_page = page_of(u, u_slot);   // the next tile's page id is on its way while this one's data is
        };

        const int vis = !row_ok ? -1 : (p.causal ? pos + len - p.Sq : len - 1);   // last visible key of the row
        const int all_vis = p.causal ? len - p.Sq : len - 1;                        // every row sees the keys up to here
        retire_loads(n_row);   // (the prescaling has consumed the query loads already)

        // ---- the tile buffers start as zeros: a request that is out of range for its descriptor must leave nothing behind that is not
        // a finite number, whether the hardware fills the slot with zeros or leaves it alone
        for (int i = tid; i < MLA_SMEM / 16; i += NT) *LDS_PTR(u32x4, smem + i * 16) = u32x4{0u, 0u, 0u, 0u};
        __syncthreads();
        request_next(0);

        int buf = 0;
        for (int t = t0; t < t1; ++t) {
            // tile t has landed (this wave's share), then everybody's share has, and everybody is done with tile t - 1, whose buffer takes
            // the next request
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            request_next(buf ^ 1);
            if (wave_rows) {
                // S^T, mask, softmax, O^T on the image in buffer `buf` (the text is shared with the FP8 sibling, fasn_mla_fp8.h)
#define MLA_TILE_AT (buf * MLA_TILEB)
#define MLA_SCORE(x) (PRESCALE ? (x) : (x) * p.c)
#define MLA_TILE_ALL_VISIBLE (k0 + KV_KT - 1 <= all_vis)
#define MLA_KEY_VISIBLE(kb, r) (k0 + (kb) * 32 + ((r) & 3) + 8 * ((r) >> 2) + 4 * hi <= vis)
#include "fasn_mla_tile.inc"
#undef MLA_TILE_AT
#undef MLA_SCORE
#undef MLA_TILE_ALL_VISIBLE
#undef MLA_KEY_VISIBLE
            }
            buf ^= 1;
        }
        // the request for the tile past the end (zero range) must land before the LDS can go to another workgroup
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }

    // ---- partial result of this key range: un-normalised accumulator + (m, l) per row; the wave of feature half 0 writes (m, l)
    float* po = p.part_o + ((int64_t)b * p.nsplit + split) * p.R * MLA_EV;
    float* pml = p.part_ml + ((int64_t)b * p.nsplit + split) * p.R * 2;
    const float l_tot = sum_across_halves(l_run);
    if (row_ok) {
        if (hi == 0 && fh == 0) {
            pml[row * 2] = m_run;
            pml[row * 2 + 1] = l_tot;
        }
#pragma unroll
        for (int d = 0; d < DBW; ++d)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                f32x4 x;
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = oacc[d][4 * gq + e];
                *reinterpret_cast<f32x4*>(po + (int64_t)row * MLA_EV + (fh * DBW + d) * 32 + 8 * gq + 4 * hi) = x;
            }
    }
}

// merges the partials of a row and scatters it back: row r of batch element b is o[b, r / Sq, r % Sq, :] / lse[b, h, pos]. One thread
// per (row, 4 features); the merge, the one rounding and the lse are the K/V-cache family's (fasn_kvcache.h).
template <typename Tag>
__global__ void __launch_bounds__(256) fasn_mla_combine_kernel(const MlaParams p) {
    using E = ET<Tag>;
    constexpr int TPR = MLA_EV / 4;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rowg = gid / TPR;   // (b, r)
    const int c4 = (int)(gid % TPR) * 4;
    if (rowg >= (int64_t)p.B * p.R) return;
    const int b = (int)(rowg / p.R), r = (int)(rowg % p.R);
    const int h = r / p.Sq, pos = r % p.Sq;
    const KvMerged m = kv_merge<MLA_EV>(c4, p.part_o, p.part_ml, p.nsplit, [&](int s) { return ((int64_t)b * p.nsplit + s) * p.R + r; });
    kv_store_row<E>(p.o + (b * p.os[0] + h * p.os[1] + (int64_t)pos * p.os[2] + c4) * 2, m);
    if (p.lse != nullptr && c4 == 0) p.lse[((int64_t)b * p.H + h) * p.Sq + pos] = kv_lse(m);
}

// kv_new row i of batch element b -> cache row seqlens[b] + i, 16 bytes per thread. Rows that would land at or beyond the capacity (or at
// a negative position) are dropped here: the host does not know the lengths.
__global__ void __launch_bounds__(256) fasn_mla_append_kernel(const MlaParams p) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)p.B * p.Sq * MLA_CPR) return;
    const int ch = (int)(gid % MLA_CPR);
    const int64_t rest = gid / MLA_CPR;
    const int i = (int)(rest % p.Sq), b = (int)(rest / p.Sq);
    const int64_t key = (int64_t)p.seqlens[b] + i;
    if (key < 0 || key >= p.capacity) return;
    const int slot = (int)(key / p.page_size), rip = (int)(key % p.page_size);
    const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
    const u32x4 x = gload16(p.kn + (b * p.kns[0] + (int64_t)i * p.kns[1]) * 2 + ch * 16);
    gstore16(p.kv + (page * p.kps + (int64_t)rip * p.krs) * 2 + ch * 16, x);
}

}  // namespace fasn
