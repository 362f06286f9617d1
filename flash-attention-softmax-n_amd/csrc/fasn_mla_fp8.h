// fasn_mla_fp8.h — the MLA decode of fasn_mla.h over a latent cache of OCP e4m3fn codes with one fp32 scale per batch element in device
// memory. The semantics are the K/V-cache family's FP8 cache (fasn_kvfp8.h) reduced to the one tensor an MLA cache has:
//   value(code) = up(code) * kv_scale[b]                                      up() the exact upcast; every finite code is an fp16 AND a bf16 number
//   x_ij  = scale * kv_scale[b] * (q_i[0:576] . up(c_j[0:576]))               one fp32 factor on the scores behind the MFMAs
//   out_i = kv_scale[b] * sum_j p_ij up(c_j[0:512]) / (n + sum_j p_ij)        on the fp32 row in the combine, before its one rounding
// so the operands of the 16-bit MFMAs are the codes themselves; neither Q nor P is quantised. Three kernels, siblings of fasn_mla.h's:
//   fasn_mla_fp8_append_kernel    kv_new rows, quantised by kv_fp8_quant16 (fasn_kvfp8.h), -> code rows len_b .. len_b + Sq - 1
//   fasn_mla_fwd_fp8_kernel       the split-K walk; work item, wave roles, Q^T registers and the tile text (fasn_mla_tile.inc) are
//                                 fasn_mla_fwd_kernel's, as are the partials it writes
//   fasn_mla_fp8_combine_kernel   kv_merge / kv_store_row with kv_scale[b] / kv_lse
//
// What is new is the way of a tile from HBM to the MFMA operands. LDS, 144 KiB as before, one workgroup per CU:
//   [0, 36 KiB) [36, 72 KiB)   two CODE buffers: a tile as it lies in the cache, 64 rows of 576 bytes, linear, filled one tile ahead by
//                              2304 buffer_load_dwordx4 ... lds requests (9 per thread against the 16-bit tile's 18) under a descriptor
//                              that ends at len_b in bytes of the code rows - rows at or beyond len_b arrive as zeros, code 0x00 = +0
//   [72, 144 KiB)              ONE 16-bit tile image in exactly the layout mla_tile_off / mla_swz describe: the fragment reads of
//                              fasn_mla.h, their lane parts and their literal offsets run on it unchanged
// Two barriers per tile, as in the family's FP8 kernels: codes of tile t landed (and everybody is done with the image of tile t - 1), then
// all 256 threads widen tile t - image slot (row r, position c') takes the 8 codes of chunk c' ^ mla_swz(r), v_cvt_pk_f32_fp8 and E::cvt8,
// both exact - and the image is published. The widening is not overlapped with the MFMAs (no split image was built).
//
// Banks of the widening - an argument from the bank model of fasn_common.h, not a measurement; no counter was read. A wave fills the 64
// consecutive image slots 64 w' .. 64 w' + 63: 1024 contiguous bytes per ds_write_b128, whatever rows they span. 64 and 72 are multiples of
// 8, so the 64 slots are 8 whole groups of 8 chunk positions, the XOR permutes inside a group, and a row's codes end where the next row's
// begin (576-byte rows, linear): the wave's ds_read_b64 takes 512 contiguous bytes, permuted in 8-byte words - each half-wave 256
// contiguous bytes, every one of the 64 banks once. Rows r and r + 32 share mla_swz and lie 32 * 72 = 9 * 256 slots apart: thread tid widens
// the slots tid + 256 i and those + 2304 from one address computation each, 18 chunks per thread and tile.
#pragma once
#include "fasn_kvfp8.h"
#include "fasn_mla.h"

namespace fasn {

constexpr int MLA8_CODEB = KV_KT * MLA_E;            // staged codes of a tile: 36 KiB
constexpr int MLA8_IMG = 2 * MLA8_CODEB;             // where the 16-bit image begins
constexpr int MLA8_SMEM = MLA8_IMG + MLA_TILEB;      // 144 KiB
static_assert(MLA8_SMEM == MLA_SMEM, "the FP8 sibling keeps the 16-bit kernel's LDS size");

struct MlaFp8 {
    const float* ks;     // kv_scale, device
    int64_t sb;          // its batch stride (0 broadcasts)
};

// codes / img: LDS addresses of a code buffer and of the image
template <typename E>
FASN_DEV void mla_fp8_widen(uint32_t codes, uint32_t img, int tid) {
    constexpr int HALF = (KV_KT / 2) * MLA_CPR;   // 2304 slots: 32 rows
#pragma unroll
    for (int i = 0; i < HALF / 256; ++i) {
        const int ci = tid + i * 256;
        const int r = ci / MLA_CPR, cp = ci - r * MLA_CPR;
        const uint32_t src = codes + r * MLA_E + ((cp ^ mla_swz(r)) << 3);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {   // row r, then row r + 32 (the same swizzle)
            const u32x2 raw = *LDS_PTR(const u32x2, (uintptr_t)(src + hf * 32 * MLA_E));
            f32x8 x;
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], false), up = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], true);
                x[4 * w] = lo[0], x[4 * w + 1] = lo[1], x[4 * w + 2] = up[0], x[4 * w + 3] = up[1];
            }
            const typename E::vec8 y = E::cvt8(x);
            u32x4 out;
            __builtin_memcpy(&out, &y, 16);
            *LDS_PTR(u32x4, (uintptr_t)(img + ci * 16 + hf * 32 * MLA_ROWB)) = out;
        }
    }
}

// p.kv points at codes; p.kps / p.krs count codes = bytes
template <typename Tag>
__global__ void __launch_bounds__(256, 1) fasn_mla_fwd_fp8_kernel(const MlaParams p, const MlaFp8 f8) {
    using E = ET<Tag>;
    using vec8 = typename E::vec8;
    constexpr bool PRESCALE = std::is_same<Tag, f16_tag>::value;
    constexpr int NT = 256;
    constexpr int KS = MLA_E / 16;                  // 36 k-steps of S^T
    constexpr int DBW = MLA_EV / 32 / 2;            // 8 feature blocks of O^T per wave
    constexpr int SCPR = MLA_E / 16;                // 36 requests of 16 codes per staged row
    constexpr int NLD = (KV_KT * SCPR) / NT;        // 9 requests per thread and tile

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
    const bool wave_rows = rb * MLA_RB + rh * 32 < p.R;   // a wave without rows only helps staging and widening

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
        // kv_scale[b] acts on the fp32 scores: one uniform load in front of the tile loop, like n. fp16: the queries carry scale * log2(e)
        // already (prescaled and rounded once, as in fasn_mla_fwd_kernel), the factor is kv_scale[b]; bf16: scale * log2(e) * kv_scale[b]
        float sc = (PRESCALE ? 1.f : p.c) * f8.ks[(int64_t)b * f8.sb];
        // Q^T of the lane's row, as fasn_mla_fwd_kernel holds it: 36 fragments, the last 24 in accumulation registers
        vec8 qf[KS];
        {
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
#pragma unroll
            for (int s = KS - 24; s < KS; ++s) asm volatile("" : "+a"(qf[s]));
        }

        // ---- staging: thread tid requests the 16-code groups tid + i * 256 of the tile, which land where they lie in the cache row (the
        // widening pass applies the swizzle). The offsets are recomputed per tile from an opaque copy of tid, as in fasn_mla_fwd_kernel.
        const int krs = (int)p.krs;
        const uint32_t lds0 = lds_addr(smem);
        const uint32_t lds_w = lds0 + wave * 1024;
        // the lane parts of the fragment addresses (mla_lds_read16 / mla_lds_read_tr), inside the image
        uint32_t ka[4], va[2][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) ka[j] = lds0 + MLA8_IMG + mla_tile_off(l31, 2 * j + hi);
        {
            const int i = lane & 15, g1 = (lane >> 4) & 1;
            const int r0 = 4 * hi + (i >> 2), sub = ((4 * (i & 3)) & 7) * 2;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                va[e][0] = lds0 + MLA8_IMG + mla_tile_off(r0, e * 4 + g1 * 2 + ((i & 3) >> 1)) + sub + fh * (DBW / 2) * 128;
                va[e][1] = (va[e][0] ^ 32u) + 8 * MLA_ROWB;
            }
        }

        // the tile that is requested next: its index, page slot and tile inside the page advance together (no division in the loop)
        int u = t0;
        int u_slot = t0 / p.tpp;
        int u_tip = t0 - u_slot * p.tpp;
        // page ids by scalar loads through the constant address space; entries of tiles outside the range are never read
        const __attribute__((address_space(4))) int* const bt_row = (const __attribute__((address_space(4))) int*)(p.bt + (int64_t)b * p.bts);
        const bool paged = p.bt != nullptr;
        auto page_of = [&](int tile, int slot) -> int {
            if (tile >= t1) return 0;
            return paged ? bt_row[slot] : b;
        };
        int u_page = page_of(u, u_slot);
        auto request_next = [&](int cb) {
            const int nvis = u < t1 ? min(KV_KT, len - u * KV_KT) : 0;   // rows of the tile below len_b (>= 1 inside the range)
            const int64_t off = (int64_t)u_page * p.kps + (int64_t)u_tip * KV_KT * p.krs;
            const uint32_t bytes = nvis > 0 ? (uint32_t)((nvis - 1) * krs + MLA_E) : 0u;
            const u32x4 rw = make_rsrc_words(p.kv + off, bytes);
            int tid_o = tid;
            asm volatile("" : "+v"(tid_o));
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int ci = tid_o + i * NT;
                const int r = ci / SCPR, ch = ci - r * SCPR;
                kv_dma16(rw, __builtin_amdgcn_readfirstlane(lds_w + cb * MLA8_CODEB + i * NT * 16), (unsigned)(r * krs + ch * 16));
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
        retire_loads(n_row);
        retire_loads(sc);

        // ---- the code buffers and the image start as zeros: a request that is out of range for its descriptor must leave nothing behind
        // that is not a finite number, whether the hardware fills the slot with zeros or leaves it alone
        for (int i = tid; i < MLA8_SMEM / 16; i += NT) *LDS_PTR(u32x4, smem + i * 16) = u32x4{0u, 0u, 0u, 0u};
        __syncthreads();
        request_next(0);

        int cb = 0;
        for (int t = t0; t < t1; ++t) {
            // the codes of tile t have landed (this wave's share), then everybody's share has, and everybody is done with the image of tile
            // t - 1 and - widened before the second barrier, one tile ago - with the codes of tile t - 1, whose buffer takes the next request
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            request_next(cb ^ 1);
            // all four waves widen tile t, rows or not; then everybody's share of the image is there
            int tid_w = tid;
            asm volatile("" : "+v"(tid_w));
            mla_fp8_widen<E>(lds0 + cb * MLA8_CODEB, lds0 + MLA8_IMG, tid_w);
            __syncthreads();
            if (wave_rows) {
#define MLA_TILE_AT 0
#define MLA_SCORE(x) ((x) * sc)
#define MLA_TILE_ALL_VISIBLE (k0 + KV_KT - 1 <= all_vis)
#define MLA_KEY_VISIBLE(kb, r) (k0 + (kb) * 32 + ((r) & 3) + 8 * ((r) >> 2) + 4 * hi <= vis)
#include "fasn_mla_tile.inc"
#undef MLA_TILE_AT
#undef MLA_SCORE
#undef MLA_TILE_ALL_VISIBLE
#undef MLA_KEY_VISIBLE
            }
            cb ^= 1;
        }
        // the request for the tile past the end (zero range) must land before the LDS can go to another workgroup
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }

    // ---- partial result of this key range, as fasn_mla_fwd_kernel writes it (kv_scale[b] is the combine's)
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

// fasn_mla_combine_kernel with kv_scale[b] on the normalised fp32 row, in front of its one rounding
template <typename Tag>
__global__ void __launch_bounds__(256) fasn_mla_fp8_combine_kernel(const MlaParams p, const MlaFp8 f8) {
    using E = ET<Tag>;
    constexpr int TPR = MLA_EV / 4;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rowg = gid / TPR;   // (b, r)
    const int c4 = (int)(gid % TPR) * 4;
    if (rowg >= (int64_t)p.B * p.R) return;
    const int b = (int)(rowg / p.R), r = (int)(rowg % p.R);
    const int h = r / p.Sq, pos = r % p.Sq;
    const KvMerged m = kv_merge<MLA_EV>(c4, p.part_o, p.part_ml, p.nsplit, [&](int s) { return ((int64_t)b * p.nsplit + s) * p.R + r; });
    kv_store_row<E>(p.o + (b * p.os[0] + h * p.os[1] + (int64_t)pos * p.os[2] + c4) * 2, m, f8.ks[(int64_t)b * f8.sb]);
    if (p.lse != nullptr && c4 == 0) p.lse[((int64_t)b * p.H + h) * p.Sq + pos] = kv_lse(m);
}

// kv_new row i of batch element b, quantised as fasn_kvcache_fp8_append quantises k_new, -> code row seqlens[b] + i: 16 elements in, 16 codes
// (one 16-byte store) out per thread. The drop rule is fasn_mla_append_kernel's.
template <typename Tag>
__global__ void __launch_bounds__(256) fasn_mla_fp8_append_kernel(const MlaParams p, const MlaFp8 f8) {
    using E = ET<Tag>;
    constexpr int CPR = MLA_E / 16;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)p.B * p.Sq * CPR) return;
    const int ch = (int)(gid % CPR);
    const int64_t rest = gid / CPR;
    const int i = (int)(rest % p.Sq), b = (int)(rest / p.Sq);
    const int64_t key = (int64_t)p.seqlens[b] + i;
    if (key < 0 || key >= p.capacity) return;
    const int slot = (int)(key / p.page_size), rip = (int)(key % p.page_size);
    const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
    const u32x4 x = kv_fp8_quant16<E>(p.kn + (b * p.kns[0] + (int64_t)i * p.kns[1]) * 2 + ch * 32, f8.ks[(int64_t)b * f8.sb]);
    gstore16(p.kv + page * p.kps + (int64_t)rip * p.krs + ch * 16, x);
}

}  // namespace fasn
