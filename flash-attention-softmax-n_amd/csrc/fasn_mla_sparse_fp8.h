// fasn_mla_sparse_fp8.h — the sparse MLA decode of fasn_mla_sparse.h over the FP8 latent cache the top-k models are served from. One cache
// row is 656 bytes:
//   [0, 512)     OCP e4m3fn codes of latent features 0 .. 511
//   [512, 528)   four fp32 scales, scale g for features 128 g .. 128 g + 127
//   [528, 656)   the 64 rotated key features as 16-bit numbers in the query's dtype, not quantised
// and the value of latent feature f is rn_T(float(up(code[f])) * scale[f / 128]): one fp32 multiply, one rounding (RNE) to the query's
// dtype T - dequantise to 16 bits, then attend. From there on every bit is fasn_mla_sparse_fwd_kernel's on the 576-feature row
// [latent | rope]: the work item (batch element, position, 64-head block, split), the wave roles, Q^T in registers, the three-tile-deep
// chain entry -> page id -> address with its ballot key mask and dead-tile skip, the lane-mask visibility hook, the tile text
// (fasn_mla_tile.inc), the partials and fasn_mla_combine_kernel. Two kernels:
//   fasn_mla_sparse_fp8_append_kernel   kv_new rows (16-bit), quantised per group of 128 features, -> 656-byte rows len_b .. len_b + Sq - 1
//   fasn_mla_sparse_fp8_fwd_kernel      the gathering split walk
//
// What is new is the way of a tile from HBM to the MFMA operands. LDS, 157696 of the CU's 163840 bytes, one workgroup per CU, all zeros
// at the start:
//   [0, 41984) [41984, 83968)   two BYTE buffers: the tile's 64 rows as they lie in the cache, 656 bytes each, linear, filled one tile ahead
//   [83968, 157696)             ONE 16-bit image in exactly the mla_tile_off / mla_swz layout: the fragment reads run on it unchanged
// Two barriers per live tile, as in fasn_mla_fwd_fp8_kernel: bytes landed and the old image free; then all 256 threads widen and the image
// is published. A tile whose key mask is 0 issues no request, is not widened and meets the first barrier only.
//
// Gathered staging, ONE ROW PER REQUEST. A row is 41 chunks of 16 bytes; 64 x 41 = 2624 chunks are no multiple of 256, and the 16-bit
// kernel's slot = tid + i * 256 would let a wave's request span three rows (64 > 41). Here wave w stages rows 16 w .. 16 w + 15: the row's
// 64-bit address comes from its owning lane into an SGPR pair (two v_readlane), lanes 0 .. 40 issue global_load_lds_dwordx4 with that
// scalar base and the offset 16 * lane under exec, LDS base r * 656 in M0 - the slot follows the lane id, so the row lands linearly. 16
// requests per wave and tile, no select, and a row that is no key is skipped by a wave-uniform branch: it is not read, and its 656 bytes
// keep what they held - zeros from the start (code 0 times scale 0 = 0), an earlier finite row later -, which a weight of exactly 0 turns
// into 0.
//
// Widening, 18 image slots per thread and tile, rows r and r + 32 (equal mla_swz) from one address computation:
//   latent   8 passes: wave w' takes row r = w' + 4 i, lane L image position L: the 8 codes of chunk L ^ mla_swz(r) (ds_read_b64), the
//            scale of group L >> 4 - the XOR stays inside 8 chunks, so the group of a slot is that of its position - as one ds_read_b32 at
//            r * 656 + 512 + 4 (L >> 4), v_cvt_pk_f32_fp8, eight fp32 multiplies, E::cvt8, one ds_write_b128
//   rope     1 pass: thread tid takes row tid >> 3, position 64 + (tid & 7): the 16 bytes of rope chunk (tid & 7) ^ mla_swz(r), copied
// Banks - an argument on the bank model of fasn_common.h (bank = (addr / 4) mod 64), not a measurement; no counter was read. Latent pass:
// a wave touches ONE row per instruction, so the 656-byte pitch (164 dwords: consecutive rows start 36 banks apart) never meets itself;
// the ds_read_b64 takes the row's 512 contiguous code bytes permuted in 8-byte words inside 64-byte groups - each half-wave 256 contiguous
// bytes, every bank once -, the ds_write_b128 1024 contiguous bytes, the scale read 4 addresses (a broadcast each). Rope pass: 8 lanes
// read the 128 contiguous rope bytes of a row, permuted in 16-byte chunks; a 16-lane service group holds two rows 36 banks apart, whose
// 32-bank spans share 4 banks - one chunk in eight meets a second access; one pass in nine.
#pragma once
#include "fasn_mla_sparse.h"

namespace fasn {

constexpr int MLA8S_ROWB = 656;                       // bytes of a cache row
constexpr int MLA8S_CPR = MLA8S_ROWB / 16;            // its 16-byte chunks: 41
constexpr int MLA8S_SCALE_AT = MLA_EV;                // the four scales
constexpr int MLA8S_ROPE_AT = MLA_EV + 16;            // the 16-bit rotated part
constexpr int MLA8S_GROUP = 128;                      // latent features per scale
constexpr int MLA8S_BYTEB = KV_KT * MLA8S_ROWB;       // a staged tile: 41984
constexpr int MLA8S_IMG = 2 * MLA8S_BYTEB;            // where the 16-bit image begins
constexpr int MLA8S_SMEM = MLA8S_IMG + MLA_TILEB;     // 157696
static_assert(MLA8S_CPR * 16 == MLA8S_ROWB && MLA8S_ROPE_AT + (MLA_E - MLA_EV) * 2 == MLA8S_ROWB, "the 656-byte row");
static_assert(MLA8S_IMG % 256 == 0 && MLA8S_SMEM <= 160 * 1024, "the image starts on a bank row; one workgroup per CU");
constexpr int MLA8S_EMIN = -30, MLA8S_EMAX = 120;     // the exponents a group's scale 2^e takes

// 16 bytes per live lane from row + off into LDS slot lds_base + 16 * lane id: the scalar-base form, one row per request. `row` has just
// left a v_readlane: a VMEM instruction that reads an SGPR a VALU instruction wrote wants 5 wait states, and the compiler's hazard pass
// does not look into this text - the s_nop 4 serves that and the one wait state between the M0 write and the LDS-DMA
FASN_DEV void mla_gather_row16(uint32_t lds_base, uint64_t row, uint32_t off) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_base), "v"(off), "s"(row) : "memory", "m0");
}

template <typename E>
FASN_DEV u32x4 mla_fp8_dequant8(u32x2 raw, float s) {
    f32x8 x;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], false), up = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], true);
        x[4 * w] = lo[0], x[4 * w + 1] = lo[1], x[4 * w + 2] = up[0], x[4 * w + 3] = up[1];
    }
    const typename E::vec8 y = E::cvt8(x * s);   // one fp32 multiply, one rounding to the element type
    u32x4 out;
    __builtin_memcpy(&out, &y, 16);
    return out;
}

// bytes / img: LDS addresses of a byte buffer and of the image; wave is uniform
template <typename E>
FASN_DEV void mla_sparse_fp8_widen(uint32_t bytes, uint32_t img, int wave, int lane, int tid) {
    constexpr int HB = (KV_KT / 2) * MLA8S_ROWB, HI = (KV_KT / 2) * MLA_ROWB;   // rows r and r + 32
#pragma unroll
    for (int i = 0; i < KV_KT / 2 / 4; ++i) {
        const int r = wave + 4 * i;
        const uint32_t src = bytes + r * MLA8S_ROWB + ((lane ^ mla_swz(r)) << 3);
        const uint32_t sca = bytes + r * MLA8S_ROWB + MLA8S_SCALE_AT + ((lane >> 4) << 2);
        const uint32_t dst = img + r * MLA_ROWB + (lane << 4);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const u32x2 raw = *LDS_PTR(const u32x2, (uintptr_t)(src + hf * HB));
            const float s = *LDS_PTR(const float, (uintptr_t)(sca + hf * HB));
            *LDS_PTR(u32x4, (uintptr_t)(dst + hf * HI)) = mla_fp8_dequant8<E>(raw, s);
        }
    }
    {
        const int r = tid >> 3, c = tid & 7;
        const uint32_t src = bytes + r * MLA8S_ROWB + MLA8S_ROPE_AT + ((c ^ mla_swz(r)) << 4);
        const uint32_t dst = img + r * MLA_ROWB + ((MLA_EV / 8 + c) << 4);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) *LDS_PTR(u32x4, (uintptr_t)(dst + hf * HI)) = *LDS_PTR(const u32x4, (uintptr_t)(src + hf * HB));
    }
}

// p.kv points at bytes; p.kps / p.krs count bytes
template <typename Tag>
__global__ void __launch_bounds__(256, 1) fasn_mla_sparse_fp8_fwd_kernel(const MlaParams p, const MlaSparse sp) {
    using E = ET<Tag>;
    using vec8 = typename E::vec8;
    constexpr bool PRESCALE = std::is_same<Tag, f16_tag>::value;
    constexpr int NT = 256;
    constexpr int KS = MLA_E / 16;
    constexpr int DBW = MLA_EV / 32 / 2;
    constexpr int RPW = KV_KT / 4;   // rows a wave stages

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int hi = lane >> 5;
    const int rh = wave & 1, fh = wave >> 1;

    // ---- the work item: (b, pos, head block, split), all wave-uniform
    const int wg = (int)blockIdx.x;
    const int split = wg % p.nsplit;
    int rest = wg / p.nsplit;
    const int hb = rest % sp.nhb;
    rest /= sp.nhb;
    const int pos = rest % p.Sq;
    const int b = rest / p.Sq;

    const int len = mla_len(p, b);
    const int t0 = min(split * sp.tps, sp.ntiles);
    const int t1 = min(t0 + sp.tps, sp.ntiles);
    const int lim = p.causal ? min(len - 1, pos + len - p.Sq) : len - 1;

    // ---- the lane's row: a head of position pos
    const int head = hb * MLA_RB + rh * 32 + l31;
    const bool row_ok = head < p.H;
    const int h = row_ok ? head : 0;
    const int row = h * p.Sq + pos;                       // partial row (dense layout)
    float n_row = p.n;
    if (p.nt != nullptr) n_row = p.nt[b * p.nsb + h * p.nsh];
    const bool wave_rows = hb * MLA_RB + rh * 32 < p.H;   // a wave without rows only helps staging and widening

    const bool sink = n_row > 0.f && split == 0;
    float m_run = sink ? 0.f : -INFINITY;
    float l_run = (sink && hi == 0) ? n_row : 0.f;
    f32x16 oacc[DBW];
#pragma unroll
    for (int d = 0; d < DBW; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;

    if (t0 < t1 && lim >= 0) {   // (uniform over the workgroup; lim < 0: no entry can be a key, nothing is read)
        // ---- the chain's first three tiles (fasn_mla_sparse_fwd_kernel's chain, addresses in bytes)
        const int* const idx_row = sp.idx + b * sp.sb + (int64_t)pos * sp.sq;
        const int* const bt_row = p.bt + (int64_t)b * p.bts;
        const bool paged = p.bt != nullptr;
        auto load_idx = [&](int tile) __attribute__((always_inline)) -> int { return tile < t1 ? idx_row[tile * KV_KT + fresh_lane_id()] : -1; };
        auto resolve = [&](int j, bool& ok, int& rip, int& page) __attribute__((always_inline)) {
            ok = j >= 0 && j <= lim;
            rip = 0, page = 0;
            if (ok) {
                if (paged) {
                    int slot = (int)__umulhi((uint32_t)j, sp.ps_magic);
                    rip = j - slot * p.page_size;
                    if (rip >= p.page_size) ++slot, rip -= p.page_size;
                    page = bt_row[slot];
                } else {
                    rip = j, page = b;
                }
            }
        };
        auto row_addr = [&](int page, int rip) __attribute__((always_inline)) -> const char* { return p.kv + ((int64_t)page * p.kps + (int64_t)rip * p.krs); };

        uint64_t mask0, mask1, mask2;     // key masks of tiles t, t + 1, t + 2
        const char* addr1;                // row address of the lane's entry of tile t + 1
        int rip2, page2, idx3;            // tile t + 2's row in its page and page id (arriving), tile t + 3's entry (arriving)
        const char* addr0;
        {
            const int j0 = load_idx(t0), j1 = load_idx(t0 + 1), j2 = load_idx(t0 + 2);
            bool ok0, ok1, ok2;
            int rip0, page0, rip1, page1;
            resolve(j0, ok0, rip0, page0);
            resolve(j1, ok1, rip1, page1);
            resolve(j2, ok2, rip2, page2);
            idx3 = load_idx(t0 + 3);
            mask0 = __ballot(ok0), mask1 = __ballot(ok1), mask2 = __ballot(ok2);
            addr0 = row_addr(page0, rip0);
            addr1 = row_addr(page1, rip1);
        }

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

        const uint32_t lds0 = lds_addr(smem);
        // the lane parts of the fragment addresses, inside the image
        uint32_t ka[4], va[2][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) ka[j] = lds0 + MLA8S_IMG + mla_tile_off(l31, 2 * j + hi);
        {
            const int i = lane & 15, g1 = (lane >> 4) & 1;
            const int r0 = 4 * hi + (i >> 2), sub = ((4 * (i & 3)) & 7) * 2;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                va[e][0] = lds0 + MLA8S_IMG + mla_tile_off(r0, e * 4 + g1 * 2 + ((i & 3) >> 1)) + sub + fh * (DBW / 2) * 128;
                va[e][1] = (va[e][0] ^ 32u) + 8 * MLA_ROWB;
            }
        }

        // ---- the requests of one tile: `a` the lane's entry's row address, `mask` the tile's key mask. This wave's rows are
        // 16 wave .. 16 wave + 15; a live row's address leaves its lane for an SGPR pair and 41 lanes fetch its 41 chunks
        auto request = [&](int cb, const char* a, uint64_t mask) __attribute__((always_inline)) {
            if (mask == 0) return;   // (uniform)
            const uint32_t a_lo = (uint32_t)(uintptr_t)a, a_hi = (uint32_t)((uintptr_t)a >> 32);
            const int ln = fresh_lane_id();
            const uint32_t off = (uint32_t)ln * 16u;
            const uint32_t dst0 = lds0 + cb * MLA8S_BYTEB + wave * (RPW * MLA8S_ROWB);
#pragma unroll
            for (int i = 0; i < RPW; ++i) {
                const int r = wave * RPW + i;
                if ((mask >> r) & 1) {   // (uniform: a row that is no key is not read)
                    // (the builtin returns a signed int: without the casts the low word's bit 31 is smeared over the high word)
                    const uint64_t s = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(a_hi, r) << 32) | (uint32_t)__builtin_amdgcn_readlane(a_lo, r);
                    if (ln < MLA8S_CPR) mla_gather_row16(__builtin_amdgcn_readfirstlane(dst0 + i * MLA8S_ROWB), s, off);
                }
            }
        };

        retire_loads(n_row);

        for (int i = tid; i < MLA8S_SMEM / 16; i += NT) *LDS_PTR(u32x4, smem + i * 16) = u32x4{0u, 0u, 0u, 0u};
        __syncthreads();
        request(0, addr0, mask0);

        int cb = 0;
        for (int t = t0; t < t1; ++t) {
            // tile t's bytes have landed (this wave's share), and with them the page ids of tile t + 2 and the entries of tile t + 3
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("" : "+v"(page2), "+v"(idx3));
            const char* const addr2 = row_addr(page2, rip2);
            bool ok3;
            int rip3, page3;
            resolve(idx3, ok3, rip3, page3);
            const uint64_t mask3 = __ballot(ok3);
            const int idx4 = load_idx(t + 4);
            // everybody's share has landed, and everybody is done with the image of the tile before and - widened one tile ago - with the
            // other byte buffer, which takes the next request
            __syncthreads();
            request(cb ^ 1, addr1, mask1);
            if (mask0 != 0) {   // (uniform over the workgroup: a dead tile is neither widened nor multiplied, and meets no second barrier)
                int tid_w = tid;
                asm volatile("" : "+v"(tid_w));
                mla_sparse_fp8_widen<E>(lds0 + cb * MLA8S_BYTEB, lds0 + MLA8S_IMG, wave, tid_w & 63, tid_w);
                __syncthreads();
                if (wave_rows) {
#define MLA_TILE_AT 0
#define MLA_SCORE(x) (PRESCALE ? (x) : (x) * p.c)
#define MLA_TILE_ALL_VISIBLE false
#define MLA_KEY_VISIBLE(kb, r) mla_key_lanes(mask0, (kb) * 32 + ((r) & 3) + 8 * ((r) >> 2))
#include "fasn_mla_tile.inc"
#undef MLA_TILE_AT
#undef MLA_SCORE
#undef MLA_TILE_ALL_VISIBLE
#undef MLA_KEY_VISIBLE
                }
            }
            cb ^= 1;
            mask0 = mask1, mask1 = mask2, mask2 = mask3;
            addr1 = addr2;
            rip2 = rip3, page2 = page3, idx3 = idx4;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }

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

// max over the 16 lanes of a DPP row: xor 1, xor 2 (quad_perm), row_half_mirror, row_mirror; every lane ends with the row's maximum
FASN_DEV float mla_max_row16(float x) {
#define FASN_DPP_MAX(ctrl) x = fmaxf(x, __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), ctrl, 0xf, 0xf, true)))
    FASN_DPP_MAX(0xB1);
    FASN_DPP_MAX(0x4E);
    FASN_DPP_MAX(0x141);
    FASN_DPP_MAX(0x140);
#undef FASN_DPP_MAX
    return x;
}

// The exponent of a group's scale 2^e from its amax a >= 0 (finite): the smallest e with a <= 448 * 2^e = 1.75 * 2^(e + 8), read from
// a's exponent and mantissa bits: a = m * 2^E with 1 <= m < 2 gives e = E - 8, one more where m > 1.75. a = 0 and the subnormals of
// fp32 (biased exponent 0) fall to the lower clamp.
FASN_DEV int mla_fp8_scale_exp(float a) {
    const uint32_t bits = __float_as_uint(a);
    const int e = (int)(bits >> 23) - 127 - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
    return min(max(e, MLA8S_EMIN), MLA8S_EMAX);
}

// kv_new row i of batch element b -> the 656-byte row seqlens[b] + i, one wave per row: lane l quantises latent features 8 l .. 8 l + 7
// (16 bytes in, 8 codes out), the amax of a group of 128 features is reduced over its 16 lanes by DPP, one lane per group stores the
// scale, eight lanes copy the rotated part bit for bit. code = rne_e4m3(clamp(x / 2^e, -448, 448)) - the division is an exact v_ldexp,
// +-Inf clamps, a NaN falls through the clamp and gives the NaN code 0x7f; the amax is over the finite elements. The drop rule is
// fasn_mla_append_kernel's. Vector stores only.
template <typename Tag>
__global__ void __launch_bounds__(256) fasn_mla_sparse_fp8_append_kernel(const MlaParams p) {
    using E = ET<Tag>;
    const int lane = threadIdx.x & 63;
    const int64_t rowi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rowi >= (int64_t)p.B * p.Sq) return;
    const int i = (int)(rowi % p.Sq), b = (int)(rowi / p.Sq);
    const int64_t key = (int64_t)p.seqlens[b] + i;
    if (key < 0 || key >= p.capacity) return;
    const int slot = (int)(key / p.page_size), rip = (int)(key % p.page_size);
    const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
    const char* const src = p.kn + (b * p.kns[0] + (int64_t)i * p.kns[1]) * 2;
    char* const dst = p.kv + page * p.kps + (int64_t)rip * p.krs;

    const u32x4 raw = gload16(src + lane * 16);
    float x[8], a = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        x[2 * w] = E::to_f32((uint16_t)(raw[w] & 0xffffu));
        x[2 * w + 1] = E::to_f32((uint16_t)(raw[w] >> 16));
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf(x[j]) < INFINITY ? fabsf(x[j]) : 0.f);   // (a NaN fails the comparison)
    const int e = mla_fp8_scale_exp(mla_max_row16(a));
    u32x2 out;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = __builtin_ldexpf(x[4 * w + j], -e);
            y[j] = v > 448.f ? 448.f : (v < -448.f ? -448.f : v);
        }
        int pk = 0;
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], pk, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], pk, true);
        uint32_t c = (uint32_t)pk;
#pragma unroll
        for (int j = 0; j < 4; ++j)   // THE NaN code is 0x7f whatever the NaN's sign (the conversion hands out 0xff as well)
            if (y[j] != y[j]) c = (c & ~(0xffu << (8 * j))) | (0x7fu << (8 * j));
        out[w] = c;
    }
    gstore8(dst + lane * 8, out);
    if ((lane & 15) == 0) *reinterpret_cast<float*>(dst + MLA8S_SCALE_AT + (lane >> 4) * 4) = __uint_as_float((uint32_t)(e + 127) << 23);
    if (lane < (MLA_E - MLA_EV) / 8) gstore16(dst + MLA8S_ROPE_AT + lane * 16, gload16(src + MLA_EV * 2 + lane * 16));
}

}  // namespace fasn
