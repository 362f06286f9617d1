// fasn_mla_sparse.h — MLA decode over the latent cache behind a TOP-K INDEX LIST (DeepSeek-V3.2's sparse attention and its successors): every
// query position attends to the cache rows its list names, int32 idx[b, pos, 0 .. topk), shared by all heads. Entry j is a key of position
// pos iff 0 <= j < len_b and (causal) j <= pos + len_b - Sq; every other value - -1 padding, stale positions, garbage - is no key, and no
// address is formed from it: neither its block-table slot nor its row is read.
//
// fasn_mla_sparse_fwd_kernel is a sibling of fasn_mla_fwd_kernel (fasn_mla.h): wave roles, Q^T registers, the LDS image with its swizzle,
// the double buffer with one barrier per tile, the tile text (fasn_mla_tile.inc), the partials' layout and the combine kernel are that
// kernel's. What differs:
//
// Work item = (batch element, query POSITION, 64-HEAD block, split): a workgroup's 64 rows are 64 heads of one position, so they share one
// list and one causal limit; lane row = head hb * 64 + rh * 32 + l31, partial row = h * Sq + pos (the dense layout: fasn_mla_combine_kernel
// is launched unchanged). Split s walks the index tiles [s * tps, (s + 1) * tps) of topk / 64, tps fixed on the host.
//
// A tile is 64 list entries, and lane L of EVERY wave owns entry L: one coalesced 256-byte load per wave, the visibility test in the lane,
// ballot() of it = the tile's 64-bit key mask in an SGPR pair, identical in the four waves. Only a lane that passes reads its block-table
// entry (a vector load under exec) and forms its row's 64-bit address - the pool may exceed 4 GiB. The chain entry -> page id -> address is
// three tiles deep and never waits on its own: at the top of iteration t (after the one s_waitcnt vmcnt(0) the tile wait needs anyway, in
// front of the barrier) the page ids of tile t + 2 and the entries of tile t + 3 have arrived beside tile t's rows; the addresses of t + 2
// are finished, the visibility of t + 3 is tested, its table loads and the entry load of t + 4 are issued - and behind the barrier the
// requests of tile t + 1 start from addresses that have been in registers for a whole tile. Five vector registers carry the chain.
//
// Gathered staging: thread tid still fills slots tid + i * 256 of the image. The 64 slots of a wave's request lie in at most two rows
// (64 < 72), r0 = the row of lane 0 and r0 + 1: two v_readlane pairs and a select hand every lane its row's address, the mask's bits r0 and
// r0 + 1 its liveness - no table in LDS. The request is global_load_lds_dwordx4 (per-lane 64-bit address, LDS base in M0, slot = lane id),
// issued under exec by the live lanes only: a row that is no key is not read, and its slots keep what they held - zeros from the start,
// finite cache data later -, which a weight of exactly 0 turns into 0. buffer_load ... lds would need a descriptor per row in SGPRs, two
// per request with an exec switch between them; the global form needs none and its address is the gather's natural currency.
//
// Mask by bit, skip by mask: a tile whose mask is 0 issues no request and runs no MFMA - a workgroup-uniform branch, so the -1 tail of a list
// costs one entry load per tile. In a live tile the key-visibility hook of the tile text is a LANE MASK built from two scalar bits of the
// key mask (the lane's keys are a literal + 4 * its half-wave): two s_bfe and one v_cndmask per score, no vector register. The
// "tile entirely visible" hook is constant false here: with both paths in the text the compiler holds the 32 scores twice across the
// branch and the kernel spills 9 to 13 registers into scratch, whose reload waits drain the row requests in flight; the one masked pass
// costs 32 v_cndmask under 104 MFMAs. 248 vector + 256 accumulation registers, no scratch.
#pragma once
#include "fasn_mla.h"

namespace fasn {

struct MlaSparse {
    const int* idx;      // [B, Sq, topk], device
    int64_t sb, sq;      // element strides (batch, position)
    int ntiles;          // topk / 64
    int tps;             // index tiles per split
    int nhb;             // 64-head blocks
    uint32_t ps_magic;   // floor(2^32 / page_size): a position's page slot is mulhi(j, magic) or one more (mla_build_sparse)
};

// 16 bytes per live lane from its own 64-bit address into LDS slot lds_base + 16 * lane id (M0 write -> LDS-DMA: one wait state)
FASN_DEV void mla_gather16(uint32_t lds_base, const char* src) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_base), "v"(src) : "memory", "m0");
}

// The lanes whose row sees key `key` + 4 hi of a tile with key mask `mask`: hi is the lane's upper half-wave, so the answer is a lane mask
// made of two scalar bits - no vector register, no vector compare
FASN_DEV bool mla_key_lanes(uint64_t mask, int key) {
    const uint32_t lo = 0u - (uint32_t)((mask >> key) & 1), up = 0u - (uint32_t)((mask >> (key + 4)) & 1);
    return __builtin_amdgcn_inverse_ballot_w64(((uint64_t)up << 32) | lo);
}

template <typename Tag>
__global__ void __launch_bounds__(256, 1) fasn_mla_sparse_fwd_kernel(const MlaParams p, const MlaSparse sp) {
    using E = ET<Tag>;
    using vec8 = typename E::vec8;
    constexpr bool PRESCALE = std::is_same<Tag, f16_tag>::value;
    constexpr int NT = 256;
    constexpr int KS = MLA_E / 16;
    constexpr int DBW = MLA_EV / 32 / 2;
    constexpr int NLD = (KV_KT * MLA_CPR) / NT;

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
    // last position the list may name: below len_b and, causal, not behind the query's own position (-1 or less: nothing is a key)
    const int lim = p.causal ? min(len - 1, pos + len - p.Sq) : len - 1;

    // ---- the lane's row: a head of position pos
    const int head = hb * MLA_RB + rh * 32 + l31;
    const bool row_ok = head < p.H;
    const int h = row_ok ? head : 0;
    const int row = h * p.Sq + pos;                       // partial row (dense layout)
    float n_row = p.n;
    if (p.nt != nullptr) n_row = p.nt[b * p.nsb + h * p.nsh];
    const bool wave_rows = hb * MLA_RB + rh * 32 < p.H;

    const bool sink = n_row > 0.f && split == 0;
    float m_run = sink ? 0.f : -INFINITY;
    float l_run = (sink && hi == 0) ? n_row : 0.f;
    f32x16 oacc[DBW];
#pragma unroll
    for (int d = 0; d < DBW; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;

    if (t0 < t1 && lim >= 0) {   // (uniform over the workgroup; lim < 0: no entry can be a key, nothing is read)
        // ---- the chain's first three tiles, resolved in the open while the query loads are in flight
        const int* const idx_row = sp.idx + b * sp.sb + (int64_t)pos * sp.sq;   // (uniform: the lane is the load's offset)
        const int* const bt_row = p.bt + (int64_t)b * p.bts;
        const bool paged = p.bt != nullptr;
        const int64_t kps2 = p.kps * 2, krs2 = p.krs * 2;
        auto load_idx = [&](int tile) __attribute__((always_inline)) -> int { return tile < t1 ? idx_row[tile * KV_KT + fresh_lane_id()] : -1; };
        // entry j of this lane: its liveness, its row inside the page and the page id on its way (exec: a dead lane reads nothing)
        auto resolve = [&](int j, bool& ok, int& rip, int& page) __attribute__((always_inline)) {
            ok = j >= 0 && j <= lim;
            rip = 0, page = 0;
            if (ok) {
                if (paged) {
                    // j / page_size without a division: the estimate is the quotient or one less (j < 2^31, page_size >= 64)
                    int slot = (int)__umulhi((uint32_t)j, sp.ps_magic);
                    rip = j - slot * p.page_size;
                    if (rip >= p.page_size) ++slot, rip -= p.page_size;
                    page = bt_row[slot];
                } else {
                    rip = j, page = b;
                }
            }
        };
        auto row_addr = [&](int page, int rip) __attribute__((always_inline)) -> const char* { return p.kv + ((int64_t)page * kps2 + (int64_t)rip * krs2); };

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

        const uint32_t lds_w = lds_addr(smem) + wave * 1024;
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

        // ---- the requests of one tile: `a` the lane's entry's row address, `mask` the tile's key mask. Slot tid + i * 256 lies in row
        // r = slot / 72; over a wave r takes lane 0's value and at most the next one
        auto request = [&](int buf, const char* a, uint64_t mask) __attribute__((always_inline)) {
            if (mask == 0) return;   // (uniform)
            const uint32_t a_lo = (uint32_t)(uintptr_t)a, a_hi = (uint32_t)((uintptr_t)a >> 32);
            int tid_o = tid;
            asm volatile("" : "+v"(tid_o));
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int ci = tid_o + i * NT;
                const int r = ci / MLA_CPR, ch = (ci - r * MLA_CPR) ^ mla_swz(r);
                const int r0 = __builtin_amdgcn_readfirstlane(r), r1 = min(r0 + 1, KV_KT - 1);
                // (the builtin returns a signed int: without the casts the low word's bit 31 is smeared over the high word)
                const uint64_t s0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(a_hi, r0) << 32) | (uint32_t)__builtin_amdgcn_readlane(a_lo, r0);
                const uint64_t s1 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(a_hi, r1) << 32) | (uint32_t)__builtin_amdgcn_readlane(a_lo, r1);
                const bool live0 = (mask >> r0) & 1, live1 = (mask >> r1) & 1;
                const bool first = r == r0;
                const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_w + buf * MLA_TILEB + i * NT * 16);
                if (first ? live0 : live1) mla_gather16(dst, reinterpret_cast<const char*>(first ? s0 : s1) + ch * 16);
            }
        };

        retire_loads(n_row);

        for (int i = tid; i < MLA_SMEM / 16; i += NT) *LDS_PTR(u32x4, smem + i * 16) = u32x4{0u, 0u, 0u, 0u};
        __syncthreads();
        request(0, addr0, mask0);

        int buf = 0;
        for (int t = t0; t < t1; ++t) {
            // tile t's rows have landed (this wave's share), and with them the page ids of tile t + 2 and the entries of tile t + 3
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("" : "+v"(page2), "+v"(idx3));
            const char* const addr2 = row_addr(page2, rip2);
            bool ok3;
            int rip3, page3;
            resolve(idx3, ok3, rip3, page3);
            const uint64_t mask3 = __ballot(ok3);
            const int idx4 = load_idx(t + 4);
            __syncthreads();
            request(buf ^ 1, addr1, mask1);
            if (wave_rows && mask0 != 0) {
#define MLA_TILE_AT (buf * MLA_TILEB)
#define MLA_SCORE(x) (PRESCALE ? (x) : (x) * p.c)
#define MLA_TILE_ALL_VISIBLE false
#define MLA_KEY_VISIBLE(kb, r) mla_key_lanes(mask0, (kb) * 32 + ((r) & 3) + 8 * ((r) >> 2))
#include "fasn_mla_tile.inc"
#undef MLA_TILE_AT
#undef MLA_SCORE
#undef MLA_TILE_ALL_VISIBLE
#undef MLA_KEY_VISIBLE
            }
            buf ^= 1;
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

}  // namespace fasn
