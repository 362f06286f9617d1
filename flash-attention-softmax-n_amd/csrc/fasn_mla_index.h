// fasn_mla_index.h — the lightning indexer in front of the sparse MLA decode (DeepSeek-V3.2): per (batch element b, query position i) the
// logit of cache position j is
//     logit[b, i, j] = sum_h w[b, h, i] * relu(q[b, h, i, :] . k_b[j, :])          h < HI (32 or 64), 128 features, no scale operand
// and the call returns the min(topk, L) positions of largest logit in ascending position order, -1 behind them. Three kernels, none shared
// with the attention kernels - there is no softmax, no V and no split merge:
//   fasn_mla_index_append_kernel   k_new rows -> index-key rows len_b .. len_b + Sq - 1 (dropped beyond the capacity)
//   fasn_mla_index_logits_kernel   one GEMM against stationary queries, the ReLU-weighted head sum in the lane, fp32 logits
//   fasn_mla_index_select_kernel   radix select of the rank-topk key, ordered compaction
//
// Logits. A work item is (batch element, position, run of `tpw` 64-key tiles); four waves, wave w owns keys 32 w .. 32 w + 31 of a 128-key
// unit. Every key row is used by ONE wave, ONCE: it goes from global memory straight into the MFMA's B operand, no LDS. The MFMA is
// v_mfma_f32_32x32x16 with the heads as M rows (A = Q) and the keys as N columns (B = K^T): lane (l & 31, g = l >> 5) owns key column l & 31
// and holds, per block of 32 heads, the 16 head rows (r & 3) + 8 (r >> 2) + 4 g. The head sum - max(acc, 0) and one fma with w_h per
// accumulator - never leaves the lane; one cross-half add (lanes l, l + 32) finishes it and lanes 0 .. 31 store 32 consecutive floats.
//
// The k index of an MFMA may be permuted freely when A and B use the same permutation: slot (k-step s, half g, j) is feature 64 g + 8 s + j.
// Lane (key r, half g) then reads the 128 contiguous bytes [128 g, 128 g + 128) of its key row as eight 16-byte loads - whole cache lines
// per lane - and k-step s consumes chunk s. Q^T is loaded once per workgroup in the same permutation and stays in registers: 8 k-steps x
// HI / 32 blocks x 4. The weights of the lane's 16 HI / 32 head rows sit in registers too (the kernel has no LDS at all). The loads of the
// next unit are issued in front of the MFMAs of the current one (two register buffers).
//
// Lengths and stale memory. len_b = clamp(seqlens[b] + seqlen_add, 0, capacity) is read in the kernel, L = len_b - (Sq - 1 - i) when
// causal. A workgroup whose run lies at or beyond L returns behind that read; a wave whose 32 keys lie at or beyond L reads no table slot
// and no row. The page id of a wave's keys is a scalar load; a 32-key group never straddles a page (page_size % 64 == 0). Positions >= L
// inside a group that has a live key read the row L - 1 instead of their own - the same group, the same page, so no address is formed
// from a table slot at or beyond the pages L needs - and write -inf where the logits row has the position.
//
// Select. One workgroup of 1024 threads per (b, i). L <= topk: the list is 0 .. L - 1 and the logits are not read. Otherwise each logit
// becomes an order-preserving 32-bit key (x + 0.0f first: -0 and +0 are one key), the key T of rank topk is found by three radix passes
// (11 + 11 + 10 bits, a 2048-bin LDS histogram, a suffix scan over the bins, the prefix narrowing pass by pass; `need` = how many entries
// equal to T still fit), and a last pass in position order takes an entry iff key > T or key == T and it is among the first `need` such -
// its output slot from an ordered scan (ballot and popcount per wave, wave totals through LDS, a running base over the chunks). The list
// is ascending and the tie rule - the lower position wins - exact.
#pragma once
#include "fasn_common.h"

namespace fasn {

constexpr int MLI_D = 128;          // features of an index key and of an index query
constexpr int MLI_ROWB = MLI_D * 2; // bytes of a row
constexpr int MLI_UNIT = 128;       // keys of a workgroup's step: 32 per wave
constexpr int MLI_SEL_NT = 1024;    // threads of the select workgroup
constexpr int MLI_BINS = 2048;

struct MlaIndexParams {
    const char* q;       // [B, HI, Sq, 128]
    int64_t qs[3];       // element strides (batch, head, position)
    const float* w;      // [B, HI, Sq]
    int64_t ws[3];
    char* kc;            // the index-key pool
    int64_t kps, krs;    // element strides (page, row)
    const int* bt;       // block table [B][bts] or nullptr (dense: page = batch element)
    int64_t bts;
    const int* seqlens;  // [B], device
    int seqlen_add;
    int page_size;
    int capacity;
    int B, Sq;
    int causal;
    int topk;
    int tpw;             // 64-key tiles per workgroup (even)
    int nrun;            // workgroups per (b, i)
    int* idx;            // [B, Sq, topk]
    int64_t is[2];
    float* lg;           // logits [B, Sq, lcols]
    int64_t ls[2];
    int lcols;           // positions a logits row has
    // append
    const char* kn;
    int64_t kns[2];      // k_new element strides (batch, row)
};

// the keys row (b, i) sees: positions 0 .. L - 1 (L <= 0: none)
FASN_DEV int mli_visible(const MlaIndexParams& p, int b, int i) {
    const int len = __builtin_amdgcn_readfirstlane(p.seqlens[b]) + p.seqlen_add;
    const int len_b = min(max(len, 0), p.capacity);
    return p.causal ? len_b - (p.Sq - 1 - i) : len_b;
}

template <typename Tag, int HI>
__global__ void __launch_bounds__(256) fasn_mla_index_logits_kernel(const MlaIndexParams p) {
    using E = ET<Tag>;
    using vec8 = typename E::vec8;
    constexpr int NB = HI / 32;   // head blocks
    constexpr int KS = 8;         // k-steps: 128 features / 16

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31, g = lane >> 5;

    const int wg = (int)blockIdx.x;
    const int run = wg % p.nrun;
    const int bi = wg / p.nrun;
    const int b = bi / p.Sq, i = bi - b * p.Sq;

    const int L = mli_visible(p, b, i);
    const int key0 = run * p.tpw * 64;   // first key of the run
    if (key0 >= L) return;               // (uniform over the workgroup: no table slot, no row)
    const int key1 = min(key0 + p.tpw * 64, (L + 63) & ~63);   // behind the run's last live tile

    // ---- Q^T in the permuted k order, and the weights of the lane's head rows
    vec8 qf[NB][KS];
    {
        const char* qp = p.q + (b * p.qs[0] + (int64_t)l31 * p.qs[1] + (int64_t)i * p.qs[2]) * 2 + g * 128;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const u32x4 raw = gload16(qp + (int64_t)nb * 32 * p.qs[1] * 2 + s * 16);
                __builtin_memcpy(&qf[nb][s], &raw, 16);
            }
    }
    float wf[NB][16];
    {
        const float* wp = p.w + b * p.ws[0] + (int64_t)i * p.ws[2];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) wf[nb][r] = wp[(int64_t)(nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * g) * p.ws[1]];
    }

    const __attribute__((address_space(4))) int* const bt_row = (const __attribute__((address_space(4))) int*)(p.bt + (int64_t)b * p.bts);
    const bool paged = p.bt != nullptr;
    // the eight chunks of the lane's key row in the unit that starts at key u (the wave's group: u + 32 wave .. + 31); a group without a
    // live key reads nothing
    auto request = [&](int u, u32x4 (&kf)[KS]) {
        const int k0 = u + wave * 32;
        if (k0 >= L) return;
        const int key = min(k0 + l31, L - 1);
        int64_t page = b;
        int rip = key;
        if (paged) {
            const int slot = k0 / p.page_size;
            page = bt_row[slot];
            rip = key - slot * p.page_size;
        }
        const char* rp = p.kc + (page * p.kps + (int64_t)rip * p.krs) * 2 + g * 128;
#pragma unroll
        for (int s = 0; s < KS; ++s) kf[s] = gload16(rp + s * 16);
    };

    float* const lrow = p.lg + b * p.ls[0] + (int64_t)i * p.ls[1];
    u32x4 kf[2][KS];
    request(key0, kf[0]);
#pragma unroll 1
    for (int u = key0; u < key1; u += 2 * MLI_UNIT) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {   // (the two register buffers by name: no dynamic indexing)
            const int uu = u + half * MLI_UNIT;
            if (uu >= key1) break;
            if (uu + MLI_UNIT < key1) request(uu + MLI_UNIT, kf[half ^ 1]);
            const int k0 = uu + wave * 32;
            const int key = k0 + l31;
            if (k0 < L) {
                f32x16 acc[NB];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    vec8 kb;
                    __builtin_memcpy(&kb, &kf[half][s], 16);
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) acc[nb] = E::mfma(qf[nb][s], kb, acc[nb]);
                }
                float part = 0.f;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) part = __builtin_fmaf(wf[nb][r], fmaxf(acc[nb][r], 0.f), part);
                const float logit = sum_across_halves(part);
                if (g == 0 && key < p.lcols) lrow[key] = key < L ? logit : -INFINITY;
            } else if (g == 0 && k0 < key1 && key < p.lcols) {
                lrow[key] = -INFINITY;   // the dead group of a live tile
            }
        }
    }
}

// ---- select -----------------------------------------------------------------------------------------------------------------------
// larger logit <=> larger key; -0.0 and +0.0 are one key
FASN_DEV uint32_t mli_key(float x) {
    const uint32_t u = __float_as_uint(x + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive prefix of `v` over the 1024 threads in thread order, through `tot` (16 words of LDS). The caller alternates between two `tot`
// arrays, so one barrier per call is enough.
FASN_DEV uint32_t mli_scan(uint32_t v, uint32_t* tot, int lane, int wave) {
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) tot[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int k = 0; k < wave; ++k) base += tot[k];
    return base + inc - v;
}

// (a template on its workgroup size, which the launch record then shows beside the name)
template <int NT>
__global__ void __launch_bounds__(NT) fasn_mla_index_select_kernel(const MlaIndexParams p) {
    static_assert(NT == MLI_SEL_NT, "the scans are written for 16 waves and two bins per thread");
    __shared__ uint32_t hist[MLI_BINS];
    __shared__ uint32_t tot[2][2][MLI_SEL_NT / 64];
    __shared__ uint32_t found[2];   // the bin of the pass, what is still needed inside it

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int b = (int)blockIdx.x / p.Sq, i = (int)blockIdx.x - b * p.Sq;
    const int L = mli_visible(p, b, i);
    int* const out = p.idx + b * p.is[0] + (int64_t)i * p.is[1];

    if (L <= p.topk) {   // (uniform) the list is 0 .. L - 1: the logits are not read
        for (int e = tid; e < p.topk; e += MLI_SEL_NT) out[e] = e < L ? e : -1;
        return;
    }
    const float* const lrow = p.lg + b * p.ls[0] + (int64_t)i * p.ls[1];

    // ---- the key T of rank topk: three passes over logit[0:L], most significant bits first
    uint32_t prefix = 0, need = (uint32_t)p.topk;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;       // the pass's digit: bits shift .. shift + nb - 1
        const int nb = pass == 2 ? 10 : 11;
        for (int e = tid; e < MLI_BINS; e += MLI_SEL_NT) hist[e] = 0;
        __syncthreads();
        for (int j = tid; j < L; j += MLI_SEL_NT) {
            const uint32_t k = mli_key(lrow[j]);
            if (pass == 0 || (k >> (shift + nb)) == prefix) atomicAdd(&hist[(k >> shift) & ((1u << nb) - 1)], 1u);
        }
        __syncthreads();
        // suffix scan: thread t holds bins 2047 - 2 t and 2046 - 2 t, `above` = entries in the bins above its first
        const int hb = MLI_BINS - 1 - 2 * tid;
        const uint32_t c0 = hist[hb], c1 = hist[hb - 1];
        const uint32_t above = mli_scan(c0 + c1, tot[pass & 1][0], lane, wave);
        if (above < need && need <= above + c0) found[0] = (uint32_t)hb, found[1] = need - above;
        else if (above + c0 < need && need <= above + c0 + c1) found[0] = (uint32_t)(hb - 1), found[1] = need - above - c0;
        __syncthreads();
        prefix = (prefix << nb) | found[0];
        need = found[1];
        __syncthreads();   // (found and hist are free for the next pass)
    }
    const uint32_t T = prefix;

    // ---- the last pass, in position order: chunks of 1024 positions, slot = entries above T so far + min(entries equal to T so far, need)
    uint32_t base_gt = 0, base_eq = 0;
    int par = 0;
#pragma unroll 1
    for (int j0 = 0; j0 < L; j0 += MLI_SEL_NT, par ^= 1) {
        const int j = j0 + tid;
        const uint32_t k = j < L ? mli_key(lrow[j]) : 0u;
        const bool gt = j < L && k > T, eq = j < L && k == T;
        const uint64_t mgt = __ballot(gt), meq = __ballot(eq);
        const uint64_t below = (1ull << lane) - 1ull;
        if (lane == 0) {
            tot[par][0][wave] = (uint32_t)__popcll(mgt);
            tot[par][1][wave] = (uint32_t)__popcll(meq);
        }
        __syncthreads();
        uint32_t gt_before = base_gt + (uint32_t)__popcll(mgt & below), eq_before = base_eq + (uint32_t)__popcll(meq & below);
        for (int wv = 0; wv < MLI_SEL_NT / 64; ++wv) {
            const uint32_t cg = tot[par][0][wv], ce = tot[par][1][wv];
            if (wv < wave) gt_before += cg, eq_before += ce;
            base_gt += cg, base_eq += ce;
        }
        if (gt || (eq && eq_before < need)) out[gt_before + min(eq_before, need)] = j;
    }
}

// k_new row i of batch element b -> index-key row seqlens[b] + i, 16 bytes per thread. Rows that would land at or beyond the capacity (or
// at a negative position) are dropped here: the host does not know the lengths.
__global__ void __launch_bounds__(256) fasn_mla_index_append_kernel(const MlaIndexParams p) {
    constexpr int CPR = MLI_ROWB / 16;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)p.B * p.Sq * CPR) return;
    const int ch = (int)(gid % CPR);
    const int64_t rest = gid / CPR;
    const int i = (int)(rest % p.Sq), b = (int)(rest / p.Sq);
    const int64_t key = (int64_t)p.seqlens[b] + i;
    if (key < 0 || key >= p.capacity) return;
    const int slot = (int)(key / p.page_size), rip = (int)(key % p.page_size);
    const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
    const u32x4 x = gload16(p.kn + (b * p.kns[0] + (int64_t)i * p.kns[1]) * 2 + ch * 16);
    gstore16(p.kc + (page * p.kps + (int64_t)rip * p.krs) * 2 + ch * 16, x);
}

}  // namespace fasn
