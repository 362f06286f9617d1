// fasn_kvfp8.h — the cache calls over an FP8 cache: decode, prefill and token-packed prefill on a paged or dense cache of OCP e4m3fn codes with one fp32 scale per
// (batch element, K/V head) in device memory (fasn_kvcache.h: KvFp8). The 16-bit kernels of fasn_kvcache.h / fasn_kvprefill.h are not
// touched; these are their siblings on the same grid and split rule.
//
//   fasn_kvcache_fwd_fp8_kernel / fasn_kvprefill_fwd_fp8_kernel   one more inclusion each of the forward texts under FASN_KV_FP8
//   fasn_kvcache_fp8_combine_kernel / fasn_kvprefill_fp8_combine_kernel   the combine kernels with v_scale in front of the one rounding
//   fasn_kvcache_fp8_append_kernel / fasn_kvprefill_fp8_append_kernel   k_new / v_new rows, quantised, -> the cache rows behind the lengths
//   fasn_kvcache_fwd_fp8_window_kernel / fasn_kvprefill_fwd_fp8_window_kernel   the sliding-window siblings: FASN_KV_FP8 with FASN_KV_WINDOW
//   fasn_kvrope_fp8_kernel   fasn_kvrope_kernel in front of this cache: rotate, round to the 16-bit type, quantise, append (and rotate q)
//   fasn_kvcache_fwd_fp8_tree_kernel / fasn_kvprefill_fwd_fp8_tree_kernel   the token-tree siblings: FASN_KV_FP8 with FASN_KV_TREE
//   fasn_kvrope_fp8_tree_kernel   fasn_kvrope_fp8_kernel at the depth positions of a token tree
//   fasn_kvcache_fp8_tree_commit_kernel   the commit of an accepted path over code rows
//   fasn_kvvarlen_fwd_fp8_kernel / fasn_kvvarlen_fwd_window_fp8_kernel   the token-packed siblings: FASN_KV_FP8 with FASN_KV_PACKED (and FASN_KV_WINDOW)
//   fasn_kvvarlen_fp8_combine_kernel / fasn_kvvarlen_fp8_append_kernel / fasn_kvvarlen_rope_fp8_kernel   their combine, quantising append and
//                                         rotate-quantise-append: the kernels of fasn_kvvarlen.h / fasn_kvrope.h in front of this cache
//
// Semantics. value(code) = up(code) * scale[b, hkv], up() the exact upcast. All 254 finite codes are bf16 AND fp16 numbers, so the operands
// of the 16-bit MFMAs are the codes themselves and the scales act in fp32:
//   x_ij  = scale * k_scale[b, hkv] * (q_i . up(Kc_j))                        one factor c8 = c * k_scale on the fp32 scores
//   out_i = v_scale[b, hkv] * sum_j p_ij up(Vc_j) / (n + sum_j p_ij)          on the fp32 output, before it is rounded once
// Visibility, the lengths, the sink on split 0, lse, rows that see nothing and the stale-memory rules are the base call's.
//
// Widening. A tile is staged as KV_KT rows of D BYTES - half the buffer_load ... lds requests, descriptor ranges in bytes of the code rows,
// rows at or beyond len_b still arrive as zeros (code 0x00 is +0) - into NBUF linear buffers per operand. Once tile t has landed all 256
// threads widen it into ONE 16-bit tile image per operand, swizzled as fasn_common.h describes, and lds_read_rowfrag / lds_read_trfrag
// run on that image unchanged; a second barrier per tile publishes it. LDS: D = 64: 2 x 3 x 4 KiB + 2 x 8 KiB = 40 KiB; D = 128:
// 2 x 2 x 8 KiB + 2 x 16 KiB = 64 KiB - two workgroups per CU, as the 16-bit kernels.
#pragma once
#include "fasn_kvprefill.h"
#include "fasn_kvrope.h"

namespace fasn {

// The packed kernels of this file carry FASN_KV_LOCAL: their host-side handles stay out of the library's dynamic symbol table (on the
// device a kernel is raised to protected visibility whatever it is given, so the code objects hold them as they hold every other kernel).
// The library exports its C entry points; no packed FP8 name is among them, and none shows up beside them.
#define FASN_KV_LOCAL __attribute__((visibility("hidden")))

constexpr int kv_fp8_smem(int D) { return 2 * kv_nbuf(D) * KV_KT * D + 2 * KV_KT * D * 2; }   // staged codes + one 16-bit image per operand

// The widening pass of one operand: thread tid fills the slots tid + i * 256 of the 16-bit image - the slots it would have staged from a
// 16-bit cache, slot ci = (row ci / CPR, chunk (ci % CPR) ^ swz) - from the 8 codes of that chunk in the linear code tile.
// v_cvt_pk_f32_fp8 is exact for all 256 codes (OCP e4m3fn on gfx950: subnormals, both zeros, NaN -> NaN) and every finite code is
// a bf16 and an fp16 number, so the conversion to the operand type rounds nothing. 64 lanes read 512 contiguous bytes, permuted in
// 8-byte words, and write 1024 contiguous bytes: no bank conflict either way.
template <typename E, int D>
FASN_DEV void kv_fp8_widen(const char* src, char* img, int tid) {
    constexpr int CPR = D / 8;
    constexpr int NLD = (KV_KT * CPR) / 256;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int ci = tid + i * 256;
        const int r = ci / CPR, ch = (ci % CPR) ^ swz_f<D>(r);
        const u32x2 raw = *LDS_PTR(const u32x2, src + r * D + ch * 8);
        f32x8 x;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], false), up = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], true);
            x[4 * w] = lo[0], x[4 * w + 1] = lo[1], x[4 * w + 2] = up[0], x[4 * w + 3] = up[1];
        }
        const typename E::vec8 y = E::cvt8(x);
        u32x4 out;
        __builtin_memcpy(&out, &y, 16);
        *LDS_PTR(u32x4, img + ci * 16) = out;
    }
}

#define FASN_KV_FP8 1
#include "fasn_kvcache_fwd.inc"
#include "fasn_kvprefill_fwd.inc"
// fasn_kvcache_fwd_fp8_window_kernel / fasn_kvprefill_fwd_fp8_window_kernel(..., KvFp8, KvWindow): the sliding-window siblings, the product
// of the two switches. From the window kernels: tlo, the split of [tlo, tiles_b) - tiles below tlo get no request and no table read -
// the full-tile test and the one-compare mask on a per-tile opaque dvis. From the FP8 kernels: everything above. Same LDS, same grid
// rule as the 16-bit window kernels; the FP8 combine kernels below serve both.
#define FASN_KV_WINDOW 1
#include "fasn_kvcache_fwd.inc"
#include "fasn_kvprefill_fwd.inc"
#undef FASN_KV_WINDOW
// fasn_kvcache_fwd_fp8_tree_kernel / fasn_kvprefill_fwd_fp8_tree_kernel(..., KvFp8, KvTree): the token-tree siblings, the product of
// FASN_KV_FP8 and FASN_KV_TREE. From the tree kernels: base, tlo and the split of [tlo, tiles_b), the conservative full-tile test, the
// per-lane 64-bit visibility word built inside the masked branch, the run-time window tree.w. From the FP8 kernels: everything above.
// Same LDS, same grid and split rule as the 16-bit tree call of the same shape; the FP8 combine kernels below serve these too.
#define FASN_KV_TREE 1
#include "fasn_kvcache_fwd.inc"
#include "fasn_kvprefill_fwd.inc"
#undef FASN_KV_TREE
// fasn_kvvarlen_fwd_fp8_kernel(..., KvPacked, KvFp8) / fasn_kvvarlen_fwd_window_fp8_kernel(..., KvPacked, KvFp8, KvWindow): the token-packed
// siblings (fasn_kvvarlen.h), the product of FASN_KV_FP8 and FASN_KV_PACKED, without and with FASN_KV_WINDOW. From the packed kernels: the
// item of the schedule kernel's table, the token rows, lse [H, T], the partial slot (item, hkv, split). From the FP8 kernels: everything
// above, the scales read at the item's b. Same LDS as the FP8 prefill, same grid and split rule as the 16-bit packed call of the same
// shape; fasn_kvvarlen_schedule_kernel serves them as it is, fasn_kvvarlen_fp8_combine_kernel below merges their partials.
#define FASN_KV_PACKED 1
#include "fasn_kvprefill_fwd.inc"
#define FASN_KV_WINDOW 1
#include "fasn_kvprefill_fwd.inc"
#undef FASN_KV_WINDOW
#undef FASN_KV_PACKED
#undef FASN_KV_FP8

// fasn_kvcache_combine_kernel with v_scale[b, hkv] on the normalised fp32 row, in front of its one rounding
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvcache_fp8_combine_kernel(const KvParams p, const KvFp8 f8) {
    using E = ET<Tag>;
    constexpr int TPR = D / 4;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rowg = gid / TPR;   // (b * Hkv + hkv, r)
    const int c4 = (int)(gid % TPR) * 4;
    if (rowg >= (int64_t)p.B * p.Hkv * p.R) return;
    const int bk = (int)(rowg / p.R), r = (int)(rowg % p.R);
    const int b = bk / p.Hkv, hkv = bk % p.Hkv, h = hkv * p.G + r / p.Sq, pos = r % p.Sq;
    const KvMerged m = kv_merge<D>(c4, p.part_o, p.part_ml, p.nsplit, [&](int s) { return ((int64_t)bk * p.nsplit + s) * p.R + r; });
    kv_store_decode_row<E>(p, b, h, pos, c4, m, f8.vs[b * f8.vsb + hkv * f8.vsh]);
}

// fasn_kvprefill_combine_kernel with v_scale[b, hkv], likewise
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvprefill_fp8_combine_kernel(const KvPrefillParams pp, const KvFp8 f8) {
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
    const int b = bk / p.Hkv, hkv = bk % p.Hkv, h = hkv * p.G + g;
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
    kv_store_row<E>(oat, m, f8.vs[b * f8.vsb + hkv * f8.vsh]);
    if (lat != nullptr) *lat = kv_lse(m);
}

// fasn_kvvarlen_combine_kernel with v_scale[b, hkv], likewise: b is the item's
template <typename Tag, int D>
FASN_KV_LOCAL __global__ void __launch_bounds__(256) fasn_kvvarlen_fp8_combine_kernel(const KvPrefillParams pp, const KvPacked pk, const KvFp8 f8) {
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
    kv_store_row<E>(oat, m, f8.vs[it.x * f8.vsb + hkv * f8.vsh]);
    if (p.lse != nullptr && c4 == 0) p.lse[(int64_t)h * pk.T + tok] = kv_lse(m);
}

// ---- quantising append
// code = rne_e4m3(clamp(float(x) / s, -448, 448)); a NaN stays a NaN code. The division is the correctly rounded fp32 division (this build
// has no fast-math). The clamp makes the saturation explicit - whatever the conversion instruction's mode does beyond 448 is never asked -
// and is written so that a NaN falls through both comparisons; v_cvt_pk_fp8_f32 rounds to nearest even and turns NaN into 0x7f / 0xff.
FASN_DEV float kv_fp8_prep(float x, float s) {
    const float y = x / s;
    return y > 448.f ? 448.f : (y < -448.f ? -448.f : y);
}
// 16 elements of a row in the query's dtype (two 16-byte loads) -> 16 codes
template <typename E>
FASN_DEV u32x4 kv_fp8_quant16(const char* src, float s) {
    u32x4 out;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const u32x4 raw = gload16(src + half * 16);
        float x[8];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            x[2 * w] = kv_fp8_prep(E::to_f32((uint16_t)(raw[w] & 0xffffu)), s);
            x[2 * w + 1] = kv_fp8_prep(E::to_f32((uint16_t)(raw[w] >> 16)), s);
        }
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            int pk = 0;
            pk = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w], x[4 * w + 1], pk, false);
            pk = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w + 2], x[4 * w + 3], pk, true);
            out[2 * half + w] = (uint32_t)pk;
        }
    }
    return out;
}

// k_new / v_new row i of (b, hkv), quantised -> cache row seqlens[b] + i: 16 codes (16 bytes stored) per thread and tensor. The rules of
// fasn_kvcache_append_kernel / fasn_kvprefill_append_kernel: rows i >= qlen_b (PREFILL) are neither read nor written, positions at or
// beyond the capacity (or negative) are dropped, `seqlens` is not modified.
template <typename Tag, int D, bool PREFILL>
FASN_DEV void kv_fp8_append(const KvParams& p, const int* qlens, const KvFp8& f8) {
    using E = ET<Tag>;
    constexpr int CPR = D / 16;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)p.B * p.Hkv * p.Sq * CPR) return;
    const int ch = (int)(gid % CPR);
    int64_t rest = gid / CPR;
    const int i = (int)(rest % p.Sq);
    rest /= p.Sq;
    const int hkv = (int)(rest % p.Hkv), b = (int)(rest / p.Hkv);
    if (PREFILL && qlens != nullptr && i >= qlens[b]) return;
    const int64_t key = (int64_t)p.seqlens[b] + i;
    if (key < 0 || key >= p.capacity) return;
    const int slot = (int)(key / p.page_size), rip = (int)(key % p.page_size);
    const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
    const u32x4 kx = kv_fp8_quant16<E>(p.kn + (b * p.kns[0] + hkv * p.kns[1] + (int64_t)i * p.kns[2]) * 2 + ch * 32, f8.ks[b * f8.ksb + hkv * f8.ksh]);
    const u32x4 vx = kv_fp8_quant16<E>(p.vn + (b * p.vns[0] + hkv * p.vns[1] + (int64_t)i * p.vns[2]) * 2 + ch * 32, f8.vs[b * f8.vsb + hkv * f8.vsh]);
    gstore16(p.k + page * p.kps + (int64_t)rip * p.krs + (int64_t)hkv * p.khs + ch * 16, kx);
    gstore16(p.v + page * p.vps + (int64_t)rip * p.vrs + (int64_t)hkv * p.vhs + ch * 16, vx);
}
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvcache_fp8_append_kernel(const KvParams p, const KvFp8 f8) {
    kv_fp8_append<Tag, D, false>(p, nullptr, f8);
}
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvprefill_fp8_append_kernel(const KvPrefillParams pp, const KvFp8 f8) {
    kv_fp8_append<Tag, D, true>(pp.kv, pp.qlens, f8);
}
// fasn_kvvarlen_append_kernel (fasn_kvvarlen.h) in front of an FP8 cache: its lanes - one thread per (token t < T, K/V head, chunk), here a
// chunk of 16 codes - its binary search in cu and its skip rules (a token of no sequence, beyond its sequence's clamped length, a row
// outside the capacity), with the arithmetic and the byte addressing of kv_fp8_append: token t of k_new / v_new, quantised with the scales
// of its sequence's (b, hkv) -> cache row seqlens[b] + (t - cu[b]).
template <typename Tag, int D>
FASN_KV_LOCAL __global__ void __launch_bounds__(256) fasn_kvvarlen_fp8_append_kernel(const KvPrefillParams pp, const KvPacked pk, const KvFp8 f8) {
    using E = ET<Tag>;
    const KvParams& p = pp.kv;
    constexpr int CPR = D / 16;
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
    const u32x4 kx = kv_fp8_quant16<E>(p.kn + (hkv * p.kns[1] + (int64_t)t * p.kns[2]) * 2 + ch * 32, f8.ks[b * f8.ksb + hkv * f8.ksh]);
    const u32x4 vx = kv_fp8_quant16<E>(p.vn + (hkv * p.vns[1] + (int64_t)t * p.vns[2]) * 2 + ch * 32, f8.vs[b * f8.vsb + hkv * f8.vsh]);
    gstore16(p.k + page * p.kps + (int64_t)rip * p.krs + (int64_t)hkv * p.khs + ch * 16, kx);
    gstore16(p.v + page * p.vps + (int64_t)rip * p.vrs + (int64_t)hkv * p.vhs + ch * 16, vx);
}

// ---- rotate-quantise-append
// 8 elements of the call's 16-bit type, as one 16-byte register value -> 8 codes: kv_fp8_quant16's arithmetic on values that are in
// registers already (the rotated key, rounded once to the 16-bit type)
template <typename E>
FASN_DEV u32x2 kv_fp8_quant8(u32x4 raw, float s) {
    float x[8];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        x[2 * w] = kv_fp8_prep(E::to_f32((uint16_t)(raw[w] & 0xffffu)), s);
        x[2 * w + 1] = kv_fp8_prep(E::to_f32((uint16_t)(raw[w] >> 16)), s);
    }
    u32x2 out;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        int pk = 0;
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w], x[4 * w + 1], pk, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w + 2], x[4 * w + 3], pk, true);
        out[w] = (uint32_t)pk;
    }
    return out;
}

// fasn_kvrope_kernel (fasn_kvrope.h) in front of an FP8 cache: the same lanes, grid, positions, dropped rows and table handling, and the
// same unit text for the rotation. A query unit is that kernel's: 16-bit in, 16-bit q_out. A K/V unit addresses the cache in BYTES: its
// 16 key elements are rotated and rounded ONCE to the call's 16-bit type - the key the 16-bit kernel would have stored - and those 16-bit
// values are quantised as kv_fp8_quant16 quantises k_new, so a rotated key has one definition across both cache types and the call is
// "eager rotation, then fasn_kv*_fp8_append" byte for byte. Chunk c of a row (16 bytes of 16-bit elements) is the 8 codes at byte 8 c:
// two 8-byte stores where the 16-bit kernel has two 16-byte stores; units at or beyond rotary_dim are quantised, not copied. The unit's
// 16 v_new elements are quantised with v_scale and stored as one 16-byte group. The tree variant follows it.
#define FASN_KVROPE_FP8 1
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvrope_fp8_kernel(const KvRopeParams rp, const KvFp8 f8) {
    using E = ET<Tag>;
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
    char* dst = nullptr;    // a query unit's row of q_out (16-bit)
    char* dst8 = nullptr;   // a K/V unit's row of the code cache
    float ksc = 1.f;
    if (!isq) {
        pos = (int64_t)p.seqlens[b] + i;
        if (pos < 0 || pos >= p.capacity) return;   // dropped: the host does not know the lengths
        const int slot = (int)(pos / p.page_size), rip = (int)(pos % p.page_size);
        const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
        src = p.kn + (b * p.kns[0] + h * p.kns[1] + (int64_t)i * p.kns[2]) * 2;
        dst8 = p.k + page * p.kps + (int64_t)rip * p.krs + (int64_t)h * p.khs;
        ksc = f8.ks[b * f8.ksb + h * f8.ksh];
        const u32x4 vx = kv_fp8_quant16<E>(p.vn + (b * p.vns[0] + h * p.vns[1] + (int64_t)i * p.vns[2]) * 2 + u * 32, f8.vs[b * f8.vsb + h * f8.vsh]);
        gstore16(p.v + page * p.vps + (int64_t)rip * p.vrs + (int64_t)h * p.vhs + u * 16, vx);
    } else {
        // len_b per lane, as in fasn_kvrope_kernel
        int len;
        if (rp.add_qlen < 0) len = min(max(p.seqlens[b] + p.seqlen_add, 0), p.capacity);
        else len = (int)min(max((int64_t)p.seqlens[b] + (rp.add_qlen ? qlen : 0), (int64_t)0), (int64_t)p.capacity);
        pos = (int64_t)i + len - qlen;
        src = p.q + (b * p.qs[0] + h * p.qs[1] + (int64_t)i * p.qs[2]) * 2;
        dst = rp.qo + (b * rp.qos[0] + h * rp.qos[1] + (int64_t)i * rp.qos[2]) * 2;
    }
#include "fasn_kvrope_unit.inc"
}

// fasn_kvrope_fp8_kernel at DEPTH positions (fasn_kvcache.h: KvTree), as fasn_kvrope_tree_kernel relates to fasn_kvrope_kernel: node i of
// k_new / v_new is still WRITTEN to cache row seqlens[b] + i, but rotated at seqlens[b] + d_i - then rounded once to the 16-bit type and
// quantised with k_scale, v_new quantised beside it - and the query at p_i = len_b - qlen_b + d_i, with
// d_i = max(popcount(mask[b, i] & the low qlen_b bits) - 1, 0). Same lanes, same grid, the same unit text; the window member of the
// operand takes no part here.
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvrope_fp8_tree_kernel(const KvRopeParams rp, const KvFp8 f8, const KvTree tree) {
    using E = ET<Tag>;
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
    char* dst = nullptr;    // a query unit's row of q_out (16-bit)
    char* dst8 = nullptr;   // a K/V unit's row of the code cache
    float ksc = 1.f;
    if (!isq) {
        const int64_t at = (int64_t)p.seqlens[b] + i;   // the row written
        if (at < 0 || at >= p.capacity) return;         // dropped: the host does not know the lengths
        pos = (int64_t)p.seqlens[b] + depth;            // the position rotated at
        const int slot = (int)(at / p.page_size), rip = (int)(at % p.page_size);
        const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
        src = p.kn + (b * p.kns[0] + h * p.kns[1] + (int64_t)i * p.kns[2]) * 2;
        dst8 = p.k + page * p.kps + (int64_t)rip * p.krs + (int64_t)h * p.khs;
        ksc = f8.ks[b * f8.ksb + h * f8.ksh];
        const u32x4 vx = kv_fp8_quant16<E>(p.vn + (b * p.vns[0] + h * p.vns[1] + (int64_t)i * p.vns[2]) * 2 + u * 32, f8.vs[b * f8.vsb + h * f8.vsh]);
        gstore16(p.v + page * p.vps + (int64_t)rip * p.vrs + (int64_t)h * p.vhs + u * 16, vx);
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

// fasn_kvvarlen_rope_kernel (fasn_kvrope.h) in front of an FP8 cache, as fasn_kvrope_fp8_kernel relates to fasn_kvrope_kernel: one lane per
// (token t < T, head, unit), the K/V units first, the token's sequence from the binary search in cu, qlen_b with the schedule kernel's
// clamps, the same unit text. A K/V unit rotates its 16 key elements, rounds them once to the 16-bit type, quantises them with the
// k_scale of the token's (b, hkv) and writes the codes - rows addressed in bytes - and quantises v_new beside it; a query unit is the
// 16-bit kernel's.
template <typename Tag, int D>
FASN_KV_LOCAL __global__ void __launch_bounds__(256) fasn_kvvarlen_rope_fp8_kernel(const KvRopeParams rp, const KvPacked pk, const KvFp8 f8) {
    using E = ET<Tag>;
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
    char* dst = nullptr;    // a query unit's row of q_out (16-bit)
    char* dst8 = nullptr;   // a K/V unit's row of the code cache
    float ksc = 1.f;
    if (!isq) {
        pos = (int64_t)p.seqlens[b] + i;
        if (pos < 0 || pos >= p.capacity) return;   // dropped: the host does not know the lengths
        const int slot = (int)(pos / p.page_size), rip = (int)(pos % p.page_size);
        const int64_t page = p.bt != nullptr ? p.bt[(int64_t)b * p.bts + slot] : b;
        src = p.kn + (h * p.kns[1] + (int64_t)t * p.kns[2]) * 2;
        dst8 = p.k + page * p.kps + (int64_t)rip * p.krs + (int64_t)h * p.khs;
        ksc = f8.ks[b * f8.ksb + h * f8.ksh];
        const u32x4 vx = kv_fp8_quant16<E>(p.vn + (h * p.vns[1] + (int64_t)t * p.vns[2]) * 2 + u * 32, f8.vs[b * f8.vsb + h * f8.vsh]);
        gstore16(p.v + page * p.vps + (int64_t)rip * p.vrs + (int64_t)h * p.vhs + u * 16, vx);
    } else {
        const int len = (int)min(max((int64_t)p.seqlens[b] + (rp.add_qlen ? qlen : 0), (int64_t)0), (int64_t)p.capacity);
        pos = i + len - qlen;
        src = p.q + (h * p.qs[1] + (int64_t)t * p.qs[2]) * 2;
        dst = rp.qo + (h * rp.qos[1] + (int64_t)t * rp.qos[2]) * 2;
    }
#include "fasn_kvrope_unit.inc"
}
#undef FASN_KVROPE_FP8

// ---- commit over code rows
// fasn_kvcache_tree_commit_kernel (fasn_kvcache.h: KvCommit, the hazards and the skip rules are stated there) on a cache of codes: the strides
// count codes, one thread owns 16 codes - one 16-byte chunk, D / 16 chunks per row - of one (b, hkv) in K and in V and walks k upward. The
// program-order argument is that kernel's: move k reads row accepted[k] > k and writes row k, no later move of the thread reads a row an
// earlier one wrote, and no other thread touches the thread's bytes.
template <int D>
__global__ void __launch_bounds__(256) fasn_kvcache_fp8_tree_commit_kernel(const KvCommit c) {
    constexpr int CPR = D / 16;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)c.B * c.Hkv * CPR) return;
    const int ch = (int)(gid % CPR);
    const int64_t rest = gid / CPR;
    const int hkv = (int)(rest % c.Hkv), b = (int)(rest / c.Hkv);
    const int64_t base = c.seqlens[b];
    const int alen = min(max(c.alens[b], 0), c.A);
    const int* const acc = c.acc + (int64_t)b * c.accs;
    const int* const bt = c.bt != nullptr ? c.bt + (int64_t)b * c.bts : nullptr;
    char* const kh = c.k + (int64_t)hkv * c.khs + ch * 16;
    char* const vh = c.v + (int64_t)hkv * c.vhs + ch * 16;
    for (int k = 0; k < alen; ++k) {
        const int node = acc[k];
        if (node <= k || node >= c.nodes) continue;   // (node == k: the row is where it belongs)
        const int64_t src = base + node, dst = base + k;
        if (dst < 0 || src >= c.capacity) continue;
        const int sslot = (int)(src / c.page_size), srip = (int)(src % c.page_size);
        const int dslot = (int)(dst / c.page_size), drip = (int)(dst % c.page_size);
        const int64_t spage = bt != nullptr ? bt[sslot] : b, dpage = bt != nullptr ? bt[dslot] : b;
        const u32x4 kx = gload16(kh + spage * c.kps + (int64_t)srip * c.krs);
        const u32x4 vx = gload16(vh + spage * c.vps + (int64_t)srip * c.vrs);
        gstore16(kh + dpage * c.kps + (int64_t)drip * c.krs, kx);
        gstore16(vh + dpage * c.vps + (int64_t)drip * c.vrs, vx);
    }
}

}  // namespace fasn
