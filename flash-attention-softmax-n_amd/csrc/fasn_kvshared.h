// fasn_kvshared.h — decode over a paged K/V cache behind a SHARED PREFIX (cascade): the prefix pages are walked once per K/V head for the
// rows of all batch elements, each batch element's own suffix as the decode call walks it, and the two are merged through the
// un-normalised fp32 partials the decode path writes anyway.
//
// Three kernels (none of the others changes):
//   fasn_kvshared_prefix_kernel   (K/V head, 128-row block, split): the tiles [0, ceil(P / 64)) of the pages `prefix_table` names. No sink.
//   fasn_kvshared_suffix_kernel   (batch element, K/V head, split): the tiles [P / 64, ceil(len_b / 64)) of the pages block_table[b] names,
//                                 keys below P hidden in the first tile. Split 0 carries the sink, as in fasn_kvcache_fwd_kernel.
//   fasn_kvshared_combine_kernel  merges a row's suffix partials and its prefix partials and scatters it to o / lse
//
// The virtual cache. P = clamp(*prefix_len, 0, pcap), pcap = min(max_prefix_pages * page_size, capacity), is read INSIDE the kernels.
// Key row j < P of every batch element is row j % page_size of page prefix_table[j / page_size]; key row j >= P is the row block_table[b]
// names. len_b, the position of a query, what it sees, n and lse are the decode call's: P moves where a key is fetched from, never
// whether it is visible.
//
// Rows. The rows of all batch elements that share a K/V head are one row space rho = b * R + r (R = G * Sq, r = g * Sq + pos as in
// fasn_kvcache.h), cut into blocks of KVS_ROWS = 128: a lane owns one row, takes its b from its own rho - rows of several batch elements
// share a wave, the rows of one may straddle two blocks - and carries the limit min(P - 1, the decode call's limit under its own len_b).
// A tile takes the unmasked branch when every lane of the wave THAT HAS A ROW sees all of it (a vote).
//
// Never read: block_table[b] entries and own cache rows of keys below P (slots wholly below P may be unset; in the tile that holds key P
// the lanes of the rows below P ask beyond the descriptor's range and get zeros), prefix-page rows at or beyond P (the descriptor of the
// last prefix tile ends at row P - 1), prefix_table entries at or beyond ceil(P / page_size), rows at or beyond len_b.
#pragma once
#include "fasn_kvcache.h"

namespace fasn {

constexpr int KVS_ROWS = 128;   // rows of a prefix-pass workgroup: one per lane of its four waves' lower and upper halves

struct KvShared {
    const int* plen;     // device, one int32
    const int* ptab;     // device, [max_prefix_pages] page ids
    int pcap;            // min(max_prefix_pages * page_size, capacity)
    int nsplit;          // splits of the prefix pass
    int nrb;             // 128-row blocks of the row space: ceil(B * R / 128)
    float* part_o;       // [Hkv][nsplit][B * R][D]
    float* part_ml;      // [Hkv][nsplit][B * R][2]
};

FASN_DEV int kvs_prefix_len(const KvShared& sh) {
    const int P = __builtin_amdgcn_readfirstlane(*sh.plen);
    return min(max(P, 0), sh.pcap);
}

// fasn_kvshared_prefix_kernel<Tag, D>(KvParams, KvShared) and fasn_kvshared_suffix_kernel<Tag, D>(KvParams, KvShared): the text of the
// decode kernel, compiled twice more (fasn_kvcache_fwd.inc, FASN_KV_SHARED = 1 / 2 with every other switch at 0).
#define FASN_KV_TREE 0
#define FASN_KV_WINDOW 0
#define FASN_KV_ALIBI 0
#define FASN_KV_FP8 0
#define FASN_KV_SHARED 1
#include "fasn_kvcache_fwd.inc"
#undef FASN_KV_SHARED
#define FASN_KV_SHARED 2
#include "fasn_kvcache_fwd.inc"
#undef FASN_KV_SHARED
#undef FASN_KV_FP8
#undef FASN_KV_ALIBI
#undef FASN_KV_WINDOW
#undef FASN_KV_TREE

// Merge the partials of a row - the suffix pass's nsplit, then the prefix pass's sh.nsplit - with the arithmetic of
// fasn_kvcache_combine_kernel and scatter it. A neutral partial (m = -inf: an empty or fully hidden range, the whole prefix pass at P = 0)
// adds nothing, so with P = 0 the sums are the decode call's, term for term. The sink sits in split 0 of the suffix pass alone.
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvshared_combine_kernel(const KvParams p, const KvShared sh) {
    using E = ET<Tag>;
    constexpr int TPR = D / 4;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rowg = gid / TPR;   // (b * Hkv + hkv, r)
    const int c4 = (int)(gid % TPR) * 4;
    if (rowg >= (int64_t)p.B * p.Hkv * p.R) return;
    const int bk = (int)(rowg / p.R), r = (int)(rowg % p.R);
    const int b = bk / p.Hkv, hkv = bk % p.Hkv, h = hkv * p.G + r / p.Sq, pos = r % p.Sq;
    const int64_t rows_all = (int64_t)p.B * p.R, rho = (int64_t)b * p.R + r;
    float mstar = -INFINITY;
    for (int s = 0; s < p.nsplit; ++s) mstar = fmaxf(mstar, p.part_ml[(((int64_t)bk * p.nsplit + s) * p.R + r) * 2]);
    for (int s = 0; s < sh.nsplit; ++s) mstar = fmaxf(mstar, sh.part_ml[(((int64_t)hkv * sh.nsplit + s) * rows_all + rho) * 2]);
    const float m_use = (mstar == -INFINITY) ? 0.f : mstar;
    float l = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < p.nsplit; ++s) {
        const int64_t base = ((int64_t)bk * p.nsplit + s) * p.R + r;
        const float ms = p.part_ml[base * 2], ls = p.part_ml[base * 2 + 1];
        if (ms == -INFINITY) continue;
        const float w = fast_exp2(ms - m_use);
        l += ls * w;
        const f32x4 a = *reinterpret_cast<const f32x4*>(p.part_o + base * D + c4);
        acc += a * w;
    }
    for (int s = 0; s < sh.nsplit; ++s) {
        const int64_t base = ((int64_t)hkv * sh.nsplit + s) * rows_all + rho;
        const float ms = sh.part_ml[base * 2], ls = sh.part_ml[base * 2 + 1];
        if (ms == -INFINITY) continue;
        const float w = fast_exp2(ms - m_use);
        l += ls * w;
        const f32x4 a = *reinterpret_cast<const f32x4*>(sh.part_o + base * D + c4);
        acc += a * w;
    }
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    typename E::vec4 y = E::cvt4(acc * inv);
    u32x2 raw;
    __builtin_memcpy(&raw, &y, 8);
    gstore8(p.o + (b * p.os[0] + h * p.os[1] + (int64_t)pos * p.os[2] + c4) * 2, raw);
    if (p.lse != nullptr && c4 == 0) p.lse[((int64_t)b * p.H + h) * p.Sq + pos] = l > 0.f ? (m_use + __builtin_log2f(l)) * kLn2 : -INFINITY;
}

}  // namespace fasn
