// fasn_kvcache.h — forward over a K/V CACHE (inference): paged or dense cache, lengths in device memory, grouped-query rows.
//
// Three kernels beside the training / prefill kernels (none of which changes):
//   fasn_kvcache_append_kernel   k_new / v_new rows -> cache rows len_b .. len_b + Sq - 1 (dropped beyond the capacity)
//   fasn_kvcache_fwd_kernel      split-K walk over the pages of one (batch element, K/V head): un-normalised partials
//   fasn_kvcache_fwd_alibi_kernel  the same walk with the ALiBi term -slope_h |j - p_i| in the scores (fasn_kvcache_fwd.inc holds both)
//   fasn_kvcache_fwd_window_kernel  the same walk over the tiles of a sliding window only: key j is visible iff p_i - W < j <= p_i
//   fasn_kvcache_fwd_tree_kernel  the same walk where the Sq new positions are the nodes of a token tree: a 64-bit word per node (KvTree)
//   fasn_kvcache_combine_kernel  merges the partials and scatters the rows back to o[b, h, pos, :] / lse[b, h, pos]
//   fasn_kvcache_tree_commit_kernel  moves the cache rows of an accepted path of a token tree behind the prefix (KvCommit)
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
constexpr int kv_nbuf(int D) { return D <= 64 ? 3 : 2; }                        // LDS tile buffers per operand (D = 32 / 64 / 128 / 256: 24 / 48 / 64 / 128 KiB of LDS)
constexpr int kv_smem(int D) { return 2 * kv_nbuf(D) * KV_KT * D * 2; }
// Workgroups per CU the forward kernels are compiled for. D = 256: two 32 KiB buffers per operand are 128 KiB of the CU's 160 - one
// workgroup, whose waves may then use the whole register file (16 accumulator blocks of O^T and the 16 Q fragments do not fit in half).
// D = 32: three 4 KiB buffers per operand (24 KiB); the registers, not the LDS, set the two workgroups the kernel is compiled for.
constexpr int kv_wg_per_cu(int D) { return D <= 128 ? 2 : 1; }
constexpr bool kv_head_dim_ok(int D) { return D == 32 || D == 64 || D == 128 || D == 256; }
// Workgroups the split rule of both calls aims at. Up to D = 128 the chip holds two to three workgroups per CU and ~1024 are four
// rounds of them. At D = 256 one workgroup fills a CU: 256 are resident, every further split is a further 128 KiB of LDS to zero, 16
// more Q fragments to fetch and a partial of D + 2 floats per row that nobody's K/V requests hide - 512 (two rounds, so that a short
// batch element's workgroups leave their CU to another's) is what the plan aims at there.
constexpr int kv_split_target(int D) { return D <= 128 ? 1024 : 512; }
// The split rule of both calls: as many splits as bring `base` workgroups to the target, each with at least min_tps of the cap_tiles
// tiles a workgroup can have to walk.
constexpr int64_t kv_nsplit(int D, int64_t base, int64_t cap_tiles, int64_t min_tps) {
    int64_t nsplit = (kv_split_target(D) + base - 1) / base;
    if (nsplit > cap_tiles / min_tps) nsplit = cap_tiles / min_tps;
    return nsplit < 1 ? 1 : nsplit;
}
// ... under a sliding window of W keys: the keys of a workgroup whose rows span `span` positions lie in W + span - 1 positions, which
// touch one tile more than they fill
constexpr int64_t kv_window_tiles(int64_t cap_tiles, int64_t W, int64_t span) {
    const int64_t t = (W + span - 1 + KV_KT - 1) / KV_KT + 1;
    return t < cap_tiles ? t : cap_tiles;
}

FASN_DEV int kv_len(const KvParams& p, int b) {
    const int len = __builtin_amdgcn_readfirstlane(p.seqlens[b]) + p.seqlen_add;
    return min(max(len, 0), p.capacity);
}

// 16 bytes per lane into LDS through a descriptor that was just built in SGPRs: as lds_dma16, with the wait states an SGPR written by
// the scalar or vector unit needs before a memory instruction reads it as a descriptor (cdna_hip_programming.md, inline-asm rule 2)
FASN_DEV void kv_dma16(u32x4 rsrc, uint32_t lds_base, uint32_t voff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lds_base), "v"(voff), "s"(rsrc) : "memory", "m0");
}

// ALiBi slopes (fasn_fwd_kvcache_alibi / fasn_fwd_kvprefill_alibi): one fp32 slope per (batch element, query head), addressed as the
// per-head n is. The logit of (row i, key j) becomes c q_i.k_j - slope2 |j - p_i| in the log2 domain, slope2 = slope log2(e),
// p_i = pos_i + len_b - qlen_b the absolute position of the query: both integers are in the kernel for the causal test already.
struct KvAlibi {
    const float* slopes;
    int sb, sh;          // element strides (batch, query head)
};

// The term of accumulator register r of key block kb: its key is k0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi, so with
// dk0 = float(k0 + 4 * hi - p_i) - one integer subtraction and one conversion per tile - the distance is |dk0 + a literal| (the absolute
// value is a source modifier): no table of per-register constants, which the D = 128 kernel has no registers for. Integers below
// 2^24 and their sums are exact in fp32: the distance is exact for every cache below 16M keys, as a converted integer would be.
FASN_DEV float kv_alibi_term(float nslope2, float dk0, int kb, int r) {
    return nslope2 * __builtin_fabsf(dk0 + (float)(kb * 32 + (r & 3) + 8 * (r >> 2)));
}

// Sliding window (fasn_fwd_kvcache_window / fasn_fwd_kvprefill_window): position p_i = pos_i + len_b - qlen_b sees the W keys
// p_i - W < j <= p_i (always causal). w = min(W, capacity) on the host: no position is beyond capacity - 1, so the clamp changes nothing
// and p - w cannot overflow. A workgroup walks the tiles from the one that holds the first key of its FIRST row's window; whatever lies
// below - cache rows, pages, block-table entries - is never read and may be gone.
struct KvWindow {
    int w;
};
// Token tree (fasn_fwd_kvcache_tree / fasn_fwd_kvprefill_tree): the qlen_b new positions of a batch element are the NODES of a tree of
// draft tokens (speculative decoding), node i in cache row base_b + i, base_b = len_b - qlen_b. Bit t of mask[b * sb + i] says that node i
// sees node t (bits at or beyond qlen_b are ignored, bit 63 is an ordinary bit); every node sees the prefix j < base_b. The position of a
// node is base_b + depth_i, depth_i = max(popcount(word & valid bits) - 1, 0): a well-formed row holds the node and its ancestors. Under
// a window a prefix key needs j > p_i - w; w is a RUN-TIME integer here, capacity + 1 (beyond every position) when there is no window:
// one tree kernel per call, not one per window. The word is read per lane inside the masked branch; nothing about memory depends on it.
struct KvTree {
    const long long* mask;   // [B][sb] words, device
    int64_t sb;              // batch stride, elements
    int w;                   // 1 .. capacity: the window; capacity + 1: none
};
// FP8 cache (fasn_fwd_kvcache_fp8 / fasn_fwd_kvprefill_fp8, kernels in fasn_kvfp8.h): a cache element is an OCP e4m3fn code whose value is
// the exact upcast of the code times one fp32 scale per (batch element, K/V head), addressed as the per-head n is. KvParams::k / v are the
// code pools and the cache strides count codes (bytes); everything else in KvParams keeps its meaning.
struct KvFp8 {
    const float* ks;     // k_scale, device
    const float* vs;     // v_scale, device
    int ksb, ksh;        // element strides (batch, K/V head)
    int vsb, vsh;
};
constexpr bool kv_fp8_head_dim_ok(int D) { return D == 64 || D == 128; }

// fasn_kvcache_fwd_kernel<Tag, D>(KvParams), fasn_kvcache_fwd_alibi_kernel<Tag, D>(KvParams, KvAlibi) and
// fasn_kvcache_fwd_window_kernel<Tag, D>(KvParams, KvWindow): one text, compiled three times.
// (A bool-templated device function behind two __global__ wrappers was tried first: the compiler then schedules and allocates the
// kernel WITHOUT the bias differently - four more VGPRs at D = 64 - and the existing instantiations are to stay byte for byte what
// they were; tools/kernel_digest.py shows they do.)
// fasn_kvcache_fwd_tree_kernel<Tag, D>(KvParams, KvTree) is the fourth compilation (FASN_KV_TREE = 1, the other two at 0).
#define FASN_KV_TREE 0
#define FASN_KV_WINDOW 0
#define FASN_KV_ALIBI 0
#include "fasn_kvcache_fwd.inc"
#undef FASN_KV_ALIBI
#define FASN_KV_ALIBI 1
#include "fasn_kvcache_fwd.inc"
#undef FASN_KV_ALIBI
#undef FASN_KV_WINDOW
#define FASN_KV_ALIBI 0
#define FASN_KV_WINDOW 1
#include "fasn_kvcache_fwd.inc"
#undef FASN_KV_WINDOW
#undef FASN_KV_TREE
#define FASN_KV_WINDOW 0
#define FASN_KV_TREE 1
#include "fasn_kvcache_fwd.inc"
#undef FASN_KV_TREE
#undef FASN_KV_WINDOW
#undef FASN_KV_ALIBI

// ---- the split merge of the K/V-cache family: the eight combine kernels (here, fasn_kvprefill.h, fasn_kvvarlen.h, fasn_kvfp8.h,
// fasn_kvprefix.h) compute their row and where its partials lie, call kv_merge, then kv_store_row and kv_lse (decode rows:
// kv_store_decode_row). One thread per (row, 4 features).
//
// A partial set is (part_o, part_ml, nsplit, at): the nsplit un-normalised partials of one row, split s at row `at(s)` of part_o [..][D]
// and part_ml [..][2]; `at` is the kernel's own index expression, so the three layouts in use stay as they are.
struct KvMerged {
    f32x4 acc;           // sum_s acc_s 2^(m_s - m*), features c4 .. c4 + 3
    float l, m_use;      // sum_s l_s 2^(m_s - m*);  m* (0 when every partial is neutral)
};
struct KvNoParts {   // the index of a set that is not there
    FASN_DEV int64_t operator()(int) const { return 0; }
};
// The merge of one set or two (the arithmetic of fasn_fwd_combine_kernel): m* = max_s m_s over the sets in the order given, then
// l = sum_s l_s 2^(m_s - m*) and acc = sum_s acc_s 2^(m_s - m*) over the sets in the same order.
template <int D, typename At1, typename At2 = KvNoParts>
FASN_DEV KvMerged kv_merge(int c4, const float* part_o1, const float* part_ml1, int nsplit1, At1 at1, const float* part_o2 = nullptr,
                           const float* part_ml2 = nullptr, int nsplit2 = 0, At2 at2 = {}) {
    float mstar = -INFINITY;
    auto take_max = [&](const float* part_ml, int nsplit, auto at) {
        for (int s = 0; s < nsplit; ++s) mstar = fmaxf(mstar, part_ml[at(s) * 2]);
    };
    take_max(part_ml1, nsplit1, at1);
    take_max(part_ml2, nsplit2, at2);
    const float m_use = (mstar == -INFINITY) ? 0.f : mstar;
    float l = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    auto add = [&](const float* part_o, const float* part_ml, int nsplit, auto at) {
        for (int s = 0; s < nsplit; ++s) {
            const int64_t base = at(s);
            const float ms = part_ml[base * 2], ls = part_ml[base * 2 + 1];
            if (ms == -INFINITY) continue;   // an empty or fully hidden range: nothing to add
            const float w = fast_exp2(ms - m_use);
            l += ls * w;
            const f32x4 a = *reinterpret_cast<const f32x4*>(part_o + base * D + c4);
            acc += a * w;
        }
    };
    add(part_o1, part_ml1, nsplit1, at1);
    add(part_o2, part_ml2, nsplit2, at2);
    return {acc, l, m_use};
}
// The store of a merged row: O = acc / l (zeros where nothing was visible) and its one rounding to oat ...
FASN_DEV f32x4 kv_merged_row(const KvMerged& m) {
    const float inv = m.l > 0.f ? 1.0f / m.l : 0.f;
    return m.acc * inv;
}
template <typename E>
FASN_DEV void kv_store_rounded(char* oat, f32x4 y4) {
    typename E::vec4 y = E::cvt4(y4);
    u32x2 raw;
    __builtin_memcpy(&raw, &y, 8);
    gstore8(oat, raw);
}
template <typename E>
FASN_DEV void kv_store_row(char* oat, const KvMerged& m) {
    kv_store_rounded<E>(oat, kv_merged_row(m));
}
// ... with v_scale (the FP8 cache's) on the normalised fp32 row, in front of the rounding
template <typename E>
FASN_DEV void kv_store_row(char* oat, const KvMerged& m, float v_scale) {
    kv_store_rounded<E>(oat, kv_merged_row(m) * v_scale);
}
// ... and the row's lse = ln(sum), which the thread of the row's first four features writes where the call has an lse
FASN_DEV float kv_lse(const KvMerged& m) { return m.l > 0.f ? (m.m_use + __builtin_log2f(m.l)) * kLn2 : -INFINITY; }
// where a decode row goes: row r of (b, hkv) is o[b, hkv * G + r / Sq, r % Sq, :] / lse[b, h, pos]
template <typename E>
FASN_DEV void kv_store_decode_row(const KvParams& p, int b, int h, int pos, int c4, const KvMerged& m) {
    kv_store_row<E>(p.o + (b * p.os[0] + h * p.os[1] + (int64_t)pos * p.os[2] + c4) * 2, m);
    if (p.lse != nullptr && c4 == 0) p.lse[((int64_t)b * p.H + h) * p.Sq + pos] = kv_lse(m);
}
template <typename E>
FASN_DEV void kv_store_decode_row(const KvParams& p, int b, int h, int pos, int c4, const KvMerged& m, float v_scale) {
    kv_store_row<E>(p.o + (b * p.os[0] + h * p.os[1] + (int64_t)pos * p.os[2] + c4) * 2, m, v_scale);
    if (p.lse != nullptr && c4 == 0) p.lse[((int64_t)b * p.H + h) * p.Sq + pos] = kv_lse(m);
}

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
    const KvMerged m = kv_merge<D>(c4, p.part_o, p.part_ml, p.nsplit, [&](int s) { return ((int64_t)bk * p.nsplit + s) * p.R + r; });
    kv_store_decode_row<E>(p, b, h, pos, c4, m);
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

// Commit of an accepted path of a token tree (fasn_kvcache_tree_commit): for k < alen_b = clamp(accepted_lens[b], 0, A) the K and V rows
// base_b + accepted[b, k] move to the rows base_b + k, base_b = seqlens[b], through the block table.
//
// Hazards. A path is strictly increasing, so accepted[b, k] >= k: row base_b + k can be the SOURCE of an earlier move (k' < k with
// accepted[b, k'] = k) and the DESTINATION of move k. One thread owns one 16-byte column chunk of one (b, hkv) in K and in V and walks
// k = 0, 1, .. upward: move k reads row accepted[k] >= k and writes row k, every later move k' > k of the thread reads a row
// accepted[k'] >= k' > k - a row no earlier move of the thread has written - and no other thread touches the thread's bytes. Program
// order inside one thread is all the ordering there is to keep: no LDS, no barrier, no second buffer. The rule is enforced, not assumed:
// a move whose index lies outside [k, nodes) is skipped, so is one whose source or destination row is negative or at / beyond the
// capacity. A malformed path therefore gives unspecified rows inside [base_b, base_b + alen_b) and never touches memory outside the
// cache; accepted[b, k] == k moves nothing. `seqlens` is not modified.
struct KvCommit {
    char* k;
    char* v;
    int64_t kps, krs, khs;            // element strides (page, row, head), as KvParams
    int64_t vps, vrs, vhs;
    const int* bt;       // block table [B][bts] or nullptr (dense: page = batch element)
    int64_t bts;
    const int* seqlens;  // [B], device: base_b
    int page_size;
    int capacity;
    int B, Hkv;
    const int* acc;      // [B][accs] node indices, device
    int64_t accs;
    const int* alens;    // [B], device
    int A;               // <= 64
    int nodes;           // node indices lie in [0, nodes)
};
template <int D>
__global__ void __launch_bounds__(256) fasn_kvcache_tree_commit_kernel(const KvCommit c) {
    constexpr int CPR = D / 8;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)c.B * c.Hkv * CPR) return;
    const int ch = (int)(gid % CPR);
    const int64_t rest = gid / CPR;
    const int hkv = (int)(rest % c.Hkv), b = (int)(rest / c.Hkv);
    const int64_t base = c.seqlens[b];
    const int alen = min(max(c.alens[b], 0), c.A);
    const int* const acc = c.acc + (int64_t)b * c.accs;
    const int* const bt = c.bt != nullptr ? c.bt + (int64_t)b * c.bts : nullptr;
    char* const kh = c.k + (int64_t)hkv * c.khs * 2 + ch * 16;
    char* const vh = c.v + (int64_t)hkv * c.vhs * 2 + ch * 16;
    for (int k = 0; k < alen; ++k) {
        const int node = acc[k];
        if (node <= k || node >= c.nodes) continue;   // (node == k: the row is where it belongs)
        const int64_t src = base + node, dst = base + k;
        if (dst < 0 || src >= c.capacity) continue;
        const int sslot = (int)(src / c.page_size), srip = (int)(src % c.page_size);
        const int dslot = (int)(dst / c.page_size), drip = (int)(dst % c.page_size);
        const int64_t spage = bt != nullptr ? bt[sslot] : b, dpage = bt != nullptr ? bt[dslot] : b;
        const u32x4 kx = gload16(kh + (spage * c.kps + (int64_t)srip * c.krs) * 2);
        const u32x4 vx = gload16(vh + (spage * c.vps + (int64_t)srip * c.vrs) * 2);
        gstore16(kh + (dpage * c.kps + (int64_t)drip * c.krs) * 2, kx);
        gstore16(vh + (dpage * c.vps + (int64_t)drip * c.vrs) * 2, vx);
    }
}

}  // namespace fasn
