// fasn_kvprefill_fwd.inc - the text of the prefill forward kernel, included by fasn_kvprefill.h once per variant (no include guard):
// FASN_KV_ALIBI / FASN_KV_WINDOW = 0 / 0, 1 / 0, 0 / 1. With both at 0 the preprocessor leaves fasn_kvprefill_fwd_kernel exactly as it
// was before the variants existed, and with FASN_KV_WINDOW == 0 the ALiBi kernel as it was before the window kernel did.
// FASN_KV_PACKED = 1 (fasn_kvvarlen.h, with the other two at 0) is the token-packed sibling: its (sequence, row block) comes from the item
// table of fasn_kvvarlen_schedule_kernel, not from the grid, and its rows are tokens of one [T, H, D] buffer. With FASN_KV_PACKED == 0
// the three kernels above are what they were. The switch is orthogonal to the other two: FASN_KV_PACKED = 1 with FASN_KV_WINDOW = 1
// (fasn_kvvarlen.h) is the packed window sibling - the body's window blocks read qlen, len, pos0 and pos_hi, which the packed branch
// defines from the item - and a packed ALiBi sibling would be one more inclusion.
// FASN_KV_TREE = 1 (fasn_kvprefill.h, with the other three at 0; undefined counts as 0) is the token-tree sibling (fasn_kvcache.h: KvTree):
// every row block walks to len_b, because a node may see any node. With FASN_KV_TREE == 0 the kernels above are what they were.
// FASN_KV_FP8 = 1 (fasn_kvfp8.h, with the other four at 0; undefined counts as 0) is the sibling over a cache of e4m3fn codes (fasn_kvcache.h:
// KvFp8; fasn_kvcache_fwd.inc: staging, widening pass); v_scale multiplies the one-split direct store. With FASN_KV_FP8 == 0 the kernels
// above are what they were. FASN_KV_FP8 = 1 with FASN_KV_WINDOW = 1 (fasn_kvfp8.h) is the sliding-window sibling over the FP8 cache: the
// window blocks of the body are orthogonal to the FP8 blocks. FASN_KV_SC is the score factor's one name (fasn_kvcache_fwd.inc).
// FASN_KV_FP8 = 1 with FASN_KV_TREE = 1 (fasn_kvfp8.h) is the token-tree sibling over the FP8 cache, by the same orthogonality.
// FASN_KV_FP8 = 1 with FASN_KV_PACKED = 1 (fasn_kvfp8.h; FASN_KV_WINDOW = 0 / 1) are the token-packed siblings over the FP8 cache: the
// packed blocks say where the item, the rows and the partial slot come from, the FP8 blocks what is staged, widened and scaled - the
// scales are read at the item's b. No block of the text carries both switches.
#if FASN_KV_FP8
#define FASN_KV_SC c8
#else
#define FASN_KV_SC p.c
#endif
template <typename Tag, int D>
#if FASN_KV_FP8 && FASN_KV_PACKED && FASN_KV_WINDOW
FASN_KV_LOCAL __global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvvarlen_fwd_window_fp8_kernel(const KvPrefillParams pp, const KvPacked pk, const KvFp8 f8, const KvWindow win) {
#elif FASN_KV_FP8 && FASN_KV_PACKED
FASN_KV_LOCAL __global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvvarlen_fwd_fp8_kernel(const KvPrefillParams pp, const KvPacked pk, const KvFp8 f8) {
#elif FASN_KV_FP8 && FASN_KV_TREE
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvprefill_fwd_fp8_tree_kernel(const KvPrefillParams pp, const KvFp8 f8, const KvTree tree) {
#elif FASN_KV_FP8 && FASN_KV_WINDOW
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvprefill_fwd_fp8_window_kernel(const KvPrefillParams pp, const KvFp8 f8, const KvWindow win) {
#elif FASN_KV_FP8
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvprefill_fwd_fp8_kernel(const KvPrefillParams pp, const KvFp8 f8) {
#elif FASN_KV_TREE
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvprefill_fwd_tree_kernel(const KvPrefillParams pp, const KvTree tree) {
#elif FASN_KV_PACKED && FASN_KV_WINDOW
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvvarlen_fwd_window_kernel(const KvPrefillParams pp, const KvPacked pk, const KvWindow win) {
#elif FASN_KV_PACKED
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvvarlen_fwd_kernel(const KvPrefillParams pp, const KvPacked pk) {
#elif FASN_KV_ALIBI
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvprefill_fwd_alibi_kernel(const KvPrefillParams pp, const KvAlibi al) {
#elif FASN_KV_WINDOW
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvprefill_fwd_window_kernel(const KvPrefillParams pp, const KvWindow win) {
#else
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvprefill_fwd_kernel(const KvPrefillParams pp) {
#endif
    using E = ET<Tag>;
    using vec8 = typename E::vec8;
    const KvParams& p = pp.kv;
    constexpr int NT = 256;
    constexpr int NBUF = kv_nbuf(D);
    constexpr int ROWB = D * 2;
    constexpr int TILEB = KV_KT * ROWB;
    constexpr int KS = D / 16;
    constexpr int DB = D / 32;
    constexpr int CPR = D / 8;
    constexpr int NLD = (KV_KT * CPR) / NT;
    // what is staged: the tile as the cache holds it, EB bytes per element (fasn_kvcache_fwd.inc)
#if FASN_KV_FP8
    constexpr int EB = 1;
#else
    constexpr int EB = 2;
#endif
    constexpr int SROWB = D * EB;
    constexpr int STILEB = KV_KT * SROWB;
    constexpr int SCPR = SROWB / 16;
    constexpr int SNLD = (KV_KT * SCPR) / NT;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const ldsK = smem;
    char* const ldsV = smem + NBUF * STILEB;
#if FASN_KV_FP8
    char* const imgK = smem + 2 * NBUF * STILEB;   // the one 16-bit tile image per operand that the staged codes are widened into
    char* const imgV = imgK + TILEB;
#endif

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int hi = lane >> 5;

#if FASN_KV_PACKED
    // ---- (item, K/V head, split): splits of a block are neighbours, the K/V heads of an item follow each other. The item - sequence,
    // row block, first token and query length of the sequence, clamped by the schedule kernel - is read wave-uniform, as kvp_qlen is;
    // a workgroup beyond the item count leaves before it reads anything else
    const int wg = (int)blockIdx.x;
    const int split = wg % p.nsplit;
    const int rest = wg / p.nsplit;
    const int hkv = rest % p.Hkv;
    const int item = rest / p.Hkv;
    if (item >= __builtin_amdgcn_readfirstlane(pk.sched[0])) return;
    const int* const it = pk.sched + KVV_HEAD + item * KVV_ITEM;
    const int b = __builtin_amdgcn_readfirstlane(it[0]);
    const int rb = __builtin_amdgcn_readfirstlane(it[1]);
    const int token0 = __builtin_amdgcn_readfirstlane(it[2]);
    const int qlen = __builtin_amdgcn_readfirstlane(it[3]);   // >= 1, rb * PB < qlen, token0 + qlen <= T
    const int pos0 = rb * pp.PB;

    // ---- the lane's row slot: a packed buffer has no padding rows, a slot beyond qlen_b is a neighbouring sequence's token and is
    // neither read nor written
    const int row = wave * 32 + l31;
    const int g = row / pp.PB;
    const int pos = pos0 + (row - g * pp.PB);
    const bool slot_ok = g < p.G && pos < qlen;
    const int h = hkv * p.G + (slot_ok ? g : 0);
    const int64_t tok = slot_ok ? token0 + pos : token0;
    const int64_t lse_at = (int64_t)h * pk.T + tok;
    char* const orow = p.o + (h * p.os[1] + tok * p.os[2]) * 2;
#else
    // ---- (batch element, K/V head, row block, split): splits of a block are neighbours, the last row block comes first
    const int wg = (int)blockIdx.x;
    const int split = wg % p.nsplit;
    const int rest = wg / p.nsplit;
    const int BK = p.B * p.Hkv;
    const int bk = rest % BK;              // b * Hkv + hkv
    const int rb = pp.nrb - 1 - rest / BK;
    const int b = bk / p.Hkv, hkv = bk % p.Hkv;
    const int pos0 = rb * pp.PB;

    // ---- the lane's row slot
    const int row = wave * 32 + l31;
    const int g = row / pp.PB;
    const int pos = pos0 + (row - g * pp.PB);
    const bool slot_ok = g < p.G && pos < p.Sq;    // the slot is a row of the output
    const int h = hkv * p.G + (slot_ok ? g : 0);
    const int64_t lse_at = ((int64_t)b * p.H + h) * p.Sq + pos;
    char* const orow = p.o + (b * p.os[0] + h * p.os[1] + (int64_t)pos * p.os[2]) * 2;

    const int qlen = kvp_qlen(pp, b);
    if (pos0 >= qlen) {
        // padding only: nothing of the cache, the table or the lengths beyond qlen_b is needed (several splits: the combine kernel writes
        // the padding rows, it never reads a partial of theirs)
        if (p.nsplit == 1 && slot_ok) {
#pragma unroll
            for (int i = 0; i < D / 16; ++i) gstore16(orow + hi * (D) + i * 16, u32x4{0u, 0u, 0u, 0u});   // each half-lane: one half of the row
            if (p.lse != nullptr && hi == 0) p.lse[lse_at] = -INFINITY;
        }
        return;
    }
#endif
    const int len = kvp_len(pp, b, qlen);
    const bool row_ok = slot_ok && pos < qlen;    // a real position

    // ---- the block's key range, from the lengths in device memory, and this split's share of it
#if FASN_KV_TREE
    // node i sits in cache row base + i and may see any node: the block's keys end at len_b, whatever its positions are. The walk starts
    // at the tile of the first key a node at depth 0 can see under the window (no window: tree.w is beyond the capacity and tlo is 0)
    const int base = len - qlen;
    const int tiles_b = (len + KV_KT - 1) / KV_KT;
    const int tlo = min(max(0, base - tree.w + 1) / KV_KT, tiles_b);
    const int tps = (tiles_b - tlo + p.nsplit - 1) / p.nsplit;
    const int t0 = min(tlo + split * tps, tiles_b);
#else
    const int pos_hi = min(pos0 + pp.PB, qlen) - 1;
    const int kend = p.causal ? max(0, min(len, pos_hi + len - qlen + 1)) : len;
    const int tiles_b = (kend + KV_KT - 1) / KV_KT;
#endif
#if FASN_KV_TREE
#elif FASN_KV_WINDOW
    // the walk starts at the tile of the first key that the window of the block's FIRST position holds; the splits share
    // [tlo, tiles_b). Tiles below tlo get no request and no table read: their pages may be gone
    const int tlo = min(max(0, pos0 + len - qlen - win.w + 1) / KV_KT, tiles_b);
    const int tps = (tiles_b - tlo + p.nsplit - 1) / p.nsplit;
    const int t0 = min(tlo + split * tps, tiles_b);
#else
    const int tps = (tiles_b + p.nsplit - 1) / p.nsplit;
    const int t0 = min(split * tps, tiles_b);
#endif
    const int t1 = min(t0 + tps, tiles_b);

    float n_row = p.n;
    if (p.nt != nullptr) n_row = p.nt[b * p.nsb + h * p.nsh];
#if FASN_KV_ALIBI
    float nslope2 = al.slopes[b * al.sb + h * al.sh] * -kLog2e;   // -slope * log2(e) of the slot's query head: lane-private, read once, like n
#endif
#if FASN_KV_FP8
    float c8 = p.c * f8.ks[b * f8.ksb + hkv * f8.ksh];   // k_scale acts on the fp32 scores: one uniform load in front of the tile loop, like n
#endif
    const bool wave_rows = wave * 32 < p.G * pp.PB;   // a wave without row slots only helps staging

    vec8 qf[KS];
    {
#if FASN_KV_PACKED
        const char* rp = p.q + (h * p.qs[1] + tok * p.qs[2]) * 2 + hi * 16;
#else
        const char* rp = p.q + (b * p.qs[0] + h * p.qs[1] + (int64_t)pos * p.qs[2]) * 2 + hi * 16;
#endif
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            u32x4 raw = {0u, 0u, 0u, 0u};
            if (row_ok) raw = gload16(rp + s * 32);
            __builtin_memcpy(&qf[s], &raw, 16);
        }
    }

    // ---- staging: thread tid fills slots tid + i * 256 of the tile image (slot = 16 bytes; the chunk that belongs there after the swizzle)
    unsigned kvoff[SNLD], vvoff[SNLD];
#pragma unroll
    for (int i = 0; i < SNLD; ++i) {
        const int ci = tid + i * NT;
#if FASN_KV_FP8
        const int r = ci / SCPR, ch = ci % SCPR;   // the staged codes lie as in the cache: the widening pass applies the swizzle
#else
        const int r = ci / CPR, ch = (ci % CPR) ^ swz_f<D>(r);
#endif
        kvoff[i] = (unsigned)(r * (int)p.krs * EB + ch * 16);
        vvoff[i] = (unsigned)(r * (int)p.vrs * EB + ch * 16);
    }
    const uint32_t ldsK_w = lds_addr(ldsK) + wave * 1024, ldsV_w = lds_addr(ldsV) + wave * 1024;
    const char* const kpool = p.k + (int64_t)hkv * p.khs * EB;
    const char* const vpool = p.v + (int64_t)hkv * p.vhs * EB;

    // the tile that is requested next: its index, page slot and tile inside the page advance together (no division in the loop)
    int u = t0;
    int u_slot = t0 / p.tpp;
    int u_tip = t0 - u_slot * p.tpp;
    // page ids: scalar loads through the constant address space (fasn_kvcache.h); entries of tiles outside the range are never read
    const __attribute__((address_space(4))) int* const bt_row = (const __attribute__((address_space(4))) int*)(p.bt + (int64_t)b * p.bts);
    const bool paged = p.bt != nullptr;
    auto page_of = [&](int tile, int slot) -> int {
        if (tile >= t1) return 0;
        return paged ? bt_row[slot] : b;
    };
    int u_page = page_of(u, u_slot);
    auto request_next = [&](int buf) {
        const int nvis = u < t1 ? min(KV_KT, len - u * KV_KT) : 0;   // rows of the tile below len_b (>= 1 inside the range)
        const int64_t koff = ((int64_t)u_page * p.kps + (int64_t)u_tip * KV_KT * p.krs) * EB;
        const int64_t voff = ((int64_t)u_page * p.vps + (int64_t)u_tip * KV_KT * p.vrs) * EB;
        const uint32_t kbytes = nvis > 0 ? (uint32_t)((nvis - 1) * (int)p.krs * EB + SROWB) : 0u;
        const uint32_t vbytes = nvis > 0 ? (uint32_t)((nvis - 1) * (int)p.vrs * EB + SROWB) : 0u;
        const u32x4 krw = make_rsrc_words(kpool + koff, kbytes), vrw = make_rsrc_words(vpool + voff, vbytes);
#pragma unroll
        for (int i = 0; i < SNLD; ++i) {
            kv_dma16(krw, __builtin_amdgcn_readfirstlane(ldsK_w + buf * STILEB + i * NT * 16), kvoff[i]);
            kv_dma16(vrw, __builtin_amdgcn_readfirstlane(ldsV_w + buf * STILEB + i * NT * 16), vvoff[i]);
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
#if !FASN_KV_TREE
    const int vis = !row_ok ? -1 : (p.causal ? pos + len - qlen : len - 1);   // last visible key of the row
    const int all_vis = p.causal ? pos0 + len - qlen : len - 1;                // every real row of the block sees the keys up to here
#endif

#pragma unroll
    for (int s = 0; s < KS; ++s) retire_loads(qf[s]);
    retire_loads(n_row);
#if FASN_KV_ALIBI
    retire_loads(nslope2);
    const int qpos = pos + len - qlen;   // absolute position of the slot's query
#endif
    // The scale rides in the exponential's argument: x = 2^(s c - m) is one fma per score in front of v_exp, the maximum is taken over the
    // raw scores and scaled once per tile - the per-score multiply of the decode kernel is gone and nothing is rounded that was not before
    // (Q pre-scaled in registers, fasn_fwd_kernel.h's way, rounds q c to bf16: the lse gate of the cache tests does not hold then).
    // That needs c > 0 (max commutes, -inf stays -inf); any other scale multiplies the scores in place and runs with ce = 1.
#if FASN_KV_ALIBI
    // ALiBi: a row's maximum must be taken over s c + bias, which no maximum over raw scores gives (the bias differs from key to key).
    // The biased score y = fma(s, c, bias) replaces s in place, for any sign of c - fasn_kvcache_fwd_kernel's element pass with its
    // multiply turned into an fma - and the rest runs as the c <= 0 path does, with ce = 1: fma(y, 1, -m) is y - m exactly.
    constexpr float ce = 1.0f;
#elif FASN_KV_FP8
    retire_loads(c8);
    const bool cpos = c8 > 0.f;
    const float ce = cpos ? c8 : 1.0f;
#else
    const bool cpos = p.c > 0.f;
    const float ce = cpos ? p.c : 1.0f;
#endif

    // ---- the tile buffers start as zeros (fasn_kvcache.h: an out-of-range request must leave nothing behind that is not finite)
    for (int i = tid; i < 2 * NBUF * STILEB / 16; i += NT) *LDS_PTR(u32x4, smem + i * 16) = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    // ---- prologue: NBUF - 1 tiles in flight
#pragma unroll
    for (int i = 0; i < NBUF - 1; ++i) request_next(i);

    int buf = 0;
    for (int t = t0; t < t1; ++t) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NBUF - 2) * 2 * SNLD) : "memory");
        __syncthreads();
        request_next(buf == 0 ? NBUF - 1 : buf - 1);
#if FASN_KV_FP8
        // all four waves widen tile t into the image, between two barriers (fasn_kvcache_fwd.inc)
        kv_fp8_widen<E, D>(ldsK + buf * STILEB, imgK, tid);
        kv_fp8_widen<E, D>(ldsV + buf * STILEB, imgV, tid);
        __syncthreads();
#endif
        if (wave_rows) {
#if FASN_KV_FP8
            const char* tK = imgK;
            const char* tV = imgV;
#else
            const char* tK = ldsK + buf * TILEB;
            const char* tV = ldsV + buf * TILEB;
#endif
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
#if FASN_KV_ALIBI
            {
                const float dk0 = (float)(k0 + 4 * hi - qpos);   // k0 is the absolute key index in every split
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sacc[kb][r] = __builtin_fmaf(sacc[kb][r], p.c, kv_alibi_term(nslope2, dk0, kb, r));
            }
#else
            if (!cpos) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sacc[kb][r] *= FASN_KV_SC;
            }
#endif
            // raw scores (times ce: log2 domain); hidden keys (beyond the row's limit, which is below len_b) go to -inf
            float mx = -INFINITY;
#if FASN_KV_TREE
            // the tile lies wholly in the prefix and wholly inside the window of the deepest position a node can have, len - 1
            // (fasn_kvcache_fwd.inc): every row sees the whole tile
            if (k0 + KV_KT - 1 < base && k0 > len - 1 - tree.w) {
#elif FASN_KV_WINDOW
            // ... and not below the window of the block's LAST real position either: then every row's window holds the whole tile
            if (k0 + KV_KT - 1 <= all_vis && k0 > pos_hi + len - qlen - win.w) {
#else
            if (k0 + KV_KT - 1 <= all_vis) {   // block-uniform (padding slots carry zero queries; their state is never stored)
#endif
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[kb][r]);
            } else {
#if FASN_KV_TREE
                // the row's word and depth, fetched inside the branch that at most two tiles of a workgroup take (fasn_kvcache_fwd.inc);
                // bits at or beyond qlen_b are dropped, a padding slot sees nothing of the tree
                unsigned long long word = 0ull;
                if (row_ok) word = (unsigned long long)tree.mask[b * tree.sb + pos] & (~0ull >> (64 - qlen));
                const int p_row = base + max(__builtin_popcountll(word) - 1, 0);
                // The lane's 64 visibility bits of this tile, bit c = key k0 + c, built once: the word moved into the tile's frame (node t is
                // key base + t; what falls off either end belongs to another tile) and the tile's prefix keys c < base - k0 that the
                // window of p_row holds, c >= p_row - w + 1 - k0. A score then costs one bit test on a literal position.
                const int off = base - k0;
                unsigned long long vm = off >= 0 ? (off < 64 ? word << off : 0ull) : (off > -64 ? word >> -off : 0ull);
                const int phi = min(off, 64), plo = max(p_row - tree.w + 1 - k0, 0);
                if (phi > plo) vm |= (~0ull >> (64 - (phi - plo))) << plo;
                vm >>= 4 * hi;
#elif FASN_KV_WINDOW
                // vis - W < key <= vis as one unsigned compare of the distance dvis - literal, dvis opaque per tile (fasn_kvcache_fwd.inc)
                int dvis = vis - k0 - 4 * hi;
                asm volatile("" : "+v"(dvis));
#endif
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = k0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
#if FASN_KV_TREE
                        const float y = ((vm >> (kb * 32 + (r & 3) + 8 * (r >> 2))) & 1ull) != 0ull ? sacc[kb][r] : -INFINITY;
#elif FASN_KV_WINDOW
                        const float y = (unsigned)(dvis - (kb * 32 + (r & 3) + 8 * (r >> 2))) < (unsigned)win.w ? sacc[kb][r] : -INFINITY;
#else
                        const float y = key <= vis ? sacc[kb][r] : -INFINITY;
#endif
                        sacc[kb][r] = y;
                        mx = fmaxf(mx, y);
                    }
            }
            mx = max_across_halves(mx) * ce;
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
                        x[e] = fast_exp2(__builtin_fmaf(sacc[kb][8 * t2 + e], ce, -m_use));
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

    const float l_tot = sum_across_halves(l_run);
    if (p.nsplit == 1) {
        // ---- the only split: normalise and store. Padding positions of a live block (qlen_b <= pos < Sq) store exact zeros / -inf.
        if (slot_ok) {
#if FASN_KV_FP8
            // v_scale acts on the fp32 output, in front of its one rounding: folded into the row's factor
            const float inv = (row_ok && l_tot > 0.f) ? f8.vs[b * f8.vsb + hkv * f8.vsh] / l_tot : 0.f;
#else
            const float inv = (row_ok && l_tot > 0.f) ? 1.0f / l_tot : 0.f;
#endif
            if (!row_ok) {
#pragma unroll
                for (int d = 0; d < DB; ++d)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
            }
#pragma unroll
            for (int d = 0; d < DB; ++d) store_block_narrow<E>(orow + d * 64, oacc[d], inv, hi);
            if (p.lse != nullptr && hi == 0) {
                const float m_use = (m_run == -INFINITY) ? 0.f : m_run;
                p.lse[lse_at] = (row_ok && l_tot > 0.f) ? (m_use + __builtin_log2f(l_tot)) * kLn2 : -INFINITY;
            }
        }
        return;
    }
    // ---- several splits: the partial of this key range, un-normalised accumulator + (m, l) per row slot
#if FASN_KV_PACKED
    const int64_t part = ((int64_t)item * p.Hkv + hkv) * p.nsplit + split;
#else
    const int64_t part = ((int64_t)bk * pp.nrb + rb) * p.nsplit + split;
#endif
    float* po = p.part_o + part * KVP_ROWS * D;
    float* pml = p.part_ml + part * KVP_ROWS * 2;
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
#undef FASN_KV_SC
