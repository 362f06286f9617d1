// fasn_kvcache_fwd.inc - the text of the decode forward kernel, included by fasn_kvcache.h once per variant (no include guard):
// FASN_KV_ALIBI / FASN_KV_WINDOW = 0 / 0, 1 / 0, 0 / 1. With both at 0 the preprocessor leaves fasn_kvcache_fwd_kernel exactly as it was
// before the variants existed, and with FASN_KV_WINDOW == 0 the ALiBi kernel as it was before the window kernel did.
// FASN_KV_TREE = 1 (with the other two at 0; undefined counts as 0) is the token-tree sibling: the new positions see the prefix and the
// nodes their word of `tree.mask` names, the window is a run-time integer. With FASN_KV_TREE == 0 the three kernels above are what they were.
// FASN_KV_FP8 = 1 (fasn_kvfp8.h, with the other three at 0; undefined counts as 0) is the sibling over a cache of e4m3fn codes (KvFp8): a tile
// is staged as D-byte rows, widened by all four waves into the 16-bit tile image the fragment reads take, and k_scale rides in the score
// factor. With FASN_KV_FP8 == 0 the four kernels above are what they were.
// FASN_KV_FP8 is orthogonal to FASN_KV_WINDOW: both at 1 (fasn_kvfp8.h) is the sliding-window sibling over the FP8 cache - the window's tile
// range, full-tile test and one-compare mask around the FP8 staging and widening. The score factor has ONE name for that, FASN_KV_SC:
// c8 under FASN_KV_FP8, p.c otherwise (a macro, so that the kernels that were there keep their tokens).
// FASN_KV_FP8 is orthogonal to FASN_KV_TREE in the same way: both at 1 (fasn_kvfp8.h) is the token-tree sibling over the FP8 cache - the tree's
// tile range, full-tile test and per-lane visibility word around the FP8 staging and widening, FASN_KV_SC in both arms of the masked loop.
// FASN_KV_PASS = FASN_KV_PASS_PREFIX / FASN_KV_PASS_SUFFIX (fasn_kvprefix.h, with the other four at 0; undefined counts as 0: no pass) are the
// two passes of the calls behind shared prefixes: the prefix pass walks the tiles [0, ceil(P / 64)) of the prefix pages for 128 rows of a row
// space of ALL batch elements, every lane with the b of its own row and the limit min(P - 1, its base limit), no sink; the suffix pass is the
// base walk over the tiles [P / 64, ceil(len_b / 64)) of the batch element's own pages, keys below P hidden in the first tile.
// FASN_KV_GROUPS is orthogonal to FASN_KV_PASS: at 1 the prefix is the one of the batch element's GROUP - the prefix pass takes its rows,
// its pages and P_g from an item of the schedule table, the suffix pass P_b from the table. With FASN_KV_PASS == 0 the eight kernels above
// are what they were.
#define FASN_KV_PASS_PREFIX 1
#define FASN_KV_PASS_SUFFIX 2
#if FASN_KV_FP8
#define FASN_KV_SC c8
#else
#define FASN_KV_SC p.c
#endif
template <typename Tag, int D>
#if FASN_KV_PASS == FASN_KV_PASS_PREFIX && FASN_KV_GROUPS
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvgroups_prefix_kernel(const KvParams p, const KvGroups gr) {
#elif FASN_KV_PASS == FASN_KV_PASS_SUFFIX && FASN_KV_GROUPS
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvgroups_suffix_kernel(const KvParams p, const KvGroups gr) {
#elif FASN_KV_PASS == FASN_KV_PASS_PREFIX
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvshared_prefix_kernel(const KvParams p, const KvShared sh) {
#elif FASN_KV_PASS == FASN_KV_PASS_SUFFIX
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvshared_suffix_kernel(const KvParams p, const KvShared sh) {
#elif FASN_KV_FP8 && FASN_KV_TREE
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvcache_fwd_fp8_tree_kernel(const KvParams p, const KvFp8 f8, const KvTree tree) {
#elif FASN_KV_FP8 && FASN_KV_WINDOW
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvcache_fwd_fp8_window_kernel(const KvParams p, const KvFp8 f8, const KvWindow win) {
#elif FASN_KV_FP8
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvcache_fwd_fp8_kernel(const KvParams p, const KvFp8 f8) {
#elif FASN_KV_TREE
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvcache_fwd_tree_kernel(const KvParams p, const KvTree tree) {
#elif FASN_KV_ALIBI
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvcache_fwd_alibi_kernel(const KvParams p, const KvAlibi al) {
#elif FASN_KV_WINDOW
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvcache_fwd_window_kernel(const KvParams p, const KvWindow win) {
#else
__global__ void __launch_bounds__(256, kv_wg_per_cu(D)) fasn_kvcache_fwd_kernel(const KvParams p) {
#endif
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
    // what is staged: the tile as the cache holds it, EB bytes per element (the image of 16-bit rows itself unless the cache holds fp8 codes)
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

    const int wg = (int)blockIdx.x;
#if FASN_KV_PASS == FASN_KV_PASS_PREFIX
#if FASN_KV_GROUPS
    // (K/V head, item, split); an item beyond the table's count leaves before it reads anything else. The item names the group, the first
    // of its 128 rows of the sorted row space, where the group's rows end and P_g; the lane's row decides its slot, the order table its b.
    // From here on the workgroup is a prefix pass behind ONE prefix: `sh` is that call's operand, `len` is what the walk covers, P_g
    const int split = wg % gr.nsplit;
    const int bk = wg / gr.nsplit;         // hkv * items_max + item
    const int hkv = bk / gr.items_max;
    if (bk - hkv * gr.items_max >= kvg_nitems(gr)) return;
    const KvgItem item = kvg_item(gr, p.B, bk - hkv * gr.items_max);
    KvShared sh;
    sh.ptab = gr.ptabs + (int64_t)item.group * gr.mpp;
    sh.nsplit = gr.nsplit;
    sh.part_o = gr.part_o;
    sh.part_ml = gr.part_ml;
    const int rho = item.row0 + (tid >> 6) * 32 + (tid & 31);
    const int rows_all = p.B * p.R;
    const bool row_ok = rho < item.rend;
    const int slot = row_ok ? rho / p.R : 0;
    int b = 0;
    if (row_ok) b = kvg_order(gr)[slot];
    const int len = item.P;
#else
    // (K/V head, row block, split); the lane's row of the row space rho = b * R + r decides its b. `len` is what the walk covers: P
    const int split = wg % sh.nsplit;
    const int bk = wg / sh.nsplit;         // hkv * nrb + row block
    const int hkv = bk / sh.nrb;
    const int rho = (bk - hkv * sh.nrb) * KVS_ROWS + (tid >> 6) * 32 + (tid & 31);
    const int rows_all = p.B * p.R;
    const int b = rho < rows_all ? rho / p.R : 0;
    const int len = kvs_prefix_len(sh);
#endif
#else
    const int split = wg % p.nsplit;
    const int bk = wg / p.nsplit;          // b * Hkv + hkv
    const int b = bk / p.Hkv, hkv = bk % p.Hkv;

    // ---- this split's tile range, from the length in device memory
    const int len = kv_len(p, b);
#endif
    const int tiles_b = (len + KV_KT - 1) / KV_KT;
#if FASN_KV_PASS == FASN_KV_PASS_PREFIX
    const int tps = (tiles_b + sh.nsplit - 1) / sh.nsplit;
    const int t0 = min(split * tps, tiles_b);
#elif FASN_KV_PASS == FASN_KV_PASS_SUFFIX
    // the walk starts at the tile that holds key P: the base call's split rule over [tlo, tiles_b), the base call's ranges at P = 0. Tiles
    // below tlo get no request and no table read: their slots may be unset
#if FASN_KV_GROUPS
    const int P = kvg_prefix_len(gr, p.B, b);   // P_b: the schedule kernel's clamp of the length of the batch element's group, 0 without one
#else
    const int P = kvs_prefix_len(sh);
#endif
    const int tlo = min(P / KV_KT, tiles_b);
    const int tps = (tiles_b - tlo + p.nsplit - 1) / p.nsplit;
    const int t0 = min(tlo + split * tps, tiles_b);
#elif FASN_KV_TREE
    // node i sits in cache row base + i; the walk starts at the tile of the first key a node at depth 0 can see under the window (no
    // window: tree.w is beyond the capacity and tlo is 0, the base kernel's split of [0, tiles_b))
    const int base = len - p.Sq;
    const int tlo = min(max(0, base - tree.w + 1) / KV_KT, tiles_b);
    const int tps = (tiles_b - tlo + p.nsplit - 1) / p.nsplit;
    const int t0 = min(tlo + split * tps, tiles_b);
#elif FASN_KV_WINDOW
    // the walk starts at the tile of the first key that the FIRST row's window holds; the splits share [tlo, tiles_b). Tiles below tlo
    // get no request and no table read: their pages may be gone
    const int tlo = min(max(0, len - p.Sq - win.w + 1) / KV_KT, tiles_b);
    const int tps = (tiles_b - tlo + p.nsplit - 1) / p.nsplit;
    const int t0 = min(tlo + split * tps, tiles_b);
#else
    const int tps = (tiles_b + p.nsplit - 1) / p.nsplit;
    const int t0 = min(split * tps, tiles_b);
#endif
    const int t1 = min(t0 + tps, tiles_b);

    // ---- the lane's row: query head of the group, position, softmax_n, causal limit
#if FASN_KV_PASS == FASN_KV_PASS_PREFIX
#if FASN_KV_GROUPS
    const int r_b = row_ok ? rho - slot * p.R : 0;   // the row inside the lane's own batch element
#else
    const bool row_ok = rho < rows_all;
    const int r_b = row_ok ? rho - b * p.R : 0;   // the row inside the lane's own batch element
#endif
    const int g = r_b / p.Sq;
    const int pos = r_b - g * p.Sq;
    const int h = hkv * p.G + g;
    // the lane's own len_b: a vector load, retired in front of the tile loop (a lane without a row reads nothing)
    int len_l = 0;
    if (row_ok) len_l = p.seqlens[b];
#else
    const int row = wave * 32 + l31;
    const bool row_ok = row < p.R;
    const int g = row_ok ? row / p.Sq : 0;
    const int pos = row_ok ? row - g * p.Sq : 0;
    const int h = hkv * p.G + g;
    float n_row = p.n;
    if (p.nt != nullptr) n_row = p.nt[b * p.nsb + h * p.nsh];
#endif
#if FASN_KV_ALIBI
    float nslope2 = al.slopes[b * al.sb + h * al.sh] * -kLog2e;   // -slope * log2(e) of the row's query head: lane-private, read once, like n
#endif
#if FASN_KV_FP8
    float c8 = p.c * f8.ks[b * f8.ksb + hkv * f8.ksh];   // k_scale acts on the fp32 scores: one uniform load in front of the tile loop, like n
#endif
#if FASN_KV_PASS == FASN_KV_PASS_PREFIX && FASN_KV_GROUPS
    const bool wave_rows = item.row0 + wave * 32 < item.rend;   // the last item of a group may be mostly idle
#elif FASN_KV_PASS == FASN_KV_PASS_PREFIX
    const bool wave_rows = (bk - hkv * sh.nrb) * KVS_ROWS + wave * 32 < rows_all;   // the last row block may be mostly idle
#else
    const bool wave_rows = wave * 32 < p.R;   // a wave without rows only helps staging
#endif

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
    // Page ids are wave-uniform and the table does not change while the kernel runs: read through the constant address space they are
    // scalar loads whose wait the compiler places at the first use - the NEXT tile's request - instead of vector loads whose wait
    // would drain the K/V requests just issued. Entries of tiles outside the range are never read.
#if FASN_KV_PASS == FASN_KV_PASS_PREFIX
    // the prefix pages: one table for every batch element; entries at or beyond ceil(P / page_size) belong to no tile of the range
    const __attribute__((address_space(4))) int* const bt_row = (const __attribute__((address_space(4))) int*)sh.ptab;
    auto page_of = [&](int tile, int slot) -> int {
        if (tile >= t1) return 0;
        return bt_row[slot];
    };
#else
    const __attribute__((address_space(4))) int* const bt_row = (const __attribute__((address_space(4))) int*)(p.bt + (int64_t)b * p.bts);
    const bool paged = p.bt != nullptr;
    auto page_of = [&](int tile, int slot) -> int {
        if (tile >= t1) return 0;
        return paged ? bt_row[slot] : b;
    };
#endif
    int u_page = page_of(u, u_slot);
    auto request_next = [&](int buf) {
        const int nvis = u < t1 ? min(KV_KT, len - u * KV_KT) : 0;   // rows of the tile below len_b (>= 1 inside the range)
        const int64_t koff = ((int64_t)u_page * p.kps + (int64_t)u_tip * KV_KT * p.krs) * EB;
        const int64_t voff = ((int64_t)u_page * p.vps + (int64_t)u_tip * KV_KT * p.vrs) * EB;
        const uint32_t kbytes = nvis > 0 ? (uint32_t)((nvis - 1) * (int)p.krs * EB + SROWB) : 0u;
        const uint32_t vbytes = nvis > 0 ? (uint32_t)((nvis - 1) * (int)p.vrs * EB + SROWB) : 0u;
        const u32x4 krw = make_rsrc_words(kpool + koff, kbytes), vrw = make_rsrc_words(vpool + voff, vbytes);
#if FASN_KV_PASS == FASN_KV_PASS_SUFFIX
        // the tile that holds key P: its rows below P are the batch element's own rows of a partially shared page and may hold anything.
        // Their lanes ask beyond every range a descriptor can have (kv_build: a tile spans less than 2^31 bytes) and get zeros
        const int lo = u == tlo ? P - tlo * KV_KT : 0;
#pragma unroll
        for (int i = 0; i < SNLD; ++i) {
            const bool below = (tid + i * NT) / SCPR < lo;
            kv_dma16(krw, __builtin_amdgcn_readfirstlane(ldsK_w + buf * STILEB + i * NT * 16), below ? 0x80000000u : kvoff[i]);
            kv_dma16(vrw, __builtin_amdgcn_readfirstlane(ldsV_w + buf * STILEB + i * NT * 16), below ? 0x80000000u : vvoff[i]);
        }
#else
#pragma unroll
        for (int i = 0; i < SNLD; ++i) {
            kv_dma16(krw, __builtin_amdgcn_readfirstlane(ldsK_w + buf * STILEB + i * NT * 16), kvoff[i]);
            kv_dma16(vrw, __builtin_amdgcn_readfirstlane(ldsV_w + buf * STILEB + i * NT * 16), vvoff[i]);
        }
#endif
        ++u;
        if (++u_tip == p.tpp) {
            u_tip = 0;
            ++u_slot;
        }
        u_page = page_of(u, u_slot);   // the next tile's page id is on its way while this one's data is
    };

    // ---- online-softmax state of the row (log2 domain); the sink (+n) belongs to split 0
#if FASN_KV_PASS == FASN_KV_PASS_PREFIX
    float m_run = -INFINITY;   // (no sink here: it belongs to split 0 of the suffix pass)
    float l_run = 0.f;
#else
    const bool sink = n_row > 0.f && split == 0;
    float m_run = sink ? 0.f : -INFINITY;
    float l_run = (sink && hi == 0) ? n_row : 0.f;   // the two half-lanes' partial sums are added at the end
#endif
    f32x16 oacc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
#if FASN_KV_PASS == FASN_KV_PASS_PREFIX
    // last visible key of the row: the base call's limit under the lane's own len_b, and below P
    len_l = min(max(len_l + p.seqlen_add, 0), p.capacity);
    int vis = !row_ok ? -1 : min(len - 1, p.causal ? pos + len_l - p.Sq : len_l - 1);
    retire_loads(vis);
#elif !FASN_KV_TREE
    const int vis = !row_ok ? -1 : (p.causal ? pos + len - p.Sq : len - 1);   // last visible key of the row
    const int all_vis = p.causal ? len - p.Sq : len - 1;                          // every row sees the keys up to here
#endif

#pragma unroll
    for (int s = 0; s < KS; ++s) retire_loads(qf[s]);
#if FASN_KV_PASS != FASN_KV_PASS_PREFIX
    retire_loads(n_row);
#endif
#if FASN_KV_ALIBI
    retire_loads(nslope2);
    const int qpos = pos + len - p.Sq;   // absolute position of the row's query
#endif
#if FASN_KV_FP8
    retire_loads(c8);
#endif

    // ---- the tile buffers start as zeros: a request that is out of range for its descriptor must leave nothing behind that is not
    // a finite number, whether the hardware fills the slot with zeros or leaves it alone (afterwards a slot holds zeros or visible rows)
    for (int i = tid; i < 2 * NBUF * STILEB / 16; i += NT) *LDS_PTR(u32x4, smem + i * 16) = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    // ---- prologue: NBUF - 1 tiles in flight
#pragma unroll
    for (int i = 0; i < NBUF - 1; ++i) request_next(i);

    int buf = 0;
    for (int t = t0; t < t1; ++t) {
        // tile t has landed (this wave's share: the NBUF - 2 younger tiles may still be in flight), then everybody's share has, and
        // everybody is done with tile t - 1, whose buffer takes the next request
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NBUF - 2) * 2 * SNLD) : "memory");
        __syncthreads();
        request_next(buf == 0 ? NBUF - 1 : buf - 1);
#if FASN_KV_FP8
        // everybody is done with the image of tile t - 1 (the barrier above) and with the codes of tile t - 1 (widened before the barrier
        // below, one tile ago): all four waves widen tile t, rows or not, then everybody's share of the image is there
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
            // scores in the log2 domain; hidden keys (beyond the row's causal limit, which is below len_b) at -inf
            float mx = -INFINITY;
#if FASN_KV_ALIBI
            // the bias is part of the score before the maximum is taken; k0 is the absolute key index in every split
            const float dk0 = (float)(k0 + 4 * hi - qpos);
#endif
#if FASN_KV_PASS == FASN_KV_PASS_PREFIX
            // every lane that has a row sees the whole tile (the rows of a wave belong to several batch elements: a vote, wave-uniform)
            if (__all(!row_ok || k0 + KV_KT - 1 <= vis)) {
#elif FASN_KV_PASS == FASN_KV_PASS_SUFFIX
            // ... and the tile holds no key below P
            if (k0 + KV_KT - 1 <= all_vis && k0 >= P) {
#elif FASN_KV_TREE
            // the tile lies wholly in the prefix and wholly inside the window of the deepest position a node can have, base + Sq - 1:
            // conservative for every depth, every row sees the whole tile
            if (k0 + KV_KT - 1 < base && k0 > len - 1 - tree.w) {
#elif FASN_KV_WINDOW
            // ... and not below the window of the LAST row, len - W, either: then every row's window holds the whole tile
            if (k0 + KV_KT - 1 <= all_vis && k0 >= len - win.w) {
#else
            if (k0 + KV_KT - 1 <= all_vis) {   // wave-uniform (lanes without a row carry zero queries; their state is never stored)
#endif
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
#if FASN_KV_ALIBI
                        sacc[kb][r] = __builtin_fmaf(sacc[kb][r], p.c, kv_alibi_term(nslope2, dk0, kb, r));
#else
                        sacc[kb][r] *= FASN_KV_SC;
#endif
                        mx = fmaxf(mx, sacc[kb][r]);
                    }
            } else {
#if FASN_KV_TREE
                // The row's word and depth are fetched HERE, not in front of the tile loop: at most two tiles per workgroup take this
                // branch (those that touch [base, len) or the window's lower edge) and three more registers across the loop are what the
                // D = 128 kernel does not have. Bits at or beyond Sq are dropped, so a key at or beyond len is hidden by construction;
                // a lane without a row sees nothing of the tree. p_row = base + depth is the position the window is taken at.
                unsigned long long word = 0ull;
                if (row_ok) word = (unsigned long long)tree.mask[b * tree.sb + pos] & (~0ull >> (64 - p.Sq));
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
                // vis - W < key <= vis as ONE unsigned compare of the distance vis - key, which is dvis minus the register's literal (a
                // lane without a row has vis = -1: its distances wrap beyond every W). dvis is made opaque per tile, or the compiler
                // hoists the 32 loop-invariant parts of the distances out of the loop and keeps them in registers across it.
                int dvis = vis - k0 - 4 * hi;
                asm volatile("" : "+v"(dvis));
#endif
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = k0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
#if FASN_KV_PASS == FASN_KV_PASS_SUFFIX
                        const float y = key <= vis && key >= P ? sacc[kb][r] * FASN_KV_SC : -INFINITY;
#elif FASN_KV_TREE
                        const float y = ((vm >> (kb * 32 + (r & 3) + 8 * (r >> 2))) & 1ull) != 0ull ? sacc[kb][r] * FASN_KV_SC : -INFINITY;
#elif FASN_KV_ALIBI
                        const float y = key <= vis ? __builtin_fmaf(sacc[kb][r], p.c, kv_alibi_term(nslope2, dk0, kb, r)) : -INFINITY;
#elif FASN_KV_WINDOW
                        const float y = (unsigned)(dvis - (kb * 32 + (r & 3) + 8 * (r >> 2))) < (unsigned)win.w ? sacc[kb][r] * FASN_KV_SC : -INFINITY;
#else
                        const float y = key <= vis ? sacc[kb][r] * FASN_KV_SC : -INFINITY;
#endif
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
#if FASN_KV_PASS == FASN_KV_PASS_PREFIX
    // the prefix partials: [Hkv][nsplit][B * R rows of the row space][D] and [...][2]; `row` becomes the row of that space
    float* po = sh.part_o + ((int64_t)hkv * sh.nsplit + split) * rows_all * D;
    float* pml = sh.part_ml + ((int64_t)hkv * sh.nsplit + split) * rows_all * 2;
    const int row = rho;
#else
    float* po = p.part_o + ((int64_t)bk * p.nsplit + split) * p.R * D;
    float* pml = p.part_ml + ((int64_t)bk * p.nsplit + split) * p.R * 2;
#endif
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
#undef FASN_KV_SC
#undef FASN_KV_PASS_PREFIX
#undef FASN_KV_PASS_SUFFIX
