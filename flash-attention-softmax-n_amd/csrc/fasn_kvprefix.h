// fasn_kvprefix.h — decode over a paged K/V cache behind SHARED PREFIXES (cascade): the prefix pages are walked once per K/V head for the
// rows of all batch elements that share them, each batch element's own suffix as the decode call walks it, and the two are merged through
// the un-normalised fp32 partials the decode path writes anyway. Two calls: ONE prefix for every batch element (KvShared), and one prefix
// per GROUP of batch elements (KvGroups: prefix groups).
//
// Kernels (none of the others changes):
//   fasn_kvshared_prefix_kernel   (K/V head, 128-row block, split): the tiles [0, ceil(P / 64)) of the pages `prefix_table` names. No sink.
//   fasn_kvshared_suffix_kernel   (batch element, K/V head, split): the tiles [P / 64, ceil(len_b / 64)) of the pages block_table[b] names,
//                                 keys below P hidden in the first tile. Split 0 carries the sink, as in fasn_kvcache_fwd_kernel.
//   fasn_kvshared_combine_kernel  merges a row's suffix partials and its prefix partials and scatters it to o / lse
//   fasn_kvgroups_schedule_kernel one workgroup: prefix_group -> the table in the call's workspace (below)
//   fasn_kvgroups_prefix_kernel   (K/V head, item, split): the tiles [0, ceil(P_g / 64)) of the pages prefix_tables[g] names, for the 128 rows
//                                 of the item. No sink.
//   fasn_kvgroups_suffix_kernel   fasn_kvshared_suffix_kernel with P = P_b, the table's entry of the batch element (0: the base call's ranges)
//   fasn_kvgroups_combine_kernel  fasn_kvshared_combine_kernel; the prefix partials are read at the sequence's slot, a sequence without a
//                                 prefix reads none
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
//
// ---- Prefix groups: the above with one prefix per group. prefix_group[b] names the prefix of batch element b, any value outside [0, G)
// means "no shared prefix"; prefix_tables [G, max_prefix_pages], prefix_lens [G] and prefix_group [B] live in device memory and are never
// read on the host.
//
// The virtual cache. For g = prefix_group[b] in [0, G): P_b = P_g = clamp(prefix_lens[g], 0, pcap); key row j < P_b is row j % page_size
// of page prefix_tables[g][j / page_size], key row j >= P_b the row block_table[b] names. For every other b, P_b = 0.
//
// The sorted row space. The grouped sequences are put in a STABLE order - by group, inside a group by batch index - and sequence number
// `slot` of that order owns the rows slot * R .. slot * R + R - 1 (R = G_heads * Sq) of the prefix partials. A group of c members has the
// c * R consecutive rows from its first member's on, cut into ceil(c * R / 128) ITEMS of 128 rows: an item never mixes groups, so the tile
// range a workgroup walks and the pages it stages are uniform. With sum ceil(x_g / 128) <= ceil(sum x_g / 128) + k - 1 over k non-empty
// groups the item count is at most items_max = ceil(B * R / 128) + min(G, B) - 1, a bound from shapes alone: the grid is
// Hkv * items_max * nsplit and items beyond the count leave before they read anything else.
//
// The table (int32, in the workspace behind the partials; include/fasn.h documents it as part of the ABI):
//   [0] item count  [1] grouped sequences  [2] [3] 0
//   [KVG_HEAD ..]           order[B]   batch element of slot s (-1 at and beyond the number of grouped sequences)
//   [KVG_HEAD + B ..]       slot[B]    slot of batch element b, -1: no prefix
//   [KVG_HEAD + 2 B ..]     plen[B]    P_b
//   [KVG_HEAD + 3 B + pad]  items[items_max][4]   (group, first row, end of the group's rows, P_g); beyond the count (-1, 0, 0, 0)
// (pad: to a multiple of four ints.) Every clamp - of prefix_lens, of prefix_group - is made ONCE, by the schedule kernel; the other three
// kernels take the table as it is: whatever the operands hold, an order entry they use is a batch index, a slot a slot of the row space, a
// group a row of prefix_tables, P_g at most pcap. Every entry is written in every call, without atomics: two runs build the same table.
//
// Never read: what is listed above, per group; and the prefix_tables row and the pages of a group without a member (no item names it).
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

constexpr int KVG_HEAD = 4;          // ints in front of the table's arrays
constexpr int KVG_ITEM = 4;          // ints per item: group, first row, end of the group's rows, P_g
constexpr int KVG_MAX_GROUPS = 1024; // three LDS counters per group in the schedule kernel: 12 KiB

struct KvGroups {
    const int* plens;    // device, [G]
    const int* ptabs;    // device, [G][mpp] page ids
    const int* pgroup;   // device, [B]
    int* tab;            // the table, in the workspace
    int G, mpp;          // groups, max_prefix_pages
    int pcap;            // min(max_prefix_pages * page_size, capacity)
    int nsplit;          // splits of the prefix pass
    int items_max;
    float* part_o;       // [Hkv][nsplit][B * R rows of the sorted row space][D]
    float* part_ml;      // [Hkv][nsplit][B * R][2]
};

constexpr int64_t kvg_items_max(int64_t B, int64_t R, int64_t G) { return (B * R + KVS_ROWS - 1) / KVS_ROWS + (G < B ? G : B) - 1; }
constexpr int64_t kvg_items_at(int64_t B) { return KVG_HEAD + (3 * B + 3) / 4 * 4; }          // ints in front of the items
constexpr int64_t kvg_table_ints(int64_t B, int64_t items_max) { return kvg_items_at(B) + items_max * KVG_ITEM; }

FASN_DEV int* kvg_order(const KvGroups& gr) { return gr.tab + KVG_HEAD; }
FASN_DEV int* kvg_slot(const KvGroups& gr, int B) { return gr.tab + KVG_HEAD + B; }
FASN_DEV int* kvg_plen(const KvGroups& gr, int B) { return gr.tab + KVG_HEAD + 2 * (int64_t)B; }
FASN_DEV int* kvg_items(const KvGroups& gr, int B) { return gr.tab + kvg_items_at(B); }

// exclusive prefix sums of (a, b) over the NT threads of the workgroup, and the totals; ws: 2 * NT / 64 ints of LDS
template <int NT>
FASN_DEV void kvg_scan2(int& a, int& b, int& ta, int& tb, int* ws) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int xa = a, xb = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int ya = __shfl_up(xa, d), yb = __shfl_up(xb, d);
        if (lane >= d) {
            xa += ya;
            xb += yb;
        }
    }
    if (lane == 63) {
        ws[2 * wave] = xa;
        ws[2 * wave + 1] = xb;
    }
    __syncthreads();
    int ba = 0, bb = 0;
    ta = 0;
    tb = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const int sa = ws[2 * w], sb = ws[2 * w + 1];
        ba += w < wave ? sa : 0;
        bb += w < wave ? sb : 0;
        ta += sa;
        tb += sb;
    }
    __syncthreads();
    a = ba + xa - a;
    b = bb + xb - b;
}

// One workgroup of NT threads. (1) NT sequences per round: the rank of a sequence among the members of its group so far - inside a wave
// by ballots over the distinct groups of the wave, across waves and rounds through a running counter per group in LDS that the waves
// update one after the other (no atomics: the order is the batch order whatever the timing). (2) The member counts and item counts of
// the groups are scanned: the first slot and first item of every group. (3) slot = first slot + rank, order, P_b. (4) One thread per item
// finds its group by binary search in the first-item array.
template <int NT>
__global__ void __launch_bounds__(NT) fasn_kvgroups_schedule_kernel(const KvParams p, const KvGroups gr) {
    constexpr int GPT = KVG_MAX_GROUPS / NT;   // groups per thread of the scan
    __shared__ int cnt[KVG_MAX_GROUPS];        // members so far; after (2) the first slot of the group
    __shared__ int ifirst[KVG_MAX_GROUPS + 1]; // first item of the group; [G] = the item count
    __shared__ int pl[KVG_MAX_GROUPS];         // P_g
    __shared__ int ws[2 * NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = p.B, G = gr.G;
    int* const order = kvg_order(gr);
    int* const slot = kvg_slot(gr, B);
    int* const plen = kvg_plen(gr, B);
    int* const items = kvg_items(gr, B);
    for (int g = tid; g < KVG_MAX_GROUPS; g += NT) {
        cnt[g] = 0;
        pl[g] = g < G ? min(max(gr.plens[g], 0), gr.pcap) : 0;
    }
    __syncthreads();
    // (1) the rank inside the group goes to slot[b] for now (-1: no prefix); the thread that writes it is the one that reads it in (3)
    for (int base = 0; base < B; base += NT) {
        const int b = base + tid;
        int g = -1;
        if (b < B) {
            const int x = gr.pgroup[b];
            g = (unsigned)x < (unsigned)G ? x : -1;
        }
        const bool member = g >= 0;
        // ballots: the lanes of the same group, the lane's rank among them, the first of them (the leader)
        int rank = 0, leader = lane, n_same = 0;
        unsigned long long todo = __ballot(member);
        while (todo != 0ull) {
            const int src = __builtin_ctzll(todo);
            const int g0 = __shfl(g, src);
            const unsigned long long same = __ballot(member && g == g0);
            if (member && g == g0) {
                rank = __builtin_popcountll(same & ((1ull << lane) - 1ull));
                leader = src;
                n_same = __builtin_popcountll(same);
            }
            todo &= ~same;
        }
        // the waves take their turns in order; the leaders of a wave have distinct groups
        int first = 0;
        for (int w = 0; w < NT / 64; ++w) {
            if (w == wave && member && leader == lane) {
                first = cnt[g];
                cnt[g] = first + n_same;
            }
            __syncthreads();
        }
        first = __shfl(first, leader);
        if (b < B) slot[b] = member ? first + rank : -1;
    }
    // (2) per thread GPT consecutive groups: members and items, scanned
    int c_loc[GPT], i_loc[GPT];
    int c_sum = 0, i_sum = 0;
#pragma unroll
    for (int j = 0; j < GPT; ++j) {
        const int c = cnt[tid * GPT + j];
        c_loc[j] = c;
        i_loc[j] = (int)(((int64_t)c * p.R + KVS_ROWS - 1) / KVS_ROWS);
        c_sum += c;
        i_sum += i_loc[j];
    }
    int c_tot, i_tot;
    kvg_scan2<NT>(c_sum, i_sum, c_tot, i_tot, ws);   // (its barriers: every cnt is read before one is overwritten)
#pragma unroll
    for (int j = 0; j < GPT; ++j) {
        cnt[tid * GPT + j] = c_sum;
        ifirst[tid * GPT + j] = i_sum;
        c_sum += c_loc[j];
        i_sum += i_loc[j];
    }
    if (tid == NT - 1) ifirst[KVG_MAX_GROUPS] = i_sum;
    __syncthreads();
    const int n_items = min(i_tot, gr.items_max);   // (i_tot <= items_max by the bound above; the min keeps a table the kernels can trust)
    // (3) slots, order, P_b
    for (int b = tid; b < B; b += NT) {
        if (b >= c_tot) order[b] = -1;
    }
    __syncthreads();   // (order is one array: the -1 of slot s and the b of slot s come from different threads)
    for (int b = tid; b < B; b += NT) {
        const int rank = slot[b];
        int s = -1, P = 0;
        if (rank >= 0) {
            const int x = gr.pgroup[b];   // in [0, G): the rank says so
            const int g = (unsigned)x < (unsigned)G ? x : 0;
            s = min(cnt[g] + rank, B - 1);
            P = pl[g];
            order[s] = b;
        }
        slot[b] = s;
        plen[b] = P;
    }
    // (4) items: the last group whose first item is at or below i (a group without members shares its first item with the next one)
    for (int i = tid; i < gr.items_max; i += NT) {
        int4 it = make_int4(-1, 0, 0, 0);
        if (i < n_items) {
            int lo = 0, hi = KVG_MAX_GROUPS;   // ifirst[lo] <= i < ifirst[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (ifirst[mid] <= i) lo = mid;
                else hi = mid;
            }
            const int g = min(lo, G - 1);
            const int s0 = cnt[g];
            const int s1 = g + 1 < KVG_MAX_GROUPS ? cnt[g + 1] : c_tot;
            it = make_int4(g, s0 * p.R + (i - ifirst[g]) * KVS_ROWS, s1 * p.R, pl[g]);
        }
        *reinterpret_cast<int4*>(items + (int64_t)i * KVG_ITEM) = it;
    }
    if (tid == 0) *reinterpret_cast<int4*>(gr.tab) = make_int4(n_items, c_tot, 0, 0);
}

// what a workgroup of the prefix pass takes from the table: its item, as the KvShared of a one-prefix call over the item's group
struct KvgItem {
    int group, row0, rend, P;
};
FASN_DEV KvgItem kvg_item(const KvGroups& gr, int B, int item) {
    const int4 it = *reinterpret_cast<const int4*>(kvg_items(gr, B) + (int64_t)item * KVG_ITEM);
    KvgItem r;
    r.group = __builtin_amdgcn_readfirstlane(it.x);
    r.row0 = __builtin_amdgcn_readfirstlane(it.y);
    r.rend = __builtin_amdgcn_readfirstlane(it.z);
    r.P = __builtin_amdgcn_readfirstlane(it.w);
    return r;
}
FASN_DEV int kvg_nitems(const KvGroups& gr) { return __builtin_amdgcn_readfirstlane(gr.tab[0]); }
FASN_DEV int kvg_prefix_len(const KvGroups& gr, int B, int b) { return __builtin_amdgcn_readfirstlane(kvg_plen(gr, B)[b]); }

// fasn_kvshared_prefix_kernel / fasn_kvshared_suffix_kernel<Tag, D>(KvParams, KvShared) and fasn_kvgroups_prefix_kernel /
// fasn_kvgroups_suffix_kernel<Tag, D>(KvParams, KvGroups): the text of the decode kernel, compiled four times more (fasn_kvcache_fwd.inc,
// FASN_KV_PASS = prefix / suffix times FASN_KV_GROUPS = 0 / 1, with every other switch at 0).
#define FASN_KV_TREE 0
#define FASN_KV_WINDOW 0
#define FASN_KV_ALIBI 0
#define FASN_KV_FP8 0
#define FASN_KV_GROUPS 0
#define FASN_KV_PASS FASN_KV_PASS_PREFIX
#include "fasn_kvcache_fwd.inc"
#undef FASN_KV_PASS
#define FASN_KV_PASS FASN_KV_PASS_SUFFIX
#include "fasn_kvcache_fwd.inc"
#undef FASN_KV_PASS
#undef FASN_KV_GROUPS
#define FASN_KV_GROUPS 1
#define FASN_KV_PASS FASN_KV_PASS_PREFIX
#include "fasn_kvcache_fwd.inc"
#undef FASN_KV_PASS
#define FASN_KV_PASS FASN_KV_PASS_SUFFIX
#include "fasn_kvcache_fwd.inc"
#undef FASN_KV_PASS
#undef FASN_KV_GROUPS
#undef FASN_KV_FP8
#undef FASN_KV_ALIBI
#undef FASN_KV_WINDOW
#undef FASN_KV_TREE

// Merge the partials of a row - the suffix pass's nsplit, then the prefix pass's - with kv_merge (fasn_kvcache.h) and scatter it. A neutral
// partial (m = -inf: an empty or fully hidden range, the whole prefix pass at P = 0) adds nothing, so with P = 0 the sums are the decode
// call's, term for term. The sink sits in split 0 of the suffix pass alone.
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
    const KvMerged m = kv_merge<D>(c4, p.part_o, p.part_ml, p.nsplit, [&](int s) { return ((int64_t)bk * p.nsplit + s) * p.R + r; },
                                   sh.part_o, sh.part_ml, sh.nsplit, [&](int s) { return ((int64_t)hkv * sh.nsplit + s) * rows_all + rho; });
    kv_store_decode_row<E>(p, b, h, pos, c4, m);
}

// ... with the prefix partials of (b, r) at row slot[b] * R + r of the sorted row space; slot -1: the suffix partials alone, which is
// fasn_kvcache_combine_kernel's sum term for term.
template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_kvgroups_combine_kernel(const KvParams p, const KvGroups gr) {
    using E = ET<Tag>;
    constexpr int TPR = D / 4;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rowg = gid / TPR;   // (b * Hkv + hkv, r)
    const int c4 = (int)(gid % TPR) * 4;
    if (rowg >= (int64_t)p.B * p.Hkv * p.R) return;
    const int bk = (int)(rowg / p.R), r = (int)(rowg % p.R);
    const int b = bk / p.Hkv, hkv = bk % p.Hkv, h = hkv * p.G + r / p.Sq, pos = r % p.Sq;
    const int sl = kvg_slot(gr, p.B)[b];
    const int nsp = sl >= 0 ? gr.nsplit : 0;   // no prefix: no prefix partial is read
    const int64_t rows_all = (int64_t)p.B * p.R, rho = (int64_t)sl * p.R + r;
    const KvMerged m = kv_merge<D>(c4, p.part_o, p.part_ml, p.nsplit, [&](int s) { return ((int64_t)bk * p.nsplit + s) * p.R + r; },
                                   gr.part_o, gr.part_ml, nsp, [&](int s) { return ((int64_t)hkv * gr.nsplit + s) * rows_all + rho; });
    kv_store_decode_row<E>(p, b, h, pos, c4, m);
}

}  // namespace fasn
