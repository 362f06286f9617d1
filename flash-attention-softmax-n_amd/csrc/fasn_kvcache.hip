// K/V-cache forward (include/fasn.h: fasn_fwd_kvcache[_alibi|_window|_tree], fasn_kvcache_append, fasn_kvcache[_alibi|_window|_tree]_plan,
// fasn_kvcache_tree_commit), in two parts:
//   1. the host layer of the whole K/V-cache family (fasn_kv_host.h declares it; fasn_kvprefill.hip, fasn_kvvarlen.hip, fasn_kvfp8.hip and
//      fasn_kvrope.hip call it): argument checks, parameter packing, the launch plan - which depends on shapes and capacity only, never on
//      the lengths in device memory - the check of a call's operand set (kv_build_ops: FP8, tree, window, ALiBi, in this order), the
//      workspace rule, the one forward / plan path of every call and the token-tree commit;
//   2. the decode entry points and the launches of fasn_kvcache.h.
#include <limits.h>
#include <math.h>
#include "fasn_kv_host.h"

namespace fasn {

int kv_check_view(const fasn_view4& v) {
    if (v.ptr == nullptr) return FASN_EINVAL;
    if (v.stride[3] != 1) return FASN_ESTRIDE;
    if (!kv_aligned16(v.ptr)) return FASN_EALIGN;
    for (int i = 0; i < 3; ++i)
        if (v.stride[i] % 8 != 0) return FASN_EALIGN;
    return FASN_OK;
}

namespace {
// a split costs its partial (R rows of D + 2 floats, written and read back) next to its tiles (64 keys of K and V): at least 4 tiles
// per split of a full cache, R / 8 when there are many rows (128 rows - every prefill: the partial moves what 4 tiles do, 16 tiles)
int64_t kv_min_tps(int R) { return R / 8 > 4 ? R / 8 : 4; }
}  // namespace

// Validation (no HIP call) + the kernel parameters, for decode, prefill and the rotary append. The plan: one workgroup per (batch
// element, K/V head, row block, split); as many splits as bring the grid to ~1024 workgroups (the split-K forward's target; ~512 at
// D = 256, kv_split_target), each with enough tiles of a FULL cache to pay for its partial - so a prefill whose row blocks fill the
// chip has one split, no partials and no combine launch. Head dims: 32, 64, 128, 256 (kv_head_dim_ok).
// The order of the checks decides which code a block that breaks two rules gets: tests/golden/kvhost_matrix.txt pins it.
int kv_build(const KvArgs& in, KvPrefillParams& pp, KvPacked* pk) {
    const fasn_kvcache_args* a = in.a;
    const bool prefill = in.call != KV_DECODE;   // (the packed call is a prefill)
    if (a == nullptr) return FASN_EINVAL;
    if (a->B <= 0 || a->H <= 0 || a->Sq <= 0 || a->D <= 0 || a->page_size <= 0) return FASN_EINVAL;
    if (a->dtype != FASN_DTYPE_F16 && a->dtype != FASN_DTYPE_BF16) return FASN_EDTYPE;
    if (!kv_head_dim_ok(a->D)) return FASN_EHEADDIM;
    const int G = a->kv_group <= 1 ? 1 : a->kv_group;
    if (a->H % G != 0) return FASN_EINVAL;
    if (!(a->softmax_n >= 0.f) || !isfinite(a->scale)) return FASN_EINVAL;
    if (a->seqlens == nullptr || a->k_cache == nullptr || a->v_cache == nullptr) return FASN_EINVAL;
    // (q_seqlens: prefill only, a decode block has none)
    if (reinterpret_cast<uintptr_t>(a->seqlens) % 4 || reinterpret_cast<uintptr_t>(a->block_table) % 4 || reinterpret_cast<uintptr_t>(in.q_seqlens) % 4) return FASN_EALIGN;
    // prefill adds qlen_b, which the host does not know: seqlen_add is a flag there (0: the cache as it is; Sq: plus the qlen_b appended
    // rows). Decode adds the number itself, whatever it is.
    if (prefill && a->seqlen_add != 0 && a->seqlen_add != a->Sq) return FASN_EINVAL;
    int rc;
    if ((rc = kv_check_view(a->q))) return rc;
    if ((rc = kv_check_view(a->o))) return rc;
    if (!kv_aligned16(a->k_cache) || !kv_aligned16(a->v_cache)) return FASN_EALIGN;
    for (int i = 0; i < 3; ++i)
        if (a->k_stride[i] % 8 != 0 || a->v_stride[i] % 8 != 0 || a->k_stride[i] < 0 || a->v_stride[i] < 0) return FASN_EALIGN;
    const bool paged = a->block_table != nullptr;
    if (paged && (a->max_pages <= 0 || a->block_table_stride < a->max_pages)) return FASN_EINVAL;
    if (paged && a->page_size % KV_KT != 0) return FASN_EUNSUPPORTED;   // a 64-key tile never straddles a page
    // decode: the rows of a K/V head are one pass of one workgroup; prefill: its query heads share one workgroup
    if ((prefill ? (int64_t)G : (int64_t)G * a->Sq) > KVP_ROWS) return FASN_EUNSUPPORTED;
    const int64_t capacity = paged ? (int64_t)a->max_pages * a->page_size : (int64_t)a->page_size;
    // the most a kernel adds to a length: seqlen_add (decode), up to Sq (prefill - bounded so even where seqlen_add is 0: kept as it was)
    const int64_t added = prefill ? a->Sq : a->seqlen_add;
    if (capacity > INT_MAX - 2 * KV_KT || added + capacity > INT_MAX) return FASN_EINVAL;
    // a tile's descriptor range and the lanes' offsets into it are 32-bit
    if ((int64_t)KV_KT * a->k_stride[1] * 2 >= (1ll << 31) || (int64_t)KV_KT * a->v_stride[1] * 2 >= (1ll << 31)) return FASN_EUNSUPPORTED;
    if (a->k_stride[1] < a->D || a->v_stride[1] < a->D) return FASN_EINVAL;
    if (a->n != nullptr) {
        if (reinterpret_cast<uintptr_t>(a->n) % 4) return FASN_EALIGN;
        if (a->n_stride_b < 0 || a->n_stride_h < 0 || (a->B - 1) * a->n_stride_b + (a->H - 1) * a->n_stride_h >= (1ll << 31)) return FASN_EINVAL;
    }
    pp = KvPrefillParams{};
    KvParams& p = pp.kv;
    p.q = static_cast<const char*>(a->q.ptr);
    p.o = static_cast<char*>(a->o.ptr);
    p.lse = a->lse;
    p.k = static_cast<char*>(a->k_cache);
    p.v = static_cast<char*>(a->v_cache);
    for (int i = 0; i < 3; ++i) {
        p.qs[i] = a->q.stride[i];
        p.os[i] = a->o.stride[i];
    }
    p.kps = a->k_stride[0], p.krs = a->k_stride[1], p.khs = a->k_stride[2];
    p.vps = a->v_stride[0], p.vrs = a->v_stride[1], p.vhs = a->v_stride[2];
    p.bt = a->block_table;
    p.bts = a->block_table_stride;
    p.seqlens = a->seqlens;
    p.seqlen_add = a->seqlen_add;
    p.page_size = a->page_size;
    p.tpp = paged ? a->page_size / KV_KT : INT_MAX;
    p.capacity = (int)capacity;
    p.B = a->B, p.H = a->H, p.G = G, p.Hkv = a->H / G, p.Sq = a->Sq;
    p.R = prefill ? KVP_ROWS : G * a->Sq;
    p.causal = a->causal ? 1 : 0;
    p.c = a->scale * kLog2e;
    p.n = a->softmax_n;
    p.nt = a->n;
    p.nsb = (int)a->n_stride_b, p.nsh = (int)a->n_stride_h;
    pp.qlens = in.q_seqlens;
    pp.PB = prefill ? KVP_ROWS / G : a->Sq;
    pp.nrb = (a->Sq + pp.PB - 1) / pp.PB;   // (decode: 1)
    int64_t base = (int64_t)p.B * p.Hkv * pp.nrb;
    if (in.call == KV_VARLEN) {
        // The packed operands, behind every base rule: B sequences whose lengths come from cu_seqlens_q alone, in a buffer of
        // total_tokens rows. The grid follows the item table's bound, not B * nrb: one split count for the whole launch.
        const fasn_kvvarlen_args* va = in.packed;
        if (va->cu_seqlens_q == nullptr || in.q_seqlens != nullptr || va->total_tokens <= 0 || va->reserved != 0 || pk == nullptr) return FASN_EINVAL;
        if (reinterpret_cast<uintptr_t>(va->cu_seqlens_q) % 4) return FASN_EALIGN;
        const int64_t items_max = kvv_items_max(p.B, p.Sq, va->total_tokens, pp.PB);
        if (items_max * p.Hkv > INT_MAX / KVP_ROWS) return FASN_EINVAL;
        *pk = KvPacked{va->cu_seqlens_q, nullptr, va->total_tokens, (int)items_max};
        base = items_max * p.Hkv;
    }
    const int64_t cap_tiles = (capacity + KV_KT - 1) / KV_KT;
    p.nsplit = (int)kv_nsplit(a->D, base, cap_tiles, kv_min_tps(p.R));
    if (base * p.nsplit > (prefill ? INT_MAX / KVP_ROWS : INT_MAX)) return FASN_EINVAL;   // (prefill: times the row slots of a workgroup)
    return FASN_OK;
}

int kv_pack_new(const fasn_view4& k_new, const fasn_view4& v_new, KvParams& p) {
    int rc;
    if ((rc = kv_check_view(k_new))) return rc;
    if ((rc = kv_check_view(v_new))) return rc;
    p.kn = static_cast<const char*>(k_new.ptr);
    p.vn = static_cast<const char*>(v_new.ptr);
    for (int i = 0; i < 3; ++i) {
        p.kns[i] = k_new.stride[i];
        p.vns[i] = v_new.stride[i];
    }
    return FASN_OK;
}

int kv_build_append(const KvArgs& in, const fasn_view4* k_new, const fasn_view4* v_new, KvPrefillParams& pp, KvPacked* pk) {
    const int rc = kv_build(in, pp, pk);
    if (rc) return rc;
    if (k_new == nullptr || v_new == nullptr) return FASN_EINVAL;
    return kv_pack_new(*k_new, *v_new, pp.kv);
}

// The tree operand of the *_tree entry points (checked after the base arguments, before any HIP call). The kernels take the window as a
// run-time integer: capacity + 1 - beyond every position - stands for "none" and for every window at or beyond the capacity.
int kv_check_tree(const fasn_kvcache_args* a, const fasn_kv_tree* t, int capacity, KvTree& kt) {
    if (t == nullptr || t->mask == nullptr || t->reserved != 0) return FASN_EINVAL;
    if (a->Sq > 64) return FASN_EUNSUPPORTED;   // one 64-bit word per node
    if (!a->causal) return FASN_EUNSUPPORTED;
    if (t->window < 0 || t->batch_stride < 0) return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(t->mask) % 8) return FASN_EALIGN;
    kt = KvTree{reinterpret_cast<const long long*>(t->mask), t->batch_stride, t->window >= 1 && t->window <= capacity ? t->window : capacity + 1};
    return FASN_OK;
}

// The FP8 operand of the *_fp8 entry points (checked after the base arguments, before any HIP call). The base checks hold a 16-bit cache
// to strides % 8 elements; here an element is a byte, so the same 16-byte rule is strides % 16. The scales follow the rules of `n`, per
// K/V head.
int kv_check_fp8(const fasn_kvcache_args* a, const fasn_kv_fp8* o, KvFp8& f8) {
    if (o == nullptr || o->k_scale == nullptr || o->v_scale == nullptr || o->reserved != 0) return FASN_EINVAL;
    if (!kv_fp8_head_dim_ok(a->D)) return FASN_EHEADDIM;
    if (reinterpret_cast<uintptr_t>(o->k_scale) % 4 || reinterpret_cast<uintptr_t>(o->v_scale) % 4) return FASN_EALIGN;
    for (int i = 0; i < 3; ++i)
        if (a->k_stride[i] % 16 != 0 || a->v_stride[i] % 16 != 0) return FASN_EALIGN;
    const int Hkv = a->H / (a->kv_group <= 1 ? 1 : a->kv_group);
    if (o->k_sb < 0 || o->k_sh < 0 || (a->B - 1) * o->k_sb + (Hkv - 1) * o->k_sh >= (1ll << 31)) return FASN_EINVAL;
    if (o->v_sb < 0 || o->v_sh < 0 || (a->B - 1) * o->v_sb + (Hkv - 1) * o->v_sh >= (1ll << 31)) return FASN_EINVAL;
    f8 = KvFp8{o->k_scale, o->v_scale, (int)o->k_sb, (int)o->k_sh, (int)o->v_sb, (int)o->v_sh};
    return FASN_OK;
}

namespace {

// The plan under a tree: the base call's rule; with a window the window call's rule over the tiles the windows of the Sq nodes can touch
// (every row block walks them all: span Sq, whatever PB is), never more splits than the base plan has.
int kv_build_tree(const fasn_kvcache_args* a, const fasn_kv_tree* t, int64_t blocks, KvPrefillParams& pp, KvTree& kt) {
    KvParams& p = pp.kv;
    const int rc = kv_check_tree(a, t, p.capacity, kt);
    if (rc) return rc;
    if (t->window >= 1) {
        const int64_t cap_tiles = ((int64_t)p.capacity + KV_KT - 1) / KV_KT;
        p.nsplit = (int)kv_nsplit(a->D, blocks, kv_window_tiles(cap_tiles, t->window, a->Sq), kv_min_tps(p.R));
    }
    return FASN_OK;
}

// The ALiBi operand of the *_alibi entry points (checked after the base arguments, before any HIP call): the rules of `n`
int kv_build_alibi(const fasn_kvcache_args* a, const fasn_alibi_slopes* s, KvAlibi& al) {
    if (s == nullptr || s->slopes == nullptr) return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(s->slopes) % 4) return FASN_EALIGN;
    if (s->stride_b < 0 || s->stride_h < 0 || (a->B - 1) * s->stride_b + (a->H - 1) * s->stride_h >= (1ll << 31)) return FASN_EINVAL;
    al = KvAlibi{s->slopes, (int)s->stride_b, (int)s->stride_h};
    return FASN_OK;
}

// The window operand of the *_window entry points (checked after the base arguments, before any HIP call), and the plan under it: the
// base rule over the tiles the window of a workgroup's rows can touch - they span PB positions - never more splits than the base plan has.
// `blocks`: the (K/V head, row block) blocks of the launch, B * Hkv * nrb or, on packed queries, items_max * Hkv.
int kv_build_window(const fasn_kvcache_args* a, const fasn_kv_window* w, int64_t blocks, KvPrefillParams& pp, KvWindow& kw) {
    KvParams& p = pp.kv;
    if (w == nullptr || w->window < 1 || w->reserved != 0) return FASN_EINVAL;
    if (!a->causal) return FASN_EUNSUPPORTED;
    kw = KvWindow{w->window < p.capacity ? w->window : p.capacity};
    const int64_t cap_tiles = ((int64_t)p.capacity + KV_KT - 1) / KV_KT;
    p.nsplit = (int)kv_nsplit(a->D, blocks, kv_window_tiles(cap_tiles, w->window, pp.PB), kv_min_tps(p.R));
    return FASN_OK;
}

// Behind the base checks: is there a kernel for this operand set (kv_ops_supported), then each operand the entry point takes, at most
// once and in ONE order - FP8, tree, window, ALiBi. The window's and the tree's plan count the same blocks.
int kv_build_ops(const KvArgs& in, const KvOps& o, KvFwd& f) {
    f.pk = KvPacked{};
    int rc = kv_build(in, f.pp, &f.pk);
    if (rc) return rc;
    f.ops = o.takes, f.dtype = in.a->dtype, f.D = in.a->D;
    f.al = KvAlibi{};
    f.kw = KvWindow{};
    f.kt = KvTree{};
    f.f8 = KvFp8{};
    if (!kv_ops_supported(in.call, o.takes)) return FASN_EUNSUPPORTED;
    const int64_t blocks = in.call == KV_VARLEN ? (int64_t)f.pk.items_max * f.pp.kv.Hkv : (int64_t)f.pp.kv.B * f.pp.kv.Hkv * f.pp.nrb;
    if ((o.takes & KV_OP_FP8) && (rc = kv_check_fp8(in.a, o.fp8, f.f8))) return rc;
    if ((o.takes & KV_OP_TREE) && (rc = kv_build_tree(in.a, o.tree, blocks, f.pp, f.kt))) return rc;
    if ((o.takes & KV_OP_WINDOW) && (rc = kv_build_window(in.a, o.window, blocks, f.pp, f.kw))) return rc;
    if ((o.takes & KV_OP_ALIBI) && (rc = kv_build_alibi(in.a, o.alibi, f.al))) return rc;
    return FASN_OK;
}

// the split partials: [B * Hkv * nrb][nsplit][R][D] and [...][R][2] floats. Decode always writes them and combines; a prefill of one
// split stores o / lse itself and needs none. The packed call: [items_max * Hkv] blocks, behind the item table it always has.
size_t kv_part_elems(KvCall call, const KvFwd& f) {
    const KvPrefillParams& pp = f.pp;
    const size_t blocks = call == KV_VARLEN ? (size_t)f.pk.items_max * pp.kv.Hkv : (size_t)pp.kv.B * pp.kv.Hkv * pp.nrb;
    return blocks * pp.kv.nsplit * pp.kv.R;
}
size_t kv_sched_bytes(KvCall call, const KvFwd& f) { return call == KV_VARLEN ? ((size_t)KVV_HEAD + (size_t)KVV_ITEM * f.pk.items_max) * sizeof(int) : 0; }
size_t kv_ws_bytes(KvCall call, const KvFwd& f, int D) {
    if (call != KV_DECODE && f.pp.kv.nsplit <= 1) return kv_sched_bytes(call, f);
    return kv_sched_bytes(call, f) + kv_part_elems(call, f) * (size_t)(D + 2) * sizeof(float);
}

// everything a forward does before its launches: base checks, the operands, then the workspace
int kv_build_forward(const KvArgs& in, const KvOps& ops, void* workspace, size_t workspace_bytes, KvFwd& f) {
    const int rc = kv_build_ops(in, ops, f);
    if (rc) return rc;
    const size_t need = kv_ws_bytes(in.call, f, in.a->D);
    if (need > 0) {   // (nothing to write beside o / lse: a NULL workspace is fine)
        if (workspace == nullptr || workspace_bytes < need) return FASN_EWORKSPACE;
        if (!kv_aligned16(workspace)) return FASN_EALIGN;
        const size_t sched = kv_sched_bytes(in.call, f);   // (a multiple of 16 bytes: the partials stay aligned)
        if (sched > 0) f.pk.sched = static_cast<int*>(workspace);
        f.pp.kv.part_o = reinterpret_cast<float*>(static_cast<char*>(workspace) + sched);
        f.pp.kv.part_ml = f.pp.kv.part_o + kv_part_elems(in.call, f) * in.a->D;
    }
    return FASN_OK;
}

}  // namespace

size_t kv_workspace_bytes(const KvArgs& in, const KvOps& ops) {
    KvFwd f;
    if (kv_build_ops(in, ops, f) != FASN_OK) return 0;
    return kv_ws_bytes(in.call, f, in.a->D);
}

int kv_forward(const KvArgs& in, const KvOps& ops, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    KvFwd f;
    const int rc = kv_build_forward(in, ops, workspace, workspace_bytes, f);
    if (rc) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const bool fp8 = (f.ops & KV_OP_FP8) != 0;
    if (in.call == KV_VARLEN) return fp8 ? kv_launch_fp8_packed(f, s) : kv_launch_packed(f, s);
    if (in.call == KV_PREFILL) return fp8 ? kv_launch_fp8_prefill(f, s) : kv_launch_prefill(f, s);
    return fp8 ? kv_launch_fp8_decode(f, s) : kv_launch_decode(f, s);
}

int kv_forward_plan(const KvArgs& in, const KvOps& ops, char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return kv_forward(in, ops, plan_workspace(), ~size_t(0), nullptr); });
}

// fasn_kvcache_tree_commit / fasn_kvcache_fp8_tree_commit: the cache's rules as kv_build states them for the members this block has (an FP8
// cache: and kv_check_fp8's head dims and 16-byte stride rule, where the 16-bit rule stands), then its own operands
int kv_build_commit(const fasn_kv_tree_commit* a, bool fp8, KvCommit& c) {
    if (a == nullptr) return FASN_EINVAL;
    if (a->B <= 0 || a->Hkv <= 0 || a->D <= 0 || a->page_size <= 0) return FASN_EINVAL;
    if (!kv_head_dim_ok(a->D) || (fp8 && !kv_fp8_head_dim_ok(a->D))) return FASN_EHEADDIM;
    if (a->seqlens == nullptr || a->k_cache == nullptr || a->v_cache == nullptr) return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(a->seqlens) % 4 || reinterpret_cast<uintptr_t>(a->block_table) % 4) return FASN_EALIGN;
    if (!kv_aligned16(a->k_cache) || !kv_aligned16(a->v_cache)) return FASN_EALIGN;
    const int64_t smul = fp8 ? 16 : 8;
    for (int i = 0; i < 3; ++i)
        if (a->k_stride[i] % smul != 0 || a->v_stride[i] % smul != 0 || a->k_stride[i] < 0 || a->v_stride[i] < 0) return FASN_EALIGN;
    const bool paged = a->block_table != nullptr;
    if (paged && (a->max_pages <= 0 || a->block_table_stride < a->max_pages)) return FASN_EINVAL;
    if (paged && a->page_size % KV_KT != 0) return FASN_EUNSUPPORTED;
    const int64_t capacity = paged ? (int64_t)a->max_pages * a->page_size : (int64_t)a->page_size;
    if (capacity > INT_MAX - 2 * KV_KT) return FASN_EINVAL;
    if (a->k_stride[1] < a->D || a->v_stride[1] < a->D) return FASN_EINVAL;
    if (a->accepted == nullptr || a->accepted_lens == nullptr || a->reserved != 0) return FASN_EINVAL;
    if (a->A > 64 || a->nodes > 64) return FASN_EUNSUPPORTED;
    if (a->A < 1 || a->nodes < 1 || a->accepted_stride < a->A) return FASN_EINVAL;
    if (reinterpret_cast<uintptr_t>(a->accepted) % 4 || reinterpret_cast<uintptr_t>(a->accepted_lens) % 4) return FASN_EALIGN;
    c = KvCommit{};
    c.k = static_cast<char*>(a->k_cache);
    c.v = static_cast<char*>(a->v_cache);
    c.kps = a->k_stride[0], c.krs = a->k_stride[1], c.khs = a->k_stride[2];
    c.vps = a->v_stride[0], c.vrs = a->v_stride[1], c.vhs = a->v_stride[2];
    c.bt = a->block_table;
    c.bts = a->block_table_stride;
    c.seqlens = a->seqlens;
    c.page_size = a->page_size;
    c.capacity = (int)capacity;
    c.B = a->B, c.Hkv = a->Hkv;
    c.acc = a->accepted;
    c.accs = a->accepted_stride;
    c.alens = a->accepted_lens;
    c.A = a->A;
    c.nodes = a->nodes;
    return FASN_OK;
}

int kv_commit(const fasn_kv_tree_commit* a, bool fp8, fasn_stream_t stream) {
    KvCommit c{};
    const int rc = kv_build_commit(a, fp8, c);
    if (rc) return rc;
    const int64_t nthr = (int64_t)c.B * c.Hkv * (a->D / (fp8 ? 16 : 8));
    if ((nthr + 255) / 256 > INT_MAX) return FASN_EINVAL;
    const unsigned grid = (unsigned)((nthr + 255) / 256);
    return fp8 ? kv_launch_fp8_commit(c, a->D, grid, (hipStream_t)stream) : kv_launch_commit(c, a->D, grid, (hipStream_t)stream);
}

namespace {

template <typename Tag, int D>
int kv_launch_decode_as(const KvFwd& f, hipStream_t s) {
    const KvParams& p = f.pp.kv;
    const unsigned grid = (unsigned)(p.B * p.Hkv * p.nsplit);
    if (f.ops == KV_OP_TREE) kv_launch<&fasn_kvcache_fwd_tree_kernel<Tag, D>>(grid, kv_smem(D), s, p, f.kt);
    else if (f.ops == KV_OP_WINDOW) kv_launch<&fasn_kvcache_fwd_window_kernel<Tag, D>>(grid, kv_smem(D), s, p, f.kw);
    else if (f.ops == KV_OP_ALIBI) kv_launch<&fasn_kvcache_fwd_alibi_kernel<Tag, D>>(grid, kv_smem(D), s, p, f.al);
    else kv_launch<&fasn_kvcache_fwd_kernel<Tag, D>>(grid, kv_smem(D), s, p);
    const int64_t nthr = (int64_t)p.B * p.Hkv * p.R * (D / 4);
    FASN_LAUNCH((fasn_kvcache_combine_kernel<Tag, D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, p);
    return launch_rc();
}
template <int D>
int kv_launch_append(const KvParams& p, hipStream_t s) {
    const int64_t nthr = (int64_t)p.B * p.Hkv * p.Sq * (D / 8);   // (at most 128 rows per K/V head: the grid fits)
    FASN_LAUNCH((fasn_kvcache_append_kernel<D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, p);
    return launch_rc();
}

}  // namespace

int kv_append(const fasn_kvcache_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    KvPrefillParams pp;
    const int rc = kv_build_append(kv_args(args), k_new, v_new, pp);
    if (rc) return rc;
    return kv_dispatch_d(args->D, [&](auto d) { return kv_launch_append<decltype(d)::value>(pp.kv, (hipStream_t)stream); });
}

int kv_launch_decode(const KvFwd& f, hipStream_t s) {
    return kv_dispatch(f.dtype, f.D, [&](auto tag, auto d) { return kv_launch_decode_as<decltype(tag), decltype(d)::value>(f, s); });
}
int kv_launch_commit(const KvCommit& c, int D, unsigned grid, hipStream_t s) {
    return kv_dispatch_d(D, [&](auto d) {
        kv_launch<&fasn_kvcache_tree_commit_kernel<decltype(d)::value>>(grid, 0, s, c);
        return launch_rc();
    });
}

}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_fwd_kvcache_workspace_bytes(const fasn_kvcache_args* args) { return kv_workspace_bytes(kv_args(args), kv_ops()); }

int fasn_fwd_kvcache(const fasn_kvcache_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(), workspace, workspace_bytes, stream);
}

int fasn_fwd_kvcache_alibi(const fasn_kvcache_args* args, const fasn_alibi_slopes* alibi, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(alibi), workspace, workspace_bytes, stream);
}

size_t fasn_fwd_kvcache_window_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_window* window) {
    return kv_workspace_bytes(kv_args(args), kv_ops(window));
}

int fasn_fwd_kvcache_window(const fasn_kvcache_args* args, const fasn_kv_window* window, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(window), workspace, workspace_bytes, stream);
}

int fasn_kvcache_append(const fasn_kvcache_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kv_append(args, k_new, v_new, stream);
}

int fasn_kvcache_plan(const fasn_kvcache_args* args, char* buf, size_t cap) { return kv_forward_plan(kv_args(args), kv_ops(), buf, cap); }

int fasn_kvcache_alibi_plan(const fasn_kvcache_args* args, const fasn_alibi_slopes* alibi, char* buf, size_t cap) {
    return kv_forward_plan(kv_args(args), kv_ops(alibi), buf, cap);
}

int fasn_kvcache_window_plan(const fasn_kvcache_args* args, const fasn_kv_window* window, char* buf, size_t cap) {
    return kv_forward_plan(kv_args(args), kv_ops(window), buf, cap);
}

size_t fasn_fwd_kvcache_tree_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_tree* tree) {
    return kv_workspace_bytes(kv_args(args), kv_ops(tree));
}

int fasn_fwd_kvcache_tree(const fasn_kvcache_args* args, const fasn_kv_tree* tree, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(tree), workspace, workspace_bytes, stream);
}

int fasn_kvcache_tree_plan(const fasn_kvcache_args* args, const fasn_kv_tree* tree, char* buf, size_t cap) {
    return kv_forward_plan(kv_args(args), kv_ops(tree), buf, cap);
}

int fasn_kvcache_tree_commit(const fasn_kv_tree_commit* commit, fasn_stream_t stream) { return kv_commit(commit, false, stream); }

}  // extern "C"
