// Rotary rotate-and-append on the K/V-cache calls (include/fasn.h: fasn_{kvcache,kvprefill,kvvarlen}_rope_append, the decode and prefill
// calls' *_tree_rope_append - the rotation at the depth positions of a token tree - and their *_fp8_rope_append / *_fp8_tree_rope_append,
// the rotate-quantise-append in front of an FP8 cache; with the *_plan siblings they have): ONE call path, kvr_call, which takes the
// operand set (FP8 and / or tree) beside the rope operand. The base call's argument checks and the FP8 and tree operands' checks are the
// family's (fasn_kv_host.h), the rope operand's live here, and the one launch is of fasn_kvrope.h or, over an FP8 cache, of fasn_kvfp8.h -
// its grid depends on shapes only, never on the lengths in device memory.
#include <limits.h>
#include "fasn_kv_host.h"
#include "fasn_kvrope.h"
#include "fasn_kvfp8.h"

namespace fasn {
namespace {

// The operand's checks (after the base arguments, before any HIP call) and the kernel parameters. `rp.kv` / `rp.qlens` are the base
// call's; `prefill`: the length rule of fasn_fwd_kvprefill; `rows`: the rows of a head in q / k_new - B * Sq, packed: total_tokens.
int kvr_build(const fasn_kvcache_args* a, bool prefill, int64_t rows, const fasn_kv_rope* r, const fasn_view4* q_out, const fasn_view4* k_new,
              const fasn_view4* v_new, KvRopeParams& rp) {
    KvParams& p = rp.kv;
    if (r == nullptr || r->cos == nullptr || r->sin == nullptr || q_out == nullptr) return FASN_EINVAL;
    if ((k_new == nullptr) != (v_new == nullptr)) return FASN_EINVAL;
    if (k_new != nullptr && a->seqlen_add != a->Sq) return FASN_EINVAL;   // the forward that follows is to see the appended rows
    if (r->rotary_dim < 16 || r->rotary_dim > a->D || r->rotary_dim % 16 != 0) return FASN_EINVAL;
    if (r->rows < p.capacity) return FASN_EINVAL;
    if (r->interleaved != 0 && r->interleaved != 1) return FASN_EINVAL;
    if (r->table_dtype != FASN_DTYPE_F32 && r->table_dtype != a->dtype) return FASN_EDTYPE;
    const int64_t esize = r->table_dtype == FASN_DTYPE_F32 ? 4 : 2;
    if (r->row_stride < r->rotary_dim / 2) return FASN_EINVAL;   // (rows overlap)
    if (!kv_aligned16(r->cos) || !kv_aligned16(r->sin) || (r->row_stride * esize) % 16 != 0) return FASN_EALIGN;
    int rc;
    if ((rc = kv_check_view(*q_out))) return rc;
    if (k_new != nullptr && (rc = kv_pack_new(*k_new, *v_new, p))) return rc;
    rp.qo = static_cast<char*>(q_out->ptr);
    for (int i = 0; i < 3; ++i) rp.qos[i] = q_out->stride[i];
    rp.cos = static_cast<const char*>(r->cos);
    rp.sin = static_cast<const char*>(r->sin);
    rp.trs = r->row_stride;
    rp.rows = r->rows;
    rp.rd = r->rotary_dim;
    rp.tf32 = r->table_dtype == FASN_DTYPE_F32 ? 1 : 0;
    rp.interleaved = r->interleaved;
    rp.add_qlen = prefill ? (a->seqlen_add != 0 ? 1 : 0) : -1;
    const int64_t upr = a->D / 16;
    rp.nkv = k_new != nullptr ? rows * p.Hkv * upr : 0;
    rp.nq = rows * p.H * upr;
    if ((rp.nkv + rp.nq + 255) / 256 > INT_MAX) return FASN_EINVAL;
    return FASN_OK;
}

}  // namespace

// One call path for every rotary append. `ops`: the operands beside the rope operand - FP8 and / or tree; the packed call has the FP8
// operand only. THE CHECK ORDER is decided here and differs between the two families: a 16-bit cache checks base -> rope ->
// tree, an FP8 cache base -> FP8 -> tree -> rope. Both orders are ABI behaviour that tests pin (tests/test_kvtree_cpu.py,
// tests/test_kvfp8_tree_cpu.py, tests/golden/kvfp8_tree_plans.txt): keep them.
int kvr_call(const KvArgs& in, const KvOps& ops, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new,
             fasn_stream_t stream) {
    KvPrefillParams pp;
    KvPacked pk{};
    int rc = kv_build(in, pp, &pk);
    if (rc) return rc;
    const bool packed = in.call == KV_VARLEN, fp8 = (ops.takes & KV_OP_FP8) != 0, tree = (ops.takes & KV_OP_TREE) != 0;
    if (packed && (ops.takes & ~KV_OP_FP8) != 0) return FASN_EUNSUPPORTED;
    KvFp8 f8{};
    KvTree kt{};
    if (fp8 && (rc = kv_check_fp8(in.a, ops.fp8, f8))) return rc;
    if (fp8 && tree && (rc = kv_check_tree(in.a, ops.tree, pp.kv.capacity, kt))) return rc;
    KvRopeParams rp{};
    rp.kv = pp.kv;
    rp.qlens = pp.qlens;
    const int64_t rows = packed ? (int64_t)pk.T : (int64_t)pp.kv.B * pp.kv.Sq;
    if ((rc = kvr_build(in.a, in.call != KV_DECODE, rows, rope, q_out, k_new, v_new, rp))) return rc;
    if (!fp8 && tree && (rc = kv_check_tree(in.a, ops.tree, pp.kv.capacity, kt))) return rc;
    const unsigned grid = (unsigned)((rp.nkv + rp.nq + 255) / 256);
    const hipStream_t s = (hipStream_t)stream;
    if (fp8)
        return kv8_dispatch(in.a->dtype, in.a->D, [&](auto tag, auto d) {
            using Tag = decltype(tag);
            constexpr int D = decltype(d)::value;
            if (tree) kv_launch<&fasn_kvrope_fp8_tree_kernel<Tag, D>>(grid, 0, s, rp, f8, kt);
            else if (packed) kv_launch<&fasn_kvvarlen_rope_fp8_kernel<Tag, D>>(grid, 0, s, rp, pk, f8);
            else kv_launch<&fasn_kvrope_fp8_kernel<Tag, D>>(grid, 0, s, rp, f8);
            return launch_rc();
        });
    return kv_dispatch(in.a->dtype, in.a->D, [&](auto tag, auto d) {
        using Tag = decltype(tag);
        constexpr int D = decltype(d)::value;
        if (tree) kv_launch<&fasn_kvrope_tree_kernel<Tag, D>>(grid, 0, s, rp, kt);
        else if (packed) kv_launch<&fasn_kvvarlen_rope_kernel<Tag, D>>(grid, 0, s, rp, pk);
        else kv_launch<&fasn_kvrope_kernel<Tag, D>>(grid, 0, s, rp);
        return launch_rc();
    });
}
namespace {
int kvr_plan(const KvArgs& in, const KvOps& ops, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new,
             char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return kvr_call(in, ops, rope, q_out, k_new, v_new, nullptr); });
}

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

int fasn_kvcache_rope_append(const fasn_kvcache_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                             const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), kv_ops(), rope, q_out, k_new, v_new, stream);
}

int fasn_kvprefill_rope_append(const fasn_kvprefill_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                               const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), kv_ops(), rope, q_out, k_new, v_new, stream);
}

int fasn_kvcache_tree_rope_append(const fasn_kvcache_args* args, const fasn_kv_rope* rope, const fasn_kv_tree* tree, const fasn_view4* q_out,
                                  const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), kv_ops(tree), rope, q_out, k_new, v_new, stream);
}

int fasn_kvprefill_tree_rope_append(const fasn_kvprefill_args* args, const fasn_kv_rope* rope, const fasn_kv_tree* tree, const fasn_view4* q_out,
                                    const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), kv_ops(tree), rope, q_out, k_new, v_new, stream);
}

int fasn_kvcache_rope_append_plan(const fasn_kvcache_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                                  const fasn_view4* v_new, char* buf, size_t cap) {
    return kvr_plan(kv_args(args), kv_ops(), rope, q_out, k_new, v_new, buf, cap);
}

int fasn_kvprefill_rope_append_plan(const fasn_kvprefill_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                                    const fasn_view4* v_new, char* buf, size_t cap) {
    return kvr_plan(kv_args(args), kv_ops(), rope, q_out, k_new, v_new, buf, cap);
}

int fasn_kvvarlen_rope_append(const fasn_kvvarlen_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                              const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), kv_ops(), rope, q_out, k_new, v_new, stream);
}

int fasn_kvvarlen_rope_append_plan(const fasn_kvvarlen_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                                   const fasn_view4* v_new, char* buf, size_t cap) {
    return kvr_plan(kv_args(args), kv_ops(), rope, q_out, k_new, v_new, buf, cap);
}

int fasn_kvcache_fp8_rope_append(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                 const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), kv_ops(fp8), rope, q_out, k_new, v_new, stream);
}

int fasn_kvprefill_fp8_rope_append(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                   const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), kv_ops(fp8), rope, q_out, k_new, v_new, stream);
}

int fasn_kvcache_fp8_rope_append_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                      const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap) {
    return kvr_plan(kv_args(args), kv_ops(fp8), rope, q_out, k_new, v_new, buf, cap);
}

int fasn_kvprefill_fp8_rope_append_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                        const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap) {
    return kvr_plan(kv_args(args), kv_ops(fp8), rope, q_out, k_new, v_new, buf, cap);
}

int fasn_kvcache_fp8_tree_rope_append(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_kv_tree* tree,
                                      const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), kv_ops(fp8, tree), rope, q_out, k_new, v_new, stream);
}

int fasn_kvprefill_fp8_tree_rope_append(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_kv_tree* tree,
                                        const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), kv_ops(fp8, tree), rope, q_out, k_new, v_new, stream);
}

int fasn_kvcache_fp8_tree_rope_append_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_kv_tree* tree,
                                           const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap) {
    return kvr_plan(kv_args(args), kv_ops(fp8, tree), rope, q_out, k_new, v_new, buf, cap);
}

int fasn_kvprefill_fp8_tree_rope_append_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_kv_tree* tree,
                                             const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap) {
    return kvr_plan(kv_args(args), kv_ops(fp8, tree), rope, q_out, k_new, v_new, buf, cap);
}

}  // extern "C"
