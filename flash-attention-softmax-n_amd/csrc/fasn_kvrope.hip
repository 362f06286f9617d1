// Rotary rotate-and-append on the K/V-cache calls (include/fasn.h: fasn_kvcache_rope_append, fasn_kvprefill_rope_append,
// fasn_kvvarlen_rope_append and their *_plan siblings, fasn_kvcache_tree_rope_append / fasn_kvprefill_tree_rope_append, and
// fasn_kvcache_fp8_rope_append / fasn_kvprefill_fp8_rope_append with their *_plan siblings - the rotate-quantise-append in front of an FP8
// cache, whose FP8 operand is checked behind the base arguments and in front of the rope operand - and fasn_kvcache_fp8_tree_rope_append /
// fasn_kvprefill_fp8_tree_rope_append, the same at the depth positions of a token tree: base, FP8 operand, tree operand, rope operand): the base call's argument checks first
// (the family's, fasn_kv_host.h), then the operand's, which live here, and the one launch of fasn_kvrope.h (the FP8 sibling: of
// fasn_kvfp8.h) - whose grid depends on shapes only, never on the lengths in device memory.
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

template <typename Tag, int D>
int kvr_launch(const KvRopeParams& rp, hipStream_t s) {
    FASN_LAUNCH((fasn_kvrope_kernel<Tag, D>), dim3((unsigned)((rp.nkv + rp.nq + 255) / 256)), dim3(256), 0, s, rp);
    return launch_rc();
}
template <typename Tag, int D>
int kvr_launch_tree(const KvRopeParams& rp, const KvTree& kt, hipStream_t s) {
    FASN_LAUNCH((fasn_kvrope_tree_kernel<Tag, D>), dim3((unsigned)((rp.nkv + rp.nq + 255) / 256)), dim3(256), 0, s, rp, kt);
    return launch_rc();
}
template <typename Tag, int D>
int kvr_launch_packed(const KvRopeParams& rp, const KvPacked& pk, hipStream_t s) {
    FASN_LAUNCH((fasn_kvvarlen_rope_kernel<Tag, D>), dim3((unsigned)((rp.nkv + rp.nq + 255) / 256)), dim3(256), 0, s, rp, pk);
    return launch_rc();
}

// the rotate-quantise-append of fasn_kvfp8.h, at the two head dims the FP8 kernels are built for (kv_check_fp8 let only these through)
template <typename Tag, int D>
int kvr_launch_fp8(const KvRopeParams& rp, const KvFp8& f8, hipStream_t s) {
    FASN_LAUNCH((fasn_kvrope_fp8_kernel<Tag, D>), dim3((unsigned)((rp.nkv + rp.nq + 255) / 256)), dim3(256), 0, s, rp, f8);
    return launch_rc();
}
template <typename Tag>
int kvr_launch_fp8_d(int D, const KvRopeParams& rp, const KvFp8& f8, hipStream_t s) {
    return D == 64 ? kvr_launch_fp8<Tag, 64>(rp, f8, s) : kvr_launch_fp8<Tag, 128>(rp, f8, s);
}

template <typename Tag, int D>
int kvr_launch_fp8_tree(const KvRopeParams& rp, const KvFp8& f8, const KvTree& kt, hipStream_t s) {
    FASN_LAUNCH((fasn_kvrope_fp8_tree_kernel<Tag, D>), dim3((unsigned)((rp.nkv + rp.nq + 255) / 256)), dim3(256), 0, s, rp, f8, kt);
    return launch_rc();
}
template <typename Tag>
int kvr_launch_fp8_tree_d(int D, const KvRopeParams& rp, const KvFp8& f8, const KvTree& kt, hipStream_t s) {
    return D == 64 ? kvr_launch_fp8_tree<Tag, 64>(rp, f8, kt, s) : kvr_launch_fp8_tree<Tag, 128>(rp, f8, kt, s);
}

// `tree`: the *_tree_rope_append calls (the rotation at depth positions); its operand is checked behind the rope operand
int kvr_call(const KvArgs& in, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream,
             bool tree = false, const fasn_kv_tree* tree_operand = nullptr) {
    KvPrefillParams pp;
    KvPacked pk{};
    int rc = kv_build(in, pp, &pk);
    if (rc) return rc;
    KvRopeParams rp{};
    rp.kv = pp.kv;
    rp.qlens = pp.qlens;
    const bool packed = in.call == KV_VARLEN;
    const int64_t rows = packed ? (int64_t)pk.T : (int64_t)pp.kv.B * pp.kv.Sq;
    if ((rc = kvr_build(in.a, in.call != KV_DECODE, rows, rope, q_out, k_new, v_new, rp))) return rc;
    if (tree) {
        KvTree kt{};
        if (packed) return FASN_EUNSUPPORTED;
        if ((rc = kv_check_tree(in.a, tree_operand, pp.kv.capacity, kt))) return rc;
        return kv_dispatch(in.a->dtype, in.a->D, [&](auto tag, auto d) { return kvr_launch_tree<decltype(tag), decltype(d)::value>(rp, kt, (hipStream_t)stream); });
    }
    if (packed)
        return kv_dispatch(in.a->dtype, in.a->D, [&](auto tag, auto d) { return kvr_launch_packed<decltype(tag), decltype(d)::value>(rp, pk, (hipStream_t)stream); });
    return kv_dispatch(in.a->dtype, in.a->D, [&](auto tag, auto d) { return kvr_launch<decltype(tag), decltype(d)::value>(rp, (hipStream_t)stream); });
}

// the *_fp8_rope_append calls: the base checks, the FP8 operand's (kv_check_fp8), the rope operand's (kvr_build), one launch on the grid
// of the 16-bit rope append. Decode and prefill only. `tree`: the *_fp8_tree_rope_append calls (the rotation at depth positions); their
// tree operand is checked behind the FP8 operand and in front of the rope operand, and the one launch is on the 16-bit tree rope grid.
int kvr_call_fp8(const KvArgs& in, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new,
                 fasn_stream_t stream, bool tree = false, const fasn_kv_tree* tree_operand = nullptr) {
    KvPrefillParams pp;
    int rc = kv_build(in, pp);
    if (rc) return rc;
    KvFp8 f8{};
    if ((rc = kv_check_fp8(in.a, fp8, f8))) return rc;
    KvTree kt{};
    if (tree && (rc = kv_check_tree(in.a, tree_operand, pp.kv.capacity, kt))) return rc;
    KvRopeParams rp{};
    rp.kv = pp.kv;
    rp.qlens = pp.qlens;
    if ((rc = kvr_build(in.a, in.call != KV_DECODE, (int64_t)pp.kv.B * pp.kv.Sq, rope, q_out, k_new, v_new, rp))) return rc;
    if (tree) {
        if (in.a->dtype == FASN_DTYPE_BF16) return kvr_launch_fp8_tree_d<bf16_tag>(in.a->D, rp, f8, kt, (hipStream_t)stream);
        return kvr_launch_fp8_tree_d<f16_tag>(in.a->D, rp, f8, kt, (hipStream_t)stream);
    }
    if (in.a->dtype == FASN_DTYPE_BF16) return kvr_launch_fp8_d<bf16_tag>(in.a->D, rp, f8, (hipStream_t)stream);
    return kvr_launch_fp8_d<f16_tag>(in.a->D, rp, f8, (hipStream_t)stream);
}

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

int fasn_kvcache_rope_append(const fasn_kvcache_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                             const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), rope, q_out, k_new, v_new, stream);
}

int fasn_kvprefill_rope_append(const fasn_kvprefill_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                               const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), rope, q_out, k_new, v_new, stream);
}

int fasn_kvcache_tree_rope_append(const fasn_kvcache_args* args, const fasn_kv_rope* rope, const fasn_kv_tree* tree, const fasn_view4* q_out,
                                  const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), rope, q_out, k_new, v_new, stream, true, tree);
}

int fasn_kvprefill_tree_rope_append(const fasn_kvprefill_args* args, const fasn_kv_rope* rope, const fasn_kv_tree* tree, const fasn_view4* q_out,
                                    const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), rope, q_out, k_new, v_new, stream, true, tree);
}

int fasn_kvcache_rope_append_plan(const fasn_kvcache_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                                  const fasn_view4* v_new, char* buf, size_t cap) {
    return kv_plan(buf, cap, [&] { return kvr_call(kv_args(args), rope, q_out, k_new, v_new, nullptr); });
}

int fasn_kvprefill_rope_append_plan(const fasn_kvprefill_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                                    const fasn_view4* v_new, char* buf, size_t cap) {
    return kv_plan(buf, cap, [&] { return kvr_call(kv_args(args), rope, q_out, k_new, v_new, nullptr); });
}

int fasn_kvvarlen_rope_append(const fasn_kvvarlen_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                              const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call(kv_args(args), rope, q_out, k_new, v_new, stream);
}

int fasn_kvvarlen_rope_append_plan(const fasn_kvvarlen_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                                   const fasn_view4* v_new, char* buf, size_t cap) {
    return kv_plan(buf, cap, [&] { return kvr_call(kv_args(args), rope, q_out, k_new, v_new, nullptr); });
}

int fasn_kvcache_fp8_rope_append(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                 const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call_fp8(kv_args(args), fp8, rope, q_out, k_new, v_new, stream);
}

int fasn_kvprefill_fp8_rope_append(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                   const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call_fp8(kv_args(args), fp8, rope, q_out, k_new, v_new, stream);
}

int fasn_kvcache_fp8_rope_append_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                      const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap) {
    return kv_plan(buf, cap, [&] { return kvr_call_fp8(kv_args(args), fp8, rope, q_out, k_new, v_new, nullptr); });
}

int fasn_kvprefill_fp8_rope_append_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_view4* q_out,
                                        const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap) {
    return kv_plan(buf, cap, [&] { return kvr_call_fp8(kv_args(args), fp8, rope, q_out, k_new, v_new, nullptr); });
}

int fasn_kvcache_fp8_tree_rope_append(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_kv_tree* tree,
                                      const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call_fp8(kv_args(args), fp8, rope, q_out, k_new, v_new, stream, true, tree);
}

int fasn_kvprefill_fp8_tree_rope_append(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_kv_tree* tree,
                                        const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_call_fp8(kv_args(args), fp8, rope, q_out, k_new, v_new, stream, true, tree);
}

int fasn_kvcache_fp8_tree_rope_append_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_kv_tree* tree,
                                           const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap) {
    return kv_plan(buf, cap, [&] { return kvr_call_fp8(kv_args(args), fp8, rope, q_out, k_new, v_new, nullptr, true, tree); });
}

int fasn_kvprefill_fp8_tree_rope_append_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_rope* rope, const fasn_kv_tree* tree,
                                             const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new, char* buf, size_t cap) {
    return kv_plan(buf, cap, [&] { return kvr_call_fp8(kv_args(args), fp8, rope, q_out, k_new, v_new, nullptr, true, tree); });
}

}  // extern "C"
