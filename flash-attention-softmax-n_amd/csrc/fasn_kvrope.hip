// Rotary rotate-and-append on the K/V-cache calls (include/fasn.h: fasn_kvcache_rope_append, fasn_kvprefill_rope_append and their
// *_plan siblings): the base call's argument checks first, then the operand's, and the one launch of fasn_kvrope.h - whose grid
// depends on shapes only, never on the lengths in device memory.
#include <limits.h>
#include "fasn.h"
#include "fasn_kvrope.h"
#include "fasn_launch.h"

namespace fasn {
namespace {

bool kvr_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int kvr_check_view(const fasn_view4& v) {   // the rules of q
    if (v.ptr == nullptr) return FASN_EINVAL;
    if (v.stride[3] != 1) return FASN_ESTRIDE;
    if (!kvr_aligned16(v.ptr)) return FASN_EALIGN;
    for (int i = 0; i < 3; ++i)
        if (v.stride[i] % 8 != 0) return FASN_EALIGN;
    return FASN_OK;
}

// The operand's checks (after the base arguments, before any HIP call) and the kernel parameters. `rp.kv` / `rp.qlens` are the base
// call's; `prefill`: the length rule of fasn_fwd_kvprefill.
int kvr_build(const fasn_kvcache_args* a, bool prefill, const fasn_kv_rope* r, const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new,
              KvRopeParams& rp) {
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
    if (!kvr_aligned16(r->cos) || !kvr_aligned16(r->sin) || (r->row_stride * esize) % 16 != 0) return FASN_EALIGN;
    int rc;
    if ((rc = kvr_check_view(*q_out))) return rc;
    if (k_new != nullptr) {
        if ((rc = kvr_check_view(*k_new))) return rc;
        if ((rc = kvr_check_view(*v_new))) return rc;
        p.kn = static_cast<const char*>(k_new->ptr);
        p.vn = static_cast<const char*>(v_new->ptr);
        for (int i = 0; i < 3; ++i) {
            p.kns[i] = k_new->stride[i];
            p.vns[i] = v_new->stride[i];
        }
    }
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
    rp.nkv = k_new != nullptr ? (int64_t)p.B * p.Hkv * p.Sq * upr : 0;
    rp.nq = (int64_t)p.B * p.H * p.Sq * upr;
    if ((rp.nkv + rp.nq + 255) / 256 > INT_MAX) return FASN_EINVAL;
    return FASN_OK;
}

template <typename Tag>
int kvr_launch(int D, const KvRopeParams& rp, hipStream_t s) {   // (the base call let only these four head dims through)
    const dim3 grid((unsigned)((rp.nkv + rp.nq + 255) / 256));
    switch (D) {
        case 32: FASN_LAUNCH((fasn_kvrope_kernel<Tag, 32>), grid, dim3(256), 0, s, rp); break;
        case 64: FASN_LAUNCH((fasn_kvrope_kernel<Tag, 64>), grid, dim3(256), 0, s, rp); break;
        case 128: FASN_LAUNCH((fasn_kvrope_kernel<Tag, 128>), grid, dim3(256), 0, s, rp); break;
        default: FASN_LAUNCH((fasn_kvrope_kernel<Tag, 256>), grid, dim3(256), 0, s, rp); break;
    }
    return launch_rc();
}

int kvr_decode(const fasn_kvcache_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new,
               fasn_stream_t stream) {
    KvRopeParams rp{};
    int rc = kv_build_params(args, rp.kv);
    if (rc) return rc;
    if ((rc = kvr_build(args, false, rope, q_out, k_new, v_new, rp))) return rc;
    if (args->dtype == FASN_DTYPE_BF16) return kvr_launch<bf16_tag>(args->D, rp, (hipStream_t)stream);
    return kvr_launch<f16_tag>(args->D, rp, (hipStream_t)stream);
}

int kvr_prefill(const fasn_kvprefill_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new, const fasn_view4* v_new,
                fasn_stream_t stream) {
    KvPrefillParams pp;
    int rc = kvp_build_params(args, pp);
    if (rc) return rc;
    KvRopeParams rp{};
    rp.kv = pp.kv;
    rp.qlens = pp.qlens;
    if ((rc = kvr_build(&args->kv, true, rope, q_out, k_new, v_new, rp))) return rc;
    if (args->kv.dtype == FASN_DTYPE_BF16) return kvr_launch<bf16_tag>(args->kv.D, rp, (hipStream_t)stream);
    return kvr_launch<f16_tag>(args->kv.D, rp, (hipStream_t)stream);
}

// the launch as text: the call itself under the launch recorder (nothing is launched, no device is touched)
template <typename Call>
int kvr_plan(char* buf, size_t cap, Call call) {
    if (buf == nullptr || cap == 0) return FASN_EINVAL;
    LaunchLog log{buf, cap, 0};
    buf[0] = 0;
    LaunchLog* const outer = t_launch_log;
    t_launch_log = &log;
    const int rc = call();
    t_launch_log = outer;
    if (rc) return rc;
    return log.len > cap ? FASN_EINVAL : (int)log.len;
}

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

int fasn_kvcache_rope_append(const fasn_kvcache_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                             const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_decode(args, rope, q_out, k_new, v_new, stream);
}

int fasn_kvprefill_rope_append(const fasn_kvprefill_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                               const fasn_view4* v_new, fasn_stream_t stream) {
    return kvr_prefill(args, rope, q_out, k_new, v_new, stream);
}

int fasn_kvcache_rope_append_plan(const fasn_kvcache_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                                  const fasn_view4* v_new, char* buf, size_t cap) {
    return kvr_plan(buf, cap, [&] { return kvr_decode(args, rope, q_out, k_new, v_new, nullptr); });
}

int fasn_kvprefill_rope_append_plan(const fasn_kvprefill_args* args, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_new,
                                    const fasn_view4* v_new, char* buf, size_t cap) {
    return kvr_plan(buf, cap, [&] { return kvr_prefill(args, rope, q_out, k_new, v_new, nullptr); });
}

}  // extern "C"
