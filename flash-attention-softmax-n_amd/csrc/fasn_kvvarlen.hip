// K/V-cache prefill on token-packed queries (include/fasn.h: fasn_fwd_kvvarlen[_window], fasn_kvvarlen_append, fasn_kvvarlen[_window]_plan):
// the entry points and the launcher of the kernels of fasn_kvvarlen.h. The argument checks, the operand set's check, the launch plan, the
// workspace rule and the forward path are the family's (fasn_kv_host.h, defined in fasn_kvcache.hip), called here with a packed block.
#include <limits.h>
#include "fasn_kv_host.h"

namespace fasn {
namespace {

template <typename Tag, int D>
int kv_launch_packed_as(const KvFwd& f, hipStream_t s) {
    const KvPrefillParams& pp = f.pp;
    const KvParams& p = pp.kv;
    FASN_LAUNCH(fasn_kvvarlen_schedule_kernel<256>, dim3(1), dim3(256), 0, s, pp, f.pk);
    const unsigned grid = (unsigned)(f.pk.items_max * p.Hkv * p.nsplit);
    if (f.ops == KV_OP_WINDOW) kv_launch<&fasn_kvvarlen_fwd_window_kernel<Tag, D>>(grid, kv_smem(D), s, pp, f.pk, f.kw);
    else kv_launch<&fasn_kvvarlen_fwd_kernel<Tag, D>>(grid, kv_smem(D), s, pp, f.pk);
    if (p.nsplit > 1) {
        const int64_t nthr = (int64_t)f.pk.items_max * p.Hkv * KVP_ROWS * (D / 4);
        FASN_LAUNCH((fasn_kvvarlen_combine_kernel<Tag, D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, pp, f.pk);
    }
    return launch_rc();
}
template <int D>
int kvv_launch_append(const KvPrefillParams& pp, const KvPacked& pk, hipStream_t s) {
    const int64_t nthr = (int64_t)pk.T * pp.kv.Hkv * (D / 8);
    if ((nthr + 255) / 256 > INT_MAX) return FASN_EINVAL;
    FASN_LAUNCH((fasn_kvvarlen_append_kernel<D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, pp, pk);
    return launch_rc();
}

}  // namespace

int kvv_append(const fasn_kvvarlen_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    KvPrefillParams pp;
    KvPacked pk;
    const int rc = kv_build_append(kv_args(args), k_new, v_new, pp, &pk);
    if (rc) return rc;
    return kv_dispatch_d(args->pf.kv.D, [&](auto d) { return kvv_launch_append<decltype(d)::value>(pp, pk, (hipStream_t)stream); });
}

int kv_launch_packed(const KvFwd& f, hipStream_t s) {
    return kv_dispatch(f.dtype, f.D, [&](auto tag, auto d) { return kv_launch_packed_as<decltype(tag), decltype(d)::value>(f, s); });
}

}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_fwd_kvvarlen_workspace_bytes(const fasn_kvvarlen_args* args) { return kv_workspace_bytes(kv_args(args), kv_ops()); }

int fasn_fwd_kvvarlen(const fasn_kvvarlen_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(), workspace, workspace_bytes, stream);
}

size_t fasn_fwd_kvvarlen_window_workspace_bytes(const fasn_kvvarlen_args* args, const fasn_kv_window* window) {
    return kv_workspace_bytes(kv_args(args), kv_ops(window));
}

int fasn_fwd_kvvarlen_window(const fasn_kvvarlen_args* args, const fasn_kv_window* window, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(window), workspace, workspace_bytes, stream);
}

int fasn_kvvarlen_append(const fasn_kvvarlen_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvv_append(args, k_new, v_new, stream);
}

int fasn_kvvarlen_plan(const fasn_kvvarlen_args* args, char* buf, size_t cap) { return kv_forward_plan(kv_args(args), kv_ops(), buf, cap); }

int fasn_kvvarlen_window_plan(const fasn_kvvarlen_args* args, const fasn_kv_window* window, char* buf, size_t cap) {
    return kv_forward_plan(kv_args(args), kv_ops(window), buf, cap);
}

}  // extern "C"
