// K/V-cache prefill (include/fasn.h: fasn_fwd_kvprefill[_alibi|_window|_tree], fasn_kvprefill_append, fasn_kvprefill[_alibi|_window|_tree]_plan):
// the prefill entry points and the launcher of the kernels of fasn_kvprefill.h. The argument checks, the operand set's check, the launch
// plan, the workspace rule and the forward path are the family's (fasn_kv_host.h, defined in fasn_kvcache.hip), called here with a
// prefill block.
#include <limits.h>
#include "fasn_kv_host.h"

namespace fasn {
namespace {

template <typename Tag, int D>
int kv_launch_prefill_as(const KvFwd& f, hipStream_t s) {
    const KvPrefillParams& pp = f.pp;
    const KvParams& p = pp.kv;
    const unsigned grid = (unsigned)(p.B * p.Hkv * pp.nrb * p.nsplit);
    if (f.ops == KV_OP_TREE) kv_launch<&fasn_kvprefill_fwd_tree_kernel<Tag, D>>(grid, kv_smem(D), s, pp, f.kt);
    else if (f.ops == KV_OP_WINDOW) kv_launch<&fasn_kvprefill_fwd_window_kernel<Tag, D>>(grid, kv_smem(D), s, pp, f.kw);
    else if (f.ops == KV_OP_ALIBI) kv_launch<&fasn_kvprefill_fwd_alibi_kernel<Tag, D>>(grid, kv_smem(D), s, pp, f.al);
    else kv_launch<&fasn_kvprefill_fwd_kernel<Tag, D>>(grid, kv_smem(D), s, pp);
    if (p.nsplit > 1) {
        const int64_t nthr = (int64_t)p.B * p.Hkv * pp.nrb * KVP_ROWS * (D / 4);
        FASN_LAUNCH((fasn_kvprefill_combine_kernel<Tag, D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, pp);
    }
    return launch_rc();
}
template <int D>
int kvp_launch_append(const KvPrefillParams& pp, hipStream_t s) {
    const int64_t nthr = (int64_t)pp.kv.B * pp.kv.Hkv * pp.kv.Sq * (D / 8);
    if ((nthr + 255) / 256 > INT_MAX) return FASN_EINVAL;   // (Sq has no limit here)
    FASN_LAUNCH((fasn_kvprefill_append_kernel<D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, pp);
    return launch_rc();
}

}  // namespace

int kvp_append(const fasn_kvprefill_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    KvPrefillParams pp;
    const int rc = kv_build_append(kv_args(args), k_new, v_new, pp);
    if (rc) return rc;
    return kv_dispatch_d(args->kv.D, [&](auto d) { return kvp_launch_append<decltype(d)::value>(pp, (hipStream_t)stream); });
}

int kv_launch_prefill(const KvFwd& f, hipStream_t s) {
    return kv_dispatch(f.dtype, f.D, [&](auto tag, auto d) { return kv_launch_prefill_as<decltype(tag), decltype(d)::value>(f, s); });
}

}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_fwd_kvprefill_workspace_bytes(const fasn_kvprefill_args* args) { return kv_workspace_bytes(kv_args(args), kv_ops()); }

int fasn_fwd_kvprefill(const fasn_kvprefill_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(), workspace, workspace_bytes, stream);
}

int fasn_fwd_kvprefill_alibi(const fasn_kvprefill_args* args, const fasn_alibi_slopes* alibi, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(alibi), workspace, workspace_bytes, stream);
}

size_t fasn_fwd_kvprefill_window_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_window* window) {
    return kv_workspace_bytes(kv_args(args), kv_ops(window));
}

int fasn_fwd_kvprefill_window(const fasn_kvprefill_args* args, const fasn_kv_window* window, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(window), workspace, workspace_bytes, stream);
}

int fasn_kvprefill_append(const fasn_kvprefill_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvp_append(args, k_new, v_new, stream);
}

int fasn_kvprefill_plan(const fasn_kvprefill_args* args, char* buf, size_t cap) { return kv_forward_plan(kv_args(args), kv_ops(), buf, cap); }

int fasn_kvprefill_alibi_plan(const fasn_kvprefill_args* args, const fasn_alibi_slopes* alibi, char* buf, size_t cap) {
    return kv_forward_plan(kv_args(args), kv_ops(alibi), buf, cap);
}

int fasn_kvprefill_window_plan(const fasn_kvprefill_args* args, const fasn_kv_window* window, char* buf, size_t cap) {
    return kv_forward_plan(kv_args(args), kv_ops(window), buf, cap);
}

size_t fasn_fwd_kvprefill_tree_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_tree* tree) {
    return kv_workspace_bytes(kv_args(args), kv_ops(tree));
}

int fasn_fwd_kvprefill_tree(const fasn_kvprefill_args* args, const fasn_kv_tree* tree, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(tree), workspace, workspace_bytes, stream);
}

int fasn_kvprefill_tree_plan(const fasn_kvprefill_args* args, const fasn_kv_tree* tree, char* buf, size_t cap) {
    return kv_forward_plan(kv_args(args), kv_ops(tree), buf, cap);
}

}  // extern "C"
