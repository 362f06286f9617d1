// K/V-cache prefill (include/fasn.h: fasn_fwd_kvprefill[_alibi|_window], fasn_kvprefill_append, fasn_kvprefill[_alibi|_window]_plan): the
// prefill entry points and the launches of fasn_kvprefill.h. The argument checks, the launch plan and the workspace rule are the
// family's (fasn_kv_host.h, defined in fasn_kvcache.hip), called here with a prefill block.
#include <limits.h>
#include "fasn_kv_host.h"

namespace fasn {
namespace {

template <typename Tag, int D>
int kvp_launch_fwd(const KvFwd& f, hipStream_t s) {
    const KvPrefillParams& pp = f.pp;
    const KvParams& p = pp.kv;
    if (f.variant == KV_TREE)
        kv_launch_tree<&fasn_kvprefill_fwd_tree_kernel<Tag, D>>(f, pp, (unsigned)(p.B * p.Hkv * pp.nrb * p.nsplit), kv_smem(D), s);
    else
        kv_launch_variant<&fasn_kvprefill_fwd_kernel<Tag, D>, &fasn_kvprefill_fwd_alibi_kernel<Tag, D>, &fasn_kvprefill_fwd_window_kernel<Tag, D>>(
            f, pp, (unsigned)(p.B * p.Hkv * pp.nrb * p.nsplit), kv_smem(D), s);
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

int kvp_forward(const fasn_kvprefill_args* args, KvVariant variant, const void* operand, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    KvFwd f;
    const int rc = kv_build_forward(kv_args(args), variant, operand, workspace, workspace_bytes, f);
    if (rc) return rc;
    return kv_dispatch(args->kv.dtype, args->kv.D, [&](auto tag, auto d) { return kvp_launch_fwd<decltype(tag), decltype(d)::value>(f, (hipStream_t)stream); });
}
int kvp_append(const fasn_kvprefill_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    KvPrefillParams pp;
    const int rc = kv_build_append(kv_args(args), k_new, v_new, pp);
    if (rc) return rc;
    return kv_dispatch_d(args->kv.D, [&](auto d) { return kvp_launch_append<decltype(d)::value>(pp, (hipStream_t)stream); });
}
int kvp_forward_plan(const fasn_kvprefill_args* args, KvVariant variant, const void* operand, char* buf, size_t cap) {
    return kv_plan(buf, cap, [&] { return kvp_forward(args, variant, operand, kv_plan_workspace(), ~size_t(0), nullptr); });
}

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_fwd_kvprefill_workspace_bytes(const fasn_kvprefill_args* args) { return kv_workspace_bytes(kv_args(args), KV_BASE, nullptr); }

int fasn_fwd_kvprefill(const fasn_kvprefill_args* args, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kvp_forward(args, KV_BASE, nullptr, workspace, workspace_bytes, stream);
}

int fasn_fwd_kvprefill_alibi(const fasn_kvprefill_args* args, const fasn_alibi_slopes* alibi, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kvp_forward(args, KV_ALIBI, alibi, workspace, workspace_bytes, stream);
}

size_t fasn_fwd_kvprefill_window_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_window* window) {
    return kv_workspace_bytes(kv_args(args), KV_WINDOW, window);
}

int fasn_fwd_kvprefill_window(const fasn_kvprefill_args* args, const fasn_kv_window* window, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kvp_forward(args, KV_WINDOW, window, workspace, workspace_bytes, stream);
}

int fasn_kvprefill_append(const fasn_kvprefill_args* args, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kvp_append(args, k_new, v_new, stream);
}

int fasn_kvprefill_plan(const fasn_kvprefill_args* args, char* buf, size_t cap) { return kvp_forward_plan(args, KV_BASE, nullptr, buf, cap); }

int fasn_kvprefill_alibi_plan(const fasn_kvprefill_args* args, const fasn_alibi_slopes* alibi, char* buf, size_t cap) {
    return kvp_forward_plan(args, KV_ALIBI, alibi, buf, cap);
}

int fasn_kvprefill_window_plan(const fasn_kvprefill_args* args, const fasn_kv_window* window, char* buf, size_t cap) {
    return kvp_forward_plan(args, KV_WINDOW, window, buf, cap);
}

size_t fasn_fwd_kvprefill_tree_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_tree* tree) {
    return kv_workspace_bytes(kv_args(args), KV_TREE, tree);
}

int fasn_fwd_kvprefill_tree(const fasn_kvprefill_args* args, const fasn_kv_tree* tree, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kvp_forward(args, KV_TREE, tree, workspace, workspace_bytes, stream);
}

int fasn_kvprefill_tree_plan(const fasn_kvprefill_args* args, const fasn_kv_tree* tree, char* buf, size_t cap) {
    return kvp_forward_plan(args, KV_TREE, tree, buf, cap);
}

}  // extern "C"
