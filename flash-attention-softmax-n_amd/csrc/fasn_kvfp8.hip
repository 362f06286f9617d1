// FP8 K/V cache (include/fasn.h: fasn_fwd_kvcache_fp8, fasn_fwd_kvprefill_fp8, their *_workspace_bytes, *_plan and *_append calls, the
// *_fp8_window and *_fp8_tree siblings of the forwards, and fasn_kvcache_fp8_tree_commit): the entry points and the launchers of the
// kernels of fasn_kvfp8.h (its rotate-quantise-appends are launched from fasn_kvrope.hip, beside the rope operand's checks). Every check,
// the launch plan, the workspace rule, the forward path and the commit are the family's (fasn_kv_host.h, defined in fasn_kvcache.hip): an
// FP8 call is a decode, a prefill or a packed block whose operand set holds the FP8 operand. The packed FP8 sets have no named entry
// points: they are reached through the operand-set calls (fasn_kv_forward, fasn_kv_append; fasn_kvcall.hip).
#include <limits.h>
#include "fasn_kv_host.h"
#include "fasn_kvfp8.h"

namespace fasn {
namespace {

// decode: the forward and, always, the combine
template <typename Tag, int D>
int kv_launch_fp8_decode_as(const KvFwd& f, hipStream_t s) {
    const KvParams& p = f.pp.kv;
    const unsigned grid = (unsigned)(p.B * p.Hkv * p.nsplit);
    if (f.ops & KV_OP_TREE) kv_launch<&fasn_kvcache_fwd_fp8_tree_kernel<Tag, D>>(grid, kv_fp8_smem(D), s, p, f.f8, f.kt);
    else if (f.ops & KV_OP_WINDOW) kv_launch<&fasn_kvcache_fwd_fp8_window_kernel<Tag, D>>(grid, kv_fp8_smem(D), s, p, f.f8, f.kw);
    else kv_launch<&fasn_kvcache_fwd_fp8_kernel<Tag, D>>(grid, kv_fp8_smem(D), s, p, f.f8);
    const int64_t nthr = (int64_t)p.B * p.Hkv * p.R * (D / 4);
    FASN_LAUNCH((fasn_kvcache_fp8_combine_kernel<Tag, D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, p, f.f8);
    return launch_rc();
}
// prefill: one split stores o / lse itself
template <typename Tag, int D>
int kv_launch_fp8_prefill_as(const KvFwd& f, hipStream_t s) {
    const KvPrefillParams& pp = f.pp;
    const KvParams& p = pp.kv;
    const unsigned grid = (unsigned)(p.B * p.Hkv * pp.nrb * p.nsplit);
    if (f.ops & KV_OP_TREE) kv_launch<&fasn_kvprefill_fwd_fp8_tree_kernel<Tag, D>>(grid, kv_fp8_smem(D), s, pp, f.f8, f.kt);
    else if (f.ops & KV_OP_WINDOW) kv_launch<&fasn_kvprefill_fwd_fp8_window_kernel<Tag, D>>(grid, kv_fp8_smem(D), s, pp, f.f8, f.kw);
    else kv_launch<&fasn_kvprefill_fwd_fp8_kernel<Tag, D>>(grid, kv_fp8_smem(D), s, pp, f.f8);
    if (p.nsplit > 1) {
        const int64_t nthr = (int64_t)p.B * p.Hkv * pp.nrb * KVP_ROWS * (D / 4);
        FASN_LAUNCH((fasn_kvprefill_fp8_combine_kernel<Tag, D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, pp, f.f8);
    }
    return launch_rc();
}

// the packed forward: the schedule kernel as it is, the forward, and with several splits the FP8 packed combine - the launches, grid and
// split count of kv_launch_packed (fasn_kvvarlen.hip) for the same shape
template <typename Tag, int D>
int kv_launch_fp8_packed_as(const KvFwd& f, hipStream_t s) {
    const KvPrefillParams& pp = f.pp;
    const KvParams& p = pp.kv;
    FASN_LAUNCH(fasn_kvvarlen_schedule_kernel<256>, dim3(1), dim3(256), 0, s, pp, f.pk);
    const unsigned grid = (unsigned)(f.pk.items_max * p.Hkv * p.nsplit);
    if (f.ops & KV_OP_WINDOW) kv_launch<&fasn_kvvarlen_fwd_window_fp8_kernel<Tag, D>>(grid, kv_fp8_smem(D), s, pp, f.pk, f.f8, f.kw);
    else kv_launch<&fasn_kvvarlen_fwd_fp8_kernel<Tag, D>>(grid, kv_fp8_smem(D), s, pp, f.pk, f.f8);
    if (p.nsplit > 1) {
        const int64_t nthr = (int64_t)f.pk.items_max * p.Hkv * KVP_ROWS * (D / 4);
        FASN_LAUNCH((fasn_kvvarlen_fp8_combine_kernel<Tag, D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, pp, f.pk, f.f8);
    }
    return launch_rc();
}

}  // namespace

// the quantising append of any block: decode and prefill rows (b, hkv, i), packed rows (t, hkv)
int kv8_append(const KvArgs& in, const fasn_kv_fp8* fp8, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    KvPrefillParams pp;
    KvPacked pk{};
    KvFp8 f8;
    int rc = kv_build_append(in, k_new, v_new, pp, &pk);
    if (rc) return rc;
    if ((rc = kv_check_fp8(in.a, fp8, f8))) return rc;
    const int64_t rows = in.call == KV_VARLEN ? (int64_t)pk.T : (int64_t)pp.kv.B * pp.kv.Sq;
    const int64_t nthr = rows * pp.kv.Hkv * (in.a->D / 16);
    if ((nthr + 255) / 256 > INT_MAX) return FASN_EINVAL;   // (a prefill's Sq has no limit)
    const dim3 grid((unsigned)((nthr + 255) / 256));
    return kv8_dispatch(in.a->dtype, in.a->D, [&](auto tag, auto d) {
        using Tag = decltype(tag);
        constexpr int D = decltype(d)::value;
        if (in.call == KV_DECODE) FASN_LAUNCH((fasn_kvcache_fp8_append_kernel<Tag, D>), grid, dim3(256), 0, (hipStream_t)stream, pp.kv, f8);
        else if (in.call == KV_PREFILL) FASN_LAUNCH((fasn_kvprefill_fp8_append_kernel<Tag, D>), grid, dim3(256), 0, (hipStream_t)stream, pp, f8);
        else FASN_LAUNCH((fasn_kvvarlen_fp8_append_kernel<Tag, D>), grid, dim3(256), 0, (hipStream_t)stream, pp, pk, f8);
        return launch_rc();
    });
}

int kv_launch_fp8_decode(const KvFwd& f, hipStream_t s) {
    return kv8_dispatch(f.dtype, f.D, [&](auto tag, auto d) { return kv_launch_fp8_decode_as<decltype(tag), decltype(d)::value>(f, s); });
}
int kv_launch_fp8_prefill(const KvFwd& f, hipStream_t s) {
    return kv8_dispatch(f.dtype, f.D, [&](auto tag, auto d) { return kv_launch_fp8_prefill_as<decltype(tag), decltype(d)::value>(f, s); });
}
int kv_launch_fp8_packed(const KvFwd& f, hipStream_t s) {
    return kv8_dispatch(f.dtype, f.D, [&](auto tag, auto d) { return kv_launch_fp8_packed_as<decltype(tag), decltype(d)::value>(f, s); });
}
int kv_launch_fp8_commit(const KvCommit& c, int D, unsigned grid, hipStream_t s) {
    if (D == 64) kv_launch<&fasn_kvcache_fp8_tree_commit_kernel<64>>(grid, 0, s, c);
    else kv_launch<&fasn_kvcache_fp8_tree_commit_kernel<128>>(grid, 0, s, c);
    return launch_rc();
}

}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_fwd_kvcache_fp8_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8) { return kv_workspace_bytes(kv_args(args), kv_ops(fp8)); }

int fasn_fwd_kvcache_fp8(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(fp8), workspace, workspace_bytes, stream);
}

int fasn_kvcache_fp8_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, char* buf, size_t cap) { return kv_forward_plan(kv_args(args), kv_ops(fp8), buf, cap); }

int fasn_kvcache_fp8_append(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kv8_append(kv_args(args), fp8, k_new, v_new, stream);
}

size_t fasn_fwd_kvprefill_fp8_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8) { return kv_workspace_bytes(kv_args(args), kv_ops(fp8)); }

int fasn_fwd_kvprefill_fp8(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(fp8), workspace, workspace_bytes, stream);
}

int fasn_kvprefill_fp8_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, char* buf, size_t cap) { return kv_forward_plan(kv_args(args), kv_ops(fp8), buf, cap); }

int fasn_kvprefill_fp8_append(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kv8_append(kv_args(args), fp8, k_new, v_new, stream);
}

// ---- the sliding window over an FP8 cache
size_t fasn_fwd_kvcache_fp8_window_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window) {
    return kv_workspace_bytes(kv_args(args), kv_ops(fp8, window));
}

int fasn_fwd_kvcache_fp8_window(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window, void* workspace, size_t workspace_bytes,
                                fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(fp8, window), workspace, workspace_bytes, stream);
}

int fasn_kvcache_fp8_window_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window, char* buf, size_t cap) {
    return kv_forward_plan(kv_args(args), kv_ops(fp8, window), buf, cap);
}

size_t fasn_fwd_kvprefill_fp8_window_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window) {
    return kv_workspace_bytes(kv_args(args), kv_ops(fp8, window));
}

int fasn_fwd_kvprefill_fp8_window(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window, void* workspace, size_t workspace_bytes,
                                  fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(fp8, window), workspace, workspace_bytes, stream);
}

int fasn_kvprefill_fp8_window_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window, char* buf, size_t cap) {
    return kv_forward_plan(kv_args(args), kv_ops(fp8, window), buf, cap);
}

// ---- the token tree over an FP8 cache
size_t fasn_fwd_kvcache_fp8_tree_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree) {
    return kv_workspace_bytes(kv_args(args), kv_ops(fp8, tree));
}

int fasn_fwd_kvcache_fp8_tree(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree, void* workspace, size_t workspace_bytes,
                              fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(fp8, tree), workspace, workspace_bytes, stream);
}

int fasn_kvcache_fp8_tree_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree, char* buf, size_t cap) {
    return kv_forward_plan(kv_args(args), kv_ops(fp8, tree), buf, cap);
}

size_t fasn_fwd_kvprefill_fp8_tree_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree) {
    return kv_workspace_bytes(kv_args(args), kv_ops(fp8, tree));
}

int fasn_fwd_kvprefill_fp8_tree(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree, void* workspace, size_t workspace_bytes,
                                fasn_stream_t stream) {
    return kv_forward(kv_args(args), kv_ops(fp8, tree), workspace, workspace_bytes, stream);
}

int fasn_kvprefill_fp8_tree_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree, char* buf, size_t cap) {
    return kv_forward_plan(kv_args(args), kv_ops(fp8, tree), buf, cap);
}

int fasn_kvcache_fp8_tree_commit(const fasn_kv_tree_commit* commit, fasn_stream_t stream) { return kv_commit(commit, true, stream); }

}  // extern "C"
