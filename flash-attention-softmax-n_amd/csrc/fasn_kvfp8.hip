// FP8 K/V cache (include/fasn.h: fasn_fwd_kvcache_fp8, fasn_fwd_kvprefill_fp8, their *_workspace_bytes, *_plan and *_append calls, the
// *_fp8_window and *_fp8_tree siblings of the forwards, and fasn_kvcache_fp8_tree_commit): the entry points and the launches of fasn_kvfp8.h
// (its rotate-quantise-appends are launched from fasn_kvrope.hip, beside the rope operand's checks). The argument checks, the FP8 operand's
// check, the window's rule, the tree operand's check, the commit block's checks, the launch plan and the workspace rule are the family's
// (fasn_kv_host.h, defined in fasn_kvcache.hip), called here with a decode or a prefill block.
#include <limits.h>
#include "fasn_kv_host.h"
#include "fasn_kvfp8.h"

namespace fasn {
namespace {

// dtype x the two head dims the FP8 kernels are built for (kv_check_fp8 let only these through)
template <typename F>
int kv8_dispatch(int dtype, int D, F f) {
    if (dtype == FASN_DTYPE_BF16) return D == 64 ? f(bf16_tag{}, std::integral_constant<int, 64>{}) : f(bf16_tag{}, std::integral_constant<int, 128>{});
    return D == 64 ? f(f16_tag{}, std::integral_constant<int, 64>{}) : f(f16_tag{}, std::integral_constant<int, 128>{});
}

// the forward of f.variant: the FP8 kernel, or its sliding-window or token-tree sibling on the same LDS
template <auto Kern, auto Window, auto Tree, typename P>
void kv8_launch_fwd(const KvFwd& f, const P& p, unsigned grid, int smem, hipStream_t s) {
    if (f.variant == KV_FP8_TREE) {
        ensure_smem<Tree>(smem);
        FASN_LAUNCH(Tree, dim3(grid), dim3(256), smem, s, p, f.f8, f.kt);
    } else if (f.variant == KV_FP8_WINDOW) {
        ensure_smem<Window>(smem);
        FASN_LAUNCH(Window, dim3(grid), dim3(256), smem, s, p, f.f8, f.kw);
    } else {
        ensure_smem<Kern>(smem);
        FASN_LAUNCH(Kern, dim3(grid), dim3(256), smem, s, p, f.f8);
    }
}

// decode: the forward and, always, the combine
template <typename Tag, int D>
int kv8_decode(const KvFwd& f, hipStream_t s) {
    const KvParams& p = f.pp.kv;
    const unsigned grid = (unsigned)(p.B * p.Hkv * p.nsplit);
    kv8_launch_fwd<&fasn_kvcache_fwd_fp8_kernel<Tag, D>, &fasn_kvcache_fwd_fp8_window_kernel<Tag, D>, &fasn_kvcache_fwd_fp8_tree_kernel<Tag, D>>(f, p, grid, kv_fp8_smem(D), s);
    const int64_t nthr = (int64_t)p.B * p.Hkv * p.R * (D / 4);
    FASN_LAUNCH((fasn_kvcache_fp8_combine_kernel<Tag, D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, p, f.f8);
    return launch_rc();
}
// prefill: one split stores o / lse itself
template <typename Tag, int D>
int kv8_prefill(const KvFwd& f, hipStream_t s) {
    const KvPrefillParams& pp = f.pp;
    const KvParams& p = pp.kv;
    const unsigned grid = (unsigned)(p.B * p.Hkv * pp.nrb * p.nsplit);
    kv8_launch_fwd<&fasn_kvprefill_fwd_fp8_kernel<Tag, D>, &fasn_kvprefill_fwd_fp8_window_kernel<Tag, D>, &fasn_kvprefill_fwd_fp8_tree_kernel<Tag, D>>(f, pp, grid, kv_fp8_smem(D), s);
    if (p.nsplit > 1) {
        const int64_t nthr = (int64_t)p.B * p.Hkv * pp.nrb * KVP_ROWS * (D / 4);
        FASN_LAUNCH((fasn_kvprefill_fp8_combine_kernel<Tag, D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, pp, f.f8);
    }
    return launch_rc();
}

// `variant` / `operand`: KV_FP8 with the fasn_kv_fp8, or KV_FP8_WINDOW / KV_FP8_TREE with the pair of operands their entry points take (a
// NULL window or tree operand of theirs is refused by that operand's rule, not taken for "none")
template <typename Args>
int kv8_forward(const Args* args, KvVariant variant, const void* operand, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    KvFwd f;
    const KvArgs in = kv_args(args);
    const int rc = kv_build_forward(in, variant, operand, workspace, workspace_bytes, f);
    if (rc) return rc;
    return kv8_dispatch(in.a->dtype, in.a->D, [&](auto tag, auto d) {
        if (in.call == KV_DECODE) return kv8_decode<decltype(tag), decltype(d)::value>(f, (hipStream_t)stream);
        return kv8_prefill<decltype(tag), decltype(d)::value>(f, (hipStream_t)stream);
    });
}

template <typename Args>
int kv8_append(const Args* args, const fasn_kv_fp8* fp8, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    KvPrefillParams pp;
    KvFp8 f8;
    const KvArgs in = kv_args(args);
    int rc = kv_build_append(in, k_new, v_new, pp);
    if (rc) return rc;
    if ((rc = kv_check_fp8(in.a, fp8, f8))) return rc;
    const int64_t nthr = (int64_t)pp.kv.B * pp.kv.Hkv * pp.kv.Sq * (in.a->D / 16);
    if ((nthr + 255) / 256 > INT_MAX) return FASN_EINVAL;   // (a prefill's Sq has no limit)
    const dim3 grid((unsigned)((nthr + 255) / 256));
    return kv8_dispatch(in.a->dtype, in.a->D, [&](auto tag, auto d) {
        using Tag = decltype(tag);
        constexpr int D = decltype(d)::value;
        if (in.call == KV_DECODE) FASN_LAUNCH((fasn_kvcache_fp8_append_kernel<Tag, D>), grid, dim3(256), 0, (hipStream_t)stream, pp.kv, f8);
        else FASN_LAUNCH((fasn_kvprefill_fp8_append_kernel<Tag, D>), grid, dim3(256), 0, (hipStream_t)stream, pp, f8);
        return launch_rc();
    });
}

template <typename Args>
int kv8_plan(const Args* args, KvVariant variant, const void* operand, char* buf, size_t cap) {
    return kv_plan(buf, cap, [&] { return kv8_forward(args, variant, operand, kv_plan_workspace(), ~size_t(0), nullptr); });
}

// fasn_kvcache_fp8_tree_commit: the commit block's checks under the rules of a cache of codes, one launch
template <int D>
int kv8_launch_commit(const KvCommit& c, hipStream_t s) {
    const int64_t nthr = (int64_t)c.B * c.Hkv * (D / 16);
    if ((nthr + 255) / 256 > INT_MAX) return FASN_EINVAL;
    FASN_LAUNCH((fasn_kvcache_fp8_tree_commit_kernel<D>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, c);
    return launch_rc();
}
int kv8_commit(const fasn_kv_tree_commit* a, fasn_stream_t stream) {
    KvCommit c{};
    const int rc = kv_build_commit(a, true, c);
    if (rc) return rc;
    return a->D == 64 ? kv8_launch_commit<64>(c, (hipStream_t)stream) : kv8_launch_commit<128>(c, (hipStream_t)stream);
}

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

size_t fasn_fwd_kvcache_fp8_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8) { return kv_workspace_bytes(kv_args(args), KV_FP8, fp8); }

int fasn_fwd_kvcache_fp8(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv8_forward(args, KV_FP8, fp8, workspace, workspace_bytes, stream);
}

int fasn_kvcache_fp8_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, char* buf, size_t cap) { return kv8_plan(args, KV_FP8, fp8, buf, cap); }

int fasn_kvcache_fp8_append(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kv8_append(args, fp8, k_new, v_new, stream);
}

size_t fasn_fwd_kvprefill_fp8_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8) { return kv_workspace_bytes(kv_args(args), KV_FP8, fp8); }

int fasn_fwd_kvprefill_fp8(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, void* workspace, size_t workspace_bytes, fasn_stream_t stream) {
    return kv8_forward(args, KV_FP8, fp8, workspace, workspace_bytes, stream);
}

int fasn_kvprefill_fp8_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, char* buf, size_t cap) { return kv8_plan(args, KV_FP8, fp8, buf, cap); }

int fasn_kvprefill_fp8_append(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_view4* k_new, const fasn_view4* v_new, fasn_stream_t stream) {
    return kv8_append(args, fp8, k_new, v_new, stream);
}

// ---- the sliding window over an FP8 cache: the FP8 operand's checks, then the window's rule and the 16-bit window call's plan
size_t fasn_fwd_kvcache_fp8_window_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window) {
    const KvFp8Window both{fp8, window};
    return kv_workspace_bytes(kv_args(args), KV_FP8_WINDOW, &both);
}

int fasn_fwd_kvcache_fp8_window(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window, void* workspace, size_t workspace_bytes,
                                fasn_stream_t stream) {
    const KvFp8Window both{fp8, window};
    return kv8_forward(args, KV_FP8_WINDOW, &both, workspace, workspace_bytes, stream);
}

int fasn_kvcache_fp8_window_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window, char* buf, size_t cap) {
    const KvFp8Window both{fp8, window};
    return kv8_plan(args, KV_FP8_WINDOW, &both, buf, cap);
}

size_t fasn_fwd_kvprefill_fp8_window_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window) {
    const KvFp8Window both{fp8, window};
    return kv_workspace_bytes(kv_args(args), KV_FP8_WINDOW, &both);
}

int fasn_fwd_kvprefill_fp8_window(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window, void* workspace, size_t workspace_bytes,
                                  fasn_stream_t stream) {
    const KvFp8Window both{fp8, window};
    return kv8_forward(args, KV_FP8_WINDOW, &both, workspace, workspace_bytes, stream);
}

int fasn_kvprefill_fp8_window_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_window* window, char* buf, size_t cap) {
    const KvFp8Window both{fp8, window};
    return kv8_plan(args, KV_FP8_WINDOW, &both, buf, cap);
}

// ---- the token tree over an FP8 cache: the FP8 operand's checks, then the tree operand's and the 16-bit tree call's plan
size_t fasn_fwd_kvcache_fp8_tree_workspace_bytes(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree) {
    const KvFp8Tree both{fp8, tree};
    return kv_workspace_bytes(kv_args(args), KV_FP8_TREE, &both);
}

int fasn_fwd_kvcache_fp8_tree(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree, void* workspace, size_t workspace_bytes,
                              fasn_stream_t stream) {
    const KvFp8Tree both{fp8, tree};
    return kv8_forward(args, KV_FP8_TREE, &both, workspace, workspace_bytes, stream);
}

int fasn_kvcache_fp8_tree_plan(const fasn_kvcache_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree, char* buf, size_t cap) {
    const KvFp8Tree both{fp8, tree};
    return kv8_plan(args, KV_FP8_TREE, &both, buf, cap);
}

size_t fasn_fwd_kvprefill_fp8_tree_workspace_bytes(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree) {
    const KvFp8Tree both{fp8, tree};
    return kv_workspace_bytes(kv_args(args), KV_FP8_TREE, &both);
}

int fasn_fwd_kvprefill_fp8_tree(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree, void* workspace, size_t workspace_bytes,
                                fasn_stream_t stream) {
    const KvFp8Tree both{fp8, tree};
    return kv8_forward(args, KV_FP8_TREE, &both, workspace, workspace_bytes, stream);
}

int fasn_kvprefill_fp8_tree_plan(const fasn_kvprefill_args* args, const fasn_kv_fp8* fp8, const fasn_kv_tree* tree, char* buf, size_t cap) {
    const KvFp8Tree both{fp8, tree};
    return kv8_plan(args, KV_FP8_TREE, &both, buf, cap);
}

int fasn_kvcache_fp8_tree_commit(const fasn_kv_tree_commit* commit, fasn_stream_t stream) { return kv8_commit(commit, stream); }

}  // extern "C"
