// Packed variable-length training attention (include/fasn.h: fasn_fwd_varlen, fasn_bwd_varlen, fasn_varlen_plan): the
// argument checks, the parameter blocks, the launches and the tail kernel. The forward, dQ and dK/dV kernels are instantiations of the
// rectangular kernels' text on the *_varlen_tag element tags (fasn_common.h): a work item is (sequence, head, block) on a grid sized from
// num_seqs and max_seqlen_*, and takes its offsets and lengths from the two tables in device memory. The *_window entry points
// (fasn_fwd_varlen_window, fasn_bwd_varlen_window, fasn_varlen_window_plan) launch the same kernels on the *_varlen_window_tag
// tags, which walk only the tiles of a sliding window, on the same grids. fasn_varlen_rope / fasn_varlen_rope_plan enter here
// for the packed call's argument checks; the rope operand's checks, the kernel and its launch are fasn_varlen_rope.hip's.
#define FASN_VARLEN_ITEMS 1   // the kernel headers compile the packed variable-length form of their kernels here (fasn_common.h)
#include <hip/hip_runtime.h>
#include <math.h>
#include "fasn.h"
#include "fasn_plan.h"
#include "fasn_bwd_launch.h"
#include "fasn_varlen_rope.h"

namespace fasn {
namespace {

// Rows nobody's sequence owns - tokens at or beyond cu[B] of their side - are written here: o / dq rows 0, lse -inf, dk / dv rows 0. One
// workgroup per 32 tokens; a workgroup whose tokens all belong to sequences (every one of them in a full pack) leaves after two scalar loads.
struct VarlenTail {
    const int* cu_q;
    const int* cu_k;
    int nseq, Tq, Tk, H, Hkv, cpr;   // cpr: 16-byte chunks of a row
    char* qrow;                      // o (forward) or dq (backward): [Tq, H, D]
    int64_t qs_h, qs_t;
    float* lse;                      // forward: [H, Tq]; nullptr in the backward
    char* krow[2];                   // dk, dv (backward): [Tk, Hkv, D]; nullptr in the forward
    int64_t ks_h[2], ks_t[2];
};
constexpr int kTailTokens = 32;
template <int TOK>
__global__ void __launch_bounds__(256) fasn_varlen_tail_kernel(const VarlenTail t) {
    const int endq = min(max(__builtin_amdgcn_readfirstlane(t.cu_q[t.nseq]), 0), t.Tq);
    const int endk = min(max(__builtin_amdgcn_readfirstlane(t.cu_k[t.nseq]), 0), t.Tk);
    const int t0 = (int)blockIdx.x * TOK, t1 = t0 + TOK;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    if (t1 > endq && t0 < t.Tq) {
        const int lo = max(t0, endq), hi = min(t1, t.Tq);
        const int per = t.H * t.cpr;
        for (int i = (int)threadIdx.x; i < (hi - lo) * per; i += 256) {
            const int tok = lo + i / per, h = (i % per) / t.cpr, c = i % t.cpr;
            gstore16(t.qrow + ((int64_t)tok * t.qs_t + (int64_t)h * t.qs_h) * 2 + c * 16, zero);
            if (t.lse != nullptr && c == 0) t.lse[(int64_t)h * t.Tq + tok] = -INFINITY;
        }
    }
    if (t.krow[0] != nullptr && t1 > endk && t0 < t.Tk) {
        const int lo = max(t0, endk), hi = min(t1, t.Tk);
        const int per = t.Hkv * t.cpr;
        for (int i = (int)threadIdx.x; i < (hi - lo) * per; i += 256) {
            const int tok = lo + i / per, h = (i % per) / t.cpr, c = i % t.cpr;
#pragma unroll
            for (int w = 0; w < 2; ++w) gstore16(t.krow[w] + ((int64_t)tok * t.ks_t[w] + (int64_t)h * t.ks_h[w]) * 2 + c * 16, zero);
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace
// a packed operand [1, heads, rows, D] of 16-bit elements: unit feature stride, 16-byte rows, less than 2^31 bytes from its first row to
// the end of its last (the kernels' descriptors and their 32-bit row offsets). (Named in fasn_varlen_rope.h: the rotary launch checks
// its outputs under the same rules.)
int check_packed(const fasn_view4& v, int rows, int D) {
    if (v.ptr == nullptr) return FASN_EINVAL;
    if (v.stride[3] != 1) return FASN_ESTRIDE;
    if (!aligned16(v.ptr) || v.stride[1] % 8 != 0 || v.stride[2] % 8 != 0) return FASN_EALIGN;
    if (v.stride[1] < 0 || v.stride[2] < 0) return FASN_EINVAL;
    if (((int64_t)(rows - 1) * v.stride[2] + D) * 2 >= (1ll << 31)) return FASN_EINVAL;
    return FASN_OK;
}
namespace {

constexpr int kBlock = 128;   // query rows / keys of a work item: four waves x 32

struct VarlenCall {
    FwdParams p;
    int dtype, mode;
    int nqblk, nkblk;
};

// qk_only: the rotary launch (fasn_varlen_rope), which reads q and k alone - the rules of v, o and lse do not apply to it, every other
// rule and code does, in this order
int build_varlen(const fasn_fwd_args* a, const fasn_varlen* vl, const float* n, int64_t n_stride_h, VarlenCall& c, bool qk_only = false) {
    if (a == nullptr || vl == nullptr) return FASN_EINVAL;
    if (vl->cu_seqlens_q == nullptr || vl->cu_seqlens_k == nullptr) return FASN_EINVAL;
    if (vl->num_seqs < 1 || vl->max_seqlen_q < 1 || vl->max_seqlen_k < 1 || vl->reserved != 0) return FASN_EINVAL;
    if (a->B != 1 || a->H <= 0 || a->Sq <= 0 || a->Sk <= 0 || a->D <= 0 || a->Dv <= 0) return FASN_EINVAL;
    if (a->dtype != FASN_DTYPE_F16 && a->dtype != FASN_DTYPE_BF16 && a->dtype != FASN_DTYPE_F32) return FASN_EDTYPE;
    if (n == nullptr && !(a->softmax_n >= 0.f)) return FASN_EINVAL;
    if (!(a->scale >= 0.f) || !isfinite(a->scale)) return FASN_EINVAL;
    if (a->kv_group < 0 || (a->kv_group > 1 && a->H % a->kv_group != 0)) return FASN_EINVAL;
    if (n != nullptr && (n_stride_h < 0 || (int64_t)(a->H - 1) * n_stride_h >= (1ll << 31))) return FASN_EINVAL;
    if (a->D != a->Dv) return FASN_EHEADDIM;
    if (a->dtype == FASN_DTYPE_F32 || a->D != 64) return FASN_EUNSUPPORTED;   // the head dims served: 64
    if (a->mask.ptr != nullptr || a->bias.ptr != nullptr || a->dropout_p != 0.f) return FASN_EUNSUPPORTED;
    // fp16 with a very large scale: the rectangular call takes its element-load kernels there (Q * scale * log2e in the operand type)
    if (a->dtype == FASN_DTYPE_F16 && fabsf(a->scale * kLog2e) > 8.f) return FASN_EUNSUPPORTED;
    int rc;
    if ((rc = check_packed(a->q, a->Sq, a->D))) return rc;
    if ((rc = check_packed(a->k, a->Sk, a->D))) return rc;
    if (!qk_only) {
        if ((rc = check_packed(a->v, a->Sk, a->D))) return rc;
        if ((rc = check_packed(a->o, a->Sq, a->D))) return rc;
        if (a->lse == nullptr) return FASN_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(vl->cu_seqlens_q) % 4 || reinterpret_cast<uintptr_t>(vl->cu_seqlens_k) % 4) return FASN_EALIGN;
    if (!qk_only && (reinterpret_cast<uintptr_t>(a->lse) % 4 || reinterpret_cast<uintptr_t>(n) % 4)) return FASN_EALIGN;

    c.nqblk = (vl->max_seqlen_q + kBlock - 1) / kBlock;
    c.nkblk = (vl->max_seqlen_k + kBlock - 1) / kBlock;
    const int64_t items = (int64_t)vl->num_seqs * a->H * (c.nqblk > c.nkblk ? c.nqblk : c.nkblk);
    if (items >= (1ll << 31)) return FASN_EINVAL;

    FwdParams& p = c.p;
    p = FwdParams{};
    p.q = (const char*)a->q.ptr;
    p.k = (const char*)a->k.ptr;
    p.v = (const char*)a->v.ptr;
    p.o = (char*)a->o.ptr;
    p.lse = a->lse;
    for (int i = 1; i < 3; ++i) {   // (batch strides 0: a work item's "batch element" is its sequence, whose base the kernel derives)
        p.qs[i] = a->q.stride[i];
        p.ks[i] = a->k.stride[i];
        p.vs[i] = a->v.stride[i];
        p.os[i] = a->o.stride[i];
    }
    p.B = vl->num_seqs;
    p.H = a->H;
    p.Sq = a->Sq;
    p.Sk = a->Sk;
    p.causal = a->causal ? 1 : 0;
    p.kvg = a->kv_group > 1 ? a->kv_group : 1;
    p.drop_scale = 1.f;
    p.c = a->scale * kLog2e;
    p.n = n == nullptr ? a->softmax_n : 0.f;
    p.nt = n;
    p.nsb = 0;
    p.nsh = (int)n_stride_h;
    p.kprot = 1;
    p.nsplit = 1;
    // the offset tables, where these instantiations look for them (fasn_fwd_kernel.h: varlen_cu_q / varlen_cu_k)
    p.part_o = reinterpret_cast<float*>(const_cast<int32_t*>(vl->cu_seqlens_q));
    p.part_ml = reinterpret_cast<float*>(const_cast<int32_t*>(vl->cu_seqlens_k));
    c.dtype = a->dtype;
    c.mode = a->causal ? MODE_CAUSAL : MODE_PLAIN;
    return FASN_OK;
}

int launch_tail(const VarlenTail& t, hipStream_t s) {
    const int rows = t.krow[0] != nullptr && t.Tk > t.Tq ? t.Tk : t.Tq;
    FASN_LAUNCH(fasn_varlen_tail_kernel<kTailTokens>, dim3((unsigned)((rows + kTailTokens - 1) / kTailTokens)), dim3(256), 0, s, t);
    return launch_rc();
}

// The schedules of the rectangular launches that assume one length per launch are off: no paired causal blocks, no folded walk, no dynamic
// deal across XCDs, no split-K (pair = 0, xq = nullptr, nsplit = 1 in the block; FOLD = 0 in the instantiation).
template <typename Tag, int MODE>
int launch_fwd_varlen(FwdParams p, int nqblk, hipStream_t s) {
    constexpr int D = 64, QB = 1, OCC = 3, NW = 4, RING = 2, SEED = 2;   // the causal / small-grid tuning point of the rectangular D = 64 forward
    static_assert(NW * QB * 32 == kBlock, "work item: 128 query rows");
    constexpr int smem = fwd_smem(D, RING, MODE, NW, QB);
    constexpr auto kern = &fasn_fwd_kernel<Tag, D, QB, MODE, OCC, NW, 0, 0, RING, 0, SEED>;
    ensure_smem<kern>(smem);
    p.nqblk = nqblk;
    FASN_LAUNCH_MODE(MODE, kern, dim3((unsigned)(nqblk * p.B * p.H)), dim3(NW * 64), smem, s, p);
    return launch_rc();
}

// The one-wave family of fasn_bwd_kernel.h: it serves grouped K/V at D = 64 - the dK/dV kernel sums the query heads of a
// group in its accumulators - and its dQ prologue publishes delta.
template <typename Tag, int MODE>
int launch_bwd_varlen(BwdParams p, int nqblk, int nkblk, hipStream_t s) {
    constexpr int D = 64;
    const int nbh = p.f.B * p.f.H;
    {
        constexpr int smem = 4 * KT * D * 2;
        constexpr auto kern = &fasn_bwd_dq_kernel<Tag, D, 1, MODE, 2>;
        ensure_smem<kern>(smem);
        p.nblk = nqblk;
        FASN_LAUNCH_MODE(MODE, kern, dim3((unsigned)(nqblk * nbh)), dim3(256), smem, s, p);
    }
    {
        constexpr int smem = 4 * QT * D * 2 + 4 * QT * 4;
        constexpr auto kern = &fasn_bwd_dkdv_kernel<Tag, D, 1, MODE, 2, 0, 1>;
        ensure_smem<kern>(smem);
        p.nblk = nkblk;
        FASN_LAUNCH_MODE(MODE, kern, dim3((unsigned)(nkblk * (nbh / p.f.kvg))), dim3(256), smem, s, p);
    }
    return launch_rc();
}

// The window operand of the *_window entry points, checked behind every rule of the base call (the rule of the cache's *_window calls).
// Returns the window the kernels walk under, 0 for none: with window >= max_seqlen_k no key of any sequence lies below a row's window, and
// the call is the causal packed call - its launches, its plan text, its bits.
int check_window(const fasn_fwd_args* a, const fasn_varlen* vl, const fasn_kv_window* win, int& window) {
    if (win == nullptr || win->window < 1 || win->reserved != 0) return FASN_EINVAL;
    if (!a->causal) return FASN_EUNSUPPORTED;
    window = win->window >= vl->max_seqlen_k ? 0 : win->window;
    return FASN_OK;
}

// windowed: the call came through a *_window entry point (win is its operand, checked here)
int fwd_varlen(const fasn_fwd_args* a, const fasn_varlen* vl, const float* n, int64_t n_stride_h, bool windowed, const fasn_kv_window* win, hipStream_t s) {
    VarlenCall c;
    int rc = build_varlen(a, vl, n, n_stride_h, c);
    if (rc) return rc;
    int window = 0;
    if (windowed && (rc = check_window(a, vl, win, window))) return rc;
    VarlenTail t{};
    t.cu_q = vl->cu_seqlens_q;
    t.cu_k = vl->cu_seqlens_k;
    t.nseq = vl->num_seqs;
    t.Tq = a->Sq;
    t.Tk = a->Sk;
    t.H = a->H;
    t.Hkv = a->H / c.p.kvg;
    t.cpr = a->D / 8;
    t.qrow = (char*)a->o.ptr;
    t.qs_h = a->o.stride[1];
    t.qs_t = a->o.stride[2];
    t.lse = a->lse;
    if ((rc = launch_tail(t, s))) return rc;
    if (window > 0) {   // (the window rides in tps: split-K is off in the packed instantiations, which never read it)
        c.p.tps = window;
        return c.dtype == FASN_DTYPE_BF16 ? launch_fwd_varlen<bf16_varlen_window_tag, MODE_CAUSAL>(c.p, c.nqblk, s)
                                          : launch_fwd_varlen<f16_varlen_window_tag, MODE_CAUSAL>(c.p, c.nqblk, s);
    }
    if (c.dtype == FASN_DTYPE_BF16)
        return c.mode == MODE_CAUSAL ? launch_fwd_varlen<bf16_varlen_tag, MODE_CAUSAL>(c.p, c.nqblk, s) : launch_fwd_varlen<bf16_varlen_tag, MODE_PLAIN>(c.p, c.nqblk, s);
    return c.mode == MODE_CAUSAL ? launch_fwd_varlen<f16_varlen_tag, MODE_CAUSAL>(c.p, c.nqblk, s) : launch_fwd_varlen<f16_varlen_tag, MODE_PLAIN>(c.p, c.nqblk, s);
}

int bwd_varlen(const fasn_bwd_args* a, const fasn_varlen* vl, bool windowed, const fasn_kv_window* win, hipStream_t s) {
    if (a == nullptr) return FASN_EINVAL;
    fasn_fwd_args f = a->fwd;
    f.softmax_n = 0.f;   // (the backward reads n through lse alone)
    VarlenCall c;
    int rc = build_varlen(&f, vl, nullptr, 0, c);
    if (rc) return rc;
    if (a->delta == nullptr) return FASN_EINVAL;
    if (a->dbias.ptr != nullptr) return FASN_EUNSUPPORTED;
    if ((rc = check_packed(a->dout, f.Sq, f.D))) return rc;
    if ((rc = check_packed(a->dq, f.Sq, f.D))) return rc;
    if ((rc = check_packed(a->dk, f.Sk, f.D))) return rc;
    if ((rc = check_packed(a->dv, f.Sk, f.D))) return rc;
    if (reinterpret_cast<uintptr_t>(a->delta) % 4) return FASN_EALIGN;
    int window = 0;
    if (windowed && (rc = check_window(&f, vl, win, window))) return rc;
    BwdParams p{};
    p.f = c.p;
    p.dout = (const char*)a->dout.ptr;
    p.dq = (char*)a->dq.ptr;
    p.dk = (char*)a->dk.ptr;
    p.dv = (char*)a->dv.ptr;
    p.delta = a->delta;
    p.scale = f.scale;
    for (int i = 1; i < 3; ++i) {
        p.dos[i] = a->dout.stride[i];
        p.dqs[i] = a->dq.stride[i];
        p.dks[i] = a->dk.stride[i];
        p.dvs[i] = a->dv.stride[i];
    }
    VarlenTail t{};
    t.cu_q = vl->cu_seqlens_q;
    t.cu_k = vl->cu_seqlens_k;
    t.nseq = vl->num_seqs;
    t.Tq = f.Sq;
    t.Tk = f.Sk;
    t.H = f.H;
    t.Hkv = f.H / c.p.kvg;
    t.cpr = f.D / 8;
    t.qrow = (char*)a->dq.ptr;
    t.qs_h = a->dq.stride[1];
    t.qs_t = a->dq.stride[2];
    t.krow[0] = (char*)a->dk.ptr;
    t.krow[1] = (char*)a->dv.ptr;
    t.ks_h[0] = a->dk.stride[1];
    t.ks_t[0] = a->dk.stride[2];
    t.ks_h[1] = a->dv.stride[1];
    t.ks_t[1] = a->dv.stride[2];
    if ((rc = launch_tail(t, s))) return rc;
    if (window > 0) {
        p.f.tps = window;
        return c.dtype == FASN_DTYPE_BF16 ? launch_bwd_varlen<bf16_varlen_window_tag, MODE_CAUSAL>(p, c.nqblk, c.nkblk, s)
                                          : launch_bwd_varlen<f16_varlen_window_tag, MODE_CAUSAL>(p, c.nqblk, c.nkblk, s);
    }
    if (c.dtype == FASN_DTYPE_BF16)
        return c.mode == MODE_CAUSAL ? launch_bwd_varlen<bf16_varlen_tag, MODE_CAUSAL>(p, c.nqblk, c.nkblk, s)
                                     : launch_bwd_varlen<bf16_varlen_tag, MODE_PLAIN>(p, c.nqblk, c.nkblk, s);
    return c.mode == MODE_CAUSAL ? launch_bwd_varlen<f16_varlen_tag, MODE_CAUSAL>(p, c.nqblk, c.nkblk, s)
                                 : launch_bwd_varlen<f16_varlen_tag, MODE_PLAIN>(p, c.nqblk, c.nkblk, s);
}

// fasn_varlen_rope: the base call's rules on the block (q and k are the sources; v, o and lse are not touched), then the rope operand's
// and the launch (fasn_varlen_rope.hip)
int rope_varlen(const fasn_fwd_args* a, const fasn_varlen* vl, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_out, int32_t inverse,
                hipStream_t s) {
    VarlenCall c;
    const int rc = build_varlen(a, vl, nullptr, 0, c, true);
    if (rc) return rc;
    return varlen_rope(a, vl, c.p.kvg, rope, q_out, k_out, inverse, s);
}

}  // namespace
}  // namespace fasn

using namespace fasn;

extern "C" {

int fasn_fwd_varlen(const fasn_fwd_args* args, const fasn_varlen* varlen, const float* n, int64_t n_stride_h, fasn_stream_t stream) {
    return fwd_varlen(args, varlen, n, n_stride_h, false, nullptr, (hipStream_t)stream);
}

int fasn_bwd_varlen(const fasn_bwd_args* args, const fasn_varlen* varlen, fasn_stream_t stream) {
    return bwd_varlen(args, varlen, false, nullptr, (hipStream_t)stream);
}

int fasn_varlen_plan(const fasn_bwd_args* args, const fasn_varlen* varlen, int32_t which, char* buf, size_t cap) {
    if (args == nullptr || (which != FASN_PLAN_FWD && which != FASN_PLAN_BWD)) return FASN_EINVAL;
    return record_plan(buf, cap, [&] {
        return which == FASN_PLAN_FWD ? fwd_varlen(&args->fwd, varlen, nullptr, 0, false, nullptr, nullptr) : bwd_varlen(args, varlen, false, nullptr, nullptr);
    });
}

int fasn_fwd_varlen_window(const fasn_fwd_args* args, const fasn_varlen* varlen, const fasn_kv_window* window, const float* n, int64_t n_stride_h,
                           fasn_stream_t stream) {
    return fwd_varlen(args, varlen, n, n_stride_h, true, window, (hipStream_t)stream);
}

int fasn_bwd_varlen_window(const fasn_bwd_args* args, const fasn_varlen* varlen, const fasn_kv_window* window, fasn_stream_t stream) {
    return bwd_varlen(args, varlen, true, window, (hipStream_t)stream);
}

int fasn_varlen_window_plan(const fasn_bwd_args* args, const fasn_varlen* varlen, const fasn_kv_window* window, int32_t which, char* buf, size_t cap) {
    if (args == nullptr || (which != FASN_PLAN_FWD && which != FASN_PLAN_BWD)) return FASN_EINVAL;
    return record_plan(buf, cap, [&] {
        return which == FASN_PLAN_FWD ? fwd_varlen(&args->fwd, varlen, nullptr, 0, true, window, nullptr) : bwd_varlen(args, varlen, true, window, nullptr);
    });
}

int fasn_varlen_rope(const fasn_fwd_args* args, const fasn_varlen* varlen, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_out,
                     int32_t inverse, fasn_stream_t stream) {
    return rope_varlen(args, varlen, rope, q_out, k_out, inverse, (hipStream_t)stream);
}

int fasn_varlen_rope_plan(const fasn_fwd_args* args, const fasn_varlen* varlen, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_out,
                          int32_t inverse, char* buf, size_t cap) {
    return record_plan(buf, cap, [&] { return rope_varlen(args, varlen, rope, q_out, k_out, inverse, nullptr); });
}

}  // extern "C"
