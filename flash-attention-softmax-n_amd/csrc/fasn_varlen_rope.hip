// Rotary position embedding on the packed variable-length training call (include/fasn.h: fasn_varlen_rope, fasn_varlen_rope_plan;
// DESIGN.md 4.27): ONE launch in front of fasn_fwd_varlen that rotates the packed q and k rows at per-sequence positions, and - with
// `inverse` - the transpose rotation that the backward applies to dq / dk where fasn_bwd_varlen left them.
//
// Positions (the cache calls' rule, per sequence, from the two offset tables in device memory): with [q0, q1) / [k0, k1) the token ranges
// of sequence b as the attention kernels clamp them (varlen_range, fasn_fwd_kernel.h), key token k0 + j sits at j and query token q0 + i
// at i + (k1 - k0) - (q1 - q0); the table row is clamp(pos, 0, rows - 1). A token of no sequence is neither read nor written.
//
// Work. The grid follows the TOKEN ROWS, not (sequence, block): ceil(Tq / 16) workgroups for the query side, then ceil(Tk / 16) for the
// key side - shapes only. A workgroup of 16 tokens finds, with wave-uniform (scalar) binary searches in the side's offsets, the sequence
// index range its first and its last token can belong to - at most ceil(log2(B + 1)) dependent scalar loads each -, its first 16 lanes
// then search that range for their own token (no step when the workgroup lies inside one sequence: the usual case) and leave the position
// in LDS. After the barrier lane i owns unit (token, head, u) = i, i + 256, ... and sends it through the text of fasn_kvrope_unit.inc -
// the cache's rotation, rounding for rounding: two 16-byte loads, two 16-byte stores and the table vectors per unit, nothing else. A lane
// reads both chunks of its unit before it writes them and no other lane touches them: q_out / k_out may be the sources themselves.
//
// Whatever the offsets hold, no access leaves the operands and the tables: a token index is below the side's rows by the grid, a
// sequence index lies in [0, B), offsets are clamped as the attention kernels clamp them, the table row is clamped.
#include <limits.h>
#include "fasn_kvrope.h"
#include "fasn_plan.h"
#include "fasn_varlen_rope.h"

namespace fasn {

struct VarlenRopeParams {
    const char* src[2];   // q, k: [rows, heads, D] by strides
    char* dst[2];         // q_out, k_out
    int64_t ss_h[2], ss_t[2], ds_h[2], ds_t[2];   // element strides between heads / tokens
    const int* cu[2];     // cu_seqlens_q, cu_seqlens_k: [nseq + 1], device
    int T[2];             // token rows of the side
    int heads[2];         // H, Hkv
    int nseq, nqblk;      // nqblk: the workgroups of the query side
    const char* cos;      // [rows][rd / 2]
    const char* sin;
    int64_t trs;          // table row stride, elements
    int rows;             // table rows, >= max_seqlen_k
    int rd;               // rotary_dim
    int tf32;             // tables are fp32 (otherwise the 16-bit type of the call)
    int interleaved;
    int inverse;          // the transpose rotation
};

constexpr int kRopeTokens = 16;   // tokens of a workgroup

template <typename Tag>
FASN_DEV void varlen_rope_unit(const VarlenRopeParams& rp, int u, const char* src, char* dst, int64_t pos) {
#define FASN_KVROPE_INVERSE 1
#include "fasn_kvrope_unit.inc"
#undef FASN_KVROPE_INVERSE
}

// the first index in [lo, hi] whose offset lies beyond token t, given that cu[hi] does (or that hi bounds the answer); reads cu[lo .. hi - 1]
FASN_DEV int varlen_rope_beyond(const int* cu, int t, int lo, int hi) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cu[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <typename Tag, int D>
__global__ void __launch_bounds__(256) fasn_varlen_rope_kernel(const VarlenRopeParams rp) {
    constexpr int UPR = D / 16, TOK = kRopeTokens;   // units per row
    constexpr int NONE = INT_MIN;
    __shared__ int s_pos[TOK];
    const int side = (int)blockIdx.x < rp.nqblk ? 0 : 1;
    const int* const cu = rp.cu[side];
    const int T = rp.T[side];
    const int t0 = ((int)blockIdx.x - (side ? rp.nqblk : 0)) * TOK;
    const int end = min(max(__builtin_amdgcn_readfirstlane(cu[rp.nseq]), 0), T);
    if (t0 >= end) return;   // (wave-uniform) tokens of no sequence
    const int ntok = min(TOK, end - t0);
    // cu[nseq] >= end > every token here: the searches end at an index <= nseq, and the sequence index below it is < nseq
    const int i0 = __builtin_amdgcn_readfirstlane(varlen_rope_beyond(cu, t0, 0, rp.nseq));
    const int i1 = __builtin_amdgcn_readfirstlane(varlen_rope_beyond(cu, t0 + ntok - 1, i0, rp.nseq));
    if ((int)threadIdx.x < ntok) {
        const int t = t0 + (int)threadIdx.x;
        const int b = varlen_rope_beyond(cu, t, i0, i1) - 1;   // in [-1, nseq - 1]
        int pos = NONE;
        if (b >= 0) {
            // the sequence's ranges as varlen_range clamps them (per lane here: the tokens of a workgroup may belong to several sequences)
            const int s0 = min(max(cu[b], 0), T), s1 = min(max(cu[b + 1], s0), T);
            if (t >= s0 && t < s1) {
                pos = t - s0;
                if (side == 0) {
                    const int k0 = min(max(rp.cu[1][b], 0), rp.T[1]), k1 = min(max(rp.cu[1][b + 1], k0), rp.T[1]);
                    pos += (k1 - k0) - (s1 - s0);
                }
            }
        }
        s_pos[threadIdx.x] = pos;
    }
    __syncthreads();
    const int per = rp.heads[side] * UPR;
    const char* const src = rp.src[side];
    char* const dst = rp.dst[side];
    const int64_t ss_h = rp.ss_h[side], ss_t = rp.ss_t[side], ds_h = rp.ds_h[side], ds_t = rp.ds_t[side];
    for (int i = (int)threadIdx.x; i < ntok * per; i += 256) {
        const int tl = i / per, r = i - tl * per;
        const int h = r / UPR, u = r % UPR;
        const int pos = s_pos[tl];
        if (pos == NONE) continue;
        const int64_t tok = t0 + tl;
        varlen_rope_unit<Tag>(rp, u, src + (tok * ss_t + h * ss_h) * 2, dst + (tok * ds_t + h * ds_h) * 2, pos);
    }
}

namespace {
bool rope_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

int varlen_rope(const fasn_fwd_args* a, const fasn_varlen* vl, int kvg, const fasn_kv_rope* r, const fasn_view4* q_out, const fasn_view4* k_out,
                int32_t inverse, hipStream_t s) {
    // the rope operand, rule for rule and code for code as the cache's rotary calls check it (fasn_kvrope.hip: kvr_build)
    if (r == nullptr || r->cos == nullptr || r->sin == nullptr || q_out == nullptr || k_out == nullptr) return FASN_EINVAL;
    if (r->rotary_dim < 16 || r->rotary_dim > a->D || r->rotary_dim % 16 != 0) return FASN_EINVAL;
    if (r->rows < vl->max_seqlen_k) return FASN_EINVAL;
    if (r->interleaved != 0 && r->interleaved != 1) return FASN_EINVAL;
    if (r->table_dtype != FASN_DTYPE_F32 && r->table_dtype != a->dtype) return FASN_EDTYPE;
    const int64_t esize = r->table_dtype == FASN_DTYPE_F32 ? 4 : 2;
    if (r->row_stride < r->rotary_dim / 2) return FASN_EINVAL;   // (rows overlap)
    if (!rope_aligned16(r->cos) || !rope_aligned16(r->sin) || (r->row_stride * esize) % 16 != 0) return FASN_EALIGN;
    int rc;
    if ((rc = check_packed(*q_out, a->Sq, a->D))) return rc;
    if ((rc = check_packed(*k_out, a->Sk, a->D))) return rc;
    if (inverse != 0 && inverse != 1) return FASN_EINVAL;

    VarlenRopeParams rp{};
    const fasn_view4* const src[2] = {&a->q, &a->k};
    const fasn_view4* const dst[2] = {q_out, k_out};
    for (int i = 0; i < 2; ++i) {
        rp.src[i] = static_cast<const char*>(src[i]->ptr);
        rp.dst[i] = static_cast<char*>(dst[i]->ptr);
        rp.ss_h[i] = src[i]->stride[1];
        rp.ss_t[i] = src[i]->stride[2];
        rp.ds_h[i] = dst[i]->stride[1];
        rp.ds_t[i] = dst[i]->stride[2];
    }
    rp.cu[0] = vl->cu_seqlens_q;
    rp.cu[1] = vl->cu_seqlens_k;
    rp.T[0] = a->Sq;
    rp.T[1] = a->Sk;
    rp.heads[0] = a->H;
    rp.heads[1] = a->H / kvg;
    rp.nseq = vl->num_seqs;
    rp.nqblk = (a->Sq + kRopeTokens - 1) / kRopeTokens;
    rp.cos = static_cast<const char*>(r->cos);
    rp.sin = static_cast<const char*>(r->sin);
    rp.trs = r->row_stride;
    rp.rows = r->rows;
    rp.rd = r->rotary_dim;
    rp.tf32 = r->table_dtype == FASN_DTYPE_F32 ? 1 : 0;
    rp.interleaved = r->interleaved;
    rp.inverse = inverse;
    const dim3 grid((unsigned)(rp.nqblk + (a->Sk + kRopeTokens - 1) / kRopeTokens));
    constexpr auto kern_bf16 = &fasn_varlen_rope_kernel<bf16_tag, 64>;
    constexpr auto kern_f16 = &fasn_varlen_rope_kernel<f16_tag, 64>;
    if (a->dtype == FASN_DTYPE_BF16) FASN_LAUNCH(kern_bf16, grid, dim3(256), 0, s, rp);
    else FASN_LAUNCH(kern_f16, grid, dim3(256), 0, s, rp);
    return launch_rc();
}

}  // namespace fasn
