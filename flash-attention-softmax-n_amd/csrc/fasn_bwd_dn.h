// fasn_bwd_dn.h — gradient of a per-(batch, head) softmax_n (fasn_bwd_dn, include/fasn.h).
//
//   Z_i = n + sum_j exp(x_ij) = exp(lse_i),  O_i = sum_j exp(x_ij) v_j / Z_i   ->   dO_i/dn = -O_i / Z_i
//   dL/dn_(b,h) = - sum_i delta_i exp(-lse_i),   delta_i = dO_i . O_i
// (under dropout O is the dropped output and the identity holds unchanged). A row with lse = -inf (no visible key, n = 0) adds 0,
// and so does a row whose delta is exactly 0, whatever its lse (0 * exp(+big) would be NaN).
// Bandwidth-bound: O and dO are read once, plus lse. Deterministic: a fixed-order two-stage reduction, no atomics -
// stage 1 writes one partial sum per (b, h, row chunk), stage 2 sums them per output element (over batch and / or heads when the
// output broadcasts there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fasn {

struct DnParams {
    const char* o;
    const char* dout;
    const float* lse;           // [B,H,Sq] contiguous
    int64_t os[3], dos[3];      // element strides (batch, head, row); feature stride 1
    int B, H, Sq;
    int cpr;                    // 16-byte chunks per row (Dv * element size / 16): a power of two, 4 .. 32
    int rpw;                    // rows per stage-1 workgroup
    int nchunk;                 // stage-1 workgroups per (b, h)
    float* part;                // [B*H][nchunk] partial sums (caller's workspace)
    float* dn;                  // out: [Bo][Ho] addressed by (dsb, dsh)
    int64_t dsb, dsh;
    int Bo, Ho;                 // 1 = summed over that dimension
};

constexpr int kDnThreads = 256;
constexpr int kDnIters = 8;     // rows per thread group and stage-1 workgroup: rpw = kDnIters * kDnThreads / cpr

inline int dn_rows_per_workgroup(int cpr) { return kDnIters * (kDnThreads / cpr); }

// dtype: FASN_DTYPE_* of O / dO
int launch_bwd_dn(const DnParams& p, int dtype, hipStream_t s);

}  // namespace fasn
