// Gradient of a per-(batch, head) softmax_n: the two reduction kernels behind fasn_bwd_dn (math and contract: fasn_bwd_dn.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include "fasn.h"
#include "fasn_common.h"
#include "fasn_bwd_dn.h"

namespace fasn {
namespace {

// dot product of the 16-byte pieces a and b of one O row and the matching dO row, in fp32
template <int DT>
FASN_DEV float dot16(const u32x4 a, const u32x4 b) {
    float s = 0.f;
    if constexpr (DT == FASN_DTYPE_BF16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s = fmaf(__uint_as_float(a[e] << 16), __uint_as_float(b[e] << 16), s);
            s = fmaf(__uint_as_float(a[e] & 0xffff0000u), __uint_as_float(b[e] & 0xffff0000u), s);
        }
    } else if constexpr (DT == FASN_DTYPE_F16) {
        const f16x8 x = __builtin_bit_cast(f16x8, a), y = __builtin_bit_cast(f16x8, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf((float)x[e], (float)y[e], s);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(__uint_as_float(a[e]), __uint_as_float(b[e]), s);
    }
    return s;
}

// sum over the workgroup in a fixed order (wave butterflies, then the waves in index order); the result is valid in thread 0
FASN_DEV float block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float t = 0.f;
    if (tid == 0)
        for (int w = 0; w < kDnThreads / 64; ++w) t += red[w];
    return t;
}

// stage 1: workgroup (b, h, chunk) -> part[bh][chunk] = sum over its rows of delta_i exp(-lse_i). A group of cpr lanes covers one row
// (lane `sub` takes the 16-byte piece sub of O and of dO); kDnIters rows per group are loaded before any arithmetic.
template <int DT>
__global__ void __launch_bounds__(kDnThreads) fasn_bwd_dn_partial_kernel(const DnParams p) {
    __shared__ float red[kDnThreads / 64];
    const int bh = (int)(blockIdx.x / (unsigned)p.nchunk), chunk = (int)(blockIdx.x % (unsigned)p.nchunk);
    const int b = bh / p.H, h = bh % p.H;
    const int tid = threadIdx.x, cpr = p.cpr, sub = tid & (cpr - 1), rpp = kDnThreads / cpr;
    const int row0 = chunk * p.rpw + tid / cpr;
    const char* ob = p.o + (b * p.os[0] + h * p.os[1]) * (DT == FASN_DTYPE_F32 ? 4 : 2) + sub * 16;
    const char* gb = p.dout + (b * p.dos[0] + h * p.dos[1]) * (DT == FASN_DTYPE_F32 ? 4 : 2) + sub * 16;
    const int64_t osr = p.os[2] * (DT == FASN_DTYPE_F32 ? 4 : 2), gsr = p.dos[2] * (DT == FASN_DTYPE_F32 ? 4 : 2);
    u32x4 a[kDnIters], g[kDnIters];
#pragma unroll
    for (int it = 0; it < kDnIters; ++it) {
        const int row = row0 + it * rpp;
        a[it] = g[it] = u32x4{0u, 0u, 0u, 0u};
        if (row < p.Sq) {
            a[it] = *reinterpret_cast<const u32x4*>(ob + row * osr);
            g[it] = *reinterpret_cast<const u32x4*>(gb + row * gsr);
        }
    }
    float acc = 0.f;
#pragma unroll
    for (int it = 0; it < kDnIters; ++it) {
        const int row = row0 + it * rpp;
        float d = dot16<DT>(a[it], g[it]);
        for (int o = cpr >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o);   // delta of the row (the group's lanes are one wave's)
        if (sub == 0 && row < p.Sq) {
            const float l = p.lse[(int64_t)bh * p.Sq + row];
            // (a row whose delta is exactly 0 - dO = 0, a pad row no loss reads - adds 0 even where exp(-lse) overflows: under an additive mask
            // such a row of a head with n = 0 has lse = -V, and 0 * inf would be NaN)
            acc += (l < -kLseFloor || d == 0.f) ? 0.f : d * expf(-l);
        }
    }
    const float t = block_sum(acc, red);
    if (tid == 0) p.part[blockIdx.x] = t;
}

// stage 2: workgroup (bo, ho) -> dn[bo * dsb + ho * dsh] = -(sum of the partial sums of every (b, h) it covers), fixed order
__global__ void __launch_bounds__(kDnThreads) fasn_bwd_dn_final_kernel(const DnParams p) {
    __shared__ float red[kDnThreads / 64];
    const int bo = (int)blockIdx.x / p.Ho, ho = (int)blockIdx.x % p.Ho;
    const int nb = p.Bo == 1 ? p.B : 1, nh = p.Ho == 1 ? p.H : 1;
    const int64_t items = (int64_t)nb * nh * p.nchunk;
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < items; i += kDnThreads) {
        const int c = (int)(i % p.nchunk);
        const int64_t r = i / p.nchunk;
        const int b = p.Bo == 1 ? (int)(r / nh) : bo, h = p.Ho == 1 ? (int)(r % nh) : ho;
        acc += p.part[((int64_t)b * p.H + h) * p.nchunk + c];
    }
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) p.dn[bo * p.dsb + ho * p.dsh] = -t;
}

}  // namespace

int launch_bwd_dn(const DnParams& p, int dtype, hipStream_t s) {
    const unsigned g1 = (unsigned)((int64_t)p.B * p.H * p.nchunk);
    switch (dtype) {
        case FASN_DTYPE_F16: hipLaunchKernelGGL(fasn_bwd_dn_partial_kernel<FASN_DTYPE_F16>, dim3(g1), dim3(kDnThreads), 0, s, p); break;
        case FASN_DTYPE_BF16: hipLaunchKernelGGL(fasn_bwd_dn_partial_kernel<FASN_DTYPE_BF16>, dim3(g1), dim3(kDnThreads), 0, s, p); break;
        case FASN_DTYPE_F32: hipLaunchKernelGGL(fasn_bwd_dn_partial_kernel<FASN_DTYPE_F32>, dim3(g1), dim3(kDnThreads), 0, s, p); break;
        default: return FASN_EDTYPE;
    }
    if (hipGetLastError() != hipSuccess) return FASN_ELAUNCH;
    hipLaunchKernelGGL(fasn_bwd_dn_final_kernel, dim3((unsigned)(p.Bo * p.Ho)), dim3(kDnThreads), 0, s, p);
    return hipGetLastError() == hipSuccess ? FASN_OK : FASN_ELAUNCH;
}

}  // namespace fasn
