// fasn_softmax.hip — stand-alone softmax_n over the last dimension (fwd + bwd).
//   y_i = exp(x_i - m) / (n * exp(-m) + sum_j exp(x_j - m)),  m = max(x) (and m >= 0 when n > 0 so that
//   n * exp(-m) cannot overflow) — reference: flash_attention_softmax_n/core/functional.py:15-29. At n == 0 the denominator is the sum
//   alone: softmax_n(x, 0) is softmax(x) for every finite row, the ones below -88 too, where exp(-m) is inf in fp32. A row that is wholly
//   -inf gives 0 when n > 0 (the denominator is n) and NaN when n == 0 (0 / 0, as torch.softmax).
//   dx_i = y_i * (dy_i - sum_j dy_j y_j)   (n enters only through y).
// One workgroup per row at a time, rows taken in a grid-stride loop (the grid is capped: HIP rejects launches of 2^32 or more
// threads, so rows >= 2^24 cannot have a workgroup each); the row is cached in registers when it fits (cols <= 256*EPT), fp32 math.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fasn.h"
#include "fasn_common.h"
#include "fasn_plan.h"

namespace fasn {

template <int DT> struct IO;
template <> struct IO<FASN_DTYPE_F32> {
    typedef float T;
    static FASN_DEV float ld(const void* p, int64_t i) { return ((const float*)p)[i]; }
    static FASN_DEV void st(void* p, int64_t i, float v) { ((float*)p)[i] = v; }
};
template <> struct IO<FASN_DTYPE_BF16> {
    static FASN_DEV float ld(const void* p, int64_t i) { return ET<bf16_tag>::to_f32(((const uint16_t*)p)[i]); }
    static FASN_DEV void st(void* p, int64_t i, float v) { ((__bf16*)p)[i] = (__bf16)v; }
};
template <> struct IO<FASN_DTYPE_F16> {
    static FASN_DEV float ld(const void* p, int64_t i) { return (float)((const _Float16*)p)[i]; }
    static FASN_DEV void st(void* p, int64_t i, float v) { ((_Float16*)p)[i] = (_Float16)v; }
};

template <bool IS_MAX>
FASN_DEV float block_reduce(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o);
        v = IS_MAX ? fmaxf(v, w) : v + w;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) r = IS_MAX ? fmaxf(r, red[i]) : r + red[i];
    return r;
}

constexpr int EPT = 16;  // cached elements per thread
constexpr int64_t kMaxRowGrid = 1 << 20;  // workgroups per launch; more rows than that are walked by the grid-stride loop

template <int DT>
__global__ void __launch_bounds__(256) softmax_n_fwd_kernel(const void* x, void* y, int64_t rows, int64_t cols, int64_t xs, int64_t ys, float n) {
    __shared__ float red[4];
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t xo = row * xs, yo = row * ys;
    const bool cached = cols <= 256 * EPT;
    float v[EPT];
    float mx = -INFINITY;
    if (cached) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int64_t c = threadIdx.x + e * 256;
            v[e] = c < cols ? IO<DT>::ld(x, xo + c) : -INFINITY;
            mx = fmaxf(mx, v[e]);
        }
    } else {
        for (int64_t c = threadIdx.x; c < cols; c += 256) mx = fmaxf(mx, IO<DT>::ld(x, xo + c));
    }
    mx = block_reduce<true>(mx, red);
    if (n > 0.f) mx = fmaxf(mx, 0.f);
    if (mx == -INFINITY) mx = 0.f;  // all -inf, n == 0: exp(-inf) / 0 -> NaN, as torch.softmax
    float sum = 0.f;
    if (cached) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            v[e] = __expf(v[e] - mx);
            sum += v[e];
        }
    } else {
        for (int64_t c = threadIdx.x; c < cols; c += 256) sum += __expf(IO<DT>::ld(x, xo + c) - mx);
    }
    sum = block_reduce<false>(sum, red);
    const float inv = 1.0f / (n > 0.f ? n * __expf(-mx) + sum : sum);   // n == 0: m is not clamped, e^-m may be inf and 0 * inf is NaN
    if (cached) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int64_t c = threadIdx.x + e * 256;
            if (c < cols) IO<DT>::st(y, yo + c, v[e] * inv);
        }
    } else {
        for (int64_t c = threadIdx.x; c < cols; c += 256) IO<DT>::st(y, yo + c, __expf(IO<DT>::ld(x, xo + c) - mx) * inv);
    }
    }
}

template <int DT>
__global__ void __launch_bounds__(256) softmax_n_bwd_kernel(const void* y, const void* dy, void* dx, int64_t rows, int64_t cols, int64_t ys, int64_t dys, int64_t dxs) {
    __shared__ float red[4];
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    float dot = 0.f;
    for (int64_t c = threadIdx.x; c < cols; c += 256) dot += IO<DT>::ld(y, row * ys + c) * IO<DT>::ld(dy, row * dys + c);
    dot = block_reduce<false>(dot, red);
    for (int64_t c = threadIdx.x; c < cols; c += 256)
        IO<DT>::st(dx, row * dxs + c, IO<DT>::ld(y, row * ys + c) * (IO<DT>::ld(dy, row * dys + c) - dot));
    }
}

// ---- one WAVE per row, 16-byte loads, no LDS and no barrier: the row lives in registers (NV 16-byte vectors per lane, so rows of
// up to 512 * NV 16-bit or 256 * NV fp32 elements), max and sum by wave shuffles. Needs 16-byte aligned rows and a row length
// that is a multiple of the vector; everything else takes the workgroup-per-row kernels above. One read and one write of every
// element (backward: two reads, one write): HBM-bound.
template <int DT>
struct VecIO {
    static constexpr int EPV = DT == FASN_DTYPE_F32 ? 4 : 8;   // elements per 16-byte vector
    static FASN_DEV void unpack(u32x4 w, float* f) {
        if constexpr (DT == FASN_DTYPE_F32) {
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = __uint_as_float(w[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (DT == FASN_DTYPE_BF16) {
                    f[2 * e] = __uint_as_float(w[e] << 16);
                    f[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
                } else {
                    f[2 * e] = ET<f16_tag>::to_f32((uint16_t)(w[e] & 0xffffu));
                    f[2 * e + 1] = ET<f16_tag>::to_f32((uint16_t)(w[e] >> 16));
                }
            }
        }
    }
    static FASN_DEV u32x4 pack(const float* f) {
        u32x4 w;
        if constexpr (DT == FASN_DTYPE_F32) {
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = __float_as_uint(f[e]);
        } else if constexpr (DT == FASN_DTYPE_BF16) {
            f32x8 x;
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = f[e];
            const bf16x8 y = __builtin_convertvector(x, bf16x8);
            __builtin_memcpy(&w, &y, 16);
        } else {
            f32x8 x;
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = f[e];
            const f16x8 y = __builtin_convertvector(x, f16x8);
            __builtin_memcpy(&w, &y, 16);
        }
        return w;
    }
};
FASN_DEV float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
FASN_DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int DT, int NV>
__global__ void __launch_bounds__(256) softmax_n_fwd_wave_kernel(const char* x, char* y, int64_t rows, int cols, int64_t xs_bytes, int64_t ys_bytes, float n) {
    constexpr int EPV = VecIO<DT>::EPV;
    const int lane = threadIdx.x & 63;
    const int nvec = cols / EPV;   // vectors per row
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        const u32x4* xr = reinterpret_cast<const u32x4*>(x + row * xs_bytes);
        u32x4 raw[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int vi = lane + 64 * i;
            raw[i] = vi < nvec ? xr[vi] : u32x4{0u, 0u, 0u, 0u};
        }
        float v[NV][EPV];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            VecIO<DT>::unpack(raw[i], v[i]);
            if (lane + 64 * i < nvec) {
#pragma unroll
                for (int e = 0; e < EPV; ++e) mx = fmaxf(mx, v[i][e]);
            }
        }
        mx = wave_max(mx);
        if (n > 0.f) mx = fmaxf(mx, 0.f);
        if (mx == -INFINITY) mx = 0.f;  // all -inf, n == 0: exp(-inf) / 0 -> NaN, as torch.softmax
        // the exponent is (x - m) log2 e with the difference taken first: fma(x, log2 e, -round(m log2 e)) leaves the rounding of m log2 e,
        // 2^-24 |m|, in every exponent - at the maximum itself too, where |m| >= 2^31 turns e^0 into 0 or inf
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const bool ok = lane + 64 * i < nvec;
#pragma unroll
            for (int e = 0; e < EPV; ++e) {
                v[i][e] = ok ? fast_exp2((v[i][e] - mx) * kLog2e) : 0.f;
                sum += v[i][e];
            }
        }
        sum = wave_sum(sum);
        const float inv = 1.0f / (n > 0.f ? n * __expf(-mx) + sum : sum);   // n == 0: m is not clamped, e^-m may be inf and 0 * inf is NaN
        u32x4* yr = reinterpret_cast<u32x4*>(y + row * ys_bytes);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int vi = lane + 64 * i;
#pragma unroll
            for (int e = 0; e < EPV; ++e) v[i][e] *= inv;
            if (vi < nvec) yr[vi] = VecIO<DT>::pack(v[i]);
        }
    }
}

template <int DT, int NV>
__global__ void __launch_bounds__(256) softmax_n_bwd_wave_kernel(const char* y, const char* dy, char* dx, int64_t rows, int cols, int64_t ys_bytes, int64_t dys_bytes, int64_t dxs_bytes) {
    constexpr int EPV = VecIO<DT>::EPV;
    const int lane = threadIdx.x & 63;
    const int nvec = cols / EPV;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        const u32x4* yr = reinterpret_cast<const u32x4*>(y + row * ys_bytes);
        const u32x4* gr = reinterpret_cast<const u32x4*>(dy + row * dys_bytes);
        float yv[NV][EPV], gv[NV][EPV];
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int vi = lane + 64 * i;
            const bool ok = vi < nvec;
            VecIO<DT>::unpack(ok ? yr[vi] : u32x4{0u, 0u, 0u, 0u}, yv[i]);
            VecIO<DT>::unpack(ok ? gr[vi] : u32x4{0u, 0u, 0u, 0u}, gv[i]);
#pragma unroll
            for (int e = 0; e < EPV; ++e) dot = __builtin_fmaf(yv[i][e], gv[i][e], dot);
        }
        dot = wave_sum(dot);
        u32x4* xr = reinterpret_cast<u32x4*>(dx + row * dxs_bytes);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int vi = lane + 64 * i;
#pragma unroll
            for (int e = 0; e < EPV; ++e) yv[i][e] *= gv[i][e] - dot;
            if (vi < nvec) xr[vi] = VecIO<DT>::pack(yv[i]);
        }
    }
}


// ---- one WORKGROUP per row, 16-byte loads, the row in registers (NV vectors per thread: rows of up to 256 * NV vectors = 32768
// 16-bit elements at NV = 16): what the wave kernels do, for rows too long for one wave. One read and one write of every element
// (the element-load kernels above read a long row three times, two bytes per lane: 1.4 TB/s at [4096 x 32768]).
template <int DT, int NV>
__global__ void __launch_bounds__(256) softmax_n_fwd_block_kernel(const char* x, char* y, int64_t rows, int cols, int64_t xs_bytes, int64_t ys_bytes, float n) {
    constexpr int EPV = VecIO<DT>::EPV;
    __shared__ float red[4];
    const int nvec = cols / EPV;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const u32x4* xr = reinterpret_cast<const u32x4*>(x + row * xs_bytes);
        u32x4 raw[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int vi = (int)threadIdx.x + 256 * i;
            raw[i] = vi < nvec ? xr[vi] : u32x4{0u, 0u, 0u, 0u};
        }
        float v[NV][EPV];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            VecIO<DT>::unpack(raw[i], v[i]);
            if ((int)threadIdx.x + 256 * i < nvec) {
#pragma unroll
                for (int e = 0; e < EPV; ++e) mx = fmaxf(mx, v[i][e]);
            }
        }
        mx = block_reduce<true>(mx, red);
        if (n > 0.f) mx = fmaxf(mx, 0.f);
        if (mx == -INFINITY) mx = 0.f;  // all -inf, n == 0: exp(-inf) / 0 -> NaN, as torch.softmax
        float sum = 0.f;   // (the exponent: as in the wave kernel)
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const bool ok = (int)threadIdx.x + 256 * i < nvec;
#pragma unroll
            for (int e = 0; e < EPV; ++e) {
                v[i][e] = ok ? fast_exp2((v[i][e] - mx) * kLog2e) : 0.f;
                sum += v[i][e];
            }
        }
        sum = block_reduce<false>(sum, red);
        const float inv = 1.0f / (n > 0.f ? n * __expf(-mx) + sum : sum);   // n == 0: m is not clamped, e^-m may be inf and 0 * inf is NaN
        u32x4* yr = reinterpret_cast<u32x4*>(y + row * ys_bytes);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int vi = (int)threadIdx.x + 256 * i;
#pragma unroll
            for (int e = 0; e < EPV; ++e) v[i][e] *= inv;
            if (vi < nvec) yr[vi] = VecIO<DT>::pack(v[i]);
        }
    }
}

template <int DT, int NV>
__global__ void __launch_bounds__(256) softmax_n_bwd_block_kernel(const char* y, const char* dy, char* dx, int64_t rows, int cols, int64_t ys_bytes, int64_t dys_bytes, int64_t dxs_bytes) {
    constexpr int EPV = VecIO<DT>::EPV;
    __shared__ float red[4];
    const int nvec = cols / EPV;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const u32x4* yr = reinterpret_cast<const u32x4*>(y + row * ys_bytes);
        const u32x4* gr = reinterpret_cast<const u32x4*>(dy + row * dys_bytes);
        u32x4 yraw[NV], graw[NV];   // kept packed: unpacked once for the dot product and once for the result
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int vi = (int)threadIdx.x + 256 * i;
            const bool ok = vi < nvec;
            yraw[i] = ok ? yr[vi] : u32x4{0u, 0u, 0u, 0u};
            graw[i] = ok ? gr[vi] : u32x4{0u, 0u, 0u, 0u};
            float yv[EPV], gv[EPV];
            VecIO<DT>::unpack(yraw[i], yv);
            VecIO<DT>::unpack(graw[i], gv);
#pragma unroll
            for (int e = 0; e < EPV; ++e) dot = __builtin_fmaf(yv[e], gv[e], dot);
        }
        dot = block_reduce<false>(dot, red);
        u32x4* xr = reinterpret_cast<u32x4*>(dx + row * dxs_bytes);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int vi = (int)threadIdx.x + 256 * i;
            float yv[EPV], gv[EPV];
            VecIO<DT>::unpack(yraw[i], yv);
            VecIO<DT>::unpack(graw[i], gv);
#pragma unroll
            for (int e = 0; e < EPV; ++e) yv[e] *= gv[e] - dot;
            if (vi < nvec) xr[vi] = VecIO<DT>::pack(yv);
        }
    }
}

// ---- dispatch. One function per direction picks the kernel, its NV and its grid from what the call was given; the launchers below and
// the plan calls (fasn_softmax_n_plan: the same entry points under the launch recorder) both go through it.
enum RowKernel { ROW_ELEMENT = 0, ROW_WAVE = 1, ROW_BLOCK = 2 };
struct RowSelect {
    RowKernel kernel;
    int nv;          // 16-byte vectors per lane (wave) or per thread (block); 0 for the element-load kernels
    unsigned grid;
};
static unsigned row_grid(int64_t groups) { return (unsigned)(groups < kMaxRowGrid ? groups : kMaxRowGrid); }
static bool off16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 != 0; }

// forward: wave NV 2 / 4 / 8 / 16 up to 128 / 256 / 512 / 1024 vectors a row, block NV 8 / 16 up to 2048 / 4096; rows that do not move in
// aligned 16-byte pieces, and longer ones, take the element-load kernel
static RowSelect select_fwd(const void* x, const void* y, int64_t rows, int64_t cols, int64_t xs, int64_t ys, int dtype) {
    const int esz = dtype == FASN_DTYPE_F32 ? 4 : 2, EPV = 16 / esz;
    const int64_t nvec = cols / EPV;
    if (cols % EPV || (xs * esz) % 16 || (ys * esz) % 16 || off16(x) || off16(y) || nvec > 256 * 16) return {ROW_ELEMENT, 0, row_grid(rows)};
    if (nvec > 64 * 16) return {ROW_BLOCK, nvec <= 256 * 8 ? 8 : 16, row_grid(rows)};   // too long for one wave's registers
    return {ROW_WAVE, nvec <= 64 * 2 ? 2 : nvec <= 64 * 4 ? 4 : nvec <= 64 * 8 ? 8 : 16, row_grid((rows + 3) / 4)};
}
// backward (two operands in registers): wave NV 2 / 4 / 8 up to 128 / 256 / 512 vectors, block NV 4 / 8 / 16 up to 1024 / 2048 / 4096
static RowSelect select_bwd(const void* y, const void* dy, const void* dx, int64_t rows, int64_t cols, int64_t ys, int64_t dys, int64_t dxs, int dtype) {
    const int esz = dtype == FASN_DTYPE_F32 ? 4 : 2, EPV = 16 / esz;
    const int64_t nvec = cols / EPV;
    if (cols % EPV || (ys * esz) % 16 || (dys * esz) % 16 || (dxs * esz) % 16 || off16(y) || off16(dy) || off16(dx) || nvec > 256 * 16)
        return {ROW_ELEMENT, 0, row_grid(rows)};
    if (nvec > 64 * 8) return {ROW_BLOCK, nvec <= 256 * 4 ? 4 : nvec <= 256 * 8 ? 8 : 16, row_grid(rows)};
    return {ROW_WAVE, nvec <= 64 * 2 ? 2 : nvec <= 64 * 4 ? 4 : 8, row_grid((rows + 3) / 4)};
}

template <int DT>
static int launch_fwd(const void* x, void* y, int64_t rows, int64_t cols, int64_t xs, int64_t ys, float n, hipStream_t s) {
    constexpr int esz = DT == FASN_DTYPE_F32 ? 4 : 2;
    const RowSelect r = select_fwd(x, y, rows, cols, xs, ys, DT);
    const dim3 grid(r.grid);
    const char* xp = (const char*)x;
    char* yp = (char*)y;
#define FASN_SM_FWD(kern, NV) FASN_LAUNCH((kern<DT, NV>), grid, dim3(256), 0, s, xp, yp, rows, (int)cols, xs * esz, ys * esz, n)
    switch (r.kernel * 100 + r.nv) {
        case ROW_WAVE * 100 + 2: FASN_SM_FWD(softmax_n_fwd_wave_kernel, 2); break;
        case ROW_WAVE * 100 + 4: FASN_SM_FWD(softmax_n_fwd_wave_kernel, 4); break;
        case ROW_WAVE * 100 + 8: FASN_SM_FWD(softmax_n_fwd_wave_kernel, 8); break;
        case ROW_WAVE * 100 + 16: FASN_SM_FWD(softmax_n_fwd_wave_kernel, 16); break;
        case ROW_BLOCK * 100 + 8: FASN_SM_FWD(softmax_n_fwd_block_kernel, 8); break;
        case ROW_BLOCK * 100 + 16: FASN_SM_FWD(softmax_n_fwd_block_kernel, 16); break;
        case ROW_ELEMENT * 100: FASN_LAUNCH(softmax_n_fwd_kernel<DT>, grid, dim3(256), 0, s, x, y, rows, cols, xs, ys, n); break;
        default: return FASN_EUNSUPPORTED;   // (a selection without a kernel: not reachable)
    }
#undef FASN_SM_FWD
    return launch_rc();
}
template <int DT>
static int launch_bwd(const void* y, const void* dy, void* dx, int64_t rows, int64_t cols, int64_t ys, int64_t dys, int64_t dxs, hipStream_t s) {
    constexpr int esz = DT == FASN_DTYPE_F32 ? 4 : 2;
    const RowSelect r = select_bwd(y, dy, dx, rows, cols, ys, dys, dxs, DT);
    const dim3 grid(r.grid);
    const char *yp = (const char*)y, *gp = (const char*)dy;
    char* xp = (char*)dx;
#define FASN_SM_BWD(kern, NV) FASN_LAUNCH((kern<DT, NV>), grid, dim3(256), 0, s, yp, gp, xp, rows, (int)cols, ys * esz, dys * esz, dxs * esz)
    switch (r.kernel * 100 + r.nv) {
        case ROW_WAVE * 100 + 2: FASN_SM_BWD(softmax_n_bwd_wave_kernel, 2); break;
        case ROW_WAVE * 100 + 4: FASN_SM_BWD(softmax_n_bwd_wave_kernel, 4); break;
        case ROW_WAVE * 100 + 8: FASN_SM_BWD(softmax_n_bwd_wave_kernel, 8); break;
        case ROW_BLOCK * 100 + 4: FASN_SM_BWD(softmax_n_bwd_block_kernel, 4); break;
        case ROW_BLOCK * 100 + 8: FASN_SM_BWD(softmax_n_bwd_block_kernel, 8); break;
        case ROW_BLOCK * 100 + 16: FASN_SM_BWD(softmax_n_bwd_block_kernel, 16); break;
        case ROW_ELEMENT * 100: FASN_LAUNCH(softmax_n_bwd_kernel<DT>, grid, dim3(256), 0, s, y, dy, dx, rows, cols, ys, dys, dxs); break;
        default: return FASN_EUNSUPPORTED;
    }
#undef FASN_SM_BWD
    return launch_rc();
}

}  // namespace fasn

using namespace fasn;

extern "C" {

int fasn_softmax_n_fwd(const void* x, void* y, int64_t rows, int64_t cols, int64_t x_row_stride, int64_t y_row_stride, float n,
                       int32_t dtype, fasn_stream_t stream) {
    if (x == nullptr || y == nullptr || rows <= 0 || cols <= 0 || !(n >= 0.f)) return FASN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case FASN_DTYPE_F16: return launch_fwd<FASN_DTYPE_F16>(x, y, rows, cols, x_row_stride, y_row_stride, n, s);
        case FASN_DTYPE_BF16: return launch_fwd<FASN_DTYPE_BF16>(x, y, rows, cols, x_row_stride, y_row_stride, n, s);
        case FASN_DTYPE_F32: return launch_fwd<FASN_DTYPE_F32>(x, y, rows, cols, x_row_stride, y_row_stride, n, s);
        default: return FASN_EDTYPE;
    }
}

int fasn_softmax_n_bwd(const void* y, const void* dy, void* dx, int64_t rows, int64_t cols, int64_t y_row_stride, int64_t dy_row_stride,
                       int64_t dx_row_stride, int32_t dtype, fasn_stream_t stream) {
    if (y == nullptr || dy == nullptr || dx == nullptr || rows <= 0 || cols <= 0) return FASN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case FASN_DTYPE_F16: return launch_bwd<FASN_DTYPE_F16>(y, dy, dx, rows, cols, y_row_stride, dy_row_stride, dx_row_stride, s);
        case FASN_DTYPE_BF16: return launch_bwd<FASN_DTYPE_BF16>(y, dy, dx, rows, cols, y_row_stride, dy_row_stride, dx_row_stride, s);
        case FASN_DTYPE_F32: return launch_bwd<FASN_DTYPE_F32>(y, dy, dx, rows, cols, y_row_stride, dy_row_stride, dx_row_stride, s);
        default: return FASN_EDTYPE;
    }
}

int fasn_softmax_n_plan(int32_t which, const void* a, const void* b, const void* c, int64_t rows, int64_t cols, int64_t a_row_stride,
                        int64_t b_row_stride, int64_t c_row_stride, int32_t dtype, char* buf, size_t cap) {
    if (which != FASN_ROW_FWD && which != FASN_ROW_BWD) return FASN_EINVAL;
    return record_plan(buf, cap, [&] {
        return which == FASN_ROW_FWD ? fasn_softmax_n_fwd(a, const_cast<void*>(b), rows, cols, a_row_stride, b_row_stride, 0.f, dtype, nullptr)
                                     : fasn_softmax_n_bwd(a, b, const_cast<void*>(c), rows, cols, a_row_stride, b_row_stride, c_row_stride, dtype, nullptr);
    });
}

}  // extern "C"
