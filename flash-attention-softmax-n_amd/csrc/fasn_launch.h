// fasn_launch.h — host-side launch plumbing shared by the per-head-dim translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <typeinfo>
#include "fasn_fwd_kernel.h"

namespace fasn {

struct FwdLaunch {
    int dtype;    // FASN_DTYPE_*
    int D;
    int mode;     // MODE_*
};

int launch_fwd_d32(const FwdParams& p, const FwdLaunch& l, hipStream_t s);
int launch_fwd_d64(const FwdParams& p, const FwdLaunch& l, hipStream_t s);
int launch_fwd_d128(const FwdParams& p, const FwdLaunch& l, hipStream_t s);
int launch_fwd_d256(const FwdParams& p, const FwdLaunch& l, hipStream_t s);
int launch_fwd_splitk(const FwdParams& p, const FwdLaunch& l, hipStream_t s);   // p.nsplit > 1, partial buffers set

// The mode a D = 256 forward runs in (launch_fwd_d256 launches it, fasn_fwd_path reports its family): bias + key padding is the dense-mask
// view of the same mask; under dropout so is key padding, and then ONE vector instantiation (MODE_GENERAL, two-wave kernel) serves every
// call whose mask / bias rows move as vectors, no operand at all included - FASN_PATH_VECTOR where D <= 128 says FASN_PATH_PLAIN.
inline int fwd_d256_mode(const FwdParams& p, int mode) {
    if (mode == MODE_BIAS_KEYPAD || (p.drop_thr && mode == MODE_KEYPAD)) mode = p.keypad_fallback;
    return (p.drop_thr && mode != MODE_GENERAL_SLOW) ? MODE_GENERAL : mode;
}

// Launch recorder (fasn_launch_plan, include/fasn.h): while the calling thread has a log installed, every launch site of the library
// (FASN_LAUNCH) writes "kernel<template arguments> grid=G block=T lds=L" into it INSTEAD of launching, and no HIP call is made - the
// host side of fasn_fwd / fasn_bwd then runs to its end exactly as for a real call, so the record is the launch table itself, not a
// description of it (bench.py prints it as roofline.kernels; tests/test_spill_gate.py looks the names up in the code objects).
// `modes` is the same record as data: bit MODE_* for every launch of a kernel that has a mode, set by the launch site from the template
// argument itself (FASN_LAUNCH_MODE). A log without a buffer records that alone - what fasn_fwd_path / fasn_bwd_path ask (fasn_plan.h).
struct LaunchLog {
    char* buf;
    size_t cap, len;
    unsigned modes;
};
extern thread_local LaunchLog* t_launch_log;
void log_launch(const char* pretty, unsigned grid, unsigned block, int smem);
template <auto Kern>
struct KernelTag {};
template <auto Kern>
const char* kernel_pretty_name() { return typeid(KernelTag<Kern>).name(); }   // mangled "fasn::KernelTag<&(void fasn::kernel<arguments>(Params))>": log_launch demangles it (__PRETTY_FUNCTION__ drops a function template's arguments)
#define FASN_LAUNCH(kern, grid, block, smem, stream, ...)                                                                    \
    do {                                                                                                                       \
        if (::fasn::t_launch_log != nullptr) ::fasn::log_launch(::fasn::kernel_pretty_name<(kern)>(), (grid).x, (block).x, (int)(smem)); \
        else hipLaunchKernelGGL(kern, grid, block, smem, stream, __VA_ARGS__);                                                \
    } while (0)
#define FASN_LAUNCH_MODE(mode, ...)   /* a kernel whose template arguments include MODE_* `mode` */                          \
    do {                                                                                                                       \
        if (::fasn::t_launch_log != nullptr) ::fasn::t_launch_log->modes |= 1u << (mode);                                      \
        FASN_LAUNCH(__VA_ARGS__);                                                                                              \
    } while (0)

// A kernel that needs more than 48 KiB of dynamic LDS must be told so once per (kernel, device). The attribute is per
// device, so the "done" state is one bit per device ordinal of THIS kernel (the template parameter is the kernel itself:
// one static per instantiation); after the first launch on a device the launch path only reads an atomic.
template <auto Kern>
inline void ensure_smem(int smem) {
    if (smem <= 48 * 1024 || t_launch_log != nullptr) return;
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    const uint64_t bit = 1ull << (dev & 63);
    if (dev < 64 && (done.load(std::memory_order_relaxed) & bit)) return;
    (void)hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (dev < 64) done.fetch_or(bit, std::memory_order_relaxed);
}
inline int launch_rc() { return (t_launch_log != nullptr || hipGetLastError() == hipSuccess) ? 0 : -6; }

constexpr bool mode_is_vec(int MODE) { return mode_is_vector(MODE); }
constexpr int fwd_smem(int D, int RING, int MODE, int NW, int QB, int BF32 = 0) {
    // K/V buffers + per-wave bias / mask images (fp32 bias: 8 KiB instead of 4; the mask area only in the modes with a dense-mask operand) + key-padding visibility words
    return (RING == 2 ? 6 : 4) * KT * D * 2 + (mode_is_vec(MODE) ? NW * QB * ((BF32 ? 8192 : 4096) + (mode_has_vmask(MODE) ? 2048 : 0)) : 0) +
           (mode_has_keypad(MODE) ? kFwdKpMaxTiles * 8 : 0);
}

// one instantiation of the forward kernel: NW waves x QB 32-row blocks per wave, staging scheme RING, accumulator seeding SEED
// Paired causal blocks (block r and block nblk-1-r in one workgroup: equal workgroups, see the kernels). Rounds 2 - 5: from two rounds of single blocks.
// Round 6 (profiles/r06_causal_pairing_threshold_ab.log, (4,16,S,D) causal): the in-order dispatcher hands unequal workgroups out head by head, so the heavy
// blocks of the last heads start late, and even a launch that is resident at once puts two heavy blocks on one CU - (4,16,2048,64) forward 0.064 -> 0.054 ms
// paired at 1.33 rounds, (4,16,2048,32) -13 % at exactly one round, (4,16,2048,128) 0.117 -> 0.090 (its 96 KiB of LDS make 512 blocks TWO rounds: `slots`
// now counts LDS). But pairs that do not fill the CUs evenly cost the forward more than they save below two rounds ((4,16,1536,64): 384 pairs on 256 CUs,
// +7 % plain, +21 % with a bias), while dQ / dK/dV gained in every case measured from 1.25 rounds on. So: two rounds, or - forward - one round and a multiple
// of 256 pairs, or - backward - 1.25 rounds.
constexpr long wg_slots(int occ_waves_per_simd, int nw, int smem) {   // workgroups the chip holds at once
    const long by_regs = occ_waves_per_simd * 4 / nw < 1 ? 1 : occ_waves_per_simd * 4 / nw;
    const long by_lds = smem > 0 ? 163840 / smem : by_regs;
    return 256L * (by_regs < by_lds ? by_regs : (by_lds < 1 ? 1 : by_lds));
}
inline bool pair_wanted(long blocks, long slots, bool backward = false) {
    if (blocks >= 2 * slots) return true;
    if (backward) return 4 * blocks >= 5 * slots;
    return blocks >= slots && blocks % 512 == 0;
}
template <typename Tag, int D, int QB, int MODE, int OCC, int NW = 4, int RING = 0, int SEED = 0, int DROP = 0, int VH = 1, int FOLD = 0, int BF32 = 0>
int launch_fwd_one(FwdParams p, hipStream_t s) {
    constexpr int BM = NW * QB * 32;
    constexpr int smem = fwd_smem(D, RING, MODE, NW, QB, BF32);
    p.nqblk = (p.Sq + BM - 1) / BM;
    constexpr auto kern = &fasn_fwd_kernel<Tag, D, QB, MODE, OCC, NW, 0, DROP, RING, 0, SEED, VH, FOLD, BF32>;
    ensure_smem<kern>(smem);
    // causal: pair block r with block nqblk-1-r in one workgroup (equal workgroups, see the kernel) when the single blocks fill the
    // chip's workgroup slots at least kPairRounds times; smaller launches keep single blocks, heaviest first
    int blocks = p.nqblk;
    p.pair = 0;
    // (round 6: also the vector mask / bias modes when the call is causal - ALiBi in a decoder: without pairs a launch of unequal workgroups handed out
    // head by head ends on heavy blocks that started late; (4,16,2048,64) causal + bias ran at 0.84 of the non-causal time instead of ~0.55)
    // (round 6: the causal dropout forward pairs its blocks too; the vector modes with dropout do not)
    constexpr bool VEC_PAIR = mode_is_vector(MODE) && !mode_has_keypad(MODE);
    if ((MODE == MODE_CAUSAL || (VEC_PAIR && p.causal)) && VH == 1 && (!DROP || MODE == MODE_CAUSAL) && p.nqblk > 1 && pair_wanted((long)p.nqblk * p.B * p.H, wg_slots(OCC, NW, smem))) {
        p.pair = 1;
        blocks = (p.nqblk + 1) / 2;
    }
    if constexpr (fwd_xq_kernel(D, MODE, 0, VH, DROP)) {
        if (p.xq != nullptr && ((p.B * p.H) & 7) == 0) {   // dynamic deal of the items across XCDs (fasn_fwd_ws; the counters are the caller's workspace, zeroed here)
            // counters that could not be zeroed (bad workspace pointer, a capture that refuses the node) would make workgroups skip or repeat
            // items: such a launch takes the static deal below instead
            const bool zeroed = t_launch_log != nullptr || hipMemsetAsync(p.xq, 0, 8 * sizeof(int), s) == hipSuccess;
            if (zeroed) {
                FASN_LAUNCH_MODE(MODE, kern, dim3((unsigned)(blocks * p.B * p.H + 8 * kXqSurplus)), dim3(NW * 64), smem, s, p);
                return launch_rc();
            }
            (void)hipGetLastError();
        }
    }
    p.xq = nullptr;   // (every other instantiation: static deal)
    FASN_LAUNCH_MODE(MODE, kern, dim3((unsigned)(blocks * p.B * p.H * VH)), dim3(NW * 64), smem, s, p);
    return launch_rc();
}

// plain / causal / key-padding launch of one (workgroup size, staging scheme) tuning point
template <typename Tag, int D, int QB, int OCC, int NW, int RING, int SEED = 0>
int launch_fwd_cfg(const FwdParams& p, int mode, hipStream_t s) {
    if (mode == MODE_PLAIN) return launch_fwd_one<Tag, D, QB, MODE_PLAIN, OCC, NW, RING, SEED>(p, s);
    if (mode == MODE_KEYPAD) return launch_fwd_one<Tag, D, QB, MODE_KEYPAD, OCC, NW, RING, SEED>(p, s);
    return launch_fwd_one<Tag, D, QB, MODE_CAUSAL, OCC, NW, RING, SEED>(p, s);
}

// dropout instantiations: plain, causal, key-padding, the vector mask / bias kernel (MODE_GENERAL serves all three mask / bias
// combinations: an absent operand is a zero-range descriptor / an all-ones word) and the element-load general kernel.
// Round 6 (dropout stream definition 2, fasn_common.h): the keep bits are applied to the PACKED weights, behind the row sums - the dropout
// kernels run at the plain kernels' tuning points, seeded accumulators and packed row sums (SEED = 2) included: 64 rows per wave at D = 64 no
// longer spill (244 registers; the round-5 hash needed 37 - 67 more), three waves per SIMD fit in 144.
// QB / OCC: the tuning point of the plain kernel for this launch (fasn_fwd_d*.hip decides by the size of the grid).
template <typename Tag, int D, int QB, int OCC>
int launch_fwd_drop(const FwdParams& p, int mode, hipStream_t s) {
    if (mode == MODE_BIAS_KEYPAD) {
        // vector bias + key-padding mask (ALiBi on a padded batch) with dropout: the visibility-word kernel at D = 128 (round 4), elsewhere
        // the dense-mask general mode of the same mask
        if constexpr (D == 128) return launch_fwd_one<Tag, D, 1, MODE_BIAS_KEYPAD, 2, 8, 2, 2, 1>(p, s);
        // head dims 32 / 64 (round 6): the same mode at the vector dropout kernels' tuning point (154 / 174 registers) instead of the
        // dense-mask general mode of the same mask (a mask image per tile next to the bias image)
        else return launch_fwd_one<Tag, D, (D == 32 ? 2 : 1), MODE_BIAS_KEYPAD, 2, 4, (D == 32 ? 2 : 0), 2, 1>(p, s);
    }
    if (mode == MODE_PLAIN) {
        if constexpr (D == 128) return launch_fwd_one<Tag, D, 1, MODE_PLAIN, 2, 8, 2, 2, 1>(p, s);   // 8 waves share a K/V tile, two per SIMD
        else return launch_fwd_one<Tag, D, QB, MODE_PLAIN, OCC, 4, 2, 2, 1>(p, s);
    }
    if (mode == MODE_CAUSAL) {
        if constexpr (D == 128) return launch_fwd_one<Tag, D, 1, MODE_CAUSAL, 2, 8, 2, 2, 1>(p, s);
        else return launch_fwd_one<Tag, D, QB, MODE_CAUSAL, OCC, 4, 2, 2, 1>(p, s);
    }
    if (mode == MODE_KEYPAD) {
        if constexpr (D == 128) return launch_fwd_one<Tag, D, 1, MODE_KEYPAD, 2, 8, 2, 2, 1>(p, s);
        else return launch_fwd_one<Tag, D, QB, MODE_KEYPAD, OCC, 4, 2, 2, 1>(p, s);
    }
    if (mode == MODE_GENERAL || mode == MODE_GENERAL_B || mode == MODE_GENERAL_M) {
        if constexpr (D == 128) return launch_fwd_one<Tag, D, 1, MODE_GENERAL, 2, 8, 2, 2, 1>(p, s);
        else return launch_fwd_one<Tag, D, (D == 32 ? 2 : 1), MODE_GENERAL, 2, 4, (D == 32 ? 2 : 0), 2, 1>(p, s);   // (the p = 0 vector kernels' small-grid tuning points)
    }
    return launch_fwd_one<Tag, D, (D == 32 ? 2 : 1), MODE_GENERAL_SLOW, 1, 4, 0, 0, 1>(p, s);
}

}  // namespace fasn
