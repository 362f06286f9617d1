// D = 64 forward instantiations: the shipped tuning points (the rejected ones and their measurements: LABNOTES.md).
#include "fasn_launch.h"
namespace fasn {
template <typename Tag>
static int launch_gen(const FwdParams& p, const FwdLaunch& l, hipStream_t s) {
    if (p.bias_f32) {   // fp32 bias next to 16-bit q / k / v (fasn_api.hip: f32_bias_vector): the fp32 image instantiations
        switch (l.mode) {
            case MODE_GENERAL: return launch_fwd_one<Tag, 64, 1, MODE_GENERAL, 2, 4, 0, 2, 0, 1, 0, 1>(p, s);
            case MODE_GENERAL_B: return launch_fwd_one<Tag, 64, 1, MODE_GENERAL_B, 2, 4, 0, 2, 0, 1, 0, 1>(p, s);
            case MODE_BIAS_KEYPAD: return launch_fwd_one<Tag, 64, 1, MODE_BIAS_KEYPAD, 2, 4, 0, 2, 0, 1, 0, 1>(p, s);
            default: break;
        }
    }
    // Round 6: the vector mask / bias modes of a large grid run EIGHT waves x 64 rows per workgroup, direct-to-LDS, one workgroup per CU (two
    // waves per SIMD, every K / V fragment read from LDS feeds two row blocks; 213 - 256 registers, no spill) - same box, (4,16,4096,64) ALiBi +
    // key padding forward: 0.443 -> 0.388 ms (-12 %; four waves x 32 rows direct-to-LDS: 0.412 / 0.425 with two / three waves per SIMD;
    // profiles/r06_d64_bias_forward_tuning_points_ab.log). Small grids keep four waves x 32 rows, register-staged.
    const long blocks512 = (long)((p.Sq + 511) / 512) * p.B * p.H;
    // (a full round of one workgroup per CU; the bias + key-padding mode pairs its batch elements by length - half as many workgroups - and needs
    // two: at (8,16,1024,64), 256 blocks, the paired 8-wave launch left half of the CUs idle, 0.089 against 0.064 ms)
    // (causal next to a mask / bias: the workgroups of a launch are unequal - a one-round launch of 512-row blocks takes as long as the same call without
    // the causal flag, the heaviest block sets the time - so the 8-wave kernel needs twice as many blocks: (4,16,2048,64) causal + bias 0.090 -> 0.068 ms, at (4,16,4096,64), two rounds, the 8-wave kernel is 2 % ahead again; profiles/r06_causal_next_to_a_bias_forward_rule_ab.log)
    if (blocks512 >= (l.mode == MODE_BIAS_KEYPAD ? 512 : 256) * (p.causal ? 2 : 1) && p.Sq >= 512) {
        switch (l.mode) {
            case MODE_GENERAL: return launch_fwd_one<Tag, 64, 2, MODE_GENERAL, 2, 8, 2, 2>(p, s);
            case MODE_GENERAL_B: return launch_fwd_one<Tag, 64, 2, MODE_GENERAL_B, 2, 8, 2, 2>(p, s);
            case MODE_GENERAL_M: return launch_fwd_one<Tag, 64, 2, MODE_GENERAL_M, 2, 8, 2, 2>(p, s);
            case MODE_BIAS_KEYPAD: return launch_fwd_one<Tag, 64, 2, MODE_BIAS_KEYPAD, 2, 8, 2, 2>(p, s);
            default: break;
        }
    }
    switch (l.mode) {
        case MODE_GENERAL: return launch_fwd_one<Tag, 64, 1, MODE_GENERAL, 2, 4, 0, 2>(p, s);
        case MODE_GENERAL_B: return launch_fwd_one<Tag, 64, 1, MODE_GENERAL_B, 2, 4, 0, 2>(p, s);
        case MODE_GENERAL_M: return launch_fwd_one<Tag, 64, 1, MODE_GENERAL_M, 2, 4, 0, 2>(p, s);
        case MODE_BIAS_KEYPAD: return launch_fwd_one<Tag, 64, 1, MODE_BIAS_KEYPAD, 2, 4, 0, 2>(p, s);
        default: return launch_fwd_one<Tag, 64, 1, MODE_GENERAL_SLOW, 1>(p, s);
    }
}
template <typename Tag>
static int go(const FwdParams& p, const FwdLaunch& l, hipStream_t s) {
    if (p.drop_thr) {   // dropout: the plain kernels' tuning points (round 6: the keep bits are applied to the packed weights - no spills at 64 rows per wave)
        const long bq2 = (long)((p.Sq + 255) / 256) * p.B * p.H;
        const bool big = (l.mode == MODE_PLAIN || (l.mode == MODE_KEYPAD && !p.causal)) && bq2 >= 512 && p.Sq >= 256;
        return big ? launch_fwd_drop<Tag, 64, 2, 2>(p, l.mode, s) : launch_fwd_drop<Tag, 64, 1, 3>(p, l.mode, s);
    }
    if (l.mode >= MODE_GENERAL && l.mode != MODE_KEYPAD) return launch_gen<Tag>(p, l, s);   // key-padding masks ride the plain tuning points
    // auto (what ABI callers get), measured on MI355X at (8,16,4096,64), 200 launches each. All plain / causal / key-padding
    // kernels run with seeded accumulators (Q pre-scaled, S starts at -m, row sums by v_dot2c on the packed weights):
    //   plain : QB=2 / 2 waves per SIMD / direct-to-LDS  1058 TFLOP/s  (unseeded two-set ring 1005; QB=1 / 3 waves 983); 1130 with the loop unrolled by its buffers
    //   causal: QB=1 / 3 waves per SIMD / direct-to-LDS   772 TFLOP/s  (unseeded 734; QB=2 719: coarser diagonal, worse tail)
    const long blocks_qb2 = (long)((p.Sq + 255) / 256) * p.B * p.H;
    const bool big_plain = (l.mode == MODE_PLAIN || (l.mode == MODE_KEYPAD && !p.causal)) && blocks_qb2 >= 512 && p.Sq >= 256;   // 512 = one full round of two workgroups per CU
    if (big_plain)   // (plain or key padding: the 64-rows-per-wave causal kernel of large launches is the folded one below)
        return l.mode == MODE_PLAIN ? launch_fwd_one<Tag, 64, 2, MODE_PLAIN, 2, 4, 2, 2>(p, s) : launch_fwd_one<Tag, 64, 2, MODE_KEYPAD, 2, 4, 2, 2>(p, s);
    // causal launches of at least two rounds at the plain kernel's tuning point with the folded two-phase walk (round 5; same box, final builds,
    // three alternations - profiles/r05_causal_forward_folded_two_phase_ab.log: C5 2.377 -> 2.362 ms, (16,16,4096,64) 0.6325 -> 0.6246, (4,32,8192,64)
    // 1.115 -> 1.085, (2,16,16384,64) 1.072 -> 1.017, C3 (fp16, two rounds) 0.3446 -> 0.3409; on other boxes C5 +2.1 %, C3 +0.3 .. +1.0 %)
    if (l.mode == MODE_CAUSAL && p.Sq >= 256 && blocks_qb2 >= 2048) return launch_fwd_one<Tag, 64, 2, MODE_CAUSAL, 2, 4, 2, 2, 0, 1, 1>(p, s);
    return launch_fwd_cfg<Tag, 64, 1, 3, 4, 2, 2>(p, l.mode, s);
}
int launch_fwd_d64(const FwdParams& p, const FwdLaunch& l, hipStream_t s) {
    return l.dtype == 1 ? go<bf16_tag>(p, l, s) : go<f16_tag>(p, l, s);
}
}  // namespace fasn
