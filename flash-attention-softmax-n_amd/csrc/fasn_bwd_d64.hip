// D = 64 backward instantiations: <QB (dQ: 32-row blocks/wave), KB (dK/dV: 32-key blocks/wave), occupancies>
// (the two-wave kernels of D = 128 measured slower here: (8,16,4096,64) backward 2.18 ms against 1.81 ms - at D = 64 the one-wave
// kernels already run two waves per SIMD and the exponentials, not registers, are the limit)
#include "fasn_bwd_launch.h"
namespace fasn {
int launch_bwd_d64(const BwdParams& p, const FwdLaunch& l, hipStream_t s) {
    // plain / causal without grouped K/V (with or without dropout): the software-pipelined kernels of fasn_bwd_pipe.h. No delta launch: the dQ
    // kernel, which runs first, computes delta = rowsum(O o dO) of its rows in its prologue (bit-identical to fasn_bwd_delta_kernel) and stores
    // it for the dK/dV kernel (C2 backward -7 %, the other D = 64 configs -1.5 .. -2.5 %; LABNOTES.md)
    if ((l.mode == MODE_PLAIN || l.mode == MODE_CAUSAL) && p.f.kvg == 1) {
        const int rc = launch_bwd_dq_pipe_d64(p, l, s);
        return rc ? rc : launch_bwd_dkdv_pipe_d64(p, l, s);
    }
    return l.dtype == 1 ? launch_bwd_mode<bf16_tag, 64, 1, 1, 2, 2>(p, l.mode, s) : launch_bwd_mode<f16_tag, 64, 1, 1, 2, 2>(p, l.mode, s);
}
}  // namespace fasn
