// fasn_varlen_rope.h - rotary position embedding on the packed variable-length training call (include/fasn.h: fasn_varlen_rope,
// fasn_varlen_rope_plan): the host interface between fasn_attnvarlen.hip, which owns the packed call's argument checks,
// and fasn_varlen_rope.hip, which owns the rope operand's checks, the kernel and its one launch.
#pragma once
#include <hip/hip_runtime.h>
#include "fasn.h"

namespace fasn {

// a packed operand [1, heads, rows, D] of 16-bit elements under the packed call's view rules (fasn_attnvarlen.hip)
int check_packed(const fasn_view4& v, int rows, int D);

// Behind every rule of build_varlen that applies (the caller's): the rope operand's rules with the codes of the cache's rotary calls,
// q_out / k_out under check_packed, `inverse`; then the launch. `kvg`: query heads per K/V head. No HIP call before the last check.
int varlen_rope(const fasn_fwd_args* a, const fasn_varlen* vl, int kvg, const fasn_kv_rope* rope, const fasn_view4* q_out, const fasn_view4* k_out,
                int32_t inverse, hipStream_t s);

}  // namespace fasn
