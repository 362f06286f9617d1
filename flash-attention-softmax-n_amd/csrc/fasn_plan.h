// fasn_plan.h — a call's launches as text, for the entry points outside the attention front end (fasn_softmax_n_plan, fasn_moments_plan):
// the call itself runs under the launch recorder of fasn_launch.h, so nothing is launched, no HIP call is made and the text is the launch
// table, not a description of it.
#pragma once
#include "fasn.h"
#include "fasn_launch.h"

namespace fasn {

// Returns the number of bytes written (without the NUL), the FASN_E* code `call` returns, or FASN_EINVAL when `cap` is too small.
template <typename Call>
int record_plan(char* buf, size_t cap, Call call) {
    if (buf == nullptr || cap == 0) return FASN_EINVAL;
    LaunchLog log{buf, cap, 0};
    buf[0] = 0;
    LaunchLog* const outer = t_launch_log;
    t_launch_log = &log;
    const int rc = call();
    t_launch_log = outer;
    if (rc) return rc;
    return log.len > cap ? FASN_EINVAL : (int)log.len;
}

}  // namespace fasn
