// fasn_plan.h — a call's launches as a record: the call itself runs under the launch recorder of fasn_launch.h, so nothing is launched,
// no HIP call is made and the record is the launch table, not a description of it. record_plan is the one place that installs a log;
// every *_plan entry point and the path queries of fasn_api.hip go through it.
#pragma once
#include "fasn.h"
#include "fasn_launch.h"

namespace fasn {

// What a recorded call is handed as its workspace, with a size of ~size_t(0): nothing is launched, so any aligned address will do.
inline void* plan_workspace() { return reinterpret_cast<void*>(uintptr_t(256)); }

// Runs `call` with `log` installed and the outer log restored behind it. Returns the number of bytes written (without the NUL; 0 for a
// log without a buffer, which records LaunchLog::modes alone), the FASN_E* code `call` returns, or FASN_EINVAL when the text did not fit.
template <typename Call>
int record_plan(LaunchLog& log, Call call) {
    LaunchLog* const outer = t_launch_log;
    t_launch_log = &log;
    const int rc = call();
    t_launch_log = outer;
    if (rc) return rc;
    return log.len > log.cap ? FASN_EINVAL : (int)log.len;
}
template <typename Call>
int record_plan(char* buf, size_t cap, Call call) {
    if (buf == nullptr || cap == 0) return FASN_EINVAL;
    buf[0] = 0;
    LaunchLog log{buf, cap, 0, 0};
    return record_plan(log, call);
}

}  // namespace fasn
