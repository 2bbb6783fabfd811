// dril_ext_record.h — what env e's thread of ext_norm_record_kernel (dril_ext_norm.h) does with the scalars of its env step on a DRIL_ENV_EXTERNAL handle under
// dril_ext_normalize_enable / dril_ext_monitor_enable: the flags byte and the sticky-error rule of dril_ext_record_device, the `returns` recursion and reset of
// NormalizeWrapperEnv.act! (normalizeWrapperEnv.jl:149-153, :167-171) and MonitorWrapperEnv's running sums (monitorWrapperEnv.jl:46-60).  No HIP dependency:
// the kernel includes it, and tests/test_ext_wrap.py drives the same lines with g++ against tests/sac_normalize_ref.py and a restatement of the monitor.
// (The recursion itself runs in norm_moments_kernel, dril_norm_wrap.h, which sums `returns` while it advances them; xr_returns_step is that one expression.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRIL_XR_HD __host__ __device__ __forceinline__
#else
#define DRIL_XR_HD inline
#endif

namespace dril {
// the DRIL_BUF_FLAGS encoding
DRIL_XR_HD uint8_t xr_flags(bool terminated, bool truncated) { return (uint8_t)((terminated ? 1 : 0) | (truncated ? 2 : 0)); }
// a truncated env whose caller passed no terminal_obs: the error word is set (a plain store; dril_ext_finish_device reads it after its drain)
DRIL_XR_HD bool xr_sticky(bool truncated, bool has_terminal_obs) { return truncated && !has_terminal_obs; }
// update_reward_stats! (:168), one env
DRIL_XR_HD float xr_returns_step(float returns, float gamma, float reward) { return returns * gamma + reward; }
// act! :149-153: returns of finished envs to zero
DRIL_XR_HD float xr_returns_reset(float returns, bool done) { return done ? 0.f : returns; }
// MonitorWrapperEnv.act! (:46-60), one env: the sums take the RAW reward in float32 and step order; where the episode ended, its return / length go to the
// rollout's row (*ep_ret / *ep_len: collected into the window in (step, env) order by launch_monitor_collect) and the sums restart
DRIL_XR_HD void xr_monitor(float reward, bool done, float& cur_ret, int32_t& cur_len, float* ep_ret, int32_t* ep_len) {
    cur_ret += reward; cur_len += 1;
    if (done) { *ep_ret = cur_ret; *ep_len = cur_len; cur_ret = 0.f; cur_len = 0; }
}
}  // namespace dril
