// dril_eval_account.h — the per-env episode accounting of a device-resident evaluate_agent (evaluation.jl:95-121) on a PPO handle: what env e's thread does with the
// reward and the done flag of its step.  The record it appends and the host's reduction of the copied list are dril_sac_eval.h's (SacEvalEvent, sac_eval_event_capacity,
// sac_eval_reduce); the list's ordering argument is written there.  No HIP dependency: dril_eval.hip (eval_account_kernel, over the E-sized per-step arrays) and
// dril_kernels.hip (evaluate_kernel, the sums in registers) include it, and tests/test_eval_device.py drives the same lines with g++ against a restatement of the
// reference's loop.
#pragma once
#include <stdint.h>

#include "dril_sac_eval.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRIL_EVAL_HD __host__ __device__ __forceinline__
#else
#define DRIL_EVAL_HD inline
#endif

namespace dril {
// the list of one evaluation: ONE counter for all envs (events past `cap` = eval_event_capacity(n, E, K) only bump it), and the E-sized running sums that travel
// between launches
struct EvalAcct { int32_t E; float* cur_ret; int32_t* cur_len; unsigned int* counter; SacEvalEvent* events; unsigned int cap; };

// Slots of the event list when one launch runs `launch_steps` env steps.  Launches of one stream are ordered, so with one launch per env step the first n episodes in
// (step, env) order sit in the first n + E slots (dril_sac_eval.h).  INSIDE a launch of evaluate_kernel the waves run their K steps at their own pace — an event of
// step s + 3 may take its slot before one of step s — so the order argument holds between launches only: fewer than n events precede the launch that completes the
// list, and that launch appends at most E K.  With n + E K slots nothing the reduction needs is ever dropped (the host stops after that launch).
inline int64_t eval_event_capacity(int64_t n_eval, int64_t n_envs, int64_t launch_steps) {
    return launch_steps <= 1 ? sac_eval_event_capacity(n_eval, n_envs) : n_eval + n_envs * launch_steps;
}

// the next free slot.  On the device every env's thread takes it through the one atomic; a host driver is one thread
DRIL_EVAL_HD unsigned int eval_take_slot(unsigned int* counter) {
#if defined(__HIP_DEVICE_COMPILE__) || defined(__CUDA_ARCH__)
    return atomicAdd(counter, 1u);
#else
    return (*counter)++;
#endif
}
// env e after env step `step` (1-based), its running sums in ret / len: current_rewards[e] += reward in float32 and in step order, current_lengths[e] += 1 (:95-96);
// where the episode ended, one event and the two sums restart (:100-121)
DRIL_EVAL_HD void eval_account(const EvalAcct& a, int32_t step, int32_t e, float rew, bool done, float& ret, int32_t& len) {
    ret += rew; len += 1;
    if (done) {
        const unsigned int i = eval_take_slot(a.counter);
        if (i < a.cap) a.events[i] = SacEvalEvent{step, e, ret, len};
        ret = 0.f; len = 0;
    }
}
// the same with the sums in the E-sized arrays (the step-granular path: one thread per env after the env's step launch)
DRIL_EVAL_HD void eval_account_env(const EvalAcct& a, int32_t step, int32_t e, float rew, bool done) {
    float r = a.cur_ret[e]; int32_t l = a.cur_len[e];
    eval_account(a, step, e, rew, done, r, l);
    a.cur_ret[e] = r; a.cur_len[e] = l;
}
}  // namespace dril
