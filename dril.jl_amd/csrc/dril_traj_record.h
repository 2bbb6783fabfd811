// dril_traj_record.h — the per-env recording of a device-resident collect_trajectory (trajectory_utils.jl:3-49), on a PPO and on a SAC handle: what the lanes of env m
// do with the action, the reward, the done flags and the observation of its step — the active test, what is written where, finalisation, and the precedence of the
// episode's end over the max_steps cut — and the copy-out of a finished recording.  No HIP dependency (traj_copy_out apart: HIP compiles only), in the manner of
// dril_eval_account.h.  Who runs it: dril_eval.hip (traj_record_kernel through traj_record_lane, traj_record_rows_kernel through traj_record_lane_rows), dril_kernels.hip
// (evaluate_modes_kernel's recording mode through traj_record_env) and the SAC handle (sac_traj_env_kernel of dril_sac_collect.hip through traj_record_env, sac_traj_record_kernel of dril_sac_eval.hip through traj_record_lane,
// both with null clamp pointers); tests/test_traj_device.py, test_sac_traj.py and test_eval_persistent_modes.py drive the same lines with g++.  The setup around the rule: dril_traj_run.h.
//
// The recording is step-major on the device, [t][m][.], so one step's writes are contiguous M-sized rows; traj_reorder puts it into the caller's per-trajectory layout.
// Every index is 64-bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/device/dril_scaling.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#define DRIL_TRAJ_HD __host__ __device__ __forceinline__
#else
#define DRIL_TRAJ_HD inline
#endif

namespace dril {
constexpr int32_t kTrajOpen = 0x7f7f7f7f;                       // length[m] of a trajectory still recording (larger than any capacity)
enum : uint8_t { kTrajTerminated = 1, kTrajTruncated = 2, kTrajCut = 4 };   // end_flags bits; kTrajCut: the reference's "Max steps reached" (:38-41)

// Tcap: the rows a trajectory can need — the env's time limit ends every episode, max_steps (> 0) may end it sooner
DRIL_TRAJ_HD int32_t traj_capacity(int32_t max_steps, int32_t episode_len) { return (max_steps > 0 && max_steps < episode_len) ? max_steps : episode_len; }
// bytes of the device recording of M trajectories of capacity Tcap (observations | actions | rewards | lengths | end flags)
DRIL_TRAJ_HD int64_t traj_bytes(int64_t M, int64_t Tcap, int64_t D, int64_t W) { return 4 * M * ((Tcap + 1) * D + Tcap * W + Tcap) + 5 * M; }

// the recording of one call.  W: 4-byte words of one action (1 for a Discrete space, A for a Box).  length[m] is kTrajOpen until trajectory m is finalised: the ONE
// word the active test reads, so the lanes of an env need no ordering among themselves (its lane 0 writes t in the launch of step t, and both values mean "record t")
struct TrajRec {
    int32_t M, D, W, Tcap;
    float* obs; uint32_t* act; float* rew;                      // [(Tcap + 1)][M][D], [Tcap][M][W], [Tcap][M]
    int32_t* length; uint8_t* end_flags; unsigned int* finished;   // [M], [M], ONE counter
};
// what happens to the values on their way into the recording.  Observations (obs_low != null: ScalingWrapperEnv) go through unscale_from_unit — rows below the final
// one always (:19-21), the final row only with final_original (:44 does not unscale).  Box actions: ClampAdapter on the agent-facing Box where clamp_low[a] <
// clamp_high[a] (to_env), then unscale! under the wrapper (act_low != null, :30-32)
struct TrajMaps {
    const float *obs_low, *obs_high, *clamp_low, *clamp_high, *act_low, *act_high;
    int32_t discrete, final_original;
};
// one env step's arrays, E-sized, env-major (the handle's per-step arrays; obs is the shadow envs' post-step, pre-reset observation)
struct TrajStep { const void* act; const float* rew; const uint8_t* term; const uint8_t* trunc; const float* obs; };

DRIL_TRAJ_HD bool traj_active(const TrajRec& r, int32_t t, int32_t m) { return t == 0 || r.length[m] >= t; }
DRIL_TRAJ_HD void traj_count_finished(unsigned int* counter) {
#if defined(__HIP_DEVICE_COMPILE__) || defined(__CUDA_ARCH__)
    atomicAdd(counter, 1u);
#else
    (*counter)++;
#endif
}
DRIL_TRAJ_HD uint32_t traj_f2u(float f) { union { float f; uint32_t u; } v; v.f = f; return v.u; }
DRIL_TRAJ_HD float traj_u2f(uint32_t u) { union { float f; uint32_t u; } v; v.u = u; return v.f; }
// the env action of word j (:28-34): predict_actions' to_env, then unscale! under ScalingWrapperEnv
DRIL_TRAJ_HD uint32_t traj_env_action(const TrajMaps& x, int32_t j, uint32_t raw) {
    if (x.discrete) return raw;
    float v = traj_u2f(raw);
    if (x.clamp_low && x.clamp_low[j] < x.clamp_high[j]) v = fminf(fmaxf(v, x.clamp_low[j]), x.clamp_high[j]);
    if (x.act_low) v = unscale_from_unit(v, x.act_low[j], x.act_high[j]);
    return traj_f2u(v);
}
// Lane j of env m after env step t (1-based; t = 0: after the initial observe, s.obs the raw observation, nothing else read).  j < D writes observation row t,
// j < W action row t - 1, lane 0 the reward of row t - 1 and, where the trajectory ends here, its length, its flags and the finished-counter.  The episode's end
// takes precedence over the cut when both fall on step Tcap.  Steps after the trajectory ended (a second episode of a fast env, steps enqueued past the last finish)
// write nothing.
// `length`: the trajectory's open / closed state as this lane holds it — kTrajOpen while it records.  obs_m / act_m: env m's D observations / W action words of this step.
DRIL_TRAJ_HD void traj_record_lane_step(const TrajRec& r, const TrajMaps& x, int32_t t, int32_t m, int32_t j, const float* obs_m, const uint32_t* act_m, float rew,
                                        bool term, bool trunc, int32_t& length) {
    if (t > r.Tcap || length != kTrajOpen) return;
    const bool done = term || trunc, cut = !done && t >= r.Tcap, last = done || cut;
    const int64_t row = (int64_t)t * r.M + m, prev = row - r.M;
    if (j < r.D) {
        const float o = obs_m[j];
        r.obs[row * r.D + j] = (x.obs_low && (!last || x.final_original)) ? unscale_from_unit(o, x.obs_low[j], x.obs_high[j]) : o;
    }
    if (j < r.W) r.act[prev * r.W + j] = traj_env_action(x, j, act_m[j]);
    if (last) length = t;
    if (j == 0) {
        r.rew[prev] = rew;
        if (last) {
            r.length[m] = t;
            r.end_flags[m] = (uint8_t)((term ? kTrajTerminated : 0) | (trunc ? kTrajTruncated : 0) | (cut ? kTrajCut : 0));
            traj_count_finished(r.finished);
        }
    }
}
// row 0: the original observation after the initial observe, and the trajectory opened
DRIL_TRAJ_HD void traj_record_lane_open(const TrajRec& r, const TrajMaps& x, int32_t m, int32_t j, const float* obs_m) {
    if (j < r.D) r.obs[(int64_t)m * r.D + j] = x.obs_low ? unscale_from_unit(obs_m[j], x.obs_low[j], x.obs_high[j]) : obs_m[j];
    if (j == 0) { r.length[m] = kTrajOpen; r.end_flags[m] = 0; }
}
// one launch per env step: the open / closed state is r.length[m], read once per lane
DRIL_TRAJ_HD void traj_record_lane(const TrajRec& r, const TrajMaps& x, const TrajStep& s, int32_t t, int32_t m, int32_t j) {
    if (t == 0) { traj_record_lane_open(r, x, m, j, s.obs + (int64_t)m * r.D); return; }
    if (t > r.Tcap || !traj_active(r, t, m)) return;
    int32_t length = kTrajOpen;
    traj_record_lane_step(r, x, t, m, j, s.obs + (int64_t)m * r.D, (const uint32_t*)s.act + (int64_t)m * r.W, s.rew[m], s.term[m] != 0, s.trunc[m] != 0, length);
}
// K env steps in ONE launch (the evaluation kernel of a device env plug-in leaves K rows: device/dril_env_evaluate.h): every lane of env m walks the rows in step order
// with the open / closed state in a register of its own, loaded from r.length[m] as the launch before left it — inside the launch the lanes of an env have no order
// among themselves, so none of them depends on what lane 0 writes meanwhile.  rew / flags: rows of n_envs entries (flag byte: bit0 terminated, bit1 truncated); obs0: (M x D) the
// observation before the launch's first step (read where t0 == 0: row 0); act (K x M x W) and obs (K x M x D): the raw actions and the post-step, pre-reset observations
struct TrajRows { int32_t K, n_envs; const float* rew; const uint8_t* flags; const float* obs0; const uint32_t* act; const float* obs; };
DRIL_TRAJ_HD void traj_record_lane_rows(const TrajRec& r, const TrajMaps& x, const TrajRows& s, int32_t t0, int32_t m, int32_t j) {
    int32_t length = kTrajOpen;
    if (t0 == 0) traj_record_lane_open(r, x, m, j, s.obs0 + (int64_t)m * r.D);
    else if (r.length[m] <= t0) length = r.length[m];                              // closed before this launch; a value > t0 is "open", or lane 0's finalisation in THIS launch, which this lane reaches by itself
    for (int32_t k = 0; k < s.K; ++k) {
        const int64_t e = (int64_t)k * s.n_envs + m, i = (int64_t)k * r.M + m;
        traj_record_lane_step(r, x, t0 + k + 1, m, j, s.obs + i * r.D, s.act + i * r.W, s.rew[e], (s.flags[e] & 1) != 0, (s.flags[e] & 2) != 0, length);
    }
}
// The same rule with ONE lane holding env m, for a kernel that keeps the env in registers over the steps of a launch (evaluate_modes_kernel, dril_kernels.hip): the lane
// has the env's values themselves — its W action words as the agent returns them, its raw reward and flags, and obs = the D original observations of the env AFTER
// the step and BEFORE its auto-reset (t = 0: after the initial observe) — and the trajectory's open / closed state in `length`, a register across the steps of a
// launch and r.length[m] across launches (the caller loads it where t0 > 0; t = 0 sets both).  Writes, lane for lane, what traj_record_lane writes for the same step
// stream (tests/test_eval_persistent_modes.py).  D and W are template parameters so that obs / act stay registers.
template <int D, int W>
DRIL_TRAJ_HD void traj_record_env(const TrajRec& r, const TrajMaps& x, int32_t t, int32_t m, const uint32_t (&act)[W], float rew, bool term, bool trunc,
                                  const float (&obs)[D], int32_t& length) {
    if (t == 0) {
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
        for (int j = 0; j < D; ++j) r.obs[(int64_t)m * D + j] = x.obs_low ? unscale_from_unit(obs[j], x.obs_low[j], x.obs_high[j]) : obs[j];
        length = kTrajOpen; r.length[m] = kTrajOpen; r.end_flags[m] = 0;
        return;
    }
    if (t > r.Tcap || length != kTrajOpen) return;
    const bool done = term || trunc, cut = !done && t >= r.Tcap, last = done || cut;
    const int64_t row = (int64_t)t * r.M + m, prev = row - r.M;
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int j = 0; j < D; ++j) r.obs[row * D + j] = (x.obs_low && (!last || x.final_original)) ? unscale_from_unit(obs[j], x.obs_low[j], x.obs_high[j]) : obs[j];
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int j = 0; j < W; ++j) r.act[prev * W + j] = traj_env_action(x, j, act[j]);
    r.rew[prev] = rew;
    if (last) {
        length = t; r.length[m] = t;
        r.end_flags[m] = (uint8_t)((term ? kTrajTerminated : 0) | (trunc ? kTrajTruncated : 0) | (cut ? kTrajCut : 0));
        traj_count_finished(r.finished);
    }
}
// the caller's layout from rows 0..longest of the step-major recording (host side): observations (D, Tcap + 1, M), actions (W, Tcap, M), rewards (Tcap, M), all
// column-major; rows past a trajectory's own length are zero
inline void traj_reorder(int64_t M, int64_t D, int64_t W, int64_t Tcap, const int32_t* length, const float* obs_tm, const uint32_t* act_tm, const float* rew_tm,
                         float* obs, uint32_t* act, float* rew) {
    for (int64_t m = 0; m < M; ++m) {
        const int64_t L = length[m];
        for (int64_t t = 0; t <= Tcap; ++t)
            for (int64_t d = 0; d < D; ++d) obs[(m * (Tcap + 1) + t) * D + d] = t <= L ? obs_tm[(t * M + m) * D + d] : 0.f;
        for (int64_t t = 0; t < Tcap; ++t) {
            for (int64_t a = 0; a < W; ++a) act[(m * Tcap + t) * W + a] = t < L ? act_tm[(t * M + m) * W + a] : 0u;
            rew[m * Tcap + t] = t < L ? rew_tm[t * M + m] : 0.f;
        }
    }
}
#if defined(__HIPCC__) || defined(__CUDACC__)
// the copy-out of a finished recording, for the PPO and the SAC handle's verb alike (host side): lengths and end flags first, then rows 0..longest only, reordered into
// the caller's five arrays.  err: the first HIP error; bad >= 0: trajectory `bad` has the impossible length bad_length and nothing further was copied; else
// longest / cuts (trajectories ended by max_steps) for dril_traj_info.  The caller words its own error
struct TrajCopyOut { hipError_t err; int32_t bad, bad_length, longest, cuts; };
inline TrajCopyOut traj_copy_out(hipStream_t stream, const TrajRec& r, float* observations, uint32_t* actions, float* rewards, int32_t* lengths, uint8_t* end_flags) {
    TrajCopyOut c{hipSuccess, -1, 0, 0, 0};
    const size_t M = (size_t)r.M, D = (size_t)r.D, W = (size_t)r.W;
    auto home = [&](void* dst, const void* src, size_t bytes) { if (c.err == hipSuccess) c.err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream); };
    auto drained = [&] { if (c.err == hipSuccess) c.err = hipStreamSynchronize(stream); return c.err == hipSuccess; };
    home(lengths, r.length, M * 4); home(end_flags, r.end_flags, M);
    if (!drained()) return c;
    for (int32_t m = 0; m < r.M; ++m) {
        if (lengths[m] < 1 || lengths[m] > r.Tcap) { c.bad = m; c.bad_length = lengths[m]; return c; }
        c.longest = std::max(c.longest, lengths[m]); c.cuts += (end_flags[m] & kTrajCut) ? 1 : 0;
    }
    std::vector<float> obs_tm((size_t)(c.longest + 1) * M * D), rew_tm((size_t)c.longest * M); std::vector<uint32_t> act_tm((size_t)c.longest * M * W);
    home(obs_tm.data(), r.obs, obs_tm.size() * 4); home(act_tm.data(), r.act, act_tm.size() * 4); home(rew_tm.data(), r.rew, rew_tm.size() * 4);
    if (!drained()) return c;
    traj_reorder(r.M, r.D, r.W, r.Tcap, lengths, obs_tm.data(), act_tm.data(), rew_tm.data(), observations, actions, rewards);
    return c;
}
#endif
}  // namespace dril
