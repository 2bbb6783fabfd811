// dril_traj_run.h — the recording setup of a device-resident collect_trajectory, for the PPO handle (dril_eval.hip) and the SAC handle (dril_sac_eval.hip) alike: the layout
// of the handle's private blob, the table of bounds behind TrajMaps, the shadow envs, and the refusals and reports in which only the verb's name differs.  Nothing
// here knows a handle: envs, stream, the blob's owner, a counter and sizes are plain arguments, and an error comes back as a hipError_t or as a message (empty:
// none) for the caller's own fail / sfail.  No HIP dependency above the #if (tests/test_traj_run.py drives traj_layout and traj_bounds_table with g++).
#pragma once
#include <string>

#include "../../include/dril_hip.h"
#include "dril_traj_record.h"
#if defined(__HIPCC__) || defined(__CUDACC__)
#include <algorithm>
#include <vector>
#include "dril_devmem.h"     // DevBuf: the blob
#include "dril_env_side.h"   // DeviceEnvs; scaled_kind_boxes (dril_env_kinds.h) through dril_internal.h
#endif

namespace dril {
// ---- the blob: one grow-only allocation per handle, carved anew by every call; every region starts on a 256-byte boundary ----
struct TrajRegion { size_t at, bytes; };
struct TrajLayout {
    size_t M, D, W, S, Tcap;
    TrajRegion obs, act, rew, len, flg, st, sc, ep, gs;        // the step-major recording (TrajRec): the five terms of traj_bytes; the shadow envs' state, step_count, episode, gstep
    TrajRegion srew, sterm, strunc, stobs, sobs, tab;          // where the shadow step and the shadow observe write; the table of bounds
    size_t total;
};
inline size_t traj_table_floats(size_t D, size_t W) { return 2 * D + 4 * W; }
inline TrajLayout traj_layout(size_t M, size_t D, size_t W, size_t S, size_t T) {
    size_t off = 0;
    auto take = [&off](size_t bytes) { const TrajRegion r{off, bytes}; off += (bytes + 255) & ~(size_t)255; return r; };
    TrajLayout L{M, D, W, S, T,
                 take((T + 1) * M * D * 4), take(T * M * W * 4), take(T * M * 4), take(M * 4), take(M),      // obs, act, rew, len, flg
                 take(M * S * 4), take(M * 4), take(M * 4), take(M * 4),                                     // st, sc, ep, gs
                 take(M * 4), take(M), take(M), take(M * D * 4), take(M * D * 4), take(traj_table_floats(D, W) * 4), 0};
    L.total = off;
    return L;
}
// ---- the table of bounds: obs_low | obs_high (D each), clamp_low | clamp_high | act_low | act_high (W each) ----
// What a handle knows of its spaces, as host arrays; a null pair is an absent map.  obs_* / act_*: the boxes ScalingWrapperEnv maps from (null: no wrapper); clamp_*:
// ClampAdapter's agent-facing Box (null: no ClampAdapter — SAC's TanhScaleAdapter stays inside the Box by construction); discrete: neither clamp nor action map
struct TrajBoxes { const float *obs_low, *obs_high, *act_low, *act_high, *clamp_low, *clamp_high; bool discrete; };
// fills tab[traj_table_floats(D, W)] (absent columns: 0) and returns the maps, their pointers into `dev`: where the caller puts the table on the device
inline TrajMaps traj_bounds_table(size_t D, size_t W, const TrajBoxes& b, bool final_original, float* tab, const float* dev) {
    const size_t col[6] = {0, D, 2 * D, 2 * D + W, 2 * D + 2 * W, 2 * D + 3 * W};
    const bool scaled = b.obs_low != nullptr, act = scaled && !b.discrete, clamp = b.clamp_low != nullptr && !b.discrete;
    for (size_t i = 0; i < traj_table_floats(D, W); ++i) tab[i] = 0.f;
    if (scaled) for (size_t i = 0; i < D; ++i) { tab[col[0] + i] = b.obs_low[i]; tab[col[1] + i] = b.obs_high[i]; }
    if (clamp) for (size_t i = 0; i < W; ++i) { tab[col[2] + i] = b.clamp_low[i]; tab[col[3] + i] = b.clamp_high[i]; }
    if (act) for (size_t i = 0; i < W; ++i) { tab[col[4] + i] = b.act_low[i]; tab[col[5] + i] = b.act_high[i]; }
    return TrajMaps{scaled ? dev + col[0] : nullptr, scaled ? dev + col[1] : nullptr, clamp ? dev + col[2] : nullptr, clamp ? dev + col[3] : nullptr,
                    act ? dev + col[4] : nullptr, act ? dev + col[5] : nullptr, b.discrete ? 1 : 0, final_original ? 1 : 0};
}
// ---- argument handling and reporting: a message, or empty ----
inline std::string traj_options_error(const char* verb, const dril_traj_options* o, bool five_arrays, int32_t n_envs) {
    if (o && five_arrays && o->n_trajectories >= 1 && o->n_trajectories <= n_envs && o->max_steps >= 0 && o->poll_steps >= 0) return {};
    return std::string(verb) + ": options and the five output arrays != NULL, 1 <= n_trajectories <= n_envs, max_steps >= 0, poll_steps >= 0";
}
// clears info (null: not asked for), gives Tcap, and refuses a recording above 1 GiB
inline std::string traj_size_error(const char* verb, const dril_traj_options* o, int32_t episode_len, int32_t D, int32_t W, dril_traj_info* info, int32_t* Tcap) {
    if (info) *info = dril_traj_info{};
    *Tcap = traj_capacity(o->max_steps, episode_len);
    const int64_t bytes = traj_bytes(o->n_trajectories, *Tcap, D, W);
    if (bytes <= (1ll << 30)) return {};
    return std::string(verb) + ": the recording needs " + std::to_string(bytes) + " bytes on the device (M = " + std::to_string(o->n_trajectories) + ", Tcap = " + std::to_string(*Tcap) + "), more than 1 GiB: record fewer envs or set max_steps";
}
#if defined(__HIPCC__) || defined(__CUDACC__)
// after traj_copy_out: its error in words, or none and `info` (null: not asked for) filled
inline std::string traj_report(const char* verb, const TrajCopyOut& c, int32_t Tcap, int32_t steps, int32_t launches, int32_t path, dril_traj_info* info) {
    if (c.err != hipSuccess) return std::string(verb) + ": copy-out: " + hipGetErrorString(c.err);
    if (c.bad >= 0) return std::string(verb) + ": trajectory " + std::to_string(c.bad) + " has length " + std::to_string(c.bad_length) + " (internal)";
    if (info) { info->capacity = Tcap; info->steps_enqueued = steps; info->launches = launches; info->longest = c.longest; info->cut_by_max_steps = c.cuts; info->reserved[DRIL_TRAJ_INFO_PATH] = path; }
    return {};
}
// ---- one call's recording.  shadow: M twins of envs 0..M-1 that never reset, a DeviceEnvs view of the handle's envs with its own arrays (unused where a kernel records from registers) ----
struct TrajRun { TrajRec rec; TrajMaps maps; DeviceEnvs shadow; float *sh_rew, *sh_tobs, *sh_obs; uint8_t *sh_term, *sh_trunc; };
// the recording of env step t (0: row 0) by either handle's kernel: a thread per (env, word) of the M recorded envs
using TrajRecordKernel = void (*)(TrajRec, TrajMaps, TrajStep, int32_t);
inline hipError_t traj_record_launch(TrajRecordKernel kernel, hipStream_t stream, const TrajRun& r, const TrajStep& s, int32_t t) {
    const int64_t n = (int64_t)r.rec.M * std::max(r.rec.D, r.rec.W);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, r.rec, r.maps, s, t);
    return hipGetLastError();
}
// the boxes ScalingWrapperEnv maps from, where the handle's envs are wrapped: a plug-in's declared spaces, or the table of the built-in scaled kinds
inline TrajBoxes traj_env_boxes(const DeviceEnvs& env) {
    if (env.module) return env.scaling ? TrajBoxes{env.obs_low.data(), env.obs_high.data(), env.desc.action_low, env.desc.action_high, nullptr, nullptr, false} : TrajBoxes{};
    if (const ScaledKindBoxes* sb = scaled_kind_boxes(env.kind)) return TrajBoxes{sb->obs_low, sb->obs_high, &sb->act_low, &sb->act_high, nullptr, nullptr, false};
    return TrajBoxes{};
}
// Grows the blob where L needs more (drain_before_free: the handle does not free under a running stream), carves it, builds r and puts the table on the device.
// Returns with `stream` drained: the table's host copy is a local
inline hipError_t traj_setup(const DeviceEnvs& env, hipStream_t stream, DevBuf<char>& blob, unsigned int* counter, const TrajLayout& L, const TrajBoxes& boxes,
                             bool final_original, bool drain_before_free, TrajRun& r) {
    if (L.total > blob.size()) {
        if (drain_before_free) { if (const hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return e; }
        if (const hipError_t e = blob.alloc(L.total); e != hipSuccess) return e;
    }
    char* b = blob;
    r.rec = TrajRec{(int32_t)L.M, (int32_t)L.D, (int32_t)L.W, (int32_t)L.Tcap, (float*)(b + L.obs.at), (uint32_t*)(b + L.act.at), (float*)(b + L.rew.at), (int32_t*)(b + L.len.at),
                    (uint8_t*)(b + L.flg.at), counter};
    r.shadow = env;                                                                // the kind / the plug-in's kernels, scaling, action_start
    r.shadow.E = (int)L.M; r.shadow.fixed_len = 1; r.shadow.episode_len = INT32_MAX; r.shadow.disc_returns = nullptr;
    r.shadow.state = (float*)(b + L.st.at); r.shadow.step_count = (int32_t*)(b + L.sc.at); r.shadow.episode = (uint32_t*)(b + L.ep.at); r.shadow.gstep = (uint32_t*)(b + L.gs.at);
    r.sh_rew = (float*)(b + L.srew.at); r.sh_term = (uint8_t*)(b + L.sterm.at); r.sh_trunc = (uint8_t*)(b + L.strunc.at); r.sh_tobs = (float*)(b + L.stobs.at); r.sh_obs = (float*)(b + L.sobs.at);
    std::vector<float> tab(traj_table_floats(L.D, L.W));
    r.maps = traj_bounds_table(L.D, L.W, boxes, final_original, tab.data(), (const float*)(b + L.tab.at));
    if (const hipError_t e = hipMemcpyAsync(b + L.tab.at, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, stream); e != hipSuccess) return e;
    return hipStreamSynchronize(stream);
}
#endif
}  // namespace dril
