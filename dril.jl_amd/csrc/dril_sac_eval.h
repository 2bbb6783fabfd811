// dril_sac_eval.h — the host arithmetic of a device-resident evaluate_agent (evaluation.jl:90-124): the event record the evaluation kernels append, and the reduction
// of a copied event list to what evaluate_agent returns.  No HIP dependency: dril_sac_handle.h includes it, and tests/test_sac_monitor_eval.py builds the same lines with
// g++.  Written against the record alone, so another handle's evaluation appends the same events and reuses it: the PPO verb dril_evaluate_agent_device does (dril_eval_account.h, dril_eval.hip).
//
// The list.  Every env keeps its running return / length on the device; where an episode ends the env's thread appends {step, env, return, length} through ONE
// atomic counter.  Launches of one stream are ordered, so every event of step s has a lower index than any event of step s + 1; inside a step the order is whatever
// the atomics made it.  The first n episodes in (step, env) order — the order the reference's loop over envs appends them in — therefore all sit in the first n + E
// slots: if episode number n finishes in step s*, fewer than n events came before that step and at most E belong to it.  That is the list's capacity; later events only
// bump the counter.  The host sorts the copied slots by (step, env) and takes n, so the result depends neither on the atomic order nor on how many steps were enqueued
// past s* before the host looked.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include "../../include/dril_hip.h"   // dril_eval_stats

namespace dril {
struct SacEvalEvent { int32_t step, env; float ret; int32_t len; };   // step: 1-based env step of the evaluation in which the episode ended
static_assert(sizeof(SacEvalEvent) == 16, "one 16-byte store per event");

inline int64_t sac_eval_event_capacity(int64_t n_eval, int64_t n_envs) { return n_eval + n_envs; }

struct SacEvalSummary { double mean_reward, std_reward, mean_length, std_length; int32_t n_episodes, n_steps; };

// events[0, n_events): the copied slots, in any order (sorted in place).  Takes the first min(n_eval, n_events) episodes in (step, env) order (:100-121), writes them to
// episode_rewards / episode_lengths (either may be null) and returns Julia's mean and corrected std (NaN for a single episode, :123-124) and n_steps = the step at which
// the last counted episode finished.  Returns the number of episodes taken.
inline int32_t sac_eval_reduce(SacEvalEvent* events, int64_t n_events, int32_t n_eval, SacEvalSummary* out, float* episode_rewards, int32_t* episode_lengths) {
    std::sort(events, events + n_events, [](const SacEvalEvent& a, const SacEvalEvent& b) { return a.step != b.step ? a.step < b.step : a.env < b.env; });
    const int32_t n = (int32_t)std::min<int64_t>(n_eval, n_events);
    double mr = 0, ml = 0;
    for (int32_t i = 0; i < n; ++i) { mr += events[i].ret; ml += events[i].len; }
    if (n > 0) { mr /= n; ml /= n; }
    double vr = 0, vl = 0;
    for (int32_t i = 0; i < n; ++i) { vr += (events[i].ret - mr) * (events[i].ret - mr); vl += (events[i].len - ml) * (events[i].len - ml); }
    out->mean_reward = mr; out->mean_length = ml;
    out->std_reward = sqrt(vr / (n - 1)); out->std_length = sqrt(vl / (n - 1));       // 0 / 0 for one episode: NaN, as Julia's std of one element
    out->n_episodes = n; out->n_steps = n > 0 ? events[n - 1].step : 0;
    for (int32_t i = 0; i < n; ++i) { if (episode_rewards) episode_rewards[i] = events[i].ret; if (episode_lengths) episode_lengths[i] = events[i].len; }
    return n;
}
// the same into the struct both handles' verbs return (dril_sac_evaluate_agent, dril_evaluate_agent_device)
inline void sac_eval_stats(SacEvalEvent* events, int64_t n_events, int32_t n_eval, dril_eval_stats* out, float* episode_rewards, int32_t* episode_lengths) {
    SacEvalSummary sum{}; sac_eval_reduce(events, n_events, n_eval, &sum, episode_rewards, episode_lengths);
    out->mean_reward = sum.mean_reward; out->std_reward = sum.std_reward; out->mean_length = sum.mean_length; out->std_length = sum.std_length; out->n_episodes = sum.n_episodes; out->n_steps = sum.n_steps;
}
}  // namespace dril
