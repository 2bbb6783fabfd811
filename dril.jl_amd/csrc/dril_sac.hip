// dril_sac.hip — the off-policy (SAC) path of libdril_hip.so, its API unit: create / destroy, the parameter, env and prediction verbs, the replay ring,
// dril_sac_train / dril_sac_iterate and profiling, of the C ABI of include/dril_sac.h.  The contractions of a net (dril_sac_net.hip), the gradient step
// (dril_sac_update.hip), the collection (dril_sac_collect.hip), the two wrappers (dril_sac_wrap.hip), the external-env verbs (dril_sac_ext.hip) and the evaluation
// (dril_sac_eval.hip) are units of their own around dril_sac_handle.h; what their kernels share is dril_sac_device.h.
//
// Reference: src/algorithms/sac.jl (losses :93-150, update! :299-404, train! :406-549), src/buffers/replay_buffer.jl,
// src/buffers/off_policy_collection.jl, src/DRiLDistributions/squashedDiagGaussian.jl.  BASELINE.json configs[4]:
// Pendulum-v1, 4096 device envs, SACLayer [512,512] relu, batch 256.
//
// Shape of the work (docs/sac.md): one gradient step is ~25 small dense contractions (256 samples x 512 x 512) separated by
// per-sample head math, all on one stream with no host round trip; one env step of the collection is the actor forward over
// 4096 envs + the env kernels of the on-policy path + a ring write.  The contractions are fp32 MFMA (v_mfma_f32_32x32x2_f32:
// exact fp32 products, fp32 accumulate) in ONE generic strided kernel: a workgroup owns one 32x32 output tile and its four
// waves split the contraction axis (in-workgroup split-K, summed through LDS in fixed wave order => deterministic), because
// with only 128..272 output tiles per contraction the chip is filled by K-parallelism, not by tiles.  Bias rides in the forward
// epilogue; [dW | db] come out of one contraction by appending a ones column to the activation operand (the flat parameter
// layout stores b right behind the column-major W, i.e. [W | b] is one (out x (in+1)) column-major matrix).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "dril_sac_handle.h"
#include "dril_policy_internal.h"   // dril_policy_from_sac_handle: the snapshot this handle gives a deployment policy (dril_policy.hip)

using namespace dril;
using namespace dril::sac;

namespace {

thread_local std::string g_sac_create_error;

// the loop-start stamp of dril_sac_iterate (phase_stamp, dril_sac_device.h: the later stamps are written by the last kernel of each phase)
__global__ void sac_stamp_kernel(unsigned long long* stamp) { phase_stamp(stamp); }

// host-batch helpers
__global__ void sac_squash_eval_kernel(int B, int A, const float* mu, const float* log_std, const float* noise, int deterministic, const float* low, const float* high,
                                       float* actions, float* logp, float* envact) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    float ls[kMaxA], a_[kMaxA], gg[kMaxA], nz[kMaxA];
    for (int a = 0; a < A; ++a) { ls[a] = log_std[a]; nz[a] = deterministic ? 0.f : noise[i * A + a]; }
    const float lp = squashed_sample_logp(mu + (size_t)i * A, ls, nz, A, a_, gg);              // deterministic: mode(d) = tanh(mean) :48-50
    for (int a = 0; a < A; ++a) {
        if (actions) actions[i * A + a] = a_[a];
        if (envact) envact[i * A + a] = sac_to_env(a_[a], low[a], high[a]);
    }
    if (logp) logp[i] = lp;
}
__global__ void sac_concat_kernel(int B, int D, int A, const float* obs, const float* act, float* xq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    for (int d = 0; d < D; ++d) xq[(size_t)i * (D + A) + d] = obs[(size_t)i * D + d];
    for (int a = 0; a < A; ++a) xq[(size_t)i * (D + A) + D + a] = act[(size_t)i * A + a];
}
__global__ void sac_noise_fill_kernel(int n, int A, SacRng rng, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int a = 0; a < A; ++a) out[i * A + a] = sac_noise(rng, 8, i, a);
}

constexpr int kXpPool = 4096;                       // HIP events of an external handle under cfg.profile_events: 1 024 env steps (act + push) between two flushes

// train!'s loop body (sac.jl:464-535) for `count` iterations WITHOUT a host synchronisation between them: {train_freq env steps, n_upd gradient steps} enqueued back to
// back, one drain at the end.  Nothing the host decides depends on device results (the replay ring's head / size are host counters, batch indices and noise are
// device Philox streams keyed by the update counter), so the launches are the ones the step-by-step sequence issues, in the same order: bit-identical state.
// fps of an iteration = env steps / HIP-event time of its collection (the reference times the same span on the host clock, off_policy_collection.jl:126-128).
int run_iterations(dril_sac_handle* h, int count, int tf, int n_upd, dril_sac_stats* stats, int64_t stats_room, double* fps, int64_t fps_room) {
    if (count <= 0) return DRIL_OK;
    SDO(collect_prepare(h, tf));
    if (n_upd > 0) { if (h->size <= 0 && tf <= 0) return sfail(h, DRIL_ERR_NOT_INITIALISED, "the replay buffer is empty"); SDO(ensure_stats(h, count * n_upd)); }
    const bool timed = h->cfg.profile_events || fps;
    const int n_st = 1 + 2 * count;                                                        // [loop start | per iteration: collection end, update end] (phase_stamp)
    if (timed) {
        SHIP(h, h->it_stamps.grow_zero((size_t)n_st));
        SHIP(h, hipMemsetAsync(h->it_stamps, 0, sizeof(unsigned long long) * n_st, h->stream));
        hipLaunchKernelGGL(sac_stamp_kernel, dim3(1), dim3(64), 0, h->stream, h->it_stamps);
    }
    for (int j = 0; j < count; ++j) {
        if (h->nz.on && tf > 0) SDO(nz_collect_begin(h));                                  // every iteration is one collect_trajectories call: it begins with observe(env)
        for (int t = 0; t < tf; ++t) SDO(collect_step(h, 0, nullptr, timed && t == tf - 1 ? h->it_stamps + 1 + 2 * j : nullptr, t == 0, t == tf - 1));
        SDO(monitor_end(h));                                                               // (the next iteration's steps reuse the rows: stream order keeps them apart)
        for (int k = 0; k < n_upd; ++k) SDO(sac_one_update(h, -1, h->stats_out + ((size_t)j * n_upd + k) * 8, timed && k == n_upd - 1 ? h->it_stamps + 2 + 2 * j : nullptr));
    }
    SDO(ssync(h));
    if (timed) {
        std::vector<unsigned long long> st((size_t)n_st);
        SHIP(h, hipMemcpy(st.data(), h->it_stamps, st.size() * 8, hipMemcpyDeviceToHost));
        unsigned long long prev = st[0];
        for (int j = 0; j < count; ++j) {
            const unsigned long long ce = st[1 + 2 * j] ? st[1 + 2 * j] : prev, ue = st[2 + 2 * j] ? st[2 + 2 * j] : ce;   // (a phase that did not run left no stamp: zero length)
            const double c = 1e3 * (double)(ce - prev) / h->wall_hz, u = 1e3 * (double)(ue - ce) / h->wall_hz;             // ms
            if (h->cfg.profile_events) { h->collect_ms += c; h->collect_steps += tf; h->update_ms += u; h->updates += n_upd; }
            if (fps && j < fps_room) fps[j] = (double)tf * h->cfg.n_envs / (c > 0 ? 1e-3 * c : 1e-9);
            prev = ue;
        }
    }
    if (stats && n_upd > 0 && stats_room > 0) {
        std::vector<dril_sac_stats> tmp((size_t)count * n_upd);
        SDO(fetch_stats(h, count * n_upd, tmp.data()));
        for (int64_t k = 0; k < std::min<int64_t>(stats_room, (int64_t)tmp.size()); ++k) stats[k] = tmp[(size_t)k];
    }
    return DRIL_OK;
}
void reset_optimizer(dril_sac_handle* h) {
    h->bt_actor[0] = h->bt_critic[0] = h->bt_ent[0] = h->cfg.adam_beta1; h->bt_actor[1] = h->bt_critic[1] = h->bt_ent[1] = h->cfg.adam_beta2;
    h->grad_updates = 0;
}
// ---- host (ABI) layout <-> padded device layout ------------------------------------------------------------------------
struct Seg { int host, dev, len; };
void param_segs(const dril_sac_handle* h, Seg (&s)[4]) {
    s[0] = {0, 0, h->Pa}; s[1] = {h->Pa, h->q0.w1, h->Pq}; s[2] = {h->Pa + h->Pq, h->q0.w1 + h->Pqd, h->Pq}; s[3] = {h->Pa + 2 * h->Pq, h->log_std_off, h->A};
}
int params_to_device(dril_sac_handle* h, float* dev, const float* host) {
    Seg s[4]; param_segs(h, s);
    for (const Seg& g : s) SHIP(h, hipMemcpyAsync(dev + g.dev, host + g.host, (size_t)g.len * 4, hipMemcpyHostToDevice, h->stream));
    return ssync(h);
}
int params_from_device(dril_sac_handle* h, float* host, const float* dev) {
    SDO(ssync(h));
    Seg s[4]; param_segs(h, s);
    for (const Seg& g : s) SHIP(h, hipMemcpy(host + g.host, dev + g.dev, (size_t)g.len * 4, hipMemcpyDeviceToHost));
    return DRIL_OK;
}

// what SAC asks of a plug-in beyond the loader's checks; decided on the host from the descriptor, before anything of the module is launched
int check_sac_plugin(const DrilEnvPluginDesc& d, std::string& msg) {
    if (d.discrete) { msg = std::string("env plug-in \"") + d.name + "\" has a Discrete action space: SAC needs a Box (sac.jl:74); Discrete plug-ins run PPO (dril_create_with_env_module)"; return DRIL_ERR_UNSUPPORTED; }
    if (d.A > kMaxA) { msg = std::string("env plug-in \"") + d.name + "\" has " + std::to_string(d.A) + " action dims: the SAC kernels hold up to " + std::to_string(kMaxA) + " (the ext_action_dim limit)"; return DRIL_ERR_UNSUPPORTED; }
    for (int a = 0; a < d.A; ++a)
        if (!(d.action_low[a] < d.action_high[a])) {
            msg = std::string("env plug-in \"") + d.name + "\": action dim " + std::to_string(a) + " has action_low " + std::to_string(d.action_low[a]) + " >= action_high " + std::to_string(d.action_high[a]) +
                  ": TanhScaleAdapter scales into a finite Box (ClampAdapter's \"no clamp\" convention has no meaning for SAC)";
            return DRIL_ERR_UNSUPPORTED;
        }
    return DRIL_OK;
}
int sac_create_impl(const dril_sac_config* cfg, const char* module_path, dril_sac_handle** out) {
    if (!cfg || !out) return sfail(nullptr, DRIL_ERR_INVALID_ARG, "null config / out pointer");
    if (cfg->abi_version != DRIL_SAC_ABI_VERSION) return sfail(nullptr, DRIL_ERR_INVALID_ARG, "dril_sac_config.abi_version mismatch");
    const bool ext = cfg->env_kind == DRIL_ENV_EXTERNAL, is_module = cfg->env_kind == DRIL_ENV_MODULE;
    if (is_module && cfg->episode_len < 0) return sfail(nullptr, DRIL_ERR_INVALID_ARG, "DRIL_ENV_MODULE: episode_len must be > 0, or 0 for the plug-in's own time limit");
    const EnvKindInfo* kinfo = env_kind_info(cfg->env_kind);
    if (!ext && !is_module && !(kinfo && kinfo->box)) return sfail(nullptr, DRIL_ERR_UNSUPPORTED, "SAC needs a Box action space (sac.jl:74): DRIL_ENV_PENDULUM[_SCALED] or DRIL_ENV_EXTERNAL");
    if (ext && (cfg->ext_obs_dim < 1 || cfg->ext_obs_dim > 1024 || cfg->ext_action_dim < 1 || cfg->ext_action_dim > kMaxA || !(cfg->ext_action_low < cfg->ext_action_high)))
        return sfail(nullptr, DRIL_ERR_INVALID_ARG, "DRIL_ENV_EXTERNAL: ext_obs_dim 1..1024, ext_action_dim 1..16, ext_action_low < ext_action_high");
    if (cfg->n_envs <= 0 || (!ext && !is_module && cfg->episode_len <= 0) || cfg->batch_size <= 0 || cfg->buffer_capacity < cfg->n_envs || cfg->train_freq <= 0 || cfg->target_update_interval <= 0)
        return sfail(nullptr, DRIL_ERR_INVALID_ARG, "n_envs, episode_len, batch_size, train_freq, target_update_interval must be positive and buffer_capacity >= n_envs");
    if (cfg->hidden1 <= 0 || cfg->hidden2 <= 0 || cfg->hidden1 % 4 || cfg->hidden2 % 4) return sfail(nullptr, DRIL_ERR_UNSUPPORTED, "hidden dims must be positive multiples of 4");
    if (cfg->activation != 0 && cfg->activation != 1) return sfail(nullptr, DRIL_ERR_INVALID_ARG, "activation: 0 tanh, 1 relu");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return sfail(nullptr, DRIL_ERR_HIP, "no HIP device: libdril_hip has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return sfail(nullptr, DRIL_ERR_INVALID_ARG, "device ordinal out of range");
    dril_sac_handle* h = new dril_sac_handle(); h->cfg = *cfg;
    {   // a plug-in's descriptor gives the spaces and the bounds: it is loaded here, before anything is sized (dril_sac_destroy unloads it on every failing path below)
        std::string msg; int rcm = h->env.open(cfg->env_kind, cfg->n_envs, cfg->episode_len, /*fixed_len=*/0, /*action_start=*/0, module_path, cfg->device, msg,
                                          "SAC steps one env per row; a world trains with PPO (dril_create_with_env_module)");
        if (!rcm && is_module) rcm = check_sac_plugin(h->env.desc, msg);
        if (rcm) { h->env.release(); delete h; return sfail(nullptr, rcm, "dril_sac_create_with_env_module: " + msg); }
        h->cfg.episode_len = h->env.episode_len;
    }
    const DrilEnvPluginDesc& desc = h->env.desc;
#define CHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { std::string m = std::string(#expr) + ": " + hipGetErrorString(_e); dril_sac_destroy(h); return sfail(nullptr, DRIL_ERR_HIP, m); } } while (0)
    CHK(hipSetDevice(cfg->device));
    CHK(hipStreamCreate(&h->stream));
    { int khz = 0; if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->cfg.device) == hipSuccess && khz > 0) h->wall_hz = 1e3 * (double)khz; }   // wall_clock64 ticks per second (phase_stamp)
    const int D = h->D = is_module ? desc.D : ext ? cfg->ext_obs_dim : kinfo->D, A = h->A = is_module ? desc.A : ext ? cfg->ext_action_dim : kinfo->A, S = h->S = is_module ? desc.S : ext ? 0 : kinfo->S, H1 = h->H1 = cfg->hidden1, H2 = h->H2 = cfg->hidden2, E = cfg->n_envs, B = cfg->batch_size, W = D + A;
    h->Pa = D * H1 + H1 + H1 * H2 + H2 + H2 * A + A; h->Pq = W * H1 + H1 + H1 * H2 + H2 + H2 + 1; h->P = h->Pa + 2 * h->Pq + A;
    h->actor = net_off(0, D, H1, H2, A); h->Pqd = round4(h->Pq); h->q0 = net_off(round4(h->actor.end), W, H1, H2, 1);
    h->log_std_off = h->q0.w1 + 4 * h->Pqd; h->Pd = round4(h->log_std_off + A);      // device layout: actor | q1 | q2 | target q1 | target q2 | log_std
    h->nq = B; h->nmax = std::max(E, 2 * B);
    h->target_entropy = cfg->auto_target_entropy ? -(float)A : cfg->target_entropy;
    h->external = ext;
    if (ext) { h->act_lo = cfg->ext_action_low; h->act_hi = cfg->ext_action_high; }
    else if (kinfo) { h->act_lo = kinfo->act_lo; h->act_hi = kinfo->act_hi; }
    {   // the bounds table of the sampling kernels
        float tb[2 * kMaxA];
        for (int a = 0; a < kMaxA; ++a) { const bool own = is_module && a < A; tb[a] = own ? desc.action_low[a] : h->act_lo; tb[kMaxA + a] = own ? desc.action_high[a] : h->act_hi; }
        CHK(h->act_bounds.alloc_zero(2 * kMaxA)); CHK(hipMemcpy(h->act_bounds, tb, sizeof(tb), hipMemcpyHostToDevice));
    }
    if (is_module) {
        h->fused_head_push = std::getenv("DRIL_SAC_NO_FUSED_HEAD_PUSH") == nullptr;           // A/B switch, latched here: head + plug-in step + push as three launches per env step
    }
    CHK(h->params.alloc_zero(h->Pd)); CHK(h->adam_m.alloc_zero(h->Pd)); CHK(h->adam_v.alloc_zero(h->Pd));
    h->target = h->params + h->q0.w1 + 2 * h->Pqd;   // the targets sit right behind the critics so that one launch runs all four Q nets (blockIdx.z stride Pqd)
    CHK(h->g_critic.alloc_zero(h->Pd)); CHK(h->g_actor.alloc_zero(h->Pd)); CHK(h->sc.alloc_zero(1)); CHK(h->sc_next.alloc_zero(1)); CHK(h->stats.alloc_zero(8));
    h->adam_blocks_c = std::min(kSacAdamBlocks, (2 * h->Pqd + 255) / 256); h->end_blocks = std::min(kSacAdamBlocks, ((h->actor.end + 3) / 4 + 2 * h->Pqd / 4 + 255) / 256);   // elementwise optimiser kernels: up to 1 024 blocks (no grid-wide fold is left in them; 256 -> 1 024: update! 0.174 -> 0.168 ms)
    // narrow first layers: their gradient, step and (critics) re-evaluation inside the optimiser kernels (first_layer_opt_block; DRIL_SAC_NO_FUSED_DW1=1: launches of their own)
    h->fused_dw1 = std::getenv("DRIL_SAC_NO_FUSED_HEADS") == nullptr && std::getenv("DRIL_SAC_NO_FUSED_DW1") == nullptr && W <= kOptL1MaxIn && H1 % 4 == 0 && B <= kOptL1MaxB;
    if (h->fused_dw1) { h->fl_a = (H1 + kOptL1Units - 1) / kOptL1Units; h->fl_c = 2 * h->fl_a; h->adam_blocks_c += h->fl_c; h->end_blocks += h->fl_a; }
    CHK(h->counter.alloc_zero(1));
    CHK(h->head_partials.alloc_zero((size_t)(2 * kMaxA + 8) * ((B + kHeadSamplesPerBlock - 1) / kHeadSamplesPerBlock + 1))); CHK(h->head_counter.alloc_zero(kMaxA + 1));   // doubles: [critic 2 | actor 2 | log_std kMaxA | entropy 2] x blocks
    h->fused_heads = std::getenv("DRIL_SAC_NO_FUSED_HEADS") == nullptr; h->fused_collect = std::getenv("DRIL_SAC_NO_FUSED_COLLECT") == nullptr; h->fused_fwd = std::getenv("DRIL_SAC_NO_FUSED_FWD") == nullptr; h->f16_fwd = std::getenv("DRIL_SAC_NO_F16_FWD") == nullptr; h->trace_enqueue = false;   // latched here: no getenv on the update path
    // evaluate_agent: env steps enqueued between two looks of the host at the event counter.  A look is one 4-byte copy and a stream drain (measured: 9 - 10 us per look on
    // built-in Pendulum, half an env step; docs/sac.md); 32 steps per look put it under half a microsecond per step, and at most 31 steps (under a millisecond) run
    // past the step that completes the list.  No more than the time limit, after which every env has finished an episode.  DRIL_SAC_EVAL_POLL=<k> overrides; 1 is the step-by-step definition.
    h->eval_poll = std::max(1, std::min(h->cfg.episode_len, 32));
    if (const char* ep = std::getenv("DRIL_SAC_EVAL_POLL")) { const long k = std::strtol(ep, nullptr, 10); if (k >= 1) h->eval_poll = (int)std::min<long>(k, 1 << 20); }
    CHK(h->env.alloc(S));
    CHK(h->obs_cur.alloc_zero((size_t)E * D)); CHK(h->obs_nxt.alloc_zero((size_t)E * D)); CHK(h->e_rew.alloc_zero(E)); CHK(h->e_tobs.alloc_zero((size_t)E * D));
    CHK(h->e_raw.alloc_zero((size_t)E * A)); CHK(h->e_envact.alloc_zero((size_t)E * A)); CHK(h->e_term.alloc_zero(E)); CHK(h->e_trunc.alloc_zero(E));
    h->cap = cfg->buffer_capacity;
    CHK(h->rb_obs.alloc_zero((size_t)h->cap * D)); CHK(h->rb_next.alloc_zero((size_t)h->cap * D)); CHK(h->rb_act.alloc_zero((size_t)h->cap * A));
    CHK(h->rb_rew.alloc_zero((size_t)h->cap)); CHK(h->rb_term.alloc_zero((size_t)h->cap)); CHK(h->rb_trunc.alloc_zero((size_t)h->cap));
    const size_t nm = h->nmax, nq = h->nq;
    if (H1 % 2 == 0) { CHK(h->col_h1p.alloc_zero((size_t)2 * nm * (H1 / 2))); CHK(h->col_w2p.alloc_zero((size_t)2 * H2 * (H1 / 2))); CHK(h->col_flags.alloc_zero(2)); }   // f16 planes of h1 [2][nm][H1/2] and of the actor's W2 [2][H2][H1/2]; their range flags
    CHK(h->xa.alloc_zero(nm * D)); CHK(h->ah1.alloc_zero(nm * H1)); CHK(h->ah2.alloc_zero(nm * H2)); CHK(h->mu.alloc_zero(nm * A));
    CHK(h->xq.alloc_zero(2 * nq * W)); h->xq_next = h->xq + nq * W; CHK(h->xq_pi.alloc_zero(nq * W));       // [xq | xq_next]: one input buffer, batch index z / 2
    CHK(h->qh1.alloc_zero(4 * nq * H1)); CHK(h->qh2.alloc_zero(4 * nq * H2)); h->th1 = h->qh1 + 2 * nq * H1; h->th2 = h->qh2 + 2 * nq * H2;   // z = 0,1 critics (kept for the reverse pass), 2,3 targets
    CHK(h->q_cur.alloc_zero(4 * nq)); h->q_next = h->q_cur + 2 * nq; CHK(h->q_pi.alloc_zero(2 * nq)); CHK(h->dq.alloc_zero(2 * nq));
    CHK(h->dz2.alloc_zero(2 * nq * H2)); CHK(h->dz1.alloc_zero(2 * nq * H1)); CHK(h->dxq.alloc_zero(2 * nq * W)); CHK(h->dmu.alloc_zero(nq * A));
    CHK(h->b_rew.alloc_zero(nq)); CHK(h->b_ne.alloc_zero(nq * A)); CHK(h->b_nn.alloc_zero(nq * A)); CHK(h->b_np.alloc_zero(nq * A)); CHK(h->b_nlp.alloc_zero(nq));
    CHK(h->a_pi.alloc_zero(nq * A)); CHK(h->g_pi.alloc_zero(nq * A)); CHK(h->lp_pi.alloc_zero(nq)); CHK(h->b_term.alloc_zero(nq));
    CHK(h->s_in.alloc_zero(nm * D)); CHK(h->s_act.alloc_zero(nm * A)); CHK(h->s_noise.alloc_zero(nm * A)); CHK(h->s_out.alloc_zero(nm * A)); CHK(h->s_out2.alloc_zero(nm * A));
    CHK(hipEventCreate(&h->ev_a)); CHK(hipEventCreate(&h->ev_b));
    if (ext) {                                                                         // the device-array verbs: hand-over events and the sticky error word and the pending statistics table
        CHK(hipEventCreateWithFlags(&h->ext_ev_in, hipEventDisableTiming)); CHK(hipEventCreateWithFlags(&h->ext_ev_out, hipEventDisableTiming));
        CHK(h->ext_err.alloc_zero(1)); CHK(h->ext_err_host.alloc(1)); *h->ext_err_host = 0;
        if (cfg->profile_events) for (int i = 0; i < kXpPool; ++i) { hipEvent_t e = nullptr; CHK(hipEventCreate(&e)); h->xp_events.push_back(e); }   // (dril_sac_profile_get on this path: act / push pairs)
        // the pending statistics table of dril_sac_update_enqueue: allocated HERE, not on first use — an allocation and its fill would be a host wait inside a sync-free verb
        CHK(h->pend_stats.alloc_zero((size_t)DRIL_SAC_PENDING_CAPACITY * 8)); CHK(h->pend_ssq.alloc_zero((size_t)DRIL_SAC_PENDING_CAPACITY * (h->adam_blocks_c + h->end_blocks)));
    }
#undef CHK
    const SacScalars sc0{logf(cfg->ent_coef_init), 0.f, 0.f, cfg->ent_coef_init};                   // init_entropy_coefficient sac.jl:207-213
    if (hipMemcpy(h->sc, &sc0, sizeof(sc0), hipMemcpyHostToDevice) != hipSuccess) { dril_sac_destroy(h); return sfail(nullptr, DRIL_ERR_HIP, "hipMemcpy(log_ent_coef)"); }
    reset_optimizer(h);
    *out = h;
    return DRIL_OK;
}
// actor means of a host batch chunk already staged in h->xa, then the squashed sample / mode
int actor_chunk(dril_sac_handle* h, const float* obs, const float* noise, int n, int deterministic, int64_t chunk_id) {
    SHIP(h, hipMemcpyAsync(h->xa, obs, (size_t)n * h->D * 4, hipMemcpyHostToDevice, h->stream));
    if (!deterministic) {
        if (noise) SHIP(h, hipMemcpyAsync(h->s_noise, noise, (size_t)n * h->A * 4, hipMemcpyHostToDevice, h->stream));
        else {
            const SacRng rng{h->cfg.seed ^ 0x0b5e55edull, h->aux_counter++};
            hipLaunchKernelGGL(sac_noise_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, h->A, rng, h->s_noise);
        }
    }
    (void)chunk_id;
    return net_forward(h, h->params, h->actor, 0, h->D, h->A, h->xa, h->D, 0, n, actor_bufs(h), 1);
}

}  // namespace

namespace dril::sac {
int sfail(dril_sac_handle* h, int code, const std::string& msg) { if (h) h->err = msg; else g_sac_create_error = msg; return code; }
int ssync(dril_sac_handle* h) { if (h->in_device_verb) h->ext_syncs += 1; SHIP(h, hipStreamSynchronize(h->stream)); return DRIL_OK; }   // (ext_syncs: dril_sac_ext_device_info.host_syncs — a wait inside a sync-free verb is a bug it would show)
}  // namespace dril::sac

// =================================================================================================================
// exported entry points (include/dril_sac.h)
// =================================================================================================================
DRIL_EXPORT int32_t dril_sac_config_default(dril_sac_config* c, int32_t env_kind) {
    const EnvKindInfo* k = env_kind_info(env_kind);
    if (!c || (k ? !k->box : (env_kind != DRIL_ENV_EXTERNAL && env_kind != DRIL_ENV_MODULE))) return sfail(nullptr, DRIL_ERR_INVALID_ARG, "SAC needs a Box action space (sac.jl:74): env_kind must be DRIL_ENV_PENDULUM[_SCALED], DRIL_ENV_EXTERNAL or DRIL_ENV_MODULE");
    memset(c, 0, sizeof(*c));
    c->abi_version = DRIL_SAC_ABI_VERSION; c->env_kind = env_kind; c->n_envs = 1; c->episode_len = k ? k->default_episode_len /* the Gymnasium time limit */ : env_kind == DRIL_ENV_MODULE ? 0 /* the descriptor's */ : 200;
    c->hidden1 = 512; c->hidden2 = 512; c->activation = 1;
    c->buffer_capacity = 1000000; c->start_steps = 100; c->batch_size = 256; c->tau = 0.005f; c->gamma = 0.99f;
    c->train_freq = 1; c->gradient_steps = 1; c->target_update_interval = 1;
    c->auto_ent_coef = 1; c->ent_coef_init = 1.0f; c->auto_target_entropy = 1; c->target_entropy = 0.0f;
    c->learning_rate = 3.0e-4f; c->adam_beta1 = 0.9f; c->adam_beta2 = 0.999f; c->adam_eps = 1.0e-8f;
    c->seed = 42;
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_sac_destroy(dril_sac_handle* h) {
    if (!h) return DRIL_OK;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->ev_a) hipEventDestroy(h->ev_a); if (h->ev_b) hipEventDestroy(h->ev_b);
    for (hipEvent_t e : h->it_events) hipEventDestroy(e);
    for (hipEvent_t e : h->xp_events) hipEventDestroy(e);
    if (h->ext_ev_in) hipEventDestroy(h->ext_ev_in); if (h->ext_ev_out) hipEventDestroy(h->ext_ev_out);
    if (h->stream) hipStreamDestroy(h->stream);
    h->env.release();
    delete h;
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_sac_create(const dril_sac_config* cfg, dril_sac_handle** out) {
    if (cfg && cfg->abi_version == DRIL_SAC_ABI_VERSION && cfg->env_kind == DRIL_ENV_MODULE) return sfail(nullptr, DRIL_ERR_UNSUPPORTED, "SAC on a device env plug-in (DRIL_ENV_MODULE) needs the plug-in's code object: use dril_sac_create_with_env_module(cfg, code_object_path, out)");
    return sac_create_impl(cfg, nullptr, out);
}
DRIL_EXPORT int32_t dril_sac_create_with_env_module(const dril_sac_config* cfg, const char* code_object_path, dril_sac_handle** out) {
    if (!cfg || !out) return sfail(nullptr, DRIL_ERR_INVALID_ARG, "null config / out pointer");
    if (cfg->abi_version != DRIL_SAC_ABI_VERSION) return sfail(nullptr, DRIL_ERR_INVALID_ARG, "dril_sac_config.abi_version mismatch");
    if (cfg->env_kind != DRIL_ENV_MODULE) return sfail(nullptr, DRIL_ERR_INVALID_ARG, "dril_sac_create_with_env_module: cfg->env_kind must be DRIL_ENV_MODULE");
    std::string msg; const int rc = check_code_object_path(code_object_path, msg);
    if (rc) return sfail(nullptr, rc, "dril_sac_create_with_env_module: " + msg);
    return sac_create_impl(cfg, code_object_path, out);
}
DRIL_EXPORT int32_t dril_sac_env_module_info_of(const dril_sac_handle* h, dril_env_module_info* out) {
    if (!h || !out) return sfail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle / out");
    if (!h->env.module) return sfail(const_cast<dril_sac_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_sac_env_module_info_of: the handle was not created with dril_sac_create_with_env_module");
    fill_module_info(h->env.desc, out);
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_env_module_obs_space_of(const dril_sac_handle* h, float* low, float* high, int32_t* declared) {
    if (!h) return sfail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!h->env.module) return sfail(const_cast<dril_sac_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_sac_env_module_obs_space_of: the handle was not created with dril_sac_create_with_env_module");
    const int D = h->env.desc.D;
    if (low) std::memcpy(low, h->env.obs_low.data(), (size_t)D * 4);
    if (high) std::memcpy(high, h->env.obs_high.data(), (size_t)D * 4);
    if (declared) *declared = h->env.obs_declared ? 1 : 0;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_scaling_enable(dril_sac_handle* h, int32_t on) {
    SNEED(h);
    std::string msg; const int rc = h->env.set_scaling(on != 0, msg);
    if (rc) return sfail(h, rc, "dril_sac_scaling_enable: " + msg);
    // the adapters act on the wrapper's action space: the table the sampling kernels read (TanhScaleAdapter per dimension, rand(action_space) of the start phase).
    // The envs have not been reset, so nothing that reads the table is in flight.
    float tb[2 * kMaxA];
    SHIP(h, hipMemcpy(tb, h->act_bounds, sizeof(tb), hipMemcpyDeviceToHost));
    h->env.agent_action_space(tb, tb + kMaxA);
    SHIP(h, hipMemcpy(h->act_bounds, tb, sizeof(tb), hipMemcpyHostToDevice));
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_agent_spaces(const dril_sac_handle* h, float* obs_low, float* obs_high, float* action_low, float* action_high, int32_t* scaling) {
    if (!h) return sfail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!h->env.module) return sfail(const_cast<dril_sac_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_sac_agent_spaces: the handle was not created with dril_sac_create_with_env_module");
    h->env.agent_obs_space(obs_low, obs_high); h->env.agent_action_space(action_low, action_high);
    if (scaling) *scaling = h->env.scaling ? 1 : 0;
    return DRIL_OK;
}

DRIL_EXPORT const char* dril_sac_last_error(const dril_sac_handle* h) { return h ? h->err.c_str() : g_sac_create_error.c_str(); }
DRIL_EXPORT int32_t dril_sac_obs_dim(const dril_sac_handle* h) { return h ? h->D : 0; }
DRIL_EXPORT int32_t dril_sac_action_dim(const dril_sac_handle* h) { return h ? h->A : 0; }
DRIL_EXPORT int64_t dril_sac_param_count(const dril_sac_handle* h) { return h ? h->P : 0; }
DRIL_EXPORT int64_t dril_sac_q_param_count(const dril_sac_handle* h) { return h ? h->Pq : 0; }

DRIL_EXPORT int32_t dril_sac_set_params(dril_sac_handle* h, const float* flat, size_t n) {
    SNEED(h); if (!flat || n != (size_t)h->P) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_set_params: n must equal dril_sac_param_count");
    SDO(params_to_device(h, h->params, flat)); h->col_w2_dirty = true;
    SHIP(h, hipMemcpy(h->target, h->params + h->q0.w1, 2 * (size_t)h->Pqd * 4, hipMemcpyDeviceToDevice));   // copy_critic_parameters sac.jl:172,191-197
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_get_params(dril_sac_handle* h, float* flat, size_t n) {
    SNEED(h); if (!flat || n != (size_t)h->P) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_get_params: n must equal dril_sac_param_count");
    return params_from_device(h, flat, h->params);
}
DRIL_EXPORT int32_t dril_sac_get_target_params(dril_sac_handle* h, float* flat, size_t n) {
    SNEED(h); if (!flat || n != 2 * (size_t)h->Pq) return sfail(h, DRIL_ERR_INVALID_ARG, "target parameters: n must equal 2 * dril_sac_q_param_count");
    SDO(ssync(h));
    for (int k = 0; k < 2; ++k) SHIP(h, hipMemcpy(flat + (size_t)k * h->Pq, h->target + (size_t)k * h->Pqd, (size_t)h->Pq * 4, hipMemcpyDeviceToHost));
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_set_target_params(dril_sac_handle* h, const float* flat, size_t n) {
    SNEED(h); if (!flat || n != 2 * (size_t)h->Pq) return sfail(h, DRIL_ERR_INVALID_ARG, "target parameters: n must equal 2 * dril_sac_q_param_count");
    SDO(ssync(h));
    for (int k = 0; k < 2; ++k) SHIP(h, hipMemcpy(h->target + (size_t)k * h->Pqd, flat + (size_t)k * h->Pq, (size_t)h->Pq * 4, hipMemcpyHostToDevice));
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_get_log_ent_coef(dril_sac_handle* h, float* v) {
    SNEED(h); if (!v) return sfail(h, DRIL_ERR_INVALID_ARG, "null out pointer");
    SDO(ssync(h)); SacScalars sc; SHIP(h, hipMemcpy(&sc, h->sc, sizeof(sc), hipMemcpyDeviceToHost)); *v = sc.log_ent; return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_set_log_ent_coef(dril_sac_handle* h, float v) {
    SNEED(h); SDO(ssync(h)); SacScalars sc; SHIP(h, hipMemcpy(&sc, h->sc, sizeof(sc), hipMemcpyDeviceToHost));
    sc.log_ent = v; sc.alpha = expf(v); SHIP(h, hipMemcpy(h->sc, &sc, sizeof(sc), hipMemcpyHostToDevice)); return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_reset_optimizer(dril_sac_handle* h) {
    SNEED(h); SDO(ssync(h));
    SHIP(h, hipMemset(h->adam_m, 0, (size_t)h->Pd * 4)); SHIP(h, hipMemset(h->adam_v, 0, (size_t)h->Pd * 4));
    SacScalars sc; SHIP(h, hipMemcpy(&sc, h->sc, sizeof(sc), hipMemcpyDeviceToHost)); sc.ent_m = sc.ent_v = 0.f;
    SHIP(h, hipMemcpy(h->sc, &sc, sizeof(sc), hipMemcpyHostToDevice));
    reset_optimizer(h); return DRIL_OK;
}

DRIL_EXPORT int32_t dril_sac_env_reset(dril_sac_handle* h, uint64_t seed) {
    SNEED(h); S_NOT_EXTERNAL(h, "dril_sac_env_reset");
    h->env.seed0 = seed;
    SHIP(h, h->env.reset(h->stream));
    if (h->mon_window) { SHIP(h, hipMemsetAsync(h->mon_cur_ret, 0, (size_t)h->cfg.n_envs * 4, h->stream)); SHIP(h, hipMemsetAsync(h->mon_cur_len, 0, (size_t)h->cfg.n_envs * 4, h->stream)); }   // MonitorWrapperEnv.reset!: the running sums restart, the window stays (monitorWrapperEnv.jl:36-42)
    h->env.ready = true; h->obs_valid = false;
    if (h->nz.on) {                                                                   // NormalizeWrapperEnv.reset! (:110-121): old_obs = the raw observation, returns = 0, the statistics stay
        SHIP(h, hipMemsetAsync(h->nz_returns, 0, (size_t)h->cfg.n_envs * 4, h->stream));
        h->nz_raw_valid = false; SDO(nz_ensure_raw(h));
    }
    return ssync(h);
}
DRIL_EXPORT int32_t dril_sac_env_observe(dril_sac_handle* h, float* host_obs) {
    SNEED(h); S_NOT_EXTERNAL(h, "dril_sac_env_observe"); if (!host_obs) return sfail(h, DRIL_ERR_INVALID_ARG, "null observation buffer");
    const float* src = h->obs_cur;
    if (h->nz.on) { if (!h->obs_valid) { SDO(nz_observe(h, false, h->obs_nxt)); src = h->obs_nxt; } }   // a peek: what the actor will see under the statistics in force; nothing is updated
    else SDO(ensure_obs(h));
    SDO(ssync(h));
    SHIP(h, hipMemcpy(host_obs, src, (size_t)h->cfg.n_envs * h->D * 4, hipMemcpyDeviceToHost));
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_sac_action_log_prob(dril_sac_handle* h, const float* obs, int64_t batch, const float* noise, float* actions, float* logp) {
    SNEED(h); if (!obs || batch <= 0) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_action_log_prob: obs / batch");
    for (int64_t o = 0; o < batch; o += h->nmax) {
        const int n = (int)std::min<int64_t>(h->nmax, batch - o);
        SDO(actor_chunk(h, obs + o * h->D, noise ? noise + o * h->A : nullptr, n, 0, o));
        hipLaunchKernelGGL(sac_squash_eval_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, h->A, h->mu, h->params + h->log_std_off, h->s_noise, 0,
                           h->act_bounds, h->act_bounds + kMaxA, h->s_out, h->s_out2, (float*)nullptr);
        SDO(ssync(h));
        if (actions) SHIP(h, hipMemcpy(actions + o * h->A, h->s_out, (size_t)n * h->A * 4, hipMemcpyDeviceToHost));
        if (logp) SHIP(h, hipMemcpy(logp + o, h->s_out2, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_predict_actions(dril_sac_handle* h, const float* obs, int64_t batch, int32_t deterministic, const float* noise, float* raw, float* env) {
    SNEED(h); if (!obs || batch <= 0) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_predict_actions: obs / batch");
    for (int64_t o = 0; o < batch; o += h->nmax) {
        const int n = (int)std::min<int64_t>(h->nmax, batch - o);
        SDO(actor_chunk(h, obs + o * h->D, noise ? noise + o * h->A : nullptr, n, deterministic, o));
        hipLaunchKernelGGL(sac_squash_eval_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, h->A, h->mu, h->params + h->log_std_off, h->s_noise, deterministic,
                           h->act_bounds, h->act_bounds + kMaxA, h->s_out, (float*)nullptr, h->s_out2);
        SDO(ssync(h));
        if (raw) SHIP(h, hipMemcpy(raw + o * h->A, h->s_out, (size_t)n * h->A * 4, hipMemcpyDeviceToHost));
        if (env) SHIP(h, hipMemcpy(env + o * h->A, h->s_out2, (size_t)n * h->A * 4, hipMemcpyDeviceToHost));
    }
    return DRIL_OK;
}
// extract_policy(agent) / extract_policy(agent, norm_env) of a SAC agent on the device (include/dril_policy.h): actor, log_std, the TanhScaleAdapter's bounds and — with_norm —
// the wrapper's observation statistics, copied device-to-device into a policy object of its own.  Reads the handle, changes nothing in it.
DRIL_EXPORT int32_t dril_policy_from_sac_handle(dril_sac_handle* h, int32_t with_norm, dril_policy** out) {
    if (!h) { policy_set_create_error("dril_policy_from_sac_handle: null handle"); return DRIL_ERR_NOT_INITIALISED; }
    SNEED(h);
    auto refuse = [&](int code, const std::string& m) { policy_set_create_error(m); return sfail(h, code, m); };
    if (!out) return refuse(DRIL_ERR_INVALID_ARG, "dril_policy_from_sac_handle: null out pointer");
    *out = nullptr;
    PolicyDeviceSource s{}; dril_policy_desc& d = s.desc;
    d.abi_version = DRIL_POLICY_ABI_VERSION; d.kind = DRIL_POLICY_SQUASHED_DIAG_GAUSSIAN; d.obs_dim = h->D; d.action_dim = h->A;
    d.n_hidden = 2; d.hidden[0] = h->H1; d.hidden[1] = h->H2; d.activation = h->cfg.activation ? 1 : 0; d.device = h->cfg.device;
    float tb[2 * kMaxA];                                                               // the table the sampling kernels read: written once, at creation
    SHIP(h, hipMemcpy(tb, h->act_bounds, sizeof(tb), hipMemcpyDeviceToHost));
    for (int a = 0; a < h->A; ++a) { d.action_low[a] = tb[a]; d.action_high[a] = tb[kMaxA + a]; }
    if (with_norm) {
        if (!h->nz.on) return refuse(DRIL_ERR_NOT_INITIALISED, "dril_policy_from_sac_handle: with_norm = 1, but the handle has no NormalizeWrapperEnv (dril_sac_normalize_enable; a DRIL_ENV_EXTERNAL handle: dril_sac_ext_normalize_enable)");
        d.has_norm = 1; d.clip_obs = h->nz.cfg.clip_obs; d.epsilon = h->nz.cfg.epsilon;
        s.obs_mean = h->nz.half(h->nz.cur); s.obs_var = s.obs_mean + h->D;
    }
    s.actor = h->params + h->actor.w1; s.n = (size_t)h->Pa; s.log_std = h->params + h->log_std_off; s.stream = h->stream;
    std::string msg;
    const int rc = policy_from_device(s, out, &msg);
    return rc ? sfail(h, rc, "dril_policy_from_sac_handle: " + msg) : DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_predict_q(dril_sac_handle* h, const float* obs, const float* actions, int64_t batch, int32_t use_target, float* q) {
    SNEED(h); if (!obs || !actions || !q || batch <= 0) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_predict_q: null pointer / empty batch");
    const int W = h->D + h->A;
    std::vector<float> tmp(2 * (size_t)h->nq);
    for (int64_t o = 0; o < batch; o += h->nq) {
        const int n = (int)std::min<int64_t>(h->nq, batch - o);
        SHIP(h, hipMemcpyAsync(h->s_in, obs + o * h->D, (size_t)n * h->D * 4, hipMemcpyHostToDevice, h->stream));
        SHIP(h, hipMemcpyAsync(h->s_act, actions + o * h->A, (size_t)n * h->A * 4, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(sac_concat_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, h->D, h->A, h->s_in, h->s_act, h->xq_next);
        if (use_target) SDO(net_forward(h, h->target, net_off(0, W, h->H1, h->H2, 1), h->Pqd, W, 1, h->xq_next, W, 0, n, q_bufs(h, h->th1, h->th2, h->q_next), 2));
        else SDO(net_forward(h, h->params, h->q0, h->Pqd, W, 1, h->xq_next, W, 0, n, q_bufs(h, h->th1, h->th2, h->q_next), 2));
        SDO(ssync(h));
        SHIP(h, hipMemcpy(tmp.data(), h->q_next, tmp.size() * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) { q[(o + i) * 2] = tmp[i]; q[(o + i) * 2 + 1] = tmp[(size_t)h->nq + i]; }       // vcat of the critics: (2 x B)
    }
    return DRIL_OK;
}

DRIL_EXPORT int64_t dril_sac_replay_size(const dril_sac_handle* h) { return h ? h->size : 0; }
DRIL_EXPORT int64_t dril_sac_replay_capacity(const dril_sac_handle* h) { return h ? h->cap : 0; }
DRIL_EXPORT int32_t dril_sac_replay_copy_out(dril_sac_handle* h, int32_t which, void* host, size_t bytes) {
    SNEED(h);
    size_t w; const char* src;
    switch (which) {
        case DRIL_RB_OBSERVATIONS: w = (size_t)h->D * 4; src = (const char*)h->rb_obs.get(); break;
        case DRIL_RB_NEXT_OBSERVATIONS: w = (size_t)h->D * 4; src = (const char*)h->rb_next.get(); break;
        case DRIL_RB_ACTIONS: w = (size_t)h->A * 4; src = (const char*)h->rb_act.get(); break;
        case DRIL_RB_REWARDS: w = 4; src = (const char*)h->rb_rew.get(); break;
        case DRIL_RB_TERMINATED: w = 1; src = (const char*)h->rb_term.get(); break;
        case DRIL_RB_TRUNCATED: w = 1; src = (const char*)h->rb_trunc.get(); break;
        default: return sfail(h, DRIL_ERR_INVALID_ARG, "unknown replay field");
    }
    if (!host || bytes != w * (size_t)h->size) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_replay_copy_out: bytes must equal replay_size * element size");
    SDO(ssync(h));
    const long long first = std::min(h->size, h->cap - h->head);                                  // logical 0.. = [head, cap) then [0, ...)
    if (first > 0) SHIP(h, hipMemcpy(host, src + (size_t)h->head * w, (size_t)first * w, hipMemcpyDeviceToHost));
    if (h->size > first) SHIP(h, hipMemcpy((char*)host + (size_t)first * w, src, (size_t)(h->size - first) * w, hipMemcpyDeviceToHost));
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_replay_fill(dril_sac_handle* h, int64_t count, const float* obs, const float* actions, const float* rewards,
                                         const uint8_t* terminated, const uint8_t* truncated, const float* next_obs) {
    SNEED(h); if (count <= 0 || !obs || !actions || !rewards || !terminated || !next_obs) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_replay_fill: null pointer / empty");
    SDO(ssync(h));
    const int64_t skip = count > h->cap ? count - h->cap : 0, n = count - skip;                   // pushes beyond the capacity overwrite the oldest
    SHIP(h, hipMemcpy(h->rb_obs, obs + skip * h->D, (size_t)n * h->D * 4, hipMemcpyHostToDevice));
    SHIP(h, hipMemcpy(h->rb_next, next_obs + skip * h->D, (size_t)n * h->D * 4, hipMemcpyHostToDevice));
    SHIP(h, hipMemcpy(h->rb_act, actions + skip * h->A, (size_t)n * h->A * 4, hipMemcpyHostToDevice));
    SHIP(h, hipMemcpy(h->rb_rew, rewards + skip, (size_t)n * 4, hipMemcpyHostToDevice));
    SHIP(h, hipMemcpy(h->rb_term, terminated + skip, (size_t)n, hipMemcpyHostToDevice));
    if (truncated) SHIP(h, hipMemcpy(h->rb_trunc, truncated + skip, (size_t)n, hipMemcpyHostToDevice)); else SHIP(h, hipMemset(h->rb_trunc, 0, (size_t)n));
    h->head = 0; h->size = n;
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_sac_train(dril_sac_handle* h, int64_t max_steps, dril_sac_stats* stats, int64_t stats_capacity, int64_t* n_updates_done,
                                   double* fps, int64_t fps_capacity, int32_t* iterations_done, int64_t* total_steps) {
    SNEED(h); S_NOT_EXTERNAL(h, "dril_sac_train");
    const int64_t E = h->cfg.n_envs, tf = h->cfg.train_freq;
    const int64_t total_start = h->cfg.start_steps > 0 ? h->cfg.start_steps : tf * E;            // sac.jl:436
    const int64_t adjusted = std::max<int64_t>(1, total_start / E) * E;                           // :437
    int64_t n_steps = adjusted / E;                                                               // :438
    const int64_t iterations = (max_steps - adjusted) / (tf * E) + 1;                             // :443 (div truncates toward zero, as in Julia)
    const int64_t total = n_steps * E + tf * E * (iterations - 1);                                // :445
    const int64_t n_upd = h->cfg.gradient_steps == -1 ? tf * E : h->cfg.gradient_steps;           // get_gradient_steps :59-65
    int64_t done = 0; int64_t it = 0;
    if (iterations > 0) {                                                                         // the first iteration: the start_steps collection (random actions), then its gradient steps
        double f = 0;
        SDO(collect(h, (int)n_steps, h->cfg.start_steps > 0, &f));                                // :485-489
        if (fps && fps_capacity > 0) fps[0] = f;
        if (n_upd > 0) {
            const int64_t room = stats ? std::max<int64_t>(0, std::min<int64_t>(n_upd, stats_capacity)) : 0;
            std::vector<dril_sac_stats> tmp((size_t)n_upd);
            SDO(run_updates(h, (int)n_upd, false, tmp.data()));                                   // :514-531
            for (int64_t k = 0; k < room; ++k) stats[k] = tmp[(size_t)k];
            done += n_upd;
        }
        it = 1;
    }
    while (it < iterations) {                                                                     // every later iteration collects train_freq steps (:511): chunks without a host sync inside
        const int cnt = (int)std::min<int64_t>(std::min<int64_t>(h->iter_chunk, std::max<int64_t>(1, 4096 / std::max<int64_t>(1, n_upd))), iterations - it);   // at most 4 096 statistics rows per drain (gradient_steps = -1 means train_freq x n_envs updates per iteration)
        SDO(run_iterations(h, cnt, (int)tf, (int)n_upd, stats ? stats + std::min<int64_t>(done, stats_capacity) : nullptr, stats ? std::max<int64_t>(0, stats_capacity - done) : 0,
                           fps && it < fps_capacity ? fps + it : nullptr, fps ? std::max<int64_t>(0, fps_capacity - it) : 0));
        done += (int64_t)cnt * n_upd; it += cnt;
    }
    if (n_updates_done) *n_updates_done = done;
    if (iterations_done) *iterations_done = (int32_t)std::max<int64_t>(0, it);
    if (total_steps) *total_steps = it > 0 ? total : 0;
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_sac_iterate(dril_sac_handle* h, int32_t iterations, dril_sac_stats* stats, int64_t stats_capacity, double* fps, int64_t fps_capacity) {
    SNEED(h); S_NOT_EXTERNAL(h, "dril_sac_iterate");
    if (iterations <= 0) return sfail(h, DRIL_ERR_INVALID_ARG, "iterations must be positive");
    if (!h->env.ready) return sfail(h, DRIL_ERR_NOT_INITIALISED, "dril_sac_env_reset has not been called");
    const int64_t E = h->cfg.n_envs, tf = h->cfg.train_freq;
    const int64_t n_upd = h->cfg.gradient_steps == -1 ? tf * E : h->cfg.gradient_steps;
    int64_t done = 0;
    for (int64_t it = 0; it < iterations; ) {
        const int cnt = (int)std::min<int64_t>(std::min<int64_t>(h->iter_chunk, std::max<int64_t>(1, 4096 / std::max<int64_t>(1, n_upd))), iterations - it);   // at most 4 096 statistics rows per drain (gradient_steps = -1 means train_freq x n_envs updates per iteration)
        SDO(run_iterations(h, cnt, (int)tf, (int)n_upd, stats ? stats + std::min<int64_t>(done, stats_capacity) : nullptr, stats ? std::max<int64_t>(0, stats_capacity - done) : 0,
                           fps && it < fps_capacity ? fps + it : nullptr, fps ? std::max<int64_t>(0, fps_capacity - it) : 0));
        done += (int64_t)cnt * n_upd; it += cnt;
    }
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_profile_get(dril_sac_handle* h, double* collect_ms, int64_t* collect_steps, double* update_ms, int64_t* updates) {
    SNEED(h);
    if (collect_ms) *collect_ms = h->collect_ms; if (collect_steps) *collect_steps = h->collect_steps;
    if (update_ms) *update_ms = h->update_ms; if (updates) *updates = h->updates;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_profile_reset(dril_sac_handle* h) { SNEED(h); h->collect_ms = h->update_ms = 0; h->collect_steps = h->updates = 0; return DRIL_OK; }
