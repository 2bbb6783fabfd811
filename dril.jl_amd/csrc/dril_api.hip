// dril_api.hip — the C ABI of libdril_hip.so (include/dril_hip.h): handle, device memory, launch sequencing.
// One HIP stream per handle; kernels of one PPO iteration are enqueued back-to-back with no host sync
// (KL early-stop and NaN detection are device flags the later kernels test), RCCL all-reduces ride the
// same stream.  The handle itself, and what this file shares with dril_comm.hip (RCCL) and dril_wrap.hip (NormalizeWrapperEnv on plug-in and external handles): dril_handle.h.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dril_handle.h"

#include "dril_policy_internal.h"   // dril_policy_from_handle: the snapshot this handle gives a deployment policy (dril_policy.hip)
#include "dril_traj_record.h"  // collect_trajectory on the device: the per-env recording traj_record_kernel runs (host-compilable)
#include "dril_traj_run.h"    // ... and its setup (blob layout, table of bounds, shadow envs, messages), shared with the SAC handle
#include "dril_ext_stream.h"  // the pointer rule and the stream hand-over of the device-array verbs, shared with the SAC handle

using namespace dril;
using namespace dril::ppo;

namespace {

// cfg.profile_events = k >= 1: the per-iteration classes (rollout, GAE, pack, moments, explained variance) are bracketed at every launch; the classes launched once per
// OPTIMISER STEP (gradient, reduce, Adam, all-reduce) at every k-th launch — a hipEventRecord costs the stream ~3.5 us and an iteration of configs[1] holds 960 such launches
// (measured round 4, same box: 350.4 / 346.9 ms with all of them bracketed, 343.7 / 343.3 with none / every 8th; hipEventDisableSystemFence changes nothing)
bool prof_per_step(int kid) { return kid == DRIL_K_PPO_GRAD || kid == DRIL_K_GRAD_REDUCE || kid == DRIL_K_ADAM || kid == DRIL_K_ALLREDUCE; }
void prof_resolve(dril_handle* h) {   // stream must be drained
    for (auto& p : h->prof_pending) {
        float ms = 0; if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { h->prof_ms[p.kid] += ms; h->prof_n[p.kid] += 1; }
        h->prof_pool.push_back({p.a, p.b});
    }
    h->prof_pending.clear();
}

// wide nets: (re)build the pre-tiled W2 / W2' images after every parameter change (enqueued on the handle's stream)
int ensure_wimg(dril_handle* h) {
    if (!h->wide || !h->wimg_dirty) return DRIL_OK;
    HIPCHK(h, launch_build_wimg(h->params, h->actor, h->cfg.hidden1, h->w2a_actor, h->w2ta_actor, h->stream));
    HIPCHK(h, launch_build_wimg(h->params, h->critic, h->cfg.hidden1, h->w2a_critic, h->w2ta_critic, h->stream));
    {                                             // the pre-split f16 fragment streams: ppo_grad_wide_split_kernel, and the forward of rollout / policy kernels
        HIPCHK(h, launch_build_wimg_split(h->params, h->actor, h->cfg.hidden1, h->w2p_actor, h->w2tp_actor, h->w2pf_actor, h->stream));
        HIPCHK(h, launch_build_wimg_split(h->params, h->critic, h->cfg.hidden1, h->w2p_critic, h->w2tp_critic, h->w2pf_critic, h->stream));
    }
    h->wimg_dirty = false;
    return DRIL_OK;
}

// ---- MonitorWrapperEnv helpers ----
MonitorArgs monitor_step_args(dril_handle* h) {   // one env step: finished episodes land in the E-sized step arrays
    MonitorArgs m{}; if (h->mon_cur_ret) { m.cur_ret = h->mon_cur_ret; m.cur_len = h->mon_cur_len; m.ep_ret = h->e_ep_ret; m.ep_len = h->e_ep_len; m.flags_out = h->e_flags; }
    return m;
}
int monitor_collect_step(dril_handle* h) {
    if (!h->mon_cur_ret) return DRIL_OK;
    HIPCHK(h, launch_monitor_collect(h->e_flags, h->e_ep_ret, h->e_ep_len, h->cfg.n_envs, 1, h->cfg.monitor_window, h->mon_cnt, h->mon_ring_ret, h->mon_ring_len, h->mon_meta, h->stream));
    return DRIL_OK;
}
}  // namespace

namespace dril::ppo {
// ---- what dril_comm.hip and dril_wrap.hip call (dril_handle.h) ----
thread_local std::string g_create_error;

void prof_begin(dril_handle* h, int kid) {
    h->prof_open = false;
    if (!h->cfg.profile_events) return;
    const int64_t i = h->prof_all[kid]++;
    if (prof_per_step(kid) && h->cfg.profile_events > 1 && i % h->cfg.profile_events) return;
    std::pair<hipEvent_t, hipEvent_t> ev;
    if (!h->prof_pool.empty()) { ev = h->prof_pool.back(); h->prof_pool.pop_back(); }
    else { hipEventCreate(&ev.first); hipEventCreate(&ev.second); }
    hipEventRecord(ev.first, h->stream);
    h->prof_pending.push_back({kid, ev.first, ev.second});
    h->prof_open = true;
}
void prof_end(dril_handle* h) {
    if (!h->prof_open) return;
    hipEventRecord(h->prof_pending.back().b, h->stream);
    h->prof_open = false;
}
int sync(dril_handle* h) { HIPCHK(h, hipStreamSynchronize(h->stream)); prof_resolve(h); return DRIL_OK; }

// fused per-kind kernels for the device envs, the layer-by-layer generic path for DRIL_ENV_EXTERNAL
hipError_t run_policy(dril_handle* h, const PolicyArgs& a) {
    if (!h->generic) return launch_policy(h->cfg.env_kind, h->cfg.hidden1, a, 8 * h->num_cus, h->stream);
    if (a.boot_where) {                       // V(terminal_observation) of the previous env step (fused into policy_kernel on the fused path): critic over all rows, kept where truncated
        PolicyArgs b = a; b.obs = a.boot_obs; b.noise = nullptr; b.actions = nullptr; b.values = h->gen_tmp; b.logp = nullptr; b.entropy = nullptr; b.mode = 2;
        b.obs_out = nullptr; b.boot_obs = nullptr; b.boot_where = nullptr; b.boot_out = nullptr; b.gstep = nullptr;
        hipError_t e = generic_policy(h->gd, b, h->gws, h->stream); if (e != hipSuccess) return e;
        e = generic_select(a.B, a.boot_where, h->gen_tmp, a.boot_out, h->stream); if (e != hipSuccess) return e;
        h->gws.launches += 1;
    }
    PolicyArgs q = a; q.boot_obs = nullptr; q.boot_where = nullptr; q.boot_out = nullptr;
    return generic_policy(h->gd, q, h->gws, h->stream);
}

PolicyArgs policy_args(dril_handle* h, const float* obs, int64_t B, const void* noise, void* actions, float* values, float* logp,
                       float* entropy, int mode) {
    PolicyArgs a{};
    a.params = h->params; a.obs = obs; a.B = B; a.noise = noise; a.actions = actions; a.values = values; a.logp = logp; a.entropy = entropy;
    a.mode = mode; a.action_start = h->cfg.action_start; a.log_std_off = h->log_std_off; a.seed = h->cfg.seed; a.call_counter = h->policy_calls;
    a.actor = h->actor; a.critic = h->critic;
    a.exact_f32 = fwd_exact(h) ? 1 : 0;
    a.w2a_actor = a.exact_f32 ? h->w2a_actor : (const float*)h->w2pf_actor.get(); a.w2a_critic = a.exact_f32 ? h->w2a_critic : (const float*)h->w2pf_critic.get();   // wide nets: W2 operand of the forward
    return a;
}

MonitorArgs monitor_rollout_args(dril_handle* h, size_t k) {   // row k / E of a step-granular rollout over a plug-in: the BUF_FLAGS byte always, finished episodes with the monitor on
    MonitorArgs m{}; m.flags_out = h->flags + k; if (h->mon_cur_ret) { m.cur_ret = h->mon_cur_ret; m.cur_len = h->mon_cur_len; m.ep_ret = h->ep_ret + k; m.ep_len = h->ep_len + k; }
    return m;
}
int monitor_collect_rollout(dril_handle* h) {
    if (!h->mon_cur_ret) return DRIL_OK;
    HIPCHK(h, launch_monitor_collect(h->flags, h->ep_ret, h->ep_len, h->cfg.n_envs, h->cfg.n_steps, h->cfg.monitor_window, h->mon_cnt, h->mon_ring_ret, h->mon_ring_len, h->mon_meta, h->stream));
    return DRIL_OK;
}

// act!(env, actions) through the E-sized per-step arrays (dril_env_step, dril_evaluate_agent, the step-granular verbs), and MonitorWrapperEnv's window after it
int env_step_arrays(dril_handle* h, const void* actions) {
    HIPCHK(h, h->env.step(actions, EnvStepOut{h->e_rew, h->e_term, h->e_trunc, h->e_tobs, nullptr}, monitor_step_args(h), h->stream));
    return monitor_collect_step(h);
}
}  // namespace dril::ppo

namespace {
// data-parallel runs: NormalizeWrapperEnv's batch moments cover every env of the job (the reference has ONE vector env, normalizeWrapperEnv.jl:21-26):
// this rank's partial table is folded to one row, RCCL sums the rows, and the apply kernels merge that row with n_stats = world * E.  One 128-byte
// all-reduce per env step; every rank applies the identical update, so the running statistics stay bit-identical across ranks
int global_partials(dril_handle* h, bool update, const double*& partials, int& nb, long long& n_stats) {
    partials = h->rms_partials; n_stats = 0;
    const int world = comm_ready(h) ? h->cfg.world_size : 1;
    if (!update || !(world > 1 || (comm_ready(h) && h->force_allreduce))) return DRIL_OK;
    HIPCHK(h, launch_fold_partials(h->rms_partials, nb, h->rms_red, h->stream));
    int rc = rccl_allreduce(h, h->rms_red, 16, kNcclFloat64); if (rc) return rc;
    partials = h->rms_red; nb = 1; n_stats = (long long)h->cfg.n_envs * world;
    return DRIL_OK;
}

// ---- step-granular env verbs on device (NormalizeWrapperEnv.observe / act!, normalizeWrapperEnv.jl:123-165) ----
int observe_dev(dril_handle* h, bool update_stats) {
    const int E = h->cfg.n_envs;
    if (h->env.module && h->pn.on) return pn_observe(h, update_stats);                 // a plug-in env under dril_normalize_enable
    if (h->env.module) { HIPCHK(h, h->env.observe(h->e_obs, h->stream)); return DRIL_OK; }   // a plug-in env without the wrapper: the observation as it is
    int nb = (E + 255) / 256; if (nb > h->rms_blocks) nb = h->rms_blocks;
    HIPCHK(h, launch_obs_partials(h->env.kind, E, h->env.state, h->e_obs_raw, h->rms_partials, nb, h->stream));
    NormObsArgs a{};
    a.E = E; a.D = h->D; a.update = (update_stats && h->cfg.norm_training && h->cfg.norm_obs) ? 1 : 0;
    { int rcg = global_partials(h, a.update != 0, a.partials, nb, a.n_stats); if (rcg) return rcg; }
    a.nblocks = nb;
    a.raw = h->e_obs_raw; a.in = h->obs_rms + h->obs_par; a.out = h->obs_rms + (h->obs_par ^ 1);
    a.obs_n = h->e_obs; a.clip = h->cfg.clip_obs; a.eps = h->cfg.norm_epsilon; a.norm_obs = h->cfg.norm_obs;
    HIPCHK(h, launch_norm_obs_apply(a, h->stream));
    h->obs_par ^= 1;
    return DRIL_OK;
}
// actions: device pointer (stored/raw policy actions; the kernels apply the adapters); rew_out/flags_out: device destinations
int step_dev(dril_handle* h, const void* actions, float* rew_out, uint8_t* flags_out) {
    const int E = h->cfg.n_envs;
    if (h->env.module && h->pn.on) return pn_step(h, actions, rew_out ? rew_out : h->e_rew_n);
    { int rcs = env_step_arrays(h, actions); if (rcs) return rcs; }
    if (h->env.module) {                                                               // plug-in env without the wrapper: the raw step is the whole step
        if (rew_out && rew_out != h->e_rew) HIPCHK(h, hipMemcpyAsync(rew_out, h->e_rew, (size_t)E * 4, hipMemcpyDeviceToDevice, h->stream));
        return DRIL_OK;
    }
    int nb = (E + 255) / 256; if (nb > h->rms_blocks) nb = h->rms_blocks;
    const int upd = (h->cfg.norm_reward && h->cfg.norm_training) ? 1 : 0;
    HIPCHK(h, launch_rew_partials(E, h->e_rew, h->env.disc_returns, h->cfg.norm_gamma, upd, h->rms_partials, nb, h->stream));
    NormRewArgs a{};
    a.E = E; a.D = h->D; a.update = upd; a.norm_obs = h->cfg.norm_obs; a.norm_reward = h->cfg.norm_reward;
    { int rcg = global_partials(h, upd != 0, a.partials, nb, a.n_stats); if (rcg) return rcg; }
    a.nblocks = nb;
    a.rew_raw = h->e_rew; a.in = h->ret_rms + h->ret_par; a.out = h->ret_rms + (h->ret_par ^ 1);
    a.obs_stats = h->obs_rms + h->obs_par; a.rew_out = rew_out; a.disc_returns = h->env.disc_returns; a.term = h->e_term; a.trunc = h->e_trunc;
    a.tobs = h->e_tobs; a.clip_obs = h->cfg.clip_obs; a.clip_reward = h->cfg.clip_reward; a.eps = h->cfg.norm_epsilon; a.flags_out = flags_out;
    HIPCHK(h, launch_norm_rew_apply(a, h->stream));
    h->ret_par ^= 1;
    return DRIL_OK;
}

// one optimiser step on [pos0, pos0+count) of the current epoch order; all launches asynchronous
int ppo_step(dril_handle* h, const float* obs, const void* actions, const float* adv, const float* ret, const float* logp_old,
             const float* val_old, const int64_t* perm, int64_t pos0, int64_t count, int64_t N, uint64_t key, int bits,
             float* step_stats, bool apply, const float4* rec = nullptr, const double* pre_stats = nullptr, const int32_t* perm32 = nullptr) {
    const int world = comm_ready(h) ? h->cfg.world_size : 1;
    const bool reduce = world > 1 || (comm_ready(h) && h->force_allreduce);   // force: exercise the RCCL path on one rank (tests)
    const int64_t tiles = (count + kTile - 1) / kTile;
    int G = h->wide ? (int)(tiles < h->Gmax ? tiles : h->Gmax) : (int)((tiles + 3) / 4); if (G > h->Gmax) G = h->Gmax; if (G < 1) G = 1;
    // hidden [64,64]: large minibatches run ppo_grad_pair_kernel (bf16 matrix cores, two waves per tile, two workgroups of two pairs per CU); small ones keep
    // the f32 kernel, whose weight staging is cheaper (no operand split per workgroup) and which the launch-bound small path is tuned for
    int variant = 0;
    if (h->wide) variant = (wide_variant(h) && rec) ? 1 : 0;
    if (h->wide && variant == 1) { const int64_t passes = (tiles + kWideSplitNT - 1) / kWideSplitNT; G = (int)(passes < h->Gmax ? passes : h->Gmax); if (G < 1) G = 1; }   // ppo_grad_wide_split_kernel takes kWideSplitNT sample tiles per pass
    if (!h->wide && !h->generic) {
        variant = h->grad_variant == 0 ? 0 : h->grad_variant > 0 ? 2 : (tiles >= kPairTilesPerCu * (int64_t)h->num_cus ? 2 : 0);   // large minibatches: the pair kernel
        if (variant == 2 && !(pair_variant(h) && rec && h->Gmax >= 2)) variant = 0;   // the pair kernel reads packed records and needs two slabs per workgroup (DRIL_GRAD_GMAX=1: not the pair kernel)
        if (variant == 2) { G = (int)(tiles < h->Gmax ? tiles : h->Gmax) & ~1; if (G < 2) G = 2; }   // pairs per net (even: two pairs per workgroup)
        if (variant == 0 && G > h->num_cus) G = h->num_cus;                                   // Gmax is sized for the pair kernel's slabs; the f32 kernel runs two workgroups per CU
    }
    int Gc = G;
    if (variant == 2 && 2 * G >= 4 * h->num_cus) {     // pair kernel filling the chip (two workgroups of two pairs per CU): the pairs are divided between the nets by their cost per tile
        const int pml = h->grad_actor_pct ? h->grad_actor_pct : (h->discrete ? 500 : 450), total = 4 * h->num_cus;   // measured optima (re-swept on the f16 arithmetic at the end of round 3): the older (actor) workgroups win the issue arbitration on a shared SIMD
        int ga = ((total * pml + 500) / 1000) & ~1; if (ga < 2) ga = 2; if (ga > total - 2) ga = total - 2;
        G = ga; Gc = total - ga;
        if (G > h->Gmax) G = h->Gmax & ~1; if (Gc > h->Gmax) Gc = h->Gmax & ~1;
    }
    if (h->generic) { G = generic_pick_slabs(h->gd, count, h->Gmax); if (G < 1) return fail(h, DRIL_ERR_UNSUPPORTED, "minibatch too large for the generic path's workspace"); Gc = G; }
    { int rcw = ensure_wimg(h); if (rcw) return rcw; }
    h->last_variant = h->generic ? 3 : h->wide ? (variant ? 4 : 2) : (variant == 2 ? 5 : variant);
    if (h->last_variant == 4 || h->last_variant == 5) h->used_f16 = true;
    h->last_G = G; h->last_Gc = Gc;
    const double* adv_stats = h->adv_stats;
    // launch-bound regime (the reference's default batch_size = 64): the advantage moments are computed inside the grad kernel and
    // reduce + norm + Adam run as one workgroup: 2 dependent launches per optimiser step instead of 6
    const bool small = !reduce && !h->wide && !h->generic && count <= 4096 && !h->no_small_path && variant != 2;   // (the pair kernel has no in-kernel moments: forced onto a small minibatch it takes the general path)
    if (h->cfg.normalize_advantage && pre_stats) adv_stats = pre_stats;   // per-epoch table (already all-reduced in data-parallel runs)
    else if (h->cfg.normalize_advantage && small) adv_stats = nullptr;
    else if (h->cfg.normalize_advantage) {
        MomentsArgs m{}; m.adv = adv; m.perm = perm; m.perm32 = perm32; m.pos0 = pos0; m.count = count; m.N = N; m.idx_lo = 0; m.n_local = N;
        m.perm_key = key; m.perm_bits = bits; m.partials = h->adv_partials; m.stop_flag = h->stop_flag;
        int nb = (int)((count + 255) / 256); if (nb > h->adv_blocks) nb = h->adv_blocks; if (nb < 1) nb = 1;
        prof_begin(h, DRIL_K_ADV_MOMENTS);
        HIPCHK(h, launch_adv_moments(m, nb, h->stream));
        HIPCHK(h, launch_moments_finalize(h->adv_partials, nb, h->adv_stats, (double)count, h->stop_flag, h->stream));
        prof_end(h);
        if (reduce) { int rc = rccl_allreduce(h, h->adv_stats, 3, kNcclFloat64); if (rc) return rc; }
    }
    GradArgs g{};
    g.params = h->params; g.obs = obs; g.actions = actions; g.adv = adv; g.ret = ret; g.logp_old = logp_old; g.val_old = val_old;
    g.perm = perm; g.perm32 = perm32; g.pos0 = pos0; g.count = count; g.N = N; g.idx_lo = 0; g.n_local = N; g.perm_key = key; g.perm_bits = bits;
    g.w2p_actor = (const u32x4*)h->w2p_actor.get(); g.w2tp_actor = (const u32x4*)h->w2tp_actor.get(); g.w2p_critic = (const u32x4*)h->w2p_critic.get(); g.w2tp_critic = (const u32x4*)h->w2tp_critic.get();
    g.rec = rec; g.w2a_actor = h->w2a_actor; g.w2ta_actor = h->w2ta_actor; g.w2a_critic = h->w2a_critic; g.w2ta_critic = h->w2ta_critic;
    g.adv_stats = adv_stats; g.inline_moments = (h->cfg.normalize_advantage && adv_stats == nullptr) ? 1 : 0; g.invB = 1.0f / (float)(count * world);
    g.clip_range = h->cfg.clip_range; g.ent_coef = h->cfg.ent_coef; g.vf_coef = h->cfg.vf_coef; g.clip_range_vf = h->cfg.clip_range_vf;
    g.has_clip_vf = h->cfg.has_clip_range_vf; g.normalize_adv = h->cfg.normalize_advantage; g.action_start = h->cfg.action_start;
    g.log_std_off = h->log_std_off; g.slabs_actor = h->slabs_a; g.slabs_critic = h->slabs_c; g.slab_a = h->slab_a; g.slab_c = h->slab_c;
    g.G = G; g.Gc = Gc; g.dbg = h->dbg; g.variant = variant; g.stop_flag = h->stop_flag; g.actor = h->actor; g.critic = h->critic;
    // host-side preconditions of the gradient kernels: a violated one would be a device fault (null advantage moments in a kernel without in-kernel
    // moments — the SIGABRT of profiles/r02_split_kernel.md "the abort of 09:41" —, a slab index past the Gmax slabs that were allocated); only a status code
    // may cross the ABI
    const bool kernel_has_inline_moments = !h->wide && !h->generic && variant != 2;
    if (g.normalize_adv && !adv_stats && !kernel_has_inline_moments) return fail(h, DRIL_ERR_INVALID_ARG, "ppo_step: advantage moments missing for a gradient kernel without in-kernel moments");
    if (G < 1 || Gc < 1 || G > h->Gmax || Gc > h->Gmax || (variant == 2 && !h->wide && !h->generic && ((G | Gc) & 1))) return fail(h, DRIL_ERR_INVALID_ARG, "ppo_step: gradient grid does not fit the slab buffers");
    prof_begin(h, DRIL_K_PPO_GRAD);
    if (h->generic) HIPCHK(h, generic_ppo_grad(h->gd, g, h->gws, h->stream));
    else HIPCHK(h, launch_ppo_grad(h->cfg.env_kind, h->cfg.hidden1, g, h->stream));
    prof_end(h);
    ReduceArgs r{};
    r.slabs_actor = h->slabs_a; r.slabs_critic = h->slabs_c; r.slab_a = h->slab_a; r.slab_c = h->slab_c; r.G = G; r.Gc = Gc;
    if (h->last_variant == 5) { r.G = G / 2; r.Gc = Gc / 2; }                       // ppo_grad_pair_kernel: G / Gc count pairs, its workgroups (two pairs each) write one slab
    r.P = h->P; r.Pa = h->Pa; r.Pc = h->Pc; r.flat = h->flat; r.norm_partials = h->norm_partials; r.n_samples_local = (double)count;
    r.stop_flag = h->stop_flag;
    if (small && apply && h->P <= 16384 && G <= 32) {
        AdamArgs ad{};
        ad.params = h->params; ad.m = h->adam_m; ad.v = h->adam_v; ad.flat = h->flat; ad.P = h->P;
        ad.norm_partials = h->norm_partials; ad.n_partials = h->n_norm_partials; ad.bt = h->bt; ad.step_parity = (int)(h->adam_steps & 1);
        ad.beta1 = h->cfg.adam_beta1; ad.beta2 = h->cfg.adam_beta2; ad.eps = h->cfg.adam_eps; ad.lr = h->lr;
        ad.max_grad_norm = h->cfg.max_grad_norm; ad.target_kl = h->cfg.target_kl; ad.ent_coef = h->cfg.ent_coef; ad.vf_coef = h->cfg.vf_coef;
        ad.has_max_grad_norm = h->cfg.has_max_grad_norm; ad.has_target_kl = h->cfg.has_target_kl; ad.use_stats = 1;
        ad.step_stats = step_stats; ad.norm_out = h->norm_out; ad.nan_flag = h->nan_flag; ad.stop_flag = h->stop_flag; ad.stop_flag_w = h->stop_flag;
        prof_begin(h, DRIL_K_ADAM);
        HIPCHK(h, launch_finish_small(r, ad, h->stream));
        prof_end(h);
        h->adam_steps += 1; h->wimg_dirty = true;
        return DRIL_OK;
    }
    prof_begin(h, DRIL_K_GRAD_REDUCE);
    HIPCHK(h, launch_grad_reduce(r, h->stream));
    prof_end(h);
    const bool norm_in_adam = reduce && apply && h->P <= 65536;                        // data-parallel: adam_kernel sums |g|^2 from the all-reduced gradient itself (one launch less per step)
    if (reduce) {
        int rc = rccl_allreduce(h, h->flat, (size_t)h->P + 8, kNcclFloat32); if (rc) return rc;
        if (!norm_in_adam) HIPCHK(h, launch_grad_norm(h->flat, h->P, h->norm_partials, h->stop_flag, h->stream));
    }
    if (!apply) return DRIL_OK;
    AdamArgs ad{}; ad.norm_from_flat = norm_in_adam ? 1 : 0;
    ad.params = h->params; ad.m = h->adam_m; ad.v = h->adam_v; ad.flat = h->flat; ad.P = h->P;
    ad.norm_partials = h->norm_partials; ad.n_partials = h->n_norm_partials; ad.bt = h->bt; ad.step_parity = (int)(h->adam_steps & 1);
    ad.beta1 = h->cfg.adam_beta1; ad.beta2 = h->cfg.adam_beta2; ad.eps = h->cfg.adam_eps; ad.lr = h->lr;
    ad.max_grad_norm = h->cfg.max_grad_norm; ad.target_kl = h->cfg.target_kl; ad.ent_coef = h->cfg.ent_coef; ad.vf_coef = h->cfg.vf_coef;
    ad.has_max_grad_norm = h->cfg.has_max_grad_norm; ad.has_target_kl = h->cfg.has_target_kl; ad.use_stats = 1;
    ad.step_stats = step_stats; ad.norm_out = h->norm_out; ad.nan_flag = h->nan_flag; ad.stop_flag = h->stop_flag; ad.stop_flag_w = h->stop_flag;
    prof_begin(h, DRIL_K_ADAM);
    HIPCHK(h, launch_adam(ad, h->stream));
    prof_end(h);
    h->adam_steps += 1; h->wimg_dirty = true;
    return DRIL_OK;
}

uint64_t perm_key(uint64_t seed, uint64_t counter, int epoch) {
    uint32_t r[4];
    philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)counter, (uint32_t)(counter >> 32), 2, (uint32_t)epoch, r);
    return ((uint64_t)r[0] << 32) | r[1];
}

int reset_optimizer(dril_handle* h) {
    HIPCHK(h, hipMemsetAsync(h->adam_m, 0, sizeof(float) * h->P, h->stream));
    HIPCHK(h, hipMemsetAsync(h->adam_v, 0, sizeof(float) * h->P, h->stream));
    const float bt[4] = {h->cfg.adam_beta1, h->cfg.adam_beta2, h->cfg.adam_beta1, h->cfg.adam_beta2};
    HIPCHK(h, hipMemcpyAsync(h->bt, bt, sizeof(bt), hipMemcpyHostToDevice, h->stream));
    h->adam_steps = 0;
    return sync(h);
}

void* buf_ptr(dril_handle* h, int which, size_t* bytes) {
    const size_t N = (size_t)h->N;
    switch (which) {
    case DRIL_BUF_OBSERVATIONS: *bytes = N * h->D * 4; return h->obs;
    case DRIL_BUF_ACTIONS: *bytes = N * act_bytes_per(h); return h->act;
    case DRIL_BUF_REWARDS: *bytes = N * 4; return h->rew;
    case DRIL_BUF_ADVANTAGES: *bytes = N * 4; return h->adv;
    case DRIL_BUF_RETURNS: *bytes = N * 4; return h->ret;
    case DRIL_BUF_LOGPROBS: *bytes = N * 4; return h->logp;
    case DRIL_BUF_VALUES: *bytes = N * 4; return h->val;
    case DRIL_BUF_FLAGS: *bytes = N; return h->flags;
    case DRIL_BUF_BOOTSTRAP: *bytes = N * 4; return h->boot;
    case DRIL_BUF_LAST_VALUES: *bytes = (size_t)h->cfg.n_envs * 4; return h->last_values;
    }
    *bytes = 0; return nullptr;
}

}  // namespace

// ================================================================================================
DRIL_EXPORT int32_t dril_config_default(dril_config* c, int32_t env_kind) {
    if (!c || env_kind < DRIL_ENV_CARTPOLE || env_kind > DRIL_ENV_MODULE) return fail(nullptr, DRIL_ERR_INVALID_ARG, "bad cfg/env_kind");
    std::memset(c, 0, sizeof(*c));
    c->abi_version = DRIL_ABI_VERSION; c->env_kind = env_kind; c->n_envs = 4; c->n_steps = 2048; c->hidden1 = c->hidden2 = 64;
    const EnvKindInfo* k = env_kind_info(env_kind);
    c->episode_len = k ? k->default_episode_len /* the Gymnasium time limit */ : env_kind == DRIL_ENV_MODULE ? 0 /* the descriptor's */ : 200; c->action_start = 1;
    c->gamma = 0.99f; c->gae_lambda = 0.95f; c->clip_range = 0.2f; c->ent_coef = 0.0f; c->vf_coef = 0.5f;
    c->max_grad_norm = 0.5f; c->has_max_grad_norm = 1; c->normalize_advantage = 1; c->batch_size = 64; c->epochs = 10;
    c->learning_rate = 3.0e-4f; c->adam_beta1 = 0.9f; c->adam_beta2 = 0.999f; c->adam_eps = 1.0e-5f;
    c->clip_obs = c->clip_reward = 10.0f; c->norm_gamma = 0.99f; c->norm_epsilon = 1.0e-8f; c->seed = 42; c->world_size = 1;
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_env_module_describe(const char* code_object_path, int32_t device, dril_env_module_info* out) {
    if (!out) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_env_module_describe: null out");
    hipModule_t mod = nullptr; DrilEnvPluginDesc d{}; std::string msg;
    const int rc = load_env_module(code_object_path, device, &mod, &d, msg);
    if (rc) return fail(nullptr, rc, "dril_env_module_describe: " + msg);
    (void)hipModuleUnload(mod);
    fill_module_info(d, out);
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_env_module_info_of(const dril_handle* h, dril_env_module_info* out) {
    if (!h || !out) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle / out");
    if (!h->env.module) return fail(const_cast<dril_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_env_module_info_of: the handle was not created with dril_create_with_env_module");
    fill_module_info(h->env.desc, out);
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_env_module_obs_space(const char* code_object_path, int32_t device, float* low, float* high, int32_t* declared) {
    std::string msg; const int rc = describe_module_obs_space(code_object_path, device, low, high, declared, msg);
    return rc ? fail(nullptr, rc, "dril_env_module_obs_space: " + msg) : DRIL_OK;
}
DRIL_EXPORT int32_t dril_env_module_obs_space_of(const dril_handle* h, float* low, float* high, int32_t* declared) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!h->env.module) return fail(const_cast<dril_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_env_module_obs_space_of: the handle was not created with dril_create_with_env_module");
    const int D = h->env.desc.D;
    if (low) std::memcpy(low, h->env.obs_low.data(), (size_t)D * 4);
    if (high) std::memcpy(high, h->env.obs_high.data(), (size_t)D * 4);
    if (declared) *declared = h->env.obs_declared ? 1 : 0;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_env_module_agents(const char* code_object_path, int32_t device, int32_t* agents) {
    if (!agents) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_env_module_agents: null agents");
    hipModule_t mod = nullptr; DrilEnvPluginDesc d{}; std::string msg;
    const int rc = load_env_module(code_object_path, device, &mod, &d, msg);
    if (rc) return fail(nullptr, rc, "dril_env_module_agents: " + msg);
    (void)hipModuleUnload(mod);
    *agents = d.agents ? d.agents : 1;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_env_module_agents_of(const dril_handle* h, int32_t* agents) {
    if (!h || !agents) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle / agents");
    if (!h->env.module) return fail(const_cast<dril_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_env_module_agents_of: the handle was not created with dril_create_with_env_module");
    *agents = h->env.agents();
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_scaling_enable(dril_handle* h, int32_t on) {
    NEED(h);
    std::string msg; const int rc = h->env.set_scaling(on != 0, msg);
    return rc ? fail(h, rc, "dril_scaling_enable: " + msg) : DRIL_OK;
}
DRIL_EXPORT int32_t dril_agent_spaces(const dril_handle* h, float* obs_low, float* obs_high, float* action_low, float* action_high, int32_t* scaling) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!h->env.module) return fail(const_cast<dril_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_agent_spaces: the handle was not created with dril_create_with_env_module");
    h->env.agent_obs_space(obs_low, obs_high);
    if (!h->env.desc.discrete) h->env.agent_action_space(action_low, action_high);
    if (scaling) *scaling = h->env.scaling ? 1 : 0;
    return DRIL_OK;
}

namespace {
#define CCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { std::string m = std::string(#expr) + ": " + hipGetErrorString(_e); dril_destroy(h); return fail(nullptr, DRIL_ERR_HIP, m); } } while (0)
int create_impl(const dril_config* cfg, const char* module_path, dril_handle** out) {
    if (!cfg || !out) return fail(nullptr, DRIL_ERR_INVALID_ARG, "null cfg/out");
    if (cfg->abi_version != DRIL_ABI_VERSION) return fail(nullptr, DRIL_ERR_INVALID_ARG, "abi_version mismatch");
    if (cfg->env_kind < DRIL_ENV_CARTPOLE || cfg->env_kind > DRIL_ENV_MODULE) return fail(nullptr, DRIL_ERR_INVALID_ARG, "unknown env_kind");
    const bool is_module = cfg->env_kind == DRIL_ENV_MODULE;
    if (is_module && (cfg->norm_obs || cfg->norm_reward)) return fail(nullptr, DRIL_ERR_UNSUPPORTED, "DRIL_ENV_MODULE: NormalizeWrapperEnv through cfg.norm_obs / cfg.norm_reward is for the built-in envs (8 observation dims); wrap a device env plug-in with dril_normalize_enable on the created handle");
    if (is_module && cfg->episode_len < 0) return fail(nullptr, DRIL_ERR_INVALID_ARG, "DRIL_ENV_MODULE: episode_len must be > 0, or 0 for the plug-in's own time limit");
    const bool ext = cfg->env_kind == DRIL_ENV_EXTERNAL;
    if (ext && (cfg->ext_obs_dim < 1 || cfg->ext_obs_dim > 1024 || cfg->ext_action_dim < 1 || cfg->ext_action_dim > 64)) return fail(nullptr, DRIL_ERR_INVALID_ARG, "DRIL_ENV_EXTERNAL: ext_obs_dim must be 1..1024 and ext_action_dim 1..64");
    // hidden_dims / activation: n_hidden == 0 is the two-layer form (hidden1, hidden2); otherwise hidden[0 .. n_hidden-1]
    if (cfg->n_hidden < 0 || cfg->n_hidden > kMaxHidden) return fail(nullptr, DRIL_ERR_INVALID_ARG, "n_hidden must be 0 (hidden1 / hidden2) or 1..4");
    if (cfg->activation < 0 || cfg->activation > 7) return fail(nullptr, DRIL_ERR_UNSUPPORTED, "activation must be 0 (tanh), 1 (relu), 2 (sigmoid), 3 (elu), 4 (leakyrelu), 5 (softplus), 6 (gelu) or 7 (swish)");
    int nh = cfg->n_hidden ? cfg->n_hidden : 2, hd[kMaxHidden] = {cfg->hidden1, cfg->hidden2, 0, 0};
    if (cfg->n_hidden) for (int l = 0; l < nh; ++l) hd[l] = cfg->hidden[l];
    for (int l = 0; l < nh; ++l) if (hd[l] < 1 || hd[l] > 1024) return fail(nullptr, DRIL_ERR_INVALID_ARG, "hidden widths must be 1..1024");
    if (ext && (cfg->norm_obs || cfg->norm_reward || cfg->monitor_window)) return fail(nullptr, DRIL_ERR_UNSUPPORTED, "DRIL_ENV_EXTERNAL: NormalizeWrapperEnv / MonitorWrapperEnv wrap the host env on the host");
    if (cfg->n_envs < 1 || cfg->n_steps < 1 || cfg->epochs < 0 || cfg->batch_size < 1) return fail(nullptr, DRIL_ERR_INVALID_ARG, "n_envs/n_steps/batch_size must be positive");
    const bool fused_shape = nh == 2 && cfg->activation == 0 && hd[0] == hd[1] && (hd[0] == 32 || hd[0] == 64 || hd[0] == 128 || hd[0] == 256);   // 32: the reference's benchmark-suite shape (f32-MFMA kernels only)   // everything else: the generic kernels (any depth <= 4, any width <= 1024, tanh / relu)
    if (cfg->monitor_window < 0) return fail(nullptr, DRIL_ERR_INVALID_ARG, "monitor_window must be >= 0");
    if (cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size) return fail(nullptr, DRIL_ERR_INVALID_ARG, "bad rank/world_size");
    if (cfg->batch_size % cfg->world_size != 0) return fail(nullptr, DRIL_ERR_INVALID_ARG, "batch_size must be divisible by world_size");
    // Multi-process RCCL on this platform needs dmabuf IPC: with the legacy IPC mode (the ROCr default) `hipIpcGetMemHandle` fails with "invalid argument" on a
    // host driver that only supports dmabuf, and ncclCommInitRank / the first collective across processes dies with it.  The ROCr runtime reads the variable
    // when it initialises, i.e. at this process's first HIP call — which for a DRiL user is normally the plug-in load or the hipSetDevice below.  It is only set if the
    // caller left it unset (bench.py and the tests export it themselves; a process that already touched HIP before dril_create must export it on its own: README "Multi-GPU").
    if (cfg->world_size > 1) setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", /*overwrite=*/0);
    dril_handle* h = nullptr;
    try { h = new dril_handle(); } catch (...) { return fail(nullptr, DRIL_ERR_INVALID_ARG, "out of host memory"); }
    h->cfg = *cfg;
    {   // a plug-in's descriptor gives the spaces: it is loaded here, before anything is sized
        std::string msg; const int rcm = h->env.open(cfg->env_kind, cfg->n_envs, cfg->episode_len, cfg->fixed_length_episodes, cfg->action_start, module_path, cfg->device, msg);
        if (rcm) { delete h; return fail(nullptr, rcm, "dril_create_with_env_module: " + msg); }
        h->cfg.episode_len = h->env.episode_len;
    }
    const DrilEnvPluginDesc& desc = h->env.desc;
    h->cfg.hidden1 = hd[0]; h->cfg.hidden2 = nh > 1 ? hd[1] : hd[0];   // the fused kernels read hidden1 (only reached with two equal layers)
    const EnvKindInfo* kinfo = env_kind_info(cfg->env_kind);
    if (kinfo) { h->discrete = kinfo->discrete; h->D = kinfo->D; h->A = kinfo->A; h->S = kinfo->S; }                             // a built-in kind: fused kernels at the fused shapes
    else if (is_module) { h->discrete = desc.discrete != 0; h->D = desc.D; h->A = desc.A; h->S = desc.S; h->generic = true; }   // no fused kernels for a plug-in env
    else { h->discrete = cfg->ext_discrete != 0; h->D = cfg->ext_obs_dim; h->A = cfg->ext_action_dim; h->S = 0; h->external = true; h->generic = true; }   // DRIL_ENV_EXTERNAL
    h->gd = GenericDims{h->D, h->A, nh, {hd[0], hd[1], hd[2], hd[3]}, h->discrete ? 1 : 0, cfg->activation};
    if (nh == 2) { h->actor = net_off(0, h->D, hd[0], hd[1], h->A); h->critic = net_off(h->actor.end, h->D, hd[0], hd[1], 1); }
    else {                                                                            // other depths exist on the generic path only, which reads just the first offset and the end of a net
        std::memset(&h->actor, 0, sizeof(h->actor)); std::memset(&h->critic, 0, sizeof(h->critic));
        h->actor.w1 = 0; h->actor.end = generic_net_size(h->gd, h->A);
        h->critic.w1 = h->actor.end; h->critic.end = h->actor.end + generic_net_size(h->gd, 1);
    }
    h->Pa = h->actor.end; h->Pc = h->critic.end - h->actor.end; h->log_std_off = h->critic.end;
    h->P = h->critic.end + (h->discrete ? 0 : h->A);
    h->N = (int64_t)cfg->n_envs * cfg->n_steps; h->lr = cfg->learning_rate;
    if (!fused_shape || std::getenv("DRIL_FORCE_GENERIC")) h->generic = true;            // DRIL_FORCE_GENERIC: run a fused-shape handle on the generic kernels (A/B and parity tests)
    if (const char* e = std::getenv("DRIL_FORCE_ALLREDUCE")) h->force_allreduce = std::atoi(e) != 0;
    if (const char* e = std::getenv("DRIL_FORCE_STEPWISE")) h->force_stepwise = std::atoi(e) != 0;
    if (const char* e = std::getenv("DRIL_GRAD_ACTOR_PERMILLE")) { h->grad_actor_pct = std::atoi(e); if (h->grad_actor_pct < 100 || h->grad_actor_pct > 900) h->grad_actor_pct = 0; }
    if (const char* e = std::getenv("DRIL_GRAD_VARIANT")) { h->grad_variant = std::atoi(e); if (h->grad_variant < -1 || h->grad_variant > 2) h->grad_variant = -1; if (h->grad_variant == 2) h->grad_variant = 1; }
    h->no_persistent = std::getenv("DRIL_NO_PERSISTENT_UPDATE") != nullptr; { const char* e = std::getenv("DRIL_NO_EPOCH_INDEX"); h->no_epoch_index = e && std::atoi(e) != 0; }
    if (const char* e = debug_env("DRIL_SMALL_CHUNK")) { const long c = std::atol(e); if (c > 0) h->small_chunk = c; }   // optimiser steps per launch of ppo_update_small_kernel (tests: launch boundaries)
    h->no_small_path = debug_env("DRIL_NO_SMALL_PATH") != nullptr;
    h->no_f32_retry = std::getenv("DRIL_NO_F32_RETRY") != nullptr;
    CCHK(hipSetDevice(cfg->device));
    hipDeviceProp_t prop; CCHK(hipGetDeviceProperties(&prop, cfg->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) { std::string m = std::string("libdril_hip targets gfx950 (MI355X) only; device is ") + prop.gcnArchName; dril_destroy(h); return fail(nullptr, DRIL_ERR_UNSUPPORTED, m); }
    h->num_cus = prop.multiProcessorCount;
    {
        char bus[64] = "?"; int ndev = -1; (void)hipDeviceGetPCIBusId(bus, (int)sizeof(bus), cfg->device); (void)hipGetDeviceCount(&ndev);
        const char* hv = std::getenv("HIP_VISIBLE_DEVICES"); const char* rv = std::getenv("ROCR_VISIBLE_DEVICES");
        h->device_info = "device " + std::to_string(cfg->device) + " of " + std::to_string(ndev) + " visible: " + prop.name + " " + prop.gcnArchName + ", " + std::to_string(prop.multiProcessorCount) + " CUs, PCI " + bus +
                         ", HIP_VISIBLE_DEVICES=" + (hv ? hv : "(unset)") + " ROCR_VISIBLE_DEVICES=" + (rv ? rv : "(unset)");
    }
    CCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const size_t E = cfg->n_envs, N = (size_t)h->N, P = h->P;
    CCHK(h->params.alloc(P)); CCHK(h->adam_m.alloc(P)); CCHK(h->adam_v.alloc(P)); CCHK(h->bt.alloc(4));
    CCHK(h->flat.alloc(P + 8)); CCHK(h->norm_out.alloc(1)); CCHK(h->w2max_dev.alloc(1));
    { const size_t words = (size_t)gae_chunks(cfg->n_steps) * cfg->n_envs; CCHK(h->gae_carry.alloc(words)); CCHK(hipMemsetAsync(h->gae_carry, 0, words * 8, h->stream));
      CCHK(h->gae_err.alloc(1)); CCHK(hipMemsetAsync(h->gae_err, 0, 4, h->stream)); }
    h->n_norm_partials = (int)((P + 31) / 32); CCHK(h->norm_partials.alloc(h->n_norm_partials));
    if (h->generic) { h->slab_a = generic_slab_size(h->gd, true); h->slab_c = generic_slab_size(h->gd, false); }
    else { h->slab_a = slab_size_actor(*kinfo, hd[0]); h->slab_c = slab_size_critic(*kinfo, hd[0]); }
    h->wide = !h->generic && hd[0] > 64;
    h->Gmax = (h->wide && hd[0] > 128) ? (h->num_cus / 2 > 0 ? h->num_cus / 2 : 1) : (!h->wide && h->grad_variant != 0) ? 3 * h->num_cus : h->num_cus;   // H = 128: 4 waves and 77 KB LDS per workgroup, two workgroups per CU   // [64,64]: 2 workgroups per CU (actor + critic), 4 waves each; wide: 1 workgroup of H/32 waves per CU
    if (h->generic) h->Gmax = 64;                                                                                                                                                                                             // generic path: one slab per row chunk of the minibatch
    if (const char* e = debug_env("DRIL_GRAD_GMAX")) { const int g = std::atoi(e); if (g > 0 && g < h->Gmax) h->Gmax = g; }   // diagnostic: fewer workgroups per net
    if (h->wide) { const size_t pb = (size_t)hd[0] * hd[0] * 6;    // three bf16 pieces per element
        CCHK(h->w2p_actor.alloc(pb)); CCHK(h->w2tp_actor.alloc(pb)); CCHK(h->w2p_critic.alloc(pb)); CCHK(h->w2tp_critic.alloc(pb));
        CCHK(h->w2pf_actor.alloc(pb)); CCHK(h->w2pf_critic.alloc(pb)); }
    if (h->wide) { const size_t hh = (size_t)hd[0] * hd[0]; CCHK(h->w2a_actor.alloc(hh)); CCHK(h->w2ta_actor.alloc(hh)); CCHK(h->w2a_critic.alloc(hh)); CCHK(h->w2ta_critic.alloc(hh)); }
    CCHK(h->slabs_a.alloc((size_t)h->Gmax * h->slab_a)); CCHK(h->slabs_c.alloc((size_t)h->Gmax * h->slab_c));
    CCHK(h->env.alloc(h->S));
    CCHK(h->obs.alloc(N * h->D)); CCHK(h->act.alloc(N * act_bytes_per(h))); CCHK(h->rew.alloc(N)); CCHK(h->adv.alloc(N));
    CCHK(h->ret.alloc(N)); CCHK(h->logp.alloc(N)); CCHK(h->val.alloc(N)); CCHK(h->boot.alloc(N)); CCHK(h->flags.alloc(N));
    CCHK(h->last_values.alloc(E));
    if (!h->generic) CCHK(h->rec.alloc((size_t)(h->D <= 4 ? 2 : 3) * N));   // packed minibatch records: 2 (D <= 4) or 3 (D <= 8) float4 per sample
    if (h->generic) CCHK(h->gen_tmp.alloc(E));
    if (ext) { CCHK(h->ext_stage_rew.alloc(N)); CCHK(h->ext_stage_flags.alloc(N)); }
    if (ext) {
        CCHK(hipEventCreateWithFlags(&h->ext_ev_in, hipEventDisableTiming)); CCHK(hipEventCreateWithFlags(&h->ext_ev_out, hipEventDisableTiming));
        CCHK(h->ext_err.alloc(1)); CCHK(hipMemsetAsync(h->ext_err, 0, 4, h->stream)); CCHK(h->ext_err_host.alloc(1)); *h->ext_err_host = 0;
    }
    if (cfg->monitor_window > 0) {
        const size_t W = cfg->monitor_window;
        CCHK(h->mon_cur_ret.alloc(E)); CCHK(h->mon_cur_len.alloc(E)); CCHK(h->ep_ret.alloc(N)); CCHK(h->ep_len.alloc(N));
        CCHK(h->mon_ring_ret.alloc(W)); CCHK(h->mon_ring_len.alloc(W)); CCHK(h->e_ep_ret.alloc(E)); CCHK(h->e_ep_len.alloc(E));
        CCHK(h->mon_cnt.alloc((size_t)cfg->n_steps)); CCHK(h->mon_meta.alloc(2)); CCHK(h->e_flags.alloc(E));
        CCHK(hipMemset(h->mon_cur_ret, 0, E * 4)); CCHK(hipMemset(h->mon_cur_len, 0, E * 4)); CCHK(hipMemset(h->mon_meta, 0, 8));
    }
    h->adv_blocks = 1024; CCHK(h->adv_partials.alloc(2 * (size_t)h->adv_blocks)); CCHK(h->adv_stats.alloc(4));
    h->ev_blocks = 1024; CCHK(h->ev_partials.alloc(4 * (size_t)h->ev_blocks));
    CCHK(h->stop_flag.alloc(1)); CCHK(h->nan_flag.alloc(1));
#ifdef DRIL_STAMPS
    CCHK(h->dbg.alloc((size_t)2 * h->Gmax * 4 * 12)); CCHK(hipMemset(h->dbg, 0, (size_t)2 * h->Gmax * 4 * 12 * 8));
#endif
    CCHK(h->e_obs.alloc(E * h->D)); CCHK(h->e_rew.alloc(E)); CCHK(h->e_tobs.alloc(E * h->D)); CCHK(h->e_term.alloc(E));
    CCHK(h->e_trunc.alloc(E)); CCHK(h->e_act.alloc(E * act_bytes_per(h)));
    CCHK(h->e_obs_raw.alloc(E * h->D)); CCHK(h->e_rew_n.alloc(E)); CCHK(h->obs_rms.alloc(2)); CCHK(h->ret_rms.alloc(2)); CCHK(h->rms_partials.alloc((size_t)h->rms_blocks * 16)); CCHK(h->rms_red.alloc(16));
    { RmsState init[2]; for (auto& r : init) { for (int d = 0; d < 8; ++d) { r.mean[d] = 0.f; r.var[d] = 1.f; } r.count = 0; }   // RunningMeanStd{T}(shape): zeros, ones, 0 (normalizeWrapperEnv.jl:14-16)
      CCHK(hipMemcpy(h->obs_rms, init, sizeof(init), hipMemcpyHostToDevice)); CCHK(hipMemcpy(h->ret_rms, init, sizeof(init), hipMemcpyHostToDevice)); }
    CCHK(hipMemsetAsync(h->params, 0, P * 4, h->stream)); CCHK(hipMemsetAsync(h->boot, 0, N * 4, h->stream));
    CCHK(hipMemsetAsync(h->flags, 0, N, h->stream)); CCHK(hipMemsetAsync(h->last_values, 0, E * 4, h->stream));
    CCHK(hipMemsetAsync(h->stop_flag, 0, 4, h->stream)); CCHK(hipMemsetAsync(h->nan_flag, 0, 4, h->stream));
    CCHK(hipMemsetAsync(h->e_tobs, 0, E * h->D * 4, h->stream));
    if (!h->discrete) { std::vector<float> ls(h->A, cfg->log_std_init); CCHK(hipMemcpyAsync(h->params + h->log_std_off, ls.data(), 4 * h->A, hipMemcpyHostToDevice, h->stream)); CCHK(hipStreamSynchronize(h->stream)); }
    int rc = reset_optimizer(h);
    if (rc) { std::string m = h->err; dril_destroy(h); return fail(nullptr, rc, m); }
    *out = h;
    return DRIL_OK;
}
#undef CCHK
}  // namespace
DRIL_EXPORT int32_t dril_create(const dril_config* cfg, dril_handle** out) {
    if (cfg && cfg->abi_version == DRIL_ABI_VERSION && cfg->env_kind == DRIL_ENV_MODULE) return fail(nullptr, DRIL_ERR_INVALID_ARG, "DRIL_ENV_MODULE needs a code object: use dril_create_with_env_module(cfg, code_object_path, out)");
    return create_impl(cfg, nullptr, out);
}
DRIL_EXPORT int32_t dril_create_with_env_module(const dril_config* cfg, const char* code_object_path, dril_handle** out) {
    if (!cfg || !out) return fail(nullptr, DRIL_ERR_INVALID_ARG, "null cfg/out");
    if (cfg->abi_version != DRIL_ABI_VERSION) return fail(nullptr, DRIL_ERR_INVALID_ARG, "abi_version mismatch");
    if (cfg->env_kind != DRIL_ENV_MODULE) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_create_with_env_module: cfg->env_kind must be DRIL_ENV_MODULE");
    std::string msg; const int rc = check_code_object_path(code_object_path, msg);
    if (rc) return fail(nullptr, rc, "dril_create_with_env_module: " + msg);
    return create_impl(cfg, code_object_path, out);
}

DRIL_EXPORT int32_t dril_destroy(dril_handle* h) {
    if (h) (void)hipSetDevice(h->cfg.device);
    if (!h) return DRIL_OK;
    if (h->pop) { h->err = "dril_destroy: the handle is a member of a population: dril_population_destroy first (the members stay alive and usable)"; return DRIL_ERR_INVALID_ARG; }
    if (h->stream) hipStreamSynchronize(h->stream);
    comm_release(h);
    h->env.release();
    if (h->ext_ev_in) (void)hipEventDestroy(h->ext_ev_in); if (h->ext_ev_out) (void)hipEventDestroy(h->ext_ev_out);
    for (auto& p : h->prof_pending) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
    for (auto& p : h->prof_pool) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return DRIL_OK;
}
DRIL_EXPORT const char* dril_last_error(const dril_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }
DRIL_EXPORT int32_t dril_synchronize(dril_handle* h) { NEED(h); return sync(h); }
DRIL_EXPORT int32_t dril_obs_dim(const dril_handle* h) { return h ? h->D : -1; }
DRIL_EXPORT int32_t dril_action_dim(const dril_handle* h) { return h ? h->A : -1; }
DRIL_EXPORT int32_t dril_is_discrete(const dril_handle* h) { return h ? (h->discrete ? 1 : 0) : -1; }
DRIL_EXPORT int64_t dril_param_count(const dril_handle* h) { return h ? h->P : -1; }

DRIL_EXPORT int32_t dril_set_params(dril_handle* h, const float* flat, size_t n) {
    NEED(h); if (!flat || n != (size_t)h->P) return fail(h, DRIL_ERR_INVALID_ARG, "dril_set_params: n != dril_param_count");
    HIPCHK(h, hipMemcpyAsync(h->params, flat, n * 4, hipMemcpyHostToDevice, h->stream)); h->wimg_dirty = true;
    if (!h->generic) {                                                                // max |W2| of the new parameters decides the forward's arithmetic (fwd_exact)
        const size_t HH = (size_t)h->cfg.hidden1 * h->cfg.hidden1; float m = 0.f;
        for (const float* w : {flat + h->actor.w2, flat + h->critic.w2}) for (size_t i = 0; i < HH; ++i) { const float x = std::fabs(w[i]); m = (x > m || x != x) ? (x != x ? INFINITY : x) : m; }
        h->w2max = m;
    }
    return sync(h);
}
DRIL_EXPORT int32_t dril_get_params(dril_handle* h, float* flat, size_t n) {
    NEED(h); if (!flat || n != (size_t)h->P) return fail(h, DRIL_ERR_INVALID_ARG, "dril_get_params: n != dril_param_count");
    HIPCHK(h, hipMemcpyAsync(flat, h->params, n * 4, hipMemcpyDeviceToHost, h->stream)); return sync(h);
}
DRIL_EXPORT int32_t dril_reset_optimizer(dril_handle* h) { NEED(h); return reset_optimizer(h); }
DRIL_EXPORT int32_t dril_set_learning_rate(dril_handle* h, float lr) { NEED(h); h->lr = lr; return DRIL_OK; }
DRIL_EXPORT int32_t dril_get_optimizer_state(dril_handle* h, float* m, float* v, size_t n, float* beta_powers, int64_t* steps) {
    NEED(h);
    if (!m || !v || !beta_powers || n != (size_t)h->P) return fail(h, DRIL_ERR_INVALID_ARG, "dril_get_optimizer_state: n != dril_param_count or null pointer");
    float bt[4];
    HIPCHK(h, hipMemcpyAsync(m, h->adam_m, n * 4, hipMemcpyDeviceToHost, h->stream)); HIPCHK(h, hipMemcpyAsync(v, h->adam_v, n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(bt, h->bt, sizeof(bt), hipMemcpyDeviceToHost, h->stream));
    int rc = sync(h); if (rc) return rc;
    const int slot = 2 * (int)(h->adam_steps & 1);                                     // the slot the NEXT step reads (ping-pong)
    beta_powers[0] = bt[slot]; beta_powers[1] = bt[slot + 1];
    if (steps) *steps = h->adam_steps;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_set_optimizer_state(dril_handle* h, const float* m, const float* v, size_t n, const float* beta_powers, int64_t steps) {
    NEED(h);
    if (!m || !v || !beta_powers || n != (size_t)h->P || steps < 0) return fail(h, DRIL_ERR_INVALID_ARG, "dril_set_optimizer_state: n != dril_param_count, null pointer or negative step count");
    const float bt[4] = {beta_powers[0], beta_powers[1], beta_powers[0], beta_powers[1]};
    HIPCHK(h, hipMemcpyAsync(h->adam_m, m, n * 4, hipMemcpyHostToDevice, h->stream)); HIPCHK(h, hipMemcpyAsync(h->adam_v, v, n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->bt, bt, sizeof(bt), hipMemcpyHostToDevice, h->stream));
    h->adam_steps = steps;
    return sync(h);
}

// ---- env verbs -----------------------------------------------------------------------------------
DRIL_EXPORT int32_t dril_env_reset(dril_handle* h, uint64_t seed) {
    NEED(h); NOT_EXTERNAL(h, "dril_env_reset");
    h->env.seed0 = seed + (uint64_t)h->cfg.rank * (uint64_t)h->cfg.n_envs;
    HIPCHK(h, h->env.reset(h->stream));
    if (h->mon_cur_ret) { HIPCHK(h, hipMemsetAsync(h->mon_cur_ret, 0, (size_t)h->cfg.n_envs * 4, h->stream)); HIPCHK(h, hipMemsetAsync(h->mon_cur_len, 0, (size_t)h->cfg.n_envs * 4, h->stream)); }   // MonitorWrapperEnv.reset! :38-44
    if (h->pn.on) {                                                                  // NormalizeWrapperEnv.reset! :110-121: old_obs = the raw observation, returns = 0, the statistics stay
        HIPCHK(h, hipMemsetAsync(h->env.disc_returns, 0, (size_t)h->cfg.n_envs * 4, h->stream)); HIPCHK(h, h->env.observe(h->e_obs_raw, h->stream));
    }
    h->env.ready = true;
    return sync(h);
}
DRIL_EXPORT int32_t dril_env_observe(dril_handle* h, float* host_obs, int32_t update_stats) {
    NEED(h); NOT_EXTERNAL(h, "dril_env_observe");
    if (!h->env.ready) return fail(h, DRIL_ERR_NOT_INITIALISED, "dril_env_observe before dril_env_reset");
    if (!host_obs) return fail(h, DRIL_ERR_INVALID_ARG, "null host_obs");
    if (normalizing(h) || h->pn.on) { int rc = observe_dev(h, update_stats != 0); if (rc) return rc; }
    else HIPCHK(h, h->env.observe(h->e_obs, h->stream));
    HIPCHK(h, hipMemcpyAsync(host_obs, h->e_obs, (size_t)h->cfg.n_envs * h->D * 4, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}
DRIL_EXPORT int32_t dril_env_step(dril_handle* h, const void* actions, float* rewards, uint8_t* terminated, uint8_t* truncated, float* terminal_obs) {
    NEED(h); NOT_EXTERNAL(h, "dril_env_step");
    if (!h->env.ready) return fail(h, DRIL_ERR_NOT_INITIALISED, "dril_env_step before dril_env_reset");
    if (!actions) return fail(h, DRIL_ERR_INVALID_ARG, "null actions");
    const size_t E = h->cfg.n_envs;
    HIPCHK(h, hipMemcpyAsync(h->e_act, actions, E * act_bytes_per(h), hipMemcpyHostToDevice, h->stream));
    float* rew_dev = h->e_rew;
    if (normalizing(h) || h->pn.on) { rew_dev = h->e_rew_n; int rc = step_dev(h, h->e_act, rew_dev, nullptr); if (rc) return rc; }
    else { int rc = env_step_arrays(h, h->e_act); if (rc) return rc; }
    if (rewards) HIPCHK(h, hipMemcpyAsync(rewards, rew_dev, E * 4, hipMemcpyDeviceToHost, h->stream));
    if (terminated) HIPCHK(h, hipMemcpyAsync(terminated, h->e_term, E, hipMemcpyDeviceToHost, h->stream));
    if (truncated) HIPCHK(h, hipMemcpyAsync(truncated, h->e_trunc, E, hipMemcpyDeviceToHost, h->stream));
    if (terminal_obs) HIPCHK(h, hipMemcpyAsync(terminal_obs, h->e_tobs, E * h->D * 4, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}
DRIL_EXPORT int32_t dril_env_get_state(dril_handle* h, float* state, int32_t* step_count) {
    NEED(h); NOT_EXTERNAL(h, "dril_env_get_state"); if (!state) return fail(h, DRIL_ERR_INVALID_ARG, "null state");
    // a world handle moves its W = n_envs / N states (S floats each, world w at float offset w S); the counters are per row for every handle
    HIPCHK(h, hipMemcpyAsync(state, h->env.state, (size_t)h->env.n_worlds() * h->S * 4, hipMemcpyDeviceToHost, h->stream));
    if (step_count) HIPCHK(h, hipMemcpyAsync(step_count, h->env.step_count, (size_t)h->cfg.n_envs * 4, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}
DRIL_EXPORT int32_t dril_env_set_state(dril_handle* h, const float* state, const int32_t* step_count) {
    NEED(h); NOT_EXTERNAL(h, "dril_env_set_state"); if (!state) return fail(h, DRIL_ERR_INVALID_ARG, "null state");
    if (step_count && h->env.is_world()) {                                             // the N rows of a world count the same steps: unequal values are refused, nothing is written
        const int N = h->env.agents();
        for (int e = 0; e < h->cfg.n_envs; ++e) if (step_count[e] != step_count[e - e % N])
            return fail(h, DRIL_ERR_INVALID_ARG, "dril_env_set_state: rows " + std::to_string(e - e % N) + " and " + std::to_string(e) + " belong to one world of " + std::to_string(N) + " agents but are given step counts " + std::to_string(step_count[e - e % N]) + " and " + std::to_string(step_count[e]) + ": the rows of a world share the world's step count");
    }
    HIPCHK(h, hipMemcpyAsync(h->env.state, state, (size_t)h->env.n_worlds() * h->S * 4, hipMemcpyHostToDevice, h->stream));
    if (step_count) HIPCHK(h, hipMemcpyAsync(h->env.step_count, step_count, (size_t)h->cfg.n_envs * 4, hipMemcpyHostToDevice, h->stream));
    return sync(h);
}
DRIL_EXPORT int32_t dril_norm_get_stats(dril_handle* h, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count) {
    NEED(h); NOT_EXTERNAL(h, "dril_norm_get_stats");
    if (h->env.module && h->pn.on) return dril_normalize_get_stats(h, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);   // the wrapper of dril_normalize_enable
    NOT_MODULE(h, "dril_norm_get_stats");
    RmsState o, r;
    HIPCHK(h, hipMemcpyAsync(&o, h->obs_rms + h->obs_par, sizeof(o), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&r, h->ret_rms + h->ret_par, sizeof(r), hipMemcpyDeviceToHost, h->stream));
    int rc = sync(h); if (rc) return rc;
    if (obs_mean) std::memcpy(obs_mean, o.mean, 4 * h->D); if (obs_var) std::memcpy(obs_var, o.var, 4 * h->D); if (obs_count) *obs_count = o.count;
    if (ret_mean) *ret_mean = r.mean[0]; if (ret_var) *ret_var = r.var[0]; if (ret_count) *ret_count = r.count;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_norm_set_stats(dril_handle* h, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count) {
    NEED(h); NOT_EXTERNAL(h, "dril_norm_set_stats");
    if (h->env.module && h->pn.on) return dril_normalize_set_stats(h, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);
    NOT_MODULE(h, "dril_norm_set_stats");
    if (!obs_mean || !obs_var) return fail(h, DRIL_ERR_INVALID_ARG, "null statistics");
    RmsState o{}, r{};
    for (int d = 0; d < 8; ++d) { o.mean[d] = d < h->D ? obs_mean[d] : 0.f; o.var[d] = d < h->D ? obs_var[d] : 1.f; r.mean[d] = 0.f; r.var[d] = 1.f; }
    o.count = obs_count; r.mean[0] = ret_mean; r.var[0] = ret_var; r.count = ret_count;
    HIPCHK(h, hipMemcpyAsync(h->obs_rms + h->obs_par, &o, sizeof(o), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->ret_rms + h->ret_par, &r, sizeof(r), hipMemcpyHostToDevice, h->stream));
    return sync(h);
}

DRIL_EXPORT int32_t dril_norm_get_original(dril_handle* h, float* obs, float* rewards) {
    NEED(h); NOT_EXTERNAL(h, "dril_norm_get_original");
    if (h->env.module && h->pn.on) return dril_normalize_get_original(h, obs, rewards);
    NOT_MODULE(h, "dril_norm_get_original");
    if (!normalizing(h)) return fail(h, DRIL_ERR_NOT_INITIALISED, "NormalizeWrapperEnv is off (cfg.norm_obs == cfg.norm_reward == 0)");
    if (obs) HIPCHK(h, hipMemcpyAsync(obs, h->e_obs_raw, (size_t)h->cfg.n_envs * h->D * 4, hipMemcpyDeviceToHost, h->stream));
    if (rewards) HIPCHK(h, hipMemcpyAsync(rewards, h->e_rew, (size_t)h->cfg.n_envs * 4, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}


// ---- policy on host batches ----------------------------------------------------------------------
namespace {
int policy_host(dril_handle* h, const float* obs, int64_t B, const void* noise, void* actions, bool actions_in, float* values, float* logp,
                float* entropy, int mode, int deterministic = 0) {
    if (!obs || B < 1) return fail(h, DRIL_ERR_INVALID_ARG, "policy: null obs or batch < 1");
    DevBuf<float> d_obs, d_val, d_lp, d_ent; DevBuf<char> d_noise, d_act;                       // freed on every return
    const size_t ab = (size_t)B * act_bytes_per(h), nb = (size_t)B * (h->discrete ? 8 : 4 * (size_t)h->A);
    HIPCHK(h, d_obs.alloc((size_t)B * h->D)); HIPCHK(h, d_val.alloc((size_t)B)); HIPCHK(h, d_lp.alloc((size_t)B)); HIPCHK(h, d_ent.alloc((size_t)B));
    HIPCHK(h, d_act.alloc(ab));
    HIPCHK(h, hipMemcpyAsync(d_obs, obs, (size_t)B * h->D * 4, hipMemcpyHostToDevice, h->stream));
    if (noise) { HIPCHK(h, d_noise.alloc(nb)); HIPCHK(h, hipMemcpyAsync(d_noise, noise, nb, hipMemcpyHostToDevice, h->stream)); }
    if (actions_in) HIPCHK(h, hipMemcpyAsync(d_act, actions, ab, hipMemcpyHostToDevice, h->stream));
    { int rcw = ensure_wimg(h); if (rcw) return rcw; }
    PolicyArgs a = policy_args(h, d_obs, B, d_noise, d_act, d_val, d_lp, d_ent, mode);
    a.deterministic = deterministic;
    HIPCHK(h, run_policy(h, a));
    h->policy_calls += 1;
    if (values) HIPCHK(h, hipMemcpyAsync(values, d_val, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (logp && mode != 2) HIPCHK(h, hipMemcpyAsync(logp, d_lp, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (entropy && mode == 1) HIPCHK(h, hipMemcpyAsync(entropy, d_ent, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (actions && mode == 0) HIPCHK(h, hipMemcpyAsync(actions, d_act, ab, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}
}  // namespace
DRIL_EXPORT int32_t dril_policy_forward(dril_handle* h, const float* obs, int64_t batch, const void* noise, void* actions, float* values, float* logprobs) {
    NEED(h); return policy_host(h, obs, batch, noise, actions, false, values, logprobs, nullptr, 0);
}
DRIL_EXPORT int32_t dril_evaluate_actions(dril_handle* h, const float* obs, const void* actions, int64_t batch, float* values, float* logprobs, float* entropy) {
    NEED(h); if (!actions) return fail(h, DRIL_ERR_INVALID_ARG, "null actions");
    return policy_host(h, obs, batch, nullptr, const_cast<void*>(actions), true, values, logprobs, entropy, 1);
}
DRIL_EXPORT int32_t dril_predict_actions(dril_handle* h, const float* obs, int64_t batch, int32_t deterministic, const void* noise, void* actions) {
    NEED(h); if (!actions) return fail(h, DRIL_ERR_INVALID_ARG, "null actions");
    return policy_host(h, obs, batch, deterministic ? nullptr : noise, actions, false, nullptr, nullptr, nullptr, 0, deterministic ? 1 : 0);
}
DRIL_EXPORT int32_t dril_predict_values(dril_handle* h, const float* obs, int64_t batch, float* values) {
    NEED(h); return policy_host(h, obs, batch, nullptr, nullptr, false, values, nullptr, nullptr, 2);
}

// extract_policy(agent) / extract_policy(agent, norm_env) (deployment_policy.jl:15-22, :52-58) on the device: the actor, log_std, the adapter's bounds and — with_norm —
// the observation statistics in force are copied device-to-device into a policy object of its own (include/dril_policy.h).  Reads the handle, changes nothing in it.
DRIL_EXPORT int32_t dril_policy_from_handle(dril_handle* h, int32_t with_norm, dril_policy** out) {
    if (!h) { policy_set_create_error("dril_policy_from_handle: null handle"); return DRIL_ERR_NOT_INITIALISED; }
    NEED(h);
    auto refuse = [&](int code, const std::string& m) { policy_set_create_error(m); return fail(h, code, m); };
    if (!out) return refuse(DRIL_ERR_INVALID_ARG, "dril_policy_from_handle: null out pointer");
    *out = nullptr;
    PolicyDeviceSource s{}; dril_policy_desc& d = s.desc;
    d.abi_version = DRIL_POLICY_ABI_VERSION; d.kind = h->discrete ? DRIL_POLICY_CATEGORICAL : DRIL_POLICY_DIAG_GAUSSIAN;
    d.obs_dim = h->D; d.action_dim = h->A; d.action_start = h->discrete ? h->cfg.action_start : 0;
    d.n_hidden = h->gd.nh; for (int l = 0; l < h->gd.nh; ++l) d.hidden[l] = h->gd.H[l];
    d.activation = h->cfg.activation; d.device = h->cfg.device;
    if (!h->discrete) for (int a = 0; a < h->A; ++a) {                                 // the Box the ClampAdapter clamps to (default_adapters.jl:4-11)
        if (h->env.module) { d.action_low[a] = h->env.desc.action_low[a]; d.action_high[a] = h->env.desc.action_high[a]; }
        else if (h->external && h->ext_bounds_set) { d.action_low[a] = h->ext_bounds.lo[a]; d.action_high[a] = h->ext_bounds.hi[a]; }   // dril_ext_set_action_bounds
        else if (h->external) { d.action_low[a] = h->cfg.ext_action_low; d.action_high[a] = h->cfg.ext_action_high; }   // low >= high: per-dimension bounds the host env clamps to itself
        else { const EnvKindInfo* k = env_kind_info(h->env.kind); d.action_low[a] = k->act_lo; d.action_high[a] = k->act_hi; }   // a built-in Box: Pendulum's torque [-2, 2], every other [-1, 1]
    }
    if (with_norm) {
        if (h->env.module && h->pn.on) {                                                   // the wrapper of dril_normalize_enable
            d.has_norm = 1; d.clip_obs = h->pn.cfg.clip_obs; d.epsilon = h->pn.cfg.epsilon;
            s.obs_mean = h->pn.half(h->pn.cur); s.obs_var = s.obs_mean + h->D;
        } else if (!h->env.module && !h->external && normalizing(h)) {                     // cfg.norm_obs / cfg.norm_reward: the built-in envs' wrapper
            d.has_norm = 1; d.clip_obs = h->cfg.clip_obs; d.epsilon = h->cfg.norm_epsilon;
            const RmsState* st = h->obs_rms + h->obs_par;
            s.obs_mean = st->mean; s.obs_var = st->var;
        } else return refuse(DRIL_ERR_NOT_INITIALISED, "dril_policy_from_handle: with_norm = 1, but the handle has no NormalizeWrapperEnv (cfg.norm_obs / cfg.norm_reward, or dril_normalize_enable on a plug-in handle)");
    }
    s.actor = h->params + h->actor.w1; s.n = (size_t)h->Pa; s.log_std = h->discrete ? nullptr : h->params + h->log_std_off; s.stream = h->stream;
    std::string msg;
    const int rc = policy_from_device(s, out, &msg);
    return rc ? fail(h, rc, "dril_policy_from_handle: " + msg) : DRIL_OK;
}

// ---- rollout ---------------------------------------------------------------------------------------
namespace {
int compute_gae(dril_handle* h) {
    if (++h->gae_tag == 0) h->gae_tag = 1;                                            // 0 = "never written" (the carry words are zero at allocation)
    prof_begin(h, DRIL_K_GAE);
    HIPCHK(h, launch_gae(h->cfg.n_envs, h->cfg.n_steps, h->cfg.gamma, h->cfg.gae_lambda, h->rew, h->val, h->flags, h->boot, h->last_values,
                         h->adv, h->ret, h->gae_carry, h->gae_tag, h->gae_err, h->stream));
    prof_end(h);
    return DRIL_OK;
}
// step-granular collect_trajectories (trajectory.jl:22-78) for wrapped envs: three launches per env step on the handle's stream
//   policy_kernel (+ V(terminal_observation) of the previous step) -> norm_step_kernel -> norm_apply_kernel
int collect_rollout_stepwise(dril_handle* h) {
    const int E = h->cfg.n_envs, T = h->cfg.n_steps, D = h->D, A = h->A;
    const size_t ab = act_bytes_per(h);
    int nb = (E + 255) / 256; if (nb > h->rms_blocks) nb = h->rms_blocks;
    int rc = observe_dev(h, true); if (rc) return rc;                                      // new_obs = observe(env), trajectory.jl:32
    for (int t = 0; t < T; ++t) {
        const size_t k = (size_t)t * E;
        const void* nz = h->noise_set ? (const void*)((const char*)h->noise_dev + k * (h->discrete ? 8 : 4 * (size_t)A)) : nullptr;
        PolicyArgs p = policy_args(h, h->e_obs, E, nz, (char*)h->act + k * ab, h->val + k, h->logp + k, nullptr, 0);
        p.gstep = h->env.gstep; p.env_seed0 = h->env.seed0; p.obs_out = h->obs + k * D;
        if (t > 0) { p.boot_obs = h->e_tobs; p.boot_where = h->e_trunc; p.boot_out = h->boot + (k - E); }   // :57-61 for step t-1
        HIPCHK(h, run_policy(h, p));   // get_action_and_values, :41
        NormStepArgs s{};
        s.E = E; s.episode_len = h->env.episode_len; s.fixed_len = h->env.fixed_len; s.action_start = h->env.action_start;
        s.seed0 = h->env.seed0; s.gamma = h->cfg.norm_gamma; s.update_ret = (h->cfg.norm_reward && h->cfg.norm_training) ? 1 : 0;
        s.actions = (const char*)h->act + k * ab; s.state = h->env.state; s.step_count = h->env.step_count; s.episode = h->env.episode; s.gstep = h->env.gstep;
        s.disc_returns = h->env.disc_returns; s.rew_raw = h->e_rew; s.term = h->e_term; s.trunc = h->e_trunc; s.flags_out = h->flags + k;
        s.tobs_raw = h->e_tobs; s.obs_raw = h->e_obs_raw; s.partials = h->rms_partials;
        if (h->mon_cur_ret) { s.mon_cur_ret = h->mon_cur_ret; s.mon_cur_len = h->mon_cur_len; s.ep_ret = h->ep_ret + k; s.ep_len = h->ep_len + k; }
        HIPCHK(h, launch_norm_step(h->env.kind, s, nb, h->stream));                              // to_env + act!, :43-44
        NormApplyArgs ap{};
        ap.E = E; ap.D = D; ap.update_obs = (h->cfg.norm_obs && h->cfg.norm_training) ? 1 : 0; ap.update_ret = s.update_ret;
        ap.norm_obs = h->cfg.norm_obs; ap.norm_reward = h->cfg.norm_reward;
        int nba = nb;
        { int rcg = global_partials(h, ap.update_obs || ap.update_ret, ap.partials, nba, ap.n_stats); if (rcg) return rcg; }
        ap.nblocks = nba;
        ap.obs_in = h->obs_rms + h->obs_par; ap.obs_out = h->obs_rms + (h->obs_par ^ 1); ap.ret_in = h->ret_rms + h->ret_par; ap.ret_out = h->ret_rms + (h->ret_par ^ 1);
        ap.rew_raw = h->e_rew; ap.rew_out = h->rew + k; ap.disc_returns = h->env.disc_returns; ap.term = h->e_term; ap.trunc = h->e_trunc; ap.tobs = h->e_tobs;
        ap.obs_raw = h->e_obs_raw; ap.obs_n = h->e_obs; ap.clip_obs = h->cfg.clip_obs; ap.clip_reward = h->cfg.clip_reward; ap.eps = h->cfg.norm_epsilon;
        HIPCHK(h, launch_norm_apply(ap, h->stream));                                                 // new_obs = observe(env), :45
        h->obs_par ^= 1; h->ret_par ^= 1;
    }
    PolicyArgs l = policy_args(h, h->e_obs, E, nullptr, nullptr, h->last_values, nullptr, nullptr, 2);
    l.boot_obs = h->e_tobs; l.boot_where = h->e_trunc; l.boot_out = h->boot + (size_t)(T - 1) * E;
    HIPCHK(h, run_policy(h, l));       // V(new_obs) for rollout-limited tails, :65-70
    return monitor_collect_rollout(h);
}

// step-granular collect_trajectories for a device env plug-in: two launch groups per env step,
//   policy (generic forward + sampling head, + V(terminal_observation) of the previous step) -> the plug-in's step kernel
// which writes reward and BUF_FLAGS byte straight into row t, the terminal observation and the next observation into the per-step arrays (one env launch where
// the built-in generic path has norm_step_kernel + norm_apply_kernel).  Noise: stream 1 at gstep, or the injected table, exactly as collect_rollout_stepwise.
int collect_rollout_module(dril_handle* h) {
    const int E = h->cfg.n_envs, T = h->cfg.n_steps, D = h->D, A = h->A;
    const size_t ab = act_bytes_per(h);
    h->rollout_launches += 1 + T;                                                                 // the opening observe and T step kernels; run_policy counts its own
    HIPCHK(h, h->env.observe(h->e_obs, h->stream));                                               // new_obs = observe(env), trajectory.jl:32
    for (int t = 0; t < T; ++t) {
        const size_t k = (size_t)t * E;
        const void* nz = h->noise_set ? (const void*)((const char*)h->noise_dev + k * (h->discrete ? 8 : 4 * (size_t)A)) : nullptr;
        PolicyArgs p = policy_args(h, h->e_obs, E, nz, (char*)h->act + k * ab, h->val + k, h->logp + k, nullptr, 0);
        p.gstep = h->env.gstep; p.env_seed0 = h->env.seed0; p.obs_out = h->obs + k * D;
        if (t > 0) { p.boot_obs = h->e_tobs; p.boot_where = h->e_trunc; p.boot_out = h->boot + (k - E); }   // :57-61 for step t-1
        HIPCHK(h, run_policy(h, p));                                                       // get_action_and_values, :41
        HIPCHK(h, h->env.step((const char*)h->act + k * ab, EnvStepOut{h->rew + k, h->e_term, h->e_trunc, h->e_tobs, h->e_obs}, monitor_rollout_args(h, k), h->stream));   // to_env + act! + observe, :43-45
    }
    PolicyArgs l = policy_args(h, h->e_obs, E, nullptr, nullptr, h->last_values, nullptr, nullptr, 2);
    l.boot_obs = h->e_tobs; l.boot_where = h->e_trunc; l.boot_out = h->boot + (size_t)(T - 1) * E;
    HIPCHK(h, run_policy(h, l));                                                           // V(new_obs) for rollout-limited tails, :65-70
    return monitor_collect_rollout(h);
}

// the fused collection (dril_rollout_fused_enable): ONE launch of the plug-in's own rollout kernel (include/device/dril_env_rollout.h) does what the loop of
// collect_rollout_module does in 6+ launches per env step, and leaves env state, counters, monitor sums and the per-step arrays as that loop leaves them
int collect_rollout_module_fused(dril_handle* h) {
    DrilEnvRolloutArgs g{};
    g.env = h->env.args();
    g.env.terminated = h->e_term; g.env.truncated = h->e_trunc; g.env.terminal_obs = h->e_tobs; g.env.obs = h->e_obs;
    g.env.mon_cur_ret = h->mon_cur_ret; g.env.mon_cur_len = h->mon_cur_len;
    g.T = h->cfg.n_steps; g.n_hidden = h->gd.nh; g.activation = h->gd.act; g.n_params = h->P;
    for (int l = 0; l < h->gd.nh; ++l) g.hidden[l] = h->gd.H[l];
    g.actor_off = h->actor.w1; g.critic_off = h->critic.w1; g.log_std_off = h->log_std_off;
    g.params = h->params; g.noise = h->noise_set ? h->noise_dev : nullptr;
    g.obs = h->obs; g.act = h->act; g.rew = h->rew; g.logp = h->logp; g.val = h->val; g.boot = h->boot; g.flags = h->flags; g.last_values = h->last_values;
    if (h->mon_cur_ret) { g.ep_ret = h->ep_ret; g.ep_len = h->ep_len; }
    h->rollout_launches += 1;
    HIPCHK(h, h->env.launch_rollout(g, h->stream));
    return monitor_collect_rollout(h);
}
// "" when the handle's net fits the plug-in's fused rollout kernel, else why not
std::string fused_rollout_unavailable(const dril_handle* h) {
    if (!h->env.module) return "the fused rollout is the collection kernel of a device env plug-in (DRIL_ENV_MODULE): the built-in envs collect with the library's own rollout_kernel, host envs (DRIL_ENV_EXTERNAL) step on the host";
    if (h->env.is_world()) return std::string("env plug-in \"") + h->env.desc.name + "\" is a world of " + std::to_string(h->env.agents()) + " agents: worlds have no fused rollout yet (DRIL_ENV_PLUGIN_ROLLOUT refuses a world at compile time); collect step-granular, which is the default";
    const EnvModuleRollout& r = h->env.rollout;
    if (!r.reason.empty()) return std::string("env plug-in \"") + h->env.desc.name + "\": " + r.reason;
    const int W = r.desc.max_width;
    if (h->D > W) return "the observation has " + std::to_string(h->D) + " dims, the plug-in's fused rollout was compiled for widths up to " + std::to_string(W) + ": rebuild it with -DDRIL_ENV_ROLLOUT_MAX_WIDTH=" + std::to_string(h->D) + " or more";
    for (int l = 0; l < h->gd.nh; ++l) if (h->gd.H[l] > W) return "hidden layer " + std::to_string(l + 1) + " is " + std::to_string(h->gd.H[l]) + " wide, the plug-in's fused rollout was compiled for widths up to " + std::to_string(W) + ": rebuild it with -DDRIL_ENV_ROLLOUT_MAX_WIDTH=" + std::to_string(h->gd.H[l]) + " or more";
    if (h->env.scaling && !r.fn_scaled) return "ScalingWrapperEnv is on, but the code object has no dril_env_plugin_rollout_scaled kernel: rebuild it with this library's include/device/dril_env_rollout.h";
    return "";
}

// "" when the handle's net fits the plug-in's fused evaluation kernel (path 2 of the evaluation / trajectory verbs), else why not
std::string fused_evaluate_unavailable(const dril_handle* h) {
    if (!h->env.module) return "the fused evaluation is a kernel of a device env plug-in (DRIL_ENV_MODULE): the built-in envs evaluate with the library's own evaluate_kernel, host envs (DRIL_ENV_EXTERNAL) step on the host";
    if (h->env.is_world()) return std::string("env plug-in \"") + h->env.desc.name + "\" is a world of " + std::to_string(h->env.agents()) + " agents: worlds have no fused evaluation yet (DRIL_ENV_PLUGIN_EVALUATE refuses a world at compile time); the evaluation and trajectory verbs run step-granular (path 0)";
    const EnvModuleEvaluate& r = h->env.evaluate;
    if (!r.reason.empty()) return std::string("env plug-in \"") + h->env.desc.name + "\": " + r.reason;
    const int W = r.desc.max_width;
    if (h->D > W) return "the observation has " + std::to_string(h->D) + " dims, the plug-in's fused evaluation was compiled for widths up to " + std::to_string(W) + ": rebuild it with -DDRIL_ENV_ROLLOUT_MAX_WIDTH=" + std::to_string(h->D) + " or more";
    for (int l = 0; l < h->gd.nh; ++l) if (h->gd.H[l] > W) return "hidden layer " + std::to_string(l + 1) + " is " + std::to_string(h->gd.H[l]) + " wide, the plug-in's fused evaluation was compiled for widths up to " + std::to_string(W) + ": rebuild it with -DDRIL_ENV_ROLLOUT_MAX_WIDTH=" + std::to_string(h->gd.H[l]) + " or more";
    if (h->env.scaling && !r.fn_scaled) return "ScalingWrapperEnv is on, but the code object has no dril_env_plugin_evaluate_scaled kernel: rebuild it with this library's include/device/dril_env_evaluate.h";
    return "";
}

// a collection that is ONE launch of the fused rollout kernel of a built-in kind (generic nets have no fused rollout kernel, wrapped envs step through the wrapper's kernels)
bool rollout_fused_applies(const dril_handle* h) { return !(normalizing(h) || h->force_stepwise || h->generic); }
// the argument block of that launch, read from the handle as it stands (collect_rollout, and a population for each of its members)
RolloutArgs rollout_args(const dril_handle* h) {
    RolloutArgs a{};
    a.params = h->params; a.state = h->env.state; a.step_count = h->env.step_count; a.episode = h->env.episode; a.gstep = h->env.gstep;
    a.obs = h->obs; a.act = h->act; a.rew = h->rew; a.logp = h->logp; a.val = h->val; a.boot = h->boot; a.flags = h->flags; a.last_values = h->last_values;
    a.noise = h->noise_set ? h->noise_dev : nullptr;
    a.E = h->env.E; a.T = h->cfg.n_steps; a.episode_len = h->env.episode_len; a.fixed_len = h->env.fixed_len;
    a.action_start = h->env.action_start; a.log_std_off = h->log_std_off; a.env_seed0 = h->env.seed0; a.actor = h->actor; a.critic = h->critic;
    a.exact_f32 = fwd_exact(h) ? 1 : 0;
    a.w2a_actor = a.exact_f32 ? h->w2a_actor : (const float*)h->w2pf_actor.get(); a.w2a_critic = a.exact_f32 ? h->w2a_critic : (const float*)h->w2pf_critic.get();
    a.mon_cur_ret = h->mon_cur_ret; a.mon_cur_len = h->mon_cur_len; a.ep_ret = h->ep_ret; a.ep_len = h->ep_len;
    return a;
}
int collect_rollout(dril_handle* h, double* fps, bool do_sync) {
    if (!h->env.ready) return fail(h, DRIL_ERR_NOT_INITIALISED, "dril_collect_rollout before dril_env_reset");
    { int rcw = ensure_wimg(h); if (rcw) return rcw; }
    if (!rollout_fused_applies(h)) {                                    // step-granular launches
        const auto t0s = std::chrono::steady_clock::now();
        if (fps) HIPCHK(h, hipStreamSynchronize(h->stream));
        prof_begin(h, DRIL_K_ROLLOUT);
        h->rollout_launches = 0; h->gws.launches = 0;
        if (h->fused_rollout) { const std::string why = fused_rollout_unavailable(h); if (!why.empty()) { prof_end(h); return fail(h, DRIL_ERR_UNSUPPORTED, "dril_collect_rollout with the fused rollout on: " + why); } }
        int rcs = h->env.module ? (h->fused_rollout ? collect_rollout_module_fused(h) : h->pn.on ? collect_rollout_module_norm(h) : collect_rollout_module(h)) : collect_rollout_stepwise(h);
        h->rollout_launches += h->gws.launches + (h->mon_cur_ret ? 1 : 0);
        prof_end(h);
        if (rcs) return rcs;
        if (fps) { HIPCHK(h, hipStreamSynchronize(h->stream)); const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0s).count(); *fps = (double)h->N / (dt > 0 ? dt : 1e-12); }
        h->noise_set = false;
        rcs = compute_gae(h); if (rcs) return rcs;
        return do_sync ? sync(h) : DRIL_OK;
    }
    const RolloutArgs a = rollout_args(h);
    const auto t0 = std::chrono::steady_clock::now();
    if (fps) HIPCHK(h, hipStreamSynchronize(h->stream));
    prof_begin(h, DRIL_K_ROLLOUT);
    HIPCHK(h, launch_rollout(h->env.kind, h->cfg.hidden1, a, h->stream));
    prof_end(h);
    if (fps) {   // fps = steps / wall time of collect_trajectories, rollout_buffer.jl:60-64
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *fps = (double)h->N / (dt > 0 ? dt : 1e-12);
    }
    h->noise_set = false;
    { int rcm = monitor_collect_rollout(h); if (rcm) return rcm; }
    int rc = compute_gae(h); if (rc) return rc;
    return do_sync ? sync(h) : DRIL_OK;
}
}  // namespace
DRIL_EXPORT int32_t dril_rollout_fused_enable(dril_handle* h, int32_t on) {
    NEED(h);
    if (on) {
        std::string why = fused_rollout_unavailable(h);
        if (why.empty() && h->pn.on) why = "NormalizeWrapperEnv is on (dril_normalize_enable): its running statistics couple all envs at every step, which is what a workgroup per tile of envs gives up; collect step-granular, or switch the wrapper off with dril_normalize_enable(h, NULL) first";
        if (!why.empty()) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_rollout_fused_enable: " + why);
    }
    h->fused_rollout = on != 0;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_rollout_fused_info(const dril_handle* h, dril_fused_rollout_info* out) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!out) return fail(const_cast<dril_handle*>(h), DRIL_ERR_INVALID_ARG, "dril_rollout_fused_info: null out pointer");
    std::memset(out, 0, sizeof(*out));
    const std::string why = fused_rollout_unavailable(h);
    out->available = why.empty() ? 1 : 0; out->enabled = h->fused_rollout ? 1 : 0; out->last_collection_launches = h->rollout_launches;
    if (h->env.module && h->env.rollout.has_desc) { out->tile = h->env.rollout.desc.tile; out->threads = h->env.rollout.desc.threads; out->max_width = h->env.rollout.desc.max_width; }
    std::snprintf(out->reason, sizeof(out->reason), "%s", why.c_str());
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_evaluate_fused_info(const dril_handle* h, dril_fused_evaluate_info* out) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!out) return fail(const_cast<dril_handle*>(h), DRIL_ERR_INVALID_ARG, "dril_evaluate_fused_info: null out pointer");
    std::memset(out, 0, sizeof(*out));
    const std::string why = fused_evaluate_unavailable(h);
    out->available = why.empty() ? 1 : 0;
    if (h->env.module && h->env.evaluate.has_desc) { out->tile = h->env.evaluate.desc.tile; out->threads = h->env.evaluate.desc.threads; out->max_width = h->env.evaluate.desc.max_width; }
    std::snprintf(out->reason, sizeof(out->reason), "%s", why.c_str());
    return DRIL_OK;
}
namespace {
// dril_ext_device_info counts per rollout: the first act of a rollout starts the counters again
void ext_count_begin(dril_handle* h) { if (h->ext_t == 0) { h->ext_steps_dev = h->ext_steps_host = h->ext_syncs = 0; h->ext_launches = 0; h->xw_added[0] = h->xw_added[1] = h->xw_added[2] = 0; } }
// the one drain of a rollout over external envs; the sticky error word of dril_ext_record_device comes back with it (a rollout may mix host and device verbs)
int ext_finish_drain(dril_handle* h, const char* verb) {
    HIPCHK(h, hipMemcpyAsync(h->ext_err_host, h->ext_err, 4, hipMemcpyDeviceToHost, h->stream));
    int rc = sync(h); if (rc) return rc;
    if (*h->ext_err_host) {
        *h->ext_err_host = 0;
        HIPCHK(h, hipMemsetAsync(h->ext_err, 0, 4, h->stream));
        return fail(h, DRIL_ERR_INVALID_ARG, std::string(verb) + ": dril_ext_record_device: truncated envs need terminal_obs (infos[i][\"terminal_observation\"], multithreadedParallelEnv.jl:64-66); the rollout is discarded");
    }
    return DRIL_OK;
}
// an argument of a device verb must be memory the handle's device can address, long enough for the array: a host pointer handed to a kernel is a GPU fault
int ext_check_ptr(dril_handle* h, const char* verb, const char* name, const void* p, size_t bytes) {
    const std::string msg = ext_ptr_problem(h->cfg.device, verb, name, p, bytes);         // dril_ext_stream.h: the rule the SAC handle's device verbs share
    return msg.empty() ? DRIL_OK : fail(h, DRIL_ERR_INVALID_ARG, msg);
}
}  // namespace
namespace dril::ppo {
// the handle's stream takes over from the caller's stream / hands back to it: two events per handle, no host wait
int ext_stream_enter(dril_handle* h, void* caller_stream) { HIPCHK(h, ext_stream_take(h->stream, h->ext_ev_in, caller_stream)); return DRIL_OK; }
int ext_stream_leave(dril_handle* h, void* caller_stream) { HIPCHK(h, ext_stream_give(h->stream, h->ext_ev_out, caller_stream)); return DRIL_OK; }
}  // namespace dril::ppo
namespace {
// the adapter's table of a Box handle as the actions-out kernel takes it (null: Discrete, or nothing to clamp)
const ExtBounds* ext_bounds_for(dril_handle* h, ExtBounds& scalar) {
    if (h->discrete) return nullptr;
    if (h->ext_bounds_set) return &h->ext_bounds;
    if (!(h->cfg.ext_action_low < h->cfg.ext_action_high)) return nullptr;
    for (int a = 0; a < h->A; ++a) { scalar.lo[a] = h->cfg.ext_action_low; scalar.hi[a] = h->cfg.ext_action_high; }
    return &scalar;
}

// a wrapper of dril_ext_normalize_enable / dril_ext_monitor_enable is on (dril_wrap.hip): the device verbs honour it, the host verbs refuse
bool xw_on(const dril_handle* h) { return h->pn.on || h->ext_mon_window > 0; }
#define XW_HOST_REFUSED(h, what) do { if (xw_on(h)) return fail(h, DRIL_ERR_UNSUPPORTED, what ": wrapper on: use the device verbs, or wrap the host env on the host (dril_ext_normalize_enable / dril_ext_monitor_enable are honoured by dril_ext_act_device / _record_device / _finish_device only)"); } while (0)
}  // namespace
// ---- collect_trajectories over HOST envs (DRIL_ENV_EXTERNAL), trajectory.jl:22-78: the caller steps its envs, the device does the rest ----
DRIL_EXPORT int32_t dril_ext_act(dril_handle* h, const float* obs, void* raw_actions, void* env_actions) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_act: the handle was not created with DRIL_ENV_EXTERNAL");
    XW_HOST_REFUSED(h, "dril_ext_act");
    if (!obs) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_act: null obs");
    if (h->ext_acted) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_act: the previous step has no dril_ext_record yet");
    if (h->ext_t >= h->cfg.n_steps) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_act: n_steps env steps are recorded; call dril_ext_finish");
    const size_t E = h->cfg.n_envs, D = h->D, A = h->A, ab = act_bytes_per(h), k = (size_t)h->ext_t * E;
    ext_count_begin(h); const int64_t l0 = h->gws.launches;
    HIPCHK(h, hipMemcpyAsync(h->obs + k * D, obs, E * D * 4, hipMemcpyHostToDevice, h->stream));                          // observation -> buffer, :46-47
    const void* nz = h->noise_set ? (const void*)((const char*)h->noise_dev + k * (h->discrete ? 8 : 4 * A)) : nullptr;
    PolicyArgs p = policy_args(h, h->obs + k * D, (int64_t)E, nz, (char*)h->act + k * ab, h->val + k, h->logp + k, nullptr, 0);     // get_action_and_values :41; raw action stored :48
    HIPCHK(h, run_policy(h, p));
    h->policy_calls += 1;
    void* first = raw_actions ? raw_actions : env_actions;                             // one device-to-host copy; the second output is a host copy of it
    if (first) HIPCHK(h, hipMemcpyAsync(first, (char*)h->act + k * ab, E * ab, hipMemcpyDeviceToHost, h->stream));
    h->ext_launches += h->gws.launches - l0;
    int rc = sync(h); if (rc) return rc;
    h->ext_syncs += 1;
    if (raw_actions && env_actions) std::memcpy(env_actions, raw_actions, E * ab);
    if (env_actions && !h->discrete && h->ext_bounds_set) {                                                               // the per-dimension table of dril_ext_set_action_bounds
        float* a = (float*)env_actions;
        for (size_t i = 0; i < E * A; ++i) { const float lo = h->ext_bounds.lo[i % A], hi = h->ext_bounds.hi[i % A]; if (lo < hi) a[i] = a[i] < lo ? lo : (a[i] > hi ? hi : a[i]); }
    } else
    if (env_actions && !h->discrete && h->cfg.ext_action_low < h->cfg.ext_action_high) {                                  // to_env(ClampAdapter) :42, default_adapters.jl:4-11; E * A floats, on the host
        float* a = (float*)env_actions; const float lo = h->cfg.ext_action_low, hi = h->cfg.ext_action_high;
        for (size_t i = 0; i < E * A; ++i) a[i] = a[i] < lo ? lo : (a[i] > hi ? hi : a[i]);
    }
    h->ext_acted = true;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_record(dril_handle* h, const float* rewards, const uint8_t* terminated, const uint8_t* truncated, const float* terminal_obs) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_record: the handle was not created with DRIL_ENV_EXTERNAL");
    XW_HOST_REFUSED(h, "dril_ext_record");
    if (!rewards || !terminated || !truncated) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_record: null rewards / terminated / truncated");
    if (!h->ext_acted) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_record without a preceding dril_ext_act");
    const size_t E = h->cfg.n_envs, D = h->D, k = (size_t)h->ext_t * E;
    float* srew = h->ext_stage_rew + k; uint8_t* fl = h->ext_stage_flags + k;     // this step's slot of the pinned staging area: not reused before the next rollout
    std::vector<int> tr;
    for (size_t e = 0; e < E; ++e) { fl[e] = (uint8_t)((terminated[e] ? 1 : 0) | (truncated[e] ? 2 : 0)); if (truncated[e]) tr.push_back((int)e); }
    if (!tr.empty() && !terminal_obs) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_record: truncated envs need terminal_obs (infos[i][\"terminal_observation\"], multithreadedParallelEnv.jl:64-66)");
    std::memcpy(srew, rewards, E * 4);
    HIPCHK(h, hipMemcpyAsync(h->rew + k, srew, E * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->flags + k, fl, E, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->boot + k, 0, E * 4, h->stream));
    if (!tr.empty()) {                                                                // V(terminal_observation) of the truncated envs only, trajectory.jl:57-61
        const size_t n = tr.size();
        std::vector<float> tobs(n * D), bv(n), row(E, 0.f);
        for (size_t j = 0; j < n; ++j) std::memcpy(&tobs[j * D], terminal_obs + (size_t)tr[j] * D, D * 4);
        HIPCHK(h, hipMemcpyAsync(h->e_tobs, tobs.data(), n * D * 4, hipMemcpyHostToDevice, h->stream));
        PolicyArgs p = policy_args(h, h->e_tobs, (int64_t)n, nullptr, nullptr, h->e_rew, nullptr, nullptr, 2);
        const int64_t l0 = h->gws.launches;
        HIPCHK(h, run_policy(h, p));
        h->ext_launches += h->gws.launches - l0;
        HIPCHK(h, hipMemcpyAsync(bv.data(), h->e_rew, n * 4, hipMemcpyDeviceToHost, h->stream));
        int rc = sync(h); if (rc) return rc;                                          // host temporaries: drain before they go out of scope
        for (size_t j = 0; j < n; ++j) row[tr[j]] = bv[j];
        HIPCHK(h, hipMemcpyAsync(h->boot + k, row.data(), E * 4, hipMemcpyHostToDevice, h->stream));
        rc = sync(h); if (rc) return rc;
        h->ext_syncs += 2;
    }
    // no truncation: nothing to wait for — the copies read the pinned slot and complete behind the next dril_ext_act
    h->ext_t += 1; h->ext_acted = false; h->ext_steps_host += 1;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_finish(dril_handle* h, const float* last_obs) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_finish: the handle was not created with DRIL_ENV_EXTERNAL");
    XW_HOST_REFUSED(h, "dril_ext_finish");
    if (!last_obs) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_finish: null last_obs");
    if (h->ext_acted || h->ext_t != h->cfg.n_steps) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_finish: the rollout needs exactly n_steps act/record pairs");
    const size_t E = h->cfg.n_envs, D = h->D;
    HIPCHK(h, hipMemcpyAsync(h->e_obs, last_obs, E * D * 4, hipMemcpyHostToDevice, h->stream));
    PolicyArgs p = policy_args(h, h->e_obs, (int64_t)E, nullptr, nullptr, h->last_values, nullptr, nullptr, 2);          // V(new_obs) where the last step left the trajectory open, :65-70
    const int64_t l0 = h->gws.launches;
    HIPCHK(h, run_policy(h, p));
    h->ext_launches += h->gws.launches - l0 + 1;
    h->ext_t = 0; h->noise_set = false;
    int rc = compute_gae(h); if (rc) return rc;                                       // compute_advantages! + returns, rollout_buffer.jl:83-87
    return ext_finish_drain(h, "dril_ext_finish");
}
DRIL_EXPORT int32_t dril_ext_steps(const dril_handle* h) { return h ? h->ext_t : -1; }

// ---- the same three verbs on DEVICE arrays: no copy across PCIe, no drain before dril_ext_finish_device (include/dril_hip.h) ----
DRIL_EXPORT int32_t dril_ext_act_device(dril_handle* h, const float* d_obs, void* d_raw_actions, void* d_env_actions, void* caller_stream) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_act_device: the handle was not created with DRIL_ENV_EXTERNAL");
    if (!d_obs) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_act_device: null obs");
    if (h->ext_acted) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_act_device: the previous step has no dril_ext_record yet");
    if (h->ext_t >= h->cfg.n_steps) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_act_device: n_steps env steps are recorded; call dril_ext_finish");
    const size_t E = h->cfg.n_envs, D = h->D, A = h->A, ab = act_bytes_per(h), k = (size_t)h->ext_t * E;
    int rc = ext_check_ptr(h, "dril_ext_act_device", "d_obs", d_obs, E * D * 4); if (rc) return rc;
    if (d_raw_actions) { rc = ext_check_ptr(h, "dril_ext_act_device", "d_raw_actions", d_raw_actions, E * ab); if (rc) return rc; }
    if (d_env_actions) { rc = ext_check_ptr(h, "dril_ext_act_device", "d_env_actions", d_env_actions, E * ab); if (rc) return rc; }
    ext_count_begin(h); const int64_t l0 = h->gws.launches;
    rc = ext_stream_enter(h, caller_stream); if (rc) return rc;
    if (h->pn.on) {                                                                   // the wrapper's observe: raw -> old_obs and the normalised row in one pass (no copy)
        int64_t added = 0;
        rc = xn_observe(h, d_obs, (int64_t)E, h->obs + k * D, true, &added); if (rc) return rc;
        h->ext_launches += added; h->xw_added[0] += added;
    } else
    HIPCHK(h, hipMemcpyAsync(h->obs + k * D, d_obs, E * D * 4, hipMemcpyDefault, h->stream));                               // observation -> buffer, :46-47
    const void* nz = h->noise_set ? (const void*)((const char*)h->noise_dev + k * (h->discrete ? 8 : 4 * A)) : nullptr;
    PolicyArgs p = policy_args(h, h->obs + k * D, (int64_t)E, nz, (char*)h->act + k * ab, h->val + k, h->logp + k, nullptr, 0);     // the host verb's forward: the same bits
    HIPCHK(h, run_policy(h, p));
    h->policy_calls += 1;
    h->ext_launches += h->gws.launches - l0;
    if (d_raw_actions || d_env_actions) {                                                                                   // to_env(ClampAdapter) :42 on the device
        ExtBounds scalar; const ExtBounds* b = ext_bounds_for(h, scalar);
        HIPCHK(h, launch_ext_actions_out((char*)h->act + k * ab, d_raw_actions, d_env_actions, (int64_t)E, (int)A, h->discrete ? 1 : 0, b, h->stream));
        h->ext_launches += 1;
    }
    rc = ext_stream_leave(h, caller_stream); if (rc) return rc;
    h->ext_acted = true;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_record_device(dril_handle* h, const float* d_rewards, const uint8_t* d_terminated, const uint8_t* d_truncated, const float* d_terminal_obs, void* caller_stream) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_record_device: the handle was not created with DRIL_ENV_EXTERNAL");
    if (!d_rewards || !d_terminated || !d_truncated) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_record_device: null rewards / terminated / truncated");
    if (!h->ext_acted) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_record_device without a preceding dril_ext_act");
    const size_t E = h->cfg.n_envs, D = h->D, k = (size_t)h->ext_t * E;
    int rc = ext_check_ptr(h, "dril_ext_record_device", "d_rewards", d_rewards, E * 4); if (rc) return rc;
    rc = ext_check_ptr(h, "dril_ext_record_device", "d_terminated", d_terminated, E); if (rc) return rc;
    rc = ext_check_ptr(h, "dril_ext_record_device", "d_truncated", d_truncated, E); if (rc) return rc;
    if (d_terminal_obs) { rc = ext_check_ptr(h, "dril_ext_record_device", "d_terminal_obs", d_terminal_obs, E * D * 4); if (rc) return rc; }
    rc = ext_stream_enter(h, caller_stream); if (rc) return rc;
    if (xw_on(h)) {                                                                   // a wrapper on: act! of the wrapper and the record in one kernel, then V(normalised terminal_observation) selected into boot[t]
        const float* tobs_norm = nullptr; int64_t own = 0;
        rc = xn_record(h, k, d_rewards, d_terminated, d_truncated, d_terminal_obs, &tobs_norm, &own); if (rc) return rc;
        const int64_t l0 = h->gws.launches;
        if (tobs_norm) {
            PolicyArgs p = policy_args(h, tobs_norm, (int64_t)E, nullptr, nullptr, h->gen_tmp, nullptr, nullptr, 2);
            HIPCHK(h, run_policy(h, p));
            HIPCHK(h, generic_select((int64_t)E, d_truncated, h->gen_tmp, h->boot + k, h->stream));
            own += 1;
        }
        h->ext_launches += h->gws.launches - l0 + own; h->xw_added[1] += own - 1;      // (the unwrapped verb's one launch of its own is ext_record_kernel)
        rc = ext_stream_leave(h, caller_stream); if (rc) return rc;
        h->ext_t += 1; h->ext_acted = false; h->ext_steps_dev += 1;
        return DRIL_OK;
    }
    if (d_terminal_obs) {                                                             // V(terminal_observation), trajectory.jl:57-61: the critic over all E columns, kept where truncated
        const int64_t l0 = h->gws.launches;
        PolicyArgs p = policy_args(h, d_terminal_obs, (int64_t)E, nullptr, nullptr, h->gen_tmp, nullptr, nullptr, 2);
        HIPCHK(h, run_policy(h, p));
        h->ext_launches += h->gws.launches - l0;
    }
    HIPCHK(h, launch_ext_record((int)E, d_rewards, d_terminated, d_truncated, d_terminal_obs ? h->gen_tmp : nullptr, h->rew + k, h->flags + k, h->boot + k, h->ext_err, h->stream));
    h->ext_launches += 1;
    rc = ext_stream_leave(h, caller_stream); if (rc) return rc;
    h->ext_t += 1; h->ext_acted = false; h->ext_steps_dev += 1;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_finish_device(dril_handle* h, const float* d_last_obs, void* caller_stream) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_finish_device: the handle was not created with DRIL_ENV_EXTERNAL");
    if (!d_last_obs) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_finish_device: null last_obs");
    if (h->ext_acted || h->ext_t != h->cfg.n_steps) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_finish_device: the rollout needs exactly n_steps act/record pairs");
    const size_t E = h->cfg.n_envs, D = h->D;
    int rc = ext_check_ptr(h, "dril_ext_finish_device", "d_last_obs", d_last_obs, E * D * 4); if (rc) return rc;
    rc = ext_stream_enter(h, caller_stream); if (rc) return rc;
    if (h->pn.on) {                                                                   // one more observe of the wrapper
        int64_t added = 0;
        rc = xn_observe(h, d_last_obs, (int64_t)E, h->e_obs, true, &added); if (rc) return rc;
        h->ext_launches += added; h->xw_added[2] += added;
    } else
    HIPCHK(h, hipMemcpyAsync(h->e_obs, d_last_obs, E * D * 4, hipMemcpyDefault, h->stream));
    PolicyArgs p = policy_args(h, h->e_obs, (int64_t)E, nullptr, nullptr, h->last_values, nullptr, nullptr, 2);          // V(new_obs) where the last step left the trajectory open, :65-70
    const int64_t l0 = h->gws.launches;
    HIPCHK(h, run_policy(h, p));
    h->ext_launches += h->gws.launches - l0 + 1;
    h->ext_t = 0; h->noise_set = false;
    rc = compute_gae(h); if (rc) return rc;                                           // compute_advantages! + returns, rollout_buffer.jl:83-87
    if (h->ext_mon_window > 0) {                                                      // MonitorWrapperEnv: this rollout's finished episodes enter the window in (step, env) order
        HIPCHK(h, launch_monitor_collect(h->flags, h->ep_ret, h->ep_len, h->cfg.n_envs, h->cfg.n_steps, h->ext_mon_window, h->mon_cnt, h->mon_ring_ret, h->mon_ring_len, h->mon_meta, h->stream));
        h->ext_launches += 2; h->xw_added[2] += 2;                                    // (its count and its collect kernel)
    }
    return ext_finish_drain(h, "dril_ext_finish_device");                             // the drain covers the read of d_last_obs: nothing for caller_stream to wait for
}
DRIL_EXPORT int32_t dril_predict_actions_device(dril_handle* h, const float* d_obs, int64_t batch, int32_t deterministic, void* d_raw_actions, void* d_env_actions, void* caller_stream) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_predict_actions_device: the handle was not created with DRIL_ENV_EXTERNAL");
    if (!d_obs || batch < 1) return fail(h, DRIL_ERR_INVALID_ARG, "dril_predict_actions_device: null obs or batch < 1");
    if (!d_raw_actions && !d_env_actions) return fail(h, DRIL_ERR_INVALID_ARG, "dril_predict_actions_device: null actions");
    const size_t B = (size_t)batch, ab = act_bytes_per(h);
    int rc = ext_check_ptr(h, "dril_predict_actions_device", "d_obs", d_obs, B * h->D * 4); if (rc) return rc;
    if (d_raw_actions) { rc = ext_check_ptr(h, "dril_predict_actions_device", "d_raw_actions", d_raw_actions, B * ab); if (rc) return rc; }
    if (d_env_actions) { rc = ext_check_ptr(h, "dril_predict_actions_device", "d_env_actions", d_env_actions, B * ab); if (rc) return rc; }
    HIPCHK(h, h->ext_pred_act.grow(B * ab)); HIPCHK(h, h->ext_pred_lp.grow(B));           // grow-only scratch: the head kernel's actions and log-probabilities (a free waits for the device)
    const bool nz_eval = h->pn.on && h->pn.cfg.norm_obs;                               // evaluation under the wrapper: the statistics in force, never updated
    if (nz_eval && batch > h->cfg.n_envs) {                                            // (up to n_envs rows fit e_obs; more: grow-only scratch, counted by dril_ext_wrap_info)
        bool grew; HIPCHK(h, h->ext_pred_obs.grow(B * h->D, &grew));
        if (grew) h->xw_allocs += 1;
    }
    rc = ext_stream_enter(h, caller_stream); if (rc) return rc;
    if (nz_eval) {
        float* scratch = batch > h->cfg.n_envs ? h->ext_pred_obs : h->e_obs; int64_t added = 0;
        rc = xn_observe(h, d_obs, batch, scratch, false, &added); if (rc) return rc;
        d_obs = scratch;
    }
    PolicyArgs a = policy_args(h, d_obs, batch, nullptr, h->ext_pred_act, nullptr, h->ext_pred_lp, nullptr, 0);
    a.deterministic = deterministic ? 1 : 0;
    HIPCHK(h, run_policy(h, a));
    h->policy_calls += 1;
    ExtBounds scalar; const ExtBounds* b = ext_bounds_for(h, scalar);
    HIPCHK(h, launch_ext_actions_out(h->ext_pred_act, d_raw_actions, d_env_actions, batch, h->A, h->discrete ? 1 : 0, b, h->stream));
    return ext_stream_leave(h, caller_stream);
}
DRIL_EXPORT int32_t dril_ext_set_action_bounds(dril_handle* h, const float* low, const float* high) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_set_action_bounds: the handle was not created with DRIL_ENV_EXTERNAL");
    if (h->discrete) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_set_action_bounds: a Discrete action space has no bounds to clamp to");
    if (!low && !high) { h->ext_bounds_set = false; return DRIL_OK; }
    if (!low || !high) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_set_action_bounds: null low / high");
    for (int a = 0; a < h->A; ++a) { h->ext_bounds.lo[a] = low[a]; h->ext_bounds.hi[a] = high[a]; }
    h->ext_bounds_set = true;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_device_info(const dril_handle* h, struct dril_ext_device_info* out) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!out) return DRIL_ERR_INVALID_ARG;
    if (!h->external) return DRIL_ERR_UNSUPPORTED;
    std::memset(out, 0, sizeof(*out));
    out->steps_device = h->ext_steps_dev; out->steps_host = h->ext_steps_host; out->host_syncs = h->ext_syncs; out->per_dim_bounds = h->ext_bounds_set ? 1 : 0;
    out->launches = h->ext_launches;
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_collect_rollout(dril_handle* h, double* fps) { NEED(h); NOT_EXTERNAL(h, "dril_collect_rollout"); return collect_rollout(h, fps, true); }
DRIL_EXPORT int32_t dril_debug_set_noise(dril_handle* h, const void* noise, size_t count) {
    NEED(h);
    if (!noise) { h->noise_set = false; return DRIL_OK; }
    const size_t need = (size_t)h->N * (h->discrete ? 1 : (size_t)h->A);
    if (count != need) return fail(h, DRIL_ERR_INVALID_ARG, "dril_debug_set_noise: count must be n_envs*n_steps (*action_dim)");
    const size_t bytes = need * (h->discrete ? 8 : 4);
    if (!h->noise_dev) HIPCHK(h, h->noise_dev.alloc(bytes));
    HIPCHK(h, hipMemcpyAsync(h->noise_dev, noise, bytes, hipMemcpyHostToDevice, h->stream));
    h->noise_set = true;
    return sync(h);
}
DRIL_EXPORT int32_t dril_buffer_copy_out(dril_handle* h, int32_t which, void* host, size_t bytes) {
    NEED(h); size_t b; void* p = buf_ptr(h, which, &b);
    if (!p || !host || b != bytes) return fail(h, DRIL_ERR_INVALID_ARG, "dril_buffer_copy_out: bad id or byte count");
    HIPCHK(h, hipMemcpyAsync(host, p, b, hipMemcpyDeviceToHost, h->stream)); return sync(h);
}
DRIL_EXPORT int32_t dril_buffer_copy_in(dril_handle* h, int32_t which, const void* host, size_t bytes) {
    NEED(h); size_t b; void* p = buf_ptr(h, which, &b);
    if (!p || !host || b != bytes) return fail(h, DRIL_ERR_INVALID_ARG, "dril_buffer_copy_in: bad id or byte count");
    HIPCHK(h, hipMemcpyAsync(p, host, b, hipMemcpyHostToDevice, h->stream)); return sync(h);
}
DRIL_EXPORT int32_t dril_compute_gae(dril_handle* h) {
    NEED(h); int rc = compute_gae(h); if (rc) return rc;
    int gave_up = 0; HIPCHK(h, hipMemcpyAsync(&gave_up, h->gae_err, 4, hipMemcpyDeviceToHost, h->stream));
    rc = sync(h); if (rc) return rc;
    if (gave_up) { (void)hipMemsetAsync(h->gae_err, 0, 4, h->stream); return fail(h, DRIL_ERR_HIP, "gae_scan_kernel: a chunk's predecessor did not publish its carry within the spin limit"); }
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_gae(int32_t E, int32_t T, float gamma, float lam, const float* rewards, const float* values, const uint8_t* flags,
                             const float* bootstrap, const float* last_values, float* advantages, float* returns) {
    if (E < 1 || T < 1 || !rewards || !values || !flags || !bootstrap || !last_values || !advantages || !returns)
        return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_gae: bad argument");
    const size_t N = (size_t)E * T;
    DevBuf<float> d_r, d_v, d_b, d_l, d_a, d_ret; DevBuf<uint8_t> d_f; DevBuf<unsigned long long> d_c; DevBuf<int> d_e;
    HIPCHK(nullptr, d_r.alloc(N)); HIPCHK(nullptr, d_v.alloc(N)); HIPCHK(nullptr, d_b.alloc(N)); HIPCHK(nullptr, d_l.alloc((size_t)E)); HIPCHK(nullptr, d_a.alloc(N)); HIPCHK(nullptr, d_ret.alloc(N)); HIPCHK(nullptr, d_f.alloc(N));
    HIPCHK(nullptr, hipMemcpy(d_r, rewards, N * 4, hipMemcpyHostToDevice)); HIPCHK(nullptr, hipMemcpy(d_v, values, N * 4, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_b, bootstrap, N * 4, hipMemcpyHostToDevice)); HIPCHK(nullptr, hipMemcpy(d_l, last_values, (size_t)E * 4, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_f, flags, N, hipMemcpyHostToDevice));
    const size_t words = (size_t)gae_chunks(T) * E; int gave_up = 0;
    HIPCHK(nullptr, d_c.alloc(words)); HIPCHK(nullptr, hipMemset(d_c, 0, words * 8)); HIPCHK(nullptr, d_e.alloc(1)); HIPCHK(nullptr, hipMemset(d_e, 0, 4));
    HIPCHK(nullptr, launch_gae(E, T, gamma, lam, d_r, d_v, d_f, d_b, d_l, d_a, d_ret, d_c, 1u, d_e, nullptr));
    HIPCHK(nullptr, hipDeviceSynchronize());
    HIPCHK(nullptr, hipMemcpy(&gave_up, d_e, 4, hipMemcpyDeviceToHost));
    if (gave_up) return fail(nullptr, DRIL_ERR_HIP, "gae_scan_kernel: a chunk's predecessor did not publish its carry within the spin limit");
    HIPCHK(nullptr, hipMemcpy(advantages, d_a, N * 4, hipMemcpyDeviceToHost)); HIPCHK(nullptr, hipMemcpy(returns, d_ret, N * 4, hipMemcpyDeviceToHost));
    return DRIL_OK;
}

// ---- PPO update ------------------------------------------------------------------------------------
DRIL_EXPORT int32_t dril_debug_set_permutation(dril_handle* h, const int64_t* perm, size_t count) {
    NEED(h);
    if (!perm) { h->perm_count = 0; return DRIL_OK; }
    const size_t need = (size_t)h->cfg.epochs * (size_t)h->N;
    if (count != need) return fail(h, DRIL_ERR_INVALID_ARG, "dril_debug_set_permutation: count must be epochs * n_envs * n_steps");
    for (size_t i = 0; i < count; ++i) if (perm[i] < 0 || perm[i] >= h->N) return fail(h, DRIL_ERR_INVALID_ARG, "dril_debug_set_permutation: index out of range");
    if (!h->perm_dev) HIPCHK(h, h->perm_dev.alloc(need));
    HIPCHK(h, hipMemcpyAsync(h->perm_dev, perm, need * 8, hipMemcpyHostToDevice, h->stream));
    h->perm_count = need;
    return sync(h);
}

namespace {
// One update in the pieces that ppo_update_once runs in order, and that a population (dril_population_ppo_update) runs member by member around ONE batched launch:
//   update_begin (sizes, memsets, packed records) -> [small_update_args + the persistent kernel | the per-step kernels] -> update_enqueue_home (explained variance,
//   max |W2|, the copies home) -> the stream drained -> update_finish (the statistics, the handle's counters, the status)
struct UpdatePlan { int world = 1; int64_t N = 0, B = 0, nb = 0, total_steps = 0; uint64_t adam_steps0 = 0; int bits = 0; };
// where an update's results land on the host: st [total_steps][16], ev [4 ev_blocks], scal = {nan flag, gae give-up flag, max |W2| bits}, keys [epochs].  Storage is the
// caller's and must not move before update_finish: vectors for a solo update, one pinned block per member in a population
struct UpdateHome { float* st = nullptr; double* ev = nullptr; int* scal = nullptr; uint64_t* keys = nullptr; };
UpdatePlan update_plan(const dril_handle* h) {
    UpdatePlan p;
    p.world = comm_ready(h) ? h->cfg.world_size : 1;
    p.N = h->N; p.B = h->cfg.batch_size / h->cfg.world_size;
    p.nb = (p.N + p.B - 1) / p.B;                             // partial last batch kept (MLUtils partial=true)
    p.total_steps = p.nb * h->cfg.epochs;
    p.adam_steps0 = h->adam_steps; p.bits = perm_bits(p.N);
    return p;
}
// the reference's default PPO() (batch_size = 64) on hidden [64,64]: every optimiser step of the iteration inside ONE launch of two persistent workgroups, one per net (dril_update_small.hip);
// single-rank only (a data-parallel run all-reduces between the gradient and the step)
bool small_persistent_applies(const dril_handle* h, const UpdatePlan& p) {
    return !h->wide && !h->generic && h->cfg.hidden1 == 64 && h->D <= 8 && p.world == 1 && !(comm_ready(h) && h->force_allreduce) && h->rec && p.B >= 2 && p.B <= 64 && h->P <= 2 * 256 * 19 &&
           !h->no_persistent && !h->no_small_path && h->grad_variant < 0 && p.total_steps > 0;   // (DRIL_GRAD_VARIANT pins one of the per-step kernels)
}
int update_begin(dril_handle* h, const UpdatePlan& p) {
    const int64_t total_steps = p.total_steps;
    h->used_f16 = false; h->spin_timeout = false;
    if (total_steps > 0) HIPCHK(h, h->step_stats.grow((size_t)total_steps * 16));
    if (total_steps > 0) HIPCHK(h, hipMemsetAsync(h->step_stats, 0, (size_t)total_steps * 16 * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(h->stop_flag, 0, 4, h->stream)); HIPCHK(h, hipMemsetAsync(h->nan_flag, 0, 4, h->stream));
    if (h->rec) { prof_begin(h, DRIL_K_PACK_RECORDS); HIPCHK(h, launch_pack_records(h->cfg.env_kind, p.N, h->obs, h->act, h->adv, h->logp, h->ret, h->rec, h->stream)); prof_end(h); }
    return DRIL_OK;
}
// the persistent kernel's argument block (step0 / nsteps / step_parity / xchg are the launch's: the caller sets them); keys[epochs] goes to the device on the handle's
// stream and must stay alive until that copy has run
int small_update_args(dril_handle* h, const UpdatePlan& p, uint64_t* keys, SmallUpdateArgs& u) {
    if (h->cfg.epochs > 0) HIPCHK(h, h->epoch_keys.grow((size_t)h->cfg.epochs));
    for (int ep = 0; ep < h->cfg.epochs; ++ep) keys[ep] = perm_key(h->cfg.seed + (uint64_t)h->cfg.rank, h->update_counter, ep);
    HIPCHK(h, hipMemcpyAsync(h->epoch_keys, keys, (size_t)h->cfg.epochs * 8, hipMemcpyHostToDevice, h->stream));
    u = SmallUpdateArgs{};
    u.params = h->params; u.adam_m = h->adam_m; u.adam_v = h->adam_v; u.bt = h->bt; u.step_parity = (int)(h->adam_steps & 1);
    u.rec = h->rec; u.val_old = h->val; u.perm = h->perm_count ? h->perm_dev : nullptr; u.keys = h->epoch_keys; u.perm_bits = p.bits;
    u.N = p.N; u.B = p.B; u.nb = (int)p.nb; u.step_stats = h->step_stats; u.norm_out = h->norm_out; u.nan_flag = h->nan_flag; u.stop_flag = h->stop_flag;
    u.lr = h->lr; u.beta1 = h->cfg.adam_beta1; u.beta2 = h->cfg.adam_beta2; u.eps = h->cfg.adam_eps; u.max_grad_norm = h->cfg.max_grad_norm;
    u.target_kl = h->cfg.target_kl; u.ent_coef = h->cfg.ent_coef; u.vf_coef = h->cfg.vf_coef; u.clip_range = h->cfg.clip_range; u.clip_range_vf = h->cfg.clip_range_vf;
    u.has_max_grad_norm = h->cfg.has_max_grad_norm; u.has_target_kl = h->cfg.has_target_kl; u.has_clip_vf = h->cfg.has_clip_range_vf;
    u.normalize_adv = h->cfg.normalize_advantage; u.action_start = h->cfg.action_start; u.P = h->P; u.Pa = h->Pa; u.Pc = h->Pc; u.dbg = h->dbg;
    return DRIL_OK;
}
// the launch that starts at step s0 of the chunked sequence: at most chunk (h->small_chunk) optimiser steps per launch (16 384: a bound on one kernel's run time, ~0.2 s)
void small_update_chunk(const UpdatePlan& p, int64_t chunk, int64_t s0, SmallUpdateArgs& u) {
    u.step0 = (int)s0; u.nsteps = (int)(p.total_steps - s0 < chunk ? p.total_steps - s0 : chunk);
    u.step_parity = s0 == 0 ? (int)(p.adam_steps0 & 1) : 0;                           // (the kernel leaves both ping-pong slots of the beta powers equal)
}
// what the persistent kernel's launches leave on the host side of the handle
void small_update_done(dril_handle* h, const UpdatePlan& p) { h->adam_steps += p.total_steps; h->wimg_dirty = true; h->last_variant = 6; h->used_f16 = true; }
int update_enqueue_home(dril_handle* h, const UpdatePlan& p, const UpdateHome& home) {
    h->update_counter += 1;
    prof_begin(h, DRIL_K_EXPLAINED_VAR);
    HIPCHK(h, launch_explained_var(h->val, h->ret, p.N, h->ev_partials, h->ev_blocks, h->stream));
    prof_end(h);
    home.scal[0] = 0; home.scal[1] = 0; home.scal[2] = 0;
    if (!h->generic) {    // max |W2| of the parameters this update leaves behind rides home with its statistics (fwd_exact: the next rollout's arithmetic)
        HIPCHK(h, launch_w2_absmax(h->params, h->actor, h->critic, h->cfg.hidden1, h->w2max_dev, h->stream));
        HIPCHK(h, hipMemcpyAsync(&home.scal[2], h->w2max_dev, 4, hipMemcpyDeviceToHost, h->stream));
    }
    if (p.total_steps > 0) HIPCHK(h, hipMemcpyAsync(home.st, h->step_stats, (size_t)p.total_steps * 16 * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(home.ev, h->ev_partials, 4 * (size_t)h->ev_blocks * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&home.scal[0], h->nan_flag, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&home.scal[1], h->gae_err, 4, hipMemcpyDeviceToHost, h->stream));
    return DRIL_OK;
}
// the stream is drained: the statistics of the update, the handle's counters and the status
int update_finish(dril_handle* h, const UpdatePlan& p, const UpdateHome& home, dril_ppo_stats* out) {
    const int world = p.world; const int64_t N = p.N, total_steps = p.total_steps; const uint64_t adam_steps0 = p.adam_steps0;
    const float* st = home.st; const double* ev = home.ev;
    const int nan = home.scal[0], gae_gave_up = home.scal[1]; unsigned w2bits; std::memcpy(&w2bits, &home.scal[2], 4);
    int rc = DRIL_OK;
    // (a rank-local early return here would leave the other ranks of a data-parallel job alone in the collectives that follow — they saw this rank's NaN advantages in the
    // all-reduced gradient and start the exact-f32 redo: the flag is folded into the explained-variance all-reduce below, and every rank returns the same code at the same point)
    if (gae_gave_up && world == 1) { (void)hipMemsetAsync(h->gae_err, 0, 4, h->stream); return fail(h, DRIL_ERR_HIP, "gae_scan_kernel: a chunk's predecessor did not publish its carry within the spin limit (advantages of this rollout are NaN)"); }
    if (!h->generic) { float m; std::memcpy(&m, &w2bits, 4); h->w2max = (m == m) ? m : INFINITY; }
#ifdef DRIL_STAMPS
    {   // shares of the LAST grad launch, averaged over waves, per head
        std::vector<unsigned long long> d((size_t)2 * h->Gmax * 4 * 12);
        hipMemcpy(d.data(), h->dbg, d.size() * 8, hipMemcpyDeviceToHost);
        const char* names_f32[] = {"gather/loop", "L1+tanh", "L2+tanh", "out+head", "dW3 block", "dz2", "h1img+dh1+dz1", "dW2 block", "dW1 block", "-"};
        const char* names_split[] = {"S1 unpack+L1", "S2 tanh+split+L2+tanh", "S3 L3+head+dW3", "S4 dz2+split+dh1+mask", "S5 dW2", "S6 dz1 img+dW1", "-", "-", "-", "-"};
        // ppo_grad_wide_split_kernel (round 5; per pass of kWideSplitNT x 32 samples)
        const char* names_wide[] = {"L1+tanh+h1 pieces", "wait B1", "L2 chain+tanh", "out partials+wait B2", "head+dW3+dz2+pieces", "wait B3", "dh1 chain", "loader+dz1+dW1", "dW2 chain", "wait B4 (+DMA)"};
        const char** names = std::getenv("DRIL_GRAD_VARIANT") && std::atoi(std::getenv("DRIL_GRAD_VARIANT")) == 0 ? names_f32 : h->wide ? names_wide : names_split;
        for (int head = 0; head < 3; ++head) {
            double acc[10] = {0}; double tiles = 0; int nw = 0;
            for (size_t w = 0; w < d.size() / 12; ++w) if (d[w * 12 + 10] > 0 && (int)d[w * 12 + 11] == head) { for (int k = 0; k < 10; ++k) acc[k] += (double)d[w * 12 + k]; tiles += (double)d[w * 12 + 10]; ++nw; }
            if (!nw) continue;
            double tot = 0; for (int k = 0; k < 10; ++k) tot += acc[k];
            fprintf(stderr, "[stamps] head %d: %d waves, %.0f tiles/wave, %.0f ticks/tile (s_memtime ticks)\n", head, nw, tiles / nw, tot / tiles);
            for (int k = 0; k < 10; ++k) fprintf(stderr, "   %-22s %8.0f ticks/tile  %5.1f %%\n", names[k], acc[k] / tiles, 100.0 * acc[k] / tot);
        }
    }
#endif
    // per-iteration means over the applied steps (ppo.jl:242-264); grad_norm also counts the KL-stopped step (:223)
    double acc[8] = {0}; int n_upd = 0, n_gn = 0, stopped = 0; float ratio_first = 0;
    for (int64_t s = 0; s < total_steps; ++s) {
        const float* o = &st[(size_t)s * 16];
        if (s == 0) ratio_first = o[6];
        if (o[9] == 1.0f) { acc[0] += o[2]; acc[1] += o[0]; acc[2] += o[1]; acc[3] += o[4]; acc[4] += o[3]; acc[5] += o[7]; acc[6] += o[8]; acc[7] += o[5]; ++n_upd; ++n_gn; }
        else if (o[11] == 1.0f) { acc[6] += o[8]; ++n_gn; stopped = 1; break; }
        else if (o[10] == 1.0f) break;
    }
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int i = 0; i < h->ev_blocks; ++i) { s0 += ev[4 * i]; s1 += ev[4 * i + 1]; s2 += ev[4 * i + 2]; s3 += ev[4 * i + 3]; }
    double nn = (double)N;
    if (world > 1) {   // explained variance over all shards: tiny host-free all-reduce of the four sums
        double v[6] = {s0, s1, s2, s3, nn, gae_gave_up ? 1.0 : 0.0}; double* d = h->adv_stats;   // reuse the 4-double scratch + norm scratch is too small: use ev_partials
        HIPCHK(h, hipMemcpyAsync(h->ev_partials, v, sizeof(v), hipMemcpyHostToDevice, h->stream)); (void)d;
        rc = rccl_allreduce(h, h->ev_partials, 6, kNcclFloat64); if (rc) return rc;
        HIPCHK(h, hipMemcpyAsync(v, h->ev_partials, sizeof(v), hipMemcpyDeviceToHost, h->stream));
        rc = sync(h); if (rc) return rc;
        s0 = v[0]; s1 = v[1]; s2 = v[2]; s3 = v[3]; nn = v[4];
        if (v[5] > 0.0) {                                                  // some rank's GAE scan gave up: every rank reports it, at this same point
            if (gae_gave_up) (void)hipMemsetAsync(h->gae_err, 0, 4, h->stream);
            return fail(h, DRIL_ERR_HIP, gae_gave_up ? "gae_scan_kernel: a chunk's predecessor did not publish its carry within the spin limit (advantages of this rollout are NaN)"
                                                     : "gae_scan_kernel gave up on another rank of the data-parallel job (its advantages are NaN): the update is invalid on every rank");
        }
    }
    const double var_d = (s1 - s0 * s0 / nn) / (nn - 1.0), var_r = (s3 - s2 * s2 / nn) / (nn - 1.0);
    h->adam_steps = adam_steps0 + (uint64_t)n_upd;     // the steps the device APPLIED (a KL stop or a non-finite gradient skips the rest; the stopping step leaves both slots of the beta powers equal, so the parity is free)
    if (out) {
        std::memset(out, 0, sizeof(*out));
        const double den = n_upd > 0 ? n_upd : 1, gden = n_gn > 0 ? n_gn : 1;
        out->entropy_loss = (float)(acc[0] / den); out->policy_loss = (float)(acc[1] / den); out->value_loss = (float)(acc[2] / den);
        out->approx_kl_div = (float)(acc[3] / den); out->clip_fraction = (float)(acc[4] / den); out->loss = (float)(acc[5] / den);
        out->grad_norm = (float)(acc[6] / gden); out->entropy = (float)(acc[7] / den);
        out->explained_variance = (float)(1.0 - var_d / var_r); out->ratio_first = ratio_first;
        out->n_updates = n_upd; out->early_stopped = stopped; out->nan_or_inf = nan;
    }
    if (nan == 2) { h->spin_timeout = true; return fail(h, DRIL_ERR_HIP, "ppo_update_small_kernel: the partner workgroup did not answer within the spin limit (its two workgroups must be resident together); DRIL_NO_PERSISTENT_UPDATE=1 selects the per-step kernels"); }
    if (nan) return fail(h, DRIL_ERR_NAN_IN_GRADS, "gradient contains nan or is not finite (ppo.jl:213-214)");
    return DRIL_OK;
}
int ppo_update_once(dril_handle* h, dril_ppo_stats* out) {
    if (h->cfg.world_size > 1 && !comm_ready(h)) return fail(h, DRIL_ERR_NOT_INITIALISED, "world_size > 1 but dril_comm_init was not called");
    const UpdatePlan plan = update_plan(h);
    const int world = plan.world;
    const int64_t N = plan.N, B = plan.B, nb = plan.nb, total_steps = plan.total_steps;
    { int rcb = update_begin(h, plan); if (rcb) return rcb; }
    const int bits = plan.bits;
    int64_t step = 0;
    const bool persistent = small_persistent_applies(h, plan);
    if (persistent) {
        std::vector<uint64_t> keys((size_t)h->cfg.epochs);
        SmallUpdateArgs u{};
        { int rca = small_update_args(h, plan, keys.data(), u); if (rca) return rca; }
        HIPCHK(h, hipStreamSynchronize(h->stream));                                    // (keys is a stack-lifetime host buffer)
        if (!h->small_xchg) HIPCHK(h, h->small_xchg.alloc((size_t)kSmallXchgWords));
        u.xchg = h->small_xchg; u.debug_solo = std::getenv("DRIL_SMALL_DEBUG_SOLO") != nullptr;
        for (int64_t s0 = 0; s0 < total_steps; s0 += h->small_chunk) {
            small_update_chunk(plan, h->small_chunk, s0, u);
            prof_begin(h, DRIL_K_PPO_GRAD);
            HIPCHK(h, launch_ppo_update_small(h->cfg.env_kind, u, h->stream));
            prof_end(h);
        }
        small_update_done(h, plan);
#ifdef DRIL_STAMPS
        {   // per-phase s_memtime ticks of the last launch, per wave
            hipStreamSynchronize(h->stream);
            std::vector<unsigned long long> d(8 * 16);
            hipMemcpy(d.data(), h->dbg, d.size() * 8, hipMemcpyDeviceToHost);
            const char* nm[16] = {"top: moments + barrier", "L1 + tanh + h1 pieces", "wait B1", "L2 + tanh + out partial", "wait B2", "head + dW3 + dz2 + pieces", "wait B3", "dh1 + dW1 + dW2", "wait B4",
                                  "dW2 overlay", "wait B5", "g + norm", "stats + Adam + images", "-", "-", "-"};
            for (int wv = 0; wv < 8; wv += 4) {
                double tot = 0; for (int k = 0; k < 15; ++k) tot += (double)d[wv * 16 + k];
                fprintf(stderr, "[small stamps] wave %d: %.0f ticks per step (100 MHz: %.2f us)\n", wv, tot / (double)total_steps, tot / (double)total_steps / 100.0);
                for (int k = 0; k < 15; ++k) fprintf(stderr, "   %-28s %8.0f ticks/step  %5.1f %%\n", nm[k], (double)d[wv * 16 + k] / (double)total_steps, 100.0 * (double)d[wv * 16 + k] / tot);
            }
        }
#endif
        step = total_steps;
    }
    for (int ep = 0; ep < h->cfg.epochs && !persistent; ++ep) {
        const uint64_t key = perm_key(h->cfg.seed + (uint64_t)h->cfg.rank, h->update_counter, ep);
        const int64_t* perm = h->perm_count ? h->perm_dev + (size_t)ep * N : nullptr;
        const bool epoch_moments = h->cfg.normalize_advantage && !perm && nb >= 2 && nb <= 2048;
        // chip-filling minibatches of the fused kernels: the epoch's order as an index array (the update kernels then read 8 bytes per sample instead of evaluating the
        // keyed bijection per lane, wave, net and tile)
        const bool index_array = !perm && !h->generic && !h->no_epoch_index && N < (1ll << 31) && (B + kTile - 1) / kTile >= kPairTilesPerCu * (int64_t)h->num_cus;
        if (index_array) {
            if (!h->epoch_index) HIPCHK(h, h->epoch_index.alloc((size_t)N));
            prof_begin(h, DRIL_K_ADV_MOMENTS);
            HIPCHK(h, launch_epoch_index(N, key, bits, h->epoch_index, h->stream));
            prof_end(h);
        }
        if (epoch_moments) {
            if (nb > 0) { HIPCHK(h, h->epoch_tables.grow((size_t)h->epoch_blocks * 2 * nb)); HIPCHK(h, h->epoch_stats.grow((size_t)3 * nb)); }
            prof_begin(h, DRIL_K_ADV_MOMENTS);
            const int eb = (int)std::min<int64_t>(h->epoch_blocks, std::max<int64_t>(64, N / 8192));       // eight waves per SIMD at chip-filling sizes: the pass is one dependent chain per sample
            HIPCHK(h, launch_epoch_moments(h->adv, N, B, (int)nb, key, bits, h->epoch_tables, eb, h->epoch_stats, h->stop_flag, h->stream));
            prof_end(h);
            if (world > 1 || (comm_ready(h) && h->force_allreduce)) {     // ONE all-reduce per epoch for the advantage moments of all its minibatches
                int rca = rccl_allreduce(h, h->epoch_stats, (size_t)3 * nb, kNcclFloat64); if (rca) return rca;
            }
        }
        for (int64_t k = 0; k < nb; ++k, ++step) {
            const int64_t pos0 = k * B, count = (pos0 + B <= N) ? B : N - pos0;
            int rc = ppo_step(h, h->obs, h->act, h->adv, h->ret, h->logp, h->val, perm, pos0, count, N, key, bits, h->step_stats + step * 16, true, h->rec,
                              epoch_moments ? h->epoch_stats + 3 * k : nullptr, index_array ? h->epoch_index : nullptr);
            if (rc) return rc;
        }
    }
    std::vector<float> st((size_t)total_steps * 16); std::vector<double> ev(4 * (size_t)h->ev_blocks); int scal[3] = {0, 0, 0};
    const UpdateHome home{st.data(), ev.data(), scal, nullptr};
    { int rce = update_enqueue_home(h, plan, home); if (rce) return rce; }
    int rc = sync(h); if (rc) return rc;
    return update_finish(h, plan, home, out);
}
// The f16-piece kernels (the default of the fused path) compute fp32-equivalent products inside f16's RANGE: a staged weight beyond ~ 350 or a gradient tile beyond
// 65 504 / SG overflows a hi piece, and the step that meets it reports a non-finite gradient without touching the parameters.  Range is not something the reference
// asks of its user, so such an update is taken back (parameters, Adam moments, beta powers and the counters as they were before it) and redone on the exact-f32
// kernels; only a gradient that is non-finite there as well is an error (ppo.jl:213-214).  Costs three small device copies per update.
// ppo_update in the pieces a population shares with it: the decision (a), the snapshot, and what follows the first pass (b), (c)
struct UpdateTry { bool may_retry = false; uint64_t adam_steps0 = 0, counter0 = 0; };
bool update_may_retry(const dril_handle* h) { return !h->generic && h->grad_variant < 0 && !h->no_f32_retry; }
// (a) known in advance that f16 cannot hold this update: a W2 entry out of range, or the latch (kRetryLatchAfter consecutive redone updates: the workload lives outside
//     f16's range, so the next kRetryLatchUpdates run the exact-f32 kernels at once instead of paying an f16 pass + snapshot + redo each) — no wasted pass, no snapshot
bool update_direct_f32(const dril_handle* h) { return update_may_retry(h) && (h->f32_latch_left > 0 || !(h->w2max < kFwdSplitMaxW)); }
int update_run_direct_f32(dril_handle* h, dril_ppo_stats* out) {
    if (h->f32_latch_left > 0) h->f32_latch_left -= 1;
    const int gv = h->grad_variant; h->grad_variant = 0;
    const int rc = ppo_update_once(h, out);
    h->grad_variant = gv; h->f32_direct_updates += 1;
    if (out) out->f32_path = 2;
    return rc;
}
int update_snapshot(dril_handle* h, UpdateTry& t) {
    t.may_retry = update_may_retry(h); t.adam_steps0 = h->adam_steps; t.counter0 = h->update_counter;
    const size_t P = (size_t)h->P;
    if (t.may_retry) {
        if (!h->retry_snap) HIPCHK(h, h->retry_snap.alloc(3 * P + 4));
        HIPCHK(h, hipMemcpyAsync(h->retry_snap, h->params, P * 4, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->retry_snap + P, h->adam_m, P * 4, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->retry_snap + 2 * P, h->adam_v, P * 4, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->retry_snap + 3 * P, h->bt, 4 * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    return DRIL_OK;
}
int update_restore(dril_handle* h, const UpdateTry& t) {
    const size_t P = (size_t)h->P;
    HIPCHK(h, hipMemcpyAsync(h->params, h->retry_snap, P * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->adam_m, h->retry_snap + P, P * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->adam_v, h->retry_snap + 2 * P, P * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->bt, h->retry_snap + 3 * P, 4 * 4, hipMemcpyDeviceToDevice, h->stream));
    h->adam_steps = t.adam_steps0; h->update_counter = t.counter0; h->wimg_dirty = true;
    return DRIL_OK;
}
// rc: what the first pass over the default kernels returned (ppo_update_once, or a population's batched launch followed by update_finish)
int update_resolve(dril_handle* h, const UpdateTry& t, int rc, dril_ppo_stats* out) {
    const bool may_retry = t.may_retry;
    // (b) the persistent two-workgroup kernel gave up waiting for its partner (the GPU is shared with another stream / process and the two workgroups were not resident
    //     together): nothing is lost — the state of before the update is in the snapshot and the per-step kernels need no co-residency.  Redone once; the handle stays on them.
    if (rc == DRIL_ERR_HIP && h->spin_timeout && may_retry) {
        { const int rr = update_restore(h, t); if (rr) return rr; }
        h->no_persistent = true; h->persistent_fallbacks += 1;
        rc = ppo_update_once(h, out);
        if (rc == DRIL_OK) h->err.clear();
    }
    // (c) an f16-piece kernel ran somewhere in this update (sticky flag, not the last step's kernel) and a step met a non-finite gradient: redo on the exact-f32 kernels
    if (rc == DRIL_ERR_NAN_IN_GRADS && may_retry && h->used_f16) {
        { const int rr = update_restore(h, t); if (rr) return rr; }
        const int gv = h->grad_variant; h->grad_variant = 0;                            // the exact-f32 kernels for this update (the persistent small kernel is f16 as well: per-step path)
        rc = ppo_update_once(h, out);
        h->grad_variant = gv; h->f32_retries += 1;
        if (out) out->f32_path = 1;
        if (rc == DRIL_OK) h->err.clear();                                              // the first pass's message is not this call's outcome
        if (rc == DRIL_OK && ++h->f32_streak >= kRetryLatchAfter) h->f32_latch_left = kRetryLatchUpdates;   // (a gradient that is non-finite on exact f32 too is not a range problem: it arms nothing)
    } else if (rc == DRIL_OK && h->used_f16) h->f32_streak = 0;                         // an update inside f16's range: the streak (and with it the latch's re-arming) ends
    return rc;
}
int ppo_update(dril_handle* h, dril_ppo_stats* out) {
    if (update_direct_f32(h)) return update_run_direct_f32(h, out);
    UpdateTry t;
    { const int rs = update_snapshot(h, t); if (rs) return rs; }
    return update_resolve(h, t, ppo_update_once(h, out), out);
}
}  // namespace
DRIL_EXPORT int32_t dril_ppo_update(dril_handle* h, dril_ppo_stats* out) { NEED(h); return ppo_update(h, out); }
// how often the f16-piece arithmetic had to be left (include/dril_hip.h): nothing here is an error — every number delivered came from kernels that could hold it
DRIL_EXPORT int64_t dril_f32_retries(const dril_handle* h) { return h ? h->f32_retries : -1; }
DRIL_EXPORT int32_t dril_f32_fallback_info(const dril_handle* h, dril_f32_fallback* out) {
    if (!h || !out) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_f32_fallback_info: null argument");
    out->retries = h->f32_retries; out->direct_updates = h->f32_direct_updates; out->persistent_fallbacks = h->persistent_fallbacks;
    out->latch_updates_left = h->f32_latch_left; out->forward_exact_f32 = (!h->generic && fwd_exact(h)) ? 1 : 0; out->max_abs_w2 = h->w2max;
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_ppo_loss_grad(dril_handle* h, const float* obs, const void* actions, const float* advantages, const float* returns,
                                       const float* old_logprobs, const float* old_values, int64_t batch, float* loss, float* stats7, float* grads) {
    NEED(h);
    if (!obs || !actions || !advantages || !returns || !old_logprobs || !old_values || batch < 1) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ppo_loss_grad: bad argument");
    if (h->cfg.world_size > 1) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ppo_loss_grad is a single-rank parity entry point");
    const size_t B = (size_t)batch;
    DevBuf<float> d_obs, d_adv, d_ret, d_lp, d_val; DevBuf<char> d_act; DevBuf<float4> d_rec;     // freed on every return
    HIPCHK(h, d_obs.alloc(B * h->D)); HIPCHK(h, d_adv.alloc(B)); HIPCHK(h, d_ret.alloc(B)); HIPCHK(h, d_lp.alloc(B)); HIPCHK(h, d_val.alloc(B)); HIPCHK(h, d_act.alloc(B * act_bytes_per(h)));
    HIPCHK(h, hipMemcpyAsync(d_obs, obs, B * h->D * 4, hipMemcpyHostToDevice, h->stream)); HIPCHK(h, hipMemcpyAsync(d_adv, advantages, B * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_ret, returns, B * 4, hipMemcpyHostToDevice, h->stream)); HIPCHK(h, hipMemcpyAsync(d_lp, old_logprobs, B * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_val, old_values, B * 4, hipMemcpyHostToDevice, h->stream)); HIPCHK(h, hipMemcpyAsync(d_act, actions, B * act_bytes_per(h), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->stop_flag, 0, 4, h->stream));
    // the same packed records dril_ppo_update builds, so that this parity entry point runs the kernel the size rule picks for `batch` in production
    // (the pair / wide split kernels read records only)
    if (h->rec) { HIPCHK(h, d_rec.alloc((size_t)(h->D <= 4 ? 2 : 3) * B)); HIPCHK(h, launch_pack_records(h->cfg.env_kind, batch, d_obs, d_act, d_adv, d_lp, d_ret, d_rec, h->stream)); }
    int rc = ppo_step(h, d_obs, d_act, d_adv, d_ret, d_lp, d_val, nullptr, 0, batch, batch, 0, /*bits=0: identity order*/ 0, nullptr, false, d_rec);
    std::vector<float> flat((size_t)h->P + 8);
    if (!rc) { hipError_t e = hipMemcpyAsync(flat.data(), h->flat, flat.size() * 4, hipMemcpyDeviceToHost, h->stream); if (e != hipSuccess) rc = fail(h, DRIL_ERR_HIP, hipGetErrorString(e)); }
    if (!rc) rc = sync(h);
    if (rc) return rc;
    const float* s = flat.data() + h->P; const float n = s[6];
    const float pl = s[0] / n, ent = s[1] / n, vl = s[5] / n;
    if (grads) std::memcpy(grads, flat.data(), (size_t)h->P * 4);
    if (loss) *loss = pl + h->cfg.ent_coef * (-ent) + h->cfg.vf_coef * vl;
    if (stats7) { stats7[0] = pl; stats7[1] = vl; stats7[2] = -ent; stats7[3] = s[2] / n; stats7[4] = s[3] / n; stats7[5] = ent; stats7[6] = s[4] / n; }
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_apply_gradients(dril_handle* h, const float* grads, size_t n, float* grad_norm) {
    NEED(h);
    if (!grads || n != (size_t)h->P) return fail(h, DRIL_ERR_INVALID_ARG, "dril_apply_gradients: n != dril_param_count");
    HIPCHK(h, hipMemcpyAsync(h->flat, grads, n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->stop_flag, 0, 4, h->stream)); HIPCHK(h, hipMemsetAsync(h->nan_flag, 0, 4, h->stream));
    HIPCHK(h, launch_grad_norm(h->flat, h->P, h->norm_partials, h->stop_flag, h->stream));
    AdamArgs ad{};
    ad.params = h->params; ad.m = h->adam_m; ad.v = h->adam_v; ad.flat = h->flat; ad.P = h->P; ad.norm_partials = h->norm_partials;
    ad.n_partials = h->n_norm_partials; ad.bt = h->bt; ad.step_parity = (int)(h->adam_steps & 1);
    ad.beta1 = h->cfg.adam_beta1; ad.beta2 = h->cfg.adam_beta2; ad.eps = h->cfg.adam_eps; ad.lr = h->lr; ad.max_grad_norm = h->cfg.max_grad_norm;
    ad.has_max_grad_norm = h->cfg.has_max_grad_norm; ad.has_target_kl = 0; ad.use_stats = 0; ad.step_stats = nullptr; ad.norm_out = h->norm_out;
    ad.nan_flag = h->nan_flag; ad.stop_flag = h->stop_flag; ad.stop_flag_w = h->stop_flag;
    HIPCHK(h, launch_adam(ad, h->stream));
    h->adam_steps += 1; h->wimg_dirty = true;
    float norm = 0; int nan = 0; unsigned w2bits = 0;
    if (!h->generic) { HIPCHK(h, launch_w2_absmax(h->params, h->actor, h->critic, h->cfg.hidden1, h->w2max_dev, h->stream)); HIPCHK(h, hipMemcpyAsync(&w2bits, h->w2max_dev, 4, hipMemcpyDeviceToHost, h->stream)); }
    HIPCHK(h, hipMemcpyAsync(&norm, h->norm_out, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&nan, h->nan_flag, 4, hipMemcpyDeviceToHost, h->stream));
    int rc = sync(h); if (rc) return rc;
    if (!h->generic) { float m; std::memcpy(&m, &w2bits, 4); h->w2max = (m == m) ? m : INFINITY; }
    if (grad_norm) *grad_norm = norm;
    if (nan == 2) return fail(h, DRIL_ERR_HIP, "ppo_update_small_kernel: the partner workgroup did not answer within the spin limit (its two workgroups must be resident together); DRIL_NO_PERSISTENT_UPDATE=1 selects the per-step kernels");
    if (nan) return fail(h, DRIL_ERR_NAN_IN_GRADS, "gradient contains nan or is not finite (ppo.jl:213-214)");
    return DRIL_OK;
}

// ---- evaluate_agent (src/evaluation.jl:54-143) ------------------------------------------------------------
namespace {
int evaluate_agent_loop(dril_handle* h, int32_t n_eval, int32_t deterministic, dril_eval_stats* out, float* ep_rewards, int32_t* ep_lengths, bool raw) {
    const int E = h->cfg.n_envs;
    int rc = DRIL_OK;
    HIPCHK(h, h->env.reset(h->stream));   // reset!(env), :87
    if (h->mon_cur_ret) { HIPCHK(h, hipMemsetAsync(h->mon_cur_ret, 0, (size_t)E * 4, h->stream)); HIPCHK(h, hipMemsetAsync(h->mon_cur_len, 0, (size_t)E * 4, h->stream)); }
    h->env.ready = true;
    std::vector<float> rew(E), cur_r(E, 0.f), er; std::vector<uint8_t> term(E), trunc(E); std::vector<int32_t> cur_l(E, 0), el;
    float* rew_n = h->e_rew_n;                                                   // wrapper-delivered rewards (see dril_env_step)
    rc = observe_dev(h, true); if (rc) return rc;                                // observations = observe(env), :88
    int steps = 0;
    while ((int)er.size() < n_eval) {
        PolicyArgs p = policy_args(h, h->e_obs, E, nullptr, h->e_act, nullptr, h->logp /*scratch*/, nullptr, 0);
        p.gstep = h->env.gstep; p.env_seed0 = h->env.seed0; p.deterministic = deterministic ? 1 : 0;
        p.logp = h->e_rew;                                                       // logprobs are not needed: park them in a scratch array
        HIPCHK(h, run_policy(h, p));   // predict_actions(agent, observations; deterministic), :92
        rc = step_dev(h, h->e_act, rew_n, nullptr); if (rc) return rc;           // act!(env, actions), :94
        HIPCHK(h, hipMemcpyAsync(rew.data(), raw ? h->e_rew : rew_n, (size_t)E * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(term.data(), h->e_term, E, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(trunc.data(), h->e_trunc, E, hipMemcpyDeviceToHost, h->stream));
        rc = observe_dev(h, true); if (rc) return rc;                            // observations = observe(env), :97
        rc = sync(h); if (rc) return rc;
        ++steps;
        for (int i = 0; i < E; ++i) {
            cur_r[i] += rew[i]; cur_l[i] += 1;                                   // :95-96
            if ((term[i] || trunc[i]) && (int)er.size() < n_eval) { er.push_back(cur_r[i]); el.push_back(cur_l[i]); cur_r[i] = 0.f; cur_l[i] = 0; }   // :100-121
        }
        if (steps > 100000000 / (E > 0 ? E : 1) + 100000) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_evaluate_agent: no episode finishes");
    }
    double mr = 0, ml = 0; for (int i = 0; i < n_eval; ++i) { mr += er[i]; ml += el[i]; }
    mr /= n_eval; ml /= n_eval;
    double vr = 0, vl = 0; for (int i = 0; i < n_eval; ++i) { vr += (er[i] - mr) * (er[i] - mr); vl += (el[i] - ml) * (el[i] - ml); }
    out->mean_reward = mr; out->mean_length = ml;
    out->std_reward = std::sqrt(vr / (n_eval - 1)); out->std_length = std::sqrt(vl / (n_eval - 1));     // Julia std: corrected; NaN for one episode
    out->n_episodes = n_eval; out->n_steps = steps;
    if (ep_rewards) std::memcpy(ep_rewards, er.data(), (size_t)n_eval * 4);
    if (ep_lengths) std::memcpy(ep_lengths, el.data(), (size_t)n_eval * 4);
    return DRIL_OK;
}
}  // namespace
DRIL_EXPORT int32_t dril_evaluate_agent(dril_handle* h, int32_t n_eval, int32_t deterministic, dril_eval_stats* out, float* ep_rewards, int32_t* ep_lengths) {
    NEED(h); NOT_EXTERNAL(h, "dril_evaluate_agent");
    if (n_eval < 1 || !out) return fail(h, DRIL_ERR_INVALID_ARG, "dril_evaluate_agent: n_eval_episodes >= 1 and out != NULL");
    const int E = h->cfg.n_envs;
    int rc = ensure_wimg(h); if (rc) return rc;
    if (h->env.module && h->pn.on) {                                                 // a plug-in env under dril_normalize_enable: the statistics in force, frozen; nothing of the wrapper moves
        const size_t ED = (size_t)E * h->D;
        DevBuf<float> keep; HIPCHK(h, keep.alloc(ED + 2 * (size_t)E));    // returns | old_rewards | old_obs
        const int training = h->pn.cfg.training;
        hipError_t e = hipMemcpyAsync(keep, h->env.disc_returns, (size_t)E * 4, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(keep + E, h->e_rew, (size_t)E * 4, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(keep + 2 * (size_t)E, h->e_obs_raw, ED * 4, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) {
            h->pn.cfg.training = 0;                                              // set_training(eval_env, false): neither statistics nor `returns` are updated
            rc = evaluate_agent_loop(h, n_eval, deterministic, out, ep_rewards, ep_lengths, /*raw_rewards=*/true);
            h->pn.cfg.training = training;
            e = hipMemcpyAsync(h->env.disc_returns, keep, (size_t)E * 4, hipMemcpyDeviceToDevice, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(h->e_rew, keep + E, (size_t)E * 4, hipMemcpyDeviceToDevice, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(h->e_obs_raw, keep + 2 * (size_t)E, ED * 4, hipMemcpyDeviceToDevice, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        }
        keep.release();
        if (rc) return rc;
        HIPCHK(h, e);
        return DRIL_OK;
    }
    return evaluate_agent_loop(h, n_eval, deterministic, out, ep_rewards, ep_lengths, h->mon_cur_ret != nullptr);   // monitored: infos[i]["episode"]["r"] is the raw return
}

// ---- evaluate_agent on the device, training state left untouched (docs/evaluation.md) --------------------------------------------------------
// The loop of evaluate_agent_loop above with the host taken out of it: the episode accounting of dril_eval_account.h runs on the device, the host looks at ONE 4-byte
// counter every K env steps, and what the loop writes of the env side is set aside before and put back after.  Two forms of the K steps between two looks:
//   path 1  ONE launch of evaluate_kernel (dril_kernels.hip): built-in kinds on the fused shapes of width 64 / 128 / 256 with no normaliser — and, where the
//           options ask for it (DRIL_EVAL_OPT_PERSISTENT), under cfg.norm_* too: evaluate_modes_kernel reads the frozen statistics as an argument
//   path 0  per env step the launches run_policy / step_dev / observe_dev make, and eval_account_kernel over the step's reward and done arrays: everything else
//   path 2  on request, a plug-in handle whose code object carries a usable evaluation kernel (include/device/dril_env_evaluate.h): ONE launch of that kernel leaves the K
//           rows of raw rewards and flag bytes, ONE launch of eval_account_rows_kernel walks them: 2 launches per K env steps
namespace dril {   // (a named namespace: tools/kernel_resources.py lists the kernels by their names)
// path 2: a thread per env walks its K rows in step order.  Inside the launch events are unordered, as on path 1: the list has eval_event_capacity(n, E, K) slots
__global__ __launch_bounds__(256) void eval_account_rows_kernel(EvalAcct a, int32_t step0, int32_t K, const float* __restrict__ rew, const uint8_t* __restrict__ flags) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    float ret = a.cur_ret[e]; int32_t len = a.cur_len[e];
    for (int32_t k = 0; k < K; ++k) { const size_t i = (size_t)k * a.E + e; eval_account(a, step0 + k + 1, e, rew[i], flags[i] != 0, ret, len); }
    a.cur_ret[e] = ret; a.cur_len[e] = len;
}
// path 2, recording: the per-trajectory rule over the K rows, a thread per (env, word) as traj_record_kernel
__global__ __launch_bounds__(256) void traj_record_rows_kernel(TrajRec r, TrajMaps x, TrajRows s, int32_t t0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t lanes = r.D > r.W ? r.D : r.W;
    if (i >= (int64_t)r.M * lanes) return;
    traj_record_lane_rows(r, x, s, t0, (int32_t)(i / lanes), (int32_t)(i % lanes));
}
}  // namespace dril
namespace {
__global__ __launch_bounds__(256) void eval_account_kernel(EvalAcct a, int32_t step, const float* __restrict__ rew, const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    eval_account_env(a, step, e, rew[e], (term[e] | trunc[e]) != 0);
}
// the default K of each path: UNMEASURED starting points (docs/evaluation.md, "Measured") — the SAC verb's min(time limit, 32) for the step-granular path, a guess for the
// persistent one.  No more than the time limit, after which every env has finished an episode
constexpr int kEvalPollStepwise = 32, kEvalPollPersistent = 64;
constexpr long long kEvalMaxLaunchEvents = 1ll << 22;   // E K of one evaluate_kernel launch: 64 MB of event slots at the most
// requested: the caller's opt-in (DRIL_EVAL_OPT_PERSISTENT / DRIL_TRAJ_OPT_PERSISTENT), which admits a normalised handle; without it, the rule every caller has had
bool eval_persistent_applies(const dril_handle* h, bool requested = false) {
    const int hd = h->cfg.hidden1;
    return !h->generic && !h->env.module && (!normalizing(h) || requested) && !h->force_stepwise && (hd == 64 || hd == 128 || hd == 256);   // (DRIL_FORCE_STEPWISE: the step-granular launches, as for the collection)
}
// evaluate_kernel's arguments from the handle (the rollout launcher's choices: fwd_exact, action_start, fixed_length_episodes); T and step0 are set per launch
void eval_kernel_args(const dril_handle* h, EvalKernelArgs& g, int deterministic) {
    RolloutArgs& a = g.r;
    a.params = h->params; a.state = h->env.state; a.step_count = h->env.step_count; a.episode = h->env.episode; a.gstep = h->env.gstep;
    a.E = h->cfg.n_envs; a.episode_len = h->env.episode_len; a.fixed_len = h->env.fixed_len; a.action_start = h->env.action_start; a.log_std_off = h->log_std_off;
    a.env_seed0 = h->env.seed0; a.actor = h->actor; a.critic = h->critic; a.exact_f32 = fwd_exact(h) ? 1 : 0;
    a.w2a_actor = a.exact_f32 ? h->w2a_actor : (const float*)h->w2pf_actor.get(); a.w2a_critic = nullptr;
    g.deterministic = deterministic ? 1 : 0;
}
// the frozen NormalizeWrapperEnv as evaluate_modes_kernel takes it: the halves of the statistics in force, read only.  raw: the accounting counts raw rewards
void eval_mode_norm(const dril_handle* h, EvalModeArgs& x, bool raw) {
    x.obs_stats = h->obs_rms + h->obs_par; x.ret_stats = h->ret_rms + h->ret_par;
    x.norm_obs = h->cfg.norm_obs ? 1 : 0; x.norm_reward = h->cfg.norm_reward ? 1 : 0; x.count_raw = raw ? 1 : 0;
    x.clip_obs = h->cfg.clip_obs; x.clip_reward = h->cfg.clip_reward; x.eps = h->cfg.norm_epsilon;
}
// path 2 applies: the request, a plug-in handle, a usable kernel for this net; DRIL_FORCE_STEPWISE wins, as everywhere
bool eval_fused_applies(const dril_handle* h, bool requested) {
    return requested && h->env.module && !h->force_stepwise && fused_evaluate_unavailable(h).empty();
}
// the argument block of a plug-in's evaluation kernel for launches of up to K steps, M recorded envs (shadow: their never-resetting twins; null when M == 0); the
// handle's blob is grown to hold the scratch.  The frozen statistics of dril_normalize_enable travel as pointers into the half in force and are only read
int eval_fused_args(dril_handle* h, DrilEnvEvaluateArgs& g, int deterministic, int K, int M, const DeviceEnvs* shadow) {
    const size_t E = (size_t)h->cfg.n_envs, D = (size_t)h->D, W = h->discrete ? 1 : (size_t)h->A, Ks = (size_t)K, Ms = (size_t)M;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_obs = take(E * D * 4), o_act = take(E * W * 4), o_rew = take(Ks * E * 4), o_flg = take(Ks * E);
    const size_t o_obs0 = take(Ms * D * 4), o_ract = take(Ks * Ms * W * 4), o_robs = take(Ks * Ms * D * 4);
    if (off > 0) HIPCHK(h, h->evalf_blob.grow(off));
    char* b = h->evalf_blob;
    g = DrilEnvEvaluateArgs{};
    g.r.env = h->env.args(); g.r.env.obs = (float*)(b + o_obs);                       // (after the call's seed is in force: seed0 is the one the reset used)
    g.r.T = K; g.r.n_hidden = h->gd.nh; g.r.activation = h->gd.act; g.r.n_params = h->P;
    for (int l = 0; l < h->gd.nh; ++l) g.r.hidden[l] = h->gd.H[l];
    g.r.actor_off = h->actor.w1; g.r.log_std_off = h->log_std_off; g.r.params = h->params;
    g.r.act = b + o_act; g.r.rew = (float*)(b + o_rew); g.r.flags = (uint8_t*)(b + o_flg);
    g.deterministic = deterministic ? 1 : 0; g.n_record = M;
    if (h->pn.on && h->pn.cfg.norm_obs) { g.norm_mean = h->pn.half(h->pn.cur); g.norm_var = g.norm_mean + h->pn.D; g.norm_eps = h->pn.cfg.epsilon; g.norm_clip = h->pn.cfg.clip_obs; }
    if (M > 0) { g.shadow = shadow->args(); g.rec_obs0 = (float*)(b + o_obs0); g.rec_act = b + o_ract; g.rec_obs = (float*)(b + o_robs); }
    return DRIL_OK;
}
// what one evaluation sets aside: device arrays in a list (copied to / from one blob), the host-side words next to them
struct EvalKeep {
    std::vector<std::pair<void*, size_t>> arrays;
    uint64_t seed0; bool ready; int obs_par, ret_par, norm_training, pn_training; DevBuf<float> mon_cur_ret; int64_t gws_launches;
};
void eval_keep_list(dril_handle* h, bool persistent, EvalKeep& k) {
    const size_t E = (size_t)h->cfg.n_envs, ED = E * h->D * 4;
    k.arrays = {{h->env.state, E * h->S * 4}, {h->env.step_count, E * 4}, {h->env.episode, E * 4}, {h->env.gstep, E * 4}, {h->env.disc_returns, E * 4}};
    if (persistent) return;                                                        // evaluate_kernel writes the envs alone (reset! zeroes `returns`)
    const std::pair<void*, size_t> step_arrays[] = {{h->e_obs, ED}, {h->e_rew, E * 4}, {h->e_tobs, ED}, {h->e_term, E}, {h->e_trunc, E}, {h->e_act, E * act_bytes_per(h)}};
    k.arrays.insert(k.arrays.end(), std::begin(step_arrays), std::end(step_arrays));
    if (normalizing(h) || h->pn.on) { k.arrays.push_back({h->e_obs_raw, ED}); k.arrays.push_back({h->e_rew_n, E * 4}); }
    if (normalizing(h)) { k.arrays.push_back({h->obs_rms, 2 * sizeof(RmsState)}); k.arrays.push_back({h->ret_rms, 2 * sizeof(RmsState)}); }   // both halves: a frozen apply copies in -> out and flips the parity
}
int eval_keep_copy(dril_handle* h, const EvalKeep& k, bool save) {
    size_t off = 0;
    for (const auto& a : k.arrays) {
        if (save) HIPCHK(h, hipMemcpyAsync(h->eval_snap + off, a.first, a.second, hipMemcpyDeviceToDevice, h->stream));
        else HIPCHK(h, hipMemcpyAsync(a.first, h->eval_snap + off, a.second, hipMemcpyDeviceToDevice, h->stream));
        off += (a.second + 15) & ~(size_t)15;
    }
    return DRIL_OK;
}
int eval_buffers(dril_handle* h, const EvalKeep& k, long long cap) {
    const size_t E = (size_t)h->cfg.n_envs;
    size_t bytes = 0; for (const auto& a : k.arrays) bytes += (a.second + 15) & ~(size_t)15;
    if (bytes > 0) HIPCHK(h, h->eval_snap.grow(bytes));
    if (!h->eval_cur_ret) HIPCHK(h, h->eval_cur_ret.alloc(E)); if (!h->eval_cur_len) HIPCHK(h, h->eval_cur_len.alloc(E)); if (!h->eval_counter) HIPCHK(h, h->eval_counter.alloc(1));
    if (!h->eval_counter_host) HIPCHK(h, h->eval_counter_host.alloc(1));
    if (cap > 0) HIPCHK(h, h->eval_events.grow((size_t)cap));
    return DRIL_OK;
}
// The pieces of one step-granular env step that the evaluation (eval_step_granular) and the recording (traj_step) share; what differs sits between them.
// wrapped: a NormalizeWrapperEnv (cfg.norm_* or dril_normalize_enable) is around the envs, its statistics frozen for the call
bool eval_wrapped(const dril_handle* h) { return normalizing(h) || h->pn.on; }
// predict_actions(agent, observations; deterministic), evaluation.jl:92 / trajectory_utils.jl:28
int eval_step_policy(dril_handle* h, int deterministic) {
    PolicyArgs p = policy_args(h, h->e_obs, h->cfg.n_envs, nullptr, h->e_act, nullptr, h->e_rew /*log-probabilities are not needed: parked where act! writes next*/, nullptr, 0);
    p.gstep = h->env.gstep; p.env_seed0 = h->env.seed0; p.deterministic = deterministic ? 1 : 0;
    HIPCHK(h, run_policy(h, p));
    return DRIL_OK;
}
// act!(env, actions), :94 / :35.  *rew: the rewards an accounting reads — raw (dril_evaluate_agent's rule; they stay in e_rew), else what the wrapper delivers
int eval_step_env(dril_handle* h, bool raw, const float** rew) {
    float* delivered = (h->env.module && !h->pn.on) ? nullptr : h->e_rew_n;
    *rew = (eval_wrapped(h) && !raw && delivered) ? delivered : h->e_rew;
    return eval_wrapped(h) ? step_dev(h, h->e_act, delivered, nullptr) : env_step_arrays(h, h->e_act);   // no wrapper: the raw step is the whole step (as dril_env_step)
}
// observations = observe(env), :88, :97 / :17, :24-26
int eval_step_observe(dril_handle* h) { if (eval_wrapped(h)) return observe_dev(h, true); HIPCHK(h, h->env.observe(h->e_obs, h->stream)); return DRIL_OK; }
// the launches of the three above.  g0: gws.launches before the policy (a generic shape's forward is several launches)
int32_t eval_step_launches(const dril_handle* h, int64_t g0) { return (h->generic ? (int32_t)(h->gws.launches - g0) : 1) + 2 + (eval_wrapped(h) ? (h->env.module ? 2 : 3) : 0); }
// one env step of path 0, enqueued: predict_actions -> act! -> accounting -> observe.  raw: the accounting reads the raw rewards (dril_evaluate_agent's rule)
int eval_step_granular(dril_handle* h, const EvalAcct& acct, int32_t step, int deterministic, bool raw, int32_t* launches) {
    const int E = h->cfg.n_envs; const int64_t g0 = h->gws.launches; const float* rew = nullptr;
    { int rc = eval_step_policy(h, deterministic); if (rc) return rc; }
    { int rc = eval_step_env(h, raw, &rew); if (rc) return rc; }
    hipLaunchKernelGGL(eval_account_kernel, dim3((E + 255) / 256), dim3(256), 0, h->stream, acct, step, rew, h->e_term, h->e_trunc);
    HIPCHK(h, hipGetLastError());
    { int rc = eval_step_observe(h); if (rc) return rc; }
    *launches += eval_step_launches(h, g0);
    return DRIL_OK;
}
// K: env steps between two looks at the counter — the ONE rule of both verbs on every path (the table of callers: docs/evaluation.md, "K").  poll_steps > 0 replaces
// the default and takes the same caps.  persistent: one launch runs the K steps (paths 1 and 2).  cap_events: E K of a launch is bounded by kEvalMaxLaunchEvents
// (the list it may fill: eval_event_capacity, dril_eval_account.h); the recording on path 1 does not ask for it.  cap_steps: Tcap, for the recording on path 2 alone
int eval_poll_steps(const dril_handle* h, int32_t poll_steps, bool persistent, bool cap_events, int cap_steps = INT32_MAX) {
    const int K = std::min(poll_steps > 0 ? poll_steps : std::max(1, std::min(h->env.episode_len, persistent ? kEvalPollPersistent : kEvalPollStepwise)), cap_steps);
    return cap_events ? (int)std::max<long long>(1, std::min<long long>(K, kEvalMaxLaunchEvents / std::max(1, h->cfg.n_envs))) : K;
}
// ---- the pieces of dril_evaluate_agent_device, in the order it runs them: prepare, set-aside, reset, enqueue, put-back, reduce.  dril_population_evaluate_device
// calls the same pieces per member (as pop_collect / pop_update call rollout_args / update_begin), so a member's evaluation is that of its handle alone ----
struct EvalPlan { bool persistent, fused, raw; int K; long long cap; EvalKeep keep; };
// prepare: which path runs, K, the list's capacity, what the call will set aside, the buffers
int eval_prepare(dril_handle* h, const dril_eval_options* o, EvalPlan& pl) {
    { int rc = ensure_wimg(h); if (rc) return rc; }
    pl.persistent = !o->force_step_granular && eval_persistent_applies(h, o->reserved[DRIL_EVAL_OPT_PERSISTENT] != 0);
    pl.fused = !o->force_step_granular && eval_fused_applies(h, o->reserved[DRIL_EVAL_OPT_PERSISTENT] != 0);   // path 2: a plug-in's own evaluation kernel (never both)
    pl.raw = (h->env.module && h->pn.on) || h->mon_cur_ret != nullptr;                  // dril_evaluate_agent's rule: raw returns under the monitor (and under a plug-in's normaliser)
    eval_keep_list(h, pl.persistent || pl.fused, pl.keep);                             // (path 2 writes the envs and scratch of its own: the per-step arrays are not touched)
    pl.K = eval_poll_steps(h, o->poll_steps, pl.persistent || pl.fused, /*cap_events=*/pl.persistent || pl.fused);
    pl.cap = eval_event_capacity(o->n_eval_episodes, h->cfg.n_envs, (pl.persistent || pl.fused) ? pl.K : 1);   // (path 0: one launch per env step)
    return eval_buffers(h, pl.keep, pl.cap);
}
// set-aside: the evaluation runs on the handle's own envs — what training would continue from is kept here and put back by eval_put_back, on every path
int eval_set_aside(dril_handle* h, EvalKeep& keep) {
    keep.seed0 = h->env.seed0; keep.ready = h->env.ready; keep.obs_par = h->obs_par; keep.ret_par = h->ret_par; keep.norm_training = h->cfg.norm_training;
    keep.pn_training = h->pn.cfg.training; keep.gws_launches = h->gws.launches;
    { int rc = eval_keep_copy(h, keep, true); if (rc) return rc; }
    h->cfg.norm_training = 0; h->pn.cfg.training = 0;                                  // set_training(env, false): the statistics in force, frozen; `returns` stands still
    keep.mon_cur_ret = std::move(h->mon_cur_ret);                                      // evaluation episodes do not enter the training env's MonitorWrapperEnv: its launches are not made
    return DRIL_OK;
}
// open the episode, for both verbs: the call's seed (env e of rank r: seed + r E + e), reset!(env) (evaluation.jl:87 / trajectory_utils.jl:10), the counter zeroed — the
// device word the kernels count in (the handle's own, or its word of a population's array).  shadow (null: none): a recording's twins of envs 0..M-1, seeded alike
int eval_open_episode(dril_handle* h, bool has_seed, uint64_t seed, unsigned int* counter, DeviceEnvs* shadow = nullptr) {
    if (has_seed) h->env.seed0 = seed + (uint64_t)h->cfg.rank * (uint64_t)h->cfg.n_envs;
    HIPCHK(h, h->env.reset(h->stream));
    h->env.ready = true;
    if (shadow) shadow->seed0 = h->env.seed0;
    if (shadow) for (void* p : {(void*)shadow->step_count, (void*)shadow->episode, (void*)shadow->gstep}) HIPCHK(h, hipMemsetAsync(p, 0, (size_t)shadow->E * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(counter, 0, 4, h->stream));
    return DRIL_OK;
}
int eval_reset(dril_handle* h, const dril_eval_options* o, unsigned int* counter, long long cap, EvalAcct& acct) {
    const int E = h->cfg.n_envs;
    { int rc = eval_open_episode(h, o->has_seed != 0, o->seed, counter); if (rc) return rc; }
    HIPCHK(h, hipMemsetAsync(h->eval_cur_ret, 0, (size_t)E * 4, h->stream)); HIPCHK(h, hipMemsetAsync(h->eval_cur_len, 0, (size_t)E * 4, h->stream));
    acct = EvalAcct{E, h->eval_cur_ret, h->eval_cur_len, counter, h->eval_events, (unsigned int)cap};
    return DRIL_OK;
}
// every env finishes an episode within the time limit, so n of them take at most ceil(n / E) time limits; one more, and the steps enqueued past a look
long long eval_max_steps(const dril_handle* h, int n_eval, int K) {
    const int E = h->cfg.n_envs;
    return ((long long)(n_eval + E - 1) / E + 1) * (long long)h->env.episode_len + K;
}
// enqueue (path 1): the argument block of the launches of K steps; step0 is set per launch
void eval_persistent_args(const dril_handle* h, const dril_eval_options* o, int K, const EvalAcct& acct, EvalKernelArgs& g) {
    eval_kernel_args(h, g, o->deterministic); g.r.T = K; g.acct = acct;           // (after the seed of eval_reset: env_seed0 is the one the reset used)
}
// put-back: the host-side words, and the copies home enqueued (the caller drains the stream)
int eval_put_back(dril_handle* h, EvalKeep& keep) {
    h->env.seed0 = keep.seed0; h->env.ready = keep.ready; h->obs_par = keep.obs_par; h->ret_par = keep.ret_par; h->cfg.norm_training = keep.norm_training;
    h->pn.cfg.training = keep.pn_training; h->mon_cur_ret = std::move(keep.mon_cur_ret); h->gws.launches = keep.gws_launches;
    return eval_keep_copy(h, keep, false);
}
// the end of either verb, after eval_set_aside: the state is put back and the stream drained whatever the run returned (rc), and the run's error is the one reported
int eval_finish(dril_handle* h, EvalKeep& keep, const char* verb, int rc) {
    const std::string msg = h->err;
    int rr = eval_put_back(h, keep);
    if (rr == DRIL_OK) { const hipError_t e = hipStreamSynchronize(h->stream); if (e != hipSuccess) rr = fail(h, DRIL_ERR_HIP, std::string(verb) + ": " + hipGetErrorString(e)); }
    if (rc != DRIL_OK) { h->err = msg; return rc; }
    return rr;
}
// the loop of either verb on every path: until `want` episodes / trajectories are counted, enqueue a chunk of env steps, copy the 4-byte counter home, drain, read it.
// enqueue(steps, launches) -> status advances both by what it put into the stream.  A chunk that would start at or past `bound` steps fails with (code, bound_msg)
struct EvalPoll { unsigned int seen = 0; long long steps = 0; int32_t launches = 0; };
template <class Enqueue> int eval_poll_loop(dril_handle* h, int want, long long bound, int code, const char* bound_msg, EvalPoll& p, Enqueue&& enqueue) {
    p = EvalPoll{};
    while (p.seen < (unsigned int)want) {
        if (p.steps >= bound) return fail(h, code, bound_msg);
        { int rc = enqueue(p.steps, p.launches); if (rc) return rc; }
        HIPCHK(h, hipMemcpyAsync(h->eval_counter_host, h->eval_counter, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        p.seen = *h->eval_counter_host;
    }
    return DRIL_OK;
}
// reduce: the first n_eval_episodes events in (step, env) order
void eval_reduce(SacEvalEvent* events, int64_t n_events, const dril_eval_options* o, dril_eval_stats* out, float* ep_rewards, int32_t* ep_lengths) { sac_eval_stats(events, n_events, o->n_eval_episodes, out, ep_rewards, ep_lengths); }
int eval_device_run(dril_handle* h, const dril_eval_options* o, const EvalPlan& pl, std::vector<SacEvalEvent>& events, dril_eval_info* info) {
    const bool persistent = pl.persistent, fused = pl.fused, raw = pl.raw; const int K = pl.K; const long long cap = pl.cap;
    const int E = h->cfg.n_envs, n_eval = o->n_eval_episodes;
    EvalAcct acct{};
    { int rc = eval_reset(h, o, h->eval_counter, cap, acct); if (rc) return rc; }
    EvalKernelArgs g{}; EvalModeArgs x{}; DrilEnvEvaluateArgs gf{};
    const bool modes = persistent && normalizing(h);                              // a frozen normaliser: evaluate_modes_kernel; otherwise evaluate_kernel as ever
    if (fused) { int rc = eval_fused_args(h, gf, o->deterministic, K, 0, nullptr); if (rc) return rc; }   // (the kernel opens every launch with its own observe)
    else if (persistent) {
        eval_persistent_args(h, o, K, acct, g);
        if (modes) eval_mode_norm(h, x, raw);
    } else { int rc = eval_step_observe(h); if (rc) return rc; }                  // observations = observe(env), :88
    EvalPoll p;
    const int rc = eval_poll_loop(h, n_eval, eval_max_steps(h, n_eval, K), DRIL_ERR_UNSUPPORTED, "dril_evaluate_agent_device: no episode finishes", p, [&](long long& steps, int32_t& launches) -> int {
        if (fused) {
            HIPCHK(h, h->env.launch_evaluate(gf, h->stream));
            hipLaunchKernelGGL(eval_account_rows_kernel, dim3((E + 255) / 256), dim3(256), 0, h->stream, acct, (int32_t)steps, (int32_t)K, gf.r.rew, gf.r.flags);
            HIPCHK(h, hipGetLastError());
            steps += K; launches += 2;
        }
        else if (persistent) { g.step0 = (int32_t)steps; HIPCHK(h, launch_evaluate(h->env.kind, h->cfg.hidden1, g, h->stream, modes ? &x : nullptr)); steps += K; launches += 1; }
        else for (int k = 0; k < K; ++k) { int rc = eval_step_granular(h, acct, (int32_t)(++steps), (o->deterministic ? 1 : 0), raw, &launches); if (rc) return rc; }
        return DRIL_OK;
    });
    if (rc) return rc;
    events.resize((size_t)std::min<long long>(p.seen, cap));
    HIPCHK(h, hipMemcpyAsync(events.data(), h->eval_events, events.size() * sizeof(SacEvalEvent), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (info) { info->path = fused ? 2 : persistent ? 1 : 0; info->launches = p.launches; info->steps_enqueued = (int32_t)p.steps; info->events = (int32_t)p.seen; }
    return DRIL_OK;
}
const char* const kEvalArgMsg = "dril_evaluate_agent_device: options and out != NULL, n_eval_episodes >= 1, poll_steps >= 0";
}  // namespace
DRIL_EXPORT int32_t dril_eval_options_default(dril_eval_options* o) {
    if (!o) return DRIL_ERR_INVALID_ARG;
    std::memset(o, 0, sizeof(*o));
    o->n_eval_episodes = 10; o->deterministic = 1;                                     // evaluation.jl:57-58
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_evaluate_agent_device(dril_handle* h, const dril_eval_options* o, dril_eval_stats* out, float* ep_rewards, int32_t* ep_lengths, dril_eval_info* info) {
    NEED(h); NOT_EXTERNAL(h, "dril_evaluate_agent");
    if (!o || !out || o->n_eval_episodes < 1 || o->poll_steps < 0) return fail(h, DRIL_ERR_INVALID_ARG, kEvalArgMsg);
    if (info) std::memset(info, 0, sizeof(*info));
    EvalPlan pl;
    { int rc = eval_prepare(h, o, pl); if (rc) return rc; }
    { int rc = eval_set_aside(h, pl.keep); if (rc) return rc; }
    std::vector<SacEvalEvent> events;
    { int rc = eval_finish(h, pl.keep, "dril_evaluate_agent_device", eval_device_run(h, o, pl, events, info)); if (rc) return rc; }
    eval_reduce(events.data(), (int64_t)events.size(), o, out, ep_rewards, ep_lengths);
    return DRIL_OK;
}

// ---- collect_trajectory on the device, training state left untouched (trajectory_utils.jl:3-49; docs/evaluation.md, "Trajectories") ------------------------------
// The step-granular launches of the evaluation above, with the episode accounting replaced by a recording of envs 0..M-1.  What no existing kernel produces is the
// observation after the last step of a TERMINATED episode (the step kernels write terminal_obs where truncated, then auto-reset), so M SHADOW envs take every step
// a second time: a DeviceEnvs view of the same kind / plug-in with its own arrays, fixed_len = 1 (masks the terminated flag, nothing else) and an unreachable time
// limit, so it never resets.  Per env step it is given the live envs' pre-step state, takes the step with the same actions, and its observe is the post-step,
// pre-reset observation of every recorded env — the very float operations the live step ran before its auto-reset.  No kernel, argument block or code object changes.
namespace dril {   // (a named namespace: tools/kernel_resources.py lists the kernel by its name)
__global__ __launch_bounds__(256) void traj_record_kernel(TrajRec r, TrajMaps x, TrajStep s, int32_t t) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t lanes = r.D > r.W ? r.D : r.W;                                   // a thread per (env, word): one step's rows are contiguous in the step-major recording
    if (i >= (int64_t)r.M * lanes) return;
    traj_record_lane(r, x, s, t, (int32_t)(i / lanes), (int32_t)(i % lanes));
}
}  // namespace dril
namespace {
// the setup shared with the SAC handle (dril_traj_run.h) with what this handle alone knows: `discrete`, and ClampAdapter on the agent-facing Box (Box(-1, 1) under ScalingWrapperEnv)
int traj_prepare(dril_handle* h, const dril_traj_options* o, int32_t Tcap, TrajRun& r) {
    const size_t W = h->discrete ? 1 : (size_t)h->A;
    std::vector<float> clamp_low(W, 0.f), clamp_high(W, 0.f);
    TrajBoxes boxes = traj_env_boxes(h->env); boxes.discrete = h->discrete; boxes.clamp_low = clamp_low.data(); boxes.clamp_high = clamp_high.data();
    const EnvKindInfo* ki = env_kind_info(h->env.kind);
    if (!h->env.module && !ki) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_collect_trajectory_device: no device env on this handle");
    if (h->env.module) { if (!h->discrete) h->env.agent_action_space(clamp_low.data(), clamp_high.data()); }
    else if (ki->box) { clamp_low[0] = ki->act_lo; clamp_high[0] = ki->act_hi; }
    const TrajLayout L = traj_layout((size_t)o->n_trajectories, (size_t)h->D, W, (size_t)h->S, (size_t)Tcap);
    HIPCHK(h, traj_setup(h->env, h->stream, h->traj_blob, h->eval_counter, L, boxes, o->final_original != 0, /*drain_before_free=*/false, r));
    return DRIL_OK;
}
// one env step, enqueued: the launches of eval_step_granular, and over the M recorded envs only a state copy, the shadow step, the shadow observe and the recording
int traj_step(dril_handle* h, const TrajRun& r, int32_t t, int deterministic, int32_t* launches) {
    const int64_t g0 = h->gws.launches; const float* raw_rew = nullptr;
    HIPCHK(h, hipMemcpyAsync(r.shadow.state, h->env.state, (size_t)r.rec.M * h->S * 4, hipMemcpyDeviceToDevice, h->stream));   // the pre-step state of envs 0..M-1 (env-major prefix)
    { int rc = eval_step_policy(h, deterministic); if (rc) return rc; }
    HIPCHK(h, r.shadow.step(h->e_act, EnvStepOut{r.sh_rew, r.sh_term, r.sh_trunc, r.sh_tobs, nullptr}, MonitorArgs{}, h->stream));   // the same step, with no reset after it
    HIPCHK(h, r.shadow.observe(r.sh_obs, h->stream));                              // observe(env) of the env that did not auto-reset
    { int rc = eval_step_env(h, /*raw=*/true, &raw_rew); if (rc) return rc; }      // (the wrapper's statistics frozen; the recording takes the raw rewards)
    HIPCHK(h, traj_record_launch(traj_record_kernel, h->stream, r, TrajStep{h->e_act, raw_rew, h->e_term, h->e_trunc, r.sh_obs}, t));
    { int rc = eval_step_observe(h); if (rc) return rc; }                          // the next obs_to_agent (normalize_obs!, :24-26)
    *launches += eval_step_launches(h, g0) + 4 + (h->env.module ? 0 : 1);          // (a built-in shadow step + observe: env_step_kernel, env_observe_kernel)
    return DRIL_OK;
}
const char* const kTrajStillOpenMsg = "dril_collect_trajectory_device: a trajectory is still open after its capacity (internal)";   // (step Tcap finalises every open one)
// the persistent form: evaluate_modes_kernel in its recording mode, K env steps per launch.  No shadow envs, no state copies, none of the per-step arrays: the lane
// that holds env m < M records it from its registers.  The last launch is shortened so that no step past Tcap is ever enqueued
int traj_persistent_run(dril_handle* h, const dril_traj_options* o, const TrajRun& r, EvalPoll& p) {
    { int rc = eval_open_episode(h, o->has_seed != 0, o->seed, h->eval_counter); if (rc) return rc; }
    EvalKernelArgs g{}; EvalModeArgs x{};
    eval_kernel_args(h, g, o->deterministic);                                      // (after the call's seed is in force)
    if (normalizing(h)) eval_mode_norm(h, x, true);                                // (no accounting while recording: the reward row is the raw reward)
    x.record = 1; x.rec = r.rec; x.maps = r.maps;
    const int K = eval_poll_steps(h, o->poll_steps, /*persistent=*/true, /*cap_events=*/false);
    return eval_poll_loop(h, r.rec.M, r.rec.Tcap, DRIL_ERR_HIP, kTrajStillOpenMsg, p, [&](long long& steps, int32_t& launches) -> int {
        g.step0 = (int32_t)steps; g.r.T = std::min(K, r.rec.Tcap - (int)steps);
        HIPCHK(h, launch_evaluate(h->env.kind, h->cfg.hidden1, g, h->stream, &x)); steps += g.r.T; launches += 1;
        return DRIL_OK;
    });
}
// path 2: a plug-in's evaluation kernel in its recording mode, K env steps per launch, and ONE launch of the per-trajectory rule over the rows it leaves.  The shadow
// envs are those of the step-granular form, stepped inside the kernel by the recorded env's own lane.  The last launch is shortened: no step past Tcap is ever enqueued
int traj_fused_run(dril_handle* h, const dril_traj_options* o, TrajRun& r, EvalPoll& p) {
    const int E = h->cfg.n_envs, M = r.rec.M, Tcap = r.rec.Tcap;
    { int rc = eval_open_episode(h, o->has_seed != 0, o->seed, h->eval_counter, &r.shadow); if (rc) return rc; }
    const int K = eval_poll_steps(h, o->poll_steps, /*persistent=*/true, /*cap_events=*/true, /*cap_steps=*/Tcap);
    DrilEnvEvaluateArgs g{};
    { int rc = eval_fused_args(h, g, o->deterministic, K, M, &r.shadow); if (rc) return rc; }
    const int64_t n = (int64_t)M * std::max(r.rec.D, r.rec.W);
    return eval_poll_loop(h, M, Tcap, DRIL_ERR_HIP, kTrajStillOpenMsg, p, [&](long long& steps, int32_t& launches) -> int {
        g.r.T = std::min(K, Tcap - (int)steps);
        HIPCHK(h, h->env.launch_evaluate(g, h->stream));
        const TrajRows rows{g.r.T, E, g.r.rew, g.r.flags, g.rec_obs0, (const uint32_t*)g.rec_act, g.rec_obs};
        hipLaunchKernelGGL(traj_record_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, r.rec, r.maps, rows, (int32_t)steps);
        HIPCHK(h, hipGetLastError());
        steps += g.r.T; launches += 2;
        return DRIL_OK;
    });
}
// the step-granular form: traj_step per env step, a look at the finished-counter every K steps
int traj_stepwise_run(dril_handle* h, const dril_traj_options* o, TrajRun& r, EvalPoll& p) {
    { int rc = eval_open_episode(h, o->has_seed != 0, o->seed, h->eval_counter, &r.shadow); if (rc) return rc; }
    { int rc = eval_step_observe(h); if (rc) return rc; }                          // observation = observe(env), :17
    HIPCHK(h, traj_record_launch(traj_record_kernel, h->stream, r, TrajStep{nullptr, nullptr, nullptr, nullptr, eval_wrapped(h) ? h->e_obs_raw : h->e_obs}, 0));   // row 0: the original observation
    const int K = eval_poll_steps(h, o->poll_steps, /*persistent=*/false, /*cap_events=*/false);
    return eval_poll_loop(h, r.rec.M, r.rec.Tcap, DRIL_ERR_HIP, kTrajStillOpenMsg, p, [&](long long& steps, int32_t& launches) -> int {
        for (int k = 0; k < K && steps < r.rec.Tcap; ++k) { int rc = traj_step(h, r, (int32_t)(++steps), (o->deterministic ? 1 : 0), &launches); if (rc) return rc; }
        return DRIL_OK;
    });
}
int traj_device_run(dril_handle* h, const dril_traj_options* o, TrajRun& r, int path, float* observations, void* actions, float* rewards, int32_t* lengths, uint8_t* end_flags, dril_traj_info* info) {
    EvalPoll p;
    { int rc = path == 2 ? traj_fused_run(h, o, r, p) : path == 1 ? traj_persistent_run(h, o, r, p) : traj_stepwise_run(h, o, r, p); if (rc) return rc; }
    const TrajCopyOut c = traj_copy_out(h->stream, r.rec, observations, (uint32_t*)actions, rewards, lengths, end_flags);
    if (const std::string msg = traj_report("dril_collect_trajectory_device", c, r.rec.Tcap, (int32_t)p.steps, p.launches, path, info); !msg.empty()) return fail(h, DRIL_ERR_HIP, msg);
    return DRIL_OK;
}
}  // namespace
DRIL_EXPORT int32_t dril_traj_options_default(dril_traj_options* o) {
    if (!o) return DRIL_ERR_INVALID_ARG;
    std::memset(o, 0, sizeof(*o));
    o->n_trajectories = 1; o->deterministic = 1;                                       // trajectory_utils.jl:6-8
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_trajectory_capacity(const dril_handle* h, const dril_traj_options* o, int32_t* capacity) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!o || !capacity || o->max_steps < 0) return fail(const_cast<dril_handle*>(h), DRIL_ERR_INVALID_ARG, "dril_trajectory_capacity: options and capacity != NULL, max_steps >= 0");
    if (h->external) return fail(const_cast<dril_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_trajectory_capacity: the envs of DRIL_ENV_EXTERNAL live on the host, with the caller");
    *capacity = traj_capacity(o->max_steps, h->env.episode_len);
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_collect_trajectory_device(dril_handle* h, const dril_traj_options* o, float* observations, void* actions, float* rewards, int32_t* lengths,
                                                   uint8_t* end_flags, dril_traj_info* info) {
    NEED(h); NOT_EXTERNAL(h, "dril_collect_trajectory_device");
    if (const std::string msg = traj_options_error("dril_collect_trajectory_device", o, observations && actions && rewards && lengths && end_flags, h->cfg.n_envs); !msg.empty()) return fail(h, DRIL_ERR_INVALID_ARG, msg);
    if (h->env.is_world() && o->n_trajectories % h->env.agents() != 0)
        return fail(h, DRIL_ERR_INVALID_ARG, "dril_collect_trajectory_device: the env is a world of " + std::to_string(h->env.agents()) + " agents and whole worlds are recorded: n_trajectories " + std::to_string(o->n_trajectories) + " is not a multiple of " + std::to_string(h->env.agents()));
    int32_t Tcap = 0;
    if (const std::string msg = traj_size_error("dril_collect_trajectory_device", o, h->env.episode_len, h->D, h->discrete ? 1 : h->A, info, &Tcap); !msg.empty()) return fail(h, DRIL_ERR_INVALID_ARG, msg);
    { int rc = ensure_wimg(h); if (rc) return rc; }
    // the opt-in one-launch form where evaluate_modes_kernel applies; elsewhere (generic shapes, plug-ins, DRIL_FORCE_STEPWISE) the request falls back silently
    const bool persistent = o->reserved[DRIL_TRAJ_OPT_PERSISTENT] != 0 && eval_persistent_applies(h, true);
    const bool fused = eval_fused_applies(h, o->reserved[DRIL_TRAJ_OPT_PERSISTENT] != 0);   // path 2: the recording mode of a plug-in's own evaluation kernel (never both)
    EvalKeep keep; eval_keep_list(h, persistent || fused, keep);
    { int rc = eval_buffers(h, keep, 0); if (rc) return rc; }
    TrajRun run{};
    { int rc = traj_prepare(h, o, Tcap, run); if (rc) return rc; }
    // as dril_evaluate_agent_device: what training would continue from is set aside here and put back by eval_finish, on every path (set_training(env, false), :12)
    { int rc = eval_set_aside(h, keep); if (rc) return rc; }
    return eval_finish(h, keep, "dril_collect_trajectory_device", traj_device_run(h, o, run, fused ? 2 : persistent ? 1 : 0, observations, actions, rewards, lengths, end_flags, info));
}

// ---- train! ------------------------------------------------------------------------------------------
DRIL_EXPORT int32_t dril_train(dril_handle* h, int64_t max_steps, dril_ppo_stats* stats, double* fps, int32_t* iterations_done) {
    NEED(h); NOT_EXTERNAL(h, "dril_train");
    const int64_t per_iter = (int64_t)h->cfg.n_steps * h->cfg.n_envs * h->cfg.world_size;
    const int64_t iterations = max_steps / per_iter;                                   // ppo.jl:117
    int32_t done = 0;
    for (int64_t i = 0; i < iterations; ++i) {
        h->lr = h->cfg.learning_rate;                                                  // ppo.jl:155-156
        double f = 0; int rc = collect_rollout(h, &f, false);                          // ppo.jl:167
        if (rc) { if (iterations_done) *iterations_done = done; return rc; }
        if (fps) fps[i] = f;
        rc = ppo_update(h, stats ? &stats[i] : nullptr);                               // ppo.jl:188-264
        if (rc) { if (iterations_done) *iterations_done = done; return rc; }
        ++done;
    }
    if (iterations_done) *iterations_done = done;
    return DRIL_OK;
}

// ---- populations: many small PPO agents per launch (docs/population.md) ------------------------------------------------------------------
// A population joins ordinary PPO handles for batched launches: one rollout_duo_pop_kernel and one ppo_update_small_pop_kernel where P solo iterations launch
// rollout_duo_kernel and ppo_update_small_kernel P times.  It keeps no copy of member state: every verb reads each handle with the solo path's own functions
// (rollout_args, update_begin, small_update_args, update_enqueue_home, update_finish, update_resolve), so a member's result is that of its handle driven alone, bit for bit.
// While joined, the members share the population's stream: whatever a member's own verbs enqueue between population calls is ordered with the batched launches.
struct dril_population {
    std::vector<dril_handle*> members; std::vector<hipStream_t> own_streams;
    hipStream_t stream = nullptr; int device = 0, cap = 1; int64_t chunk = 16384, total_steps = 0; int n_chunks = 1;
    PinnedBuf<RolloutArgs> h_rargs; DevBuf<RolloutArgs> d_rargs; PinnedBuf<SmallUpdateArgs> h_uargs; DevBuf<SmallUpdateArgs> d_uargs;   // pinned / device: [n] and [n_chunks][n]
    DevBuf<unsigned long long> xchg;                             // n x kSmallXchgWords
    std::vector<PinnedBuf<char>> home_blocks; std::vector<UpdateHome> homes;   // one pinned block per member: where its update's results land
    std::vector<int> failed;                                     // status of a member that failed in the current call (it sits out the rest of the iteration)
    struct dril_population_info info{};
    PinnedBuf<EvalKernelArgs> h_eargs; DevBuf<EvalKernelArgs> d_eargs; // dril_population_evaluate_device: pinned / device [n]
    DevBuf<unsigned int> eval_counters; PinnedBuf<unsigned int> h_eval_counters;   // device / pinned [n]: member m's EvalAcct.counter is word m, looked at with ONE copy per K env steps
    PinnedBuf<SacEvalEvent> h_eval_events;   // pinned, grow-only: where the members' event lists land
    double eval_ms = 0;                                          // HIP-event time of the evaluate_pop_kernel launches of the last evaluation
    struct Ev { int kind; hipEvent_t a, b; }; std::vector<Ev> ev_pending; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::string err;
};
namespace {
int pop_fail(dril_population* p, int code, const std::string& msg) { p->err = msg; return code; }
#define POPCHK(p, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return pop_fail(p, DRIL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)
// "" when the handle can be a member, else why not (the shape on which a solo iteration is one rollout_duo_kernel launch and one ppo_update_small_kernel launch)
std::string pop_ineligible(const dril_handle* h, int& code) {
    code = DRIL_ERR_UNSUPPORTED;
    if (h->external) return "an external handle (DRIL_ENV_EXTERNAL): its envs live with the caller";
    if (h->env.is_world()) return "a world of a device env plug-in";
    if (h->env.module || !env_kind_info(h->cfg.env_kind)) return "a device env plug-in handle (DRIL_ENV_MODULE): populations take the built-in env kinds";
    if (normalizing(h) || h->pn.on) return "a normalising handle (NormalizeWrapperEnv collects step by step)";
    if (h->cfg.world_size > 1 || comm_ready(h)) return "world_size > 1: members are single-rank handles";
    if (h->generic || h->wide || h->cfg.hidden1 != 64) return "a generic or wide net: members have hidden_dims [64,64] with tanh";
    const UpdatePlan plan = update_plan(h);
    if (plan.B > 64) return "batch_size " + std::to_string((long long)plan.B) + " > 64: the persistent update kernel takes minibatches of 2..64 samples";
    if (h->force_stepwise || !rollout_fused_applies(h) || !rollout_duo_applies(h->cfg.hidden1, h->cfg.n_envs)) return "its collection is not one launch of rollout_duo_kernel (n_envs <= 16384, not step-granular)";
    if (h->grad_variant >= 0 || h->no_persistent || h->no_small_path || !small_persistent_applies(h, plan)) return "its update is not one launch of ppo_update_small_kernel (2 <= batch_size <= 64, default gradient variant, persistent update on)";
    return "";
}
// what fixes the kernel instance and the grid must be equal across members
std::string pop_mismatch(const dril_handle* a, const dril_handle* b, int& code) {
    const dril_config &x = a->cfg, &y = b->cfg;
    code = DRIL_ERR_INVALID_ARG;
    if (x.device != y.device) return "mixed devices (device " + std::to_string(y.device) + " against member 0's " + std::to_string(x.device) + ")";
    if (x.env_kind != y.env_kind) return "mixed env kinds (" + std::to_string(y.env_kind) + " against member 0's " + std::to_string(x.env_kind) + ")";
    if (x.n_envs != y.n_envs || x.n_steps != y.n_steps || x.batch_size != y.batch_size || x.epochs != y.epochs) return "mixed shapes (n_envs, n_steps, batch_size and epochs must equal member 0's)";
    if (x.hidden1 != y.hidden1 || x.hidden2 != y.hidden2 || x.n_hidden != y.n_hidden || x.activation != y.activation) return "mixed shapes (hidden dims and activation must equal member 0's)";
    if (x.normalize_advantage != y.normalize_advantage) return "mixed shapes (normalize_advantage must equal member 0's)";
    return "";
}
void pop_release(dril_population* p) {
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    for (size_t m = 0; m < p->members.size(); ++m) { dril_handle* h = p->members[m]; if (h->pop == p) { h->stream = p->own_streams[m]; h->pop = nullptr; } }
    for (auto& e : p->ev_pending) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    for (auto& e : p->ev_pool) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}
// HIP-event brackets of the batched kernels (member 0's cfg.profile_events), resolved when the stream is drained
void pop_ev_begin(dril_population* p, int kind) {
    if (!p->members[0]->cfg.profile_events) return;
    std::pair<hipEvent_t, hipEvent_t> ev;
    if (!p->ev_pool.empty()) { ev = p->ev_pool.back(); p->ev_pool.pop_back(); } else { hipEventCreate(&ev.first); hipEventCreate(&ev.second); }
    hipEventRecord(ev.first, p->stream);
    p->ev_pending.push_back({kind, ev.first, ev.second});
}
void pop_ev_end(dril_population* p) { if (p->members[0]->cfg.profile_events && !p->ev_pending.empty()) hipEventRecord(p->ev_pending.back().b, p->stream); }
int pop_sync(dril_population* p) {
    POPCHK(p, hipStreamSynchronize(p->stream));
    for (auto& e : p->ev_pending) {
        float ms = 0; if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) (e.kind == 0 ? p->info.last_rollout_ms : e.kind == 1 ? p->info.last_update_ms : p->eval_ms) += ms;
        p->ev_pool.push_back({e.a, e.b});
    }
    p->ev_pending.clear();
    for (dril_handle* h : p->members) prof_resolve(h);
    return DRIL_OK;
}
void pop_member_failed(dril_population* p, int m, int rc, const char* verb, int& first) {
    p->failed[m] = rc;
    if (first == DRIL_OK) { first = rc; p->err = std::string(verb) + ": member " + std::to_string(m) + ": " + p->members[m]->err; }
}
void pop_call_begin(dril_population* p) {
    (void)hipSetDevice(p->device);
    std::fill(p->failed.begin(), p->failed.end(), DRIL_OK);
    struct dril_population_info& i = p->info;
    i.last_rollout_launches = i.last_update_launches = i.last_solo_rollouts = i.last_solo_updates = 0; i.last_launches_per_iteration = 0; i.last_rollout_ms = i.last_update_ms = 0;
}
// collect_rollout of every member that has not failed in this call: ONE rollout_duo_pop_kernel launch for the members whose collection is that kernel's solo twin on the
// f16-piece forward, collect_rollout itself for the others; then per member what follows the launch in collect_rollout (monitor window, GAE)
int pop_collect(dril_population* p, double* fps, bool do_sync, int& first) {
    const int n = (int)p->members.size();
    std::vector<int> batched, solo;
    for (int m = 0; m < n; ++m) {
        dril_handle* h = p->members[m];
        if (p->failed[m]) continue;
        if (fps) fps[m] = 0;
        if (!h->env.ready) { pop_member_failed(p, m, fail(h, DRIL_ERR_NOT_INITIALISED, "dril_collect_rollout before dril_env_reset"), "dril_population_collect_rollout", first); continue; }
        { const int rcw = ensure_wimg(h); if (rcw) { pop_member_failed(p, m, rcw, "dril_population_collect_rollout", first); continue; } }
        if (rollout_fused_applies(h) && h->cfg.hidden1 == 64 && rollout_duo_applies(h->cfg.hidden1, h->env.E) && !fwd_exact(h)) batched.push_back(m); else solo.push_back(m);
    }
    if (!batched.empty()) {
        const int nbat = (int)batched.size();
        for (int k = 0; k < nbat; ++k) p->h_rargs[k] = rollout_args(p->members[batched[k]]);
        hipError_t e = hipMemcpyAsync(p->d_rargs, p->h_rargs, sizeof(RolloutArgs) * (size_t)nbat, hipMemcpyHostToDevice, p->stream);
        const auto t0 = std::chrono::steady_clock::now();
        if (fps && e == hipSuccess) e = hipStreamSynchronize(p->stream);
        pop_ev_begin(p, 0);
        if (e == hipSuccess) e = launch_rollout_pop(p->members[0]->cfg.env_kind, p->d_rargs, nbat, p->members[0]->env.E, p->stream);
        pop_ev_end(p);
        double f = 0;
        if (fps && e == hipSuccess) {   // fps = steps / wall time of collect_trajectories (rollout_buffer.jl:60-64): every member of the launch waited for the whole launch
            e = hipStreamSynchronize(p->stream);
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            f = (double)p->members[0]->N / (dt > 0 ? dt : 1e-12);
        }
        p->info.last_rollout_launches += 1; p->info.total_rollout_launches += 1;
        for (int k = 0; k < nbat; ++k) {
            const int m = batched[k]; dril_handle* h = p->members[m];
            int rc = e == hipSuccess ? DRIL_OK : fail(h, DRIL_ERR_HIP, std::string("rollout_duo_pop_kernel: ") + hipGetErrorString(e));
            if (!rc) { if (fps) fps[m] = f; h->noise_set = false; rc = monitor_collect_rollout(h); }
            if (!rc) rc = compute_gae(h);
            if (rc) pop_member_failed(p, m, rc, "dril_population_collect_rollout", first);
        }
    }
    for (int m : solo) {
        double f = 0; const int rc = collect_rollout(p->members[m], fps ? &f : nullptr, false);
        if (fps) fps[m] = f;
        p->info.last_solo_rollouts += 1; p->info.total_solo_rollouts += 1;
        if (rc) pop_member_failed(p, m, rc, "dril_population_collect_rollout", first);
    }
    if (do_sync) { const int rc = pop_sync(p); if (rc) return rc; }
    return DRIL_OK;
}
// ppo_update of every member that has not failed in this call: the members whose update is one run of the persistent kernel go through ppo_update_small_pop_kernel
// (at most cap members per launch: a pair of workgroups needs both resident at once), the others through ppo_update; ONE drain of the stream, then per member
// update_finish and what ppo_update does after its first pass (the redo of a pair that never met, or of an update that left f16's range: alone, on the solo kernels)
int pop_update(dril_population* p, dril_ppo_stats* out, int& first) {
    const int n = (int)p->members.size();
    struct Run { int m; UpdatePlan plan; UpdateTry t; };
    std::vector<Run> batched; std::vector<int> solo;
    for (int m = 0; m < n; ++m) {
        dril_handle* h = p->members[m];
        if (p->failed[m]) continue;
        if (out) std::memset(&out[m], 0, sizeof(dril_ppo_stats));
        const UpdatePlan plan = update_plan(h);
        if (!small_persistent_applies(h, plan) || update_direct_f32(h) || plan.total_steps != p->total_steps) { solo.push_back(m); continue; }
        Run r{m, plan, UpdateTry{}};
        SmallUpdateArgs u{};
        int rc = update_snapshot(h, r.t);
        if (!rc) rc = update_begin(h, plan);
        if (!rc) rc = small_update_args(h, plan, p->homes[m].keys, u);
        if (rc) { pop_member_failed(p, m, rc, "dril_population_ppo_update", first); continue; }
        p->h_uargs[(size_t)p->n_chunks * n + batched.size()] = u;                       // behind the launch table: the member's block, copied into every launch's row below
        batched.push_back(r);
    }
    const int nbat = (int)batched.size();
    hipError_t e = hipSuccess;
    if (nbat > 0) {
        int c = 0;
        for (int64_t s0 = 0; s0 < p->total_steps; s0 += p->chunk, ++c)
            for (int k = 0; k < nbat; ++k) {
                SmallUpdateArgs& u = p->h_uargs[(size_t)c * nbat + k];
                u = p->h_uargs[(size_t)p->n_chunks * n + k];                              // the member's block as small_update_args filled it (kept behind the launch table)
                u.xchg = p->xchg + (size_t)k * kSmallXchgWords; u.debug_solo = 0;
                small_update_chunk(batched[k].plan, p->chunk, s0, u);
            }
        e = hipMemcpyAsync(p->d_uargs, p->h_uargs, sizeof(SmallUpdateArgs) * (size_t)p->n_chunks * nbat, hipMemcpyHostToDevice, p->stream);
        pop_ev_begin(p, 1);
        for (c = 0; c < p->n_chunks && e == hipSuccess; ++c)
            for (int g0 = 0; g0 < nbat && e == hipSuccess; g0 += p->cap) {
                const int cnt = nbat - g0 < p->cap ? nbat - g0 : p->cap;
                e = launch_ppo_update_small_pop(p->members[0]->cfg.env_kind, p->d_uargs + (size_t)c * nbat + g0, cnt, p->xchg + (size_t)g0 * kSmallXchgWords, (size_t)cnt * kSmallXchgWords, p->stream);
                p->info.last_update_launches += 1; p->info.total_update_launches += 1;
            }
        pop_ev_end(p);
    }
    std::vector<char> enq((size_t)nbat, 0);
    for (int k = 0; k < nbat; ++k) {
        const int m = batched[k].m; dril_handle* h = p->members[m];
        int rc = e == hipSuccess ? DRIL_OK : fail(h, DRIL_ERR_HIP, std::string("ppo_update_small_pop_kernel: ") + hipGetErrorString(e));
        if (!rc) { small_update_done(h, batched[k].plan); rc = update_enqueue_home(h, batched[k].plan, p->homes[m]); }
        if (rc) pop_member_failed(p, m, rc, "dril_population_ppo_update", first); else enq[k] = 1;
    }
    if (nbat > 0) { const int rc = pop_sync(p); if (rc) return rc; }                       // ONE drain for the whole population
    for (int k = 0; k < nbat; ++k) {
        if (!enq[k]) continue;
        const int m = batched[k].m; dril_handle* h = p->members[m];
        const int64_t redo0 = h->persistent_fallbacks + h->f32_retries;
        int rc = update_finish(h, batched[k].plan, p->homes[m], out ? &out[m] : nullptr);
        rc = update_resolve(h, batched[k].t, rc, out ? &out[m] : nullptr);
        if (h->persistent_fallbacks + h->f32_retries != redo0) { p->info.last_solo_updates += 1; p->info.total_solo_updates += 1; }   // redone alone, on the solo kernels
        if (rc) pop_member_failed(p, m, rc, "dril_population_ppo_update", first);
    }
    for (int m : solo) {
        const int rc = ppo_update(p->members[m], out ? &out[m] : nullptr);
        p->info.last_solo_updates += 1; p->info.total_solo_updates += 1;
        if (rc) pop_member_failed(p, m, rc, "dril_population_ppo_update", first);
    }
    return DRIL_OK;
}
// dril_evaluate_agent_device of every member, with the pieces of the solo verb (eval_prepare .. eval_reduce).  The members whose evaluation is evaluate_kernel on the
// f16-piece forward share ONE evaluate_pop_kernel launch and ONE look at the n counters per K env steps; a member that has its episodes sits out the later launches
// (T = 0).  The others (exact-f32 forward, force_step_granular, DRIL_FORCE_STEPWISE) run the solo verb after the batched loop
int pop_evaluate(dril_population* p, const dril_eval_options* o, dril_eval_stats* out, float* ep_rewards, int32_t* ep_lengths, dril_eval_info* member_info,
                 dril_population_eval_info* info, int& first) {
    const char* verb = "dril_population_evaluate_device";
    const int n = (int)p->members.size(), n_eval = o->n_eval_episodes;
    struct Run { int m; EvalPlan pl; EvalKernelArgs g; long long steps, max_steps; unsigned int seen; int32_t launches; bool done; size_t ev_off, ev_n; };
    std::vector<Run> batched; std::vector<int> solo;
    for (int m = 0; m < n; ++m) {
        dril_handle* h = p->members[m];
        std::memset(&out[m], 0, sizeof(dril_eval_stats));
        if (member_info) std::memset(&member_info[m], 0, sizeof(dril_eval_info));
        Run r{}; r.m = m;
        int rc = eval_prepare(h, o, r.pl);
        if (rc) { pop_member_failed(p, m, rc, verb, first); continue; }
        if (!r.pl.persistent || r.pl.fused || normalizing(h) || fwd_exact(h) || h->cfg.hidden1 != 64) { solo.push_back(m); continue; }   // not evaluate_kernel<K, 64, false, true>: alone, below
        rc = eval_set_aside(h, r.pl.keep);
        if (rc) { pop_member_failed(p, m, rc, verb, first); continue; }
        EvalAcct acct{};
        rc = eval_reset(h, o, p->eval_counters + batched.size(), r.pl.cap, acct);
        if (!rc) { eval_persistent_args(h, o, r.pl.K, acct, r.g); r.max_steps = eval_max_steps(h, n_eval, r.pl.K); }
        else { pop_member_failed(p, m, rc, verb, first); r.done = true; }              // (set aside already: it is put back with the others, and takes no launch)
        batched.push_back(std::move(r));
    }
    const int nbat = (int)batched.size();
    hipError_t e = hipSuccess;
    // per round: the blocks built in pinned memory (a member that has its episodes, or ran into its bound, gets T = 0), ONE copy to the device, ONE launch, ONE copy
    // of the counters home, ONE synchronise
    for (;;) {
        int active = 0;
        for (int k = 0; k < nbat; ++k) {
            Run& r = batched[k]; dril_handle* h = p->members[r.m];
            if (!r.done && r.seen >= (unsigned int)n_eval) r.done = true;
            if (!r.done && r.steps >= r.max_steps) { r.done = true; pop_member_failed(p, r.m, fail(h, DRIL_ERR_UNSUPPORTED, "dril_evaluate_agent_device: no episode finishes"), verb, first); }
            EvalKernelArgs& g = p->h_eargs[k];
            g = r.g; g.r.T = r.done ? 0 : r.pl.K; g.step0 = (int32_t)r.steps;
            if (!r.done) { ++active; r.steps += r.pl.K; r.launches += 1; }
        }
        if (active == 0) break;
        e = hipMemcpyAsync(p->d_eargs, p->h_eargs, sizeof(EvalKernelArgs) * (size_t)nbat, hipMemcpyHostToDevice, p->stream);
        pop_ev_begin(p, 2);
        if (e == hipSuccess) e = launch_evaluate_pop(p->members[0]->cfg.env_kind, p->d_eargs, nbat, p->members[0]->cfg.n_envs, p->stream);
        pop_ev_end(p);
        if (e == hipSuccess) e = hipMemcpyAsync(p->h_eval_counters, p->eval_counters, sizeof(unsigned int) * (size_t)nbat, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
        if (info) { info->launches += 1; info->looks += 1; }
        if (e != hipSuccess) break;
        for (int k = 0; k < nbat; ++k) if (!batched[k].done) batched[k].seen = p->h_eval_counters[k];
    }
    if (e != hipSuccess)
        for (Run& r : batched) if (!p->failed[r.m]) pop_member_failed(p, r.m, fail(p->members[r.m], DRIL_ERR_HIP, std::string("evaluate_pop_kernel: ") + hipGetErrorString(e)), verb, first);
    // the event lists home (one pinned area for all members), then every member's state put back; ONE drain
    size_t total = 0;
    for (Run& r : batched) { r.ev_off = total; r.ev_n = p->failed[r.m] ? 0 : (size_t)std::min<long long>(r.seen, r.pl.cap); total += r.ev_n; }
    if (total > 0) (void)p->h_eval_events.grow(total);                                 // (a failure leaves it empty: the copies below report it)
    for (Run& r : batched) {
        dril_handle* h = p->members[r.m];
        const std::string msg = h->err;
        int rc = DRIL_OK;
        if (r.ev_n > 0) {
            if (!p->h_eval_events) rc = fail(h, DRIL_ERR_HIP, "dril_population_evaluate_device: no pinned memory for the event lists");
            else { const hipError_t ce = hipMemcpyAsync(p->h_eval_events + r.ev_off, h->eval_events, r.ev_n * sizeof(SacEvalEvent), hipMemcpyDeviceToHost, p->stream);
                   if (ce != hipSuccess) rc = fail(h, DRIL_ERR_HIP, std::string("dril_population_evaluate_device: ") + hipGetErrorString(ce)); }
        }
        const int rr = eval_put_back(h, r.pl.keep);
        if (p->failed[r.m]) h->err = msg;                                               // what the solo call would have said
        else if (rc || rr) pop_member_failed(p, r.m, rc ? rc : rr, verb, first);
    }
    if (nbat > 0) { const int rc = pop_sync(p); if (rc) { for (Run& r : batched) if (!p->failed[r.m]) p->failed[r.m] = rc; if (first == DRIL_OK) first = rc; } }
    for (Run& r : batched) {
        if (p->failed[r.m]) continue;
        eval_reduce(p->h_eval_events + r.ev_off, (int64_t)r.ev_n, o, &out[r.m], ep_rewards ? ep_rewards + (size_t)r.m * n_eval : nullptr, ep_lengths ? ep_lengths + (size_t)r.m * n_eval : nullptr);
        if (member_info) { dril_eval_info& mi = member_info[r.m]; mi.path = 1; mi.launches = r.launches; mi.steps_enqueued = (int32_t)r.steps; mi.events = (int32_t)r.seen; }
        if (info) info->batched_members += 1;
    }
    for (int m : solo) {
        const int rc = dril_evaluate_agent_device(p->members[m], o, &out[m], ep_rewards ? ep_rewards + (size_t)m * n_eval : nullptr, ep_lengths ? ep_lengths + (size_t)m * n_eval : nullptr,
                                                  member_info ? &member_info[m] : nullptr);
        if (info) info->solo_members += 1;
        if (rc) pop_member_failed(p, m, rc, verb, first);
    }
    if (info) info->kernel_ms = p->eval_ms;
    return DRIL_OK;
}
}  // namespace

#define JCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { const std::string msg = std::string("dril_population_join: " #expr ": ") + hipGetErrorString(_e); pop_release(p); return fail(nullptr, DRIL_ERR_HIP, msg); } } while (0)
DRIL_EXPORT int32_t dril_population_join(dril_handle** members, int32_t n, dril_population** out) {
    if (!out) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_population_join: null out");
    *out = nullptr;
    if (!members || n < 1 || n > DRIL_POPULATION_MAX) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_population_join: 1.." + std::to_string(DRIL_POPULATION_MAX) + " members");
    for (int m = 0; m < n; ++m) {
        const dril_handle* h = members[m];
        const std::string who = "dril_population_join: member " + std::to_string(m) + ": ";
        if (!h) return fail(nullptr, DRIL_ERR_INVALID_ARG, who + "null handle");
        for (int q = 0; q < m; ++q) if (members[q] == h) return fail(nullptr, DRIL_ERR_INVALID_ARG, who + "the same handle as member " + std::to_string(q));
        if (h->pop) return fail(nullptr, DRIL_ERR_INVALID_ARG, who + "the handle is already a member of a population");
        int code = DRIL_OK;
        std::string why = pop_ineligible(h, code);
        if (why.empty() && m > 0) why = pop_mismatch(members[0], h, code);
        if (!why.empty()) return fail(nullptr, code, who + why);
    }
    dril_handle* h0 = members[0];
    (void)hipSetDevice(h0->cfg.device);
    dril_population* p = new dril_population();
    p->device = h0->cfg.device;
    p->cap = h0->num_cus / 4 > 0 ? h0->num_cus / 4 : 1;                               // two workgroups per member, at most half the CUs per launch
    if (const char* e = debug_env("DRIL_POP_CAP")) { const int c = std::atoi(e); if (c > 0 && c < p->cap) p->cap = c; }   // tests: more than one launch per verb
    p->chunk = h0->small_chunk;
    for (int m = 0; m < n; ++m) if (members[m]->small_chunk < p->chunk) p->chunk = members[m]->small_chunk;
    p->total_steps = update_plan(h0).total_steps;
    p->n_chunks = (int)((p->total_steps + p->chunk - 1) / p->chunk);
    JCHK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    JCHK(p->h_rargs.alloc((size_t)n));
    JCHK(p->h_uargs.alloc(((size_t)p->n_chunks + 1) * n));   // the launch table, and behind it one block per member
    JCHK(p->d_rargs.alloc((size_t)n));
    JCHK(p->d_uargs.alloc((size_t)p->n_chunks * n));
    JCHK(p->xchg.alloc((size_t)n * kSmallXchgWords));
    JCHK(p->h_eargs.alloc((size_t)n));
    JCHK(p->d_eargs.alloc((size_t)n));
    JCHK(p->h_eval_counters.alloc((size_t)n));
    JCHK(p->eval_counters.alloc((size_t)n));
    p->home_blocks.resize((size_t)n); p->homes.assign((size_t)n, UpdateHome{}); p->failed.assign((size_t)n, DRIL_OK);
    for (int m = 0; m < n; ++m) {
        const dril_handle* h = members[m];
        const size_t st = ((size_t)p->total_steps * 16 * 4 + 15) & ~(size_t)15, ev = 4 * (size_t)h->ev_blocks * 8, keys = (size_t)h->cfg.epochs * 8;
        JCHK(p->home_blocks[m].alloc(st + ev + keys + 16));
        char* b = p->home_blocks[m];
        p->homes[m] = UpdateHome{(float*)b, (double*)(b + st), (int*)(b + st + ev + keys), (uint64_t*)(b + st + ev)};
    }
    for (int m = 0; m < n; ++m) {                                                      // from here on nothing fails: the members move onto the population's stream
        dril_handle* h = members[m];
        (void)hipStreamSynchronize(h->stream);
        p->members.push_back(h); p->own_streams.push_back(h->stream);
        h->stream = p->stream; h->pop = p;
    }
    p->info.members = n; p->info.cap = p->cap;
    *out = p;
    return DRIL_OK;
}
#undef JCHK
DRIL_EXPORT int32_t dril_population_destroy(dril_population* p) { if (p) pop_release(p); return DRIL_OK; }
DRIL_EXPORT const char* dril_population_last_error(const dril_population* p) { return p ? p->err.c_str() : g_create_error.c_str(); }
DRIL_EXPORT int32_t dril_population_info(const dril_population* p, struct dril_population_info* out) {
    if (!p || !out) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_population_info: null argument");
    *out = p->info;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_population_collect_rollout(dril_population* p, double* fps) {
    if (!p) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null population");
    pop_call_begin(p);
    int first = DRIL_OK;
    const int rc = pop_collect(p, fps, true, first);
    p->info.last_launches_per_iteration = p->info.last_rollout_launches;
    return rc ? rc : first;
}
DRIL_EXPORT int32_t dril_population_ppo_update(dril_population* p, dril_ppo_stats* out) {
    if (!p) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null population");
    pop_call_begin(p);
    int first = DRIL_OK;
    const int rc = pop_update(p, out, first);
    p->info.last_launches_per_iteration = p->info.last_update_launches;
    return rc ? rc : first;
}
DRIL_EXPORT int32_t dril_population_train(dril_population* p, int64_t max_steps, dril_ppo_stats* stats, double* fps, int32_t* iterations_done) {
    if (!p) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null population");
    pop_call_begin(p);
    const int n = (int)p->members.size();
    const dril_handle* h0 = p->members[0];
    const int64_t per_iter = (int64_t)h0->cfg.n_steps * h0->cfg.n_envs * h0->cfg.world_size;
    const int64_t iterations = max_steps / per_iter;                                   // ppo.jl:117
    int32_t done = 0; int first = DRIL_OK, rc = DRIL_OK;
    for (int64_t i = 0; i < iterations && rc == DRIL_OK && first == DRIL_OK; ++i) {
        for (dril_handle* h : p->members) h->lr = h->cfg.learning_rate;                // ppo.jl:155-156
        rc = pop_collect(p, fps ? fps + i * n : nullptr, false, first);                // ppo.jl:167
        if (rc == DRIL_OK) rc = pop_update(p, stats ? stats + i * n : nullptr, first); // ppo.jl:188-264; a member that failed sits out, the others finish the iteration
        if (rc == DRIL_OK && first == DRIL_OK) ++done;
    }
    if (rc != DRIL_OK || first != DRIL_OK) (void)hipStreamSynchronize(p->stream);
    const int64_t ran = done + ((rc || first) ? 1 : 0);
    p->info.last_launches_per_iteration = ran > 0 ? (double)(p->info.last_rollout_launches + p->info.last_update_launches) / (double)ran : 0.0;
    if (iterations_done) *iterations_done = done;
    return rc ? rc : first;
}
DRIL_EXPORT int32_t dril_population_evaluate_device(dril_population* p, const dril_eval_options* o, dril_eval_stats* out, float* episode_rewards, int32_t* episode_lengths,
                                                    dril_eval_info* member_info, dril_population_eval_info* info) {
    if (!p) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_population_evaluate_device: null population");
    if (!o || !out || o->n_eval_episodes < 1 || o->poll_steps < 0) return pop_fail(p, DRIL_ERR_INVALID_ARG, "dril_population_evaluate_device: options and out != NULL, n_eval_episodes >= 1, poll_steps >= 0");
    (void)hipSetDevice(p->device);
    std::fill(p->failed.begin(), p->failed.end(), DRIL_OK);
    p->eval_ms = 0;
    if (info) std::memset(info, 0, sizeof(*info));
    int first = DRIL_OK;
    const int rc = pop_evaluate(p, o, out, episode_rewards, episode_lengths, member_info, info, first);
    return rc ? rc : first;
}

DRIL_EXPORT int64_t dril_debug_device_bytes_live(void) { return g_devmem_live_bytes.load(); }
DRIL_EXPORT const char* dril_device_info(const dril_handle* h) { return h ? h->device_info.c_str() : ""; }

// ---- measurement ----------------------------------------------------------------------------------------
DRIL_EXPORT int32_t dril_profile_get(dril_handle* h, int32_t kid, double* total_ms, int64_t* launches) {
    NEED(h); if (kid < 0 || kid >= DRIL_K_COUNT) return fail(h, DRIL_ERR_INVALID_ARG, "bad kernel id");
    int rc = sync(h); if (rc) return rc;
    if (total_ms) *total_ms = h->prof_ms[kid]; if (launches) *launches = h->prof_n[kid];
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_profile_launches(dril_handle* h, int32_t kid, int64_t* all_launches) {
    NEED(h); if (kid < 0 || kid >= DRIL_K_COUNT || !all_launches) return fail(h, DRIL_ERR_INVALID_ARG, "bad kernel id");
    *all_launches = h->prof_all[kid];
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_profile_reset(dril_handle* h) {
    NEED(h); int rc = sync(h); if (rc) return rc;
    for (int i = 0; i < DRIL_K_COUNT; ++i) { h->prof_ms[i] = 0; h->prof_n[i] = 0; h->prof_all[i] = 0; }
    return DRIL_OK;
}
DRIL_EXPORT const char* dril_kernel_name(int32_t kid) {
    static const char* names[] = {"rollout_kernel", "gae_kernel", "adv_moments_kernel", "ppo_grad_kernel", "grad_reduce_kernel", "adam_kernel", "ncclAllReduce", "pack_records_kernel", "explained_var_kernel"};
    static_assert(sizeof(names) / sizeof(names[0]) == DRIL_K_COUNT, "one name per kernel class");
    return (kid >= 0 && kid < DRIL_K_COUNT) ? names[kid] : "?";
}
DRIL_EXPORT int32_t dril_kernel_count(void) { return DRIL_K_COUNT; }
static const char* grad_kernel_base(int variant) {
    switch (variant) {
        case 0: return "ppo_grad_kernel: f32 (v_mfma_f32_32x32x2_f32)";
        case 2: return "ppo_grad_wide_kernel: f32 (v_mfma_f32_32x32x2_f32)";
        case 6: return "ppo_update_small_kernel: f32 (f16x2 split, f32 accumulate; v_mfma_f32_32x32x16_f16 x 3 per k16 step on two-piece f16 operands = 2^-24 relative, input layer on v_mfma_f32_32x32x2_f32; two persistent workgroups (actor | critic), all optimiser steps of the iteration in one launch)";
        case 5: return "ppo_grad_pair_kernel: f32 (f16x2 split, f32 accumulate; v_mfma_f32_32x32x16_f16 x 3 per k16 step on two-piece f16 operands = 2^-24 relative, input layer on v_mfma_f32_32x32x2_f32)";
        case 4: return "ppo_grad_wide_split_kernel: f32 (f16x2 split, f32 accumulate; v_mfma_f32_32x32x16_f16 x 3 per k16 step on two-piece f16 operands = 2^-24 relative, input layer on f32 MFMAs, dW1 / dW3 in f32 on the vector ALU)";
        case 3: return "generic path: f32 contractions (sac_gemm_*; large ones bf16x3 split, f32 accumulate)";
        default: return "none yet";
    }
}
DRIL_EXPORT const char* dril_grad_kernel_info(const dril_handle* h) {
    if (!h) return "?";
    const char* base = grad_kernel_base(h->last_variant);
    if (h->last_variant < 0 || h->last_variant == 6) return base;              // no step yet; ppo_update_small_kernel has no slab grid
    std::snprintf(h->grad_info, sizeof(h->grad_info), "%s; grid G=%d Gc=%d", base, h->last_G, h->last_Gc);   // what ppo_step launched: slabs (ppo_grad_pair_kernel: pairs) of the actor, of the critic
    return h->grad_info;
}
DRIL_EXPORT const char* dril_version(void) { return "dril_hip 0.2 (gfx950, abi 2)"; }
