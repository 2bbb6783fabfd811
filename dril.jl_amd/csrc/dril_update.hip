// dril_update.hip — the PPO update of the handle (dril_handle.h): one optimiser step (ppo_step: which gradient kernel, which grid, which tail), one update in the pieces a
// population shares with it, the exact-f32 redo and its latch, and the parity entry points dril_ppo_loss_grad / dril_apply_gradients.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dril_handle.h"

using namespace dril;
using namespace dril::ppo;

namespace {
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
}  // namespace
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

DRIL_EXPORT int32_t dril_debug_get_step_stats(dril_handle* h, float* out, size_t rows) {
    NEED(h);
    if (!out || (int64_t)rows > h->last_update_steps || rows * 16 > h->step_stats.size()) return fail(h, DRIL_ERR_INVALID_ARG, "dril_debug_get_step_stats: null pointer, or more rows than the last update had optimiser steps");
    HIPCHK(h, hipMemcpyAsync(out, h->step_stats, rows * 16 * 4, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}

namespace dril::ppo {
// One update in the pieces that ppo_update_once runs in order, and that a population (dril_population_ppo_update) runs member by member around ONE batched launch:
//   update_begin (sizes, memsets, packed records) -> [small_update_args + the persistent kernel | the per-step kernels] -> update_enqueue_home (explained variance,
//   max |W2|, the copies home) -> the stream drained -> update_finish (the statistics, the handle's counters, the status)
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
    h->used_f16 = false; h->spin_timeout = false; h->last_update_steps = total_steps;
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
// the one-launch update of a generic handle (dril_update_fused_enable, dril_update_generic_small.hip).  Eligibility is the handle's own and does not change between
// updates: generic, single rank, 2 <= batch_size <= 64, no pinned route, a net inside the kernel's caps
std::string update_fused_unavailable(const dril_handle* h) {
    if (!h->generic) return "the handle runs the fused kernels of a built-in env kind (two equal tanh layers of 32 / 64 / 128 / 256): at batch_size <= 64 on hidden_dims [64,64] its update already is one launch of ppo_update_small_kernel, and larger minibatches fill the chip per step; nothing to enable";
    if (h->cfg.world_size > 1 || comm_ready(h) || h->force_allreduce) return "the handle is part of a data-parallel job (world_size > 1, a ready communicator or DRIL_FORCE_ALLREDUCE): its optimiser step all-reduces between the gradient and Adam, which one launch cannot hold; keep the per-step route, which is the default";
    const int64_t B = h->cfg.batch_size;
    if (B < kGuMinBatch || B > kGuMaxBatch) return "batch_size = " + std::to_string(B) + ": the kernel holds a minibatch of " + std::to_string(kGuMinBatch) + " to " + std::to_string(kGuMaxBatch) + " samples in one workgroup; larger minibatches are not launch-bound: keep the per-step route, which is the default";
    if (h->no_persistent) return "DRIL_NO_PERSISTENT_UPDATE is set: every update of this handle runs the per-step kernels; unset it and create the handle again";
    if (h->grad_variant >= 0) return "DRIL_GRAD_VARIANT is set: it pins the per-step kernels; unset it and create the handle again";
    const std::string why = generic_update_unfit(h->gd, h->P);
    if (!why.empty()) return why;
    return "";
}
bool update_fused_applies(const dril_handle* h, const UpdatePlan& p) { return h->update_fused && p.total_steps > 0 && update_fused_unavailable(h).empty(); }
// the arithmetic is f32: no range redo follows
void update_fused_done(dril_handle* h, const UpdatePlan& p, int64_t launches) {
    h->adam_steps += p.total_steps; h->wimg_dirty = true; h->last_variant = 7; h->used_f16 = false;
    h->update_fused_path = 1; h->update_fused_launches = launches;
}
int generic_update_args(dril_handle* h, const UpdatePlan& p, uint64_t* keys, GenericUpdateArgs& g) {
    g = GenericUpdateArgs{};
    { const int rc = small_update_args(h, p, keys, g.u); if (rc) return rc; }
    g.obs = h->obs; g.actions = h->act; g.adv = h->adv; g.ret = h->ret; g.logp = h->logp;
    return DRIL_OK;
}
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
}  // namespace dril::ppo
namespace {
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
    const bool fused = !persistent && update_fused_applies(h, plan);
    h->update_fused_path = 0; h->update_fused_launches = 0;
    if (fused) {
        std::vector<uint64_t> keys((size_t)h->cfg.epochs);
        GenericUpdateArgs g{};
        { int rca = generic_update_args(h, plan, keys.data(), g); if (rca) return rca; }
        HIPCHK(h, hipStreamSynchronize(h->stream));                                    // (keys is a stack-lifetime host buffer)
        int64_t launches = 0;
        for (int64_t s0 = 0; s0 < total_steps; s0 += h->update_fused_chunk, ++launches) {
            small_update_chunk(plan, h->update_fused_chunk, s0, g.u);
            prof_begin(h, DRIL_K_PPO_GRAD);
            HIPCHK(h, launch_ppo_update_generic_small(h->gd, g, h->stream));
            prof_end(h);
        }
        update_fused_done(h, plan, launches);
        step = total_steps;
    }
    for (int ep = 0; ep < h->cfg.epochs && !persistent && !fused; ++ep) {
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
bool update_may_retry(const dril_handle* h) { return !h->generic && h->grad_variant < 0 && !h->no_f32_retry; }
int update_run_direct_f32(dril_handle* h, dril_ppo_stats* out) {
    if (h->f32_latch_left > 0) h->f32_latch_left -= 1;
    const int gv = h->grad_variant; h->grad_variant = 0;
    const int rc = ppo_update_once(h, out);
    h->grad_variant = gv; h->f32_direct_updates += 1;
    if (out) out->f32_path = 2;
    return rc;
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
}  // namespace
namespace dril::ppo {
// (a) known in advance that f16 cannot hold this update: a W2 entry out of range, or the latch (kRetryLatchAfter consecutive redone updates: the workload lives outside
//     f16's range, so the next kRetryLatchUpdates run the exact-f32 kernels at once instead of paying an f16 pass + snapshot + redo each) — no wasted pass, no snapshot
bool update_direct_f32(const dril_handle* h) { return update_may_retry(h) && (h->f32_latch_left > 0 || !(h->w2max < kFwdSplitMaxW)); }
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
}  // namespace dril::ppo
DRIL_EXPORT int32_t dril_ppo_update(dril_handle* h, dril_ppo_stats* out) { NEED(h); return ppo_update(h, out); }
DRIL_EXPORT int32_t dril_update_fused_enable(dril_handle* h, int32_t on) {
    NEED(h);
    if (on) { const std::string why = update_fused_unavailable(h); if (!why.empty()) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_update_fused_enable: " + why); }
    h->update_fused = on != 0;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_update_fused_info(const dril_handle* h, dril_update_fused_report* out) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!out) return fail(const_cast<dril_handle*>(h), DRIL_ERR_INVALID_ARG, "dril_update_fused_info: null out pointer");
    std::memset(out, 0, sizeof(*out));
    const std::string why = update_fused_unavailable(h);
    out->available = why.empty() ? 1 : 0; out->enabled = h->update_fused ? 1 : 0;
    out->max_width = kGuMaxWidth; out->max_obs_dim = kGuMaxObs; out->max_action_dim = kGuMaxAct; out->max_params = kGuMaxParams; out->max_hidden_layers = kMaxHidden;
    out->min_batch = kGuMinBatch; out->max_batch = kGuMaxBatch; out->faster_up_to_batch = kGuFasterBatch;
    out->last_update_path = h->update_fused_path; out->last_update_launches = h->update_fused_launches; out->steps_per_launch = h->update_fused_chunk;
    std::snprintf(out->reason, sizeof(out->reason), "%s", why.c_str());
    return DRIL_OK;
}
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
