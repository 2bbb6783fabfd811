// dril_pop.hip — populations of PPO handles (dril_handle.h): struct dril_population and the dril_population_* verbs.  Calls only what dril_handle.h declares.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "dril_handle.h"

using namespace dril;
using namespace dril::ppo;

// ---- populations: many small PPO agents per launch (docs/population.md) ------------------------------------------------------------------
// A population joins ordinary PPO handles for batched launches: one rollout_duo_pop_kernel and one ppo_update_small_pop_kernel where P solo iterations launch
// rollout_duo_kernel and ppo_update_small_kernel P times.  Normalising members (NormalizeWrapperEnv with dril_norm_rollout_enable on) collect through one
// rollout_norm_pop_kernel launch, after each member's opening observe.  It keeps no copy of member state: every verb reads each handle with the solo path's own functions
// (rollout_args, update_begin, small_update_args, update_enqueue_home, update_finish, update_resolve), so a member's result is that of its handle driven alone, bit for bit.
// Handles of ONE device env plug-in code object whose solo iteration is the fused rollout plus the one-launch generic update join as well ("Plug-in members"): their
// collections are one launch of the code object's dril_env_plugin_rollout_pop, their updates one launch of ppo_update_generic_small_pop_kernel per chunk, no cap.
// While joined, the members share the population's stream: whatever a member's own verbs enqueue between population calls is ordered with the batched launches.
struct dril_population {
    std::vector<dril_handle*> members; std::vector<hipStream_t> own_streams;
    hipStream_t stream = nullptr; int device = 0, cap = 1; int64_t chunk = 16384, total_steps = 0; int n_chunks = 1;
    PinnedBuf<NormRolloutArgs> h_nargs; DevBuf<NormRolloutArgs> d_nargs;   // normalising members: the blocks of rollout_norm_pop_kernel, pinned / device [n]
    PinnedBuf<RolloutArgs> h_rargs; DevBuf<RolloutArgs> d_rargs; PinnedBuf<SmallUpdateArgs> h_uargs; DevBuf<SmallUpdateArgs> d_uargs;   // pinned / device: [n] and [n_chunks][n]
    DevBuf<unsigned long long> xchg;                             // n x kSmallXchgWords
    // plug-in members (docs/population.md, "Plug-in members"): the blocks of the plug-in's dril_env_plugin_rollout_pop, pinned / device [n], and of
    // ppo_update_generic_small_pop_kernel, pinned [n_chunks + 1][n] (the launch table, and behind it one block per member) / device [n_chunks][n]
    PinnedBuf<DrilEnvRolloutArgs> h_margs; DevBuf<DrilEnvRolloutArgs> d_margs; PinnedBuf<GenericUpdateArgs> h_gargs; DevBuf<GenericUpdateArgs> d_gargs;
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
// whether the collection of a plug-in handle is ONE launch of its code object's fused rollout kernel, the population entry aside
bool module_rollout_fused(const dril_handle* h) { return h->env.module && !h->env.is_world() && h->fused_rollout && !h->pn.on && !h->force_stepwise && fused_rollout_unavailable(h).empty(); }
// "" when a device env plug-in handle can be a member, else why not and what to do: its solo iteration is exactly one dril_env_plugin_rollout launch plus
// ceil(steps / update_fused_chunk) launches of ppo_update_generic_small_kernel, and its code object carries the population entry of the rollout
std::string pop_plugin_ineligible(const dril_handle* h) {
    const std::string who = std::string("device env plug-in \"") + h->env.desc.name + "\": ";
    if (h->pn.on) return who + "NormalizeWrapperEnv is on (dril_normalize_enable): its collection is step-granular; populations take plug-in handles that collect with the fused rollout";
    if (h->force_stepwise) return who + "DRIL_FORCE_STEPWISE is set: every collection of this handle runs the step-granular launches; unset it and create the handle again";
    if (!h->fused_rollout) return who + "its collection is step-granular: a plug-in handle becomes eligible with the one-launch collection, dril_rollout_fused_enable(h, 1), and the one-launch update, dril_update_fused_enable(h, 1)";
    { const std::string why = fused_rollout_unavailable(h); if (!why.empty()) return who + "its fused rollout is not available: " + why; }
    if (!h->update_fused) return who + "its update runs the per-step kernels: a plug-in handle becomes eligible with the one-launch update, dril_update_fused_enable(h, 1)";
    { const std::string why = update_fused_unavailable(h); if (!why.empty()) return who + "its one-launch update is not available: " + why; }
    if (update_plan(h).total_steps < 1) return who + "epochs < 1: there is no update to batch";
    const EnvModuleRolloutPop& r = h->env.rollout_pop;
    if (!r.reason.empty()) return who + r.reason;
    if (h->env.scaling && !r.fn_scaled) return who + "ScalingWrapperEnv is on, but the code object has no dril_env_plugin_rollout_pop_scaled kernel: rebuild it with this library's include/device/dril_env_rollout_pop.h (DRIL_ENV_PLUGIN_ROLLOUT_POP)";
    if (r.desc.tile != h->env.rollout.desc.tile || r.desc.threads != h->env.rollout.desc.threads || r.desc.max_width != h->env.rollout.desc.max_width) return who + "the population entry was compiled with another tile, thread count or maximum width than the fused rollout of the same code object: rebuild the plug-in from one source";
    return "";
}
// "" when the handle can be a member, else why not (the shape on which a solo iteration is one rollout_duo_kernel launch and one ppo_update_small_kernel launch; for a
// device env plug-in: pop_plugin_ineligible)
std::string pop_ineligible(const dril_handle* h, int& code) {
    code = DRIL_ERR_UNSUPPORTED;
    if (h->external) return "an external handle (DRIL_ENV_EXTERNAL): its envs live with the caller";
    if (h->env.is_world()) return "a world of a device env plug-in";
    if (h->env.module) return pop_plugin_ineligible(h);
    if (!env_kind_info(h->cfg.env_kind)) return "a device env plug-in handle (DRIL_ENV_MODULE): populations take the built-in env kinds";
    if (h->pn.on || (normalizing(h) && !h->norm_rollout)) return "a normalising handle (NormalizeWrapperEnv collects step by step): a built-in handle becomes eligible with the one-launch collection, dril_norm_rollout_enable(h, 1)";
    if (normalizing(h)) { const std::string why = norm_rollout_unavailable(h); if (!why.empty()) return "a normalising handle whose one-launch collection is not available: " + why; }
    if (h->cfg.world_size > 1 || comm_ready(h)) return "world_size > 1: members are single-rank handles";
    if (h->generic || h->wide || h->cfg.hidden1 != 64) return "a generic or wide net: members have hidden_dims [64,64] with tanh";
    const UpdatePlan plan = update_plan(h);
    if (plan.B > 64) return "batch_size " + std::to_string((long long)plan.B) + " > 64: the persistent update kernel takes minibatches of 2..64 samples";
    if (!normalizing(h) && (h->force_stepwise || !rollout_fused_applies(h) || !rollout_duo_applies(h->cfg.hidden1, h->cfg.n_envs))) return "its collection is not one launch of rollout_duo_kernel (n_envs <= 16384, not step-granular)";
    if (h->grad_variant >= 0 || h->no_persistent || h->no_small_path || !small_persistent_applies(h, plan)) return "its update is not one launch of ppo_update_small_kernel (2 <= batch_size <= 64, default gradient variant, persistent update on)";
    return "";
}
// what fixes the kernel instance and the grid must be equal across members
std::string pop_mismatch(const dril_handle* a, const dril_handle* b, int& code) {
    const dril_config &x = a->cfg, &y = b->cfg;
    code = DRIL_ERR_INVALID_ARG;
    if (x.device != y.device) return "mixed devices (device " + std::to_string(y.device) + " against member 0's " + std::to_string(x.device) + ")";
    if ((a->env.module != nullptr) != (b->env.module != nullptr)) return "mixed members (device env plug-in handles and built-in env kinds do not share a launch: one population each)";
    if (a->env.module) {
        if (a->env.code_hash != b->env.code_hash || a->env.code_size != b->env.code_size) return std::string("mixed code objects (plug-in \"") + b->env.desc.name + "\" against member 0's \"" + a->env.desc.name + "\": the members run ONE code object's kernel)";
        if (a->env.scaling != b->env.scaling) return "mixed scaling (ScalingWrapperEnv must be on for every member or for none)";
    }
    if (x.env_kind != y.env_kind) return "mixed env kinds (" + std::to_string(y.env_kind) + " against member 0's " + std::to_string(x.env_kind) + ")";
    if (x.n_envs != y.n_envs || x.n_steps != y.n_steps || x.batch_size != y.batch_size || x.epochs != y.epochs) return "mixed shapes (n_envs, n_steps, batch_size and epochs must equal member 0's)";
    if (x.hidden1 != y.hidden1 || x.hidden2 != y.hidden2 || x.n_hidden != y.n_hidden || x.activation != y.activation) return "mixed shapes (hidden dims and activation must equal member 0's)";
    if (a->env.module) {
        const GenericDims &g = a->gd, &k = b->gd;
        bool same = g.nh == k.nh && g.act == k.act && g.D == k.D && g.A == k.A && g.discrete == k.discrete;
        for (int l = 0; same && l < g.nh; ++l) same = g.H[l] == k.H[l];
        if (!same) return "mixed shapes (the number of hidden layers, every width and the activation must equal member 0's)";
    }
    if (x.normalize_advantage != y.normalize_advantage) return "mixed shapes (normalize_advantage must equal member 0's)";
    if ((x.norm_obs != 0) != (y.norm_obs != 0) || (x.norm_reward != 0) != (y.norm_reward != 0) || (x.norm_training != 0) != (y.norm_training != 0) || a->norm_rollout != b->norm_rollout)
        return "mixed NormalizeWrapperEnv (norm_obs, norm_reward, norm_training and dril_norm_rollout_enable must equal member 0's; clips, epsilon, norm_gamma and the statistics are free)";
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
    std::vector<int> batched, nbatched, mbatched, solo;           // one rollout_duo_pop_kernel launch; one rollout_norm_pop_kernel launch; one launch of the plug-in's dril_env_plugin_rollout_pop; alone
    for (int m = 0; m < n; ++m) {
        dril_handle* h = p->members[m];
        if (p->failed[m]) continue;
        if (fps) fps[m] = 0;
        if (!h->env.ready) { pop_member_failed(p, m, fail(h, DRIL_ERR_NOT_INITIALISED, "dril_collect_rollout before dril_env_reset"), "dril_population_collect_rollout", first); continue; }
        { const int rcw = ensure_wimg(h); if (rcw) { pop_member_failed(p, m, rcw, "dril_population_collect_rollout", first); continue; } }
        if (module_rollout_fused(h) && h->env.rollout_pop.reason.empty() && p->h_margs) mbatched.push_back(m);
        else if (rollout_fused_applies(h) && h->cfg.hidden1 == 64 && rollout_duo_applies(h->cfg.hidden1, h->env.E) && !fwd_exact(h)) batched.push_back(m);
        else if (norm_rollout_applies(h)) nbatched.push_back(m);
        else solo.push_back(m);
    }
    if (!nbatched.empty()) {                                      // collect_rollout's one-launch route, member by member around ONE launch
        const int nbat = (int)nbatched.size();
        hipError_t e = hipSuccess;
        const auto t0 = std::chrono::steady_clock::now();
        if (fps) e = hipStreamSynchronize(p->stream);
        pop_ev_begin(p, 0);
        std::vector<int> orc((size_t)nbat, DRIL_OK);
        for (int k = 0; k < nbat; ++k) {
            dril_handle* h = p->members[nbatched[k]];
            orc[k] = observe_dev(h, true);                          // new_obs = observe(env), trajectory.jl:32 (two launches per member)
            p->h_nargs[k] = norm_rollout_args(h);                   // (a member whose observe failed keeps its block: the launch is skipped below)
            if (orc[k]) e = hipErrorUnknown;
        }
        if (e == hipSuccess) e = hipMemcpyAsync(p->d_nargs, p->h_nargs, sizeof(NormRolloutArgs) * (size_t)nbat, hipMemcpyHostToDevice, p->stream);
        if (e == hipSuccess) e = launch_rollout_norm_pop(p->members[0]->cfg.env_kind, p->d_nargs, nbat, p->members[0]->env.E, p->stream);
        pop_ev_end(p);
        double f = 0;
        if (fps && e == hipSuccess) {
            e = hipStreamSynchronize(p->stream);
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            f = (double)p->members[0]->N / (dt > 0 ? dt : 1e-12);
        }
        p->info.last_rollout_launches += 1 + 2 * nbat; p->info.total_rollout_launches += 1 + 2 * nbat;
        for (int k = 0; k < nbat; ++k) {
            const int m = nbatched[k]; dril_handle* h = p->members[m];
            int rc = orc[k] ? orc[k] : e == hipSuccess ? DRIL_OK : fail(h, DRIL_ERR_HIP, std::string("rollout_norm_pop_kernel: ") + hipGetErrorString(e));
            if (!rc) { if (fps) fps[m] = f; norm_rollout_done(h); h->noise_set = false; rc = monitor_collect_rollout(h); }
            if (!rc) rc = compute_gae(h);
            if (rc) pop_member_failed(p, m, rc, "dril_population_collect_rollout", first);
        }
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
    if (!mbatched.empty()) {                                      // collect_rollout's fused plug-in route, member by member around ONE launch of member 0's kernel
        const int nbat = (int)mbatched.size();
        for (int k = 0; k < nbat; ++k) p->h_margs[k] = module_rollout_args(p->members[mbatched[k]]);   // (an injected noise table rides in the member's block)
        hipError_t e = hipMemcpyAsync(p->d_margs, p->h_margs, sizeof(DrilEnvRolloutArgs) * (size_t)nbat, hipMemcpyHostToDevice, p->stream);
        const auto t0 = std::chrono::steady_clock::now();
        if (fps && e == hipSuccess) e = hipStreamSynchronize(p->stream);
        pop_ev_begin(p, 0);
        if (e == hipSuccess) e = p->members[mbatched[0]]->env.launch_rollout_pop(p->d_margs, nbat, p->stream);
        pop_ev_end(p);
        double f = 0;
        if (fps && e == hipSuccess) {
            e = hipStreamSynchronize(p->stream);
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            f = (double)p->members[0]->N / (dt > 0 ? dt : 1e-12);
        }
        p->info.last_rollout_launches += 1; p->info.total_rollout_launches += 1;
        for (int k = 0; k < nbat; ++k) {
            const int m = mbatched[k]; dril_handle* h = p->members[m];
            int rc = e == hipSuccess ? DRIL_OK : fail(h, DRIL_ERR_HIP, std::string("dril_env_plugin_rollout_pop: ") + hipGetErrorString(e));
            if (!rc) {                                              // what collect_rollout leaves around collect_rollout_module_fused
                if (fps) fps[m] = f;
                h->gws.launches = 0; h->rollout_launches = 1 + (h->mon_cur_ret ? 1 : 0);
                rc = monitor_collect_rollout(h); h->noise_set = false;
            }
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
    std::vector<Run> batched, gbatched; std::vector<int> solo;    // one ppo_update_small_pop_kernel launch per chunk; one ppo_update_generic_small_pop_kernel launch per chunk; alone
    for (int m = 0; m < n; ++m) {
        dril_handle* h = p->members[m];
        if (p->failed[m]) continue;
        if (out) std::memset(&out[m], 0, sizeof(dril_ppo_stats));
        const UpdatePlan plan = update_plan(h);
        if (!small_persistent_applies(h, plan) && update_fused_applies(h, plan) && plan.total_steps == p->total_steps && p->h_gargs) {   // ppo_update's one-launch route of a generic handle
            GenericUpdateArgs g{};
            h->update_fused_path = 0; h->update_fused_launches = 0;
            int rc = update_begin(h, plan);
            if (!rc) rc = generic_update_args(h, plan, p->homes[m].keys, g);
            if (rc) { pop_member_failed(p, m, rc, "dril_population_ppo_update", first); continue; }
            p->h_gargs[(size_t)p->n_chunks * n + gbatched.size()] = g;                     // behind the launch table, as below
            gbatched.push_back(Run{m, plan, UpdateTry{}});
            continue;
        }
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
    // the generic members: one launch of n workgroups per chunk (no cap: the workgroups never wait for one another); a member that stopped (target_kl, a non-finite
    // gradient) idles through the later chunks on its own stop_flag.  The route is f32 throughout: no redo follows
    const int ngen = (int)gbatched.size();
    hipError_t eg = hipSuccess;
    if (ngen > 0) {
        int c = 0;
        for (int64_t s0 = 0; s0 < p->total_steps; s0 += p->chunk, ++c)
            for (int k = 0; k < ngen; ++k) {
                GenericUpdateArgs& g = p->h_gargs[(size_t)c * ngen + k];
                g = p->h_gargs[(size_t)p->n_chunks * n + k];
                small_update_chunk(gbatched[k].plan, p->chunk, s0, g.u);
            }
        const GenericDims& gd = p->members[gbatched[0].m]->gd;
        eg = prepare_ppo_update_generic_small_pop(gd, p->h_gargs, p->n_chunks * ngen);
        if (eg == hipSuccess) eg = hipMemcpyAsync(p->d_gargs, p->h_gargs, sizeof(GenericUpdateArgs) * (size_t)p->n_chunks * ngen, hipMemcpyHostToDevice, p->stream);
        pop_ev_begin(p, 1);
        for (c = 0; c < p->n_chunks && eg == hipSuccess; ++c) {
            eg = launch_ppo_update_generic_small_pop(gd, p->d_gargs + (size_t)c * ngen, ngen, p->stream);
            p->info.last_update_launches += 1; p->info.total_update_launches += 1;
        }
        pop_ev_end(p);
    }
    std::vector<char> genq((size_t)ngen, 0);
    for (int k = 0; k < ngen; ++k) {
        const int m = gbatched[k].m; dril_handle* h = p->members[m];
        int rc = eg == hipSuccess ? DRIL_OK : fail(h, DRIL_ERR_HIP, std::string("ppo_update_generic_small_pop_kernel: ") + hipGetErrorString(eg));
        if (!rc) { update_fused_done(h, gbatched[k].plan, p->n_chunks); rc = update_enqueue_home(h, gbatched[k].plan, p->homes[m]); }
        if (rc) pop_member_failed(p, m, rc, "dril_population_ppo_update", first); else genq[k] = 1;
    }
    std::vector<char> enq((size_t)nbat, 0);
    for (int k = 0; k < nbat; ++k) {
        const int m = batched[k].m; dril_handle* h = p->members[m];
        int rc = e == hipSuccess ? DRIL_OK : fail(h, DRIL_ERR_HIP, std::string("ppo_update_small_pop_kernel: ") + hipGetErrorString(e));
        if (!rc) { small_update_done(h, batched[k].plan); rc = update_enqueue_home(h, batched[k].plan, p->homes[m]); }
        if (rc) pop_member_failed(p, m, rc, "dril_population_ppo_update", first); else enq[k] = 1;
    }
    if (nbat > 0 || ngen > 0) { const int rc = pop_sync(p); if (rc) return rc; }           // ONE drain for the whole population
    for (int k = 0; k < ngen; ++k) {
        if (!genq[k]) continue;
        const int m = gbatched[k].m;
        const int rc = update_finish(p->members[m], gbatched[k].plan, p->homes[m], out ? &out[m] : nullptr);
        if (rc) pop_member_failed(p, m, rc, "dril_population_ppo_update", first);              // (its error does not stop the others)
    }
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
        if (h->env.module || !r.pl.persistent || r.pl.fused || normalizing(h) || fwd_exact(h) || h->cfg.hidden1 != 64) { solo.push_back(m); continue; }   // not evaluate_kernel<K, 64, false, true>: alone, below
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
    const bool plugin = h0->env.module != nullptr;                                     // (pop_mismatch: then every member is a handle of the same code object)
    p->chunk = plugin ? h0->update_fused_chunk : h0->small_chunk;
    for (int m = 0; m < n; ++m) { const int64_t c = plugin ? members[m]->update_fused_chunk : members[m]->small_chunk; if (c < p->chunk) p->chunk = c; }
    p->total_steps = update_plan(h0).total_steps;
    p->n_chunks = (int)((p->total_steps + p->chunk - 1) / p->chunk);
    JCHK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    JCHK(p->h_rargs.alloc((size_t)n));
    JCHK(p->h_uargs.alloc(((size_t)p->n_chunks + 1) * n));   // the launch table, and behind it one block per member
    JCHK(p->d_rargs.alloc((size_t)n));
    JCHK(p->h_nargs.alloc((size_t)n));
    JCHK(p->d_nargs.alloc((size_t)n));
    JCHK(p->d_uargs.alloc((size_t)p->n_chunks * n));
    JCHK(p->xchg.alloc((size_t)n * kSmallXchgWords));
    if (plugin) {
        JCHK(p->h_margs.alloc((size_t)n)); JCHK(p->d_margs.alloc((size_t)n));
        JCHK(p->h_gargs.alloc(((size_t)p->n_chunks + 1) * n)); JCHK(p->d_gargs.alloc((size_t)p->n_chunks * n));
    }
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
