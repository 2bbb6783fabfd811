// dril_handle.h — the PPO handle (include/dril_hip.h: dril_handle) and what the units of its host code share: the struct itself, the error and entry macros, the one-line
// predicates several units read, and the prototypes of the functions that cross a unit boundary, under the name of the unit that defines them.  The units:
//   dril_api.hip      create / destroy, the parameter, optimiser-state, env and policy verbs, dril_train, profiling and info
//   dril_rollout.hip  collect_rollout on every path, GAE, the rollout buffer's verbs
//   dril_ext.hip      the DRIL_ENV_EXTERNAL verbs on host and device arrays
//   dril_update.hip   ppo_step, the PPO update and its exact-f32 redo, dril_ppo_loss_grad / dril_apply_gradients
//   dril_eval.hip     evaluate_agent (host loop and on the device), collect_trajectory on the device, their four kernels
//   dril_pop.hip      populations: struct dril_population and the dril_population_* verbs
//   dril_comm.hip     RCCL, the loopback communicator, the all-reduce
//   dril_wrap.hip     NormalizeWrapperEnv on plug-in and external handles, the monitor's statistics
// The library is built with -fvisibility=hidden: what is declared here has external linkage inside libdril_hip.so and is not exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/dril_hip.h"
#include "dril_internal.h"
#include "dril_devmem.h"     // DevBuf / PinnedBuf: every allocation a handle or a population holds; a raw pointer member is not owned
#include "dril_norm_wrap.h"    // NormalizeWrapperEnv for any observation width: what this handle's wrapper on plug-ins shares with the SAC handle's (NormWrap, norm_moments_kernel, nz_*)
#include "dril_env_side.h"    // DeviceEnvs: the envs this handle steps on the device (a built-in kind or a device env plug-in), shared with the SAC handle

#define DRIL_EXPORT extern "C" __attribute__((visibility("default")))

namespace dril::ppo {
struct LoopGroup;   // debug loopback communicator (dril_comm.hip)

struct ProfEvent { int kid; hipEvent_t a, b; };
}  // namespace dril::ppo

struct dril_handle {
    dril_config cfg;
    int D = 0, A = 0, S = 0, P = 0, Pa = 0, Pc = 0, log_std_off = 0;
    bool discrete = true;
    dril::NetOff actor{}, critic{};
    int64_t N = 0;
    hipStream_t stream = nullptr;
    int num_cus = 256;
    std::string device_info;   // "device <ordinal> of <visible>: <name> <arch>, PCI <bus id>, HIP_VISIBLE_DEVICES=.. ROCR_VISIBLE_DEVICES=.." (dril_device_info; part of every RCCL failure message)
    dril::DevBuf<float> params, adam_m, adam_v, bt, flat, norm_out;
    dril::DevBuf<double> norm_partials; int n_norm_partials = 0;
    dril::DevBuf<float> slabs_a, slabs_c; int slab_a = 0, slab_c = 0, Gmax = 0;
    dril::DeviceEnvs env;   // the envs on the device: simulator state and counters, the seed, and for DRIL_ENV_MODULE the loaded plug-in (dril_env_side.h)
    dril::DevBuf<float> obs, rew, adv, ret, logp, val, boot, last_values;
    dril::DevBuf<char> act; dril::DevBuf<uint8_t> flags;
    dril::DevBuf<char> noise_dev; bool noise_set = false;
    dril::DevBuf<int64_t> perm_dev; size_t perm_count = 0;
    dril::DevBuf<int32_t> epoch_index; bool no_epoch_index = false;   // the device DataLoader order of the current epoch, written out (large minibatches; DRIL_NO_EPOCH_INDEX)
    dril::DevBuf<double> adv_partials, adv_stats, ev_partials; int adv_blocks = 0, ev_blocks = 0;
    dril::DevBuf<float> step_stats;
    dril::DevBuf<int> stop_flag, nan_flag;
    dril::DevBuf<float> e_obs, e_rew, e_tobs; dril::DevBuf<uint8_t> e_term, e_trunc; dril::DevBuf<char> e_act;
    uint64_t adam_steps = 0, update_counter = 0; uint32_t policy_calls = 0;
    float lr = 0;
    dril::DevBuf<unsigned long long> dbg;
    bool force_allreduce = false, force_stepwise = false;
    bool fused_rollout = false; int64_t rollout_launches = 0;   // dril_rollout_fused_enable; launch calls of the last plug-in collection (dril_rollout_fused_info)
    // dril_norm_rollout_enable: the opt-in, the launches and the path (1 = rollout_norm_kernel, 0 = step-granular) of the last normalised collection, and how often
    // an enabled handle collected step-granular because its forward was the exact-f32 one (dril_norm_rollout_info)
    bool norm_rollout = false; int norm_rollout_path = 0; int64_t norm_rollout_launches = 0, norm_rollout_fallbacks = 0;
    dril::DevBuf<double> epoch_tables, epoch_stats; int epoch_blocks = 2048;   // per-epoch advantage moments
    dril::DevBuf<float> w2a_actor, w2ta_actor, w2a_critic, w2ta_critic; bool wide = false, wimg_dirty = true;   // wide nets (H > 64)
    dril::DevBuf<char> w2pf_actor, w2pf_critic;   // wide nets: the forward stream in the k-order of a register B operand (net_forward_wide_split)
    dril::DevBuf<char> w2p_actor, w2tp_actor, w2p_critic, w2tp_critic;   // wide nets: pre-split bf16 fragment streams of W2 / W2' (ppo_grad_wide_split_kernel)
    // MonitorWrapperEnv (cfg.monitor_window > 0)
    dril::DevBuf<float> mon_cur_ret, ep_ret, mon_ring_ret, e_ep_ret; dril::DevBuf<int32_t> mon_cur_len, ep_len, mon_ring_len, e_ep_len;
    dril::DevBuf<int> mon_cnt, mon_meta; dril::DevBuf<uint8_t> e_flags;
    dril::DevBuf<float4> rec;   // packed minibatch records (see pack_records_kernel)
    dril::DevBuf<dril::RmsState> obs_rms, ret_rms; int obs_par = 0, ret_par = 0;   // ping-pong RunningMeanStd pairs
    dril::DevBuf<double> rms_partials; int rms_blocks = 256; dril::DevBuf<float> e_obs_raw; dril::DevBuf<float> e_rew_n;   // e_obs_raw / e_rew: get_original_obs / get_original_rewards; e_rew_n: rewards as the wrapper delivers them
    dril::DevBuf<double> rms_red;   // data-parallel: this step's partial sums folded to one row and summed over ranks
    int grad_actor_pct = 0;   // ppo_grad_pair_kernel: share (per mille) of the pairs given to the actor; 0 = by head (env DRIL_GRAD_ACTOR_PERMILLE)
    int last_G = 0, last_Gc = 0; mutable char grad_info[640] = {0};   // the grid of that step (slabs of the actor / of the critic; ppo_grad_pair_kernel: pairs) and the text dril_grad_kernel_info returns
    int last_variant = -1;  // which gradient kernel the last optimiser step ran: 0 ppo_grad_kernel, 2 ppo_grad_wide_kernel, 3 generic path, 4 ppo_grad_wide_split_kernel, 5 ppo_grad_pair_kernel, 6 ppo_update_small_kernel, 7 ppo_update_generic_small_kernel (dril_grad_kernel_info)
    int grad_variant = -1;  // env DRIL_GRAD_VARIANT: 0 = the exact-f32 kernels (ppo_grad_kernel / ppo_grad_wide_kernel), 1 = the bf16-split kernels (ppo_grad_pair_kernel at hidden 64, ppo_grad_wide_split_kernel at 128 / 256) for every minibatch size, -1 = default: wide nets split, hidden 64 by minibatch size
    bool external = false; bool generic = false; dril::DevBuf<float> gen_tmp;   // generic: layer-by-layer kernels (host envs, or a device env whose hidden_dims the fused kernels are not built for)
    dril::GenericDims gd{}; dril::GenericWs gws; int ext_t = 0; bool ext_acted = false;   // DRIL_ENV_EXTERNAL: host envs, generic kernels
    dril::PinnedBuf<float> ext_stage_rew; dril::PinnedBuf<uint8_t> ext_stage_flags;   // pinned [T][E] staging: dril_ext_record returns without draining the stream
    // the device-array verbs (dril_ext_*_device): the two ordering events (created once), the sticky error word and its pinned host copy, the ClampAdapter's
    // per-dimension table (dril_ext_set_action_bounds), the counters of dril_ext_device_info, grow-only scratch of dril_predict_actions_device
    hipEvent_t ext_ev_in = nullptr, ext_ev_out = nullptr; dril::DevBuf<int> ext_err; dril::PinnedBuf<int> ext_err_host;
    dril::ExtBounds ext_bounds{}; bool ext_bounds_set = false;
    int ext_steps_dev = 0, ext_steps_host = 0, ext_syncs = 0; int64_t ext_launches = 0;
    dril::DevBuf<char> ext_pred_act; dril::DevBuf<float> ext_pred_lp;
    // NormalizeWrapperEnv around a plug-in env (dril_normalize_enable; kernels: dril_norm_wrap.h, dril_ppo_norm.h).  pn_red: the one row a data-parallel job all-reduces.
    // The wrapper's other arrays are the handle's own: disc_returns (`returns`), e_obs_raw / e_rew (old_obs / old_rewards: dril_normalize_get_original), e_rew_n (the
    // rewards dril_env_step delivers)
    NormWrap pn; int pn_rows_cap = 0; dril::DevBuf<double> pn_red;
    // the same wrapper and MonitorWrapperEnv around the envs of a DRIL_ENV_EXTERNAL handle (dril_ext_normalize_enable / dril_ext_monitor_enable; kernels: dril_ext_norm.h): pn
    // again, with e_tobs as the scratch of normalised terminal observations; ext_mon_window sizes the monitor arrays above (cfg.monitor_window stays 0).  xw_added: launches
    // the wrappers added to the act / record / finish calls of the current rollout; xw_allocs: allocations inside those calls since enable (dril_ext_wrap_info)
    int ext_mon_window = 0; int64_t xw_added[3] = {0, 0, 0}, xw_allocs = 0; dril::DevBuf<float> ext_pred_obs;
    void* comm = nullptr;
    dril::ppo::LoopGroup* loop = nullptr;   // debug loopback communicator (dril_debug_comm_loopback)
    dril_population* pop = nullptr;   // the population the handle is a member of (dril_population_join): dril_destroy waits for dril_population_destroy
    int64_t allreduce_calls = 0;
    dril::DevBuf<float> retry_snap; bool no_f32_retry = false; int64_t f32_retries = 0;   // ppo_update: state before the update (for the exact-f32 redo of an update that left f16's range); DRIL_NO_F32_RETRY; how often it happened
    // the redo's bookkeeping (dril_f32_fallback_info): used_f16 = an f16-piece kernel ran in the current update (sticky over its optimiser steps — the LAST step's kernel says nothing
    // about a ragged tail); streak = consecutive redone updates; after kRetryLatchAfter of them the next kRetryLatchUpdates updates run the exact-f32 kernels directly (no wasted f16
    // pass, no snapshot), then ONE update probes f16 again; direct = updates run that way (latched, or max |W2| out of f16's range)
    bool used_f16 = false, spin_timeout = false; int f32_streak = 0, f32_latch_left = 0; int64_t f32_direct_updates = 0, persistent_fallbacks = 0;
    dril::DevBuf<unsigned long long> gae_carry; unsigned gae_tag = 0; dril::DevBuf<int> gae_err;   // gae_scan_kernel: the chunk-to-chunk carry words, the launch tag that validates them, its give-up flag
    dril::DevBuf<unsigned> w2max_dev; float w2max = 0.f;   // max |W2| over both nets (fused kernels): host copy refreshed by dril_set_params and with every optimiser run's statistics
    bool no_small_path = false;   // DRIL_NO_SMALL_PATH (with DRIL_DEBUG=1), latched in dril_create
    bool no_persistent = false; dril::DevBuf<unsigned long long> small_xchg; dril::DevBuf<uint64_t> epoch_keys; int64_t small_chunk = 16384;   // ppo_update_small_kernel (batch_size <= 64): DRIL_NO_PERSISTENT_UPDATE; per-epoch DataLoader keys on the device
    // dril_update_fused_enable: the opt-in of a generic handle, the path (1 = ppo_update_generic_small_kernel, 0 = per step) and the kernel launches of the last update,
    // the optimiser steps per launch (kGuChunk; DRIL_SMALL_CHUNK with DRIL_DEBUG=1)
    bool update_fused = false; int update_fused_path = 0; int64_t update_fused_launches = 0, update_fused_chunk = dril::kGuChunk;
    int64_t last_update_steps = 0;   // epochs x minibatches of the last update: the rows of step_stats that are its own (dril_debug_get_step_stats)
    std::vector<dril::ppo::ProfEvent> prof_pending; std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pool;
    double prof_ms[DRIL_K_COUNT] = {0}; int64_t prof_n[DRIL_K_COUNT] = {0}, prof_all[DRIL_K_COUNT] = {0}; bool prof_open = false;
    // dril_evaluate_agent_device: where the env side is set aside for the call, the per-env running sums, the event list and its counter (pinned host word for the poll)
    dril::DevBuf<char> eval_snap; dril::DevBuf<float> eval_cur_ret; dril::DevBuf<int32_t> eval_cur_len;
    dril::DevBuf<unsigned int> eval_counter; dril::PinnedBuf<unsigned int> eval_counter_host; dril::DevBuf<dril::SacEvalEvent> eval_events;
    // dril_collect_trajectory_device: ONE grow-only blob for the step-major recording, the shadow envs' arrays and the table of bounds (the counter and its pinned word are the evaluation's)
    dril::DevBuf<char> traj_blob;
    // path 2 of both verbs (a plug-in's fused evaluation kernel): ONE grow-only blob for the observation and action scratch, the K rows of rewards and flag bytes and,
    // when recording, the rows of raw actions and post-step observations
    dril::DevBuf<char> evalf_blob;
    std::string err;
};

namespace dril::ppo {
extern thread_local std::string g_create_error;   // what dril_last_error(NULL) reports (dril_api.hip)
inline int fail(dril_handle* h, int code, const std::string& msg) { if (h) h->err = msg; else g_create_error = msg; return code; }
#define HIPCHK(h, expr)                                                                                      \
    do { hipError_t _e = (expr); if (_e != hipSuccess)                                                       \
        return fail(h, DRIL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)
// every entry point makes the handle's device current first: a process may hold handles on several devices
#define NEED(h) do { if (!(h)) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle"); (void)hipSetDevice((h)->cfg.device); } while (0)
#define NOT_EXTERNAL(h, what) do { if ((h)->external) return fail(h, DRIL_ERR_UNSUPPORTED, what ": the envs of DRIL_ENV_EXTERNAL live on the host (use dril_ext_act / dril_ext_record / dril_ext_finish)"); } while (0)
#define NOT_MODULE(h, what) do { if ((h)->env.module) return fail(h, DRIL_ERR_UNSUPPORTED, what ": NormalizeWrapperEnv is off on this device env plug-in handle (DRIL_ENV_MODULE): switch it on with dril_normalize_enable, then this verb forwards to dril_normalize_*"); } while (0)

inline bool comm_ready(const dril_handle* h) { return h->comm != nullptr || h->loop != nullptr; }
constexpr int kNcclFloat32 = 7, kNcclFloat64 = 8;   // the dtype argument of rccl_allreduce
inline bool normalizing(const dril_handle* h) { return h->cfg.norm_obs || h->cfg.norm_reward; }
inline size_t act_bytes_per(const dril_handle* h) { return h->discrete ? 4 : 4 * (size_t)h->A; }
// wide nets: 1 = ppo_grad_wide_split_kernel (bf16 matrix cores), 0 = the f32-MFMA ppo_grad_wide_kernel (DRIL_GRAD_VARIANT; records are needed by the split form)
// default by measurement (profiles/r02_wide_split.md): the split form for both wide widths (hidden 256: 176-183 vs 118 TFLOP/s; hidden 128: 151 vs 113.5)
inline int wide_variant(const dril_handle* h) { return (h->wide && h->rec && (h->grad_variant < 0 ? 1 : h->grad_variant)) ? 1 : 0; }
// hidden [64,64]: may ppo_grad_pair_kernel run at all (it reads packed records; DRIL_GRAD_VARIANT=0 pins the exact-f32 kernel)
// minibatches of at least this many 32-sample tiles per CU run ppo_grad_pair_kernel (measured on the f16 arithmetic, 256 CUs: 65 536 samples 50.7 us against 64.8 us on the
// exact-f32 kernel, 16 384 samples 42.2 against 39.0; with the bf16 x 3 arithmetic of rounds 2 - 3 the crossover was at 16 tiles per CU)
constexpr int kPairTilesPerCu = 8;
inline bool pair_variant(const dril_handle* h) { return !h->wide && !h->generic && h->cfg.hidden1 == 64 && h->grad_variant != 0 && h->rec && h->D <= 8; }   // (D > 4, Acrobot: dW1 / db1 through a third piece image on the matrix cores — 16 (D + 1) per-lane accumulators would not fit)
// the forward of the fused rollout / policy kernels: f16 two-piece W2 while every W2 entry is inside f16's range, else (or with DRIL_GRAD_VARIANT=0: "exact f32 everywhere") the f32-MFMA instantiations
inline bool fwd_exact(const dril_handle* h) { return h->grad_variant == 0 || h->cfg.hidden1 == 32 || !(h->w2max < kFwdSplitMaxW); }   // (hidden 32 has no f16-piece instantiation)
constexpr int kRetryLatchAfter = 2, kRetryLatchUpdates = 16;

// ---- dril_api.hip ----
// HIP-event brackets of the kernel classes (cfg.profile_events)
void prof_begin(dril_handle* h, int kid);
void prof_end(dril_handle* h);
void prof_resolve(dril_handle* h);   // stream must be drained
int sync(dril_handle* h);
// wide nets: (re)build the pre-tiled W2 / W2' images after every parameter change (enqueued on the handle's stream)
int ensure_wimg(dril_handle* h);
// fused per-kind kernels for the device envs, the layer-by-layer generic path for DRIL_ENV_EXTERNAL
hipError_t run_policy(dril_handle* h, const PolicyArgs& a);
PolicyArgs policy_args(dril_handle* h, const float* obs, int64_t B, const void* noise, void* actions, float* values, float* logp, float* entropy, int mode);
MonitorArgs monitor_rollout_args(dril_handle* h, size_t k);   // row k / E of a step-granular rollout over a plug-in: the BUF_FLAGS byte always, finished episodes with the monitor on
int monitor_collect_rollout(dril_handle* h);
// act!(env, actions) through the E-sized per-step arrays (dril_env_step, dril_evaluate_agent, the step-granular verbs), and MonitorWrapperEnv's window after it
int env_step_arrays(dril_handle* h, const void* actions);
// data-parallel runs: this rank's partial table of NormalizeWrapperEnv's batch moments folded to one row and summed over the ranks
int global_partials(dril_handle* h, bool update, const double*& partials, int& nb, long long& n_stats);
// the step-granular env verbs on device (NormalizeWrapperEnv.observe / act!).  actions: device pointer; rew_out / flags_out: device destinations
int observe_dev(dril_handle* h, bool update_stats);
int step_dev(dril_handle* h, const void* actions, float* rew_out, uint8_t* flags_out);

// ---- dril_rollout.hip ----
int compute_gae(dril_handle* h);
// "" when the handle's net fits the plug-in's fused evaluation kernel (path 2 of the evaluation / trajectory verbs), else why not
std::string fused_evaluate_unavailable(const dril_handle* h);
// a collection that is ONE launch of the fused rollout kernel of a built-in kind, and the argument block of that launch, read from the handle as it stands
bool rollout_fused_applies(const dril_handle* h);
RolloutArgs rollout_args(const dril_handle* h);
// the one-launch collection of a normalising built-in handle (dril_norm_rollout_enable): "" when the handle may take it, else why not; whether this collection takes
// it (enabled, available, on the f16-piece forward); its argument block, read from the handle AFTER the opening observe; the host's bookkeeping after the launch
std::string norm_rollout_unavailable(const dril_handle* h);
bool norm_rollout_applies(const dril_handle* h);
NormRolloutArgs norm_rollout_args(const dril_handle* h);
void norm_rollout_done(dril_handle* h);
// a plug-in's fused collection (dril_rollout_fused_enable): "" when the handle's net fits the plug-in's kernel, else why not; the argument block of its ONE launch, read
// from the handle as it stands (collect_rollout, and a population for each of its members)
std::string fused_rollout_unavailable(const dril_handle* h);
DrilEnvRolloutArgs module_rollout_args(const dril_handle* h);
int collect_rollout(dril_handle* h, double* fps, bool do_sync);

// ---- dril_ext.hip ----
// the handle's stream takes over from the caller's stream / hands back to it: two events per handle, no host wait
int ext_stream_enter(dril_handle* h, void* caller_stream);
int ext_stream_leave(dril_handle* h, void* caller_stream);

// ---- dril_update.hip ----
// One update in the pieces that ppo_update runs in order, and that a population runs member by member around ONE batched launch (the order: dril_update.hip)
struct UpdatePlan { int world = 1; int64_t N = 0, B = 0, nb = 0, total_steps = 0; uint64_t adam_steps0 = 0; int bits = 0; };
// where an update's results land on the host: st [total_steps][16], ev [4 ev_blocks], scal = {nan flag, gae give-up flag, max |W2| bits}, keys [epochs].  Storage is the
// caller's and must not move before update_finish: vectors for a solo update, one pinned block per member in a population
struct UpdateHome { float* st = nullptr; double* ev = nullptr; int* scal = nullptr; uint64_t* keys = nullptr; };
struct UpdateTry { bool may_retry = false; uint64_t adam_steps0 = 0, counter0 = 0; };
UpdatePlan update_plan(const dril_handle* h);
bool small_persistent_applies(const dril_handle* h, const UpdatePlan& p);
int update_begin(dril_handle* h, const UpdatePlan& p);
int small_update_args(dril_handle* h, const UpdatePlan& p, uint64_t* keys, SmallUpdateArgs& u);
void small_update_chunk(const UpdatePlan& p, int64_t chunk, int64_t s0, SmallUpdateArgs& u);
void small_update_done(dril_handle* h, const UpdatePlan& p);
// the one-launch update of a generic handle (dril_update_fused_enable): "" when the handle may take it, else why not and what to do; whether this update takes it;
// what its launches leave on the host side of the handle
std::string update_fused_unavailable(const dril_handle* h);
bool update_fused_applies(const dril_handle* h, const UpdatePlan& p);
void update_fused_done(dril_handle* h, const UpdatePlan& p, int64_t launches);
// that update's argument block but for the launch's own words (small_update_chunk per launch; the launcher fills the LDS plan): small_update_args and the rollout
// buffer's arrays.  keys as in small_update_args
int generic_update_args(dril_handle* h, const UpdatePlan& p, uint64_t* keys, GenericUpdateArgs& g);
int update_enqueue_home(dril_handle* h, const UpdatePlan& p, const UpdateHome& home);
int update_finish(dril_handle* h, const UpdatePlan& p, const UpdateHome& home, dril_ppo_stats* out);
bool update_direct_f32(const dril_handle* h);
int update_snapshot(dril_handle* h, UpdateTry& t);
int update_resolve(dril_handle* h, const UpdateTry& t, int rc, dril_ppo_stats* out);
int ppo_update(dril_handle* h, dril_ppo_stats* out);

// ---- dril_eval.hip ----
// what one evaluation sets aside: device arrays in a list (copied to / from one blob), the host-side words next to them
struct EvalKeep {
    std::vector<std::pair<void*, size_t>> arrays;
    uint64_t seed0; bool ready; int obs_par, ret_par, norm_training, pn_training; DevBuf<float> mon_cur_ret; int64_t gws_launches;
};
struct EvalPlan { bool persistent, fused, raw; int K; long long cap; EvalKeep keep; };
// the pieces of dril_evaluate_agent_device, in the order it runs them: prepare, set-aside, reset, enqueue, put-back, reduce
int eval_prepare(dril_handle* h, const dril_eval_options* o, EvalPlan& pl);
int eval_set_aside(dril_handle* h, EvalKeep& keep);
int eval_reset(dril_handle* h, const dril_eval_options* o, unsigned int* counter, long long cap, EvalAcct& acct);
long long eval_max_steps(const dril_handle* h, int n_eval, int K);
void eval_persistent_args(const dril_handle* h, const dril_eval_options* o, int K, const EvalAcct& acct, EvalKernelArgs& g);
int eval_put_back(dril_handle* h, EvalKeep& keep);
void eval_reduce(SacEvalEvent* events, int64_t n_events, const dril_eval_options* o, dril_eval_stats* out, float* ep_rewards, int32_t* ep_lengths);

// ---- dril_comm.hip ----
int rccl_allreduce(dril_handle* h, void* buf, size_t count, int dtype);
// dril_destroy's part of the communicator: the RCCL communicator destroyed, the loopback group left
void comm_release(dril_handle* h);

// ---- dril_wrap.hip ----
// observe(env) of the wrapper (:123-137): the plug-in's observe kernel into e_obs_raw, then moments + apply into e_obs
int pn_observe(dril_handle* h, bool update_stats);
// act!(env, actions) of the wrapper (:139-165) through the E-sized per-step arrays: raw rewards stay in e_rew, the delivered ones go to rew_out
int pn_step(dril_handle* h, const void* actions, float* rew_out);
// collect_rollout_module's loop under dril_normalize_enable
int collect_rollout_module_norm(dril_handle* h);
// observe (:123-137) of B rows of the caller's array into obs_out; *added: the launches enqueued
int xn_observe(dril_handle* h, const float* raw, int64_t B, float* obs_out, bool rollout, int64_t* added);
// act! (:139-165) with the record's own work and the monitor's sums, row k / E of the buffer.  tobs_norm: where the critic must read the terminal observations
int xn_record(dril_handle* h, size_t k, const float* d_rewards, const uint8_t* d_terminated, const uint8_t* d_truncated, const float* d_terminal_obs, const float** tobs_norm, int64_t* launches);
}  // namespace dril::ppo
