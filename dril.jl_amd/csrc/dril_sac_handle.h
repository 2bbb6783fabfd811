// dril_sac_handle.h — the SAC handle (include/dril_sac.h: dril_sac_handle) and what the units of its host code share: the struct itself, the types of its members, the
// error and entry macros, and the prototypes of the functions that cross a unit boundary, under the name
// of the unit that defines them.  The units:
//   dril_sac.hip          create / destroy, the parameter, env and prediction verbs, the replay ring, dril_sac_train / dril_sac_iterate, profiling
//   dril_sac_net.hip      the contractions of one net (net_forward, net_backward, actor_hidden) and the two kernels of the collection forward
//   dril_sac_update.hip   one gradient step (sac_one_update) with its kernels, the statistics rows, dril_sac_update and its debug verbs
//   dril_sac_collect.hip  the collection: the head, push and env-step kernels, one collected step, dril_sac_collect_rollout / _continue
//   dril_sac_wrap.hip     MonitorWrapperEnv / NormalizeWrapperEnv around the handle's device envs: dril_sac_monitor_*, dril_sac_normalize_*
//   dril_sac_ext.hip      the DRIL_ENV_EXTERNAL verbs on host and device arrays, and the two wrappers around such a handle's envs
//   dril_sac_eval.hip     evaluate_agent and collect_trajectory on the device
// A kernel is defined in the unit that launches it; what kernels of several units share is dril_sac_device.h.
// The library is built with -fvisibility=hidden: what is declared here has external linkage inside libdril_hip.so and is not exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/dril_sac.h"
#include "dril_internal.h"
#include "dril_devmem.h"       // DevBuf / PinnedBuf: every allocation the handle holds; a raw pointer member is not owned
#include "dril_gemm.h"         // GemmArgs
#include "dril_sac_eval.h"     // SacEvalEvent
#include "dril_env_side.h"     // DeviceEnvs: the envs this handle steps on the device (a built-in Box kind or a device env plug-in), shared with the PPO handle
#include "dril_norm_wrap.h"    // NormalizeWrapperEnv for any observation width: what this handle's wrapper shares with the PPO handle's on plug-ins (NormWrap, norm_moments_kernel, nz_*)
#include "dril_sac_device.h"   // CollectHeadArgs, PushArgs, CollectEnvArgs: argument blocks the units hand to each other
#include "dril_sac_norm.h"     // NzApplyArgs

#define DRIL_EXPORT extern "C" __attribute__((visibility("default")))

namespace dril::sac {
// device scalars shared by the kernels of one gradient step
struct SacScalars { float log_ent, ent_m, ent_v, alpha; };
}  // namespace dril::sac

// =================================================================================================================
// handle
// =================================================================================================================
struct dril_sac_handle {
    dril_sac_config cfg;
    int D = 0, A = 0, S = 0, H1 = 0, H2 = 0, nmax = 0;
    int P = 0, Pa = 0, Pq = 0;                       // host (ABI) layout: actor | q1 | q2 | log_std
    int Pd = 0, Pqd = 0, log_std_off = 0;            // DEVICE layout: every net starts on a 16-byte boundary (float4 operand loads); pads stay zero
    dril::NetOff actor{}, q0{};                            // device offsets
    hipStream_t stream = nullptr;
    dril::DevBuf<float> params, adam_m, adam_v, g_critic, g_actor;
    float* target = nullptr;                         // alias: the target critics inside params
    dril::DevBuf<dril::sac::SacScalars> sc; dril::DevBuf<float> stats; dril::DevBuf<float> stats_out;
    dril::DevBuf<double> ssq_rows;   // [updates stats_out holds][adam_blocks_c + end_blocks] squared-gradient partials per update, summed on the host (grad_norm statistic)
    dril::DevBuf<unsigned int> counter; int adam_blocks_c = 0, end_blocks = 0;
    dril::DevBuf<dril::sac::SacScalars> sc_next;   // ping-pong partner of `sc` (fused heads: the entropy step writes the new state here, then the two are swapped)
    dril::DevBuf<double> head_partials; dril::DevBuf<unsigned int> head_counter; dril::DevBuf<unsigned> col_h1p; dril::DevBuf<unsigned> col_w2p; dril::DevBuf<int> col_flags; int col_tag = 0, col_w2tag = 0; bool col_w2_dirty = true, f16_fwd = true, l2_attr_set = false;   // the f16-piece collection forward (sac_collect_l2_kernel)
    dril::DevBuf<unsigned long long> it_stamps; double wall_hz = 1e8; bool fused_heads = true; bool fused_dw1 = false; int fl_c = 0, fl_a = 0; bool fused_collect = true; bool fused_fwd = true; bool trace_enqueue = false; std::vector<hipEvent_t> it_events; int iter_chunk = 64;   // fused output-layer + head kernels (DRIL_SAC_NO_FUSED_HEADS=1: the round-1 launch sequence, A/B)
    int upd_route[3] = {-1, 0, 0}; mutable char upd_info[160] = {0};   // what the last sac_one_update enqueued: {first layers in the gather, PRE head, launched yet} (dril_sac_update_info)
    float bt_actor[2], bt_critic[2], bt_ent[2]; int64_t grad_updates = 0; uint64_t update_counter = 0, aux_counter = 0;
    float target_entropy = 0, act_lo = -2.0f, act_hi = 2.0f; bool external = false;   // bounds of the agent-facing action space: Box(-2,2), Box(-1,1) under ScalingWrapperEnv
    dril::DevBuf<float> act_bounds;                     // device table [low[kMaxA] | high[kMaxA]] the sampling kernels read: the pair above in every entry, or a plug-in's bounds per dimension
    // env: the envs on the device — simulator state and counters, the seed, and for DRIL_ENV_MODULE the loaded plug-in (dril_env_side.h; SAC has no DiscreteAdapter and
    // no fixed-length episodes: action_start 0, fixed_len 0)
    dril::DeviceEnvs env; bool fused_head_push = true;
    dril::DevBuf<float> obs_cur, obs_nxt, e_rew, e_tobs, e_raw, e_envact; dril::DevBuf<uint8_t> e_term, e_trunc;
    bool obs_valid = false;
    // replay ring
    long long cap = 0, size = 0, head = 0;
    dril::DevBuf<float> rb_obs, rb_next, rb_act, rb_rew; dril::DevBuf<uint8_t> rb_term, rb_trunc;
    // batch + activations
    dril::DevBuf<float> xa, ah1, ah2, mu;               // actor: [nmax][D], [nmax][H], [nmax][A]
    dril::DevBuf<float> xq, xq_pi; float* xq_next = nullptr;                 // [B][D+A]; xq_next: alias (second half of xq)
    dril::DevBuf<float> qh1, qh2; float *th1 = nullptr, *th2 = nullptr;      // [2][nq][H]; th1 / th2: aliases (z = 2,3 of qh1 / qh2)
    dril::DevBuf<float> q_cur, q_pi, dq; float* q_next = nullptr; // [2][nq]; q_next: alias (second half of q_cur)
    dril::DevBuf<float> dz2, dz1, dxq, dmu;            // [2][nq][H], [2][nq][D+A], [B][A]
    dril::DevBuf<float> b_rew, b_ne, b_nn, b_np, b_nlp, a_pi, g_pi, lp_pi; dril::DevBuf<uint8_t> b_term;
    int nq = 0;
    // MonitorWrapperEnv (dril_sac_monitor_enable; mon_window == 0: off, every pointer null): running sums per env, the ring of the last mon_window finished episodes
    // with meta = {count, head}, and the finished-episode block [mon_rows_cap][E] of the collection in flight (mon_row: its next row)
    int mon_window = 0, mon_rows_cap = 0, mon_row = 0; dril::DevBuf<float> mon_cur_ret, mon_ring_ret, mon_ep_ret; dril::DevBuf<int32_t> mon_cur_len, mon_ring_len, mon_ep_len;
    dril::DevBuf<int> mon_meta; dril::DevBuf<uint8_t> mon_flags;
    // evaluate_agent (dril_sac_evaluate_agent): the env-side snapshot, the per-env running sums, the event list and its counter (pinned host word for the poll)
    int eval_poll = 0; dril::DevBuf<float> ev_state, ev_obs, ev_mon_ret, ev_cur_ret; dril::DevBuf<int32_t> ev_sc, ev_mon_len, ev_cur_len; dril::DevBuf<uint32_t> ev_ep, ev_gs;
    dril::DevBuf<unsigned int> ev_counter; dril::PinnedBuf<unsigned int> ev_counter_host; dril::DevBuf<dril::SacEvalEvent> ev_events;
    // dril_sac_collect_trajectory: ONE grow-only blob for the step-major recording, the shadow envs' arrays (plug-ins) and the table of bounds (the counter and its pinned word are the evaluation's)
    dril::DevBuf<char> traj_blob;
    // NormalizeWrapperEnv (dril_sac_normalize_enable; nz.on false: every pointer null; kernels: dril_norm_wrap.h, dril_sac_norm.h).  nz_old_obs (E x D) is the raw
    // observation of the envs' present state once nz_raw_valid
    NormWrap nz; bool nz_raw_valid = false;
    dril::DevBuf<float> nz_returns, nz_old_obs, nz_old_rew;
    // device-array verbs of an external handle (dril_sac_ext_*_device, dril_sac_update_enqueue, dril_sac_flush): the two hand-over events, the sticky error word and
    // its pinned host copy, the pending statistics table (DRIL_SAC_PENDING_CAPACITY rows, allocated at create) + its squared-gradient partials, what a flush has to free, and the counters of the info struct
    hipEvent_t ext_ev_in = nullptr, ext_ev_out = nullptr; dril::DevBuf<int> ext_err; dril::PinnedBuf<int> ext_err_host;
    bool ext_acted = false, ext_bounds_set = false, in_device_verb = false;
    int64_t fwd_launches = 0;                        // kernels enqueued through gemm / gemm_pair / the elementwise first layer since create: what `launches` of the info struct is counted from
    dril::DevBuf<float> pend_stats; dril::DevBuf<double> pend_ssq; int pend_n = 0; struct InjectedBatches { dril::DevBuf<long long> idx; dril::DevBuf<float> ne, nn, np; }; std::vector<InjectedBatches> pend_free;
    int64_t ext_steps_dev = 0, ext_steps_host = 0, ext_syncs = 0, ext_flushes = 0, ext_launches = 0;
    // NormalizeWrapperEnv / MonitorWrapperEnv on an external handle (dril_sac_ext_normalize_enable / dril_sac_ext_monitor_enable) live in nz / nz_* / mon_* above, which
    // the built-in verbs never touch on such a handle.  xw_begin: the next act opens a collection (dril_sac_ext_collection_begin); xw_live: one is in progress (cleared
    // by enable / set_stats / normalize_reset); the counters of dril_sac_ext_wrap_info
    bool xw_begin = false, xw_live = false; int64_t xw_launches_act = 0, xw_launches_push = 0;
    // cfg.profile_events on an external handle: HIP events around what act_device and push_device enqueue (a pair per call, recorded and never waited for); dril_sac_flush
    // reads them after its drain into collect_ms / collect_steps (dril_sac_profile_get).  The pool is created at create (kXpPool events: nothing is created inside the
    // sync-free verbs) and re-used after every flush; calls made while it is full are not timed
    std::vector<hipEvent_t> xp_events; size_t xp_n = 0, xp_pairs = 0;
    // injected inputs (tests)
    dril::DevBuf<float> collect_noise; size_t collect_noise_count = 0;
    int inj_updates = 0; dril::DevBuf<long long> inj_idx; dril::DevBuf<float> inj_ne, inj_nn, inj_np;
    // host-batch scratch
    dril::DevBuf<float> s_in, s_act, s_noise, s_out, s_out2;
    // timing
    hipEvent_t ev_a = nullptr, ev_b = nullptr; double collect_ms = 0, update_ms = 0; int64_t collect_steps = 0, updates = 0;
    std::string err;
};

namespace dril::sac {
int sfail(dril_sac_handle* h, int code, const std::string& msg);   // h == null: what dril_sac_last_error(NULL) reports (dril_sac.hip)
#define SHIP(h, expr)                                                                                        \
    do { hipError_t _e = (expr); if (_e != hipSuccess)                                                       \
        return sfail(h, DRIL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)
#define SNEED(h) do { if (!(h)) return sfail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle"); (void)hipSetDevice((h)->cfg.device); } while (0)
#define SDO(expr) do { int _rc = (expr); if (_rc != DRIL_OK) return _rc; } while (0)
#define S_NOT_EXTERNAL(h, what) do { if ((h)->external) return sfail(h, DRIL_ERR_UNSUPPORTED, what ": the envs of DRIL_ENV_EXTERNAL live on the host (dril_sac_predict_actions + dril_sac_ext_push)"); } while (0)

inline int round4(int x) { return (x + 3) & ~3; }
// One net = {W1 b1 W2 b2 W3 b3} at `P + off` (+ z * zP for the second critic); activations are (features x n) column-major
struct NetBufs { float* h1; float* h2; float* out; long long zh, zo, zh2; };   // [Z][n][H1], [Z][n][O], [Z][n][H2]: batch strides of h1 / out / h2 (zh2 == 0: H1 == H2 shapes, use zh)
inline NetBufs actor_bufs(dril_sac_handle* h) { return NetBufs{h->ah1, h->ah2, h->mu, 0, 0, 0}; }
inline NetBufs q_bufs(dril_sac_handle* h, float* h1, float* h2, float* out) { return NetBufs{h1, h2, out, (long long)h->nq * h->H1, (long long)h->nq, (long long)h->nq * h->H2}; }

// ---- dril_sac.hip ----
int ssync(dril_sac_handle* h);   // drains the handle's stream; inside a sync-free device verb the wait is counted

// ---- dril_sac_net.hip ----
int gemm(dril_sac_handle* h, GemmArgs g, int Z);
int net_forward(dril_sac_handle* h, const float* P, NetOff off, long long zP, int in, int O, const float* X, int ldx, long long zX, int n,
                NetBufs b, int Z, int zdivX = 1, bool hidden_only = false, bool first_done = false);
int net_backward(dril_sac_handle* h, const float* P, NetOff off, long long zP, int in, int O, const float* X, int ldx, long long zX, int n,
                 NetBufs b, const float* dOut, float* G, float* dX, int Z, bool have_dz2 = false, bool skip_w1 = false);
// predict_actions_raw up to the output layer for the envs' current observations; *out: the argument block of the head that follows
int actor_hidden(dril_sac_handle* h, int use_random, const float* inj_noise, CollectHeadArgs* out);

// ---- dril_sac_update.hip ----
// one update!(agent, alg, batch), enqueued.  `slot`: index into the injected batches (-1: Philox); `out`: device statistics row; ssq_row_in: a row of the pending table
int sac_one_update(dril_sac_handle* h, int slot, float* out, unsigned long long* stamp = nullptr, double* ssq_row_in = nullptr);
// room for the statistics rows of n gradient steps in the table of dril_sac_update
int ensure_stats(dril_sac_handle* h, int n);
// the statistics rows of the last n gradient steps, stream drained (rows_dev / ssq_dev: the pending table of dril_sac_update_enqueue; null: the table of dril_sac_update)
int fetch_stats(dril_sac_handle* h, int n, dril_sac_stats* out, const float* rows_dev = nullptr, const double* ssq_dev = nullptr);
// n gradient steps enqueued back to back, one drain, their statistics (out: null = none); injected: step k takes batch k of dril_sac_debug_set_batches
int run_updates(dril_sac_handle* h, int n_updates, bool injected, dril_sac_stats* out);

// ---- dril_sac_collect.hip ----
int ensure_obs(dril_sac_handle* h);
void ring_advance(dril_sac_handle* h);
CollectEnvArgs env_kernel_args(dril_sac_handle* h, const CollectHeadArgs& ca, const PushArgs& pa, const MonitorArgs& mon);
// the launches another unit enqueues: the action head of all envs, the ring write of one env step, and the one launch of an evaluation / a trajectory step over a
// built-in Box kind (sac_eval_env_kernel / sac_traj_env_kernel are compiled with sac_collect_env_kernel)
void launch_collect_head(dril_sac_handle* h, const CollectHeadArgs& ca);
void launch_push(dril_sac_handle* h, const PushArgs& pa);
struct EvalEnvArgs { CollectEnvArgs env; EvalAcctArgs acct; NzEvalArgs nz; };
struct TrajEnvArgs { CollectEnvArgs env; NzEvalArgs nz; TrajRec rec; TrajMaps maps; int32_t t; };
hipError_t launch_eval_env(dril_sac_handle* h, const EvalEnvArgs& a);
hipError_t launch_traj_env(dril_sac_handle* h, const TrajEnvArgs& a);
// one step of collect_trajectories for all envs, enqueued (the caller has called collect_prepare); `first` / `last`: the step's place in its collection
int collect_step(dril_sac_handle* h, int use_random, const float* inj_noise, unsigned long long* stamp = nullptr, bool first = true, bool last = true);
// before the steps of a collection: the observation of the envs' present state (the raw one under NormalizeWrapperEnv) and MonitorWrapperEnv's block of n_steps rows
int collect_prepare(dril_sac_handle* h, int n_steps);
// a whole collection of n_steps, drained; cont: it continues the collection the previous call began (dril_sac_collect_continue)
int collect(dril_sac_handle* h, int n_steps, int use_random, double* fps, bool cont = false);

// ---- dril_sac_wrap.hip ----
// MonitorWrapperEnv: its arrays, the block of a collection's rows, the row of the step being enqueued, the window launch after a collection's last step, log_stats over the window
void monitor_free(dril_sac_handle* h);
hipError_t monitor_alloc(dril_sac_handle* h, int32_t window, size_t rows);
int monitor_begin(dril_sac_handle* h, int n_steps);
MonitorArgs monitor_row(dril_sac_handle* h);
int monitor_end(dril_sac_handle* h);
int monitor_read(dril_sac_handle* h, float* ep_rew_mean, float* ep_len_mean, int32_t* n_episodes);
// NormalizeWrapperEnv: its arrays, the raw observation of the envs' present state, the moments and apply launches, observe(env) into `out` and at the head of a collection
void normalize_free(dril_sac_handle* h);
hipError_t normalize_alloc(dril_sac_handle* h, size_t rows);
int nz_ensure_raw(dril_sac_handle* h);
int nz_moments_over(dril_sac_handle* h, const float* raw, const float* rew, int* rows);
int nz_moments(dril_sac_handle* h, bool obs, bool ret, int* rows);
int nz_apply(dril_sac_handle* h, NzApplyArgs p, int rows, bool upd_obs, bool upd_ret);
int nz_observe(dril_sac_handle* h, bool update, float* out);
int nz_collect_begin(dril_sac_handle* h);
// the bodies of the verbs that read or write a wrapper that is on: one definition for dril_sac_normalize_* (device envs) and dril_sac_ext_normalize_* (external handles)
int nzv_get_config(dril_sac_handle* h, const std::string& verb, dril_sac_normalize_config* cfg);
int nzv_get_stats(dril_sac_handle* h, const std::string& verb, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count);
int nzv_set_stats(dril_sac_handle* h, const std::string& verb, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count);
int nzv_get_returns(dril_sac_handle* h, const std::string& verb, float* returns);

}  // namespace dril::sac
