"""GPU (-m gpu): MonitorWrapperEnv statistics and evaluate_agent of a SAC handle (dril_sac_monitor_enable / _get_stats, dril_sac_evaluate_agent) through the C ABI.

  * the monitor's window equals the finished episodes recomputed from the replay ring, for every collection form the handle has, built-in env and plug-in;
  * monitor on = monitor off for every ring field; env_reset clears the running sums and keeps the window; monitor_enable(0) forgets it;
  * evaluation against the definition on a plug-in compiled here whose episode lengths and rewards are closed-form in (env, step);
  * the result does not depend on how often the host looks (DRIL_SAC_EVAL_POLL=1 against the default);
  * physics of an evaluation: Pendulum against the CPU oracle's env verbs, reacher3 against the NumPy twin of tests/test_env_plugin.py;
  * evaluation has no side effect on ring, parameters, targets, entropy coefficient or monitor; the refusals; sac_train_ over MonitorWrapperEnv.
Switches are latched when a handle is created, so they are set around the creation only (as test_gpu_sac.py does)."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from test_env_plugin import _reacher_obs, _reacher_step
from test_gpu_sac_env_plugin import GENCO, _co, assert_rings_equal, init_params, make_module, ring, to_env

pytestmark = pytest.mark.gpu
F = np.float32


def make_builtin(pkg, E, T_lim=200, hidden=(32, 32), B=16, cap=4096, seed=7, env=None, **alg_kw):
    env = env or pkg.PendulumEnv(max_steps=T_lim)
    alg = pkg.SAC(batch_size=B, buffer_capacity=cap, **alg_kw)
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=hidden)
    return pkg.SacHandle(pkg.make_sac_config(env, E, alg, layer, seed=seed)), layer


def with_env(monkeypatch, switches, make):
    for k in switches:
        monkeypatch.setenv(k, "1")
    try:
        return make()
    finally:
        for k in switches:
            monkeypatch.delenv(k)


def episodes_of(rew, done):
    """the finished episodes of a [T][E] block in (step, env) order: float32 sums in step order, as MonitorWrapperEnv keeps them"""
    T, E = rew.shape
    cur, ln, out = np.zeros(E, F), np.zeros(E, np.int64), []
    for t in range(T):
        cur = (cur + rew[t]).astype(F); ln += 1
        for e in np.nonzero(done[t])[0]:
            out.append((cur[e], ln[e])); cur[e] = 0; ln[e] = 0
    return out


def window_of(eps, W):
    last = eps[-W:]
    return float(np.mean([float(r) for r, _ in last])), float(np.mean([l for _, l in last])), len(last)


def ring_episodes(pkg, h, E):
    r = ring(pkg, h)
    rew = r["rew"].reshape(-1, E)
    return episodes_of(rew, (r["term"] | r["trunc"]).reshape(-1, E).astype(bool))


def collect_35(h):
    h.collect_rollout(1, True)                                        # the start phase counts like any other step
    h.collect_rollout(4, False)
    h.collect_rollout(30, False)


# ---- 4: the monitor equals the ring ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name,switches", [("pendulum", ()), ("pendulum", ("DRIL_SAC_NO_FUSED_COLLECT",)), ("pendulum", ("DRIL_SAC_NO_FUSED_FWD",)),
                                               ("reacher3", ()), ("reacher3", ("DRIL_SAC_NO_FUSED_HEAD_PUSH",)), ("reacher3", ("DRIL_SAC_NO_FUSED_FWD",))])
@pytest.mark.parametrize("W", [3, 100])
def test_monitor_window_equals_the_episodes_of_the_ring(pkg, monkeypatch, env_name, switches, W):
    E = 8
    if env_name == "pendulum":
        h, layer = with_env(monkeypatch, switches, lambda: make_builtin(pkg, E, T_lim=10))
    else:
        h, layer, _ = with_env(monkeypatch, switches, lambda: make_module(pkg, _co("reacher3"), E, max_steps=10 if W == 3 else 9))
    h.set_params(init_params(pkg, layer, scale_out=3.0))
    h.monitor_enable(W)
    r0, l0, n0 = h.monitor_stats()
    assert n0 == 0 and math.isnan(r0) and math.isnan(l0)              # an empty window leaves the means untouched
    h.env_reset(5)
    collect_35(h)
    assert h.replay_size() == 35 * E
    eps = ring_episodes(pkg, h, E)
    assert len(eps) == 3 * E
    want = window_of(eps, W)
    got = h.monitor_stats()
    assert got[2] == want[2] == min(W, 3 * E)
    assert abs(got[0] - want[0]) <= 1e-6 * abs(want[0]) and abs(got[1] - want[1]) <= 1e-6 * want[1], (got, want)
    if W == 3:                                                        # the last three of a step's eight: (step, env) order, not the reverse
        assert abs(got[0] - float(np.mean([float(r) for r, _ in eps[:3]]))) > 1e-4


# ---- 5: monitor on = monitor off; reset and disable ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name", ["pendulum", "reacher3"])
def test_monitor_leaves_the_ring_alone_and_reset_keeps_the_window(pkg, env_name):
    E, capi = 8, pkg._capi
    def make():
        if env_name == "pendulum":
            return make_builtin(pkg, E, T_lim=10)
        h, layer, _ = make_module(pkg, _co("reacher3"), E, max_steps=10)
        return h, layer
    (on, layer), (off, _) = make(), make()
    flat = init_params(pkg, layer, scale_out=3.0)
    on.monitor_enable(100)
    for h in (on, off):
        h.set_params(flat); h.env_reset(5); collect_35(h)
    assert_rings_equal(ring(pkg, on), ring(pkg, off))
    assert np.array_equal(on.env_observe(), off.env_observe())
    with pytest.raises(pkg.DrilError) as e:
        off.monitor_stats()
    assert e.value.code == capi.ERR_NOT_INITIALISED and "off" in str(e.value)
    # 35 steps = three episodes and five steps into the fourth: reset! drops those five (monitorWrapperEnv.jl:36-42) and keeps the window
    assert on.monitor_stats()[2] == 3 * E
    on.env_reset(6)
    on.collect_rollout(10, False)
    rew, ln, n = on.monitor_stats()
    assert n == 4 * E
    eps = ring_episodes(pkg, on, E)                                   # the ring does not know about the reset: cut its rows at step 35
    r = ring(pkg, on)
    tail = episodes_of(r["rew"].reshape(-1, E)[35:], (r["term"] | r["trunc"]).reshape(-1, E).astype(bool)[35:])
    assert len(tail) == E and all(l == 10 for _, l in tail)
    want = window_of(eps[:3 * E] + tail, 100)
    assert abs(rew - want[0]) <= 1e-6 * abs(want[0]) and abs(ln - 10.0) <= 1e-6
    on.monitor_enable(100)                                            # the same wrapper again: nothing forgotten
    assert on.monitor_stats()[2] == 4 * E
    on.monitor_enable(0)
    with pytest.raises(pkg.DrilError):
        on.monitor_stats()
    on.monitor_enable(5)
    assert on.monitor_stats()[2] == 0
    on.collect_rollout(10, False)
    assert on.monitor_stats()[2] == 5
    with pytest.raises(pkg.DrilError) as e:
        on.monitor_enable(-1)
    assert e.value.code == capi.ERR_INVALID_ARG


# ---- 6: evaluation against the definition --------------------------------------------------------------------------------------------------------------------------
_STAIRS = '''#include "device/dril_env_plugin.h"
struct Stairs {
    static constexpr int S = 2, D = 2, A = 1;
    static constexpr bool discrete = false;
    static constexpr int episode_len = 50;
    static constexpr float action_low[A] = {-1.0f}, action_high[A] = {1.0f};
    static constexpr const char* name = "Stairs";
    DRIL_ENV_FN static void reset(const DrilEnvRng& rng, float* st) { st[0] = 0.0f; st[1] = (float)(rng.env_seed % 4096u); }   // evaluated with seed 0: the env's index
    DRIL_ENV_FN static void observe(const float* st, float* obs) { obs[0] = st[0]; obs[1] = st[1]; }
    DRIL_ENV_FN static float step(float* st, const float* act_f, int act_i, bool* terminated) {
        st[0] = st[0] + 1.0f;
        *terminated = (int)st[0] >= 3 + ((int)st[1]) % 5;
        return 0.5f * st[0] + st[1];
    }
};
DRIL_ENV_PLUGIN(Stairs)
'''


def test_evaluation_equals_the_closed_form_episode_list(pkg, tmp_path):
    src = tmp_path / "stairs.hip"; src.write_text(_STAIRS)
    co = tmp_path / "stairs.hsaco"
    subprocess.run([*GENCO, str(src), "-o", str(co)], check=True)
    E = 12
    h, layer, _ = make_module(pkg, co, E, cap=64)
    h.set_params(init_params(pkg, layer))
    length = lambda e: 3 + e % 5
    ret = lambda e: F(sum(F(0.5) * F(k) + F(e) for k in range(1, length(e) + 1)))
    for n_eval in (1, E - 1, E, 3 * E + 2):
        events, s = [], 0
        while len(events) < n_eval:                                   # evaluation.jl:92-122: step, then the envs in index order
            s += 1
            events += [(s, e) for e in range(E) if s % length(e) == 0]
        events = events[:n_eval]
        stats, er, el = h.evaluate_agent(n_eval, True, seed=0)
        want_r, want_l = np.array([ret(e) for _, e in events], F), np.array([length(e) for _, e in events], np.int32)
        assert np.array_equal(er, want_r) and np.array_equal(el, want_l), (n_eval, er, want_r)
        assert stats["n_steps"] == events[-1][0]
        assert stats["mean_reward"] == pytest.approx(want_r.astype(np.float64).mean(), rel=1e-12) and stats["mean_length"] == pytest.approx(want_l.mean(), rel=1e-12)
        if n_eval == 1:
            assert math.isnan(stats["std_reward"]) and math.isnan(stats["std_length"])
        else:
            assert stats["std_reward"] == pytest.approx(want_r.astype(np.float64).std(ddof=1), rel=1e-12) and stats["std_length"] == pytest.approx(want_l.std(ddof=1), rel=1e-12)
    assert h.replay_size() == 0                                       # evaluations alone leave the ring empty


# ---- 7: the result does not depend on the poll interval --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name", ["pendulum", "reacher3"])
def test_evaluation_is_independent_of_the_poll_interval(pkg, monkeypatch, env_name):
    E = 24
    def make():
        if env_name == "pendulum":
            return make_builtin(pkg, E, T_lim=60, hidden=(64, 64))
        h, layer, _ = make_module(pkg, _co("reacher3"), E, hidden=(64, 64), max_steps=40)
        return h, layer
    default, layer = make()
    monkeypatch.setenv("DRIL_SAC_EVAL_POLL", "1")
    try:
        single, _ = make()
    finally:
        monkeypatch.delenv("DRIL_SAC_EVAL_POLL")
    monkeypatch.setenv("DRIL_SAC_EVAL_POLL", "7")
    try:
        seven, _ = make()
    finally:
        monkeypatch.delenv("DRIL_SAC_EVAL_POLL")
    flat = init_params(pkg, layer, scale_out=3.0)
    for h in (default, single, seven):
        h.set_params(flat)
    for det, n_eval in ((True, 2 * E + 5), (False, E + 1), (False, 3)):
        out = [h.evaluate_agent(n_eval, det, seed=11) for h in (default, single, seven)]
        for st, er, el in out[1:]:
            assert np.array_equal(er, out[0][1]) and np.array_equal(el, out[0][2]) and st["n_steps"] == out[0][0]["n_steps"]
            assert st["mean_reward"] == out[0][0]["mean_reward"]
        assert np.isfinite(out[0][1]).all() and (out[0][2] >= 1).all()


# ---- 8: physics ---------------------------------------------------------------------------------------------------------------------------------------------------------
def constant_actor(pkg, layer, bias):
    ps = layer.initialparameters(np.random.default_rng(0))
    ps["actor_head"]["layer_3"]["weight"][...] = 0                    # mu = b3 whatever the observation
    ps["actor_head"]["layer_3"]["bias"][...] = np.asarray(bias, F)
    return pkg.sac_flatten_params(ps)


def test_pendulum_evaluation_follows_the_oracle_envs(pkg, oracle_mod):
    E, T_lim, b, seed, capi = 8, 20, 0.3, 31, pkg._capi
    h, layer = make_builtin(pkg, E, T_lim=T_lim)
    h.set_params(constant_actor(pkg, layer, [b]))
    stats, er, el = h.evaluate_agent(2 * E, True, seed=seed)
    act = to_env(np.full(E, np.tanh(F(b)), F), F(-2), F(2))            # mode = tanh(mean); TanhScaleAdapter squashes again and scales into Box(-2, 2)
    cfg = capi.default_config(capi.ENV_PENDULUM)
    cfg.n_envs, cfg.n_steps, cfg.batch_size, cfg.epochs, cfg.episode_len = E, 8, 8, 1, T_lim
    o = oracle_mod.Oracle(cfg); o.env_reset(seed)
    rew = np.zeros((2 * T_lim, E), F); done = np.zeros((2 * T_lim, E), bool)
    for t in range(2 * T_lim):
        r, term, trunc, _ = o.env_step(act)
        rew[t], done[t] = r, term | trunc
    want = episodes_of(rew, done)
    assert len(want) == 2 * E and stats["n_steps"] == 2 * T_lim and (el == T_lim).all()
    np.testing.assert_allclose(er, np.array([r for r, _ in want], F), rtol=1e-4)
    assert len(np.unique(er)) > E                                     # seeded seed + e: the envs differ, and so do an env's two episodes
    # a sample: reproducible for one seed, not the mode, not another seed's
    s1, s2, s3 = (h.evaluate_agent(E, False, seed=s)[1] for s in (seed, seed, seed + 1))
    assert np.array_equal(s1, s2) and not np.array_equal(s1, er[:E]) and not np.array_equal(s1, s3)


def test_reacher3_evaluation_follows_the_numpy_twin(pkg):
    E, T_lim, seed = 6, 7, 21
    b = np.array([0.4, -0.2, 0.9], F)
    h, layer, _ = make_module(pkg, _co("reacher3"), E, max_steps=T_lim)
    h.set_params(constant_actor(pkg, layer, b))
    stats, er, el = h.evaluate_agent(E, True, seed=seed)
    h.env_reset(seed)
    st = h.env_observe()[:, :9]                                       # reacher3 shows its whole state
    act = np.tile(to_env(np.tanh(b), -np.ones(3, F), np.ones(3, F)), (E, 1))
    total = np.zeros(E, F)
    for _ in range(T_lim):
        st, rew, out = _reacher_step(st, act)
        assert not out.any()
        total = (total + rew).astype(F)
    assert (el == T_lim).all() and stats["n_steps"] == T_lim
    np.testing.assert_allclose(er, total, rtol=1e-4)
    s1, s2, s3 = (h.evaluate_agent(E, False, seed=s)[1] for s in (seed, seed, seed + 1))
    assert np.array_equal(s1, s2) and not np.array_equal(s1, er) and not np.array_equal(s1, s3)


# ---- 9: no side effects ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name", ["pendulum", "reacher3"])
def test_evaluation_has_no_side_effect_on_training(pkg, env_name):
    E = 8
    def make():
        if env_name == "pendulum":
            return make_builtin(pkg, E, T_lim=4, cap=256)
        h, layer, _ = make_module(pkg, _co("reacher3"), E, max_steps=4, cap=256)
        return h, layer
    (a, layer), (b, _) = make(), make()
    flat = init_params(pkg, layer, scale_out=3.0)
    st0, er0, el0 = a.evaluate_agent(E + 2, True, seed=3)             # an empty ring, envs never reset: an evaluation brings its own reset
    assert a.replay_size() == 0 and (el0 == 4).all() and st0["n_steps"] == 8
    for h, evaluate in ((a, True), (b, False)):
        h.set_params(flat); h.monitor_enable(100); h.env_reset(9)
        h.collect_rollout(5, False)
        if evaluate:
            h.evaluate_agent(3 * E, False, seed=77)
            h.evaluate_agent(2, True, seed=9)
        h.collect_rollout(5, False)
        h.update(3)
    assert_rings_equal(ring(pkg, a), ring(pkg, b))
    assert np.array_equal(a.get_params(), b.get_params()) and np.array_equal(a.get_target_params(), b.get_target_params())
    assert a.get_log_ent_coef() == b.get_log_ent_coef()
    assert a.monitor_stats() == b.monitor_stats() and a.monitor_stats()[2] == 2 * E
    assert np.array_equal(a.env_observe(), b.env_observe())
    assert not np.array_equal(a.get_params(), flat)


# ---- 10: refusals ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_an_external_handle_and_bad_arguments(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    healthy, layer = make_builtin(pkg, 8, T_lim=10, cap=256)
    healthy.set_params(init_params(pkg, layer)); healthy.env_reset(1)

    def still_collects():
        n = healthy.replay_size()
        healthy.collect_rollout(2, False)
        assert healthy.replay_size() == min(256, n + 16) and np.isfinite(healthy.replay(capi.RB_REWARDS)).all()

    cfg = capi.DrilSacConfig()
    assert lib.dril_sac_config_default(C.byref(cfg), capi.ENV_EXTERNAL) == capi.OK
    cfg.n_envs, cfg.hidden1, cfg.hidden2, cfg.batch_size, cfg.buffer_capacity = 4, 32, 32, 8, 64
    cfg.ext_obs_dim, cfg.ext_action_dim, cfg.ext_action_low, cfg.ext_action_high = 5, 2, -1.0, 1.0
    ext = pkg.SacHandle(cfg)
    for call in (lambda: ext.monitor_enable(100), ext.monitor_stats, lambda: ext.evaluate_agent(3)):
        with pytest.raises(pkg.DrilError) as e:
            call()
        assert e.value.code == capi.ERR_UNSUPPORTED and "host" in str(e.value), str(e.value)
        still_collects()
    st = capi.DrilEvalStats()
    assert lib.dril_sac_evaluate_agent(healthy._h, 0, 1, 0, C.byref(st), None, None) == capi.ERR_INVALID_ARG
    assert lib.dril_sac_evaluate_agent(healthy._h, 3, 1, 0, None, None, None) == capi.ERR_INVALID_ARG
    assert lib.dril_sac_monitor_enable(healthy._h, -3) == capi.ERR_INVALID_ARG
    still_collects()
    stats, er, el = healthy.evaluate_agent(3)                         # and the healthy handle evaluates: episode_rewards / lengths may also be NULL
    assert lib.dril_sac_evaluate_agent(healthy._h, 3, 1, healthy.cfg.seed, C.byref(st), None, None) == capi.OK
    assert st.mean_reward == stats["mean_reward"] and st.n_episodes == 3 and st.n_steps == 10
    still_collects()


# ---- 11: sac_train_ over MonitorWrapperEnv, evaluate_agent of an agent --------------------------------------------------------------------------------------------------------
def test_sac_train_feeds_the_monitor_and_an_agent_evaluates(pkg):
    E = 8
    env = pkg.MonitorWrapperEnv(pkg.DeviceParallelEnv(pkg.PendulumEnv(), E, seed=3), 100)
    alg = pkg.SAC(batch_size=64, buffer_capacity=4096, start_steps=100)
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(64, 64))
    agent = pkg.SACAgent(layer, alg, seed=1)
    agent, rb, ts, _ = pkg.sac_train_(agent, env, alg, 8 * 420)
    assert set(ts) == {"actor_losses", "critic_losses", "entropy_losses", "entropy_coefficients", "q_values", "learning_rates", "grad_norms", "fps", "steps_taken"}
    rew, ln, n = rb.handle.monitor_stats()
    eps = ring_episodes(pkg, rb.handle, E)
    assert n == len(eps) == 2 * E and ln == 200.0 and np.isfinite(rew)
    want = window_of(eps, 100)
    assert abs(rew - want[0]) <= 1e-6 * abs(want[0])
    er, el = pkg.sac_evaluate_agent(agent, env, return_stats=False)
    assert len(er) == 10 and (el == 200).all() and np.isfinite(er).all()
    stats = pkg.sac_evaluate_agent(agent, env)
    assert set(stats) == {"mean_reward", "std_reward", "mean_length", "std_length"} and stats["mean_length"] == 200.0
    assert stats["mean_reward"] == pytest.approx(float(np.mean(er.astype(np.float64))), rel=1e-12)
    with pytest.raises(RuntimeError, match="threshold"):
        pkg.sac_evaluate_agent(agent, env, reward_threshold=1.0)
    # the callback form switches the monitor on too
    class Quiet:
        def on_rollout_end(self, loc):
            return True
    agent2 = pkg.SACAgent(layer, alg, seed=1)
    _, rb2, _, _ = pkg.sac_train_(agent2, env, alg, 8 * 210, callbacks=[Quiet()])
    assert rb2.handle.monitor_stats()[2] == E
