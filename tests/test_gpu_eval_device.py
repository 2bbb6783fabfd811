"""GPU (-m gpu): evaluate_agent of a PPO handle on the device (dril_evaluate_agent_device, docs/evaluation.md), every check through the C ABI / pkg.Handle.

Checkers: (1) dril_evaluate_agent, the per-step host loop of the same library — same cfg, same parameters, EXACT equality of episodes, lengths, n_steps and the four
statistics (the same host arithmetic), on both paths of the new verb; (2) the CPU oracle's orc_evaluate_agent with test_evaluate_agent's tolerances; (3) for what the
call must NOT do, a twin handle that ran the same training without any evaluation, compared bitwise.
The status "no episode finishes" is not provoked: every device env, plug-ins included, truncates at its time limit inside the library's own step wrapper, so no
conforming env reaches it."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

from test_gpu_env_plugin import ALL_BUFS, _cfg, _co, _params

pytestmark = pytest.mark.gpu
E = 24                                                     # test_evaluate_agent's sizes: 24 envs, short time limits
N_EVALS = (10, E, 60, 1)                                   # below E, equal to E, 2.5 x E, one episode (std NaN)
K_STEPWISE, K_PERSISTENT = 32, 64                          # the verb's default poll intervals (docs/evaluation.md), capped by the time limit
STAT_KEYS = ("mean_reward", "std_reward", "mean_length", "std_length", "n_steps")


def limit(kind):
    return 15 if kind else 60                              # MountainCar / Pendulum / Acrobot: every episode ends at the time limit; CartPole: poles fall first


def net_size(D, hidden, out):
    n, k = 0, D
    for h in list(hidden) + [out]:
        n += k * h + h; k = h
    return n


def nudged_params(h, hidden, seed=21):
    """test_evaluate_agent's parameters; CartPole: its nudge of the actor's output bias, so that lengths differ between envs"""
    flat = _params(h.P, seed, 0.5)
    if h.discrete and h.A == 2:
        b3 = net_size(h.D, hidden, h.A) - h.A
        flat[b3:b3 + 2] = (0.8, -0.8)
    return flat


def make(pkg, kind, hidden=(64, 64), seed=13, params_seed=21, **kw):
    cfg = _cfg(pkg, kind, n_envs=E, n_steps=4, episode_len=kw.pop("episode_len", limit(kind)), batch_size=E, hidden1=hidden[0], hidden2=hidden[1], **kw)
    h = pkg.Handle(cfg)
    h.set_params(nudged_params(h, hidden, params_seed))
    if seed is not None:
        h.env_reset(seed)
    return h


def same_stats(a, b):
    for k in STAT_KEYS:
        assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


def assert_equal_runs(old, new, where):
    (so, ro, lo), (sn, rn, ln, info) = old, new
    assert np.array_equal(ln, lo), (where, ln, lo)
    assert np.array_equal(rn, ro), (where, rn, ro)
    same_stats(so, sn)
    assert info["events"] >= len(lo) and info["steps_enqueued"] >= sn["n_steps"] and info["launches"] >= 1
    return info


# ---- 1: parity with the old verb, exact ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 6, 7])
@pytest.mark.parametrize("hidden,path", [((64, 64), 1), ((128, 128), 1), ((256, 256), 1), ((32, 48), 0)])
def test_episodes_equal_the_host_loop_exactly(pkg, kind, hidden, path):
    for kw in ({}, dict(monitor_window=20), dict(fixed_length_episodes=1)):
        old, new = make(pkg, kind, hidden, **kw), make(pkg, kind, hidden, **kw)
        for det in (True, False):
            for n in N_EVALS:
                ref = old.evaluate_agent(n, det)
                info = assert_equal_runs(ref, new.evaluate_agent_device(n, det), (kind, hidden, kw, det, n))
                assert info["path"] == path
                if n == 1:
                    assert math.isnan(ref[0]["std_reward"]) and math.isnan(ref[0]["std_length"])
                if kind == 0 and n >= E and not kw.get("fixed_length_episodes"):
                    assert len(set(ref[2].tolist())) > 1, "CartPole: every episode has the same length, the comparison says little"
                if path == 1 and n == 60:                                              # the same on the step-granular launches
                    info = assert_equal_runs(ref, new.evaluate_agent_device(n, det, force_step_granular=True), (kind, hidden, kw, det, n, "forced"))
                    assert info["path"] == 0
        old.close(); new.close()


# ---- 2: parity with the CPU oracle ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,det,kw", [(0, True, {}), (0, False, {}), (1, True, dict(monitor_window=50)), (1, False, {}), (3, True, {})])
@pytest.mark.parametrize("force", [False, True])
def test_episodes_match_the_cpu_oracle(pkg, oracle_mod, kind, det, kw, force):
    """test_evaluate_agent's sizes, parameters and tolerances: lengths exact, returns rtol = atol = 2e-4"""
    cfg = _cfg(pkg, kind, n_envs=E, n_steps=4, episode_len=limit(kind), batch_size=E, **kw)
    h, o = pkg.Handle(cfg), oracle_mod.Oracle(cfg)
    flat = _params(h.P, 21, 0.5)
    if kind == 0:
        flat[4608:4610] = (0.8, -0.8)
    h.set_params(flat); o.set_params(flat)
    h.env_reset(13); o.env_reset(13)
    n = 40
    sh, rh, lh, info = h.evaluate_agent_device(n, det, force_step_granular=force)
    so, ro, lo = o.evaluate_agent(n, det)
    assert info["path"] == (0 if force else 1)
    assert np.array_equal(lh, lo)
    np.testing.assert_allclose(rh, ro, rtol=2e-4, atol=2e-4)
    for k in ("mean_reward", "std_reward", "mean_length", "std_length"):
        assert sh[k] == pytest.approx(so[k], rel=2e-4, abs=2e-4), k
    assert sh["n_steps"] == so["n_steps"]
    if kind == 0:
        assert np.allclose(rh, lh) and len(set(lh.tolist())) > 1


# ---- 3: normalisers: frozen for the call, statistics untouched -------------------------------------------------------------------------------------------------------
def stats_equal(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


@pytest.mark.parametrize("monitor", [0, 30])
@pytest.mark.parametrize("hidden", [(64, 64), (32, 48)])
def test_builtin_normaliser_is_frozen_and_equals_a_twin_that_does_not_train(pkg, monitor, hidden):
    kw = dict(norm_obs=1, norm_reward=1, monitor_window=monitor)
    a = make(pkg, 1, hidden, norm_training=1, **kw)
    a.collect_rollout(); a.collect_rollout()                                           # statistics that are not the initial ones
    st = a.norm_get_stats()
    assert st["obs_count"] > 0 and st["ret_count"] > 0 and not np.allclose(st["obs_var"], 1.0)
    b = make(pkg, 1, hidden, norm_training=0, **kw)
    b.norm_set_stats(st["obs_mean"], st["obs_var"], st["obs_count"], st["ret_mean"], st["ret_var"], st["ret_count"])
    for det in (True, False):
        for n in (10, 60):
            info = assert_equal_runs(b.evaluate_agent(n, det), a.evaluate_agent_device(n, det), (monitor, hidden, det, n))
            assert info["path"] == 0                                                   # no persistent form under a normaliser
    assert stats_equal(st, a.norm_get_stats())                                         # bitwise: nothing merged, nothing moved


def test_plugin_normaliser_is_frozen_and_equals_the_old_verb(pkg):
    kw = dict(n_envs=E, n_steps=8, batch_size=E * 8, epochs=1, episode_len=10, seed=7, monitor_window=40)
    h = pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, **kw), env_module=_co("reacher3"))
    h.normalize_enable(clip_obs=1.25, clip_reward=0.75, gamma=0.9, epsilon=1e-6)
    h.set_params(_params(h.P, 1, 0.2)); h.env_reset(4)
    h.collect_rollout(); h.collect_rollout()
    before = (h.normalize_get_stats(), h.normalize_get_returns(), h.normalize_get_original())
    assert before[0]["obs_count"] > 0
    for det in (True, False):
        for n in (10, 60):
            new = h.evaluate_agent_device(n, det)
            after = (h.normalize_get_stats(), h.normalize_get_returns(), h.normalize_get_original())
            assert stats_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
            assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1], after[2][1]) and h.normalize_config()["training"] is True
            st, sc = h.env_get_state()
            info = assert_equal_runs(h.evaluate_agent(n, det), new, (det, n))           # the old verb on the same handle (it resets the envs: put them back)
            h.env_set_state(st, sc)
            assert info["path"] == 0


# ---- 4: plug-ins -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scaling", [("cartpole_fused", False), ("reacher3_fused", False), ("pendulum_fused", True)])
@pytest.mark.parametrize("fused", [False, True])
def test_plugins_equal_the_old_verb(pkg, name, scaling, fused):
    kw = dict(n_envs=E, n_steps=4, batch_size=E * 4, episode_len=60 if name.startswith("cartpole") else 15)
    h = pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, **kw), env_module=_co(name))
    if scaling:
        h.scaling_enable(True)
    if fused:
        h.rollout_fused_enable(True)
    h.set_params(nudged_params(h, (64, 64)))
    h.env_reset(13)
    for det in (True, False):
        for n in N_EVALS:
            new = h.evaluate_agent_device(n, det)
            info = assert_equal_runs(h.evaluate_agent(n, det), new, (name, fused, det, n))
            assert info["path"] == 0
            if name.startswith("cartpole") and n >= E:
                assert len(set(new[2].tolist())) > 1
    assert h.rollout_fused_info()["enabled"] == fused


# ---- 5: the result does not depend on the poll interval ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fused_shape", "plugin"])
def test_poll_interval_changes_nothing(pkg, which):
    if which == "fused_shape":
        h, L, K0, path = make(pkg, 0, (64, 64)), limit(0), K_PERSISTENT, 1
    else:
        L, K0, path = 15, K_STEPWISE, 0
        h = pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, n_envs=E, n_steps=4, batch_size=E * 4, episode_len=L), env_module=_co("reacher3"))
        h.set_params(nudged_params(h, (64, 64))); h.env_reset(13)
    for det in (True, False):
        for n in (10, 60):
            runs = {k: h.evaluate_agent_device(n, det, poll_steps=k) for k in (0, 1, 7)}
            for k, (s, r, l, info) in runs.items():
                K = k if k else min(K0, L)
                assert info["path"] == path
                assert np.array_equal(r, runs[1][1]) and np.array_equal(l, runs[1][2]) and s["n_steps"] == runs[1][0]["n_steps"], (det, n, k)
                assert s["n_steps"] <= info["steps_enqueued"] <= s["n_steps"] + K - 1, (k, info, s["n_steps"])
                assert info["steps_enqueued"] % K == 0
            assert runs[1][3]["steps_enqueued"] == runs[1][0]["n_steps"]               # K = 1: the step-by-step definition enqueues nothing past the last episode


# ---- 6: isolation ----------------------------------------------------------------------------------------------------------------------------------------------------
def snapshot(h, normalised):
    out = dict(params=h.get_params(), opt=h.get_optimizer_state(), state=h.env_get_state(), obs=h.env_observe(update_stats=False), monitor=h.monitor_stats())
    out["bufs"] = [h.buffer(w) for w in ALL_BUFS]
    out["launches"] = h.rollout_fused_info()["last_collection_launches"] if h.cfg.env_kind == 8 else None      # (plug-in handles: the launch calls of the last collection)
    if normalised:
        out["norm"] = h.norm_get_stats(); out["orig"] = h.norm_get_original()
    return out


def assert_bitwise(a, b):
    assert np.array_equal(a["params"], b["params"])
    assert np.array_equal(a["opt"]["m"], b["opt"]["m"]) and np.array_equal(a["opt"]["v"], b["opt"]["v"]) and a["opt"]["steps"] == b["opt"]["steps"] and a["opt"]["beta_powers"] == b["opt"]["beta_powers"]
    for w, (x, y) in enumerate(zip(a["bufs"], b["bufs"])):
        assert np.array_equal(x, y, equal_nan=True), f"DRIL_BUF {w}"
    assert np.array_equal(a["state"][0], b["state"][0]) and np.array_equal(a["state"][1], b["state"][1])
    assert np.array_equal(a["obs"], b["obs"])
    assert a["monitor"] == b["monitor"] and a["launches"] == b["launches"]
    if "norm" in a:
        assert stats_equal(a["norm"], b["norm"]) and all(np.array_equal(x, y) for x, y in zip(a["orig"], b["orig"]))


@pytest.mark.parametrize("case", ["fused", "normalised", "generic", "plugin"])
def test_evaluations_between_training_iterations_change_nothing(pkg, case):
    """A: env_reset, collect, update, collect, update.  B: the same with evaluations of both paths, stochastic and deterministic, under other seeds, after the reset
    and after each update.  Everything training continues from is bitwise equal afterwards.  fused: CartPole [64,64] (both paths); normalised: Pendulum under
    cfg.norm_* with training statistics; generic: CartPole [32,48] (the generic kernels, their launch counter); plugin: reacher3 with its fused rollout on"""
    normalised, persistent = case == "normalised", case == "fused"
    hidden = (32, 48) if case == "generic" else (64, 64)
    kw = dict(monitor_window=30, epochs=2, seed=5, n_envs=E, n_steps=16, batch_size=96, hidden1=hidden[0], hidden2=hidden[1])
    if normalised:
        kw.update(norm_obs=1, norm_reward=1, norm_training=1)

    def mk():
        if case == "plugin":
            h = pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, episode_len=12, **kw), env_module=_co("reacher3_fused"))
            h.rollout_fused_enable(True)
            return h
        return pkg.Handle(_cfg(pkg, 1 if normalised else 0, episode_len=12 if normalised else 40, **kw))
    a, b = mk(), mk()
    flat = nudged_params(a, hidden)
    evals = []

    def evaluate(h):
        for det in (True, False):
            for force in (False, True):
                evals.append(h.evaluate_agent_device(7, det, seed=1000 + len(evals), force_step_granular=force))
                assert evals[-1][3]["path"] == (1 if persistent and not force else 0)

    for h, with_eval in ((a, False), (b, True)):
        h.set_params(flat); h.env_reset(13)
        if with_eval:
            evaluate(h)
        for _ in range(2):
            h.collect_rollout(); h.ppo_update()
            if with_eval:
                evaluate(h)
    assert len(evals) == 12 and all(np.isfinite(e[1]).all() for e in evals)
    assert a.monitor_stats()[2] > 0                                                    # training episodes are in the window; the evaluations' are not
    assert_bitwise(snapshot(a, normalised), snapshot(b, normalised))
    a.collect_rollout(); b.collect_rollout()                                           # and what follows is the same too (noise stream position, counters)
    assert_bitwise(snapshot(a, normalised), snapshot(b, normalised))


def test_a_never_reset_handle_evaluates_and_stays_unreset(pkg):
    capi = pkg._capi
    h = make(pkg, 0, seed=None)
    ref = make(pkg, 0, seed=3)
    for force in (False, True):
        new = h.evaluate_agent_device(30, True, seed=3, force_step_granular=force)
        assert_equal_runs(ref.evaluate_agent(30, True), new, force)
        for refused in (h.collect_rollout, h.env_observe, lambda: h.env_step(np.ones(E, np.int32))):
            with pytest.raises(pkg.DrilError) as e:
                refused()
            assert e.value.code == capi.ERR_NOT_INITIALISED and "before dril_env_reset" in str(e.value)


# ---- 7: data-parallel -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kw", [(0, {}), (1, dict(norm_obs=1, norm_reward=1, norm_training=1))])
def test_ranks_evaluate_their_own_envs_without_an_all_reduce(pkg, kind, kw):
    common = dict(n_steps=4, batch_size=2 * E, episode_len=limit(kind), seed=11, **kw)
    hs = [pkg.Handle(_cfg(pkg, kind, n_envs=E, rank=r, world_size=2, **common)) for r in range(2)]
    pkg.Handle.comm_loopback(hs)
    flat = nudged_params(hs[0], (64, 64))
    out, err = [None, None], [None, None]

    def run(r):
        try:
            hs[r].set_params(flat); hs[r].env_reset(21)
            calls = hs[r].comm_allreduce_calls()
            res = [hs[r].evaluate_agent_device(30, det, force_step_granular=force) for det in (True, False) for force in (False, True)]
            out[r] = (res, hs[r].comm_allreduce_calls() - calls)
        except BaseException as ex:   # noqa: BLE001 - re-raised below
            err[r] = ex
    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in ts]; [t.join() for t in ts]
    for ex in err:
        if ex is not None:
            raise ex
    for r in range(2):
        res, calls = out[r]
        assert calls == 0
        one = pkg.Handle(_cfg(pkg, kind, n_envs=E, **{**common, "batch_size": E}))    # the same global env indices in a handle of its own
        one.set_params(flat); one.env_reset(21 + r * E)
        i = 0
        for det in (True, False):
            for force in (False, True):
                want = one.evaluate_agent_device(30, det, force_step_granular=force)
                assert np.array_equal(res[i][1], want[1]) and np.array_equal(res[i][2], want[2]) and res[i][0]["n_steps"] == want[0]["n_steps"], (r, det, force)
                i += 1
    assert not np.array_equal(out[0][0][0][1], out[1][0][0][1]) or not np.array_equal(out[0][0][0][2], out[1][0][0][2])   # the ranks own different envs


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_healthy(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    h = make(pkg, 0)
    want = h.evaluate_agent_device(12, True)
    o, st, info = capi.DrilEvalOptions(), capi.DrilEvalStats(), capi.DrilEvalInfo()
    er, el = np.zeros(12, np.float32), np.zeros(12, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda opt, out: lib.dril_evaluate_agent_device(h._h, opt, out, p(er), p(el), C.byref(info))
    for field, bad in (("n_eval_episodes", 0), ("n_eval_episodes", -3), ("poll_steps", -1)):
        lib.dril_eval_options_default(C.byref(o)); o.n_eval_episodes = 12
        setattr(o, field, bad)
        assert call(C.byref(o), C.byref(st)) == capi.ERR_INVALID_ARG, field
        assert b"dril_evaluate_agent_device" in lib.dril_last_error(h._h)
    lib.dril_eval_options_default(C.byref(o)); o.n_eval_episodes = 12
    assert call(None, C.byref(st)) == capi.ERR_INVALID_ARG and call(C.byref(o), None) == capi.ERR_INVALID_ARG
    assert lib.dril_evaluate_agent_device(None, C.byref(o), C.byref(st), None, None, None) == capi.ERR_NOT_INITIALISED
    ext = pkg.Handle(_cfg(pkg, capi.ENV_EXTERNAL, n_envs=2, n_steps=2, batch_size=2, ext_obs_dim=6, ext_action_dim=3, ext_discrete=1))
    with pytest.raises(pkg.DrilError) as e:
        ext.evaluate_agent_device(3)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(pkg.DrilError) as e_old:
        ext.evaluate_agent(3)
    assert str(e.value) == str(e_old.value) and "DRIL_ENV_EXTERNAL live on the host" in str(e.value)   # the old verb's message
    # a failed call leaves the handle healthy; NULL episode arrays and NULL info are legal
    assert lib.dril_evaluate_agent_device(h._h, C.byref(o), C.byref(st), None, None, None) == capi.OK
    assert st.n_episodes == 12 and st.mean_reward == want[0]["mean_reward"] and st.n_steps == want[0]["n_steps"]
    again = h.evaluate_agent_device(12, True)
    assert np.array_equal(again[1], want[1]) and np.array_equal(again[2], want[2])


# ---- 9: the host mirror ---------------------------------------------------------------------------------------------------------------------------------------------
def test_host_mirror_isolated_returns_the_same_numbers_and_leaves_the_monitor_alone(pkg):
    def fresh():
        env = pkg.MonitorWrapperEnv(pkg.DeviceParallelEnv(pkg.CartPoleEnv(max_steps=100), 32, seed=3), 20)
        agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space()), pkg.PPO(n_steps=16, batch_size=128, epochs=1), seed=0)
        return env, agent
    env, agent = fresh()
    plain = pkg.evaluate_agent(agent, env, n_eval_episodes=12)
    assert env.handle.monitor_stats()[2] >= 12                                         # today's behaviour: the episodes enter the window
    env, agent = fresh()
    before = env.bind(agent.alg, agent.layer).monitor_stats()
    iso = pkg.evaluate_agent(agent, env, n_eval_episodes=12, isolated=True)
    assert iso == plain and iso["mean_reward"] == iso["mean_length"] > 0
    assert np.array_equal(env.handle.monitor_stats(), before, equal_nan=True) and before[2] == 0
    er, el = pkg.evaluate_agent(agent, env, n_eval_episodes=12, isolated=True, return_stats=False)
    assert len(er) == len(el) == 12 and float(np.mean(er)) == pytest.approx(iso["mean_reward"])
    with pytest.raises(RuntimeError):
        pkg.evaluate_agent(agent, env, n_eval_episodes=5, reward_threshold=1e9, isolated=True)
