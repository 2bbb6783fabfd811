"""GPU (-m gpu): NormalizeWrapperEnv around a device env plug-in of a PPO handle (dril_normalize_*, kernels dril_ppo_norm.h), every check through the C ABI / pkg.Handle.

Checkers: (1) the NumPy restatement of the wrapper (tests/sac_normalize_ref.py) fed the raw observations / rewards of a TWIN plug-in handle without the wrapper that is
stepped with the same actions; (2) the built-in Pendulum / CartPole under cfg.norm_* (pinned by the CPU oracle elsewhere) against their plug-in twins under the new verbs.
Every test begins with dril_normalize_enable, so without the feature every one of them fails there (missing symbol)."""
import ctypes as C
import subprocess
import threading

import numpy as np
import pytest

import sac_normalize_ref as ref
from test_gpu_env_plugin import ALL_BUFS, _cfg, _co, _params, _stats
from test_gpu_sac_env_plugin import GENCO
from test_gpu_sac_normalize import _WIDE, assert_stats

pytestmark = pytest.mark.gpu
F = np.float32
KW = dict(clip_obs=1.25, clip_reward=0.75, gamma=0.9, epsilon=1e-6)
TOL = dict(rtol=3e-5, atol=3e-5)


@pytest.fixture(scope="module")
def cos(tmp_path_factory):
    """name -> code object: the three examples and the wide test plug-in at 133 dims (three column tiles, a ragged last one) and 300 dims (five tiles)"""
    d = tmp_path_factory.mktemp("wide_ppo")
    (d / "wide.hip").write_text(_WIDE)
    out = {n: _co(n) for n in ("reacher3", "cartpole", "pendulum")}
    for D in (133, 300):
        out[f"wide{D}"] = d / f"wide{D}.hsaco"
        subprocess.run([*GENCO, f"-DWIDE_D={D}", str(d / "wide.hip"), "-o", str(out[f"wide{D}"])], check=True)
    return out


def mk(pkg, co, E, T=4, L=5, normalize=None, **kw):
    kw = {**dict(n_envs=E, n_steps=T, batch_size=E * T, epochs=1, episode_len=L, seed=7), **kw}
    h = pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, **kw), env_module=co)
    if normalize is not None:
        h.normalize_enable(**normalize)
    return h


def rand_actions(h, rng):
    return rng.integers(1, 3, h.E).astype(np.int32) if h.discrete else rng.uniform(-1.5, 1.5, (h.E, h.A)).astype(F)


def flag_bytes(term, trunc):
    return term.astype(np.uint8) | (trunc.astype(np.uint8) << 1)


# ---- 1: the wrapper is the reference's wrapper ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,E", [("reacher3", 37), ("wide133", 70), ("wide300", 530), ("cartpole", 50)])
@pytest.mark.parametrize("norm_obs,norm_reward", [(1, 1), (1, 0), (0, 1)])
def test_step_verbs_equal_the_numpy_wrapper_over_a_twin_without_it(pkg, cos, name, E, norm_obs, norm_reward):
    kw = dict(norm_obs=norm_obs, norm_reward=norm_reward, **KW)
    h, u = mk(pkg, cos[name], E, normalize=kw), mk(pkg, cos[name], E)
    assert h.normalize_config() == pytest.approx(dict(training=True, **kw))
    w = ref.Wrapper(E, h.D, **kw)
    for x in (h, u):
        x.env_reset(11)
    assert np.array_equal(h.normalize_get_original()[0], u.env_observe())              # reset! stores old_obs
    rng = np.random.default_rng(3)
    n_trunc = 0
    for t in range(12):
        raw = u.env_observe()
        got, exp = h.env_observe(), w.observe(raw)
        assert np.allclose(got, exp, **TOL), (t, np.abs(got - exp).max())
        if not norm_obs:
            assert np.array_equal(got, raw)
        assert np.array_equal(h.normalize_get_original()[0], raw)
        act = rand_actions(h, rng)
        ru, tu, uu, ou = u.env_step(act); rh, th, uh, oh = h.env_step(act)
        assert np.array_equal(tu, th) and np.array_equal(uu, uh)
        rn, on = w.act(ru, tu, uu, ou)
        assert np.allclose(rh, rn, **TOL), (t, np.abs(rh - rn).max())
        assert np.allclose(oh[uu], on[uu], **TOL)                                        # the statistics as they are BEFORE the following observe
        assert np.array_equal(h.normalize_get_original()[1], ru)
        assert np.allclose(h.normalize_get_returns(), w.returns, **TOL)
        n_trunc += int(uu.sum())
    assert n_trunc > 0
    st = h.normalize_get_stats()
    assert st["obs_count"] == (12 * E if norm_obs else 0) and st["ret_count"] == (12 * E if norm_reward else 0)
    assert_stats(st, w)
    old = h.norm_get_stats()                                                             # with the wrapper on, the built-in envs' verbs forward
    assert all(np.array_equal(st[k], old[k]) for k in st)
    if norm_obs:
        assert np.abs(got).max() == F(1.25)                                              # the clip is hit and held
    peek = h.env_observe(update_stats=False)
    assert np.allclose(peek, w.normalize_obs(u.env_observe()), **TOL)
    assert all(np.array_equal(st[k], v) for k, v in h.normalize_get_stats().items())     # a peek moves nothing


# ---- 2: a whole rollout ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,E", [("reacher3", 48), ("wide300", 40)])
def test_rollout_buffer_equals_the_numpy_wrapper_over_the_raw_steps(pkg, cos, name, E):
    capi = pkg._capi
    T, L = 14, 5
    h, u = mk(pkg, cos[name], E, T, L, normalize=KW), mk(pkg, cos[name], E, T, L)
    flat = _params(h.P, 5, 0.1)
    for x in (h, u):
        x.set_params(flat); x.env_reset(13)
    w = ref.Wrapper(E, h.D, **KW)
    rng = np.random.default_rng(1)
    for k in (1, 2):
        h.set_noise(rng.standard_normal((E * T, h.A)).astype(F))
        h.collect_rollout()
        act = h.buffer(capi.BUF_ACTIONS).reshape(T, E, h.A)
        obs, rew, boot = np.empty((T, E, h.D), F), np.empty((T, E), F), np.zeros((T, E), F)
        flags = np.empty((T, E), np.uint8)
        cur = w.observe(u.env_observe())                                                 # trajectory.jl:32
        for t in range(T):
            obs[t] = cur
            r, term, trunc, tobs = u.env_step(act[t])                                    # the raw per-step data of the same rollout (the plug-in clamps the raw action itself)
            rew[t], tn = w.act(r, term, trunc, tobs)
            flags[t] = flag_bytes(term, trunc)
            if trunc.any():
                boot[t, trunc] = h.predict_values(tn[trunc])
            cur = w.observe(u.env_observe())
        assert np.array_equal(h.buffer(capi.BUF_FLAGS).reshape(T, E), flags) and (flags & 2).any()
        got = h.buffer(capi.BUF_OBSERVATIONS).reshape(T, E, h.D)
        assert np.allclose(got, obs, **TOL), np.abs(got - obs).max()
        assert np.allclose(h.buffer(capi.BUF_REWARDS).reshape(T, E), rew, **TOL)
        assert np.allclose(h.buffer(capi.BUF_VALUES), h.predict_values(got.reshape(T * E, h.D)), rtol=1e-4, atol=1e-4)   # V of the row the buffer holds
        tr = (flags & 2) != 0
        assert np.allclose(h.buffer(capi.BUF_BOOTSTRAP).reshape(T, E)[tr], boot[tr], rtol=2e-4, atol=2e-4)              # V(normalised terminal observation)
        assert np.allclose(h.buffer(capi.BUF_LAST_VALUES), h.predict_values(cur), rtol=2e-4, atol=2e-4)
        st = h.normalize_get_stats()
        assert st["obs_count"] == k * E * (T + 1) and st["ret_count"] == k * E * T
        assert_stats(st, w)
        assert np.allclose(h.normalize_get_returns(), w.returns, **TOL)
        assert np.array_equal(h.env_get_state()[0], u.env_get_state()[0])


# ---- 3: twin against built-in ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("cartpole", 0), ("pendulum", 1)])
def test_twin_under_the_verbs_equals_the_builtin_under_cfg_norm(pkg, cos, monkeypatch, name, kind):
    """The built-in env under cfg.norm_* on the generic kernels against its plug-in twin under dril_normalize_enable, two iterations with the update.  Decided once:
    agreement to 1e-5 relative, not to the bit.  The two paths add the same float32 values into float64 sums in different orders (the built-in: 256 envs per table
    row, one thread per env; here: rows of 16+ envs, lanes over the flat (env, dim) index), so a batch mean can differ in its last float64 digits and, rarely, in
    the float32 it is rounded to; everything downstream of the statistics inherits that.  Flags and Discrete actions are compared exactly."""
    capi = pkg._capi
    E, T = 64, 24
    nk = dict(norm_obs=1, norm_reward=1, clip_obs=5.0, clip_reward=2.0, gamma=0.95, epsilon=1e-6)
    kw = dict(n_envs=E, n_steps=T, batch_size=E * T // 2, epochs=2, episode_len=9, seed=3, hidden1=64, hidden2=64, monitor_window=50)
    monkeypatch.setenv("DRIL_FORCE_GENERIC", "1")
    b = pkg.Handle(_cfg(pkg, kind, norm_training=1, norm_gamma=nk["gamma"], norm_epsilon=nk["epsilon"], **{k: nk[k] for k in ("norm_obs", "norm_reward", "clip_obs", "clip_reward")}, **kw))
    monkeypatch.delenv("DRIL_FORCE_GENERIC")
    m = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, **kw), env_module=cos[name])
    m.normalize_enable(**nk)
    flat = _params(b.P, 3, 0.4)
    for h in (b, m):
        h.set_params(flat); h.env_reset(11)
    close = dict(rtol=1e-5, atol=1e-5)
    for it in range(2):
        rng = np.random.default_rng(10 + it)
        nz = rng.random(E * T) if kind == 0 else (rng.standard_normal((E * T, 1)) * 2).astype(F)
        perm = np.stack([rng.permutation(E * T) for _ in range(2)]).astype(np.int64)
        for h in (b, m):
            h.set_noise(nz); h.collect_rollout()
        assert np.array_equal(b.buffer(capi.BUF_FLAGS), m.buffer(capi.BUF_FLAGS)) and (m.buffer(capi.BUF_FLAGS) & 2).any()
        for which in ALL_BUFS:
            x, y = b.buffer(which), m.buffer(which)
            if which == capi.BUF_FLAGS or (which == capi.BUF_ACTIONS and kind == 0):
                assert np.array_equal(x, y), (it, which)
            else:
                wide = which in (capi.BUF_ADVANTAGES, capi.BUF_RETURNS)
                assert np.allclose(x, y, rtol=1e-4 if wide else 1e-5, atol=1e-4 if wide else 1e-5), (it, which, np.abs(x - y).max())
        sb, sm = b.norm_get_stats(), m.normalize_get_stats()
        assert sb["obs_count"] == sm["obs_count"] == (it + 1) * E * (T + 1) and sb["ret_count"] == sm["ret_count"] == (it + 1) * E * T
        for k in ("obs_mean", "obs_var", "ret_mean", "ret_var"):
            assert np.allclose(sb[k], sm[k], **close), (it, k)
        assert b.monitor_stats() == pytest.approx(m.monitor_stats(), rel=1e-5)
        for h in (b, m):
            h.set_permutation(perm)
        ub, um = b.ppo_update(), m.ppo_update()
        assert ub.n_updates == um.n_updates == 4 and ub.loss == pytest.approx(um.loss, rel=1e-3, abs=1e-5)
        assert np.allclose(b.get_params(), m.get_params(), rtol=1e-4, atol=1e-5)


# ---- 4: behaviour ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_frozen_statistics_and_the_set_get_round_trip_at_300_dims(pkg, cos):
    E = 45
    h, u = mk(pkg, cos["wide300"], E, normalize=KW), mk(pkg, cos["wide300"], E)
    rng = np.random.default_rng(0)
    st = dict(obs_mean=rng.standard_normal(300).astype(F), obs_var=rng.uniform(0.5, 2, 300).astype(F), obs_count=1234, ret_mean=0.5, ret_var=2.25, ret_count=77)
    h.normalize_set_stats(**st)
    back = h.normalize_get_stats()
    assert all(np.array_equal(np.asarray(st[k], F), np.asarray(back[k], F)) for k in st)
    h.normalize_set_training(False)
    assert h.normalize_config()["training"] is False
    w = ref.Wrapper(E, 300, training=False, **KW); w.set_stats(st)
    for x in (h, u):
        x.env_reset(2)
    for t in range(7):
        raw = u.env_observe()
        assert np.allclose(h.env_observe(), w.observe(raw), **TOL)
        act = rand_actions(h, rng)
        ru, tu, uu, ou = u.env_step(act); rh, _, _, oh = h.env_step(act)
        rn, on = w.act(ru, tu, uu, ou)
        assert np.allclose(rh, rn, **TOL) and np.allclose(oh[uu], on[uu], **TOL)
    assert not h.normalize_get_returns().any()                                           # training off: the returns recursion does not run
    now = h.normalize_get_stats()
    assert all(np.array_equal(back[k], now[k]) for k in back)


def test_reset_keeps_statistics_reenable_keeps_them_and_null_means_off(pkg, cos):
    capi = pkg._capi
    E, T = 32, 8                                                                         # (episode_len 5: the rollout ends three steps into an episode, `returns` are not zero)
    h, never = mk(pkg, cos["reacher3"], E, T, normalize=KW), mk(pkg, cos["reacher3"], E, T)
    flat = _params(h.P, 4, 0.2)
    for x in (h, never):
        x.set_params(flat); x.env_reset(5)
    h.collect_rollout()
    st = h.normalize_get_stats()
    assert st["obs_count"] == E * (T + 1) and h.normalize_get_returns().any()
    h.env_reset(5)                                                                       # reset! :110-121
    assert not h.normalize_get_returns().any()
    assert all(np.array_equal(st[k], v) for k, v in h.normalize_get_stats().items())
    h.normalize_enable(**{**KW, "training": False})                                      # only `training` differs: the same wrapper
    assert all(np.array_equal(st[k], v) for k, v in h.normalize_get_stats().items()) and h.normalize_config()["training"] is False
    h.normalize_enable(**{**KW, "clip_obs": 3.0})                                        # another wrapper: fresh
    fresh = h.normalize_get_stats()
    assert fresh["obs_count"] == 0 and not fresh["obs_mean"].any() and (fresh["obs_var"] == 1).all() and fresh["ret_var"] == 1
    h.normalize_enable(False)                                                            # NULL: off, and the handle is the handle that never had it
    with pytest.raises(pkg.DrilError) as e:
        h.normalize_get_stats()
    assert e.value.code == capi.ERR_NOT_INITIALISED
    with pytest.raises(pkg.DrilError) as e:
        h.norm_get_stats()
    assert e.value.code == capi.ERR_UNSUPPORTED
    h.env_reset(5)
    nz = np.random.default_rng(0).standard_normal((E * T, 3)).astype(F)
    for x in (h, never):
        x.set_noise(nz); x.collect_rollout()
    for which in ALL_BUFS:
        assert np.array_equal(h.buffer(which), never.buffer(which)), which


def test_evaluate_leaves_no_trace_and_the_monitor_sees_raw_rewards(pkg, cos):
    capi = pkg._capi
    E, T, L = 16, 40, 10
    h = mk(pkg, cos["reacher3"], E, T, L, normalize=KW, monitor_window=1000)
    u = mk(pkg, cos["reacher3"], E, T, L, monitor_window=1000)
    flat = _params(h.P, 1, 0.2)
    for x in (h, u):
        x.set_params(flat); x.env_reset(4)
    h.collect_rollout()
    act = h.buffer(capi.BUF_ACTIONS).reshape(T, E, 3)
    raw = np.stack([u.env_step(act[t])[0] for t in range(T)])                            # the twin's raw rewards under the same actions, through its own monitor
    assert h.monitor_stats() == pytest.approx(u.monitor_stats(), rel=1e-6) and h.monitor_stats()[2] > E
    assert not np.allclose(h.buffer(capi.BUF_REWARDS).reshape(T, E), raw)               # the buffer holds normalised rewards
    before = (h.normalize_get_stats(), h.normalize_get_returns(), h.normalize_get_original())
    s1, r1, l1 = h.evaluate_agent(12, True)
    s2, r2, l2 = h.evaluate_agent(12, True)
    assert np.array_equal(r1, r2) and np.array_equal(l1, l2) and (l1 <= L).all() and np.isfinite(r1).all()
    after = (h.normalize_get_stats(), h.normalize_get_returns(), h.normalize_get_original())
    assert all(np.array_equal(before[0][k], after[0][k]) for k in before[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1], after[2][1]) and h.normalize_config()["training"] is True
    # raw episode returns: the same frozen statistics on a twin whose reward half is off give the same episodes
    v = mk(pkg, cos["reacher3"], E, T, L, normalize={**KW, "norm_reward": 0}, monitor_window=1000)
    v.set_params(flat); v.env_reset(4); st = before[0]
    v.normalize_set_stats(st["obs_mean"], st["obs_var"], st["obs_count"], 0.0, 1.0, 0)
    _, r3, l3 = v.evaluate_agent(12, True)
    assert np.array_equal(l1, l3) and np.allclose(r1, r3, rtol=1e-6) and np.abs(r1).max() > L * 0.75   # more than an episode of clipped rewards could sum to


# ---- 5: two loopback ranks ------------------------------------------------------------------------------------------------------------------------------------------
def test_two_loopback_ranks_share_one_set_of_statistics(pkg, cos):
    capi = pkg._capi
    E, T, L = 24, 6, 4
    kw = dict(n_steps=T, batch_size=2 * E * T, epochs=1, episode_len=L, seed=9)
    hs = [pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=E, rank=r, world_size=2, **kw), env_module=cos["reacher3"]) for r in range(2)]
    one = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=2 * E, **kw), env_module=cos["reacher3"])   # the same 2 E envs in one handle, without the wrapper
    pkg.Handle.comm_loopback(hs)
    flat = _params(one.P, 2, 0.2)
    out, err = [None, None], [None, None]

    def run(r):
        try:
            hs[r].normalize_enable(**KW); hs[r].set_params(flat); hs[r].env_reset(21); hs[r].collect_rollout()
            out[r] = dict(stats=hs[r].normalize_get_stats(), act=hs[r].buffer(capi.BUF_ACTIONS), obs=hs[r].buffer(capi.BUF_OBSERVATIONS),
                          rew=hs[r].buffer(capi.BUF_REWARDS), calls=hs[r].comm_allreduce_calls())
        except BaseException as ex:   # noqa: BLE001 - re-raised below
            err[r] = ex
    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in ts]; [t.join() for t in ts]
    for ex in err:
        if ex is not None:
            raise ex
    a, b = out[0]["stats"], out[1]["stats"]
    assert all(np.array_equal(a[k], b[k]) for k in a)                                    # bit-identical across ranks
    assert out[0]["calls"] == out[1]["calls"] == T + 1                                   # the opening observe, then ONE all-reduce per step (act! and observe share a row)
    act = np.concatenate([out[r]["act"].reshape(T, E, 3) for r in range(2)], axis=1)
    one.env_reset(21)
    w = ref.Wrapper(2 * E, 12, **KW)
    cur = w.observe(one.env_observe())
    for t in range(T):
        for r in range(2):
            assert np.allclose(out[r]["obs"].reshape(T, E, 12)[t], cur[r * E:(r + 1) * E], **TOL), (t, r)
        rew, term, trunc, tobs = one.env_step(act[t])
        rn, _ = w.act(rew, term, trunc, tobs)
        for r in range(2):
            assert np.allclose(out[r]["rew"].reshape(T, E)[t], rn[r * E:(r + 1) * E], **TOL), (t, r)
        cur = w.observe(one.env_observe())
    assert a["obs_count"] == 2 * E * (T + 1) and a["ret_count"] == 2 * E * T
    assert_stats(a, w)


# ---- 6: training ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_reacher3_trains_under_the_wrapper(pkg, cos):
    """train_ through the public Python surface: DeviceModuleEnv(..., normalize={}) + MonitorWrapperEnv + Agent — the configuration of
    examples/ppo_device_plugin.py 64 40 --normalize.  One real run of it on an MI355X: the mean episode return over the monitor window went from -220.2 after the
    first rollout to -21.9 after the fortieth (-20.8 after the thirty-ninth); evaluate_agent, 20 deterministic episodes: -14.8 +- 4.7.  The margin asked for is 100."""
    env = pkg.MonitorWrapperEnv(pkg.DeviceModuleEnv(cos["reacher3"], 64, seed=0, normalize={}), stats_window=64)
    alg = pkg.PPO(n_steps=100, batch_size=1600, epochs=10, learning_rate=1e-3)
    agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space()), alg, seed=0)
    seen = []

    class Log:
        def on_rollout_end(self, loc):
            seen.append(loc["env"].handle.monitor_stats()[0]); return True
    pkg.train_(agent, env, alg, 64 * 100 * 40, callbacks=[Log()])
    assert len(seen) == 40 and np.isfinite(seen).all()
    assert seen[-1] > seen[0] + TRAIN_MARGIN, (seen[0], seen[-1])
    st = env.handle.normalize_get_stats()
    assert st["obs_count"] == 40 * 64 * 101 and st["ret_count"] == 40 * 64 * 100
    obs = np.ones((2, 12), F)
    assert np.allclose(pkg.unnormalize_obs_(obs.copy(), env), np.sqrt(st["obs_var"] + F(1e-8)) + st["obs_mean"])
    assert pkg.get_original_obs(env).shape == (64, 12) and pkg.get_original_rewards(env).shape == (64,)
    ev = pkg.evaluate_agent(agent, env, n_eval_episodes=16)
    assert np.isfinite(ev["mean_reward"]) and ev["mean_reward"] < 0                      # raw returns: every reacher3 reward is negative
    assert all(np.array_equal(st[k], v) for k, v in env.handle.normalize_get_stats().items())


TRAIN_MARGIN = 100.0


# ---- 7: refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, cos):
    capi = pkg._capi
    lib = capi.load_library()
    builtin = pkg.Handle(_cfg(pkg, 0, n_envs=4, n_steps=2, batch_size=8))
    ext = pkg.Handle(_cfg(pkg, capi.ENV_EXTERNAL, n_envs=2, n_steps=2, batch_size=2, ext_obs_dim=6, ext_action_dim=3, ext_discrete=1))
    for h, word in ((builtin, "cfg.norm_obs"), (ext, "host")):
        for call in (h.normalize_enable, h.normalize_config, h.normalize_get_stats, h.normalize_get_original, h.normalize_get_returns, lambda: h.normalize_set_training(True)):
            with pytest.raises(pkg.DrilError) as e:
                call()
            assert e.value.code == capi.ERR_UNSUPPORTED and word in str(e.value), str(e.value)
    h = mk(pkg, cos["reacher3"], 4, 2)
    for call in (h.normalize_config, h.normalize_get_stats, h.normalize_get_original, h.normalize_get_returns, lambda: h.normalize_set_training(True),
                 lambda: h.normalize_set_stats(np.zeros(12), np.ones(12), 0, 0, 1, 0)):
        with pytest.raises(pkg.DrilError) as e:
            call()
        assert e.value.code == capi.ERR_NOT_INITIALISED and "dril_normalize_enable" in str(e.value)
    h.normalize_enable(False)                                                            # off when off: nothing to do
    for bad in (dict(clip_obs=-1.0), dict(clip_reward=-0.5), dict(epsilon=-1e-3), dict(clip_obs=float("nan"))):
        with pytest.raises(pkg.DrilError) as e:
            h.normalize_enable(**bad)
        assert e.value.code == capi.ERR_INVALID_ARG
    with pytest.raises(TypeError):
        h.normalize_enable(clip=3)
    h.normalize_enable()
    c = capi.DrilNormalizeConfig()
    assert lib.dril_normalize_get_config(h._h, C.byref(c)) == capi.OK
    assert (c.training, c.norm_obs, c.norm_reward, c.clip_obs, c.clip_reward, c.gamma, c.epsilon) == (1, 1, 1, 10.0, 10.0, F(0.99), F(1e-8))
    assert lib.dril_normalize_get_config(h._h, None) == capi.ERR_INVALID_ARG
    with pytest.raises(pkg.DrilError) as e:
        h.normalize_set_stats(np.zeros(12), np.ones(12), -1, 0, 1, 0)
    assert e.value.code == capi.ERR_INVALID_ARG
    assert lib.dril_normalize_get_original(h._h, None, None) == capi.ERR_INVALID_ARG and lib.dril_normalize_get_returns(h._h, None) == capi.ERR_INVALID_ARG
    with pytest.raises(pkg.DrilError) as e:                                              # the pinned refusals point to the verb / the keyword
        pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=4, n_steps=2, batch_size=8, norm_obs=1), env_module=cos["reacher3"])
    assert e.value.code == capi.ERR_UNSUPPORTED and "NormalizeWrapperEnv" in str(e.value) and "dril_normalize_enable" in str(e.value)
    with pytest.raises(pkg.DrilError) as e:
        pkg.NormalizeWrapperEnv(pkg.DeviceModuleEnv(cos["reacher3"], 4))
    assert e.value.code == capi.ERR_UNSUPPORTED and "NormalizeWrapperEnv" in str(e.value) and "normalize=" in str(e.value)
    with pytest.raises(TypeError):
        pkg.DeviceModuleEnv(cos["reacher3"], 4, normalize=dict(clip=1.0))
