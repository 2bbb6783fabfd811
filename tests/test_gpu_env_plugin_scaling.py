"""GPU (-m gpu): the declared observation space of a device env plug-in and ScalingWrapperEnv on it (dril_scaling_enable / dril_sac_scaling_enable): the env side
launches the plug-in's own _scaled kernels where it launched observe / step.

Checkers: (1) the built-in DRIL_ENV_PENDULUM_SCALED, which the pendulum example under the wrapper restates, bit for bit — env verbs, every rollout buffer field, two
PPO iterations on the generic kernels, SAC collection into the ring; (2) a second, unwrapped handle of the same plug-in in lock step plus the NumPy float32
formulas of scalingWrapperEnv.jl (reacher3); (3) tests/sac_normalize_ref.py-style NumPy moments for NormalizeWrapperEnv outside the wrapper.
Each test is one bounded run; a refused call never launches anything of the module's optional kernels."""
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ENVS = ROOT / "examples" / "envs"
ALL_BUFS = range(10)
F = np.float32


def _co(name):
    p = ENVS / f"{name}_plugin.hsaco"
    assert p.exists(), f"{p}: built by the default target of dril.jl_amd/csrc/Makefile"
    return p


def _cfg(pkg, kind, **kw):
    c = pkg._capi.default_config(kind)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _stats(s):
    return tuple(getattr(s, n) for n, _ in type(s)._fields_)


def scale(x, lo, hi):       # scale! scalingWrapperEnv.jl:71-74, every operation in float32
    return ((x.astype(F) - lo) * (F(2) / (hi - lo)) - F(1)).astype(F)


def unscale(x, lo, hi):     # unscale! :76-79
    return ((x.astype(F) + F(1)) / (F(2) / (hi - lo)) + lo).astype(F)


def test_the_examples_report_their_observation_space(pkg):
    c, p, r = (pkg.describe_env_module(_co(n)) for n in ("cartpole", "pendulum", "reacher3"))
    assert p["obs_declared"] and p["obs_low"].tolist() == [-1.0, -1.0, -8.0] and p["obs_high"].tolist() == [1.0, 1.0, 8.0]
    assert r["obs_declared"] and r["obs_low"].shape == (12,) and np.isfinite(r["obs_low"]).all() and (r["obs_low"] < r["obs_high"]).all()
    assert c["obs_declared"] and np.isinf(c["obs_low"][[1, 3]]).all() and np.isinf(c["obs_high"][[1, 3]]).all() and F(c["obs_high"][0]) == F(4.8)
    h = pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, n_envs=4, n_steps=2, batch_size=8), env_module=_co("pendulum"))
    sp = h.env_module_obs_space()
    assert sp["declared"] and sp["low"].tolist() == [-1.0, -1.0, -8.0]
    a = h.agent_spaces()
    assert not a["scaling"] and a["obs_high"].tolist() == [1.0, 1.0, 8.0] and a["action_low"].tolist() == [-2.0]
    h.scaling_enable(True)
    a = h.agent_spaces()
    assert a["scaling"] and a["obs_low"].tolist() == [-1.0] * 3 and a["obs_high"].tolist() == [1.0] * 3 and (a["action_low"].tolist(), a["action_high"].tolist()) == ([-1.0], [1.0])
    assert h.env_module_info()["action_low"].tolist() == [-2.0] and h.env_module_obs_space()["high"].tolist() == [1.0, 1.0, 8.0]   # the env's own, wrapper or not


def test_scaled_pendulum_plugin_env_verbs_equal_the_builtin_scaled_kind_to_the_bit(pkg):
    capi = pkg._capi
    E, L = 32, 60
    b = pkg.Handle(_cfg(pkg, capi.ENV_PENDULUM_SCALED, n_envs=E, n_steps=2, batch_size=E, episode_len=L))
    m = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=E, n_steps=2, batch_size=E, episode_len=L), env_module=_co("pendulum"))
    m.scaling_enable(True)
    b.env_reset(5); m.env_reset(5)
    rng = np.random.default_rng(0)
    n_trunc = 0
    for t in range(320):
        ob = b.env_observe()
        assert np.array_equal(ob, m.env_observe()), t
        assert (np.abs(ob) <= 1.0).all()
        act = rng.uniform(-1.7, 1.7, (E, 1)).astype(F)                  # beyond Box(-1, 1): the ClampAdapter of the wrapper's action space
        rb, tb, ub, tob = b.env_step(act); rm, tm, um, tom = m.env_step(act)
        assert np.array_equal(rb, rm) and np.array_equal(tb, tm) and np.array_equal(ub, um), t
        assert np.array_equal(tob[ub], tom[um]), t                      # the terminal observation is scaled on both sides
        sb, cb = b.env_get_state(); sm, cm = m.env_get_state()
        assert np.array_equal(sb, sm) and np.array_equal(cb, cm), t
        n_trunc += int(ub.sum())
    assert n_trunc > 0


def test_scaled_twin_collection_and_update_equal_the_builtin_scaled_kind_on_the_generic_kernels(pkg, monkeypatch):
    capi = pkg._capi
    E, T = 64, 24
    kw = dict(n_envs=E, n_steps=T, batch_size=E * T // 2, epochs=2, episode_len=9, seed=3, hidden1=48, hidden2=80, monitor_window=50, profile_events=1)
    monkeypatch.setenv("DRIL_FORCE_GENERIC", "1")
    b = pkg.Handle(_cfg(pkg, capi.ENV_PENDULUM_SCALED, **kw))
    monkeypatch.delenv("DRIL_FORCE_GENERIC")
    m = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, **kw), env_module=_co("pendulum"))
    plain = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, **kw), env_module=_co("pendulum"))
    m.scaling_enable(True)
    assert m.P == b.P
    flat = (np.random.default_rng(3).standard_normal(b.P) * 0.4).astype(F)
    for h in (b, m, plain):
        h.set_params(flat); h.env_reset(11)
    for it in range(2):
        rng = np.random.default_rng(10 + it)
        nz = (rng.standard_normal((E * T, 1)) * 2).astype(F)
        perm = np.stack([rng.permutation(E * T) for _ in range(2)]).astype(np.int64)
        for h in (b, m, plain):
            h.profile_reset(); h.set_noise(nz); h.collect_rollout()
        for which in ALL_BUFS:
            assert np.array_equal(b.buffer(which), m.buffer(which)), (it, which)
        assert (m.buffer(capi.BUF_FLAGS) & 2).any() and (np.abs(m.buffer(capi.BUF_OBSERVATIONS)) <= 1.0).all()
        assert (np.abs(m.buffer(capi.BUF_ACTIONS)) > 1.0).any()         # the buffer keeps the raw action
        assert b.monitor_stats() == m.monitor_stats()
        # no launch is added per env step: the collection of the wrapped handle counts what the unwrapped one counts
        lm, lp = ({k: v["launches"] for k, v in h.profile().items()} for h in (m, plain))
        assert lm == lp and lm[pkg._capi.load_library().dril_kernel_name(capi.K_ROLLOUT).decode()] > 0
        for h in (b, m):
            h.set_permutation(perm)
        sb, sm = b.ppo_update(), m.ppo_update()
        assert _stats(sb) == _stats(sm) and sb.n_updates == 4
        assert np.array_equal(b.get_params(), m.get_params())
    assert not np.array_equal(plain.buffer(capi.BUF_OBSERVATIONS), m.buffer(capi.BUF_OBSERVATIONS))
    ev_b, ev_m = b.evaluate_agent(4, True), m.evaluate_agent(4, True)   # dril_evaluate_agent steps the wrapped envs
    assert ev_b[0]["mean_reward"] == ev_m[0]["mean_reward"] and ev_b[0]["n_steps"] == ev_m[0]["n_steps"]


def test_reacher3_scaled_kernels_follow_the_unwrapped_plugin_and_the_reference_formulas(pkg):
    capi = pkg._capi
    E, L = 48, 45
    mk = lambda: pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=E, n_steps=2, batch_size=E, episode_len=L), env_module=_co("reacher3"))
    w, p = mk(), mk()
    w.scaling_enable(True)
    sp = w.env_module_obs_space(); lo, hi = sp["low"], sp["high"]
    info = w.env_module_info(); alo, ahi = info["action_low"], info["action_high"]
    w.env_reset(9); p.env_reset(9)
    # (the device contracts scale!'s multiply and subtract into one fused operation, NumPy rounds twice: observations to an ulp of the unit box, all else to the bit)
    close = lambda got, want: np.testing.assert_allclose(got, want, rtol=0, atol=3e-7)
    rng = np.random.default_rng(1)
    n_term = n_trunc = 0
    for t in range(200):
        close(w.env_observe(), scale(p.env_observe(), lo, hi))
        act = rng.uniform(-1.6, 1.6, (E, 3)).astype(F)
        act[: E // 3] = F(1.5)                                          # a third of the envs leaves |p| <= 2: terminations
        rw, tw, uw, ow = w.env_step(act)
        rp, tp, up, op = p.env_step(unscale(np.clip(act, F(-1), F(1)), alo, ahi))
        assert np.array_equal(rw, rp) and np.array_equal(tw, tp) and np.array_equal(uw, up), t
        close(ow[uw], scale(op[up], lo, hi))
        (sw, cw), (s2, c2) = w.env_get_state(), p.env_get_state()
        assert np.array_equal(sw, s2) and np.array_equal(cw, c2), t
        n_term += int(tw.sum()); n_trunc += int(uw.sum())
    assert n_term > 0 and n_trunc > 0


def test_normalize_wrapper_sits_outside_the_scaling_wrapper(pkg):
    """NormalizeWrapperEnv(ScalingWrapperEnv(env)): the originals the wrapper keeps are the SCALED observations, what it hands out is their normalisation
    with its own statistics, and those statistics are moments of scaled observations"""
    capi = pkg._capi
    E = 40
    mk = lambda: pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=E, n_steps=2, batch_size=E, episode_len=30), env_module=_co("reacher3"))
    n, s = mk(), mk()
    for h in (n, s):
        h.scaling_enable(True)
    n.normalize_enable(norm_reward=False)
    n.env_reset(4); s.env_reset(4)
    seen = []
    rng = np.random.default_rng(2)
    for t in range(25):
        act = rng.uniform(-1, 1, (E, 3)).astype(F)
        n.env_step(act); s.env_step(act)
        got, raw = n.env_observe(), s.env_observe()                     # observe(::NormalizeWrapperEnv): the batch enters the statistics, then is normalised with them
        seen.append(raw)
        assert np.array_equal(n.normalize_get_original()[0], raw), t    # get_original_obs: the scaled observation, to the bit
        st = n.normalize_get_stats()
        want = np.clip((raw - st["obs_mean"]) / np.sqrt(st["obs_var"] + 1e-8), -10, 10)
        np.testing.assert_allclose(got, want, rtol=2e-4, atol=2e-5)
    pooled = np.concatenate(seen).astype(np.float64)
    assert st["obs_count"] >= len(pooled) and (np.abs(st["obs_mean"]) < 1.0).all()
    np.testing.assert_allclose(st["obs_mean"], pooled.mean(0), rtol=0, atol=0.05)   # moments of observations in Box(-1, 1), not of positions up to 2.2


def test_sac_collection_under_the_wrapper_equals_the_builtin_scaled_kind(pkg, monkeypatch):
    from test_gpu_sac_env_plugin import assert_rings_equal, init_params, ring
    E, T_lim, steps, B, hidden = 8, 5, 11, 16, (32, 32)
    cap = 8 * E
    env = pkg.ScalingWrapperEnv(pkg.PendulumEnv(max_steps=T_lim))
    alg = pkg.SAC(batch_size=B, buffer_capacity=cap)
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=hidden)
    monkeypatch.setenv("DRIL_SAC_NO_FUSED_COLLECT", "1")               # the built-in on head -> step -> observe -> push
    b = pkg.SacHandle(pkg.make_sac_config(env, E, alg, layer, seed=7))
    monkeypatch.delenv("DRIL_SAC_NO_FUSED_COLLECT")
    info = pkg.describe_env_module(_co("pendulum"))
    menv = pkg.host.ModuleEnv(str(_co("pendulum")), info, T_lim, scaling=True)
    mlayer = pkg.SACLayer(menv.observation_space(), menv.action_space(), hidden_dims=hidden)
    m = pkg.SacHandle(pkg.make_sac_config(menv, E, alg, mlayer, seed=7), env_module=_co("pendulum"))
    m.scaling_enable(True)
    a = m.agent_spaces()
    assert a["scaling"] and (a["action_low"].tolist(), a["action_high"].tolist()) == ([-1.0], [1.0]) and m.env_module_info()["action_low"].tolist() == [-2.0]
    flat = init_params(pkg, layer)
    rng = np.random.default_rng(3)
    nz_rand, nz_pol = rng.random((2, E, 1)).astype(F), rng.normal(0, 1, (steps, E, 1)).astype(F)
    for x in (b, m):
        x.set_params(flat); x.env_reset(11)
        x.set_collect_noise(nz_rand); x.collect_rollout(2, True)       # the start phase: rand(action_space) of the WRAPPER's Box(-1, 1)
        x.set_collect_noise(nz_pol); x.collect_rollout(steps, False)
        assert x.replay_size() == cap
    rb, rm = ring(pkg, b), ring(pkg, m)
    assert rb["trunc"].sum() >= E and (np.abs(rm["obs"]) <= 1.0).all()
    assert_rings_equal(rb, rm)
    assert np.array_equal(b.env_observe(), m.env_observe())
    ev_b, ev_m = b.evaluate_agent(4, True, seed=5), m.evaluate_agent(4, True, seed=5)
    assert ev_b[0]["mean_reward"] == ev_m[0]["mean_reward"]


def test_refusals_say_what_to_do_and_leave_the_handle_as_it_was(pkg, tmp_path):
    import subprocess
    from test_env_plugin import GENCO
    from test_env_plugin_scaling import INFINITE, NO_SPACE, SRC
    capi = pkg._capi
    mk = lambda path: pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=4, n_steps=2, batch_size=8), env_module=path)

    def refused(h, code, *words):
        with pytest.raises(pkg.DrilError) as e:
            h.scaling_enable(True)
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)
    refused(pkg.Handle(_cfg(pkg, capi.ENV_PENDULUM, n_envs=4, n_steps=2, batch_size=8)), capi.ERR_UNSUPPORTED, "DRIL_ENV_PENDULUM_SCALED")
    refused(mk(_co("cartpole")), capi.ERR_UNSUPPORTED, "Discrete")
    for decl, words in ((NO_SPACE, ("declares no observation space", "obs_low[D]")), (INFINITE, ("observation dim 0", "finite"))):
        src = tmp_path / "walk.hip"; src.write_text(SRC % decl)
        co = tmp_path / f"walk{len(decl)}.hsaco"
        subprocess.run(GENCO + [str(src), "-o", str(co)], check=True)
        assert pkg.describe_env_module(co)["obs_declared"] == bool(decl)
        h = mk(co)
        refused(h, capi.ERR_UNSUPPORTED, *words)
        h.env_reset(1)                                                  # a refused handle is a healthy unwrapped one
        assert h.env_observe().shape == (4, 2) and not h.agent_spaces()["scaling"]
    h = mk(_co("pendulum"))
    h.env_reset(1)
    refused(h, capi.ERR_INVALID_ARG, "between create and the first env reset")
    assert not h.agent_spaces()["scaling"] and (np.abs(h.env_observe()[:, 2]) <= 1.0).all()
    with pytest.raises(pkg.DrilError):
        pkg.ScalingWrapperEnv(pkg.DeviceModuleEnv(_co("cartpole"), 4))


def test_python_wrapper_trains_ppo_and_sac_on_reacher3(pkg):
    env = pkg.ScalingWrapperEnv(pkg.DeviceModuleEnv(_co("reacher3"), 16, seed=3))
    assert isinstance(env, pkg.DeviceModuleEnv) and env.observation_space() == pkg.Box((-1.0,) * 12, (1.0,) * 12) and env.action_space() == pkg.Box((-1.0,) * 3, (1.0,) * 3)
    env2 = pkg.DeviceModuleEnv(_co("reacher3"), 16, seed=3, scaling=True)
    plain = pkg.DeviceModuleEnv(_co("reacher3"), 16, seed=3)
    assert env._bind_extra() == env2._bind_extra() != plain._bind_extra()
    obs, raw = np.stack(env.observe()), np.stack(plain.observe())
    assert np.allclose(obs, env.scale_observation(raw), rtol=0, atol=3e-7) and np.allclose(env.unscale_observation(obs), raw, atol=1e-5)
    alg = pkg.PPO(n_steps=32, batch_size=128, epochs=2)
    layer = pkg.ActorCriticLayer(env.observation_space(), env.action_space())
    agent = pkg.Agent(layer, alg, seed=0)
    pkg.train_(agent, env, alg, 16 * 32 * 2)
    assert env.handle.agent_spaces()["scaling"] and (np.abs(env.handle.buffer(pkg._capi.BUF_OBSERVATIONS)) <= 1.0 + 1e-6).all()
    salg = pkg.SAC(batch_size=32, buffer_capacity=2048, start_steps=64)
    sagent = pkg.SACAgent(pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(32, 32)), salg, seed=0)
    _, rb, *_ = pkg.sac_train_(sagent, env, salg, 16 * 12)
    assert rb.handle.agent_spaces()["scaling"] and (np.abs(rb.handle.replay(pkg._capi.RB_OBSERVATIONS)) <= 1.0 + 1e-6).all()
