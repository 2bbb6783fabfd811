"""GPU (-m gpu): the fused rollout of a device env plug-in (include/device/dril_env_rollout.h, dril_rollout_fused_enable) — one launch per PPO collection.

Checkers: (1) the CPU oracle's built-in CartPole / Pendulum / scaled Pendulum, which the *_fused_plugin twins restate, with the inputs, comparison and tolerances of
test_collect_rollout_matches_oracle; (2) the step-granular collection of the same code object (pinned by tests/test_gpu_env_plugin.py; another f32-equivalent
arithmetic of the nets), within the tolerances tests/test_gpu_external.py holds the generic kernels to; (3) evaluate_actions on the stored rows; (4) the kernel
against itself: determinism, batch invariance, ragged tiles, continuation; (5) the env verbs of a second handle driven with the recorded actions.
Nothing here tries to make the device fault: every refusal is a host-side check made before anything is launched."""
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

import fused_rollout_helpers as F
from test_gpu_env_plugin import _reacher_step

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ENVS = ROOT / "examples" / "envs"
ALL_BUFS = range(10)
ROW_BUFS = (F.BUF_OBSERVATIONS, F.BUF_ACTIONS, F.BUF_REWARDS, F.BUF_FLAGS, F.BUF_LOGPROBS, F.BUF_VALUES, F.BUF_BOOTSTRAP)


def _co(name):
    p = ENVS / f"{name}_plugin.hsaco"
    assert p.exists(), f"{p}: built by the default target of dril.jl_amd/csrc/Makefile"
    return p


def _cfg(pkg, kind, **kw):
    c = pkg._capi.default_config(kind)
    hidden = kw.pop("hidden", None)
    for k, v in kw.items():
        setattr(c, k, v)
    if hidden is not None:
        c.n_hidden = len(hidden)
        for i, w in enumerate(hidden):
            c.hidden[i] = w
    return c


def _params(P, seed, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(P) * scale).astype(np.float32)


def _fused(pkg, name, **kw):
    h = pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, **kw), env_module=_co(name))
    h.rollout_fused_enable(True)
    info = h.rollout_fused_info()
    assert info["available"] and info["enabled"] and info["reason"] == "" and (info["tile"], info["threads"], info["max_width"]) == (16, 256, 256)
    return h


# ---- 1 / 6: against the CPU oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,E,T,L,fixed,scaling", [(*c, False) for c in F.ORACLE_CASES] + [("pendulum", 2, 40, 30, 12, False, True)])
def test_fused_collection_matches_the_oracle(pkg, oracle_mod, name, kind, E, T, L, fixed, scaling):
    """every buffer field of a fused collection against the trajectory-based oracle of the built-in kind the twin restates (kind 2: ScalingWrapperEnv(Pendulum),
    through dril_scaling_enable and dril_env_plugin_rollout_scaled); injected noise and the shared Philox stream, two collections without a reset"""
    kw = dict(n_envs=E, n_steps=T, episode_len=L, batch_size=max(2, (E * T) // 4), epochs=2, fixed_length_episodes=int(fixed))
    cfg = _cfg(pkg, kind, **kw)

    def make():
        h = pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, **kw), env_module=_co(f"{name}_fused"))
        if scaling:
            h.scaling_enable(True)
        h.rollout_fused_enable(True)
        return h
    h = F.compare_with_oracle(make, oracle_mod, cfg, lambda h: h.collect_rollout(), f"fused {name} kind={kind} E={E}")
    assert h.rollout_fused_info()["last_collection_launches"] == 1


# ---- 2: fused against step-granular on one code object --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,activation", [((64, 64), 0), ((128, 128, 128), 6)])
def test_fused_matches_the_step_granular_collection(pkg, hidden, activation):
    """reacher3, E 256 x T 40, L 13; injected noise, then the Philox stream.  The step-granular collection is the yardstick.  Envs whose flags differ anywhere are left
    out: at most 2 % of the envs, and for each the first differing step must be a termination whose position is within 1e-5 of the +-2 boundary."""
    capi = pkg._capi
    E, T, L = 256, 40, 13
    kw = dict(n_envs=E, n_steps=T, batch_size=E * T // 2, epochs=2, seed=7, episode_len=L, hidden=hidden, activation=activation)
    saw_term = False
    for inject in (True, False):
        ref = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, **kw), env_module=_co("reacher3_fused"))
        fus = _fused(pkg, "reacher3_fused", **kw)
        assert not ref.rollout_fused_info()["enabled"]
        flat = _params(ref.P, 5, 0.3)
        for h in (ref, fus):
            h.set_params(flat); h.env_reset(11)
            st, sc = h.env_get_state()
            st[: E // 8, 0] = 1.9; st[: E // 8, 3] = 1.0                   # an eighth of the envs starts on its way out of |p| <= 2: terminations
            h.env_set_state(st, sc)
            if inject:
                h.set_noise(np.random.default_rng(2).standard_normal((E * T, 3)).astype(np.float32))
            h.collect_rollout()
        ff, fr = fus.buffer(capi.BUF_FLAGS).reshape(T, E), ref.buffer(capi.BUF_FLAGS).reshape(T, E)
        assert (fr & 2).any()
        saw_term |= bool((fr & 1).any())
        same = (ff == fr).all(axis=0)
        assert (~same).mean() <= 0.02, f"{(~same).sum()} of {E} envs differ in their flags"
        obs_f, act_f = fus.buffer(capi.BUF_OBSERVATIONS).reshape(T, E, 12), fus.buffer(capi.BUF_ACTIONS).reshape(T, E, 3)
        for e in np.flatnonzero(~same):
            t = int(np.flatnonzero(ff[:, e] != fr[:, e])[0])
            assert (ff[t, e] ^ fr[t, e]) == 1, (e, t, ff[t, e], fr[t, e])                          # a termination on one side only
            pos = _reacher_step(obs_f[t, e:e + 1, :9], act_f[t, e:e + 1])[0][0, :3]
            assert np.abs(np.abs(pos) - 2).min() < 1e-5, (e, t, pos)
        for which, tol, width in ((capi.BUF_OBSERVATIONS, 2e-5, 12), (capi.BUF_VALUES, 5e-5, 1), (capi.BUF_LOGPROBS, 3e-4, 1), (capi.BUF_REWARDS, 1e-4, 1),
                                  (capi.BUF_ADVANTAGES, 1e-3, 1), (capi.BUF_RETURNS, 1e-3, 1)):
            a, b = fus.buffer(which).reshape(T, E, width)[:, same], ref.buffer(which).reshape(T, E, width)[:, same]
            print(f"[fused vs step-granular {hidden}] inject={inject} buffer {which}: max |diff| {np.abs(a - b).max():.3e}")
            np.testing.assert_allclose(a, b, atol=tol, rtol=tol, err_msg=f"buffer {which}")
        tr = ((fr & 2) != 0) & same[None, :]
        np.testing.assert_allclose(fus.buffer(capi.BUF_BOOTSTRAP).reshape(T, E)[tr], ref.buffer(capi.BUF_BOOTSTRAP).reshape(T, E)[tr], atol=3e-4, rtol=3e-4)
        live = same & (fr[T - 1] == 0)
        np.testing.assert_allclose(fus.buffer(capi.BUF_LAST_VALUES)[live], ref.buffer(capi.BUF_LAST_VALUES)[live], atol=5e-5, rtol=5e-5)
        # everything that is not floating-point arithmetic of the nets: counters
        assert np.array_equal(fus.env_get_state()[1][same], ref.env_get_state()[1][same])
    assert saw_term


# ---- 3: the stored rows against evaluate_actions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tol_lp", [("cartpole_fused", 1e-4), ("reacher3_fused", 3e-4)])
def test_stored_values_and_logprobs_equal_evaluate_actions(pkg, name, tol_lp):
    capi = pkg._capi
    h = _fused(pkg, name, n_envs=48, n_steps=20, batch_size=480, episode_len=7)
    h.set_params(_params(h.P, 3, 0.3)); h.env_reset(2); h.collect_rollout()
    val, lp, _ = h.evaluate_actions(h.buffer(capi.BUF_OBSERVATIONS), h.buffer(capi.BUF_ACTIONS))       # the generic kernels: another arithmetic
    np.testing.assert_allclose(val, h.buffer(capi.BUF_VALUES), atol=5e-5, rtol=5e-5)
    np.testing.assert_allclose(lp, h.buffer(capi.BUF_LOGPROBS), atol=tol_lp, rtol=tol_lp)


# ---- 4: the kernel against itself ------------------------------------------------------------------------------------------------------------------------
def test_determinism_batch_invariance_ragged_tiles_and_continuation(pkg):
    capi = pkg._capi
    T, L = 12, 5
    kw = dict(n_steps=T, batch_size=16 * T, epochs=1, episode_len=L, seed=9, monitor_window=100)
    mk = lambda E, **extra: _fused(pkg, "reacher3_fused", n_envs=E, **{**kw, **extra})
    a, b = mk(37), mk(37)                                                     # 37 = two full tiles and a ragged one of five envs
    flat = _params(a.P, 2, 0.2)
    for h in (a, b):
        h.set_params(flat); h.env_reset(21); h.collect_rollout()
    for which in ALL_BUFS:
        assert np.array_equal(a.buffer(which), b.buffer(which)), which       # two fused collections from the same seed: all ten buffers
    assert np.isfinite(a.buffer(capi.BUF_ADVANTAGES)).all() and (a.buffer(capi.BUF_FLAGS) & 2).any()
    # env e's rows are the same bits whatever E is and whichever tile e falls into: E = 1, and envs [16, 24) on their own (seed0 = seed + first env)
    for lo, n in ((0, 1), (16, 8), (32, 5)):
        p = mk(n); p.set_params(flat); p.env_reset(21 + lo); p.collect_rollout()
        for which, width in ((capi.BUF_OBSERVATIONS, 12), (capi.BUF_ACTIONS, 3), (capi.BUF_REWARDS, 1), (capi.BUF_FLAGS, 1), (capi.BUF_LOGPROBS, 1), (capi.BUF_VALUES, 1), (capi.BUF_BOOTSTRAP, 1)):
            assert np.array_equal(p.buffer(which).reshape(T, n, width), a.buffer(which).reshape(T, 37, width)[:, lo:lo + n]), (lo, n, which)
        assert np.array_equal(p.buffer(capi.BUF_LAST_VALUES), a.buffer(capi.BUF_LAST_VALUES)[lo:lo + n])
    # a second collection without a reset continues the first: rows [T, 2T) of one collection over 2T steps
    first = {w: a.buffer(w) for w in ROW_BUFS}
    a.collect_rollout()
    both = mk(37, n_steps=2 * T, batch_size=37 * 2 * T); both.set_params(flat); both.env_reset(21); both.collect_rollout()
    for which in ROW_BUFS:
        whole = both.buffer(which)
        rows = whole.reshape(2 * T, -1)
        assert np.array_equal(rows[:T].reshape(-1), first[which].reshape(-1)) and np.array_equal(rows[T:].reshape(-1), a.buffer(which).reshape(-1)), which
    assert np.array_equal(both.buffer(capi.BUF_LAST_VALUES), a.buffer(capi.BUF_LAST_VALUES))
    assert np.array_equal(both.env_get_state()[0], a.env_get_state()[0]) and np.array_equal(both.env_get_state()[1], a.env_get_state()[1])


def test_two_loopback_ranks_reproduce_a_single_handle_in_every_field(pkg):
    """world_size 2: rank r's envs are envs [rE, (r+1)E) of a single handle over 2E envs — the construction of test_two_loopback_ranks_own_the_global_env_indices,
    now including values, log-probabilities and bootstrap values, bit for bit"""
    capi = pkg._capi
    E, T = 8, 12
    kw = dict(n_steps=T, batch_size=2 * E * T, epochs=1, episode_len=5, seed=9)
    one = _fused(pkg, "reacher3_fused", n_envs=2 * E, **kw)
    hs = [_fused(pkg, "reacher3_fused", n_envs=E, rank=r, world_size=2, **kw) for r in range(2)]
    pkg.Handle.comm_loopback(hs)
    flat = _params(one.P, 2, 0.2)
    one.set_params(flat); one.env_reset(21); one.collect_rollout()
    fields = ((capi.BUF_OBSERVATIONS, 12), (capi.BUF_ACTIONS, 3), (capi.BUF_REWARDS, 1), (capi.BUF_FLAGS, 1), (capi.BUF_LOGPROBS, 1), (capi.BUF_VALUES, 1), (capi.BUF_BOOTSTRAP, 1))
    out, err = [None, None], [None, None]

    def run(r):
        try:
            hs[r].set_params(flat); hs[r].env_reset(21); hs[r].collect_rollout()
            out[r] = {w: hs[r].buffer(w) for w, _ in fields}
        except BaseException as ex:   # noqa: BLE001 - re-raised below
            err[r] = ex
    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in ts]; [t.join() for t in ts]
    for ex in err:
        if ex is not None:
            raise ex
    for w, width in fields:
        whole = one.buffer(w).reshape(T, 2 * E, width)
        for r in range(2):
            assert np.array_equal(out[r][w].reshape(T, E, width), whole[:, r * E:(r + 1) * E]), (w, r)


# ---- 5: monitor, evaluate_agent and the env verbs after a fused collection --------------------------------------------------------------------------
def test_monitor_evaluate_and_env_verbs_after_a_fused_collection(pkg):
    capi = pkg._capi
    E, T, L = 16, 64, 10
    kw = dict(n_envs=E, n_steps=T, batch_size=E * T // 2, epochs=2, seed=7, episode_len=L, monitor_window=1000)
    a = _fused(pkg, "reacher3_fused", **kw)
    b = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, **kw), env_module=_co("reacher3_fused"))
    flat = _params(a.P, 1, 0.2)
    for h in (a, b):
        h.set_params(flat); h.env_reset(4)
    a.collect_rollout()
    rew, fl = a.buffer(capi.BUF_REWARDS).reshape(T, E), a.buffer(capi.BUF_FLAGS).reshape(T, E)
    rets, lens = [], []
    cur_r, cur_l = np.zeros(E, np.float32), np.zeros(E, np.int64)
    for t in range(T):
        cur_r += rew[t]; cur_l += 1
        for e in np.nonzero(fl[t])[0]:
            rets.append(cur_r[e]); lens.append(cur_l[e]); cur_r[e] = 0; cur_l[e] = 0
    r_mean, l_mean, n = a.monitor_stats()
    assert n == len(rets) > E and l_mean == pytest.approx(np.mean(lens)) and r_mean == pytest.approx(np.mean(rets), rel=1e-5)
    # the step-granular env verbs of a second handle, driven with the recorded actions, end where the fused collection ended
    act, obs = a.buffer(capi.BUF_ACTIONS).reshape(T, E, 3), a.buffer(capi.BUF_OBSERVATIONS).reshape(T, E, 12)
    for t in range(T):
        assert np.array_equal(b.env_observe(), obs[t]), t
        rb, tb, ub, _ = b.env_step(act[t])
        assert np.array_equal(rb, rew[t]) and np.array_equal(tb, (fl[t] & 1) != 0) and np.array_equal(ub, (fl[t] & 2) != 0), t
    (sa, ca), (sb, cb) = a.env_get_state(), b.env_get_state()
    assert np.array_equal(sa, sb) and np.array_equal(ca, cb) and np.array_equal(a.env_observe(), b.env_observe())
    (ra, la, na), (rb_, lb, nb) = a.monitor_stats(), b.monitor_stats()
    assert na == nb and la == pytest.approx(lb) and ra == pytest.approx(rb_, rel=1e-6)
    ea, eb = a.evaluate_agent(12, True), b.evaluate_agent(12, True)          # dril_evaluate_agent stays step-granular
    assert np.array_equal(ea[1], eb[1]) and np.array_equal(ea[2], eb[2]) and ea[0]["n_steps"] == eb[0]["n_steps"]
    step = np.random.default_rng(0).uniform(-1.5, 1.5, (E, 3)).astype(np.float32)
    (r1, t1, u1, o1), (r2, t2, u2, o2) = a.env_step(step), b.env_step(step)
    assert np.array_equal(r1, r2) and np.array_equal(t1, t2) and np.array_equal(u1, u2) and np.array_equal(o1[u1], o2[u2])
    # a step-granular collection after a fused one, and a fused one after it, continue from the same envs
    a.rollout_fused_enable(False); a.collect_rollout(); assert a.rollout_fused_info()["last_collection_launches"] > T
    a.rollout_fused_enable(True); a.collect_rollout(); assert a.rollout_fused_info()["last_collection_launches"] <= 3
    assert np.isfinite(a.buffer(capi.BUF_ADVANTAGES)).all()


# ---- 7: launches ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_launch_count_of_a_fused_collection_does_not_depend_on_T(pkg):
    """dril_profile_launches(DRIL_K_ROLLOUT) counts the event brackets of the rollout class — one per collection on either path — so the count that can grow with T is
    dril_rollout_fused_info's last_collection_launches (the launch calls the collection enqueued): both are asserted for the fused path, the second for the step-granular one"""
    capi = pkg._capi
    name = capi.load_library().dril_kernel_name(capi.K_ROLLOUT).decode()
    counts = {}
    for fused in (True, False):
        for T in (8, 64):
            h = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=32, n_steps=T, batch_size=32 * T, episode_len=5, profile_events=1, monitor_window=10), env_module=_co("reacher3_fused"))
            h.rollout_fused_enable(fused)
            h.set_params(_params(h.P, 0)); h.env_reset(1); h.profile_reset(); h.collect_rollout()
            counts[fused, T] = (h.profile()[name]["launches"], h.rollout_fused_info()["last_collection_launches"])
    print("[launches] (event brackets, launch calls):", counts)
    assert counts[True, 8] == counts[True, 64] and max(counts[True, 8]) <= 3 and min(counts[True, 8]) >= 1
    assert counts[False, 64][1] > counts[False, 8][1] >= 6 * 8 and counts[False, 64][1] >= 6 * 64


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_status_and_message(pkg, tmp_path):
    capi = pkg._capi
    small = dict(n_envs=4, n_steps=2, batch_size=8)

    def refused(call, *words):
        with pytest.raises(pkg.DrilError) as e:
            call()
        assert e.value.code == capi.ERR_UNSUPPORTED and all(w in str(e.value) for w in words), str(e.value)
    builtin = pkg.Handle(_cfg(pkg, 0, **small))
    refused(lambda: builtin.rollout_fused_enable(True), "device env plug-in")
    assert not builtin.rollout_fused_info()["available"]
    plain = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, **small), env_module=_co("reacher3"))           # a code object without the kernel
    refused(lambda: plain.rollout_fused_enable(True), "DRIL_ENV_PLUGIN_ROLLOUT(Env)", "rebuild")
    info = plain.rollout_fused_info()
    assert not info["available"] and not info["enabled"] and "DRIL_ENV_PLUGIN_ROLLOUT" in info["reason"] and info["tile"] == 0
    plain.rollout_fused_enable(False)                                                              # switching off what is off is no error
    plain.set_params(_params(plain.P, 0)); plain.env_reset(1); plain.collect_rollout()             # ... and the handle is a healthy step-granular one
    assert np.isfinite(plain.buffer(capi.BUF_ADVANTAGES)).all()
    other = tmp_path / "rollout_abi7.hsaco"                                                        # another rollout ABI number: the handle is created, the fused path is not available
    subprocess.run(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "--no-gpu-bundle-output", "-O3", "-fno-slp-vectorize", "-std=c++17", "-DDRIL_ENV_ROLLOUT_ABI=7u",
                    "-I", str(ROOT / "include"), str(ENVS / "reacher3_fused_plugin.hip"), "-o", str(other)], check=True)
    h7 = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, **small), env_module=other)
    refused(lambda: h7.rollout_fused_enable(True), "fused rollout ABI 7", "rebuild")
    assert not h7.rollout_fused_info()["available"]
    h7.set_params(_params(h7.P, 0)); h7.env_reset(1); h7.collect_rollout()
    assert np.isfinite(h7.buffer(capi.BUF_ADVANTAGES)).all() and h7.rollout_fused_info()["last_collection_launches"] > 2
    wide = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, hidden=(64, 320), **small), env_module=_co("reacher3_fused"))
    refused(lambda: wide.rollout_fused_enable(True), "hidden layer 2 is 320 wide", "DRIL_ENV_ROLLOUT_MAX_WIDTH=320")
    assert not wide.rollout_fused_info()["enabled"]
    norm = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, **small), env_module=_co("reacher3_fused"))
    norm.normalize_enable()
    refused(lambda: norm.rollout_fused_enable(True), "NormalizeWrapperEnv", "dril_normalize_enable")
    assert not norm.rollout_fused_info()["enabled"]
    fus = _fused(pkg, "reacher3_fused", **small)
    refused(lambda: fus.normalize_enable(), "dril_rollout_fused_enable(h, 0)")
    assert fus.rollout_fused_info()["enabled"]                                                     # a refused handle stays as it was
    fus.set_params(_params(fus.P, 0)); fus.env_reset(1); fus.collect_rollout()
    assert np.isfinite(fus.buffer(capi.BUF_ADVANTAGES)).all()
    with pytest.raises(pkg.DrilError) as e:
        pkg.DeviceModuleEnv(_co("reacher3"), 4, fused_rollout=True)._h()
    assert e.value.code == capi.ERR_UNSUPPORTED and "DRIL_ENV_PLUGIN_ROLLOUT" in str(e.value)


# ---- 9 / 10: training ---------------------------------------------------------------------------------------------------------------------------------------
def test_reacher3_training_with_the_fused_rollout_improves_the_episode_return(pkg):
    """the configuration of test_reacher3_training_improves_the_episode_return with fused_rollout=True; the margin asked for is that test's (100)"""
    env = pkg.MonitorWrapperEnv(pkg.DeviceModuleEnv(_co("reacher3_fused"), 64, seed=0, fused_rollout=True), stats_window=64)
    alg = pkg.PPO(n_steps=100, batch_size=1600, epochs=10, learning_rate=1e-3)
    agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space()), alg, seed=0)
    seen = []

    class Log:
        def on_rollout_end(self, loc):
            seen.append(loc["env"].handle.monitor_stats()[0]); return True
    pkg.train_(agent, env, alg, 64 * 100 * 40, callbacks=[Log()])
    info = env.handle.rollout_fused_info()
    assert info["enabled"] and info["last_collection_launches"] <= 3
    print(f"[fused training] mean episode return {seen[0]:.1f} -> {seen[-1]:.1f}")
    assert len(seen) == 40 and np.isfinite(seen).all()
    assert seen[-1] > seen[0] + 100.0, (seen[0], seen[-1])


def test_dril_train_equals_collect_and_update_called_one_after_the_other(pkg):
    E, T = 32, 16
    kw = dict(n_envs=E, n_steps=T, batch_size=128, epochs=2, episode_len=9, seed=4)
    a, b = _fused(pkg, "reacher3_fused", **kw), _fused(pkg, "reacher3_fused", **kw)
    flat = _params(a.P, 1, 0.1)
    for h in (a, b):
        h.set_params(flat); h.env_reset(4)
    sa, _ = a.train(3 * E * T + 5)
    sb = []
    for _ in range(3):
        b.collect_rollout(); sb.append(b.ppo_update())
    assert len(sa) == 3 and a.rollout_fused_info()["last_collection_launches"] == 1
    for x, y in zip(sa, sb):
        assert x.n_updates == y.n_updates == 2 * 4 and x.loss == pytest.approx(y.loss, rel=1e-6, abs=1e-8)
    np.testing.assert_allclose(a.get_params(), b.get_params(), rtol=1e-6, atol=1e-8)
    assert not np.array_equal(a.get_params(), flat)
    for which in ALL_BUFS:
        assert np.array_equal(a.buffer(which), b.buffer(which)), which
