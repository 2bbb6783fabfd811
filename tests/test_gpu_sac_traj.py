"""GPU (-m gpu): collect_trajectory of a SAC handle on the device (dril_sac_collect_trajectory, docs/sac.md "Trajectories"), every check through the C ABI /
pkg.SacHandle.

Checkers, none of which is the verb itself: (1) the replay ring of a twin handle after dril_sac_env_reset(seed) + dril_sac_collect_rollout — the draws of a
stochastic recording are the collection's, so observations, rewards, flags and the next_obs of truncated steps are compared BITWISE; (2) env_step of a PPO handle of
the same kind without wrappers, fed the recorded env actions (`replay` of tests/test_gpu_traj_device.py); (3) for the row neither can see, the observation after the
last step of a terminated episode: a fixed_length_episodes PPO twin stepped once from the recorded state, the kind's termination predicate, and for reacher3 the
NumPy twin of tests/test_env_plugin.py; (4) dril_sac_evaluate_agent on the same seed; (5) for what the call must NOT do, a twin that never recorded, bitwise.

Shapes: E = 37 (kEnvsPerBlock = 16: two full workgroups and a partial one), M in {1, 17, 37}, hidden (32, 32), plug-ins at E = 12.  Time limits of 9 - 20 steps,
except MountainCarContinuous, which needs about 80 steps of pumping to terminate: its limit is the median first-episode length of the 37 envs under a long limit
(taken from dril_sac_evaluate_agent), so that some recorded envs terminate before it and the others are truncated at it."""
import ctypes as C

import numpy as np
import pytest

from test_env_plugin import _reacher_obs, _reacher_step
from test_gpu_sac_env_plugin import _co, assert_rings_equal, init_params, make_module, ring, to_env
from test_gpu_sac_monitor_eval import constant_actor
from test_gpu_traj_device import bits, feature_policy, make as ppo_make, replay, same_trajs

pytestmark = pytest.mark.gpu
F = np.float32
E = 37
MS = (1, 17, 37)
EP = 12                                                                                # plug-ins
TERM, TRUNC, CUT = 1, 2, 4
SEED = 13
HID = (32, 32)


# ---- handles ---------------------------------------------------------------------------------------------------------------------------------------------------------
def sac(pkg, name, n, T_lim, act="relu", cap=4096, seed=7, B=16, **alg_kw):
    """-> (handle, layer): a built-in Box kind ("pendulum" 1, "pendulum_scaled" 2, "mcc" 4, "mcc_scaled" 7) or a plug-in ("reacher3", "pendulum_plugin[_scaled]")"""
    if name in ("reacher3", "pendulum_plugin", "pendulum_plugin_scaled"):
        h, layer, _ = make_module(pkg, _co("reacher3" if name == "reacher3" else "pendulum"), n, hidden=HID, B=B, cap=cap, seed=seed, max_steps=T_lim, act=act, **alg_kw)
        if name.endswith("_scaled"):
            h.scaling_enable(True)
        return h, layer
    env = {"pendulum": lambda: pkg.PendulumEnv(max_steps=T_lim), "mcc": lambda: pkg.MountainCarContinuousEnv(max_steps=T_lim),
           "pendulum_scaled": lambda: pkg.ScalingWrapperEnv(pkg.PendulumEnv(max_steps=T_lim)),
           "mcc_scaled": lambda: pkg.ScalingWrapperEnv(pkg.MountainCarContinuousEnv(max_steps=T_lim))}[name]()
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=HID, activation=act)
    return pkg.SacHandle(pkg.make_sac_config(env, n, pkg.SAC(batch_size=B, buffer_capacity=cap, **alg_kw), layer, seed=seed)), layer


def agent_box(h, name):
    """the agent-facing Box TanhScaleAdapter scales into"""
    b = F(2) if name in ("pendulum", "pendulum_plugin") else F(1)
    return np.full(h.A, -b, F), np.full(h.A, b, F)


def first_episodes(r):
    """per env of a [T][E] ring: the length of its first episode (every env finishes within the block: the time limit)"""
    done = (r["term"] | r["trunc"]).astype(bool)
    assert done.any(0).all()
    return done.argmax(0) + 1


def shaped(pkg, h, T, n):
    return {k: v.reshape(T, n, *v.shape[1:]) for k, v in ring(pkg, h).items()}


_PUMP = {}


def pump_limit(pkg):
    """MountainCarContinuous under the policy that pushes where the car moves (tanh layers: +-3 either way): the time limit at which terminated and truncated first
    episodes both occur among the 37 envs — the median first-episode length under a long limit, from dril_sac_evaluate_agent"""
    if "limit" not in _PUMP:
        probe, _ = sac(pkg, "mcc", E, 300, act="tanh")
        probe.set_params(feature_policy(probe, HID, 1, 100.0, (3.0,)))
        _, _, el = probe.evaluate_agent(E, True, seed=SEED)
        probe.close()
        assert el.max() < 2 * el.min()                                                  # the first E events are the envs' first episodes: no env finished twice
        lens = np.sort(el)
        _PUMP["limit"] = int(lens[len(lens) // 2])
        print(f"MountainCarContinuous first-episode lengths {lens.tolist()} -> time limit {_PUMP['limit']}")
        assert lens[0] < _PUMP["limit"] < 300
    return _PUMP["limit"]


def pump(pkg, n=E, **kw):
    h, layer = sac(pkg, "mcc", n, pump_limit(pkg), act="tanh", **kw)
    h.set_params(feature_policy(h, HID, 1, 100.0, (3.0,)))
    return h


# ---- 1: a stochastic recording equals the collection's ring ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,T", [("pendulum", E, 9), ("mcc", E, 20), ("reacher3", EP, 7)])
def test_stochastic_recording_equals_the_collections_ring(pkg, name, n, T):
    s = 77
    (h, layer), (twin, _) = sac(pkg, name, n, T), sac(pkg, name, n, T)
    flat = init_params(pkg, layer, scale_out=3.0)
    h.set_params(flat); twin.set_params(flat)
    trajs, lengths, flags, info = h.collect_trajectory(n, deterministic=False, seed=s)
    assert len(trajs) == n and info["capacity"] == T and info["path"] == 0 and info["longest"] == int(lengths.max())
    twin.env_reset(s); twin.collect_rollout(T, False)
    r = shaped(pkg, twin, T, n)
    L = first_episodes(r)
    assert np.array_equal(lengths, L)
    lo, hi = agent_box(h, name)
    worst = 0.0
    for m in range(n):
        o, a, rw = trajs[m]
        l = int(L[m])
        assert o.shape == (l + 1, h.D) and a.shape == (l, h.A) and rw.shape == (l,)
        assert flags[m] == int(r["term"][l - 1, m]) | int(r["trunc"][l - 1, m]) << 1, (name, m)
        assert np.array_equal(bits(o[:l]), bits(r["obs"][:l, m])), (name, m, "observations")
        assert np.array_equal(bits(rw), bits(r["rew"][:l, m])), (name, m, "rewards")
        if r["trunc"][l - 1, m]:
            assert np.array_equal(bits(o[l]), bits(r["next"][l - 1, m])), (name, m, "final row")
        want = to_env(r["act"][:l, m].reshape(l, h.A), lo, hi)                         # the ring stores the raw action: to_env on the host (another tanhf)
        worst = max(worst, float(np.abs(a - want).max()))
        np.testing.assert_allclose(a, want, rtol=0, atol=1e-6)
    print(f"{name}: max |recorded action - to_env(ring raw action)| = {worst:.3g}")
    assert (flags & TRUNC).any()
    h.close(); twin.close()


# ---- 2: replay through other kernels ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,deterministic", [("pendulum", True), ("pendulum", False), ("mcc", True), ("mcc", False)])
def test_recorded_actions_replay_through_the_ppo_env_kernels(pkg, name, deterministic):
    if name == "pendulum":
        T = 12
        h, layer = sac(pkg, name, E, T)
        h.set_params(init_params(pkg, layer, scale_out=3.0))
    else:
        T = pump_limit(pkg)
        h = pump(pkg)
    trajs, lengths, flags, _ = h.collect_trajectory(E, deterministic=deterministic, seed=SEED)
    if name == "mcc" and deterministic:
        assert (flags == TERM).any() and ((flags & TRUNC) != 0).any(), flags
    plain = ppo_make(pkg, 1 if name == "pendulum" else 4, (64, 64), T, n_envs=E)
    replay(plain, SEED, trajs, None)                                                    # observations and rewards to the bit, the end at the recorded step, truncated final rows
    h.close(); plain.close()


# ---- 3: final rows of terminated episodes -------------------------------------------------------------------------------------------------------------------------------
def test_final_rows_of_terminated_mountaincar_episodes(pkg):
    limit = pump_limit(pkg)
    h = pump(pkg)
    trajs, lengths, flags, _ = h.collect_trajectory(E, seed=SEED)
    only_term, trunc = flags == TERM, (flags & TRUNC) != 0
    assert only_term.any() and trunc.any(), flags                                      # terminated and truncated recorded envs both occur
    # the twin that never terminates and never resets: every env in the recorded state of the step before its last one (the observation is the state), stepped once
    f = ppo_make(pkg, 4, (64, 64), limit, n_envs=E, fixed_length_episodes=1)
    f.env_reset(SEED)
    f.env_set_state(np.stack([trajs[m][0][-2] for m in range(E)]), np.zeros(E, np.int32))
    _, term, tr, _ = f.env_step(np.stack([trajs[m][1][-1] for m in range(E)]))
    assert not term.any() and not tr.any()
    after = f.env_observe(update_stats=False)
    final = np.stack([trajs[m][0][-1] for m in range(E)])
    assert np.array_equal(bits(final), bits(after))
    goal = (final[:, 0] >= F(0.45)) & (final[:, 1] >= 0)                               # MountainCarContinuous-v0: position >= 0.45 and velocity >= 0
    assert goal[(flags & TERM) != 0].all() and not goal[flags == TRUNC].any()
    h.close(); f.close()


def test_final_rows_of_terminated_reacher3_episodes(pkg):
    b = np.array([3.0, 3.0, 3.0], F)                                                   # every joint pushed the same way: |p| > 2 after twenty-odd steps

    def mk(T):
        h, layer = sac(pkg, "reacher3", EP, T)
        h.set_params(constant_actor(pkg, layer, b))
        return h
    probe = mk(60)
    _, _, el = probe.evaluate_agent(EP, True, seed=SEED)
    probe.close()
    lens = np.sort(el)
    limit = int(lens[len(lens) // 2])
    print(f"reacher3 first-episode lengths {lens.tolist()} -> time limit {limit}")
    assert el.max() < 2 * el.min() and lens[0] < limit < 60
    h = mk(limit)
    trajs, lengths, flags, _ = h.collect_trajectory(EP, seed=SEED)
    assert ((flags & TERM) != 0).any() and (flags == TRUNC).any(), flags
    worst = 0.0
    for m in range(EP):
        o, a, _ = trajs[m]
        nst, _, out = _reacher_step(o[-2][None, :9], a[-1][None])
        assert bool(out[0]) == bool(flags[m] & TERM), (m, flags[m])                    # the final state is out of bounds exactly where the episode terminated
        worst = max(worst, float(np.abs(o[-1][:9] / nst[0] - 1).max()))
        np.testing.assert_allclose(o[-1][:9], nst[0], rtol=1e-4)
        assert np.array_equal(bits(o[-1][9:]), bits(_reacher_obs(o[-1][None, :9])[0, 9:]))   # p - g of the row's own p and g
        assert (np.abs(o[-1][:3]) > 2).any() == bool(flags[m] & TERM)
    print(f"reacher3: max relative |final row - NumPy twin| = {worst:.3g}")
    h.close()


# ---- 4: consistency with dril_sac_evaluate_agent ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [True, False])
def test_recorded_rewards_sum_to_the_evaluations_returns(pkg, deterministic):
    T, s = 12, 77
    h, layer = sac(pkg, "pendulum", E, T)
    h.set_params(init_params(pkg, layer, scale_out=3.0))
    trajs, lengths, flags, _ = h.collect_trajectory(E, deterministic=deterministic, seed=s)
    assert (lengths == T).all() and (flags == TRUNC).all()
    _, er, el = h.evaluate_agent(E, deterministic, seed=s)                              # every episode lasts T: the first E events are the envs' first episodes in env order
    sums = np.zeros(E, F)
    for t in range(T):
        sums = (sums + np.array([trajs[m][2][t] for m in range(E)], F)).astype(F)      # float32, step order
    assert np.array_equal(bits(sums), bits(er)) and np.array_equal(el, lengths)
    other = h.collect_trajectory(E, deterministic=not deterministic, seed=s)[0]
    assert any(not np.array_equal(trajs[m][1], other[m][1]) for m in range(E))          # the draws are draws
    h.close()


# ---- 5: ScalingWrapperEnv ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["kind2", "kind7", "plugin"])
def test_scaling_wrapper_rows_are_unscaled_and_the_final_row_is_not(pkg, which):
    """Against the ring of a scaled twin (a stochastic recording: the collection's draws), with host.py's unscale_observation / unscale_action: observations to
    atol = 1e-5 as tests/test_gpu_traj_device.py compares the same maps, rewards and the default final row to the bit; the actions to 1e-6 of the agent-facing Box
    (the adapter's bound of tests/test_sac_env_plugin.py) times the slope of unscale!.  Against the recording of the unscaled twin kind under an actor whose mean
    does not depend on the observation (the two agents see different observations): observations to the same atol = 1e-5."""
    T, s = 10, 77
    scaled, plain, n = {"kind2": ("pendulum_scaled", "pendulum", E), "kind7": ("mcc_scaled", "mcc", E), "plugin": ("pendulum_plugin_scaled", "pendulum_plugin", EP)}[which]
    env = pkg.DeviceModuleEnv(_co("pendulum"), n, scaling=True).env if which == "plugin" else pkg.ScalingWrapperEnv(pkg.MountainCarContinuousEnv() if which == "kind7" else pkg.PendulumEnv())
    (h, layer), (twin, _), (p, _) = sac(pkg, scaled, n, T), sac(pkg, scaled, n, T), sac(pkg, plain, n, T)
    flat = init_params(pkg, layer, scale_out=3.0)
    h.set_params(flat); twin.set_params(flat)
    twin.env_reset(s); twin.collect_rollout(T, False)
    r = shaped(pkg, twin, T, n)
    L = first_episodes(r)
    one = np.ones(h.A, F)
    slope = float(np.abs(env.unscale_action(one) - env.unscale_action(-one)).max()) / 2
    for final_original in (False, True):
        trajs, lengths, flags, _ = h.collect_trajectory(n, deterministic=False, seed=s, final_original=final_original)
        assert np.array_equal(lengths, L)
        worst = 0.0
        for m in range(n):
            o, a, rw = trajs[m]
            l = int(L[m])
            want_o = env.unscale_observation(r["obs"][:l, m])
            worst = max(worst, float(np.abs(o[:l] - want_o).max()))
            np.testing.assert_allclose(o[:l], want_o, rtol=0, atol=1e-5)
            np.testing.assert_allclose(a, env.unscale_action(to_env(r["act"][:l, m].reshape(l, h.A), -one, one)), rtol=0, atol=1e-6 * slope)
            assert np.array_equal(bits(rw), bits(r["rew"][:l, m]))
            if r["trunc"][l - 1, m] and not final_original:
                assert np.array_equal(bits(o[l]), bits(r["next"][l - 1, m])), (which, m)  # observe(env) as ScalingWrapperEnv delivers it (:44)
            if r["trunc"][l - 1, m] and final_original:
                np.testing.assert_allclose(o[l], env.unscale_observation(r["next"][l - 1, m]), rtol=0, atol=1e-5)
        print(f"{which} final_original={final_original}: max |recorded - unscale_observation(ring)| = {worst:.3g}")
        assert not np.allclose(trajs[0][0][:-1], r["obs"][:L[0], 0], atol=1e-3)          # the rows are not the scaled ones
    # the unscaled twin kind
    const = constant_actor(pkg, layer, [0.3])
    h.set_params(const); p.set_params(const)
    ts, ls, fs, _ = h.collect_trajectory(n, seed=s)
    tp, lp, fp, _ = p.collect_trajectory(n, seed=s)
    assert np.array_equal(ls, lp) and np.array_equal(fs, fp)
    worst = 0.0
    for m in range(n):
        l = int(ls[m])
        worst = max(worst, float(np.abs(ts[m][0][:l] - tp[m][0][:l]).max()))
        np.testing.assert_allclose(ts[m][0][:l], tp[m][0][:l], rtol=0, atol=1e-5)
        np.testing.assert_allclose(ts[m][1], tp[m][1], rtol=0, atol=1e-6 * slope)       # the action row is the unscaled action
        np.testing.assert_allclose(env.unscale_observation(ts[m][0][l]), tp[m][0][l], rtol=0, atol=1e-5)   # and the final row is scaled
    print(f"{which}: max |recorded - unscaled twin kind's recording| = {worst:.3g}")
    for x in (h, twin, p):
        x.close()


# ---- 6: the normaliser is frozen, the recording raw ---------------------------------------------------------------------------------------------------------------------
def _nz_snapshot(h):
    st = h.norm_get_stats()
    orig = h.norm_get_original()
    return [np.asarray(st[k]) for k in sorted(st)] + [h.norm_get_returns(), orig[0], orig[1]]


@pytest.mark.parametrize("name,n", [("pendulum", E), ("reacher3", EP)])
def test_normaliser_is_frozen_and_the_recording_is_raw(pkg, name, n):
    T = 9
    (a, layer), (plain, _) = sac(pkg, name, n, T), sac(pkg, name, n, T)
    flat = init_params(pkg, layer, scale_out=3.0)
    a.set_params(flat); plain.set_params(flat)
    a.normalize_enable(clip_obs=5.0); a.env_reset(4)
    a.collect_rollout(3, True); a.collect_rollout(5, False)                              # training collections: the statistics are not the initial ones
    st = a.norm_get_stats()
    assert st["obs_count"] > 0 and not np.allclose(st["obs_var"], 1.0) and a.norm_get_returns().any()
    keep = _nz_snapshot(a)
    recs = []
    for training in (True, False):
        a.normalize_set_training(training)
        recs.append(a.collect_trajectory(n, seed=SEED))
        after = _nz_snapshot(a)
        assert len(keep) == len(after) and all(x.dtype == y.dtype and np.array_equal(bits(x) if x.dtype == F else x, bits(y) if y.dtype == F else y) for x, y in zip(keep, after)), training
    same_trajs(recs[0][0], recs[1][0], n, "training flag")                             # frozen for the call whatever the flag
    trajs = recs[0][0]
    got = plain.collect_trajectory(n, seed=SEED)[0]                                     # no wrapper: another agent input, other actions
    assert all(np.array_equal(bits(x[0][0]), bits(y[0][0])) for x, y in zip(got, trajs))           # the same first observation, raw
    assert any(not np.array_equal(bits(x[1][0]), bits(y[1][0])) for x, y in zip(got, trajs))       # and already another first action
    ppo = ppo_make(pkg, 1, (64, 64), T, n_envs=n, **(dict(module="reacher3") if name == "reacher3" else {}))
    replay(ppo, SEED, trajs, None)                                                      # the recording is the env's own: raw observations and rewards, the final rows too
    for x in (a, plain, ppo):
        x.close()


# ---- 7: independence -----------------------------------------------------------------------------------------------------------------------------------------------------
def _check_independence(h, n, ms, limit):
    base, base_len, base_flags, info = h.collect_trajectory(n, seed=SEED)
    assert info["longest"] == base_len.max() and info["cut_by_max_steps"] == 0
    for M in ms:
        for poll in (1, 7, 0):
            trajs, lengths, flags, info = h.collect_trajectory(M, seed=SEED, poll_steps=poll)
            same_trajs(trajs, base, M, (M, poll))
            assert np.array_equal(lengths, base_len[:M]) and np.array_equal(flags, base_flags[:M])
            K = poll or min(limit, 32)
            longest = int(lengths.max())
            assert info["longest"] == longest and info["capacity"] == limit
            assert info["steps_enqueued"] == min(-(-longest // K) * K, limit), (M, poll, info)   # whole groups of K, never past Tcap
            assert info["launches"] >= info["steps_enqueued"]
    for max_steps in (1, 5):
        trajs, lengths, flags, info = h.collect_trajectory(n, max_steps=max_steps, seed=SEED)
        cut = base_len > max_steps
        assert np.array_equal(lengths, np.minimum(base_len, max_steps)) and np.array_equal(flags, np.where(cut, CUT, base_flags))   # bit 2 exactly where the episode had not ended
        assert info["capacity"] == min(max_steps, limit) and info["cut_by_max_steps"] == int(cut.sum()) and info["longest"] == int(lengths.max()) and info["steps_enqueued"] <= max_steps
        for m in range(n):
            l = int(lengths[m])
            for x, y in zip(trajs[m], (base[m][0][:l + 1], base[m][1][:l], base[m][2][:l])):
                assert np.array_equal(bits(x), bits(y)), (max_steps, m)
    return base_len, base_flags


def test_a_trajectory_depends_on_nothing_but_its_env_builtin(pkg):
    limit = pump_limit(pkg)
    h = pump(pkg)
    base_len, base_flags = _check_independence(h, E, MS, limit)
    assert len(np.unique(base_len)) > 2 and (base_flags == TERM).any()
    h.close()


def test_a_trajectory_depends_on_nothing_but_its_env_plugin(pkg):
    h, layer = sac(pkg, "reacher3", EP, 15)
    h.set_params(init_params(pkg, layer, scale_out=3.0))
    _check_independence(h, EP, (1, 7, EP), 15)
    h.close()


# ---- 8: isolation -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pendulum", "reacher3"])
def test_recordings_between_iterations_change_nothing(pkg, name):
    n = 16
    hs = []
    for _ in range(2):
        h, layer = sac(pkg, name, n, 6, train_freq=2, gradient_steps=1)
        h.set_params(init_params(pkg, layer, scale_out=3.0)); h.monitor_enable(100); h.env_reset(8)
        h.collect_rollout(2, True)
        hs.append(h)
    a, b = hs
    first = [a.iterate(3)[0], b.iterate(3)[0]]
    recs = []
    for det in (True, False):
        for M, max_steps in ((1, None), (n, 5), (7, None)):
            recs.append(b.collect_trajectory(M, max_steps=max_steps, deterministic=det, seed=1000 + len(recs)))
    assert all(np.isfinite(t[2]).all() for rec in recs for t in rec[0])
    nxt = [a.iterate(2)[0], b.iterate(2)[0]]
    assert [bytes(s) for s in first[0]] == [bytes(s) for s in first[1]]
    assert [bytes(s) for s in nxt[0]] == [bytes(s) for s in nxt[1]] and len(nxt[0]) == 2   # the update statistics of the next iterations
    assert_rings_equal(ring(pkg, a), ring(pkg, b))
    assert np.array_equal(bits(a.get_params()), bits(b.get_params())) and np.array_equal(bits(a.get_target_params()), bits(b.get_target_params()))
    assert bits(np.array([a.get_log_ent_coef()], F))[0] == bits(np.array([b.get_log_ent_coef()], F))[0]
    ma, mb = a.monitor_stats(), b.monitor_stats()
    assert ma == mb and ma[2] > 0                                                       # training episodes are in the window; the recorded ones are not
    assert np.array_equal(bits(a.env_observe()), bits(b.env_observe()))
    a.close(); b.close()


def test_a_never_reset_handle_records_and_stays_unreset(pkg):
    capi = pkg._capi
    (h, layer), (g, _) = sac(pkg, "pendulum", E, 9), sac(pkg, "pendulum", E, 9)
    flat = init_params(pkg, layer, scale_out=3.0)
    h.set_params(flat); g.set_params(flat)
    g.env_reset(3); g.collect_rollout(4, False)
    a, b = h.collect_trajectory(17, seed=SEED), g.collect_trajectory(17, seed=SEED)
    same_trajs(a[0], b[0], 17, "never reset")
    with pytest.raises(pkg.DrilError) as e:
        h.collect_rollout(1, False)
    assert e.value.code == capi.ERR_NOT_INITIALISED
    assert h.replay_size() == 0
    h.close(); g.close()


# ---- 9: refusals ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_healthy(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    n, T = 24, 20
    h, layer = sac(pkg, "pendulum", n, T)
    h.set_params(init_params(pkg, layer, scale_out=3.0)); h.env_reset(3)
    want = h.collect_trajectory(n)
    o, info, cap = capi.DrilTrajOptions(), capi.DrilTrajInfo(), C.c_int32()
    obs, act, rew = np.zeros((n, T + 1, 3), F), np.zeros((n, T, 1), F), np.zeros((n, T), F)
    lengths, flags = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    arrays = [p(obs), p(act), p(rew), p(lengths), p(flags)]
    call = lambda opt, arr=arrays: lib.dril_sac_collect_trajectory(h._h, opt, *arr, C.byref(info))
    for field, bad in (("n_trajectories", 0), ("n_trajectories", -2), ("n_trajectories", n + 1), ("max_steps", -1), ("poll_steps", -1)):
        lib.dril_traj_options_default(C.byref(o)); o.n_trajectories = n
        setattr(o, field, bad)
        assert call(C.byref(o)) == capi.ERR_INVALID_ARG, field
        assert b"dril_sac_collect_trajectory" in lib.dril_sac_last_error(h._h)
    lib.dril_traj_options_default(C.byref(o)); o.n_trajectories = n
    assert call(None) == capi.ERR_INVALID_ARG
    for i in range(5):
        assert call(C.byref(o), arrays[:i] + [None] + arrays[i + 1:]) == capi.ERR_INVALID_ARG, i
    assert lib.dril_sac_collect_trajectory(None, C.byref(o), *arrays, None) == capi.ERR_NOT_INITIALISED
    assert lib.dril_sac_trajectory_capacity(h._h, None, C.byref(cap)) == capi.ERR_INVALID_ARG and lib.dril_sac_trajectory_capacity(h._h, C.byref(o), None) == capi.ERR_INVALID_ARG
    for max_steps, want_cap in ((0, T), (5, 5), (T, T), (T + 1, T)):
        o.max_steps = max_steps
        assert lib.dril_sac_trajectory_capacity(h._h, C.byref(o), C.byref(cap)) == capi.OK and cap.value == want_cap
    o.max_steps = 0
    # a recording past 1 GiB on the device: refused before anything is allocated, with its size, M and Tcap
    big, _ = sac(pkg, "pendulum", n, 4_000_000)
    with pytest.raises(pkg.DrilError) as e:
        big.collect_trajectory(n)
    assert e.value.code == capi.ERR_INVALID_ARG and str(4 * n * (4_000_001 * 3 + 2 * 4_000_000) + 5 * n) in str(e.value) and f"M = {n}" in str(e.value) and "Tcap = 4000000" in str(e.value)
    assert len(big.collect_trajectory(n, max_steps=6)[0]) == n                           # max_steps bounds the recording
    big.close()
    cfg = capi.DrilSacConfig()
    assert lib.dril_sac_config_default(C.byref(cfg), capi.ENV_EXTERNAL) == capi.OK
    cfg.n_envs, cfg.hidden1, cfg.hidden2, cfg.batch_size, cfg.buffer_capacity = 4, 32, 32, 8, 64
    cfg.ext_obs_dim, cfg.ext_action_dim, cfg.ext_action_low, cfg.ext_action_high = 5, 2, -1.0, 1.0
    ext = pkg.SacHandle(cfg)
    with pytest.raises(pkg.DrilError) as e:
        ext.collect_trajectory(1)
    assert e.value.code == capi.ERR_UNSUPPORTED and "DRIL_ENV_EXTERNAL" in str(e.value)
    xo, xa = np.zeros((1, 2, 5), F), np.zeros((1, 1, 2), F)
    lib.dril_traj_options_default(C.byref(o))
    assert lib.dril_sac_collect_trajectory(ext._h, C.byref(o), p(xo), p(xa), p(rew), p(lengths), p(flags), None) == capi.ERR_UNSUPPORTED
    assert b"dril_sac_predict_actions" in lib.dril_sac_last_error(ext._h)
    ext.close()
    # a refused call leaves the handle healthy: it records again, with the same result; NULL info is legal; the persistent request is accepted and ignored
    lib.dril_traj_options_default(C.byref(o)); o.n_trajectories = n
    o.reserved[capi.TRAJ_OPT_PERSISTENT] = 1
    assert call(C.byref(o)) == capi.OK and info.reserved[capi.TRAJ_INFO_PATH] == 0 and info.capacity == T
    assert lib.dril_sac_collect_trajectory(h._h, C.byref(o), *arrays, None) == capi.OK
    assert np.array_equal(lengths, want[1]) and np.array_equal(flags, want[2])
    for m in range(n):
        L = lengths[m]
        assert np.array_equal(obs[m, :L + 1], want[0][m][0]) and np.array_equal(act[m, :L], want[0][m][1]) and np.array_equal(rew[m, :L], want[0][m][2])
        assert not obs[m, L + 1:].any() and not act[m, L:].any() and not rew[m, L:].any()   # rows past the trajectory's length are zero
    h.collect_rollout(2, False)
    assert h.replay_size() == 2 * n
    h.close()


# ---- 10: the Python mirror ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_python_mirror(pkg):
    import warnings
    alg = pkg.SAC(batch_size=16, buffer_capacity=256)

    def fresh(env):
        return pkg.SACAgent(pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=HID), alg, seed=1)
    env = pkg.DeviceParallelEnv(pkg.PendulumEnv(max_steps=12), 8, seed=3)
    agent = fresh(env)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        obs, act, rew = pkg.sac_collect_trajectory(agent, env)
    assert not any("Max steps reached" in str(w.message) for w in caught)              # no warning where no trajectory is cut
    assert obs.shape == (13, 3) and act.shape == (12, 1) and rew.shape == (12,) and (np.abs(act) <= 2).all() and (rew <= 0).all()
    many = pkg.sac_collect_trajectory(agent, env, n_trajectories=5, norm_env=env)
    assert len(many) == 5 and all(np.array_equal(x, y) for x, y in zip(many[0], (obs, act, rew)))
    with pytest.warns(UserWarning, match="Max steps reached"):
        o3, a3, r3 = pkg.sac_collect_trajectory(agent, env, max_steps=3)
    assert len(r3) == 3 and np.array_equal(o3, obs[:4]) and np.array_equal(a3, act[:3])
    sto = pkg.sac_collect_trajectory(agent, env, deterministic=False, seed=9)
    assert np.array_equal(sto[0], pkg.sac_collect_trajectory(agent, env, deterministic=False, seed=9)[0]) and not np.array_equal(sto[1], act)
    # NormalizeWrapperEnv: the warning of sac_evaluate_agent without statistics, none with them
    with pytest.warns(RuntimeWarning, match="no normalize_stats were given"):
        nobs, _, _ = pkg.sac_collect_trajectory(agent, env, normalize=dict(clip_obs=5.0))
    assert np.array_equal(nobs[0], obs[0])                                              # the recording is raw
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        st = dict(obs_mean=np.array([0.5, -0.5, 1.0], F), obs_var=np.array([0.1, 0.2, 4.0], F), obs_count=100, ret_mean=0.0, ret_var=1.0, ret_count=100)
        o_n, a_n, _ = pkg.sac_collect_trajectory(agent, env, normalize=dict(clip_obs=5.0), normalize_stats=st)
    assert np.array_equal(o_n[0], obs[0]) and not np.array_equal(a_n[0], act[0])          # the agent saw the normalised observation
    # a device env plug-in
    menv = pkg.DeviceModuleEnv(_co("reacher3"), 6, seed=4, max_steps=9)
    magent = fresh(menv)
    o, a, r = pkg.sac_collect_trajectory(magent, menv)
    assert o.shape == (10, 12) and a.shape == (9, 3) and r.shape == (9,)
    several = pkg.sac_collect_trajectory(magent, menv, n_trajectories=6)
    assert len(several) == 6 and np.array_equal(several[0][0], o) and not np.array_equal(several[1][0], o)
    with pytest.raises(NotImplementedError):
        pkg.sac_collect_trajectory(agent, env, norm_env=object())
    with pytest.raises(NotImplementedError):
        pkg.sac_collect_trajectory(agent, pkg.HostParallelEnv([], seed=0))
