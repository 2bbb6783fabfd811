"""GPU (-m gpu): collect_trajectory of a PPO handle on the device (dril_collect_trajectory_device, docs/evaluation.md "Trajectories"), every check through the C ABI /
pkg.Handle.

Checkers: (1) the per-step host loop on a twin handle — env_reset(seed), env_observe(update_stats=False), predict_actions(deterministic=True), to_env in NumPy,
env_step — built into trajectories by the reference's loop (trajectory_utils.jl:16-45), compared BITWISE; (2) for the row the host loop cannot see, the observation
after the last step of a terminated episode: a second twin with fixed_length_episodes = 1, put into the recorded state of the step before and stepped once with the
recorded action, and the kind's own termination predicate; (3) for what the call must NOT do, a twin that trained without it, compared bitwise.

Shapes: E = 300 (two workgroups, the second partial), M in {1, 37, 300}.  A comparison that never met a termination proves nothing, so every kind that can terminate
is driven by a policy that makes it terminate (CartPole: a nudged random net; MountainCar / MountainCarContinuous: push where the car moves; Acrobot: torque against
the first joint's velocity), and its time limit is taken from the host loop itself: the median first-episode length of the recorded envs under a long limit, so that
some recorded envs terminate before it and the others are truncated at it.  Each test asserts that on the host loop's own flags first."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_gpu_env_plugin import _cfg, _co
from test_gpu_eval_device import assert_bitwise, nudged_params, snapshot, stats_equal

pytestmark = pytest.mark.gpu
E = 300
MS = (1, 37, 300)
F = np.float32
TERM, TRUNC, CUT = 1, 2, 4
SEED = 13


# ---- handles, policies, the host loop ------------------------------------------------------------------------------------------------------------------------------
def feature_policy(h, hidden, feature, gain, out_w):
    """an actor whose outputs are out_w * tanh(2 tanh(gain * obs[feature])), everything else zero (flat layout: actor {W1 b1 W2 b2 W3 b3} first, W column-major)"""
    H1, H2 = hidden
    flat = np.zeros(h.P, F)
    flat[feature * H1] = gain                                                          # W1 (H1 x D): (0, feature)
    w2 = H1 * h.D + H1
    flat[w2] = 2.0                                                                     # W2 (H2 x H1): (0, 0)
    w3 = w2 + H2 * H1 + H2
    flat[w3:w3 + len(out_w)] = out_w                                                   # W3 (O x H2): column 0
    return flat


def policy_for(h, kind, hidden):
    if kind == 3:
        return feature_policy(h, hidden, 1, 100.0, (-3.0, 0.0, 3.0))                   # MountainCar: push where the car moves
    if kind in (4, 7):
        return feature_policy(h, hidden, 1, 100.0, (3.0,))
    if kind == 6:
        return feature_policy(h, hidden, 4, -5.0, (-3.0, 0.0, 3.0))                    # Acrobot: torque against the first joint's velocity pumps it up
    return nudged_params(h, hidden)                                                    # CartPole: poles fall at different steps; Pendulum: never terminates


def make(pkg, kind, hidden=(64, 64), episode_len=20, module=None, scaling=False, fused=False, n_envs=E, flat=None, **kw):
    cfg = _cfg(pkg, pkg._capi.ENV_MODULE if module else kind, n_envs=n_envs, n_steps=kw.pop("n_steps", 2), batch_size=kw.pop("batch_size", n_envs), episode_len=episode_len,
               hidden1=hidden[0], hidden2=hidden[1], **kw)
    h = pkg.Handle(cfg, env_module=_co(module) if module else None)
    if scaling:
        h.scaling_enable(True)
    if fused:
        h.rollout_fused_enable(True)
    h.set_params(policy_for(h, kind, hidden) if flat is None else flat)
    return h


def agent_bounds(h, kind, scaling=False):
    """the agent-facing Box the ClampAdapter acts on (None: Discrete)"""
    if h.discrete:
        return None
    if h.cfg.env_kind == 8:
        info = h.env_module_info()
        return (np.full(h.A, -1, F), np.full(h.A, 1, F)) if scaling else (info["action_low"][:h.A].astype(F), info["action_high"][:h.A].astype(F))
    b = F(2) if kind == 1 else F(1)
    return np.full(h.A, -b, F), np.full(h.A, b, F)


def to_env(raw, bounds):
    return raw if bounds is None else np.clip(raw, bounds[0], bounds[1]).astype(F)


def host_loop(h, seed, steps, bounds, original=None):
    """`steps` env steps of the per-step verbs on all E envs.  Row t: the observation the agent saw and the original one before step t + 1, the simulator state there,
    the env action, the raw reward, the flags and terminal_obs of the step.  original(h): the raw observation / reward under a normaliser (None: what the verbs return)"""
    h.env_reset(seed)
    keys = ("agent", "orig", "state", "sc", "act", "rew", "term", "trunc", "tobs")
    out = {k: [] for k in keys}
    obs = h.env_observe(update_stats=False)
    for _ in range(steps):
        st, sc = h.env_get_state()
        act = to_env(h.predict_actions(obs, deterministic=True), bounds)
        orig = original(h)[0] if original else obs
        rew, term, trunc, tobs = h.env_step(act)
        if original:
            rew = original(h)[1]
        for k, v in zip(keys, (obs, orig, st, sc, act, rew, term, trunc, tobs)):
            out[k].append(np.array(v, copy=True))
        obs = h.env_observe(update_stats=False)
    out = {k: np.stack(v) for k, v in out.items()}
    out["next"] = obs
    return out


def first_lengths(loop):
    done = loop["term"] | loop["trunc"]
    assert done.any(0).all(), "an env never finished within the loop"
    return done.argmax(0) + 1


def build(loop, m, max_steps=None):
    """trajectory_utils.jl:16-45 for env m on the host loop's arrays -> (observations (L), actions, rewards, final observation or None where the host loop cannot see
    it (terminated: the env auto-reset), end flags); the episode's end takes precedence over the cut"""
    obs, acts, rews, t = [], [], [], 0
    while True:
        obs.append(loop["orig"][t, m]); acts.append(loop["act"][t, m]); rews.append(loop["rew"][t, m])
        term, trunc = bool(loop["term"][t, m]), bool(loop["trunc"][t, m])
        t += 1
        if term or trunc:
            return np.stack(obs), np.stack(acts), np.asarray(rews, F), (loop["tobs"][t - 1, m] if trunc else None), int(term) | int(trunc) << 1
        if max_steps and len(obs) >= max_steps:
            nxt = loop["orig"][t, m] if t < len(loop["orig"]) else loop["next"][m]
            return np.stack(obs), np.stack(acts), np.asarray(rews, F), nxt, CUT


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == F else a.dtype)


def assert_traj(got, want, where, final=True):
    o, a, r = got
    wo, wa, wr, wfinal, _ = want
    L = len(wr)
    assert len(r) == L and len(a) == L and len(o) == L + 1, (where, len(r), L)
    assert np.array_equal(bits(o[:L]), bits(wo)), (where, "observations")
    assert np.array_equal(bits(a), bits(wa)), (where, "actions")
    assert np.array_equal(bits(r), bits(wr)), (where, "rewards")
    if final and wfinal is not None:
        assert np.array_equal(bits(o[L]), bits(wfinal)), (where, "final observation")


def same_trajs(a, b, n, where):
    for m in range(n):
        for x, y in zip(a[m], b[m]):
            assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), (where, m)


LONG = {0: 200, 3: 300, 4: 300, 6: 300, 7: 300}                                        # the probe's time limit for the kinds that can terminate
_REF = {}


def reference(pkg, kind, hidden=(64, 64), action_start=None):
    """computed once per configuration and shared: the time limit (see the module docstring), the host loop on a twin, its trajectories of all E envs"""
    key = (kind, hidden, action_start)
    if key in _REF:
        return _REF[key]
    kw = {} if action_start is None else dict(action_start=action_start)
    limit = 12
    if kind in LONG:
        probe = make(pkg, kind, hidden, LONG[kind], **kw)
        lens = np.sort(first_lengths(host_loop(probe, SEED, LONG[kind], agent_bounds(probe, kind)))[:37])
        probe.close()
        limit = int(lens[len(lens) // 2])
        assert lens[0] < limit < LONG[kind], (kind, lens)                              # some of the first 37 envs terminate before the median; the probe's own limit is not it
    twin = make(pkg, kind, hidden, limit, **kw)
    bounds = agent_bounds(twin, kind)
    loop = host_loop(twin, SEED, limit, bounds)
    twin.close()
    want = [build(loop, m) for m in range(E)]
    flags = np.array([w[4] for w in want])
    if kind in LONG:                                                                   # on the host loop's own flags, among the 37 recorded envs
        assert ((flags[:37] & TERM) != 0).any() and ((flags[:37] & TRUNC) != 0).any(), (kind, flags[:37])
    else:
        assert (flags == TRUNC).all()
    _REF[key] = dict(limit=limit, loop=loop, want=want, flags=flags, kw=kw, bounds=bounds)
    return _REF[key]


# ---- 1: exact equality with the host loop ----------------------------------------------------------------------------------------------------------------------------
CASES = [(k, hd, None) for k in (0, 1, 3, 4, 6) for hd in ((64, 64), (32, 48))] + [(0, (256, 256), None), (0, (64, 64), 0), (0, (64, 64), 1)]


@pytest.mark.parametrize("kind,hidden,action_start", CASES)
def test_trajectories_equal_the_host_loop_bitwise(pkg, kind, hidden, action_start):
    ref = reference(pkg, kind, hidden, action_start)
    h = make(pkg, kind, hidden, ref["limit"], **ref["kw"])
    for M in MS:
        trajs, lengths, flags, info = h.collect_trajectory_device(M, seed=SEED)
        assert len(trajs) == M and info["capacity"] == ref["limit"] and info["longest"] == int(lengths.max()) and info["cut_by_max_steps"] == 0
        assert np.array_equal(flags, ref["flags"][:M]), (kind, M)
        assert lengths.max() <= info["steps_enqueued"] <= ref["limit"] and info["launches"] >= 7 * info["steps_enqueued"]
        for m in range(M):
            assert_traj(trajs[m], ref["want"][m], (kind, hidden, M, m))
    if h.discrete:
        start = h.cfg.action_start
        acts = np.concatenate([t[1] for t in trajs])
        assert acts.min() >= start and acts.max() <= start + h.A - 1 and len(np.unique(acts)) > 1   # the numbering dril_env_step takes
    # max_steps: the cut, and the episode's end taking precedence where both fall on one step
    for max_steps in (1, 5):
        trajs, lengths, flags, info = h.collect_trajectory_device(37, max_steps=max_steps, seed=SEED)
        want = [build(ref["loop"], m, max_steps) for m in range(37)]
        assert info["capacity"] == min(max_steps, ref["limit"]) and np.array_equal(flags, [w[4] for w in want]) and info["cut_by_max_steps"] == int((flags == CUT).sum())
        assert (flags == CUT).any() and lengths.max() <= max_steps
        for m in range(37):
            assert_traj(trajs[m], want[m], (kind, hidden, "max_steps", max_steps, m))
    h.close()


# ---- 2: the rows the host loop cannot see: the observation after the last step of a terminated episode ---------------------------------------------------------------
def terminated_predicate(kind, obs):
    if kind == 0:                                                                      # CartPole: |x| > 2.4 or |theta| > 12 degrees (the observation is the state)
        return (np.abs(obs[:, 0]) > F(2.4)) | (np.abs(obs[:, 2]) > F(0.20943951023931953))
    assert kind == 3                                                                   # MountainCar: position >= 0.5 and velocity >= 0
    return (obs[:, 0] >= F(0.5)) & (obs[:, 1] >= 0)


@pytest.mark.parametrize("kind", [0, 3, 4, 6, 7])
def test_final_rows_of_terminated_episodes(pkg, kind):
    ref = reference(pkg, kind)
    h = make(pkg, kind, (64, 64), ref["limit"])
    trajs, lengths, flags, _ = h.collect_trajectory_device(E, seed=SEED)
    assert np.array_equal(flags, ref["flags"]) and ((flags & TERM) != 0).sum() >= 2
    loop = ref["loop"]
    # the twin that never terminates and never resets: every env in the recorded state of the step before its last one, stepped once with the recorded action
    f = make(pkg, kind, (64, 64), ref["limit"], fixed_length_episodes=1)
    f.env_reset(SEED)
    idx = lengths - 1
    f.env_set_state(loop["state"][idx, np.arange(E)], np.zeros(E, np.int32))
    acts = np.stack([trajs[m][1][-1] for m in range(E)])
    if kind == 7:
        acts = loop["act"][idx, np.arange(E)]                                          # (the scaled twin takes the agent-facing action; the recorded one is unscaled)
    _, term, trunc, _ = f.env_step(acts)
    assert not term.any() and not trunc.any()
    after = f.env_observe(update_stats=False)
    final = np.stack([trajs[m][0][-1] for m in range(E)])
    assert np.array_equal(bits(final), bits(after)), kind
    f.close(); h.close()
    # shadow cross-check: at truncated steps the final row is the live terminal_obs
    tr = (flags & TRUNC) != 0
    assert tr.any() and np.array_equal(bits(final[tr]), bits(loop["tobs"][idx, np.arange(E)][tr]))
    if kind in (0, 3):
        only_term, only_trunc = flags == TERM, flags == TRUNC
        assert terminated_predicate(kind, final[only_term]).all() and only_term.any()
        assert not terminated_predicate(kind, final[only_trunc]).any() and only_trunc.any()


# ---- 3: ScalingWrapperEnv ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["kind2", "kind7", "plugin"])
def test_scaling_wrapper_rows_are_unscaled_and_the_final_row_is_not(pkg, which):
    """rows 0..L-1 and the actions against host.py's unscale_observation / unscale_action of the host loop's (scaled) values: the actions to the bit and the
    observations to atol = 1e-5, as tests/test_gpu_env_plugin_scaling.py compares the same maps; rewards and the default final row to the bit"""
    if which == "plugin":
        limit = 12
        mk = lambda **kw: make(pkg, 1, (64, 64), limit, module="pendulum", scaling=True, **kw)
        env = pkg.DeviceModuleEnv(_co("pendulum"), E, scaling=True).env
        kind = 1
    else:
        kind = 2 if which == "kind2" else 7
        ref = reference(pkg, kind)
        limit = ref["limit"]
        mk = lambda **kw: make(pkg, kind, (64, 64), limit, **kw)
        env = pkg.ScalingWrapperEnv(pkg.PendulumEnv() if kind == 2 else pkg.MountainCarContinuousEnv())
    twin = mk()
    bounds = (np.full(twin.A, -1, F), np.full(twin.A, 1, F))
    loop = host_loop(twin, SEED, limit, bounds) if which == "plugin" else ref["loop"]
    h = mk()
    for final_original in (False, True):
        trajs, lengths, flags, _ = h.collect_trajectory_device(37, seed=SEED, final_original=final_original)
        worst = 0.0
        for m in range(37):
            wo, wa, wr, wfinal, wflags = build(loop, m)
            o, a, r = trajs[m]
            L = len(wr)
            assert flags[m] == wflags and lengths[m] == L
            want_o = env.unscale_observation(wo)
            worst = max(worst, float(np.abs(o[:L] - want_o).max()))
            np.testing.assert_allclose(o[:L], want_o, rtol=0, atol=1e-5)
            assert np.array_equal(bits(a), bits(env.unscale_action(wa).astype(F))), (which, m)
            assert np.array_equal(bits(r), bits(wr))
            if wfinal is not None and not final_original:
                assert np.array_equal(bits(o[L]), bits(wfinal)), (which, m)             # observe(env) as ScalingWrapperEnv delivers it (:44)
            if wfinal is not None and final_original:
                np.testing.assert_allclose(o[L], env.unscale_observation(wfinal), rtol=0, atol=1e-5)
        print(f"{which} final_original={final_original}: max |recorded - unscale_observation(host loop)| = {worst:.3g}")
        assert not np.allclose(trajs[0][0][:-1], build(loop, 0)[0], atol=1e-3)            # the rows are not the scaled ones
    twin.close(); h.close()


# ---- 4: normalisers ------------------------------------------------------------------------------------------------------------------------------------------------------
def replay(plain, seed, trajs, bounds):
    """the recorded actions through env_step of a handle without wrappers, from env_reset(seed): the recorded observations and rewards to the bit, and the final row
    where the step truncates (terminal_obs)"""
    plain.env_reset(seed)
    M = len(trajs)
    longest = max(len(t[2]) for t in trajs)
    for t in range(longest):
        obs = plain.env_observe(update_stats=False)
        act = np.zeros((plain.E,) if plain.discrete else (plain.E, plain.A), np.int32 if plain.discrete else F)
        if plain.discrete:
            act[:] = plain.cfg.action_start
        live = [m for m in range(M) if len(trajs[m][2]) > t]
        for m in live:
            act[m] = trajs[m][1][t]
        rew, term, trunc, tobs = plain.env_step(act)
        for m in live:
            o, a, r = trajs[m]
            assert np.array_equal(bits(o[t]), bits(obs[m])) and bits(r[t:t + 1])[0] == bits(rew[m:m + 1])[0], (t, m)
            assert (len(r) == t + 1) == bool(term[m] or trunc[m]), (t, m)
            if trunc[m]:
                assert np.array_equal(bits(o[t + 1]), bits(tobs[m])), (t, m)


@pytest.mark.parametrize("which", ["builtin", "plugin"])
def test_normalisers_are_frozen_and_the_recording_is_raw(pkg, which):
    """a: a training normaliser after one collection.  b: the twin with training off and a's statistics.  plain: the same envs without the wrapper.
    builtin (Pendulum, cfg.norm_*): b runs the host loop, compared bitwise.  plugin (reacher3, D = 12, A = 3, dril_normalize_enable): b runs the verb itself — on this
    shape the host's dril_predict_actions (actor and critic in one pair launch) and the step-granular launches (the actor alone) round differently in the last bits,
    for every verb of the library, so a host loop is no bitwise checker there; that the agent saw the normalised observation is shown by the trajectories being
    those of b, and not those of plain nor of a twin with other statistics"""
    limit = 12
    if which == "builtin":
        nkw = dict(norm_obs=1, norm_reward=1)
        a = make(pkg, 1, (64, 64), limit, n_steps=8, batch_size=E * 8, norm_training=1, **nkw)
        b = make(pkg, 1, (64, 64), limit, norm_training=0, **nkw)
        c = make(pkg, 1, (64, 64), limit, norm_training=0, **nkw)
        plain = make(pkg, 1, (64, 64), limit)
        get_stats, original = (lambda h: h.norm_get_stats()), (lambda h: h.norm_get_original())
        a.env_reset(4); a.collect_rollout()                                            # one training collection: the statistics are not the initial ones
        st = get_stats(a)
        b.norm_set_stats(st["obs_mean"], st["obs_var"], st["obs_count"], st["ret_mean"], st["ret_var"], st["ret_count"])
    else:
        mk = lambda **kw: make(pkg, 1, (64, 64), limit, module="reacher3", **kw)
        a, b, c, plain = mk(n_steps=8, batch_size=E * 8), mk(), mk(), mk()
        assert (a.D, a.A) == (12, 3)
        for h in (a, b, c):
            h.normalize_enable(clip_obs=1.25, clip_reward=0.75, gamma=0.9, epsilon=1e-6)
        get_stats, original = (lambda h: h.normalize_get_stats()), (lambda h: h.normalize_get_original())
        a.env_reset(4); a.collect_rollout()
        st = get_stats(a)
        b.normalize_set_stats(**st); b.normalize_set_training(False); c.normalize_set_training(False)
    assert st["obs_count"] > 0 and not np.allclose(st["obs_var"], 1.0)
    keep = (get_stats(a), original(a), a.env_get_state())
    bounds = agent_bounds(b, 1)
    trajs, lengths, flags, _ = a.collect_trajectory_device(37, seed=SEED)
    if which == "builtin":
        loop = host_loop(b, SEED, limit, bounds, original=original)                    # the frozen twin: normalised observations to the agent, raw ones recorded
        assert not np.allclose(loop["agent"], loop["orig"], atol=1e-3)
        for m in range(37):
            assert_traj(trajs[m], build(loop, m), (which, m), final=False)             # raw observations and rewards, the frozen twin's actions
            assert flags[m] == build(loop, m)[4]
    else:
        twin, twin_len, twin_flags, _ = b.collect_trajectory_device(37, seed=SEED)
        same_trajs(trajs, twin, 37, which)
        assert np.array_equal(lengths, twin_len) and np.array_equal(flags, twin_flags)
    for other in (plain, c):                                                           # no wrapper / the initial statistics: another agent input, other actions
        got = other.collect_trajectory_device(37, seed=SEED)[0]
        assert all(np.array_equal(bits(x[0][0]), bits(y[0][0])) for x, y in zip(got, trajs))        # the same first observation, raw
        assert any(not np.array_equal(bits(x[1][0]), bits(y[1][0])) for x, y in zip(got, trajs))    # and already another first action
    replay(plain, SEED, trajs, bounds)                                                 # the recording is the env's own: raw observations and rewards, the final rows too
    after = (get_stats(a), original(a), a.env_get_state())
    assert stats_equal(keep[0], after[0])                                              # bitwise: nothing merged, nothing moved
    assert all(np.array_equal(x, y) for x, y in zip(keep[1], after[1])) and all(np.array_equal(x, y) for x, y in zip(keep[2], after[2]))
    for h in (a, b, c, plain):
        h.close()


# ---- 5: stochastic draws ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_stochastic_draws_are_those_of_evaluate_agent(pkg, kind):
    L, s = 12, 77
    h = make(pkg, kind, (64, 64), L, fixed_length_episodes=1)
    trajs, lengths, flags, _ = h.collect_trajectory_device(E, deterministic=False, seed=s)
    assert (lengths == L).all() and (flags == TRUNC).all()
    _, er, el, info = h.evaluate_agent_device(n_eval_episodes=E, deterministic=False, seed=s, force_step_granular=True)
    assert info["path"] == 0 and (el == L).all()
    sums = np.zeros(E, F)
    for t in range(L):
        sums = (sums + np.array([trajs[m][2][t] for m in range(E)], F)).astype(F)      # float32, step order; all episodes end at step L: (step, env) order is env order
    assert np.array_equal(bits(sums), bits(er))
    det = h.collect_trajectory_device(E, deterministic=True, seed=s)[0]
    assert any(not np.array_equal(trajs[m][1], det[m][1]) for m in range(E))            # the draws are draws
    plain = make(pkg, kind, (64, 64), L, fixed_length_episodes=1)
    replay(plain, s, trajs, agent_bounds(plain, kind))
    h.close(); plain.close()


# ---- 6: independence ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cartpole", "plugin"])
def test_a_trajectory_depends_on_nothing_but_its_env(pkg, which):
    if which == "cartpole":
        ref = reference(pkg, 0)
        mk = lambda fused=False: make(pkg, 0, (64, 64), ref["limit"])
    else:
        mk = lambda fused=False: make(pkg, 1, (64, 64), 15, module="reacher3_fused", fused=fused)
    h = mk()
    base, base_len, base_flags, _ = h.collect_trajectory_device(E, seed=SEED)
    for M in MS:
        for poll in (1, 7, 0):
            trajs, lengths, flags, info = h.collect_trajectory_device(M, seed=SEED, poll_steps=poll)
            same_trajs(trajs, base, M, (which, M, poll))
            assert np.array_equal(lengths, base_len[:M]) and np.array_equal(flags, base_flags[:M])
            if poll == 1:
                assert info["steps_enqueued"] == lengths.max()                         # K = 1 enqueues nothing past the last finish
    if which == "plugin":
        g = mk(fused=True)
        assert g.rollout_fused_info()["enabled"]
        same_trajs(g.collect_trajectory_device(37, seed=SEED)[0], base, 37, "fused rollout on")
        g.close()
    h.close()


# ---- 7: isolation ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fused", "normalised", "generic", "plugin"])
def test_trajectories_between_training_iterations_change_nothing(pkg, case):
    """test_gpu_eval_device's isolation test with this verb in the evaluation's place: A trains, B trains with recordings after the reset and after each update"""
    n = 24
    normalised = case == "normalised"
    hidden = (32, 48) if case == "generic" else (64, 64)
    kw = dict(monitor_window=30, epochs=2, seed=5, n_envs=n, n_steps=16, batch_size=96, hidden1=hidden[0], hidden2=hidden[1])
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
    recs = []

    def record(h):
        for det in (True, False):
            for M, max_steps in ((1, None), (n, 5), (7, None)):
                recs.append(h.collect_trajectory_device(M, max_steps=max_steps, deterministic=det, seed=1000 + len(recs)))

    for h, with_rec in ((a, False), (b, True)):
        h.set_params(flat); h.env_reset(13)
        if with_rec:
            record(h)
        for _ in range(2):
            h.collect_rollout(); h.ppo_update()
            if with_rec:
                record(h)
    assert len(recs) == 18 and all(np.isfinite(t[2]).all() for r in recs for t in r[0])
    assert a.monitor_stats()[2] > 0                                                    # training episodes are in the window; the recorded ones are not
    assert_bitwise(snapshot(a, normalised), snapshot(b, normalised))
    a.collect_rollout(); b.collect_rollout()                                           # and what follows is the same too (noise stream position, counters)
    assert_bitwise(snapshot(a, normalised), snapshot(b, normalised))
    a.close(); b.close()


def test_a_never_reset_handle_records_and_stays_unreset(pkg):
    capi = pkg._capi
    ref = reference(pkg, 0)
    h = make(pkg, 0, (64, 64), ref["limit"])
    trajs, _, flags, _ = h.collect_trajectory_device(37, seed=SEED)
    assert np.array_equal(flags, ref["flags"][:37])
    for m in range(37):
        assert_traj(trajs[m], ref["want"][m], m)
    for refused in (h.collect_rollout, h.env_observe, lambda: h.env_step(np.ones(E, np.int32))):
        with pytest.raises(pkg.DrilError) as e:
            refused()
        assert e.value.code == capi.ERR_NOT_INITIALISED and "before dril_env_reset" in str(e.value)
    h.close()


@pytest.mark.parametrize("kind,kw", [(0, {}), (1, dict(norm_obs=1, norm_reward=1, norm_training=1))])
def test_ranks_record_their_own_envs_without_an_all_reduce(pkg, kind, kw):
    n = 24
    common = dict(n_steps=4, batch_size=2 * n, episode_len=15 if kind else 60, seed=11, **kw)
    hs = [pkg.Handle(_cfg(pkg, kind, n_envs=n, rank=r, world_size=2, **common)) for r in range(2)]
    pkg.Handle.comm_loopback(hs)
    flat = nudged_params(hs[0], (64, 64))
    out, err = [None, None], [None, None]

    def run(r):
        try:
            hs[r].set_params(flat); hs[r].env_reset(21)
            calls = hs[r].comm_allreduce_calls()
            res = [hs[r].collect_trajectory_device(n, deterministic=det) for det in (True, False)]
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
        one = pkg.Handle(_cfg(pkg, kind, n_envs=n, **{**common, "batch_size": n}))      # the same global env indices in a handle of its own
        one.set_params(flat); one.env_reset(21 + r * n)
        for i, det in enumerate((True, False)):
            want = one.collect_trajectory_device(n, deterministic=det)
            same_trajs(res[i][0], want[0], n, (r, det))
            assert np.array_equal(res[i][1], want[1]) and np.array_equal(res[i][2], want[2])
        one.close()
    assert any(not np.array_equal(x[0], y[0]) for x, y in zip(out[0][0][0][0], out[1][0][0][0]))   # the ranks own different envs


# ---- 8: refusals and the Python mirror ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_healthy(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    n = 24
    h = make(pkg, 0, (64, 64), 20, n_envs=n)
    h.env_reset(3)
    want = h.collect_trajectory_device(n)
    o, info, cap = capi.DrilTrajOptions(), capi.DrilTrajInfo(), C.c_int32()
    obs, act, rew = np.zeros((n, 21, 4), F), np.zeros((n, 20), np.int32), np.zeros((n, 20), F)
    lengths, flags = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    arrays = [p(obs), p(act), p(rew), p(lengths), p(flags)]
    call = lambda opt, arr=arrays: lib.dril_collect_trajectory_device(h._h, opt, *arr, C.byref(info))
    for field, bad in (("n_trajectories", 0), ("n_trajectories", -2), ("n_trajectories", n + 1), ("max_steps", -1), ("poll_steps", -1)):
        lib.dril_traj_options_default(C.byref(o)); o.n_trajectories = n
        setattr(o, field, bad)
        assert call(C.byref(o)) == capi.ERR_INVALID_ARG, field
        assert b"dril_collect_trajectory_device" in lib.dril_last_error(h._h)
    lib.dril_traj_options_default(C.byref(o)); o.n_trajectories = n
    assert call(None) == capi.ERR_INVALID_ARG
    for i in range(5):
        assert call(C.byref(o), arrays[:i] + [None] + arrays[i + 1:]) == capi.ERR_INVALID_ARG, i
    assert lib.dril_collect_trajectory_device(None, C.byref(o), *arrays, None) == capi.ERR_NOT_INITIALISED
    assert lib.dril_trajectory_capacity(h._h, None, C.byref(cap)) == capi.ERR_INVALID_ARG and lib.dril_trajectory_capacity(h._h, C.byref(o), None) == capi.ERR_INVALID_ARG
    for max_steps, want_cap in ((0, 20), (5, 5), (20, 20), (21, 20)):
        o.max_steps = max_steps
        assert lib.dril_trajectory_capacity(h._h, C.byref(o), C.byref(cap)) == capi.OK and cap.value == want_cap
    o.max_steps = 0
    # a recording past 1 GiB on the device: refused before anything is allocated, with its size, M and Tcap
    big = make(pkg, 0, (64, 64), 4_000_000, n_envs=n)
    with pytest.raises(pkg.DrilError) as e:
        big.collect_trajectory_device(n)
    assert e.value.code == capi.ERR_INVALID_ARG and str(4 * n * (4_000_001 * 4 + 2 * 4_000_000) + 5 * n) in str(e.value) and f"M = {n}" in str(e.value) and "Tcap = 4000000" in str(e.value)
    assert len(big.collect_trajectory_device(n, max_steps=6)[0]) == n                   # max_steps bounds the recording
    big.close()
    ext = pkg.Handle(_cfg(pkg, capi.ENV_EXTERNAL, n_envs=2, n_steps=2, batch_size=2, ext_obs_dim=6, ext_action_dim=3, ext_discrete=1))
    with pytest.raises(pkg.DrilError) as e:
        ext.collect_trajectory_device(1)
    assert e.value.code == capi.ERR_UNSUPPORTED and "DRIL_ENV_EXTERNAL" in str(e.value)
    # a failed call leaves the handle healthy; NULL info is legal
    assert lib.dril_collect_trajectory_device(h._h, C.byref(o), *arrays, None) == capi.OK
    assert np.array_equal(lengths, want[1]) and np.array_equal(flags, want[2])
    for m in range(n):
        L = lengths[m]
        assert np.array_equal(obs[m, :L + 1], want[0][m][0]) and np.array_equal(act[m, :L], want[0][m][1]) and np.array_equal(rew[m, :L], want[0][m][2])
        assert not obs[m, L + 1:].any() and not act[m, L:].any() and not rew[m, L:].any()   # rows past the trajectory's length are zero
    h.close()


def test_python_mirror(pkg):
    def fresh(max_steps=60, n=32):
        env = pkg.MonitorWrapperEnv(pkg.DeviceParallelEnv(pkg.CartPoleEnv(max_steps=max_steps), n, seed=3), 20)
        agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space()), pkg.PPO(n_steps=16, batch_size=128, epochs=1), seed=0)
        return env, agent
    env, agent = fresh()
    before = env.bind(agent.alg, agent.layer).monitor_stats()
    import warnings
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        obs, act, rew = pkg.collect_trajectory(agent, env)
    assert not any("Max steps reached" in str(w.message) for w in caught)              # no warning where no trajectory is cut
    assert obs.shape == (len(rew) + 1, 4) and act.shape == rew.shape and 1 <= len(rew) <= 60 and (rew == 1).all()
    assert np.array_equal(env.handle.monitor_stats(), before, equal_nan=True)
    many = pkg.collect_trajectory(agent, env, n_trajectories=5, norm_env=env)
    assert len(many) == 5 and all(np.array_equal(x, y) for x, y in zip(many[0], (obs, act, rew)))
    with pytest.warns(UserWarning, match="Max steps reached"):
        o3, a3, r3 = pkg.collect_trajectory(agent, env, max_steps=3)
    assert len(r3) == 3 and np.array_equal(o3, obs[:4]) and np.array_equal(a3, act[:3])
    sto = pkg.collect_trajectory(agent, env, deterministic=False, seed=9)
    assert np.array_equal(sto[0], pkg.collect_trajectory(agent, env, deterministic=False, seed=9)[0])
    with pytest.raises(NotImplementedError):
        pkg.collect_trajectory(agent, env, norm_env=object())
    with pytest.raises(NotImplementedError):
        pkg.collect_trajectory(agent, pkg.HostParallelEnv([], seed=0))
