"""GPU (-m gpu): NormalizeWrapperEnv / MonitorWrapperEnv around the device-resident envs of a DRIL_ENV_EXTERNAL SAC handle (dril_sac_ext_normalize_* /
dril_sac_ext_monitor_* / dril_sac_ext_collection_begin / dril_sac_ext_wrap_info; docs/sac.md last section), honoured by dril_sac_ext_act_device / _push_device and
dril_sac_predict_actions_device.  Every test begins with one of the new verbs.

The env is the script of tests/test_gpu_ext_wrap.py (pre-drawn observations, rewards, flags and terminal observations for 8 steps, uploaded with tests/hip_mem.py; no
simulator): step 0 has no truncation and terminal_obs = NULL, so has step 5; rows of terminal_obs whose env was not truncated hold NaN.  It runs as 8 collections of
one step (a begin before every act) and as 2 collections of 4.  Steps 0 and 1 draw random actions from injected uniforms, the later ones sample the policy from
injected normals.  The reference is tests/sac_normalize_ref.py (Wrapper, replay_through over the raw ring of a plain twin handle) and tests/ext_wrap_ref.py's Monitor;
tests/sac_ext_wrap_ref.py restates the verb order where a test leaves replay_through's (frozen statistics, a NULL terminal_obs under a truncated flag).

Tolerance: TOL = 3e-5 (rtol = atol), that of tests/test_gpu_ext_wrap.py and tests/test_gpu_env_plugin_normalize.py for the same normaliser core.  Every comparison
prints its largest difference before it asserts."""
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import hip_mem
import sac_normalize_ref as ref
from ext_wrap_ref import Monitor
from sac_ext_wrap_ref import ExtVerbs, run_script
from test_gpu_ext_wrap import _script
from test_gpu_sac_normalize import assert_stats

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
F = np.float32

STEPS, A, N_RANDOM, BATCH = 8, 2, 2, 8
SIZES = [5, 257]                                                                     # a ragged single table row under one wave; several table rows and a tail
DIMS = [1, 24, 133, 300]                                                             # 24: two envs per wave with idle lanes; 133: D > 64, one ragged column tile; 300: two tiles of 256
HIDDEN = (32, 32)
KW = dict(clip_obs=1.25, clip_reward=0.75, gamma=0.9, epsilon=1e-6)
TOL = 3e-5
RB = ("RB_OBSERVATIONS", "RB_ACTIONS", "RB_REWARDS", "RB_TERMINATED", "RB_TRUNCATED", "RB_NEXT_OBSERVATIONS")
STAT_KEYS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count")


class _Spaces:
    """what make_sac_config reads of an external env"""

    def __init__(self, pkg, D):
        self.kind, self._o, self._a = pkg._capi.ENV_EXTERNAL, pkg.Box(low=(-10.0,) * D, high=(10.0,) * D), pkg.Box(low=(-1.0,) * A, high=(1.0,) * A)

    def observation_space(self):
        return self._o

    def action_space(self):
        return self._a


def _handle(pkg, E, D, cap=None, seed=5):
    env = _Spaces(pkg, D)
    alg = pkg.SAC(batch_size=BATCH, buffer_capacity=cap or STEPS * E, learning_rate=3e-3)
    h = pkg.SacHandle(pkg.make_sac_config(env, E, alg, pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=HIDDEN), seed=7))
    h.set_params((np.random.default_rng(seed).standard_normal(h.P) * 0.3).astype(F))
    return h


@functools.lru_cache(maxsize=None)
def _noise(E):
    rng = np.random.default_rng(77 + E)
    n, u = rng.standard_normal((STEPS, E, A)).astype(F), rng.random((STEPS, E, A), dtype=F)
    n.setflags(write=False); u.setflags(write=False)
    return n, u


class _Dev:
    """the script on the device"""

    def __init__(self, E, D):
        sc, up = _script(E, D), hip_mem.to_device
        n, u = _noise(E)
        self.obs = [up(sc["obs"][t]) for t in range(STEPS + 1)]
        self.rew = [up(sc["rew"][t]) for t in range(STEPS)]; self.term = [up(sc["term"][t]) for t in range(STEPS)]; self.trunc = [up(sc["trunc"][t]) for t in range(STEPS)]
        self.tobs = [up(sc["tobs"][t]) if sc["trunc"][t].any() else None for t in range(STEPS)]
        self.noise = [up(u[t]) if t < N_RANDOM else up(n[t]) for t in range(STEPS)]
        self.stored, self.env = hip_mem.empty((E, A), F), hip_mem.empty((E, A), F)


def _step(h, dev, t, tobs="script"):
    h.ext_act_device(dev.obs[t], t < N_RANDOM, dev.noise[t], dev.stored, dev.env)
    h.ext_push_device(dev.rew[t], dev.term[t], dev.trunc[t], dev.obs[t + 1], dev.tobs[t] if tobs == "script" else tobs)


def _run(h, dev, T, first=0, k=None):
    for c in range((STEPS - first) // T if k is None else k):
        h.ext_collection_begin()
        for t in range(first + c * T, first + (c + 1) * T):
            _step(h, dev, t)


def _ring(pkg, h):
    return {n: h.replay(getattr(pkg._capi, n)) for n in RB}


@functools.lru_cache(maxsize=None)
def _plain(E, D):
    """the twin without wrappers over the whole script: its ring (the raw fields replay_through starts from), computed once per shape, shared, never changed"""
    import __graft_entry__ as g
    pkg = g.load_package()
    h, dev = _handle(pkg, E, D), _Dev(E, D)
    launches, last = [], 0
    for t in range(STEPS):
        h.ext_act_device(dev.obs[t], t < N_RANDOM, dev.noise[t], dev.stored, dev.env)
        n = h.ext_device_info()["launches"]; a = n - last; last = n
        h.ext_push_device(dev.rew[t], dev.term[t], dev.trunc[t], dev.obs[t + 1], dev.tobs[t])
        n = h.ext_device_info()["launches"]; launches.append((a, n - last)); last = n
    assert h.flush() == []
    ring = _ring(pkg, h)
    h.close()
    for a in ring.values():
        a.setflags(write=False)
    raw = dict(obs=ring["RB_OBSERVATIONS"].reshape(STEPS, E, D), rew=ring["RB_REWARDS"].reshape(STEPS, E), next=ring["RB_NEXT_OBSERVATIONS"].reshape(STEPS, E, D),
               term=ring["RB_TERMINATED"].reshape(STEPS, E), trunc=ring["RB_TRUNCATED"].reshape(STEPS, E))
    return dict(ring=ring, raw=raw, launches=launches)


def _close(name, got, want, tol=TOL):
    d = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()) if np.size(got) else 0.0
    print(f"{name}: max |difference| = {d:.3e} (tolerance {tol:.0e})")
    np.testing.assert_allclose(got, want, rtol=tol, atol=tol, err_msg=name)


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check_rows(what, got, exp, raw, kw, rows=None):
    """obs / reward / next-obs rows (time-major, the last `rows` of them) against the expected ring"""
    sl = slice(None) if rows is None else slice(-rows, None)
    flat = lambda a: a.reshape((-1,) + a.shape[2:])[sl]
    assert np.isfinite(exp["obs"]).all() and np.isfinite(exp["next"]).all() and np.isfinite(exp["rew"]).all(), "the expected ring is finite"
    if kw["norm_obs"]:
        _close(what + " observations", got["RB_OBSERVATIONS"], flat(exp["obs"]))
        _close(what + " next observations", got["RB_NEXT_OBSERVATIONS"], flat(exp["next"]))
        assert (np.abs(exp["obs"]) == F(KW["clip_obs"])).any() and (np.abs(exp["next"]) == F(KW["clip_obs"])).any(), "the observation clip must be hit"
        assert (np.abs(got["RB_OBSERVATIONS"]) <= F(KW["clip_obs"])).all() and (np.abs(got["RB_NEXT_OBSERVATIONS"]) <= F(KW["clip_obs"])).all()
    else:
        assert _bits(got["RB_OBSERVATIONS"], flat(raw["obs"])) and _bits(got["RB_NEXT_OBSERVATIONS"], flat(raw["next"])), "norm_obs == 0: the raw bits"
    if kw["norm_reward"]:
        _close(what + " rewards", got["RB_REWARDS"], flat(exp["rew"]))
        assert (np.abs(exp["rew"]) == F(KW["clip_reward"])).any() and (np.abs(got["RB_REWARDS"]) <= F(KW["clip_reward"])).all(), "the reward clip must be hit"
    else:
        assert _bits(got["RB_REWARDS"], flat(raw["rew"]))
    assert np.isfinite(got["RB_NEXT_OBSERVATIONS"]).all(), "no NaN row of terminal_obs reached the ring"


# ---- 1. the ring against the NumPy wrapper --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_obs,norm_reward", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("T", [1, 4], ids=["train_freq1", "train_freq4"])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("E", SIZES)
def test_ring_equals_the_numpy_wrapper(pkg, E, D, T, norm_obs, norm_reward):
    capi, sc, plain, k = pkg._capi, _script(E, D), _plain(E, D), STEPS // T
    kw = dict(KW, norm_obs=norm_obs, norm_reward=norm_reward)
    cap = 6 * E + 3 if D == 24 else STEPS * E                                        # D = 24: the ring wraps in the middle of a block of the push kernel
    h, dev = _handle(pkg, E, D, cap), _Dev(E, D)
    h.ext_normalize_enable(**kw)
    assert h.ext_normalize_config() == dict(kw, training=True, clip_obs=F(1.25), clip_reward=F(0.75), gamma=F(0.9), epsilon=F(1e-6))
    st = h.ext_normalize_get_stats()                                                 # a fresh wrapper: mean 0, var 1, counts 0, returns 0
    assert not st["obs_mean"].any() and (st["obs_var"] == 1).all() and st["obs_count"] == 0 and (st["ret_mean"], st["ret_var"], st["ret_count"]) == (0.0, 1.0, 0)
    assert not h.ext_normalize_get_returns().any()
    w = ref.Wrapper(E, D, **kw)
    with np.errstate(invalid="ignore"):
        exp = ref.replay_through(w, plain["raw"], sc["obs"][STEPS], T, k)
    _run(h, dev, T)
    assert h.flush() == []
    info, wi = h.ext_device_info(), h.ext_wrap_info()
    assert info["host_syncs"] == 0 and info["steps_device"] == STEPS and wi["allocations"] == 0 and wi["normalize_on"] == 1 and wi["monitor_on"] == 0
    rows = min(cap, STEPS * E)
    got = _ring(pkg, h)
    what = f"E={E} D={D} T={T} {norm_obs}{norm_reward}"
    _check_rows(what, got, exp, plain["raw"], kw, rows)
    # flags: the plain twin's bits.  Actions: the twin's bits where they do not depend on the observation (the random steps; every step with norm_obs == 0), else
    # what the host verb computes from the ring's own (normalised) observation rows and the same noise
    assert _bits(got["RB_TERMINATED"], plain["ring"]["RB_TERMINATED"][-rows:]) and _bits(got["RB_TRUNCATED"], plain["ring"]["RB_TRUNCATED"][-rows:])
    assert got["RB_TRUNCATED"].sum() >= 2 and got["RB_TERMINATED"].sum() >= 2
    lead = rows % E                                                                  # (a ring that wrapped begins in the middle of a step: the whole steps)
    act, pact = got["RB_ACTIONS"][lead:].reshape(-1, E, A), plain["ring"]["RB_ACTIONS"][-rows:][lead:].reshape(-1, E, A)
    n_rand = max(0, N_RANDOM - (STEPS - act.shape[0]))
    assert n_rand == 0 or _bits(act[:n_rand], pact[:n_rand])
    if norm_obs == 0:
        assert _bits(act, pact)
    else:
        obs_rows, nz = got["RB_OBSERVATIONS"][lead:].reshape(-1, E, D), _noise(E)[0]
        for i in range(n_rand, act.shape[0]):
            t = STEPS - act.shape[0] + i
            assert _bits(act[i], h.predict_actions(obs_rows[i], False, nz[t])[0]), t
        assert not _bits(act[n_rand:], pact[n_rand:])                                # the actor did read the normalised observation
    st = h.ext_normalize_get_stats()
    assert_stats(st, w)
    assert st["obs_count"] == k * E * (T + 1) * norm_obs and st["ret_count"] == k * E * T * norm_reward
    o_obs, o_rew = h.ext_normalize_get_original()
    assert _bits(o_obs, sc["obs"][STEPS]) and _bits(o_rew, sc["rew"][STEPS - 1])
    _close(what + " returns", h.ext_normalize_get_returns(), w.returns)
    assert _bits(dev.obs[STEPS].get(), sc["obs"][STEPS]) and _bits(dev.obs[0].get(), sc["obs"][0])   # the caller's arrays are never written
    # the same configuration up to `training`: statistics and returns stay, training is set; then reset!: returns <- 0, statistics kept
    h.ext_normalize_enable(**dict(kw, training=False))
    st2 = h.ext_normalize_get_stats()
    assert all(np.array_equal(st2[n], st[n]) for n in STAT_KEYS) and h.ext_normalize_config()["training"] is False
    _close(what + " returns kept", h.ext_normalize_get_returns(), w.returns)
    h.ext_normalize_reset()
    assert not h.ext_normalize_get_returns().any() and all(np.array_equal(h.ext_normalize_get_stats()[n], st[n]) for n in STAT_KEYS)
    assert h.ext_device_info()["host_syncs"] == 0
    h.close()


# ---- 2. sync-free, the launch budget, off is the plain handle ------------------------------------------------------------------------------------------------------
def _per_verb_launches(h, dev, T):
    out, last = [], 0
    for c in range(STEPS // T):
        h.ext_collection_begin()
        for t in range(c * T, (c + 1) * T):
            h.ext_act_device(dev.obs[t], t < N_RANDOM, dev.noise[t], dev.stored, dev.env)
            n = h.ext_device_info()["launches"]; a = n - last; last = n
            h.ext_push_device(dev.rew[t], dev.term[t], dev.trunc[t], dev.obs[t + 1], dev.tobs[t])
            n = h.ext_device_info()["launches"]; out.append((a, n - last)); last = n
    return out


@pytest.mark.parametrize("E,D", [(5, 1), (257, 300)])
def test_sync_free_launch_budget_and_off_is_the_plain_handle(pkg, E, D):
    T, plain, dev = 4, _plain(E, D), _Dev(E, D)
    norm, both, mon, off = (_handle(pkg, E, D) for _ in range(4))
    norm.ext_normalize_enable(**KW)
    both.ext_monitor_enable(3); both.ext_normalize_enable(**KW)
    mon.ext_monitor_enable(3)
    off.ext_monitor_enable(3); off.ext_normalize_enable(**KW); off.ext_normalize_enable(False); off.ext_monitor_enable(0)   # enabled, then disabled
    assert off.ext_wrap_info() == dict(normalize_on=0, monitor_on=0, monitor_window=0, launches_act=0, launches_push=0, allocations=0)
    pl = plain["launches"]
    for name, h in (("normalize", norm), ("normalize + monitor", both), ("monitor", mon)):
        got = _per_verb_launches(h, dev, T)
        da, dp = [g[0] - p[0] for g, p in zip(got, pl)], [g[1] - p[1] for g, p in zip(got, pl)]
        print(f"E={E} D={D} {name}: launches added per act {da}, per push {dp} (plain: act {pl[0][0]} / {pl[-1][0]}, push {pl[0][1]})")
        assert all(0 <= x <= 2 for x in da) and all(0 <= x <= 2 for x in dp), "at most two launches more than the plain handle per call"
        info, wi = h.ext_device_info(), h.ext_wrap_info()
        assert info["host_syncs"] == 0 and wi["allocations"] == 0 and (wi["launches_act"], wi["launches_push"]) == (sum(da), sum(dp))
        if name == "monitor":
            assert sum(da) == sum(dp) == 0                                           # the sums ride in the push kernel
        else:
            assert [x for t, x in enumerate(da) if t % T == 0] == [1] * (STEPS // T) and sum(da) == STEPS // T   # the moments of the opening act only
            assert dp == [1] * STEPS                                                 # the moments of every push
        assert h.flush() == [] and h.ext_device_info()["host_syncs"] == 0
    assert _per_verb_launches(off, dev, T) == pl                                     # a handle that switched both off enqueues what one that never had them does
    assert off.flush() == []
    ring = _ring(pkg, off)
    for n in RB:
        assert _bits(ring[n], plain["ring"][n]), n
    m = Monitor(E, 3)
    sc = _script(E, D)
    for t in range(STEPS):
        m.act(sc["rew"][t], sc["term"][t], sc["trunc"][t])
    for h in (both, mon):
        r, l, n = h.ext_monitor_stats()
        assert n == 3 and np.isclose(r, m.stats()[0], rtol=1e-6, atol=1e-6) and l == m.stats()[1]
    for h in (norm, both, mon, off):
        h.close()


@pytest.mark.parametrize("normalize", [False, True], ids=["monitor_alone", "inside_the_normaliser"])
def test_full_monitor_block_is_collected_inside_a_push(pkg, normalize):
    """the block of buffered steps holds 256 rows at 5 envs: the 257th push finds it full and enqueues the window's collection first — one launch more, no host wait,
    the window what the reference's is.  260 steps: the 8-step script played round and round"""
    E, D, W, n_steps, block = 5, 1, 3, 260, 256
    sc, dev = _script(E, D), _Dev(E, D)
    h, plain = _handle(pkg, E, D), _handle(pkg, E, D)
    h.ext_monitor_enable(W)
    if normalize:
        h.ext_normalize_enable(**KW)
    m, extra = Monitor(E, W), []
    for i in range(n_steps):
        t = i % STEPS
        counts = []
        for x in (plain, h):
            n0 = x.ext_device_info()["launches"]
            x.ext_collection_begin()
            x.ext_act_device(dev.obs[t], False, dev.noise[t] if t >= N_RANDOM else dev.noise[N_RANDOM], dev.stored, dev.env)
            n1 = x.ext_device_info()["launches"]
            x.ext_push_device(dev.rew[t], dev.term[t], dev.trunc[t], dev.obs[t + 1], dev.tobs[t])
            counts.append((n1 - n0, x.ext_device_info()["launches"] - n1))
        extra.append((counts[1][0] - counts[0][0], counts[1][1] - counts[0][1]))
        m.act(sc["rew"][t], sc["term"][t], sc["trunc"][t])
    base = 1 if normalize else 0                                                     # the normaliser's moments, per opening act and per push
    print(f"normalize={normalize}: launches added by push {block} (0-based): {extra[block][1]}, by every other push {base}")
    assert [a for a, _ in extra] == [base] * n_steps
    assert [p for _, p in extra] == [base] * block + [base + 1] + [base] * (n_steps - block - 1) and base + 1 <= 2
    wi, info = h.ext_wrap_info(), h.ext_device_info()
    assert info["host_syncs"] == 0 and (wi["launches_act"], wi["launches_push"]) == (base * n_steps, base * n_steps + 1)
    r, l, n = h.ext_monitor_stats()
    wr, wl, wn = m.stats()
    assert n == wn == W and np.isclose(r, wr, rtol=1e-6, atol=1e-6) and np.isclose(l, wl, rtol=1e-6)
    assert h.flush() == [] and plain.flush() == []
    h.close(); plain.close()


# ---- 3. frozen statistics and predict_actions_device ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,D", [(5, 24), (257, 133)])
def test_frozen_statistics_and_predict_actions_device(pkg, E, D):
    sc, T = _script(E, D), 4
    h, dev = _handle(pkg, E, D), _Dev(E, D)
    h.ext_normalize_enable(**KW)
    rng = np.random.default_rng(3)
    given = dict(obs_mean=rng.uniform(-1, 1, D).astype(F), obs_var=rng.uniform(0.5, 4, D).astype(F), obs_count=1000, ret_mean=0.25, ret_var=2.5, ret_count=500)
    h.ext_normalize_set_stats(*(given[n] for n in STAT_KEYS))
    v = ExtVerbs(ref.Wrapper(E, D, **KW)); v.w.set_stats(given)
    # predict: the statistics in force, never updated, whatever `training` says (it is on here); the pending step and the wrapper's caches are not touched
    plain = _handle(pkg, E, D)
    for B in (5, 40):                                                                # 40 > nmax = 16: chunks, the last one partial
        obs, nz = (rng.uniform(-2, 2, (B, D)) * 3).astype(F), rng.standard_normal((B, A)).astype(F)
        d_raw, d_env = hip_mem.empty((B, A), F).fill_bytes(0xFF), hip_mem.empty((B, A), F).fill_bytes(0xFF)
        xn = v.predict_obs(obs)
        assert (np.abs(xn) == F(KW["clip_obs"])).any()
        for det, noise in ((True, None), (False, nz)):
            h.predict_actions_device(hip_mem.to_device(obs), det, None if noise is None else hip_mem.to_device(noise), d_raw, d_env)
            want_raw, want_env = plain.predict_actions(xn, det, noise)
            d = np.abs(d_raw.get() - want_raw).max()
            print(f"E={E} D={D} B={B} deterministic={det}: max |raw action difference| = {d:.3e}")
            assert np.array_equal(d_raw.get(), want_raw) and np.array_equal(d_env.get(), want_env), (B, det)
    st = h.ext_normalize_get_stats()
    assert all(np.array_equal(st[n], given[n]) for n in ("obs_mean", "obs_var")) and st["obs_count"] == 1000 and st["ret_count"] == 500
    assert h.ext_device_info()["steps_device"] == 0 and not h.ext_normalize_get_original()[0].any()
    # one collection with training on, then training off: statistics unchanged to the bit, rows normalised under them, returns change only by the reset of finished envs
    _run(h, dev, T, 0, 1)
    exp0 = run_script(v, sc, T, 1)
    h.ext_normalize_set_training(False); v.w.training = False
    st1, ret1 = h.ext_normalize_get_stats(), h.ext_normalize_get_returns()
    assert st1["obs_count"] == 1000 + E * (T + 1) and st1["ret_count"] == 500 + E * T
    _run(h, dev, T, T, 1)
    exp1 = run_script(v, sc, T, 1, first=T)
    assert h.flush() == []
    st2, ret2 = h.ext_normalize_get_stats(), h.ext_normalize_get_returns()
    assert all(np.array_equal(st2[n], st1[n]) for n in STAT_KEYS)
    done = np.zeros(E, bool)
    for t in range(T, 2 * T):
        done |= (sc["term"][t] | sc["trunc"][t]).astype(bool)
    assert done.any() and (E == 5 or not done.all()) and not ret2[done].any() and _bits(ret2[~done], ret1[~done]) and ret1[done].any()
    exp = {f: np.concatenate([exp0[f], exp1[f]]) for f in exp0}
    raw = run_script(ExtVerbs(), sc, T, 2)
    _check_rows(f"E={E} D={D} frozen", _ring(pkg, h), exp, raw, dict(KW, norm_obs=1, norm_reward=1))
    assert h.ext_device_info()["host_syncs"] == 0
    h.close(); plain.close()


# ---- 4. the monitor's window ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True], ids=["monitor_alone", "inside_the_normaliser"])
@pytest.mark.parametrize("E,D", [(5, 24), (257, 1)])
def test_monitor_window_wraps_and_counts_raw_rewards(pkg, E, D, normalize):
    sc, W = _script(E, D), 3
    h, dev = _handle(pkg, E, D, 5 * E + 2), _Dev(E, D)
    h.ext_monitor_enable(W)
    assert h.ext_monitor_stats()[2] == 0 and np.isnan(h.ext_monitor_stats()[0])
    if normalize:
        h.ext_normalize_enable(**KW)
    m = Monitor(E, W)
    n_eps = 0
    for half in range(2):
        _run(h, dev, 4, 4 * half, 1)
        for t in range(4 * half, 4 * half + 4):
            m.act(sc["rew"][t], sc["term"][t], sc["trunc"][t]); n_eps += int((sc["term"][t] | sc["trunc"][t]).sum())
        if half == 1:
            assert h.flush() == []                                                   # the flush collects what is outstanding; get_stats then finds nothing to add
        r, l, n = h.ext_monitor_stats()
        wr, wl, wn = m.stats()
        print(f"E={E} D={D} normalize={normalize} after {4 * half + 4} steps: window ({r}, {l}, {n}), reference ({wr}, {wl}, {wn}), {n_eps} episodes so far")
        assert n == wn == W and n_eps > W and np.isclose(r, wr, rtol=1e-6, atol=1e-6) and np.isclose(l, wl, rtol=1e-6)
        assert h.ext_monitor_stats() == (r, l, n)                                    # reading twice adds nothing
    info, wi = h.ext_device_info(), h.ext_wrap_info()
    assert info["host_syncs"] == 0 and wi["monitor_on"] == 1 and wi["monitor_window"] == W and wi["normalize_on"] == int(normalize) and wi["allocations"] == 0
    if not normalize:                                                                # the ring is the plain handle's
        plain = _plain(E, D)
        for n in RB:
            assert _bits(h.replay(getattr(pkg._capi, n)), plain["ring"][n][-(5 * E + 2):]), n
    h.ext_monitor_enable(W)                                                          # the same window again: kept
    assert h.ext_monitor_stats()[2] == W
    h.ext_monitor_enable(0)
    with pytest.raises(pkg.DrilError) as e:
        h.ext_monitor_stats()
    assert e.value.code == pkg._capi.ERR_NOT_INITIALISED
    h.close()


# ---- 5. the sticky error under the wrapper -------------------------------------------------------------------------------------------------------------------------
def test_truncation_without_terminal_obs_under_the_wrapper(pkg):
    E, D = 257, 24
    capi, sc = pkg._capi, _script(E, D)
    h, dev = _handle(pkg, E, D), _Dev(E, D)
    h.ext_normalize_enable(**KW)
    h.ext_collection_begin()
    for t in range(3):                                                               # steps 1 and 2 have truncated envs; terminal_obs = NULL throughout
        _step(h, dev, t, tobs=None)
    with pytest.raises(pkg.DrilError) as e:
        h.flush()
    assert e.value.code == capi.ERR_INVALID_ARG and "terminal_obs" in str(e.value)
    assert h.flush() == []                                                           # returned once, then cleared
    v = ExtVerbs(ref.Wrapper(E, D, **KW))
    exp = run_script(v, sc, 3, 1, tobs_none=(0, 1, 2))
    assert sc["trunc"][1].any() and sc["trunc"][2].any()
    got = _ring(pkg, h)
    _close("next observations: the normalised next obs where the terminal observation belongs", got["RB_NEXT_OBSERVATIONS"], exp["next"].reshape(-1, D))
    _close("observations", got["RB_OBSERVATIONS"], exp["obs"].reshape(-1, D)); _close("rewards", got["RB_REWARDS"], exp["rew"].reshape(-1))
    assert_stats(h.ext_normalize_get_stats(), v.w)                                   # the statistics updates are kept
    for t in range(3, 6):                                                            # the handle stays usable: the same collection goes on, correctly now
        _step(h, dev, t)
    assert h.flush() == [] and h.replay_size() == 6 * E
    h.close()


def test_collection_goes_on_across_a_flush(pkg):
    """a flush or a sticky error does not end a collection: the later acts need no begin and update nothing"""
    E, D = 5, 24
    sc = _script(E, D)
    h, dev = _handle(pkg, E, D), _Dev(E, D)
    h.ext_normalize_enable(**KW)
    h.ext_collection_begin()
    v = ExtVerbs(ref.Wrapper(E, D, **KW)); v.collection_begin()
    rows = []
    for t in range(4):
        _step(h, dev, t)
        assert h.flush() == []
        v.act(sc["obs"][t]); rows.append(v.push(sc["rew"][t], sc["term"][t], sc["trunc"][t], sc["obs"][t + 1], sc["tobs"][t] if sc["trunc"][t].any() else None))
    st = h.ext_normalize_get_stats()
    assert st["obs_count"] == E * 5 and st["ret_count"] == E * 4
    assert_stats(st, v.w)
    _close("observations", h.replay(pkg._capi.RB_OBSERVATIONS), np.concatenate([r["obs"] for r in rows]))
    h.close()


# ---- 6. refusals and statuses --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_statuses(pkg):
    capi = pkg._capi
    E, D = 5, 24
    h, dev = _handle(pkg, E, D), _Dev(E, D)
    f, H = h._f, h._h
    P = lambda a: None if a is None else C.c_void_p(a.ptr)
    msg = lambda: (f("last_error")(H) or b"").decode()
    INV, NI, UNS = capi.ERR_INVALID_ARG, capi.ERR_NOT_INITIALISED, capi.ERR_UNSUPPORTED
    obs, rew, te, tr, out = P(dev.obs[0]), P(dev.rew[0]), P(dev.term[0]), P(dev.trunc[0]), P(dev.env)
    cfg = capi.DrilSacNormalizeConfig()
    # the wrapper is off
    info = capi.DrilSacExtWrapInfo()
    assert f("ext_wrap_info")(H, C.byref(info)) == capi.OK and (info.normalize_on, info.monitor_on) == (0, 0)
    for verb, call in (("ext_normalize_get_config", lambda: f("ext_normalize_get_config")(H, C.byref(cfg))), ("ext_normalize_set_training", lambda: f("ext_normalize_set_training")(H, 1)),
                       ("ext_normalize_get_returns", lambda: f("ext_normalize_get_returns")(H, None)), ("ext_normalize_reset", lambda: f("ext_normalize_reset")(H, None)),
                       ("ext_normalize_get_original", lambda: f("ext_normalize_get_original")(H, None, None)), ("ext_monitor_get_stats", lambda: f("ext_monitor_get_stats")(H, None, None, None))):
        assert call() == NI and msg().startswith("dril_sac_" + verb), (verb, msg())
    assert f("ext_normalize_enable")(H, None) == capi.OK and f("ext_collection_begin")(H) == capi.OK                 # off: nothing to do, a no-op
    assert f("ext_act_device")(H, obs, 0, None, None, out, None) == capi.OK and f("ext_push_device")(H, rew, te, tr, obs, None, None) == capi.OK   # a plain handle needs no begin
    # bad configurations: the handle is left as it was
    for field, val in (("clip_obs", -1.0), ("clip_reward", float("nan")), ("epsilon", -1e-3), ("epsilon", float("nan")), ("clip_obs", float("nan"))):
        assert f("normalize_config_default")(C.byref(cfg)) == capi.OK
        setattr(cfg, field, val)
        assert f("ext_normalize_enable")(H, C.byref(cfg)) == INV and field.split("_")[0] in msg(), (field, msg())
    assert f("ext_monitor_enable")(H, -1) == INV
    assert h.ext_wrap_info()["normalize_on"] == 0 and h.ext_wrap_info()["monitor_on"] == 0
    # the built-in families stay refused on an external handle
    assert f("normalize_config_default")(C.byref(cfg)) == capi.OK
    assert f("normalize_enable")(H, C.byref(cfg)) == UNS and f("monitor_enable")(H, 3) == UNS and f("normalize_get_config")(H, C.byref(cfg)) == UNS
    # wrapper on: an act needs a collection; enable / disable / set_stats / reset with an act pending are refused; the host push is refused
    h.ext_normalize_enable(**KW)
    assert f("ext_act_device")(H, obs, 0, None, None, out, None) == NI and "dril_sac_ext_collection_begin" in msg()
    assert h.ext_device_info()["launches"] == 5 + 1                                  # (the plain step above: copy, three forward launches, head; push) nothing was enqueued by the refused act
    h.ext_collection_begin()
    assert f("ext_act_device")(H, obs, 0, None, None, out, None) == capi.OK
    assert f("ext_normalize_enable")(H, None) == INV and "pending" in msg()
    assert f("normalize_config_default")(C.byref(cfg)) == capi.OK and f("ext_normalize_enable")(H, C.byref(cfg)) == INV and f("ext_monitor_enable")(H, 3) == INV
    assert f("ext_normalize_reset")(H, None) == INV
    assert h.ext_wrap_info()["normalize_on"] == 1 and h.ext_wrap_info()["monitor_on"] == 0 and h.ext_normalize_config()["clip_obs"] == F(1.25)
    z = np.zeros(E, F)
    with pytest.raises(pkg.DrilError):
        h.ext_push(np.zeros((E, D)), np.zeros((E, A)), z, z, z, np.zeros((E, D)))
    assert f("ext_push_device")(H, rew, te, tr, obs, None, None) == capi.OK
    with pytest.raises(pkg.DrilError) as e:                                          # no act pending, the wrapper still on
        h.ext_push(np.zeros((E, D)), np.zeros((E, A)), z, z, z, np.zeros((E, D)))
    assert e.value.code == UNS and "use the device verbs, or wrap the host env on the host" in str(e.value)
    # set_stats and reset end the collection
    st = h.ext_normalize_get_stats()
    h.ext_normalize_set_stats(*(st[n] for n in STAT_KEYS))
    assert f("ext_act_device")(H, obs, 0, None, None, out, None) == NI
    h.ext_collection_begin(); _step(h, dev, 0); h.ext_normalize_reset()
    assert f("ext_act_device")(H, obs, 0, None, None, out, None) == NI
    assert f("ext_normalize_get_stats")(H, None, None, None, None, None, None) == INV and f("ext_normalize_set_stats")(H, None, None, 0, 0.0, 1.0, 0) == INV
    om = np.zeros(D, F)
    assert f("ext_normalize_set_stats")(H, om.ctypes.data_as(C.c_void_p), om.ctypes.data_as(C.c_void_p), -1, 0.0, 1.0, 0) == INV
    h.ext_normalize_enable(False); h.ext_monitor_enable(3); h.ext_monitor_enable(0)
    h.ext_push(np.zeros((E, D)), np.zeros((E, A)), z, z, z, np.zeros((E, D)))       # wrappers off: the host verb works again
    assert h.flush() == []
    h.close()
    # every new verb on a device-env handle: DRIL_ERR_UNSUPPORTED, with a message that points to the built-in family
    env = pkg.PendulumEnv(max_steps=200)
    hp = pkg.SacHandle(pkg.make_sac_config(env, 8, pkg.SAC(batch_size=BATCH, buffer_capacity=64), pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(32, 32))))
    f, H = hp._f, hp._h
    assert f("normalize_config_default")(C.byref(cfg)) == capi.OK
    calls = {"ext_normalize_enable": lambda: f("ext_normalize_enable")(H, C.byref(cfg)), "ext_normalize_get_config": lambda: f("ext_normalize_get_config")(H, C.byref(cfg)),
             "ext_normalize_set_training": lambda: f("ext_normalize_set_training")(H, 1), "ext_normalize_get_stats": lambda: f("ext_normalize_get_stats")(H, None, None, None, None, None, None),
             "ext_normalize_set_stats": lambda: f("ext_normalize_set_stats")(H, None, None, 0, 0.0, 1.0, 0), "ext_normalize_get_original": lambda: f("ext_normalize_get_original")(H, None, None),
             "ext_normalize_get_returns": lambda: f("ext_normalize_get_returns")(H, None), "ext_normalize_reset": lambda: f("ext_normalize_reset")(H, None),
             "ext_collection_begin": lambda: f("ext_collection_begin")(H), "ext_monitor_enable": lambda: f("ext_monitor_enable")(H, 3),
             "ext_monitor_get_stats": lambda: f("ext_monitor_get_stats")(H, None, None, None), "ext_wrap_info": lambda: f("ext_wrap_info")(H, C.byref(info))}
    for verb, call in calls.items():
        assert call() == UNS, verb
        m = (f("last_error")(H) or b"").decode()
        assert m.startswith("dril_sac_" + verb + ":") and "DRIL_ENV_EXTERNAL" in m, (verb, m)
        if verb.startswith("ext_normalize_") and verb != "ext_normalize_reset" or verb == "ext_monitor_enable":
            assert "dril_sac_normalize_enable" in m or "dril_sac_monitor_enable" in m, (verb, m)
    hp.close()


# ---- 7. update_enqueue after wrapped pushes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,D", [(5, 24), (257, 133)])
def test_enqueued_updates_after_wrapped_pushes(pkg, E, D):
    """dril_sac_update_enqueue over the ring the wrapped pushes wrote, against dril_sac_update on twin handles filled through dril_sac_replay_fill, the same injected
    batches and noise.  test_enqueued_updates_are_the_updates compares the two verbs bit for bit over ONE ring; here the ring comes from the wrapped pushes, so the
    comparison has the two links of that chain, each at its own tolerance and no wider:
      1. the wrapped ring equals the NumPy-normalised rows within TOL = 3e-5 — all the ring inputs may differ by;
      2. enqueued updates over that ring equal dril_sac_update on a twin filled with the ring's OWN bytes BIT FOR BIT: statistics rows, parameters, targets, entropy
         coefficient — the tolerance of test_enqueued_updates_are_the_updates, unchanged.
    A second twin holds the NumPy-normalised rows themselves.  Its statistics (losses, mean Q, entropy coefficient, gradient norm) are smooth in the ring, so they
    are asserted at gain x TOL, the gain bounded by the product of the three layers' spectral norms of a 32 x 32 net with weights of standard deviation 0.3, about
    (0.3 sqrt(32))^2 x 0.3 sqrt(D + A) < 30: rtol = atol = 1e-3.  Its parameters are printed, not asserted: an Adam step moves a coordinate by lr x g / (|g| + eps),
    which is not continuous in g at 0, so no bound tied to 3e-5 holds for every coordinate — link 2 carries the parameters.
    Measured on an MI355X: ring rows against NumPy at most 1.2e-7 (E=5, D=24) and 3.6e-7 (E=257, D=133); link 2 bit-equal; against the NumPy-filled twin (E=5, D=24) statistics
    differ by at most 1.9e-6 and parameters by at most 6.0e-8, (E=257, D=133) statistics by at most 3.4e-3 in absolute terms on a value of order ten (inside
    rtol = 1e-3), parameters by at most 3.1e-6 (median 0)."""
    capi, sc, n_upd = pkg._capi, _script(E, D), 2
    h, own, twin, dev = _handle(pkg, E, D), _handle(pkg, E, D), _handle(pkg, E, D), _Dev(E, D)
    h.ext_normalize_enable(**KW)
    _run(h, dev, 4)
    ring = _ring(pkg, h)
    exp = run_script(ExtVerbs(ref.Wrapper(E, D, **KW)), sc, 4, 2)
    _close(f"E={E} D={D} ring observations", ring["RB_OBSERVATIONS"], exp["obs"].reshape(-1, D)); _close(f"E={E} D={D} ring rewards", ring["RB_REWARDS"], exp["rew"].reshape(-1))
    _close(f"E={E} D={D} ring next observations", ring["RB_NEXT_OBSERVATIONS"], exp["next"].reshape(-1, D))
    assert _bits(ring["RB_TERMINATED"], exp["term"].reshape(-1)) and _bits(ring["RB_TRUNCATED"], exp["trunc"].reshape(-1))
    own.replay_fill(ring["RB_OBSERVATIONS"], ring["RB_ACTIONS"], ring["RB_REWARDS"], ring["RB_TERMINATED"], ring["RB_TRUNCATED"], ring["RB_NEXT_OBSERVATIONS"])
    twin.replay_fill(exp["obs"].reshape(-1, D), ring["RB_ACTIONS"], exp["rew"].reshape(-1), ring["RB_TERMINATED"], ring["RB_TRUNCATED"], exp["next"].reshape(-1, D))
    rng = np.random.default_rng(11)
    idx = rng.integers(0, STEPS * E, (n_upd, BATCH)).astype(np.int64)
    ne, nn, npi = (rng.standard_normal((n_upd, BATCH, A)).astype(F) for _ in range(3))
    for x in (h, own, twin):
        x.set_batches(n_upd, idx, ne, nn, npi)
    h.update_enqueue(n_upd)
    assert h.ext_device_info()["host_syncs"] == 0 and h.ext_device_info()["pending_updates"] == n_upd
    got, same, want = h.flush(), own.update(n_upd), twin.update(n_upd)
    fields = ("actor_loss", "critic_loss", "entropy_loss", "mean_q_values", "entropy_coefficient", "grad_norm", "has_entropy_loss")
    rows = lambda st: [tuple(getattr(s_, k) for k in fields) for s_ in st]
    assert len(got) == n_upd and rows(got) == rows(same)                             # link 2: bit for bit
    assert np.array_equal(h.get_params(), own.get_params()) and np.array_equal(h.get_target_params(), own.get_target_params()) and h.get_log_ent_coef() == own.get_log_ent_coef()
    assert not np.array_equal(h.get_params(), (np.random.default_rng(5).standard_normal(h.P) * 0.3).astype(F))   # the updates moved the parameters
    g, w_ = np.array(rows(got), np.float64)[:, :6], np.array(rows(want), np.float64)[:, :6]
    dp = np.abs(h.get_params() - twin.get_params())
    used = float((np.abs(g - w_) / (1e-3 + 1e-3 * np.abs(w_))).max())
    print(f"E={E} D={D}: against the NumPy-filled twin: statistics max |difference| = {np.abs(g - w_).max():.3e}, {used:.3f} of the tolerance (rtol = atol = 1e-3); parameters max {dp.max():.3e}, median {np.median(dp):.3e}")
    assert np.isfinite(g).all()
    np.testing.assert_allclose(g, w_, rtol=1e-3, atol=1e-3)
    for x in (h, own, twin):
        x.close()


# ---- 8. the Python mirror ------------------------------------------------------------------------------------------------------------------------------------------
class _ScriptedDeviceEnv:
    """ONE batched env on hip_mem arrays that plays the script whatever the actions are"""

    def __init__(self, pkg, E, D):
        self.pkg, self.n_envs, self.D, self.t, self.dev = pkg, E, D, 0, _Dev(E, D)

    def observation_space(self):
        return self.pkg.Box(low=(-10.0,) * self.D, high=(10.0,) * self.D)

    def action_space(self):
        return self.pkg.Box(low=(-1.0,) * A, high=(1.0,) * A)

    def reset_(self):
        pass

    def observe(self):
        return self.dev.obs[self.t]

    def act_(self, actions):
        t = self.t; self.t += 1
        return self.dev.rew[t], self.dev.term[t], self.dev.trunc[t], self.dev.tobs[t]


@pytest.mark.parametrize("train_freq", [1, 2])
def test_python_mirror_trains_under_both_wrappers(pkg, train_freq):
    E, D, W = 5, 24, 3
    sc = _script(E, D)
    env = pkg.NormalizeWrapperEnv(pkg.MonitorWrapperEnv(pkg.DeviceArrayParallelEnv(_ScriptedDeviceEnv(pkg, E, D), seed=3, empty=hip_mem.empty), W), **KW)
    alg = pkg.SAC(start_steps=0, train_freq=train_freq, gradient_steps=2, batch_size=BATCH, buffer_capacity=STEPS * E, learning_rate=3e-3)
    agent = pkg.SACAgent(pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=HIDDEN), alg, seed=0)
    iters = 6 // train_freq
    agent, rb, stats, timer = pkg.sac_train_(agent, env, alg, iters * train_freq * E)
    h = rb.handle
    assert timer["host_syncs"] == 0 and timer["iterations"] == iters and h.ext_device_info()["steps_device"] == 6 and len(stats["critic_losses"]) == 2 * iters
    assert env.wrapper_handle() is h and h.ext_wrap_info()["normalize_on"] == 1 and h.ext_wrap_info()["monitor_window"] == W and h.ext_wrap_info()["allocations"] == 0
    v = ExtVerbs(ref.Wrapper(E, D, **KW), Monitor(E, W))
    exp = run_script(v, sc, train_freq, iters)
    st = h.ext_normalize_get_stats()
    assert_stats(st, v.w)
    assert st["obs_count"] == iters * E * (train_freq + 1) and st["ret_count"] == 6 * E
    _close("ring observations", h.replay(pkg._capi.RB_OBSERVATIONS), exp["obs"].reshape(-1, D)); _close("ring rewards", h.replay(pkg._capi.RB_REWARDS), exp["rew"].reshape(-1))
    _close("ring next observations", h.replay(pkg._capi.RB_NEXT_OBSERVATIONS), exp["next"].reshape(-1, D))
    r, l, n = h.ext_monitor_stats()
    wr, wl, wn = v.mon.stats()
    assert (r, l, n) == env.monitor_stats() and n == wn == W and np.isclose(r, wr, rtol=1e-6, atol=1e-6) and np.isclose(l, wl)
    # the helpers answer from the SAC handle: statistics, originals, extract_policy(agent, env)
    assert _bits(pkg.get_original_obs(env), sc["obs"][6]) and _bits(pkg.get_original_rewards(env), sc["rew"][5])
    pol = pkg.extract_policy(agent, env)
    obs = (np.random.default_rng(4).uniform(-2, 2, (7, D)) * 3).astype(F)
    want = h.predict_actions(v.w.normalize_obs(obs), True)[1]
    got = np.stack([np.asarray(a, F) for a in pol(list(obs), deterministic=True)])
    _close("extract_policy(agent, env) against predict on normalised observations", got, want, 1e-4)
    assert not np.allclose(got, h.predict_actions(obs, True)[1], atol=1e-3)         # not the raw observation
    pol.close()
    # evaluation: frozen statistics from the training handle, raw returns; no statistics given: the RuntimeWarning of the built-in path
    ev = pkg.NormalizeWrapperEnv(pkg.DeviceArrayParallelEnv(_ScriptedDeviceEnv(pkg, E, D), seed=3, empty=hip_mem.empty), **KW)
    er, el = pkg.sac_evaluate_agent(agent, ev, n_eval_episodes=3, deterministic=True, return_stats=False, normalize_stats=h)
    m = Monitor(E, 100)
    for t in range(STEPS):
        m.act(sc["rew"][t], sc["term"][t], sc["trunc"][t])
        if len(m.window) >= 3:
            break
    assert np.array_equal(er, np.asarray([w_[0] for w_ in m.window[:3]], F)) and list(el) == [w_[1] for w_ in m.window[:3]]
    assert all(np.array_equal(h.ext_normalize_get_stats()[k], st[k]) for k in STAT_KEYS)   # the training statistics were read, not changed
    ev2 = pkg.NormalizeWrapperEnv(pkg.DeviceArrayParallelEnv(_ScriptedDeviceEnv(pkg, E, D), seed=3, empty=hip_mem.empty), **KW)
    with pytest.warns(RuntimeWarning, match="normalize_stats"):
        pkg.sac_evaluate_agent(agent, ev2, n_eval_episodes=1)
    # a second run on the handle that comes back through the replay buffer keeps its statistics
    env.env.t = 6
    pkg.sac_train_(agent, env, alg, train_freq * E, replay_buffer=rb)
    assert h.ext_normalize_get_stats()["obs_count"] == st["obs_count"] + E * (train_freq + 1)
    with pytest.raises(NotImplementedError, match="normalize"):
        pkg.sac_train_(agent, env, alg, E, normalize=dict())
    h.close()


def test_torch_example_trains_under_both_flags(pkg):
    torch = pytest.importorskip("torch", reason="the example env is written in torch")
    if not torch.cuda.is_available():
        pytest.skip("torch.cuda.is_available() is false on this machine: the torch example env needs torch's own GPU runtime (every other test of this file uses tests/hip_mem.py)")
    r = subprocess.run([sys.executable, str(ROOT / "examples" / "sac_torch_envs.py"), "--iterations", "40", "--envs", "64", "--normalize", "--monitor"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "host_syncs=0" in r.stdout and "obs_count=" in r.stdout and "ep_rew_mean=" in r.stdout, r.stdout[-2000:]
