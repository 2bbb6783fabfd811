"""GPU (-m gpu): NormalizeWrapperEnv / MonitorWrapperEnv around the envs of a DRIL_ENV_EXTERNAL PPO handle, honoured by the device-array verbs
(dril_ext_normalize_* / dril_ext_monitor_* / dril_ext_wrap_info; docs/external_envs.md section 10, "Wrappers on device-resident arrays").  Every test begins with one of the new verbs.

The env is a script (pre-drawn observations, rewards, flags and terminal observations per step, uploaded with tests/hip_mem.py; no simulator), two rollouts of
T = 4 steps in a row because statistics and `returns` carry over.  The reference is tests/sac_normalize_ref.py's Wrapper (the reference's float32 arithmetic and
call order, batch moments from float64 sums) and tests/ext_wrap_ref.py's Monitor.

Tolerances: TOL = 3e-5 (rtol = atol) is tests/test_gpu_env_plugin_normalize.py's for this same normaliser core; values against predict_values of the row the buffer
holds 1e-4, bootstrap and last values against predict_values of the NumPy-normalised observation 2e-4 (the normalised input differs by up to TOL between the two).
Every comparison prints its largest difference before it asserts."""
import ctypes as C
import functools
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import hip_mem
import sac_normalize_ref as ref
from ext_wrap_ref import Monitor
from test_gpu_sac_normalize import assert_stats

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
F = np.float32

T, K, A = 4, 2, 2                                                                    # steps per rollout, rollouts in a row, Box action dims
SIZES = [5, 257]                                                                     # one table row with a tail; 17 rows and two apply blocks
DIMS = [1, 24, 133]                                                                  # 133: three column tiles of 64, the last one ragged
HIDDEN = (32, 48)
KW = dict(clip_obs=1.25, clip_reward=0.75, gamma=0.9, epsilon=1e-6)
TOL = 3e-5


def _cfg(pkg, E, D, **kw):
    c = pkg._capi.default_config(pkg._capi.ENV_EXTERNAL)
    c.ext_obs_dim, c.ext_action_dim, c.ext_discrete, c.hidden1, c.hidden2 = D, A, 0, HIDDEN[0], HIDDEN[1]
    c.ext_action_low, c.ext_action_high = -1.0, 1.0
    c.n_envs, c.n_steps, c.batch_size, c.epochs, c.seed = E, T, E, 1, 11
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _handle(pkg, E, D, seed=5):
    h = pkg.Handle(_cfg(pkg, E, D))
    h.set_params((np.random.default_rng(seed).standard_normal(h.P) * 0.3).astype(F))
    return h


@functools.lru_cache(maxsize=None)
def _script(E, D, steps=K * T):
    """obs[g] (steps + 1: obs[c T + T] closes rollout c and opens rollout c + 1), rew, term, trunc, tobs per step, the sampling noise.
    step 0: env 0 terminates, nobody is truncated (terminal_obs is NULL there); step 1: env 1 and the LAST env (the grid tail) are truncated only; step 2: env 2 is
    terminated AND truncated, the last env terminates; from step 3 on a termination and a truncation per step, except step 5: nothing is truncated again.
    Rows of terminal_obs whose env was not truncated hold NaN: they must never be selected."""
    rng = np.random.default_rng(2000 + 7 * E + D)
    obs = (rng.uniform(-2, 2, (steps + 1, E, D)) * rng.uniform(0.5, 3.0, D) + rng.uniform(-1, 1, D)).astype(F)
    rew = (2.0 * rng.standard_normal((steps, E))).astype(F)
    term, trunc = np.zeros((steps, E), np.uint8), np.zeros((steps, E), np.uint8)
    term[0, 0] = 1; trunc[1, 1 % E] = 1; term[2, 2 % E] = trunc[2, 2 % E] = 1
    trunc[1, E - 1] = 1; term[2, E - 1] = 1
    for t in range(3, steps):
        term[t, (t + 1) % E] = 1
        if t != 5:
            trunc[t, (t + 3) % E] = 1
    tobs = (rng.uniform(-2, 2, (steps, E, D)) * 2.0).astype(F)
    tobs[trunc == 0] = np.nan
    noise = (3.0 * rng.standard_normal((steps * E, A))).astype(F)
    for a in (obs, rew, term, trunc, tobs, noise):
        a.setflags(write=False)
    return dict(obs=obs, rew=rew, term=term, trunc=trunc, tobs=tobs, noise=noise)


class _Dev:
    """the script on the device"""

    def __init__(self, E, D, steps=K * T):
        sc = _script(E, D, steps)
        up = hip_mem.to_device
        self.obs = [up(sc["obs"][t]) for t in range(steps + 1)]
        self.rew = [up(sc["rew"][t]) for t in range(steps)]; self.term = [up(sc["term"][t]) for t in range(steps)]; self.trunc = [up(sc["trunc"][t]) for t in range(steps)]
        self.tobs = [up(sc["tobs"][t]) if sc["trunc"][t].any() else None for t in range(steps)]
        self.raw, self.env = hip_mem.empty((E, A), F), hip_mem.empty((E, A), F)
        self.zeros = hip_mem.to_device(np.zeros(E, np.uint8))


def _rollout(h, dev, c):
    """rollout c of the script through the device verbs -> (dril_ext_device_info, dril_ext_wrap_info) as they stand before finish"""
    for t in range(c * T, (c + 1) * T):
        h.ext_act_device(dev.obs[t], dev.raw, dev.env)
        h.ext_record_device(dev.rew[t], dev.term[t], dev.trunc[t], dev.tobs[t])
    before = (h.ext_device_info(), h.ext_wrap_info())
    h.ext_finish_device(dev.obs[(c + 1) * T])
    return before


def _expected(E, D, c_done, **kw):
    """the NumPy wrapper run over the first c_done rollouts of the script -> (wrapper, per rollout: obs rows, reward rows, normalised terminal obs, last obs)"""
    sc = _script(E, D)
    w = ref.Wrapper(E, D, **kw)
    out = []
    with np.errstate(invalid="ignore"):
        for c in range(c_done):
            o, r, tb = [], [], []
            for t in range(c * T, (c + 1) * T):
                o.append(w.observe(sc["obs"][t]))
                rn, tn = w.act(sc["rew"][t], sc["term"][t], sc["trunc"][t], sc["tobs"][t])
                r.append(rn); tb.append(tn)
            out.append(dict(obs=np.stack(o), rew=np.stack(r), tobs=np.stack(tb), last=w.observe(sc["obs"][(c + 1) * T])))
    return w, out


def _close(name, got, want, tol):
    d = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()) if np.size(got) else 0.0
    print(f"{name}: max |difference| = {d:.3e} (tolerance {tol:.0e})")
    np.testing.assert_allclose(got, want, rtol=tol, atol=tol, err_msg=name)


def _check_rollout(pkg, h, E, D, c, exp, kw):
    capi, sc = pkg._capi, _script(E, D)
    sl = slice(c * T, (c + 1) * T)
    buf = lambda n: h.buffer(getattr(capi, "BUF_" + n))
    obs, rew, fl = buf("OBSERVATIONS").reshape(T, E, D), buf("REWARDS").reshape(T, E), buf("FLAGS").reshape(T, E)
    what = f"E={E} D={D} {kw} rollout {c}"
    if kw["norm_obs"]:
        _close(what + " observations", obs, exp["obs"], TOL)
        assert (np.abs(exp["obs"]) == F(KW["clip_obs"])).any() and (np.abs(obs) <= F(KW["clip_obs"])).all(), "the observation clip must be hit"
    else:
        assert np.array_equal(obs.view(np.uint32), sc["obs"][sl].view(np.uint32)), "norm_obs == 0: the raw bits"
    if kw["norm_reward"]:
        _close(what + " rewards", rew, exp["rew"], TOL)
        assert (np.abs(exp["rew"]) == F(KW["clip_reward"])).any() and (np.abs(rew) <= F(KW["clip_reward"])).all(), "the reward clip must be hit"
    else:
        assert np.array_equal(rew.view(np.uint32), sc["rew"][sl].view(np.uint32))
    assert np.array_equal(fl, sc["term"][sl] | (sc["trunc"][sl] << 1))
    tr = sc["trunc"][sl] != 0
    boot = buf("BOOTSTRAP").reshape(T, E)
    assert np.isfinite(boot).all() and (boot[~tr] == 0).all(), "no NaN row was selected; 0 where not truncated"
    want = h.predict_values(exp["tobs"][tr]) if kw["norm_obs"] else h.predict_values(sc["tobs"][sl][tr])
    _close(what + " bootstrap", boot[tr], want, 2e-4)
    _close(what + " last values", buf("LAST_VALUES"), h.predict_values(exp["last"]), 2e-4)
    _close(what + " values", buf("VALUES"), h.predict_values(obs.reshape(T * E, D)), 1e-4)
    assert np.isfinite(buf("ADVANTAGES")).all() and np.isfinite(buf("RETURNS")).all()


# ---- 1. the buffer against the NumPy wrapper ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_obs,norm_reward", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("E", SIZES)
def test_buffer_equals_the_numpy_wrapper(pkg, E, D, norm_obs, norm_reward):
    kw = dict(KW, norm_obs=norm_obs, norm_reward=norm_reward)
    h = _handle(pkg, E, D)
    h.ext_normalize_enable(**kw)
    assert h.ext_normalize_config() == dict(kw, training=True, clip_obs=F(1.25), clip_reward=F(0.75), gamma=F(0.9), epsilon=F(1e-6))
    st = h.ext_normalize_get_stats()                                                 # a fresh wrapper: mean 0, var 1, counts 0, returns 0
    assert not st["obs_mean"].any() and (st["obs_var"] == 1).all() and st["obs_count"] == 0 and (st["ret_mean"], st["ret_var"], st["ret_count"]) == (0.0, 1.0, 0)
    assert not h.ext_normalize_get_returns().any()
    sc, dev = _script(E, D), _Dev(E, D)
    for c in range(K):
        w, exp = _expected(E, D, c + 1, **kw)
        info, wi = _rollout(h, dev, c)
        assert info["host_syncs"] == 0 and info["steps_device"] == T and wi["allocations"] == 0 and wi["normalize_on"] == 1 and wi["monitor_on"] == 0
        _check_rollout(pkg, h, E, D, c, exp[c], kw)
        st = h.ext_normalize_get_stats()
        assert_stats(st, w)
        assert st["obs_count"] == (c + 1) * E * (T + 1) * norm_obs and st["ret_count"] == (c + 1) * E * T * norm_reward
        o_obs, o_rew = h.ext_normalize_get_original()
        assert np.array_equal(o_obs.view(np.uint32), sc["obs"][(c + 1) * T].view(np.uint32)) and np.array_equal(o_rew.view(np.uint32), sc["rew"][(c + 1) * T - 1].view(np.uint32))
        _close(f"E={E} D={D} returns", h.ext_normalize_get_returns(), w.returns, TOL)
    h.ext_normalize_reset()                                                          # reset! of the wrapper: returns <- 0, statistics kept
    assert not h.ext_normalize_get_returns().any()
    st2 = h.ext_normalize_get_stats()
    assert np.array_equal(st2["obs_mean"], st["obs_mean"]) and st2["ret_var"] == st["ret_var"] and st2["obs_count"] == st["obs_count"]
    h.ext_normalize_enable(**dict(kw, training=False))                               # the same configuration up to `training`: statistics stay, training is set
    st3 = h.ext_normalize_get_stats()
    assert np.array_equal(st3["obs_var"], st["obs_var"]) and st3["ret_count"] == st["ret_count"] and h.ext_normalize_config()["training"] is False
    h.close()


# ---- 2. sync-free, no allocation, the launch budget; 3. off is the parent ------------------------------------------------------------------------------------
def _per_verb_launches(h, dev, c, sc):
    """launches (dril_ext_device_info) enqueued by each call of rollout c -> (act list, record list, finish)"""
    h.set_noise(sc["noise"][c * T * h.E:(c + 1) * T * h.E])
    acts, recs, last = [], [], 0
    for t in range(c * T, (c + 1) * T):
        h.ext_act_device(dev.obs[t], dev.raw, dev.env)
        n = h.ext_device_info()["launches"]; acts.append(n - last); last = n
        h.ext_record_device(dev.rew[t], dev.term[t], dev.trunc[t], dev.tobs[t])
        n = h.ext_device_info()["launches"]; recs.append(n - last); last = n
    info = h.ext_device_info()
    assert info["host_syncs"] == 0 and info["steps_device"] == T and info["steps_host"] == 0
    h.ext_finish_device(dev.obs[(c + 1) * T])
    assert h.ext_device_info()["host_syncs"] == 0
    return acts, recs, h.ext_device_info()["launches"] - last


@pytest.mark.parametrize("E,D", [(5, 1), (257, 133)])
def test_sync_free_launch_budget_and_off_is_the_parent(pkg, E, D):
    sc, dev = _script(E, D), _Dev(E, D)
    plain, norm, both, off = (_handle(pkg, E, D) for _ in range(4))
    norm.ext_normalize_enable(**KW)
    both.ext_monitor_enable(3); both.ext_normalize_enable(**KW)
    off.ext_monitor_enable(3); off.ext_normalize_enable(**KW); off.ext_normalize_enable(False); off.ext_monitor_enable(0)   # enabled, then disabled
    assert off.ext_wrap_info()["normalize_on"] == 0 and off.ext_wrap_info()["monitor_on"] == 0
    for c in range(K):
        pa, pr, pf = _per_verb_launches(plain, dev, c, sc)
        for h, mon in ((norm, 0), (both, 2)):                                        # the monitor's window: the two launches of its collector at finish
            a, r, f = _per_verb_launches(h, dev, c, sc)
            print(f"E={E} D={D} rollout {c} monitor={bool(mon)}: launches per act {a} (plain {pa}), per record {r} (plain {pr}), finish {f} (plain {pf})")
            assert all(0 < x - y <= 2 for x, y in zip(a, pa)) and all(0 <= x - y <= 2 for x, y in zip(r, pr)) and 0 < f - pf <= 2 + mon
            wi = h.ext_wrap_info()
            assert wi["allocations"] == 0
            assert (wi["launches_act"], wi["launches_record"], wi["launches_finish"]) == (sum(a) - sum(pa), sum(r) - sum(pr), f - pf)
        assert (pa, pr, pf) == _per_verb_launches(off, dev, c, sc)                   # a handle that switched both off enqueues what one that never had them does
        for n in ("OBSERVATIONS", "ACTIONS", "VALUES", "LOGPROBS", "REWARDS", "FLAGS", "BOOTSTRAP", "LAST_VALUES", "ADVANTAGES", "RETURNS"):
            x, y = (hh.buffer(getattr(pkg._capi, "BUF_" + n)) for hh in (off, plain))
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), n
        assert off.ext_wrap_info()["launches_act"] == 0
    for h in (plain, norm, both, off):
        h.close()


# ---- 4. frozen statistics ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,D", [(5, 24), (257, 133)])
def test_frozen_statistics(pkg, E, D):
    h = _handle(pkg, E, D)
    h.ext_normalize_enable(**dict(KW, training=False))
    rng = np.random.default_rng(E + D)
    given = dict(obs_mean=rng.uniform(-1, 1, D).astype(F), obs_var=rng.uniform(0.5, 4.0, D).astype(F), obs_count=1000, ret_mean=0.25, ret_var=2.5, ret_count=777)
    h.ext_normalize_set_stats(**given)
    dev = _Dev(E, D)
    w = ref.Wrapper(E, D, training=False, **KW); w.set_stats(given)
    kw = dict(KW, norm_obs=1, norm_reward=1)
    for c in range(K):
        _rollout(h, dev, c)
        st = h.ext_normalize_get_stats()
        for k, v in given.items():                                                   # bitwise unchanged
            assert np.array_equal(np.asarray(st[k], F).view(np.uint32), np.asarray(v, F).view(np.uint32)) if k.endswith(("mean", "var")) else st[k] == v, k
        assert not h.ext_normalize_get_returns().any()                               # returns of a fresh wrapper: bitwise unchanged too
        _, exp = _expected_frozen(E, D, c, w)
        _check_rollout(pkg, h, E, D, c, exp, kw)
    # after a training rollout `returns` are non-zero; frozen, they change only by the reset of finished envs (normalizeWrapperEnv.jl:149-153 runs whatever `training` says)
    h.ext_normalize_set_training(True)
    _rollout(h, dev, 0)
    before, st_before = h.ext_normalize_get_returns(), h.ext_normalize_get_stats()
    assert before.any()
    h.ext_normalize_set_training(False)
    _rollout(h, dev, 1)
    sc = _script(E, D)
    done = (sc["term"][T:2 * T] | sc["trunc"][T:2 * T]).any(0)
    assert np.array_equal(h.ext_normalize_get_returns().view(np.uint32), np.where(done, F(0), before).view(np.uint32))
    st_after = h.ext_normalize_get_stats()
    assert all(np.array_equal(np.asarray(st_after[k]), np.asarray(st_before[k])) for k in st_before)
    h.close()


def _expected_frozen(E, D, c, w):
    sc = _script(E, D)
    o, r, tb = [], [], []
    with np.errstate(invalid="ignore"):
        for t in range(c * T, (c + 1) * T):
            o.append(w.observe(sc["obs"][t]))
            rn, tn = w.act(sc["rew"][t], sc["term"][t], sc["trunc"][t], sc["tobs"][t])
            r.append(rn); tb.append(tn)
        return w, dict(obs=np.stack(o), rew=np.stack(r), tobs=np.stack(tb), last=w.observe(sc["obs"][(c + 1) * T]))


# ---- 5. evaluation ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,D", [(5, 1), (257, 133)])
def test_predict_actions_device_normalises_and_never_updates(pkg, E, D):
    h, twin = _handle(pkg, E, D), _handle(pkg, E, D)
    h.ext_normalize_enable(**KW)                                                     # training = 1
    dev = _Dev(E, D)
    _rollout(h, dev, 0)                                                              # statistics worth the name
    st = h.ext_normalize_get_stats()
    ret, orig = h.ext_normalize_get_returns(), h.ext_normalize_get_original()
    w = ref.Wrapper(E, D, **KW); w.set_stats(st)
    for B in (E, E + 3):                                                             # up to n_envs rows; more: the grow-only scratch, counted once
        obs = (np.random.default_rng(B).uniform(-4, 4, (B, D))).astype(F)
        d_obs, d_env, d_env2 = hip_mem.to_device(obs), hip_mem.empty((B, A), F), hip_mem.empty((B, A), F)
        h.predict_actions_device(d_obs, True, None, d_env)
        twin.predict_actions_device(hip_mem.to_device(w.normalize_obs(obs)), True, None, d_env2)
        _close(f"E={E} D={D} B={B} deterministic actions", d_env.get(), d_env2.get(), 1e-4)
    assert h.ext_wrap_info()["allocations"] == 1
    st2 = h.ext_normalize_get_stats()
    assert all(np.array_equal(np.asarray(st2[k]), np.asarray(st[k])) for k in st) and h.ext_normalize_config()["training"] is True
    assert np.array_equal(h.ext_normalize_get_returns(), ret) and all(np.array_equal(x, y) for x, y in zip(h.ext_normalize_get_original(), orig))
    h.close(); twin.close()


# ---- 6. the monitor ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("E,D", [(5, 1), (257, 24)])
def test_monitor_window(pkg, E, D, normalize):
    W = 3
    h = _handle(pkg, E, D)
    h.ext_monitor_enable(W)
    assert h.ext_monitor_stats() == (0.0, 0.0, 0)
    if normalize:
        h.ext_normalize_enable(**KW)
    sc, dev = _script(E, D), _Dev(E, D)
    mon = Monitor(E, W)
    for c in range(K):
        _rollout(h, dev, c)
        for t in range(c * T, (c + 1) * T):
            mon.act(sc["rew"][t], sc["term"][t], sc["trunc"][t])                     # RAW rewards: the monitor sits inside the normaliser
        got = h.ext_monitor_stats()
        print(f"E={E} D={D} normalize={normalize} rollout {c}: monitor {got}, restatement {mon.stats()}")
        assert got == mon.stats()
    assert int((sc["term"] | sc["trunc"]).astype(bool).sum()) > W and got[2] == W     # more episodes than the window holds
    with pytest.raises(pkg.DrilError) as e:
        h.monitor_stats()                                                            # the existing verb keeps its status on an external handle
    assert e.value.code == pkg._capi.ERR_NOT_INITIALISED
    h.ext_monitor_enable(0)
    with pytest.raises(pkg.DrilError) as e:
        h.ext_monitor_stats()
    assert e.value.code == pkg._capi.ERR_NOT_INITIALISED
    h.close()


# ---- 7. the sticky error ---------------------------------------------------------------------------------------------------------------------------------------
def test_truncated_flag_without_terminal_obs_under_the_wrapper(pkg):
    E, D = 5, 24
    kw = dict(KW, norm_obs=1, norm_reward=1)
    h = _handle(pkg, E, D)
    h.ext_normalize_enable(**kw)
    dev = _Dev(E, D)
    for t in range(T):
        h.ext_act_device(dev.obs[t], dev.raw, dev.env)
        h.ext_record_device(dev.rew[t], dev.term[t], dev.trunc[t], None)             # steps 1 .. 3 have truncated envs: NULL is a false statement there
    with pytest.raises(pkg.DrilError) as e:
        h.ext_finish_device(dev.obs[T])
    assert e.value.code == pkg._capi.ERR_INVALID_ARG and "terminal_obs" in str(e.value) and h.ext_steps() == 0
    w, exp = _expected(E, D, 2, **kw)
    st = h.ext_normalize_get_stats()                                                 # the discarded rollout's updates were enqueued: the statistics keep them
    assert st["obs_count"] == E * (T + 1) and st["ret_count"] == E * T
    _rollout(h, dev, 1)                                                              # usable afterwards: the second rollout of the script equals the wrapper's
    _check_rollout(pkg, h, E, D, 1, exp[1], kw)
    assert_stats(h.ext_normalize_get_stats(), w)
    h.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    E, D = 5, 24
    UNS, INV, NI = capi.ERR_UNSUPPORTED, capi.ERR_INVALID_ARG, capi.ERR_NOT_INITIALISED
    cfg = capi.DrilNormalizeConfig(); lib.dril_normalize_config_default(C.byref(cfg))
    err = lambda hh: lib.dril_last_error(hh._h).decode()
    h = _handle(pkg, E, D)
    for call in (lambda: h.ext_normalize_config(), lambda: h.ext_normalize_get_stats(), lambda: h.ext_normalize_get_original(), lambda: h.ext_normalize_get_returns(),
                 lambda: h.ext_normalize_set_training(True), lambda: h.ext_normalize_reset(), lambda: h.ext_monitor_stats(),
                 lambda: h.ext_normalize_set_stats(np.zeros(D), np.ones(D), 0, 0.0, 1.0, 0)):
        with pytest.raises(pkg.DrilError) as e:                                      # getters while off
            call()
        assert e.value.code == NI
    cart = pkg.Handle(capi.default_config(capi.ENV_CARTPOLE))                        # a built-in handle
    info = capi.DrilExtWrapInfo()
    assert lib.dril_ext_normalize_enable(cart._h, C.byref(cfg)) == UNS and "cfg.norm_obs" in err(cart) and "dril_normalize_enable" in err(cart)
    assert lib.dril_ext_monitor_enable(cart._h, 3) == UNS and "cfg.monitor_window" in err(cart) and lib.dril_ext_wrap_info(cart._h, C.byref(info)) == UNS
    assert lib.dril_ext_normalize_get_stats(cart._h, None, None, None, None, None, None) == UNS and lib.dril_ext_monitor_get_stats(cart._h, None, None, None) == UNS
    two = pkg.Handle(_cfg(pkg, E, D, world_size=2, rank=0, batch_size=E * 2))       # a data-parallel external handle
    assert lib.dril_ext_normalize_enable(two._h, C.byref(cfg)) == UNS and "world_size" in err(two) and two.ext_wrap_info()["normalize_on"] == 0
    for field, bad in (("clip_obs", -1.0), ("clip_reward", float("nan")), ("epsilon", -1e-3)):
        c = capi.DrilNormalizeConfig(); lib.dril_normalize_config_default(C.byref(c)); setattr(c, field, bad)
        assert lib.dril_ext_normalize_enable(h._h, C.byref(c)) == INV and h.ext_wrap_info()["normalize_on"] == 0, field
    assert lib.dril_ext_monitor_enable(h._h, -1) == INV
    # the existing family and the create-time fields stay refused on an external handle, with the word "host" in the message
    assert lib.dril_normalize_enable(h._h, C.byref(cfg)) == UNS and "host" in err(h)
    with pytest.raises(pkg.DrilError) as e:
        pkg.Handle(_cfg(pkg, E, D, monitor_window=5))
    assert e.value.code == UNS and "host" in str(e.value)
    dev = _Dev(E, D)
    h.ext_act_device(dev.obs[0], dev.raw, dev.env)                                   # enable inside a rollout: an act is pending ...
    assert lib.dril_ext_normalize_enable(h._h, C.byref(cfg)) == INV and "rollout" in err(h) and lib.dril_ext_monitor_enable(h._h, 3) == INV
    h.ext_record_device(dev.rew[0], dev.term[0], dev.trunc[0], dev.tobs[0])
    assert h.ext_steps() == 1 and lib.dril_ext_normalize_enable(h._h, C.byref(cfg)) == INV   # ... or steps are recorded
    assert h.ext_wrap_info()["normalize_on"] == 0 and h.ext_wrap_info()["monitor_on"] == 0
    for t in range(1, T):
        h.ext_act_device(dev.obs[t], dev.raw, dev.env); h.ext_record_device(dev.rew[t], dev.term[t], dev.trunc[t], dev.tobs[t])
    h.ext_finish_device(dev.obs[T])
    sc = _script(E, D)
    for on, off in ((lambda: h.ext_normalize_enable(**KW), lambda: h.ext_normalize_enable(False)), (lambda: h.ext_monitor_enable(3), lambda: h.ext_monitor_enable(0))):
        on()                                                                         # host verbs while a wrapper is on
        rew, fl = sc["rew"][0], sc["term"][0]
        assert lib.dril_ext_act(h._h, sc["obs"][0].ctypes.data_as(C.c_void_p), None, None) == UNS and "device verbs" in err(h) and "on the host" in err(h)
        assert lib.dril_ext_record(h._h, rew.ctypes.data_as(C.c_void_p), fl.ctypes.data_as(C.c_void_p), fl.ctypes.data_as(C.c_void_p), None) == UNS
        assert lib.dril_ext_finish(h._h, sc["obs"][0].ctypes.data_as(C.c_void_p)) == UNS and h.ext_steps() == 0
        off()
    raw, ea = h.ext_act(sc["obs"][0])                                                # off again: the host verbs work
    h.ext_record(sc["rew"][0], sc["term"][0], sc["trunc"][0], None)
    for hh in (h, cart, two):
        hh.close()


# ---- 9. the Python mirror ----------------------------------------------------------------------------------------------------------------------------------------
STEPS = 16


class _ScriptedDeviceEnv:
    """ONE batched env on hip_mem arrays that plays the script (round and round) whatever the actions are"""

    def __init__(self, pkg, E, D):
        self.pkg, self.n_envs, self.D, self.t = pkg, E, D, 0
        self.dev = _Dev(E, D, steps=STEPS)

    def observation_space(self):
        return self.pkg.Box(low=(-10.0,) * self.D, high=(10.0,) * self.D)

    def action_space(self):
        return self.pkg.Box(low=(-1.0,) * A, high=(1.0,) * A)

    def reset_(self):
        pass

    def observe(self):
        return self.dev.obs[self.t % STEPS]

    def act_(self, actions):
        t = self.t % STEPS; self.t += 1
        return self.dev.rew[t], self.dev.term[t], self.dev.trunc[t], self.dev.tobs[t]


def test_python_mirror(pkg, tmp_path):
    E, D, W = 5, 24, 3
    inner = _ScriptedDeviceEnv(pkg, E, D)
    env = pkg.NormalizeWrapperEnv(pkg.MonitorWrapperEnv(pkg.DeviceArrayParallelEnv(inner, seed=3, empty=hip_mem.empty), W), **KW)
    assert isinstance(env, pkg.DeviceArrayParallelEnv) and env.env is inner
    alg = pkg.PPO(n_steps=T, batch_size=E, epochs=1)
    agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space(), hidden_dims=HIDDEN), alg, seed=0)
    stats, timer = pkg.train_(agent, env, alg, 2 * T * E)
    h = env.handle
    wi = h.ext_wrap_info()                                                           # bind switched both wrappers on; two wrapped rollouts ran
    assert wi["normalize_on"] == 1 and wi["monitor_on"] == 1 and wi["monitor_window"] == W and wi["allocations"] == 0 and h.ext_device_info()["host_syncs"] == 0
    assert len(stats["losses"]) == 2 and np.isfinite(stats["losses"]).all()
    sc, mon = _script(E, D, STEPS), Monitor(E, W)
    for t in range(2 * T):
        mon.act(sc["rew"][t], sc["term"][t], sc["trunc"][t])
    assert len(env.last_monitor_stats) == 2 and env.last_monitor_stats[-1] == mon.stats() == env.monitor_stats()   # what log_stats logs: raw returns
    st = h.ext_normalize_get_stats()
    assert st["obs_count"] == 2 * E * (T + 1) and st["ret_count"] == 2 * E * T
    # evaluate_agent: frozen statistics, raw returns, the monitor's window does not move
    er, el = pkg.evaluate_agent(agent, env, n_eval_episodes=4, deterministic=True, return_stats=False)
    assert len(er) == 4 and env.monitor_stats() == mon.stats()
    st2 = h.ext_normalize_get_stats()
    assert all(np.array_equal(np.asarray(st2[k]), np.asarray(st[k])) for k in st)
    assert not h.ext_normalize_get_returns().any()                                   # evaluate_agent resets the env: reset_() zeroed the wrapper's returns
    # the helpers every other wrapped env has
    o = pkg.get_original_obs(env)
    assert o.shape == (E, D) and pkg.get_original_rewards(env).shape == (E,)
    x = np.ones((E, D), F)
    assert np.allclose(pkg.unnormalize_obs_(x.copy(), env), np.sqrt(st["obs_var"] + F(KW["epsilon"])) + st["obs_mean"])
    assert np.allclose(pkg.unnormalize_rewards_(np.ones(E, F), env), np.sqrt(F(st["ret_var"]) + F(KW["epsilon"])))
    fp = pkg.save_normalization_stats(env, tmp_path / "norm")
    saved = np.load(fp)
    assert float(saved["clip_obs"]) == KW["clip_obs"] and float(saved["gamma"]) == KW["gamma"]
    h.ext_normalize_set_stats(np.zeros(D), np.ones(D), 0, 0.0, 1.0, 0)
    pkg.load_normalization_stats_(env, fp)
    st3 = h.ext_normalize_get_stats()                                                # the round trip, bitwise
    assert all(np.array_equal(np.asarray(st3[k], F).view(np.uint32), np.asarray(st[k], F).view(np.uint32)) if not k.endswith("count") else st3[k] == st[k] for k in st)
    # extract_policy(agent, env): a NormWrapperPolicy with the frozen statistics acts on RAW observations like evaluate_agent's path
    policy = pkg.extract_policy(agent, env)
    assert isinstance(policy, pkg.NormWrapperPolicy)
    raw_obs = sc["obs"][3]
    d_env = hip_mem.empty((E, A), F)
    h.set_params(pkg.flatten_params(agent.train_state.parameters))
    h.predict_actions_device(hip_mem.to_device(raw_obs), True, None, d_env)
    _close("extract_policy vs predict_actions_device", policy.act(raw_obs, deterministic=True), d_env.get(), 1e-4)
    with pytest.raises(TypeError, match="on the host"):
        pkg.NormalizeWrapperEnv(object.__new__(pkg.HostParallelEnv))
    policy.close(); h.close()


def test_torch_example_env_trains_under_the_wrappers(pkg):
    torch = pytest.importorskip("torch", reason="the example env is written in torch")
    if not torch.cuda.is_available():
        pytest.skip("torch.cuda.is_available() is false on this machine: the torch example env needs torch's own GPU runtime (every other test of this file uses tests/hip_mem.py)")
    spec = importlib.util.spec_from_file_location("ppo_torch_envs", ROOT / "examples" / "ppo_torch_envs.py")
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    E = 64
    env = ex.make_env(E, normalize=True, monitor=True, max_steps=20)
    alg = pkg.PPO(n_steps=32, batch_size=E * 32 // 4, epochs=2)
    agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space(), hidden_dims=(64, 64)), alg, seed=0)
    stats, timer = pkg.train_(agent, env, alg, 2 * 32 * E)
    wi, info = env.handle.ext_wrap_info(), env.handle.ext_device_info()
    assert wi["normalize_on"] == 1 and wi["monitor_on"] == 1 and wi["allocations"] == 0 and info["host_syncs"] == 0 and info["steps_device"] == 32
    assert len(stats["losses"]) == 2 and all(np.isfinite(stats[k]).all() for k in ("losses", "value_losses", "policy_losses", "grad_norms"))
    rew_mean, len_mean, n = env.monitor_stats()
    assert n > 0 and len_mean == 20.0 and rew_mean < 0                               # 20-step episodes, raw (negative) pendulum returns
    assert env.handle.ext_normalize_get_stats()["obs_count"] == 2 * E * 33
