"""GPU (-m gpu): the device-array verbs of DRIL_ENV_EXTERNAL (dril_ext_act_device / _record_device / _finish_device, dril_predict_actions_device,
dril_ext_set_action_bounds, dril_ext_device_info) against the HOST verbs of the same library on a twin handle: same parameters, same injected noise,
same scripted env data (pre-drawn observations, rewards, flags per step; no simulator).  Device memory comes from tests/hip_mem.py (ctypes on the HIP
runtime), so nothing here needs torch.cuda — except the one test of the torch example, which says so when it skips.

Bitwise between the twins: observations, actions, values, log-probabilities, rewards, flags of the buffer, and the raw / env actions handed back.
With a tolerance: the bootstrap rows (the host verb forwards the truncated columns only, the device verb all E), advantages, returns, last values, and the
parameters after one update — the tolerances of tests/test_gpu_external.py::test_external_rollout_and_update_vs_oracle (its lines 156-157 and 168), restated in
TOL / PARAM_TOL below.  Every test prints the largest bootstrap difference it saw before it asserts."""
import ctypes as C
import functools
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import hip_mem

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

T = 3
# (name, obs dim, action dim, discrete, per-dimension bounds or None = the config's scalar pair (-1, 1))
SPACES = {
    "d1_discrete3": (1, 3, True, None),
    "d24_box3_perdim": (24, 3, False, ((-1.0, -0.5, 0.25), (1.0, 0.5, 0.25))),      # the third dimension has low >= high: not clamped
    "d4_box1_scalar": (4, 1, False, None),
}
HIDDEN = [(32, 48), (64, 64)]
SIZES = [5, 257]                                                                     # one block with a tail; two blocks with a tail of one
# test_gpu_external.py:156-157 (values / bootstrap / last values 1e-4, advantages / returns 1e-3) and :168 (parameters after update!)
TOL = {"BOOTSTRAP": 1e-4, "LAST_VALUES": 1e-4, "ADVANTAGES": 1e-3, "RETURNS": 1e-3}
PARAM_TOL = dict(rtol=3e-4, atol=3e-6)
BITWISE = ("OBSERVATIONS", "ACTIONS", "VALUES", "LOGPROBS", "REWARDS", "FLAGS")


def _cfg(pkg, space, hidden, E, **kw):
    D, A, discrete, _ = SPACES[space]
    c = pkg._capi.default_config(pkg._capi.ENV_EXTERNAL)
    c.ext_obs_dim, c.ext_action_dim, c.ext_discrete, c.hidden1, c.hidden2 = D, A, int(discrete), hidden[0], hidden[1]
    c.ext_action_low, c.ext_action_high = -1.0, 1.0
    c.n_envs, c.n_steps, c.batch_size, c.epochs, c.seed = E, T, E, 2, 11
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _handle(pkg, space, hidden, E, seed=5):
    h = pkg.Handle(_cfg(pkg, space, hidden, E))
    h.set_params((np.random.default_rng(seed).standard_normal(h.P) * 0.3).astype(np.float32))
    bounds = SPACES[space][3]
    if bounds is not None:
        h.ext_set_action_bounds(*bounds)
    return h


@functools.lru_cache(maxsize=None)
def _script(space, E, steps=T):
    """the scripted env: obs[t] (steps + 1 of them, the last one is last_obs), rew, term, trunc, tobs per step, and the sampling noise.
    env 0 terminates only at step 1, env 1 is truncated only at step 2, env 2 is terminated AND truncated at step 3 (the last step of a T = 3 rollout);
    the LAST env (the grid tail of the per-env kernels) is truncated at step 2 and terminated at step 3.  No truncation at step 1: terminal_obs is NULL there.
    Rows of terminal_obs whose env was not truncated hold NaN: they must never be selected."""
    D, A, discrete, _ = SPACES[space]
    rng = np.random.default_rng(1000 + 7 * E + D)
    obs = rng.uniform(-2, 2, (steps + 1, E, D)).astype(np.float32)
    rew = rng.standard_normal((steps, E)).astype(np.float32)
    term, trunc = np.zeros((steps, E), np.uint8), np.zeros((steps, E), np.uint8)
    term[0, 0] = 1; trunc[1, 1] = 1; term[2, 2] = trunc[2, 2] = 1
    trunc[1, E - 1] = 1; term[2, E - 1] = 1
    for t in range(3, steps):                                                        # longer scripts (the evaluation of the Python mirror): a few more episode ends
        term[t, (t + 1) % E] = 1; trunc[t, (t + 3) % E] = 1
    tobs = rng.uniform(-2, 2, (steps, E, D)).astype(np.float32)
    tobs[trunc == 0] = np.nan
    n = steps * E
    noise = rng.random(n) if discrete else (3.0 * rng.standard_normal((n, A))).astype(np.float32)   # 3 sigma: many Box actions leave the bounds
    for a in (obs, rew, term, trunc, tobs, noise):
        a.setflags(write=False)
    return dict(obs=obs, rew=rew, term=term, trunc=trunc, tobs=tobs, noise=noise)


def _tobs(sc, t):
    return sc["tobs"][t] if sc["trunc"][t].any() else None


def _buffers(pkg, h):
    capi = pkg._capi
    return {n: h.buffer(getattr(capi, "BUF_" + n)) for n in BITWISE + tuple(TOL)}


def _perm(E):
    return np.stack([np.random.default_rng(50 + e).permutation(E * T) for e in range(2)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _host_reference(space, hidden, E):
    """the twin: one rollout through the HOST verbs and one update.  Computed once per case, shared by every test, never changed"""
    import __graft_entry__ as g
    pkg = g.load_package()
    sc = _script(space, E)
    h = _handle(pkg, space, hidden, E)
    h.set_noise(sc["noise"])
    raws, envs = [], []
    for t in range(T):
        raw, ea = h.ext_act(sc["obs"][t]); raws.append(raw); envs.append(ea)
        h.ext_record(sc["rew"][t], sc["term"][t], sc["trunc"][t], _tobs(sc, t))
    h.ext_finish(sc["obs"][T])
    info = h.ext_device_info()
    ref = dict(buf=_buffers(pkg, h), raw=raws, env=envs, info=info)
    h.set_permutation(_perm(E)); h.ppo_update()
    ref["params"] = h.get_params()
    h.close()
    for a in list(ref["buf"].values()) + raws + envs + [ref["params"]]:
        a.setflags(write=False)
    return ref


class _Dev:
    """the script on the device, uploaded on `stream` (None: blocking copies), and the two action output arrays"""

    def __init__(self, space, E, stream=None, steps=T):
        D, A, discrete, _ = SPACES[space]
        sc = _script(space, E, steps)
        up = lambda a: hip_mem.to_device(a, stream)
        self.obs = [up(sc["obs"][t]) for t in range(steps + 1)]
        self.rew = [up(sc["rew"][t]) for t in range(steps)]; self.term = [up(sc["term"][t]) for t in range(steps)]; self.trunc = [up(sc["trunc"][t]) for t in range(steps)]
        self.tobs = [up(sc["tobs"][t]) if sc["trunc"][t].any() else None for t in range(steps)]
        shape, dt = ((E,), np.int32) if discrete else ((E, A), np.float32)
        self.raw, self.env = hip_mem.empty(shape, dt).fill_bytes(0xFF), hip_mem.empty(shape, dt).fill_bytes(0xFF)
        self.zeros = hip_mem.to_device(np.zeros(E, np.uint8))                        # flags of a step in which nothing ends
        hip_mem.chk(hip_mem.lib().hipStreamSynchronize(None), "hipStreamSynchronize")   # the fills ran on the null stream, which a stream of the test's own does not wait for


def _device_step(h, dev, t, stream=None):
    """one act / record pair through the device verbs -> (raw, env) actions read back on the caller's stream"""
    sp = None if stream is None else stream.ptr
    h.ext_act_device(dev.obs[t], dev.raw, dev.env, sp)
    raw, ea = dev.raw.get(stream), dev.env.get(stream)                               # stream None: a blocking copy on the null stream, which the library made wait
    h.ext_record_device(dev.rew[t], dev.term[t], dev.trunc[t], dev.tobs[t], sp)
    return raw, ea


def _host_step(h, sc, t):
    raw, ea = h.ext_act(sc["obs"][t])
    h.ext_record(sc["rew"][t], sc["term"][t], sc["trunc"][t], _tobs(sc, t))
    return raw, ea


def _check_actions(space, ref, t, raw, ea):
    D, A, discrete, bounds = SPACES[space]
    assert np.array_equal(raw, ref["raw"][t]) and np.array_equal(ea, ref["env"][t]), (space, t)
    if discrete:
        assert np.array_equal(ea, raw)                                               # DiscreteAdapter: the identity
        return
    lo, hi = (np.asarray(b, np.float32) for b in (bounds if bounds is not None else ((-1.0,) * A, (1.0,) * A)))
    want = np.where(lo < hi, np.clip(raw, lo, hi), raw)                              # ClampAdapter per dimension; low >= high: not clamped
    assert np.array_equal(ea, want)
    clamped = lo < hi
    assert ((raw[:, clamped] < lo[clamped]) | (raw[:, clamped] > hi[clamped])).any(), "the scripted noise must push some actions out of the bounds"
    assert (ea != raw).any()
    if (~clamped).any():
        assert np.array_equal(ea[:, ~clamped], raw[:, ~clamped]) and (np.abs(raw[:, ~clamped]) > 1).any()


def _check_rollout(pkg, h, ref, what):
    got = _buffers(pkg, h)
    boot_diff = float(np.abs(got["BOOTSTRAP"] - ref["buf"]["BOOTSTRAP"]).max())
    print(f"{what}: max |bootstrap(device verbs) - bootstrap(host verbs)| = {boot_diff:.3e}")
    for n in BITWISE:
        assert np.array_equal(got[n], ref["buf"][n]), (what, n)
    fl = got["FLAGS"].reshape(T, -1)
    assert fl[0, 0] == 1 and fl[1, 1] == 2 and fl[2, 2] == 3 and fl[1, -1] == 2 and fl[2, -1] == 1 and int((fl != 0).sum()) == 5
    boot = got["BOOTSTRAP"].reshape(T, -1)
    assert np.isfinite(boot).all() and (boot[(fl & 2) == 0] == 0).all() and (boot[(fl & 2) != 0] != 0).all()   # V(terminal_obs) where truncated, 0 elsewhere: no NaN column was selected
    for n, tol in TOL.items():
        np.testing.assert_allclose(got[n], ref["buf"][n], atol=tol, rtol=tol, err_msg=f"{what} {n}")
    assert np.isfinite(got["ADVANTAGES"]).all() and np.isfinite(got["RETURNS"]).all()


def _check_update(h, ref, E):
    h.set_permutation(_perm(E)); h.ppo_update()
    np.testing.assert_allclose(h.get_params(), ref["params"], **PARAM_TOL)


# ---- 1. equality with the host verbs, 3. sync-free -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("hidden", HIDDEN, ids=lambda h: f"h{h[0]}x{h[1]}")
@pytest.mark.parametrize("space", list(SPACES))
def test_device_verbs_equal_the_host_verbs(pkg, space, hidden, E):
    ref = _host_reference(space, hidden, E)
    assert ref["info"]["steps_host"] == T and ref["info"]["steps_device"] == 0 and ref["info"]["host_syncs"] == T + 2 * 2   # one drain per host act, two more per truncation step
    h = _handle(pkg, space, hidden, E)
    h.set_noise(_script(space, E)["noise"])
    dev = _Dev(space, E)
    for t in range(T):
        raw, ea = _device_step(h, dev, t)
        _check_actions(space, ref, t, raw, ea)
        assert h.ext_steps() == t + 1
    info = h.ext_device_info()
    assert info["host_syncs"] == 0 and info["steps_device"] == T and info["steps_host"] == 0, info   # sync-free, the two truncation steps included
    assert info["per_dim_bounds"] == (SPACES[space][3] is not None) and info["launches"] > 0
    h.ext_finish_device(dev.obs[T])
    assert h.ext_steps() == 0 and h.ext_device_info()["host_syncs"] == 0             # the drain of finish is the rollout's one wait, not an act / record wait
    _check_rollout(pkg, h, ref, f"{space} {hidden} E={E}")
    _check_update(h, ref, E)
    h.close()


# ---- 2. a rollout that mixes host and device verbs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space,hidden,E", [("d1_discrete3", (32, 48), 5), ("d24_box3_perdim", (64, 64), 257), ("d4_box1_scalar", (32, 48), 257)])
def test_mixed_rollout(pkg, space, hidden, E):
    ref, sc = _host_reference(space, hidden, E), _script(space, E)
    h = _handle(pkg, space, hidden, E)
    h.set_noise(sc["noise"])
    dev = _Dev(space, E)
    for t in range(T):
        raw, ea = _host_step(h, sc, t) if t == 1 else _device_step(h, dev, t)       # steps 1 and 3 on device arrays, step 2 (a truncation step) on host arrays
        _check_actions(space, ref, t, raw, ea)
    info = h.ext_device_info()
    assert (info["steps_device"], info["steps_host"], info["host_syncs"]) == (2, 1, 3), info
    h.ext_finish_device(dev.obs[T])
    _check_rollout(pkg, h, ref, f"mixed {space} E={E}")
    _check_update(h, ref, E)
    h.close()


# ---- 4. the caller's stream ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_stream", [True, False], ids=["own_stream", "null_stream"])
@pytest.mark.parametrize("space,hidden,E", [("d24_box3_perdim", (64, 64), 257), ("d1_discrete3", (32, 48), 5)])
def test_caller_stream_orders_inputs_and_outputs(pkg, monkeypatch, space, hidden, E, own_stream):
    """inputs uploaded with hipMemcpyAsync on the test's stream, outputs read with hipMemcpyAsync + hipStreamSynchronize of THAT stream only; dril_synchronize never
    runs during act / record"""
    ref = _host_reference(space, hidden, E)
    h = _handle(pkg, space, hidden, E)
    h.set_noise(_script(space, E)["noise"])
    called = []
    monkeypatch.setattr(h, "synchronize", lambda: called.append(1))
    stream = hip_mem.Stream() if own_stream else None
    dev = _Dev(space, E, stream)                                                     # async uploads: ordered before the library's work by the entry event alone
    for t in range(T):
        raw, ea = _device_step(h, dev, t, stream)
        _check_actions(space, ref, t, raw, ea)
    assert not called and h.ext_device_info()["host_syncs"] == 0
    h.ext_finish_device(dev.obs[T], None if stream is None else stream.ptr)
    _check_rollout(pkg, h, ref, f"stream={own_stream} {space} E={E}")
    h.close()


# ---- 5. the sticky error ---------------------------------------------------------------------------------------------------------------------------------------
def test_truncated_flag_without_terminal_obs_is_reported_by_finish(pkg):
    space, hidden, E = "d4_box1_scalar", (32, 48), 5
    ref, sc = _host_reference(space, hidden, E), _script(space, E)
    h = _handle(pkg, space, hidden, E)
    h.set_noise(sc["noise"])
    dev = _Dev(space, E)
    for t in range(T):
        h.ext_act_device(dev.obs[t], dev.raw, dev.env)
        h.ext_record_device(dev.rew[t], dev.term[t], dev.trunc[t], None)             # steps 2 and 3 have truncated envs: NULL is a false statement there
    assert h.ext_steps() == T
    with pytest.raises(pkg.DrilError) as e:
        h.ext_finish_device(dev.obs[T])
    assert e.value.code == pkg._capi.ERR_INVALID_ARG and "terminal_obs" in str(e.value)
    assert h.ext_steps() == 0                                                        # not collected
    h.set_noise(sc["noise"])                                                         # a complete rollout on the same handle succeeds and equals the twin's
    for t in range(T):
        raw, ea = _device_step(h, dev, t)
        _check_actions(space, ref, t, raw, ea)
    h.ext_finish_device(dev.obs[T])
    _check_rollout(pkg, h, ref, "after the sticky error")
    _check_update(h, ref, E)
    h.close()


# ---- 6. statuses -------------------------------------------------------------------------------------------------------------------------------------------------
def test_statuses(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    space, E = "d4_box1_scalar", 5
    h = _handle(pkg, space, (32, 48), E)
    dev = _Dev(space, E)
    P = lambda a: C.c_void_p(a.ptr)
    obs, rew, fl = P(dev.obs[0]), P(dev.rew[0]), P(dev.zeros)
    INV = capi.ERR_INVALID_ARG
    assert lib.dril_ext_act_device(h._h, None, P(dev.raw), P(dev.env), None) == INV and b"null obs" in lib.dril_last_error(h._h)
    assert lib.dril_ext_record_device(h._h, rew, fl, fl, None, None) == INV          # record before act
    assert lib.dril_ext_act_device(h._h, obs, None, None, None) == capi.OK           # both outputs may be NULL
    assert lib.dril_ext_act_device(h._h, obs, None, None, None) == INV               # act twice
    for args in ((None, fl, fl), (rew, None, fl), (rew, fl, None)):
        assert lib.dril_ext_record_device(h._h, *args, None, None) == INV            # null rewards / flags
    assert h.ext_steps() == 0
    assert lib.dril_ext_record_device(h._h, rew, fl, fl, None, None) == capi.OK and h.ext_steps() == 1
    h.ext_act_device(dev.obs[1], dev.raw, None); h.ext_record_device(dev.rew[1], dev.zeros, dev.zeros)
    assert lib.dril_ext_finish_device(h._h, obs, None) == INV and h.ext_steps() == 2  # finish after two of three steps
    assert lib.dril_ext_finish_device(h._h, None, None) == INV
    h.ext_act_device(dev.obs[2], None, dev.env); h.ext_record_device(dev.rew[2], dev.zeros, dev.zeros)
    assert lib.dril_ext_act_device(h._h, obs, None, None, None) == INV               # a fourth act in a T = 3 rollout
    assert lib.dril_ext_finish_device(h._h, obs, None) == capi.OK and h.ext_steps() == 0
    assert lib.dril_predict_actions_device(h._h, None, 5, 1, P(dev.raw), None, None) == INV
    assert lib.dril_predict_actions_device(h._h, obs, 5, 1, None, None, None) == INV
    assert lib.dril_predict_actions_device(h._h, obs, 0, 1, P(dev.raw), None, None) == INV
    assert lib.dril_ext_set_action_bounds(h._h, (C.c_float * 1)(0.0), None) == INV
    disc = _handle(pkg, "d1_discrete3", (32, 48), E)
    assert lib.dril_ext_set_action_bounds(disc._h, (C.c_float * 3)(), (C.c_float * 3)()) == INV
    cart = pkg.Handle(capi.default_config(capi.ENV_CARTPOLE))                        # a device-env handle: the envs are not the caller's
    info = capi.DrilExtDeviceInfo()
    UNS = capi.ERR_UNSUPPORTED
    assert lib.dril_ext_act_device(cart._h, obs, None, None, None) == UNS and lib.dril_ext_record_device(cart._h, rew, fl, fl, None, None) == UNS
    assert lib.dril_ext_finish_device(cart._h, obs, None) == UNS and lib.dril_predict_actions_device(cart._h, obs, 5, 1, P(dev.raw), None, None) == UNS
    assert lib.dril_ext_set_action_bounds(cart._h, None, None) == UNS and lib.dril_ext_device_info(cart._h, C.byref(info)) == UNS
    for hh in (h, disc, cart):
        hh.close()


# ---- 7. dril_predict_actions_device ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("space", ["d1_discrete3", "d24_box3_perdim"])
def test_predict_actions_device(pkg, space, B):
    """deterministic and stochastic (the handle's own noise stream) against dril_predict_actions on a twin at the same stream position"""
    D, A, discrete, bounds = SPACES[space]
    hd, hh = _handle(pkg, space, (32, 48), 7), _handle(pkg, space, (32, 48), 7)     # the batch is independent of n_envs
    rng = np.random.default_rng(B)
    obs = rng.uniform(-2, 2, (B, D)).astype(np.float32)
    d_obs = hip_mem.to_device(obs)
    shape, dt = ((B,), np.int32) if discrete else ((B, A), np.float32)
    d_raw, d_env = hip_mem.empty(shape, dt), hip_mem.empty(shape, dt)
    if not discrete:                                                                 # a wide policy, so that sampled and mean actions leave the bounds
        for x in (hd, hh):
            p = x.get_params(); p[-A:] = 1.0; p[:-A] *= 4.0; x.set_params(p)
    for deterministic in (True, False, False):                                       # the second stochastic call draws at the NEXT position of the stream
        hd.predict_actions_device(d_obs, deterministic, d_raw, d_env)
        want = hh.predict_actions(obs, deterministic)
        raw, ea = d_raw.get(), d_env.get()
        assert np.array_equal(raw, want), (space, B, deterministic)
        if discrete:
            assert np.array_equal(ea, raw) and raw.min() >= 1 and raw.max() <= A
        else:
            lo, hi = np.asarray(bounds[0], np.float32), np.asarray(bounds[1], np.float32)
            assert np.array_equal(ea, np.where(lo < hi, np.clip(raw, lo, hi), raw)) and (ea != raw).any()
    hd.predict_actions_device(d_obs, False, None, d_env)                             # one output alone
    assert np.array_equal(d_raw.get(), want)
    hd.close(); hh.close()


# ---- 8. the Python mirror ----------------------------------------------------------------------------------------------------------------------------------------
STEPS = 6


class _ScriptedDeviceEnv:
    """ONE batched env on hip_mem arrays that plays the script whatever the actions are"""

    def __init__(self, pkg, space, E):
        self.pkg, self.space, self.n_envs, self.t = pkg, space, E, 0
        self.dev = _Dev(space, E, steps=STEPS)
        self.seen = []

    def observation_space(self):
        D = SPACES[self.space][0]
        return self.pkg.Box(low=(-2.0,) * D, high=(2.0,) * D)

    def action_space(self):
        D, A, discrete, bounds = SPACES[self.space]
        return self.pkg.Discrete(A) if discrete else self.pkg.Box(low=bounds[0], high=bounds[1])

    def reset_(self):
        pass

    def observe(self):
        return self.dev.obs[self.t]

    def act_(self, actions):
        self.seen.append(actions.get())
        t = self.t; self.t += 1
        return self.dev.rew[t], self.dev.term[t], self.dev.trunc[t], self.dev.tobs[t]


class _ScriptedHostEnv:
    """env i of the same script with the reference's per-env verbs (HostParallelEnv steps a list of these)"""

    def __init__(self, pkg, space, E, i):
        self.pkg, self.space, self.sc, self.i, self.t, self.pending = pkg, space, _script(space, E, STEPS), i, 0, False

    observation_space = _ScriptedDeviceEnv.observation_space
    action_space = _ScriptedDeviceEnv.action_space

    def reset_(self):
        self.pending = False

    def observe(self):                                                               # between act_ and the auto-reset: the terminal observation
        return self.sc["tobs"][self.t - 1, self.i] if self.pending else self.sc["obs"][self.t, self.i]

    def act_(self, a):
        self.t += 1; self.pending = bool(self.sc["trunc"][self.t - 1, self.i])
        return float(self.sc["rew"][self.t - 1, self.i])

    def terminated(self):
        return bool(self.sc["term"][self.t - 1, self.i])

    def truncated(self):
        return bool(self.sc["trunc"][self.t - 1, self.i])


@pytest.mark.parametrize("space", ["d1_discrete3", "d24_box3_perdim"])
def test_python_mirror_fills_the_same_buffer_as_host_parallel_env(pkg, space):
    E = 5
    mk_dev = lambda: pkg.DeviceArrayParallelEnv(_ScriptedDeviceEnv(pkg, space, E), seed=3, empty=hip_mem.empty)
    mk_host = lambda: pkg.HostParallelEnv([_ScriptedHostEnv(pkg, space, E, i) for i in range(E)], seed=3)
    denv, henv = mk_dev(), mk_host()
    alg = pkg.PPO(n_steps=T, batch_size=E, epochs=1)
    agent = pkg.Agent(pkg.ActorCriticLayer(denv.observation_space(), denv.action_space(), hidden_dims=(32, 48)), alg, seed=0)
    bd, bh = (pkg.RolloutBuffer(T, E, alg.gae_lambda, alg.gamma) for _ in range(2))
    pkg.collect_rollout_(bd, agent, alg, denv); pkg.collect_rollout_(bh, agent, alg, henv)
    info = denv.handle.ext_device_info()
    assert info["host_syncs"] == 0 and info["steps_device"] == T and info["per_dim_bounds"] == (not denv.handle.discrete)
    for n in ("observations", "actions", "rewards", "logprobs", "values", "flags"):
        assert np.array_equal(getattr(bd, n), getattr(bh, n)), n
    assert (bd.flags != 0).sum() == 5
    np.testing.assert_allclose(bd.advantages, bh.advantages, atol=TOL["ADVANTAGES"], rtol=TOL["ADVANTAGES"])
    np.testing.assert_allclose(bd.returns, bh.returns, atol=TOL["RETURNS"], rtol=TOL["RETURNS"])
    np.testing.assert_allclose(denv.handle.buffer(pkg._capi.BUF_BOOTSTRAP), henv.handle.buffer(pkg._capi.BUF_BOOTSTRAP), atol=TOL["BOOTSTRAP"], rtol=TOL["BOOTSTRAP"])
    if not denv.handle.discrete:                                                     # the env saw the ClampAdapter's output: no NumPy clip ran on this path
        lo, hi = (np.asarray(b, np.float32) for b in SPACES[space][3])
        raw = bd.actions.reshape(T, E, -1)
        for t in range(T):
            assert np.array_equal(denv.env.seen[t], np.where(lo < hi, np.clip(raw[t], lo, hi), raw[t]))
    # evaluate_agent: fresh envs at the start of the same script; same episode returns and lengths
    ed, eh = mk_dev(), mk_host()
    rd, ld = pkg.evaluate_agent(agent, ed, n_eval_episodes=7, deterministic=True, return_stats=False)
    rh, lh = pkg.evaluate_agent(agent, eh, n_eval_episodes=7, deterministic=True, return_stats=False)
    assert np.array_equal(rd, rh) and np.array_equal(ld, lh) and len(rd) == 7
    sd, sh = pkg.evaluate_agent(agent, mk_dev(), n_eval_episodes=7), pkg.evaluate_agent(agent, mk_host(), n_eval_episodes=7)
    assert sd == sh
    for e in (denv, henv, ed, eh):
        e.handle.close()


def test_torch_example_env_trains_without_host_waits(pkg):
    torch = pytest.importorskip("torch", reason="the example env is written in torch")
    if not torch.cuda.is_available():
        pytest.skip("torch.cuda.is_available() is false on this machine: the torch example env needs torch's own GPU runtime (every other test of this file uses tests/hip_mem.py)")
    spec = importlib.util.spec_from_file_location("ppo_torch_envs", ROOT / "examples" / "ppo_torch_envs.py")
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    E = 64
    env = pkg.DeviceArrayParallelEnv(ex.TorchPendulums(E, max_steps=20), stream=lambda: torch.cuda.current_stream().cuda_stream)
    alg = pkg.PPO(n_steps=32, batch_size=E * 32 // 4, epochs=2)
    agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space(), hidden_dims=(64, 64)), alg, seed=0)
    seen = []

    class _Watch:
        def on_rollout_end(self, loc):
            seen.append(env.handle.ext_device_info()); return True

    stats, timer = pkg.train_(agent, env, alg, 2 * 32 * E, callbacks=[_Watch()])
    assert len(seen) == 2 and all(i["host_syncs"] == 0 and i["steps_device"] == 32 and i["steps_host"] == 0 for i in seen), seen
    assert len(stats["losses"]) == 2 and all(np.isfinite(stats[k]).all() for k in ("losses", "value_losses", "policy_losses", "grad_norms", "explained_variances"))
    assert (env.handle.buffer(pkg._capi.BUF_FLAGS) & 2).any()                        # 20-step episodes in 32-step rollouts: truncation steps were part of it
    env.handle.close()
