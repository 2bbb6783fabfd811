"""GPU (-m gpu): the device-array verbs of a DRIL_ENV_EXTERNAL SAC handle (dril_sac_ext_act_device / _push_device, dril_sac_predict_actions_device,
dril_sac_update_enqueue / dril_sac_flush, dril_sac_ext_set_action_bounds, dril_sac_ext_device_info; docs/sac.md last section) against the HOST verbs of the same
library on a twin handle: same parameters, same noise, same scripted env data (pre-drawn observations, rewards, flags per step; no simulator).  The comparison is
the library with itself, so everything is compared bitwise.  Device memory comes from tests/hip_mem.py, so nothing here needs torch.cuda — except the one test of
the torch example, which says so when it skips.

Script (T = 3 steps): step 0 has no truncation and terminal_obs = NULL; at step 1 env 1 and the last env are truncated; at step 2 env 2 is terminated and
truncated.  terminal_obs rows of envs that were not truncated hold NaN."""
import ctypes as C
import functools
import importlib.util
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import hip_mem

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

T = 3
BATCH = 8
# name -> (obs dim, action dim, (low, high) per dimension)
SPACES = {
    "d3_a1_scalar": (3, 1, ((-2.0,), (2.0,))),
    "d24_a3_perdim": (24, 3, ((-1.0, -0.5, 0.25), (1.0, 0.5, 2.0))),                 # three different intervals
}
SIZES = [5, 257]                                                                     # one block with a tail; several blocks with a tail of one
CAPS = {"wrap": lambda E: 2 * E + 3, "roomy": lambda E: 8 * E}                      # wrap: the third push wraps the ring in the middle of a block
# (space, hidden): each space with one of the two hidden shapes, both sizes and both capacities
NETS = [("d3_a1_scalar", (32, 64)), ("d24_a3_perdim", (64, 64))]
CASES = [(sp, hid, E, cap) for sp, hid in NETS for E in SIZES for cap in CAPS]
RB = ("RB_OBSERVATIONS", "RB_ACTIONS", "RB_REWARDS", "RB_TERMINATED", "RB_TRUNCATED", "RB_NEXT_OBSERVATIONS")


class _Spaces:
    """what make_sac_config reads of an external env"""

    def __init__(self, pkg, space):
        D, A, (lo, hi) = SPACES[space]
        self.kind, self._o, self._a = pkg._capi.ENV_EXTERNAL, pkg.Box(low=(-10.0,) * D, high=(10.0,) * D), pkg.Box(low=lo, high=hi)

    def observation_space(self):
        return self._o

    def action_space(self):
        return self._a


def _handle(pkg, space, hidden, E, cap, seed=5):
    D, A, (lo, hi) = SPACES[space]
    env = _Spaces(pkg, space)
    alg = pkg.SAC(batch_size=BATCH, buffer_capacity=CAPS[cap](E), learning_rate=3e-3)
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=hidden)
    h = pkg.SacHandle(pkg.make_sac_config(env, E, alg, layer, seed=7, per_dim_bounds=True))
    if len(set(lo)) > 1 or len(set(hi)) > 1:
        h.ext_set_action_bounds(lo, hi)
    h.set_params((np.random.default_rng(seed).standard_normal(h.P) * 0.3).astype(np.float32))
    return h


@functools.lru_cache(maxsize=None)
def _script(space, E, steps=T):
    D, A, _ = SPACES[space]
    rng = np.random.default_rng(2000 + 7 * E + D)
    obs = rng.uniform(-2, 2, (steps + 1, E, D)).astype(np.float32)
    rew = rng.standard_normal((steps, E)).astype(np.float32)
    term, trunc = np.zeros((steps, E), np.uint8), np.zeros((steps, E), np.uint8)
    trunc[1, 1] = 1; trunc[1, E - 1] = 1; term[2, 2] = trunc[2, 2] = 1
    for t in range(3, steps):                                                        # longer scripts (the Python mirror): a few more episode ends
        term[t, (t + 1) % E] = 1; trunc[t, (t + 3) % E] = 1
    tobs = rng.uniform(-2, 2, (steps, E, D)).astype(np.float32)
    tobs[trunc == 0] = np.nan
    noise = rng.standard_normal((steps, E, A)).astype(np.float32)
    for a in (obs, rew, term, trunc, tobs, noise):
        a.setflags(write=False)
    return dict(obs=obs, rew=rew, term=term, trunc=trunc, tobs=tobs, noise=noise)


def _tobs(sc, t):
    return sc["tobs"][t] if sc["trunc"][t].any() else None


def _ring(pkg, h):
    return {n: h.replay(getattr(pkg._capi, n)) for n in RB}


def _host_step(h, sc, t, noise=True):
    stored, ea = h.predict_actions(sc["obs"][t], False, sc["noise"][t] if noise else None)
    h.ext_push(sc["obs"][t], stored, sc["rew"][t], sc["term"][t], sc["trunc"][t], sc["obs"][t + 1], _tobs(sc, t))
    return stored, ea


def _stats_rows(stats):
    return [tuple(getattr(s, f) for f in ("actor_loss", "critic_loss", "entropy_loss", "mean_q_values", "entropy_coefficient", "grad_norm", "has_entropy_loss")) for s in stats]


@functools.lru_cache(maxsize=None)
def _host_reference(space, hidden, E, cap, injected=True):
    """the twin: three steps through the HOST verbs, then update(2) twice.  Computed once per case, shared by every test, never changed"""
    import __graft_entry__ as g
    pkg = g.load_package()
    sc = _script(space, E)
    h = _handle(pkg, space, hidden, E, cap)
    stored, envs = [], []
    for t in range(T):
        s, e = _host_step(h, sc, t, injected); stored.append(s); envs.append(e)
    ref = dict(stored=stored, env=envs, ring=_ring(pkg, h), size=h.replay_size(), info=h.ext_device_info())
    st = h.update(2) + h.update(2)
    ref.update(stats=_stats_rows(st), params=h.get_params(), target=h.get_target_params(), log_ent=h.get_log_ent_coef())
    h.close()
    for a in list(ref["ring"].values()) + stored + envs + [ref["params"], ref["target"]]:
        a.setflags(write=False)
    return ref


class _Dev:
    """the script on the device, uploaded on `stream` (None: blocking copies), and the two action output arrays"""

    def __init__(self, space, E, stream=None, steps=T):
        D, A, _ = SPACES[space]
        sc = _script(space, E, steps)
        up = lambda a: hip_mem.to_device(a, stream)
        self.obs = [up(sc["obs"][t]) for t in range(steps + 1)]
        self.rew = [up(sc["rew"][t]) for t in range(steps)]; self.term = [up(sc["term"][t]) for t in range(steps)]; self.trunc = [up(sc["trunc"][t]) for t in range(steps)]
        self.tobs = [up(sc["tobs"][t]) if sc["trunc"][t].any() else None for t in range(steps)]
        self.noise = [up(sc["noise"][t]) for t in range(steps)]
        self.stored, self.env = hip_mem.empty((E, A), np.float32).fill_bytes(0xFF), hip_mem.empty((E, A), np.float32).fill_bytes(0xFF)
        hip_mem.chk(hip_mem.lib().hipStreamSynchronize(None), "hipStreamSynchronize")   # the fills ran on the null stream, which a stream of the test's own does not wait for


def _device_step(h, dev, t, stream=None, noise=True):
    sp = None if stream is None else stream.ptr
    h.ext_act_device(dev.obs[t], False, dev.noise[t] if noise else None, dev.stored, dev.env, sp)
    stored, ea = dev.stored.get(stream), dev.env.get(stream)                         # stream None: a blocking copy on the null stream, which the library made wait
    h.ext_push_device(dev.rew[t], dev.term[t], dev.trunc[t], dev.obs[t + 1], dev.tobs[t], sp)
    return stored, ea


def _assert_ring(pkg, h, ref, what=""):
    assert h.replay_size() == ref["size"], what
    got = _ring(pkg, h)
    for n in RB:
        assert np.array_equal(got[n], ref["ring"][n], equal_nan=True), (what, n)
    return got


# ---- 1. ring equality -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("injected", [True, False], ids=["noise_injected", "noise_handle_stream"])
@pytest.mark.parametrize("space,hidden,E,cap", CASES)
def test_device_steps_fill_the_ring_of_the_host_verbs(pkg, space, hidden, E, cap, injected):
    sc, ref = _script(space, E), _host_reference(space, hidden, E, cap, injected)
    h, dev = _handle(pkg, space, hidden, E, cap), _Dev(space, E)
    for t in range(T):
        stored, ea = _device_step(h, dev, t, noise=injected)
        assert np.array_equal(stored, ref["stored"][t]) and np.array_equal(ea, ref["env"][t]), (t, np.abs(stored - ref["stored"][t]).max())
    lo, hi = (np.asarray(b, np.float32) for b in SPACES[space][2])
    assert (ea >= lo).all() and (ea <= hi).all() and np.isfinite(stored).all()
    got = _assert_ring(pkg, h, ref)
    n = CAPS[cap](E)
    assert h.replay_size() == min(3 * E, n)
    # the ring's last 3E (or capacity) rows in logical order are the script's steps: truncated rows hold the terminal observation, no NaN came from the NaN rows
    rows = min(3 * E, n)
    nxt = np.concatenate([np.where(sc["trunc"][t][:, None] != 0, sc["tobs"][t], sc["obs"][t + 1]) for t in range(T)])[-rows:]
    term = np.concatenate([sc["term"][t] for t in range(T)])[-rows:]
    trunc = np.concatenate([sc["trunc"][t] for t in range(T)])[-rows:]
    assert not np.isnan(got["RB_NEXT_OBSERVATIONS"][term == 0]).any()
    assert np.array_equal(got["RB_NEXT_OBSERVATIONS"], nxt) and np.array_equal(got["RB_TRUNCATED"], trunc) and trunc.sum() >= 2
    info = h.ext_device_info()
    assert info["launches"] == 6 * T, info                                           # per step: the observation's copy, three forward launches, the head; one push (docs/sac.md)
    assert info["host_syncs"] == 0 and info["steps_device"] == T and info["steps_host"] == 0 and ref["info"]["steps_host"] == T
    assert info["per_dim_bounds"] == (space == "d24_a3_perdim")
    h.close()


# ---- 2. random actions ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space,E", [("d3_a1_scalar", 257), ("d24_a3_perdim", 5), ("d24_a3_perdim", 257)])
def test_random_actions_are_numpy_float32_arithmetic(pkg, space, E):
    D, A, (lo, hi) = SPACES[space]
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    h, dev = _handle(pkg, space, (32, 64), E, "roomy"), _Dev(space, E)
    u = np.random.default_rng(3).random((E, A), dtype=np.float32)
    u[0, 0] = 0.0; u[-1, -1] = np.nextafter(np.float32(1), np.float32(0))
    h.ext_act_device(dev.obs[0], True, hip_mem.to_device(u), dev.stored, dev.env)
    stored, ea = dev.stored.get(), dev.env.get()
    want = lo + u * (hi - lo)                                                        # float32 throughout: each operation rounded on its own
    assert want.dtype == np.float32 and np.array_equal(stored, want) and np.array_equal(ea, want)
    assert (ea >= lo).all() and (ea <= hi).all()
    h.ext_push_device(dev.rew[0], dev.term[0], dev.trunc[0], dev.obs[1], None)
    assert np.array_equal(h.replay(pkg._capi.RB_ACTIONS), want)                      # the env-space action is what the ring stores (:72)
    h.ext_act_device(dev.obs[1], True, None, dev.stored, dev.env)                    # the handle's own stream
    stored, ea = dev.stored.get(), dev.env.get()
    assert np.array_equal(stored, ea) and (ea >= lo).all() and (ea <= hi).all() and np.unique(ea).size > 1
    assert h.ext_device_info()["host_syncs"] == 0
    h.close()


# ---- 3. enqueued updates ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space,hidden,E,cap", [c for c in CASES if c[2] == 5 or c[3] == "wrap"])
def test_enqueued_updates_are_the_updates(pkg, space, hidden, E, cap):
    capi = pkg._capi
    ref = _host_reference(space, hidden, E, cap)
    h, dev = _handle(pkg, space, hidden, E, cap), _Dev(space, E)
    for t in range(T):
        _device_step(h, dev, t)
    h.update_enqueue(2); h.update_enqueue(2)
    info = h.ext_device_info()
    assert info["pending_updates"] == 4 and info["pending_capacity"] >= 4096 and info["pending_capacity"] == capi.SAC_PENDING_CAPACITY and info["flushes"] == 0
    stats = h.flush()
    info = h.ext_device_info()
    assert info["pending_updates"] == 0 and info["flushes"] == 1 and info["host_syncs"] == 0
    assert _stats_rows(stats) == ref["stats"] and len(stats) == 4
    assert np.array_equal(h.get_params(), ref["params"]) and np.array_equal(h.get_target_params(), ref["target"]) and h.get_log_ent_coef() == ref["log_ent"]
    assert not np.array_equal(ref["params"], (np.random.default_rng(5).standard_normal(h.P) * 0.3).astype(np.float32))   # the updates moved the parameters
    with pytest.raises(pkg.DrilError) as e:                                          # a request the pending table cannot hold: refused, nothing enqueued, no implicit wait
        h.update_enqueue(info["pending_capacity"] + 1)
    assert e.value.code == capi.ERR_INVALID_ARG and "flush first" in str(e.value)
    assert h.ext_device_info()["pending_updates"] == 0 and np.array_equal(h.get_params(), ref["params"]) and h.flush() == []
    h.close()


def test_update_enqueue_on_an_empty_ring(pkg):
    h = _handle(pkg, "d3_a1_scalar", (32, 64), 5, "roomy")
    with pytest.raises(pkg.DrilError) as e:
        h.update_enqueue(1)
    assert e.value.code == pkg._capi.ERR_NOT_INITIALISED
    assert h.flush() == []                                                           # legal with nothing pending
    h.close()


# ---- 4. mixed loop ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space,hidden,E,cap", [c for c in CASES if c[3] == "wrap"])
def test_host_and_device_steps_mix(pkg, space, hidden, E, cap):
    sc, ref = _script(space, E), _host_reference(space, hidden, E, cap)
    h, dev = _handle(pkg, space, hidden, E, cap), _Dev(space, E)
    _host_step(h, sc, 0)
    stored, ea = _device_step(h, dev, 1)
    assert np.array_equal(stored, ref["stored"][1]) and np.array_equal(ea, ref["env"][1])
    _host_step(h, sc, 2)
    _assert_ring(pkg, h, ref)
    info = h.ext_device_info()
    assert info["steps_device"] == 1 and info["steps_host"] == 2 and info["host_syncs"] == 0
    h.close()


# ---- 5. caller stream -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_stream", [True, False], ids=["own_stream", "null_stream"])
def test_caller_stream_orders_inputs_and_outputs(pkg, own_stream):
    space, hidden, E, cap = "d24_a3_perdim", (64, 64), 257, "wrap"
    ref = _host_reference(space, hidden, E, cap)
    stream = hip_mem.Stream() if own_stream else None
    h = _handle(pkg, space, hidden, E, cap)
    dev = _Dev(space, E, stream)                                                     # async uploads on the test's stream: the library must order itself behind them
    for t in range(T):
        stored, ea = _device_step(h, dev, t, stream)                                 # outputs read on that stream only
        assert np.array_equal(stored, ref["stored"][t]) and np.array_equal(ea, ref["env"][t]), t
    h.update_enqueue(2); h.update_enqueue(2)
    info = h.ext_device_info()
    assert info["host_syncs"] == 0 and info["flushes"] == 0 and info["pending_updates"] == 4
    assert _stats_rows(h.flush()) == ref["stats"]                                    # the end: the one drain
    _assert_ring(pkg, h, ref)
    assert np.array_equal(h.get_params(), ref["params"])
    h.close()
    if stream is not None:
        stream.close()


# ---- 6. sticky error --------------------------------------------------------------------------------------------------------------------------------------------------
def test_truncation_without_terminal_obs_is_a_sticky_error(pkg):
    space, hidden, E, cap = "d3_a1_scalar", (32, 64), 257, "roomy"
    capi, sc, ref = pkg._capi, _script(space, E), _host_reference(space, hidden, E, cap)
    h, dev = _handle(pkg, space, hidden, E, cap), _Dev(space, E)
    _device_step(h, dev, 0)
    for t in (1, 2):                                                                 # truncated envs, terminal_obs = NULL
        h.ext_act_device(dev.obs[t], False, dev.noise[t], dev.stored, dev.env)
        h.ext_push_device(dev.rew[t], dev.term[t], dev.trunc[t], dev.obs[t + 1], None)
    with pytest.raises(pkg.DrilError) as e:
        h.flush()
    assert e.value.code == capi.ERR_INVALID_ARG and "terminal_obs" in str(e.value)
    assert h.flush() == []                                                           # returned once, then cleared
    nxt = h.replay(capi.RB_NEXT_OBSERVATIONS)                                        # documented: the rows stay, with next_obs where the terminal observation belongs
    assert np.array_equal(nxt, np.concatenate([sc["obs"][t + 1] for t in range(T)]))
    for t in range(T):                                                               # the handle stays usable: a correct sequence produces the twin's rows
        _device_step(h, dev, t)
    assert h.flush() == [] and h.replay_size() == 6 * E
    for n in RB:
        assert np.array_equal(h.replay(getattr(capi, n))[3 * E:], ref["ring"][n], equal_nan=True), n
    h.close()


# ---- 7. predict_actions_device ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space,hidden", NETS)
def test_predict_actions_device_matches_the_host_verb(pkg, space, hidden):
    D, A, _ = SPACES[space]
    hd, hh = _handle(pkg, space, hidden, 5, "roomy"), _handle(pkg, space, hidden, 5, "roomy")
    rng = np.random.default_rng(17)
    nmax = max(5, 2 * BATCH)
    for B in (5, 40, 257):                                                           # 40 and 257 > nmax = 16: chunks, the last one partial
        assert B <= nmax or B % nmax
        obs, nz = rng.uniform(-2, 2, (B, D)).astype(np.float32), rng.standard_normal((B, A)).astype(np.float32)
        d_obs, d_nz = hip_mem.to_device(obs), hip_mem.to_device(nz)
        d_raw, d_env = hip_mem.empty((B, A), np.float32).fill_bytes(0xFF), hip_mem.empty((B, A), np.float32).fill_bytes(0xFF)
        for det, noise, d_noise in ((True, None, None), (False, nz, d_nz), (False, None, None)):   # the last: both handles' own streams, chunk by chunk
            hd.predict_actions_device(d_obs, det, d_noise, d_raw, d_env)
            want_raw, want_env = hh.predict_actions(obs, det, noise)
            assert np.array_equal(d_raw.get(), want_raw) and np.array_equal(d_env.get(), want_env), (B, det, noise is None)
        d_env.fill_bytes(0xFF)
        hd.predict_actions_device(d_obs, True, None, None, d_env)                    # one output alone
        assert np.array_equal(d_env.get(), hh.predict_actions(obs, True)[1])
    info = hd.ext_device_info()
    assert info["host_syncs"] == 0 and info["steps_device"] == 0                     # the pending step is not touched
    hd.close(); hh.close()


# ---- 8. statuses ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_statuses(pkg):
    capi = pkg._capi
    space, E = "d24_a3_perdim", 5
    D, A, _ = SPACES[space]
    h, dev = _handle(pkg, space, (64, 64), E, "roomy"), _Dev(space, E)
    f, H = h._f, h._h
    P = lambda a: None if a is None else C.c_void_p(a.ptr)
    inv, msg = capi.ERR_INVALID_ARG, lambda: (h._f("last_error")(H) or b"").decode()
    obs, rew, te, tr, out = P(dev.obs[0]), P(dev.rew[0]), P(dev.term[0]), P(dev.trunc[0]), P(dev.env)
    # null pointers
    assert f("ext_act_device")(H, None, 0, None, None, None, None) == inv
    assert f("ext_push_device")(H, rew, te, tr, obs, None, None) == inv and "without a preceding" in msg()          # push before act
    assert f("predict_actions_device")(H, None, 5, 0, None, out, out, None) == inv
    assert f("predict_actions_device")(H, obs, 0, 0, None, out, out, None) == inv
    assert f("predict_actions_device")(H, obs, 5, 0, None, None, None, None) == inv                                  # both outputs NULL
    assert f("ext_set_action_bounds")(H, None, None) == inv
    assert f("update_enqueue")(H, 0) == inv
    # a host pointer passed as a device array; a too-short allocation
    host = np.zeros((E, D), np.float32)
    assert f("ext_act_device")(H, host.ctypes.data_as(C.c_void_p), 0, None, None, out, None) == inv and "d_obs" in msg() and "not memory of device" in msg()
    short = hip_mem.empty((E * D - 1,), np.float32)
    assert f("ext_act_device")(H, P(short), 0, None, None, out, None) == inv and "d_obs" in msg() and "ends before" in msg()
    short_out = hip_mem.empty((E * A - 1,), np.float32)
    assert f("ext_act_device")(H, obs, 0, None, None, P(short_out), None) == inv and "d_env_actions" in msg()
    assert f("predict_actions_device")(H, obs, 6, 0, None, out, None, None) == inv and "ends before" in msg()       # batch 6 of a 5-row array
    assert h.ext_device_info()["launches"] == 0                                      # nothing was enqueued by any refused call
    # act twice; null arguments of a push with a pending act
    assert f("ext_act_device")(H, obs, 0, None, None, out, None) == capi.OK
    assert f("ext_act_device")(H, obs, 0, None, None, out, None) == inv and "ext_push_device" in msg()
    for args in ((None, te, tr, obs), (rew, None, tr, obs), (rew, te, None, obs), (rew, te, tr, None)):
        assert f("ext_push_device")(H, *args, None, None) == inv
    assert f("ext_push_device")(H, rew, te, tr, P(short), None, None) == inv and "d_next_obs" in msg()
    z = np.zeros(E, np.float32)
    with pytest.raises(pkg.DrilError):                                               # the host push may not overtake a pending device act
        h.ext_push(np.zeros((E, D)), np.zeros((E, A)), z, z, z, np.zeros((E, D)))
    assert f("ext_push_device")(H, rew, te, tr, obs, None, None) == capi.OK and h.replay_size() == E
    # bounds
    for lo, hi, dim in (((-1, 0.5, 0), (1, 0.5, 1), "dimension 1"), ((-1, -1, 2), (1, 1, 1), "dimension 2"), ((np.nan, 0, 0), (1, 1, 1), "dimension 0"), ((0, 0, 0), (1, np.inf, 1), "dimension 1")):
        with pytest.raises(pkg.DrilError) as e:
            h.ext_set_action_bounds(lo, hi)
        assert e.value.code == inv and dim in str(e.value), (dim, str(e.value))
    with pytest.raises(ValueError, match="action_dim"):
        h.ext_set_action_bounds((0, 0), (1, 1))
    h.close()
    # every verb on a device-env handle
    env = pkg.PendulumEnv(max_steps=200)
    alg = pkg.SAC(batch_size=BATCH, buffer_capacity=64)
    hp = pkg.SacHandle(pkg.make_sac_config(env, 8, alg, pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(32, 32))))
    f, H, uns = hp._f, hp._h, capi.ERR_UNSUPPORTED
    lohi = np.asarray([-1.0], np.float32), np.asarray([1.0], np.float32)
    calls = {"ext_act_device": lambda: f("ext_act_device")(H, obs, 0, None, None, out, None),
             "ext_push_device": lambda: f("ext_push_device")(H, rew, te, tr, obs, None, None),
             "predict_actions_device": lambda: f("predict_actions_device")(H, obs, 5, 0, None, out, None, None),
             "update_enqueue": lambda: f("update_enqueue")(H, 1), "flush": lambda: f("flush")(H, None, 0, None),
             "ext_set_action_bounds": lambda: f("ext_set_action_bounds")(H, lohi[0].ctypes.data_as(C.c_void_p), lohi[1].ctypes.data_as(C.c_void_p)),
             "ext_device_info": lambda: f("ext_device_info")(H, C.byref(capi.DrilSacExtDeviceInfo()))}
    for verb, call in calls.items():                                                 # each with a message of its own
        assert call() == uns, verb
        m = (hp._f("last_error")(H) or b"").decode()
        assert m.startswith("dril_sac_" + verb + ":") and "DRIL_ENV_EXTERNAL" in m, (verb, m)
    hp.close()


def test_per_dimension_bounds_reach_the_host_verb_and_the_policy(pkg):
    """dril_sac_ext_set_action_bounds rewrites the one table: dril_sac_predict_actions and dril_policy_from_sac_handle honour it with no code of their own"""
    space = "d24_a3_perdim"
    D, A, (lo, hi) = SPACES[space]
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    h = _handle(pkg, space, (64, 64), 5, "roomy")
    obs = np.random.default_rng(1).uniform(-2, 2, (64, D)).astype(np.float32)
    raw, ea = h.predict_actions(obs, True)
    th = np.tanh(raw)                                                                # to_env(TanhScaleAdapter): low + (tanh(raw) + 1) / 2 * (high - low)
    np.testing.assert_allclose(ea, lo + (th + 1) * 0.5 * (hi - lo), rtol=1e-5, atol=1e-6)
    assert (ea >= lo).all() and (ea <= hi).all()
    pol = pkg.NeuralPolicy.from_handle(h)
    assert np.array_equal(np.asarray(pol.desc.action_low[:A], np.float32), lo) and np.array_equal(np.asarray(pol.desc.action_high[:A], np.float32), hi)
    pol.close(); h.close()


# ---- 9. the Python mirror ---------------------------------------------------------------------------------------------------------------------------------------------
STEPS = 5


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
        lo, hi = SPACES[self.space][2]
        return self.pkg.Box(low=lo, high=hi)

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

    def __init__(self, pkg, space, E, i, seen):
        self.pkg, self.space, self.sc, self.i, self.t, self.pending, self.seen = pkg, space, _script(space, E, STEPS), i, 0, False, seen

    observation_space = _ScriptedDeviceEnv.observation_space
    action_space = _ScriptedDeviceEnv.action_space

    def reset_(self):
        self.pending = False

    def observe(self):                                                               # between act_ and the auto-reset: the terminal observation
        return self.sc["tobs"][self.t - 1, self.i] if self.pending else self.sc["obs"][self.t, self.i]

    def act_(self, a):
        self.seen.setdefault(self.t, {})[self.i] = np.asarray(a, np.float32).ravel()
        self.t += 1; self.pending = bool(self.sc["trunc"][self.t - 1, self.i])
        return float(self.sc["rew"][self.t - 1, self.i])

    def terminated(self):
        return bool(self.sc["term"][self.t - 1, self.i])

    def truncated(self):
        return bool(self.sc["trunc"][self.t - 1, self.i])


def test_python_mirror_with_per_dimension_bounds(pkg):
    """the same loop on the Box with three different intervals.  HostParallelEnv refuses such a Box (one pair per handle), so the twin is the host verbs driven here:
    predict_actions + ext_push + update per iteration on a handle with the same seed, parameters and bounds"""
    space, E, iters = "d24_a3_perdim", 5, 4
    lo, hi = SPACES[space][2]
    denv = pkg.DeviceArrayParallelEnv(_ScriptedDeviceEnv(pkg, space, E), seed=3, empty=hip_mem.empty)
    alg = pkg.SAC(start_steps=0, train_freq=1, gradient_steps=2, batch_size=BATCH, buffer_capacity=3 * E + 2, learning_rate=3e-3)
    mk = lambda: pkg.SACAgent(pkg.SACLayer(denv.observation_space(), denv.action_space(), hidden_dims=(32, 64)), alg, seed=0)
    ad, rbd, sd, td = pkg.sac_train_(mk(), denv, alg, iters * E)
    assert td["host_syncs"] == 0 and td["flushes"] >= 1 and rbd.handle.ext_device_info()["per_dim_bounds"], td
    sc, agent = _script(space, E, STEPS), mk()
    h = pkg.SacHandle(pkg.make_sac_config(denv, E, alg, agent.layer, seed=3, per_dim_bounds=True))
    h.ext_set_action_bounds(lo, hi)
    h.set_params(pkg.sac_flatten_params(agent.parameters)); h.set_target_params(agent.q_target_parameters); h.set_log_ent_coef(agent.log_ent_coef)
    stats = []
    for t in range(iters):
        stored, ea = h.predict_actions(sc["obs"][t])
        assert np.array_equal(denv.env.seen[t], ea), t                               # the env was handed the host verb's env-space actions
        h.ext_push(sc["obs"][t], stored, sc["rew"][t], sc["term"][t], sc["trunc"][t], sc["obs"][t + 1], sc["tobs"][t] if sc["trunc"][t].any() else None)
        stats += h.update(2)
    for n in RB:
        assert np.array_equal(rbd.handle.replay(getattr(pkg._capi, n)), h.replay(getattr(pkg._capi, n)), equal_nan=True), n
    assert np.array_equal(pkg.sac_flatten_params(ad.parameters), h.get_params()) and np.array_equal(ad.q_target_parameters, h.get_target_params())
    assert ad.log_ent_coef == h.get_log_ent_coef() and sd["critic_losses"] == [s.critic_loss for s in stats] and sd["grad_norms"] == [s.grad_norm for s in stats]
    henv = pkg.HostParallelEnv([_ScriptedHostEnv(pkg, space, E, i, {}) for i in range(E)], seed=3)
    with pytest.raises(NotImplementedError, match="one \\(low, high\\) pair"):       # the host loop is as it was
        pkg.sac_train_(mk(), henv, alg, E)
    h.close(); rbd.handle.close()


def test_flush_error_carries_the_statistics_rows(pkg):
    """a flush that returns the sticky error has emptied the pending table: the rows travel in the exception, and the training loop keeps them"""
    space, E = "d3_a1_scalar", 5
    h, dev = _handle(pkg, space, (32, 64), E, "roomy"), _Dev(space, E)
    _device_step(h, dev, 0)
    h.ext_act_device(dev.obs[1], False, dev.noise[1], None, dev.env)
    h.ext_push_device(dev.rew[1], dev.term[1], dev.trunc[1], dev.obs[2], None)        # truncated envs, terminal_obs = NULL
    h.update_enqueue(2)
    with pytest.raises(pkg.DrilError) as e:
        h.flush()
    assert "terminal_obs" in str(e.value) and len(e.value.stats) == 2 and all(np.isfinite(s.critic_loss) for s in e.value.stats)
    assert h.ext_device_info()["pending_updates"] == 0 and h.flush() == []
    h.close()


def test_python_mirror_trains_like_host_parallel_env(pkg, space="d3_a1_scalar"):
    E, iters = 5, 4
    seen_host = {}
    denv = pkg.DeviceArrayParallelEnv(_ScriptedDeviceEnv(pkg, space, E), seed=3, empty=hip_mem.empty)
    henv = pkg.HostParallelEnv([_ScriptedHostEnv(pkg, space, E, i, seen_host) for i in range(E)], seed=3)
    alg = pkg.SAC(start_steps=0, train_freq=1, gradient_steps=2, batch_size=BATCH, buffer_capacity=3 * E + 2, learning_rate=3e-3)
    mk = lambda: pkg.SACAgent(pkg.SACLayer(denv.observation_space(), denv.action_space(), hidden_dims=(32, 64)), alg, seed=0)
    ad, rbd, sd, td = pkg.sac_train_(mk(), denv, alg, iters * E)
    ah, rbh, sh, th = pkg.sac_train_(mk(), henv, alg, iters * E)
    assert td["iterations"] == th["iterations"] == iters and ad.steps_taken == ah.steps_taken == iters * E and ad.gradient_updates == ah.gradient_updates == 2 * iters
    assert td["host_syncs"] == 0 and td["flushes"] >= 1, td
    info = rbd.handle.ext_device_info()
    assert info["steps_device"] == iters and info["steps_host"] == 0 and info["per_dim_bounds"] == (space == "d24_a3_perdim")
    for n in RB:
        assert np.array_equal(rbd.handle.replay(getattr(pkg._capi, n)), rbh.handle.replay(getattr(pkg._capi, n)), equal_nan=True), n
    assert rbd.handle.replay_size() == 3 * E + 2                                     # wrapped
    assert np.array_equal(pkg.sac_flatten_params(ad.parameters), pkg.sac_flatten_params(ah.parameters))
    assert np.array_equal(ad.q_target_parameters, ah.q_target_parameters) and ad.log_ent_coef == ah.log_ent_coef
    for k in ("actor_losses", "critic_losses", "entropy_losses", "entropy_coefficients", "q_values", "grad_norms"):
        assert sd[k] == sh[k] and len(sd[k]) == 2 * iters, k
    for t in range(iters):                                                           # both envs were handed the same env-space actions
        assert np.array_equal(denv.env.seen[t], np.stack([seen_host[t][i] for i in range(E)])), t
    # a callback reads statistics that are complete when it runs: one flush per hook
    calls = []

    class _Watch:
        def on_rollout_end(self, loc):
            calls.append((len(loc["training_stats"]["critic_losses"]), loc["replay_buffer"].handle.ext_device_info()["pending_updates"])); return True

    denv2 = pkg.DeviceArrayParallelEnv(_ScriptedDeviceEnv(pkg, space, E), seed=3, empty=hip_mem.empty)
    a2, rbd2, s2, t2 = pkg.sac_train_(mk(), denv2, alg, iters * E, callbacks=[_Watch()])
    assert calls == [(2 * i, 0) for i in range(iters)] and t2["host_syncs"] == 0 and t2["flushes"] == iters + 1
    assert np.array_equal(pkg.sac_flatten_params(a2.parameters), pkg.sac_flatten_params(ah.parameters)) and s2["critic_losses"] == sh["critic_losses"]
    with pytest.raises(NotImplementedError, match="normalize"):
        pkg.sac_train_(mk(), denv2, alg, E, normalize=dict())
    # evaluation over the same script: deterministic actions of the trained agent, episode accounting on the host
    ed = pkg.DeviceArrayParallelEnv(_ScriptedDeviceEnv(pkg, space, E), seed=3, empty=hip_mem.empty)
    er, el = pkg.sac_evaluate_agent(ad, ed, n_eval_episodes=4, deterministic=True, return_stats=False)
    sc = _script(space, E, STEPS)
    want_r, want_l, cur_r, cur_l = [], [], np.zeros(E, np.float32), np.zeros(E, np.int64)
    for t in range(STEPS):
        cur_r += sc["rew"][t]; cur_l += 1
        for i in np.nonzero(sc["term"][t] | sc["trunc"][t])[0]:
            if len(want_r) < 4:
                want_r.append(float(cur_r[i])); want_l.append(int(cur_l[i])); cur_r[i] = 0; cur_l[i] = 0
        if len(want_r) >= 4:
            break
    assert np.array_equal(er, np.asarray(want_r, np.float32)) and np.array_equal(el, want_l)
    want_act = rbh.handle.predict_actions(sc["obs"][0], True)[1]
    assert np.array_equal(ed.env.seen[0], want_act)                                 # predict_actions_device handed the env what the host verb computes
    for r in (rbd, rbh, rbd2):
        r.handle.close()


# ---- 10. the example --------------------------------------------------------------------------------------------------------------------------------------------------
def test_torch_example_trains_without_host_waits(pkg):
    torch = pytest.importorskip("torch", reason="the example env is written in torch")
    if not torch.cuda.is_available():
        pytest.skip("torch.cuda.is_available() is false on this machine: the torch example env needs torch's own GPU runtime (every other test of this file uses tests/hip_mem.py)")
    r = subprocess.run([sys.executable, str(ROOT / "examples" / "sac_torch_envs.py"), "--iterations", "40", "--envs", "64"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "host_syncs=0" in r.stdout and "steps_device=" in r.stdout, r.stdout[-2000:]
