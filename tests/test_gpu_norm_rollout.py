"""GPU (-m gpu): the one-launch collection of a normalising built-in handle (dril_norm_rollout_enable, rollout_norm_kernel, docs/normalized_rollout.md) against the
step-granular collection of a twin handle — policy_kernel -> norm_step_kernel -> norm_apply_kernel per env step — and against the CPU oracle.

What must be bit-equal and what is held to a tolerance:
  bit-equal   observations, actions, rewards, log-probabilities, flags, the running statistics and their counts, env state and counters, the monitor's figures, the
              wrapper's original observations / rewards: the actor's forward is the one of rollout_duo_kernel (bit-equal to policy_kernel's for these outputs,
              test_stepwise_path_equals_persistent_kernel), the simulator is one definition, and the batch moments are summed by norm_step_kernel's own tree
  1e-6        values, last values, bootstrap values: the critic's two forward forms, the atol test_stepwise_path_equals_persistent_kernel grants the same two forms
  2e-6 / (1 - gamma lambda)   advantages and returns: GAE's geometric sum over delta_t = r_t + gamma V_{t+1} - V_t, each delta off by at most (1 + gamma) 1e-6 < 2e-6
Worst measured value difference over every case below (MI355X): see docs/normalized_rollout.md, "Equality"."""
import numpy as np
import pytest

import split_budget
from test_gpu_env_plugin import _co

pytestmark = pytest.mark.gpu
T, L = 40, 13


def _cfg(pkg, kind, **kw):
    c = pkg._capi.default_config(kind)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _params(P, seed, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(P) * scale).astype(np.float32)


def _mk(pkg, kind, E, flags, optin, n_steps=T, seed=21, params=None, **kw):
    kw = {**dict(n_envs=E, n_steps=n_steps, episode_len=L, batch_size=E * n_steps, epochs=1, monitor_window=64, norm_training=1, norm_obs=flags[0], norm_reward=flags[1]), **kw}
    h = pkg.Handle(_cfg(pkg, kind, **kw))
    h.set_params(_params(h.P, 8, 0.4) if params is None else params)
    h.env_reset(seed)
    if optin:
        h.norm_rollout_enable(True)
    return h


def _noise(h, rng):
    N = h.cfg.n_envs * h.cfg.n_steps
    return rng.random(N) if h.discrete else rng.standard_normal((N, h.A)).astype(np.float32)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _assert_left_equal(a, b, where):
    """what a collection leaves on the handle, bit for bit: statistics and counts, env state and counters, the monitor, the wrapper's originals"""
    sa, sb = a.norm_get_stats(), b.norm_get_stats()
    assert sa.keys() == sb.keys()
    for k in sa:
        np.testing.assert_array_equal(_bits(np.asarray(sa[k])), _bits(np.asarray(sb[k])), err_msg=f"{where}: statistics, {k}")
    for x, y in zip(a.env_get_state(), b.env_get_state()):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"{where}: env state")
    np.testing.assert_array_equal(np.asarray(a.monitor_stats(), np.float64), np.asarray(b.monitor_stats(), np.float64), err_msg=f"{where}: monitor")
    for x, y, n in zip(a.norm_get_original(), b.norm_get_original(), ("obs", "rewards")):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"{where}: original {n}")


def _assert_rollout_equal(capi, a, b, where):
    """buffers of handle a (one launch) against twin b (step-granular) -> the worst |difference| of the values, last values and truncated bootstrap values"""
    for w in (capi.BUF_OBSERVATIONS, capi.BUF_ACTIONS, capi.BUF_REWARDS, capi.BUF_LOGPROBS, capi.BUF_FLAGS):
        np.testing.assert_array_equal(_bits(a.buffer(w)), _bits(b.buffer(w)), err_msg=f"{where}: buffer {w}")
    fl = a.buffer(capi.BUF_FLAGS).reshape(-1)
    tr = (fl & 2).astype(bool)
    worst = 0.0
    for w in (capi.BUF_VALUES, capi.BUF_LAST_VALUES, capi.BUF_BOOTSTRAP):
        x, y = a.buffer(w).reshape(-1).astype(np.float64), b.buffer(w).reshape(-1).astype(np.float64)
        if w == capi.BUF_BOOTSTRAP:
            x, y = x[tr], y[tr]
        if x.size:
            worst = max(worst, float(np.abs(x - y).max()))
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-6, err_msg=f"{where}: buffer {w}")
    bound = 2e-6 / (1.0 - a.cfg.gamma * a.cfg.gae_lambda)
    for w in (capi.BUF_ADVANTAGES, capi.BUF_RETURNS):
        np.testing.assert_allclose(a.buffer(w).astype(np.float64), b.buffer(w).astype(np.float64), rtol=0, atol=bound, err_msg=f"{where}: buffer {w}")
    _assert_left_equal(a, b, where)
    return worst, tr.any(), fl.astype(bool).any()


@pytest.mark.parametrize("flags", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("E", [1, 5, 32, 33, 128])      # batch variance 0; ragged single tile; full tile; ragged second tile; the cap (two waves of moments)
@pytest.mark.parametrize("kind", [0, 1, 2, 6])          # Categorical D = 4; DiagGaussian, truncation only; scaled; D = 6, three actions
def test_equals_step_granular_path(pkg, kind, E, flags):
    """two consecutive rollouts, the first on injected noise, the second on the envs' Philox streams: handle A with the opt-in, twin B without"""
    capi = pkg._capi
    a, b = _mk(pkg, kind, E, flags, True), _mk(pkg, kind, E, flags, False)
    rng = np.random.default_rng(2)
    truncs = ends = False
    for r in range(2):
        if r == 0:
            nz = _noise(a, rng); a.set_noise(nz); b.set_noise(nz)
        a.collect_rollout(); b.collect_rollout()
        ia, ib = a.norm_rollout_info(), b.norm_rollout_info()
        assert ia["last_collection_path"] == 1 and ib["last_collection_path"] == 0 and ia["total_stepwise_fallbacks"] == 0
        worst, tr, en = _assert_rollout_equal(capi, a, b, f"kind {kind}, E {E}, flags {flags}, rollout {r}")
        print(f"[norm rollout] kind {kind} E {E} flags {flags} rollout {r}: worst value difference {worst:.3e}")
        truncs |= bool(tr); ends |= bool(en)
    assert truncs and ends and a.monitor_stats()[2] > 0            # nothing above compared empty sets
    sa = a.norm_get_stats()
    assert sa["obs_count"] == (2 * E * (T + 1) if flags[0] else 0) and sa["ret_count"] == (2 * E * T if flags[1] else 0)
    a.close(); b.close()


@pytest.mark.parametrize("kind,E", [(1, 33), (0, 128)])
def test_leaves_what_the_loop_leaves(pkg, kind, E):
    """one opt-in rollout, the opt-in switched off, one step-granular rollout == two step-granular rollouts; the step verbs in between see the same envs"""
    capi = pkg._capi
    a, b = _mk(pkg, kind, E, (1, 1), True), _mk(pkg, kind, E, (1, 1), False)
    a.collect_rollout(); b.collect_rollout()
    _assert_left_equal(a, b, "after the first rollout")
    np.testing.assert_array_equal(_bits(a.env_observe(True)), _bits(b.env_observe(True)))
    _assert_left_equal(a, b, "after env_observe")
    a.norm_rollout_enable(False)
    a.collect_rollout(); b.collect_rollout()
    assert a.norm_rollout_info()["last_collection_path"] == 0
    for w in range(10):
        if w == capi.BUF_BOOTSTRAP:
            tr = (a.buffer(capi.BUF_FLAGS).reshape(-1) & 2).astype(bool)
            np.testing.assert_array_equal(_bits(a.buffer(w).reshape(-1)[tr]), _bits(b.buffer(w).reshape(-1)[tr]))
        else:
            np.testing.assert_array_equal(_bits(a.buffer(w)), _bits(b.buffer(w)), err_msg=f"buffer {w}")       # the same kernels on the same state: every buffer, values included
    _assert_left_equal(a, b, "after the second rollout")
    a.close(); b.close()


@pytest.mark.parametrize("kind", [1, 0])
def test_frozen_statistics(pkg, kind):
    """norm_training = 0 with set statistics: statistics and counts untouched, buffers equal the step-granular twin's"""
    capi = pkg._capi
    E = 33
    a, b = _mk(pkg, kind, E, (1, 1), True, norm_training=0), _mk(pkg, kind, E, (1, 1), False, norm_training=0)
    rng = np.random.default_rng(5)
    om, ov = rng.standard_normal(a.D).astype(np.float32) * 0.3, (0.5 + rng.random(a.D)).astype(np.float32)
    for h in (a, b):
        h.norm_set_stats(om, ov, 1234, 0.25, 1.75, 777)
    before = a.norm_get_stats()
    a.collect_rollout(); b.collect_rollout()
    after = a.norm_get_stats()
    for k in before:
        np.testing.assert_array_equal(_bits(np.asarray(before[k])), _bits(np.asarray(after[k])), err_msg=k)
    assert after["obs_count"] == 1234 and after["ret_count"] == 777
    assert a.norm_rollout_info()["last_collection_path"] == 1
    _assert_rollout_equal(capi, a, b, f"frozen, kind {kind}")
    a.close(); b.close()


def test_launch_count_does_not_depend_on_n_steps(pkg):
    n = {}
    for steps in (8, 40):
        h = _mk(pkg, 1, 33, (1, 1), True, n_steps=steps)
        h.collect_rollout()
        info = h.norm_rollout_info()
        assert info["last_collection_path"] == 1 and info["enabled"] and info["available"] and info["max_envs"] == 128
        n[steps] = info["last_collection_launches"]
        h.close()
    assert n[8] == n[40] and 0 < n[8] < 8


def test_exact_f32_forward_collects_step_granular(pkg):
    """parameters with max |W2| >= 350 run the exact-f32 forward: the collection reports path 0, is counted, and equals the twin everywhere"""
    capi = pkg._capi
    kind, E = 1, 33
    probe = _mk(pkg, kind, E, (1, 1), False)
    big = _params(probe.P, 8, 0.4)
    sl = split_budget.w2_slices(probe.D, 64, probe.A, probe.discrete)
    big[sl[0].start + 5] = 400.0; big[sl[1].start + 70] = -380.0
    probe.close()
    a, b = _mk(pkg, kind, E, (1, 1), True, params=big), _mk(pkg, kind, E, (1, 1), False, params=big)
    assert a.f32_fallback_info()["forward_exact_f32"] == 1
    a.collect_rollout(); b.collect_rollout()
    info = a.norm_rollout_info()
    assert info["last_collection_path"] == 0 and info["total_stepwise_fallbacks"] == 1 and info["enabled"]
    for w in range(10):
        x, y = a.buffer(w).reshape(-1), b.buffer(w).reshape(-1)
        if w == capi.BUF_BOOTSTRAP:
            tr = (a.buffer(capi.BUF_FLAGS).reshape(-1) & 2).astype(bool); x, y = x[tr], y[tr]
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"buffer {w}")
    _assert_left_equal(a, b, "exact-f32 fallback")
    a.close(); b.close()


def test_matches_oracle(pkg, oracle_mod):
    """test_normalize_wrapper_rollout_matches_oracle (tests/test_gpu_parity.py) with the opt-in on: kind 1, E = 33 (a ragged second tile), its tolerances"""
    capi = pkg._capi
    kind, flags, E, T_, L_ = 1, (1, 1), 33, 30, 9
    cfg = _cfg(pkg, kind, n_envs=E, n_steps=T_, episode_len=L_, batch_size=E * T_ // 2, epochs=1, norm_training=1, norm_obs=flags[0], norm_reward=flags[1], clip_obs=5.0, clip_reward=2.0)
    h, o = pkg.Handle(cfg), oracle_mod.Oracle(cfg)
    h.norm_rollout_enable(True)
    flat = _params(h.P, 31, 0.4); h.set_params(flat); o.set_params(flat)
    h.env_reset(9); o.env_reset(9)
    rng = np.random.default_rng(2)
    for rollout in range(2):
        noise = rng.standard_normal((E * T_, h.A)).astype(np.float32)
        h.set_noise(noise); o.set_noise(noise)
        h.collect_rollout(); o.collect_rollout()
        assert h.norm_rollout_info()["last_collection_path"] == 1
        sh = h.norm_get_stats(); om, ov, oc, rm, rv, rc = o.norm_stats()
        assert (sh["obs_count"], sh["ret_count"]) == (oc, rc)
        assert oc == E * (T_ + 1) * (rollout + 1)
        np.testing.assert_allclose(sh["obs_mean"], om, rtol=2e-5, atol=2e-6); np.testing.assert_allclose(sh["obs_var"], ov, rtol=1e-4, atol=1e-6)
        assert sh["ret_mean"] == pytest.approx(rm, rel=1e-4, abs=1e-5) and sh["ret_var"] == pytest.approx(rv, rel=1e-4, abs=1e-5)
        for which, tol in ((capi.BUF_OBSERVATIONS, 1e-4), (capi.BUF_VALUES, 2e-4), (capi.BUF_LOGPROBS, 2e-4), (capi.BUF_REWARDS, 2e-4), (capi.BUF_ADVANTAGES, 2e-3), (capi.BUF_RETURNS, 2e-3)):
            np.testing.assert_allclose(h.buffer(which).reshape(T_, E, -1), o.buffer(which).reshape(T_, E, -1), atol=tol, rtol=tol)
        fh, fo = h.buffer(capi.BUF_FLAGS).reshape(T_, E), o.buffer(capi.BUF_FLAGS).reshape(T_, E)
        np.testing.assert_array_equal(fh, fo)
        tr = (fo & 2).astype(bool)
        assert tr.any()
        np.testing.assert_allclose(h.buffer(capi.BUF_BOOTSTRAP).reshape(T_, E)[tr], o.buffer(capi.BUF_BOOTSTRAP).reshape(T_, E)[tr], atol=2e-4, rtol=2e-4)
        assert np.abs(h.buffer(capi.BUF_OBSERVATIONS)).max() <= 5.0 + 1e-6 and np.abs(h.buffer(capi.BUF_REWARDS)).max() <= 2.0 + 1e-6
        st, sc = h.env_get_state(); o.env_set_state(st, sc)
    h.close()


def _refused(pkg, h, needle):
    with pytest.raises(pkg.DrilError) as ei:
        h.norm_rollout_enable(True)
    assert ei.value.code == pkg._capi.ERR_UNSUPPORTED and needle in str(ei.value), str(ei.value)
    info = h.norm_rollout_info()
    assert not info["enabled"] and not info["available"] and needle in info["reason"]


def _collects_as(capi, h, twin):
    h.collect_rollout(); twin.collect_rollout()
    for w in range(8):
        np.testing.assert_array_equal(_bits(h.buffer(w)), _bits(twin.buffer(w)), err_msg=f"buffer {w}")
    h.close(); twin.close()


def test_refusals(pkg, monkeypatch):
    """every row of the refusal list: DRIL_ERR_UNSUPPORTED with a message that says what to do, and the handle collects afterwards as a handle never asked"""
    capi = pkg._capi
    kw = dict(n_envs=8, n_steps=6, episode_len=4, batch_size=48, epochs=1)
    mk = lambda kind=1, **k: (lambda h: (h.set_params(_params(h.P, 8, 0.4)), h.env_reset(3), h)[2])(pkg.Handle(_cfg(pkg, kind, **{**kw, **k})))
    norm = dict(norm_obs=1, norm_reward=1, norm_training=1)
    # not a normalising built-in handle: a built-in without the wrapper, a plug-in, an external handle
    h = mk(); _refused(pkg, h, "no NormalizeWrapperEnv"); _collects_as(capi, h, mk())
    h = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, **kw), env_module=_co("pendulum")); _refused(pkg, h, "dril_normalize_enable"); h.close()
    c = _cfg(pkg, capi.ENV_EXTERNAL, **kw); c.ext_obs_dim, c.ext_action_dim, c.ext_discrete, c.ext_action_low, c.ext_action_high = 3, 1, 0, -1.0, 1.0
    h = pkg.Handle(c); _refused(pkg, h, "dril_ext_normalize_enable"); h.close()
    # a generic net, a wide net, hidden 32
    for hd, needle in ((128, "[64,64]"), (32, "[64,64]")):
        h = mk(**norm, hidden1=hd, hidden2=hd); _refused(pkg, h, needle); _collects_as(capi, h, mk(**norm, hidden1=hd, hidden2=hd))
    h = mk(**norm, hidden1=64, hidden2=48); _refused(pkg, h, "generic"); _collects_as(capi, h, mk(**norm, hidden1=64, hidden2=48))
    # n_envs > max_envs
    h = mk(**{**norm, "n_envs": 129, "batch_size": 129 * 6}); _refused(pkg, h, "n_envs = 129"); _collects_as(capi, h, mk(**{**norm, "n_envs": 129, "batch_size": 129 * 6}))
    # world_size > 1 (no communicator yet: nothing to collect with), and a ready communicator on one rank
    h = mk(**norm, world_size=2, rank=0); _refused(pkg, h, "data-parallel"); h.close()
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    h = mk(**norm); h.comm_init(h.comm_unique_id()); _refused(pkg, h, "data-parallel"); _collects_as(capi, h, mk(**norm))
    # DRIL_FORCE_STEPWISE / DRIL_FORCE_GENERIC (latched at create)
    monkeypatch.setenv("DRIL_FORCE_STEPWISE", "1")
    h = mk(**norm); monkeypatch.delenv("DRIL_FORCE_STEPWISE"); _refused(pkg, h, "DRIL_FORCE_STEPWISE"); _collects_as(capi, h, mk(**norm))
    monkeypatch.setenv("DRIL_FORCE_GENERIC", "1")
    h = mk(**norm); twin = mk(**norm); monkeypatch.delenv("DRIL_FORCE_GENERIC"); _refused(pkg, h, "DRIL_FORCE_GENERIC"); _collects_as(capi, h, twin)
    # and the handle all of this is for
    h = mk(**norm); h.norm_rollout_enable(True); assert h.norm_rollout_info()["enabled"]; h.norm_rollout_enable(False); assert not h.norm_rollout_info()["enabled"]; h.close()


def test_training(pkg):
    """three dril_train iterations of the README's shape (PPO() defaults: 4 envs x 2048 steps, minibatches of 64, 10 epochs) on normalised Pendulum with the opt-in,
    against the twin: statuses OK, statistics finite, n_updates as the twin's, parameters within the tolerances tests/test_gpu_parity.py grants two forms of one update
    (rtol 1e-4, atol 2e-6: test_small_minibatch_persistent_update, ppo_update_small_kernel against ppo_grad_kernel)"""
    capi = pkg._capi
    hs = []
    for optin in (True, False):
        cfg = _cfg(pkg, capi.ENV_PENDULUM, norm_obs=1, norm_reward=1, norm_training=1, monitor_window=100)
        h = pkg.Handle(cfg)
        layer = pkg.ActorCriticLayer(pkg.PendulumEnv().observation_space(), pkg.PendulumEnv().action_space())
        h.set_params(pkg.flatten_params(layer.initialparameters(np.random.default_rng(0))))
        h.env_reset(11)
        if optin:
            h.norm_rollout_enable(True)
        hs.append(h)
    a, b = hs
    sa, _ = a.train(3 * a.N)[:2]; sb, _ = b.train(3 * b.N)[:2]
    assert len(sa) == len(sb) == 3
    assert a.norm_rollout_info()["last_collection_path"] == 1 and a.norm_rollout_info()["total_stepwise_fallbacks"] == 0
    for x, y in zip(sa, sb):
        assert x.n_updates == y.n_updates == 10 * (a.N // 64) and not x.nan_or_inf
        assert all(np.isfinite(getattr(x, f)) for f in ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl_div", "grad_norm", "explained_variance"))
    pa, pb = a.get_params(), b.get_params()
    print(f"[norm rollout] three iterations: max |parameter difference| {np.abs(pa - pb).max():.3e}")
    np.testing.assert_allclose(pa, pb, rtol=1e-4, atol=2e-6)
    a.close(); b.close()
