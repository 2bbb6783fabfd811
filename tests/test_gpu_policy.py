"""GPU (-m gpu): deployment policies (include/dril_policy.h, policy_act_kernel) through the C ABI and the Python mirror.

Checkers: (1) tests/policy_ref.py, a float64 NumPy restatement; (2) the training handles' own predict_actions on hand-normalised observations; (3) the policy against
itself: batch invariance bit for bit, kernel path against the layer-contraction path, a copy that the handle's later life does not reach.
Every test builds a policy first, so without the feature every one of them fails there (missing symbol)."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import policy_ref as ref
from test_gpu_env_plugin import _cfg, _co, _params
from test_gpu_sac_env_plugin import make_module

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
F = np.float32
CAT, GAUSS, SQUASH = 0, 1, 2


def build(pkg, kind, dims, act="tanh", seed=0, norm=False, low=None, high=None, scale=1.0, action_start=1):
    """-> (policy, dict of what it was built from)"""
    rng = np.random.default_rng(seed)
    D, A = dims[0], dims[-1]
    layers = ref.random_actor(rng, dims, scale)
    ls = None if kind == CAT else (rng.standard_normal(A) * 0.3 - 0.5).astype(F)
    mean, var = ((rng.standard_normal(D) * 0.5).astype(F), (rng.random(D) + 0.25).astype(F)) if norm else (None, None)
    if kind != CAT and low is None:
        low, high = -np.ones(A, F), np.ones(A, F)
    desc = pkg.deployment.make_policy_desc(kind, D, A, dims[1:-1], act, action_start=action_start if kind == CAT else 0, action_low=low, action_high=high,
                                           clip_obs=2.5 if norm else None, epsilon=1e-6)
    p = pkg.NeuralPolicy.create(desc, ref.flat_actor(layers), ls, mean, var)
    return p, dict(layers=layers, ls=ls, mean=mean, var=var, low=low, high=high, act=act, kind=kind, D=D, A=A, start=action_start, norm=norm)


def expect(s, obs, deterministic, noise=None):
    """float64: -> (raw, env, margin or None)"""
    x = ref.normalize(obs, s["mean"], s["var"], 1e-6, 2.5) if s["norm"] else obs
    z = ref.mlp(s["layers"], x, s["act"])
    if s["kind"] == CAT:
        a, margin = ref.categorical(z, deterministic, noise, s["start"])
        return a, a, margin
    fn = ref.diag_gaussian if s["kind"] == GAUSS else ref.squashed
    raw, env = fn(z, s["ls"], deterministic, noise, s["low"], s["high"])
    return raw, env, None


def check_against_ref(p, s, B, seed=1):
    rng = np.random.default_rng(seed)
    obs = (rng.standard_normal((B, s["D"])) * 1.5).astype(F)
    for deterministic in (True, False):
        noise = None if deterministic else (rng.random(B) if s["kind"] == CAT else rng.standard_normal((B, s["A"])).astype(F))
        raw, env = p.act(obs, deterministic, noise, want_raw=True)
        eraw, eenv, margin = expect(s, obs.astype(np.float64), deterministic, None if noise is None else noise.astype(np.float64))
        if s["kind"] == CAT:
            ok = margin > (1e-4 if deterministic else 1e-5)                  # argmax / the CDF step compared only where float64 leaves no doubt
            assert ok.mean() > 0.9
            np.testing.assert_array_equal(env[ok], eenv[ok]); np.testing.assert_array_equal(raw, env)
            assert env.min() >= s["start"] and env.max() < s["start"] + s["A"]
        else:
            np.testing.assert_allclose(raw, eraw, atol=1e-5, rtol=1e-5); np.testing.assert_allclose(env, eenv, atol=1e-5, rtol=1e-5)


# ---- 1: against float64 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dims,act,kw", [
    (CAT, (4, 64, 64, 2), "tanh", {}),
    (GAUSS, (3, 256, 256, 2), "tanh", dict(low=np.array([-0.05, 0.0], F), high=np.array([0.1, 0.0], F), norm=True)),   # a clamp that bites; a dimension without one
    (SQUASH, (3, 512, 512, 1), "relu", dict(low=np.array([-2.0], F), high=np.array([2.0], F))),
    (GAUSS, (7, 1024, 3), "tanh", {}),
    (CAT, (1024, 48, 5), "tanh", dict(norm=True, action_start=0)),
    (GAUSS, (6, 40, 64), "relu", {}),
    (SQUASH, (12, 100, 36, 48, 20, 16), "swish", dict(norm=True)),
])
def test_kernel_equals_float64_reference(pkg, kind, dims, act, kw):
    p, s = build(pkg, kind, dims, act, **kw)
    for B in (1, 5, 64, 200):
        check_against_ref(p, s, B, seed=B)


@pytest.mark.parametrize("act", ref.ACTIVATIONS)
def test_four_layers_every_activation(pkg, act):
    p, s = build(pkg, GAUSS, (9, 100, 36, 48, 20, 4), act, seed=3, scale=1.5)
    check_against_ref(p, s, 37)
    q, t = build(pkg, CAT, (9, 100, 36, 48, 20, 6), act, seed=4, scale=2.0)
    check_against_ref(q, t, 70)


# ---- 2: batch invariance, the two paths -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dims,act", [(GAUSS, (5, 256, 256, 3), "tanh"), (SQUASH, (12, 1024, 300, 4), "gelu"), (GAUSS, (17, 70, 33, 2), "elu")])
def test_batch_invariance_bit_for_bit(pkg, kind, dims, act):
    p, s = build(pkg, kind, dims, act, seed=5, norm=True)
    rng = np.random.default_rng(9)
    obs = rng.standard_normal((256, dims[0])).astype(F)
    raw256, env256 = p.act(obs, True, want_raw=True)
    for j in (0, 3, 100, 255):
        r1, e1 = p.act(obs[j:j + 1], True, want_raw=True)
        assert r1.tobytes() == raw256[j:j + 1].tobytes() and e1.tobytes() == env256[j:j + 1].tobytes()
        others = rng.standard_normal((17, dims[0])).astype(F); others[11] = obs[j]
        r17, _ = p.act(others, True, want_raw=True)
        assert r17[11].tobytes() == raw256[j].tobytes()
    noise = rng.standard_normal((256, dims[-1])).astype(F)                   # sampled, injected draws: the same per row
    rs, _ = p.act(obs, False, noise, want_raw=True)
    r1, _ = p.act(obs[77:78], False, noise[77:78], want_raw=True)
    assert r1.tobytes() == rs[77:78].tobytes()


def test_over_threshold_path_agrees_with_the_kernel(pkg):
    for kind, dims, act in ((GAUSS, (6, 256, 256, 3), "tanh"), (CAT, (20, 100, 36, 5), "gelu"), (SQUASH, (3, 512, 512, 2), "relu")):
        p, s = build(pkg, kind, dims, act, seed=6, norm=True)
        rng = np.random.default_rng(2)
        obs = rng.standard_normal((700, dims[0])).astype(F)
        noise = rng.random(700) if kind == CAT else rng.standard_normal((700, dims[-1])).astype(F)
        big = p.act(obs, False, noise, want_raw=True)                        # 700 > 256: the layer contractions + head launch
        p.set_threshold(1 << 20)
        ker = p.act(obs, False, noise, want_raw=True)                        # the same batch through policy_act_kernel
        p.set_threshold(0)
        if kind == CAT:
            assert (big[1] == ker[1]).mean() > 0.995
        else:
            np.testing.assert_allclose(big[0], ker[0], atol=1e-5, rtol=1e-5); np.testing.assert_allclose(big[1], ker[1], atol=1e-5, rtol=1e-5)
        check = expect(s, obs[:300].astype(np.float64), False, noise[:300].astype(np.float64))
        if kind != CAT:
            np.testing.assert_allclose(big[1][:300], check[1], atol=1e-5, rtol=1e-5)


# ---- 3: against the training handles ---------------------------------------------------------------------------------------------------------------------------------
def _hand_norm(obs, st, eps, clip):
    return np.clip((obs - st["obs_mean"]) / np.sqrt(st["obs_var"] + F(eps)), -clip, clip).astype(F)


def test_from_handle_cartpole_and_pendulum(pkg):
    cap = pkg._capi
    h = pkg.Handle(_cfg(pkg, cap.ENV_CARTPOLE, n_envs=8, n_steps=4, batch_size=32))
    h.set_params(_params(h.P, 1, 0.5))
    p = pkg.NeuralPolicy.from_handle(h)
    obs = np.random.default_rng(0).standard_normal((64, 4)).astype(F)
    assert (p.kind, p.D, p.A, p.hidden_dims, p.desc.action_start) == (CAT, 4, 2, (64, 64), 1)
    flat, ls = p.get_params()
    assert ls is None and np.array_equal(flat, h.get_params()[:flat.size])
    mism = p.act(obs, True) != h.predict_actions(obs, deterministic=True)
    assert mism.mean() < 0.02                                               # (the handle's second layer runs on f16 pieces: ties may fall the other way)
    u = np.random.default_rng(1).random(64)
    assert (p.act(obs, False, u) != h.predict_actions(obs, noise=u)).mean() < 0.02
    with pytest.raises(pkg.DrilError) as e:
        pkg.NeuralPolicy.from_handle(h, with_norm=True)
    assert e.value.code == cap.ERR_NOT_INITIALISED and "NormalizeWrapperEnv" in str(e.value)
    # Pendulum under cfg.norm_obs: statistics that have moved
    g = pkg.Handle(_cfg(pkg, cap.ENV_PENDULUM, n_envs=16, n_steps=8, batch_size=128, norm_obs=1, norm_reward=1, norm_training=1, clip_obs=3.0, norm_epsilon=1e-6))
    g.set_params(_params(g.P, 2, 0.4)); g.env_reset(3); g.collect_rollout()
    st = g.norm_get_stats()
    q = pkg.NeuralPolicy.from_handle(g, with_norm=True)
    assert isinstance(q, pkg.NormWrapperPolicy) and q.clip_obs == 3.0 and q.eps == pytest.approx(1e-6) and q.kind == GAUSS
    mean, var = q.get_norm()
    assert np.array_equal(mean, st["obs_mean"]) and np.array_equal(var, st["obs_var"]) and st["obs_count"] > 0
    raw_obs = (np.random.default_rng(4).standard_normal((50, 3)) * np.array([1, 1, 4])).astype(F)
    z = np.random.default_rng(5).standard_normal((50, 1)).astype(F)
    for det, nz in ((True, None), (False, z)):
        want = g.predict_actions(_hand_norm(raw_obs, st, 1e-6, 3.0), deterministic=det, noise=nz)
        raw, env = q.act(raw_obs, det, nz, want_raw=True)
        np.testing.assert_allclose(raw, want, atol=1e-4, rtol=1e-4); np.testing.assert_allclose(env, np.clip(want, -2.0, 2.0), atol=1e-4, rtol=1e-4)


def test_from_handle_plugin_with_normalize_enable(pkg):
    h = pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, n_envs=32, n_steps=8, batch_size=256, episode_len=20, n_hidden=3, hidden=(C.c_int32 * 4)(48, 100, 24, 0), activation=6),
                   env_module=_co("reacher3"))
    h.normalize_enable(clip_obs=1.5, epsilon=1e-5)
    h.set_params(_params(h.P, 3, 0.3)); h.env_reset(1); h.collect_rollout()
    st = h.normalize_get_stats()
    p = pkg.NeuralPolicy.from_handle(h, with_norm=True)
    assert (p.D, p.A, p.hidden_dims, p.activation, p.clip_obs) == (12, 3, (48, 100, 24), "gelu", 1.5)
    assert p.action_space.low == (-1.0,) * 3 and p.action_space.high == (1.0,) * 3
    obs = (np.random.default_rng(6).standard_normal((40, 12)) * 2).astype(F)
    z = np.random.default_rng(7).standard_normal((40, 3)).astype(F)
    want = h.predict_actions(_hand_norm(obs, st, 1e-5, 1.5), noise=z)
    raw, env = p.act(obs, False, z, want_raw=True)
    np.testing.assert_allclose(raw, want, atol=1e-4, rtol=1e-4); np.testing.assert_allclose(env, np.clip(want, -1, 1), atol=1e-4, rtol=1e-4)
    plain = pkg.NeuralPolicy.from_handle(h)                                  # extract_policy(agent): the same actor, observations as they are
    np.testing.assert_allclose(plain.act(_hand_norm(obs, st, 1e-5, 1.5), True), p.act(obs, True), atol=1e-6)


def test_from_sac_handles(pkg):
    from test_gpu_sac_normalize import make
    h, layer = make(pkg, "pendulum", 16, 50, hidden=(64, 64))
    h.set_params(_params(h.P, 8, 0.3))
    p = pkg.NeuralPolicy.from_handle(h)
    assert (p.kind, p.D, p.A, p.hidden_dims, p.activation) == (SQUASH, 3, 1, (64, 64), "relu") and p.action_space.high == (2.0,)
    obs = np.random.default_rng(0).standard_normal((33, 3)).astype(F)
    z = np.random.default_rng(1).standard_normal((33, 1)).astype(F)
    for det, nz in ((True, None), (False, z)):
        wraw, wenv = h.predict_actions(obs, deterministic=det, noise=nz)
        raw, env = p.act(obs, det, nz, want_raw=True)
        np.testing.assert_allclose(raw, wraw, atol=1e-4, rtol=1e-4); np.testing.assert_allclose(env, wenv, atol=1e-4, rtol=1e-4)
    with pytest.raises(pkg.DrilError) as e:
        pkg.NeuralPolicy.from_handle(h, with_norm=True)
    assert e.value.code == pkg._capi.ERR_NOT_INITIALISED
    # a plug-in handle with its wrapper
    m, _, _ = make_module(pkg, _co("reacher3"), 24, hidden=(40, 56), act="tanh", max_steps=15)
    m.normalize_enable(clip_obs=2.0, epsilon=1e-6)
    m.set_params(_params(m.P, 9, 0.3)); m.env_reset(2); m.collect_rollout(6, True)
    st = m.norm_get_stats()
    q = pkg.NeuralPolicy.from_handle(m, with_norm=True)
    assert (q.D, q.A, q.hidden_dims, q.activation, q.clip_obs) == (12, 3, (40, 56), "tanh", 2.0) and st["obs_count"] > 0
    obs = (np.random.default_rng(3).standard_normal((29, 12)) * 2).astype(F)
    z = np.random.default_rng(4).standard_normal((29, 3)).astype(F)
    wraw, wenv = m.predict_actions(_hand_norm(obs, st, 1e-6, 2.0), noise=z)
    raw, env = q.act(obs, False, z, want_raw=True)
    np.testing.assert_allclose(raw, wraw, atol=1e-4, rtol=1e-4); np.testing.assert_allclose(env, wenv, atol=1e-4, rtol=1e-4)


# ---- 4: a copy, without side effects ----------------------------------------------------------------------------------------------------------------------------------
def test_policy_is_a_copy_of_a_ppo_handle(pkg):
    cap = pkg._capi
    def fresh():
        h = pkg.Handle(_cfg(pkg, cap.ENV_PENDULUM, n_envs=16, n_steps=16, batch_size=64, epochs=2, norm_obs=1, norm_reward=1, norm_training=1, hidden1=32, hidden2=32))
        h.set_params(_params(h.P, 11, 0.3)); h.env_reset(5); h.collect_rollout()
        return h
    a, b = fresh(), fresh()
    obs = np.random.default_rng(0).standard_normal((20, 3)).astype(F)
    p = pkg.NeuralPolicy.from_handle(a, with_norm=True)
    for i in range(100):
        p.act(obs, i % 2 == 0)
    # the handle with an extraction and 100 policy calls behind it is the handle without, bit for bit — now and in what it does next
    assert a.get_params().tobytes() == b.get_params().tobytes() and all(np.array_equal(x, y) for x, y in zip(a.norm_get_stats().values(), b.norm_get_stats().values()))
    a.collect_rollout(); b.collect_rollout()
    for which in (cap.BUF_OBSERVATIONS, cap.BUF_ACTIONS, cap.BUF_REWARDS, cap.BUF_LOGPROBS, cap.BUF_VALUES):
        assert a.buffer(which).tobytes() == b.buffer(which).tobytes()
    before, h_before = p.act(obs, True), a.predict_actions(obs, deterministic=True)
    a.ppo_update()
    assert not np.array_equal(a.predict_actions(obs, deterministic=True), h_before)       # training moved the handle ...
    assert p.act(obs, True).tobytes() == before.tobytes()                                  # ... and not the policy
    a.close(); b.close()
    assert p.act(obs, True).tobytes() == before.tobytes()                                  # the policy outlives the handle


def test_policy_is_a_copy_of_a_sac_handle(pkg):
    from test_gpu_sac_normalize import make
    def fresh():
        h, _ = make(pkg, "pendulum", 8, 30, hidden=(32, 32), B=16)
        h.normalize_enable()
        h.set_params(_params(h.P, 12, 0.3)); h.env_reset(4); h.collect_rollout(8, True)
        return h
    a, b = fresh(), fresh()
    obs = np.random.default_rng(0).standard_normal((10, 3)).astype(F)
    p = pkg.NeuralPolicy.from_handle(a, with_norm=True)
    for _ in range(100):
        p.act(obs, False)
    assert a.get_params().tobytes() == b.get_params().tobytes() and a.replay_size() == b.replay_size() == 64
    a.collect_rollout(4, False); b.collect_rollout(4, False)
    for which in (pkg._capi.RB_OBSERVATIONS, pkg._capi.RB_ACTIONS, pkg._capi.RB_REWARDS):
        assert a.replay(which).tobytes() == b.replay(which).tobytes()
    before, h_before = p.act(obs, True), a.predict_actions(obs, deterministic=True)[1]
    a.update(3)
    assert not np.array_equal(a.predict_actions(obs, deterministic=True)[1], h_before)
    assert p.act(obs, True).tobytes() == before.tobytes()
    a.close(); b.close()
    assert p.act(obs, True).tobytes() == before.tobytes()


# ---- 5: sampling ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_own_noise_stream(pkg):
    p, s = build(pkg, GAUSS, (4, 32, 2), seed=7)
    obs = np.zeros((6, 4), F)
    p.set_seed(123); a1, a2 = p.act(obs, False), p.act(obs, False)
    p.set_seed(123); b1, b2 = p.act(obs, False), p.act(obs, False)
    assert a1.tobytes() == b1.tobytes() and a2.tobytes() == b2.tobytes()       # same seed, same sequence of calls
    assert not np.array_equal(a1, a2) and len(np.unique(a1[:, 0])) == 6         # another call, another row: another draw
    p.set_seed(124); assert not np.array_equal(p.act(obs, False), a1)
    mu = ref.mlp(s["layers"], obs[:1], "tanh")[0]
    p.set_seed(5)
    z = (np.concatenate([p.act(np.zeros((4000, 4), F), False, want_raw=True)[0] for _ in range(5)]) - mu) / np.exp(s["ls"])   # 20 000 standard normals per dimension
    assert abs(z.mean()) < 0.03 and abs(z.std() - 1) < 0.03 and abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 0.03


def test_sampled_categorical_matches_softmax(pkg):
    p, s = build(pkg, CAT, (4, 64, 64, 5), seed=8, scale=3.0, action_start=0)
    x = np.random.default_rng(1).standard_normal((1, 4)).astype(F)
    probs = ref.softmax(ref.mlp(s["layers"], x, "tanh"))[0]
    p.set_seed(77)
    n = 20000
    draws = np.concatenate([p.act(np.repeat(x, 200, axis=0), False) for _ in range(n // 200)])     # kernel path: 100 calls of 200 rows
    freq = np.bincount(draws, minlength=5) / n
    assert (np.abs(freq - probs) <= 3 * np.sqrt(probs * (1 - probs) / n) + 1e-4).all(), (freq, probs)


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_carry_a_status_and_a_message(pkg):
    lib, cap = pkg._capi.load_library(), pkg._capi
    p, s = build(pkg, GAUSS, (4, 16, 2))
    obs, out = np.zeros((2, 4), F), np.zeros((2, 2), F)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for args, word in (((None, 2, 1, None, None, ptr(out)), b"null obs"), ((ptr(obs), 0, 1, None, None, ptr(out)), b"batch"), ((ptr(obs), 2, 1, None, None, None), b"null")):
        assert lib.dril_policy_act(p._p, *args) == cap.ERR_INVALID_ARG and word in lib.dril_policy_last_error(p._p)
    flat = np.zeros(3, F)
    assert lib.dril_policy_get_params(p._p, ptr(flat), 3, None) == cap.ERR_INVALID_ARG
    assert lib.dril_policy_get_norm(p._p, ptr(flat), ptr(flat)) == cap.ERR_NOT_INITIALISED
    mk = pkg.deployment.make_policy_desc
    for desc, n in ((mk(1, 4, 2, (8,) * 5, "tanh"), 58), (mk(1, 4, 2, (1025,), "tanh"), 58), (mk(1, 4, 2, (8,), "tanh"), 57)):
        q = C.c_void_p()
        assert lib.dril_policy_create(C.byref(desc), ptr(np.zeros(64, F)), n, ptr(np.zeros(2, F)), None, None, C.byref(q)) == cap.ERR_INVALID_ARG
        assert lib.dril_policy_last_error(None) and not q.value
    assert np.isfinite(p.act(obs, True)).all()                                # the policy is still usable after its refusals


# ---- 7: the Python mirror, the file, the example --------------------------------------------------------------------------------------------------------------------
def test_extract_policy_save_and_load(pkg, tmp_path):
    env = pkg.PendulumEnv()
    layer = pkg.ActorCriticLayer(env.observation_space(), env.action_space(), hidden_dims=(48, 24), activation="elu", log_std_init=-0.7)
    agent = pkg.Agent(layer, pkg.PPO(n_steps=8, batch_size=32, epochs=1), seed=3)
    agent.train_state.parameters["actor_head"]["layer_3"]["weight"] *= 50.0
    p = pkg.extract_policy(agent)
    assert type(p) is pkg.NeuralPolicy and p.hidden_dims == (48, 24) and p.activation == "elu" and p.action_space.low == (-2.0,)
    layers = [(agent.train_state.parameters["actor_head"][f"layer_{l}"]["weight"], agent.train_state.parameters["actor_head"][f"layer_{l}"]["bias"]) for l in (1, 2, 3)]
    obs = np.random.default_rng(0).standard_normal((9, 3)).astype(F)
    want = np.clip(ref.mlp(layers, obs, "elu"), -2, 2)
    one = p(obs[0])
    assert one.shape == (1,) and np.allclose(one, want[0], atol=1e-5)
    many = p(list(obs))
    assert isinstance(many, list) and len(many) == 9 and np.allclose(np.stack(many), want, atol=1e-5)
    g1, g2 = p(obs[0], deterministic=False, rng=np.random.default_rng(4)), p(obs[0], deterministic=False, rng=np.random.default_rng(4))
    assert np.array_equal(g1, g2) and not np.allclose(g1, one)
    venv = pkg.NormalizeWrapperEnv(pkg.DeviceParallelEnv(env, 8, seed=1), clip_obs=4.0)
    pkg.train_(agent, venv, agent.alg, 64)
    q = pkg.extract_policy(agent, venv)
    assert type(q) is pkg.NormWrapperPolicy and q.clip_obs == 4.0 and venv.handle.norm_get_stats()["obs_count"] > 0
    assert np.array_equal(q.get_norm()[0], venv.handle.norm_get_stats()["obs_mean"])
    path = pkg.save_policy(q, tmp_path / "deploy")
    r = pkg.load_policy(path)
    assert type(r) is pkg.NormWrapperPolicy and bytes(r.desc) == bytes(q.desc)
    big = np.random.default_rng(1).standard_normal((300, 3)).astype(F)
    for o in (obs, big):
        assert r.act(o, True).tobytes() == q.act(o, True).tobytes()
    z = np.random.default_rng(2).standard_normal((9, 1)).astype(F)
    assert r.act(obs, False, z).tobytes() == q.act(obs, False, z).tobytes()


def test_example_runs_to_the_end():
    r = subprocess.run([sys.executable, str(ROOT / "examples" / "deploy_policy.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "episode return" in r.stdout
