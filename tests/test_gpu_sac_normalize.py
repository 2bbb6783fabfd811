"""GPU (-m gpu): NormalizeWrapperEnv on the SAC handle (dril_sac_normalize_*), every check through the C ABI / SacHandle.

  * random-action streams: the ring of a wrapped handle equals the NumPy wrapper (tests/sac_normalize_ref.py) applied to the raw ring of a twin handle without the
    wrapper, in the reference's update order — built-in kinds, reacher3 (D = 12) and a plug-in compiled here with 133 observation dims; the three switch settings;
  * policy-driven one-step collections: the row just pushed and the statistics from get_original + the NumPy wrapper, the stored action from predict_actions;
  * frozen statistics, the set / get round trip, env_reset; evaluate_agent without side effects; iterate = collect + update; sac_train_ paths and checkpoints;
  * off means off, and the refusals."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sac_normalize_ref as ref
from test_gpu_sac_env_plugin import GENCO, _co, assert_rings_equal, init_params, make_module, ring

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = Path(__file__).resolve().parents[1]

_WIDE = '''#include "device/dril_env_plugin.h"
struct Wide {
    static constexpr int S = 2, D = WIDE_D, A = 2;
    static constexpr bool discrete = false;
    static constexpr int episode_len = 9;
    static constexpr float action_low[A] = {-1.0f, -2.0f}, action_high[A] = {1.0f, 0.5f};
    static constexpr const char* name = "Wide133";
    DRIL_ENV_FN static void reset(const DrilEnvRng& rng, float* st) {
        const DrilEnvWords r = rng.words(0);
        st[0] = DrilEnvRng::u01(r.w[0]) * 2.0f - 1.0f; st[1] = DrilEnvRng::u01(r.w[1]) * 4.0f - 2.0f;
    }
    DRIL_ENV_FN static void observe(const float* st, float* obs) {
        for (int i = 0; i < D; ++i) obs[i] = (float)(1 + i % 7) * (float)(1 + i % 7) * st[i & 1] + (float)(i % 11) * 3.0f - 0.01f * (float)i * st[0] * st[1];
    }
    DRIL_ENV_FN static float step(float* st, const float* act_f, int act_i, bool* terminated) {
        st[0] = 0.9f * st[0] + 0.3f * act_f[0]; st[1] = 0.8f * st[1] - 0.5f * act_f[1] + 0.1f * st[0];
        *terminated = st[1] > 2.5f;
        return 5.0f - st[0] * st[0] - 3.0f * st[1];
    }
};
DRIL_ENV_PLUGIN(Wide)
'''


@pytest.fixture(scope="module")
def wide_co(tmp_path_factory):
    """{D: code object}: 133 dims (more than two waves' worth of columns and a ragged tail), 300 dims (a second column tile of the moments kernel, 602 table columns)"""
    d = tmp_path_factory.mktemp("wide")
    (d / "wide.hip").write_text(_WIDE)
    out = {}
    for D in (133, 300):
        out[D] = d / f"wide{D}.hsaco"
        subprocess.run([*GENCO, f"-DWIDE_D={D}", str(d / "wide.hip"), "-o", str(out[D])], check=True)
    return out


def make(pkg, name, E, T_lim, wide_co=None, hidden=(32, 32), B=16, cap=1 << 14, seed=7, **alg_kw):
    """-> (handle, layer) over a built-in kind or a plug-in"""
    if name in ("reacher3", "wide", "wide300"):
        h, layer, _ = make_module(pkg, _co("reacher3") if name == "reacher3" else wide_co[300 if name == "wide300" else 133], E, hidden=hidden, B=B, cap=cap, seed=seed, max_steps=T_lim, **alg_kw)
        return h, layer
    env = {"pendulum": lambda: pkg.PendulumEnv(max_steps=T_lim), "mountaincar": lambda: pkg.MountainCarContinuousEnv(max_steps=T_lim),
           "pendulum_scaled": lambda: pkg.ScalingWrapperEnv(pkg.PendulumEnv(max_steps=T_lim))}[name]()
    alg = pkg.SAC(batch_size=B, buffer_capacity=cap, **alg_kw)
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=hidden)
    return pkg.SacHandle(pkg.make_sac_config(env, E, alg, layer, seed=seed)), layer


def tm(r, E):
    """ring fields time-major: (steps, E, ...)"""
    return {k: v.reshape(-1, E, *v.shape[1:]) for k, v in r.items()}


def assert_stats(st, w, rtol=2e-5):
    assert st["obs_count"] == w.obs_count and st["ret_count"] == w.ret_count
    scale = np.sqrt(w.obs_var) + np.abs(w.obs_mean) + 1e-6
    assert np.all(np.abs(st["obs_mean"] - w.obs_mean) <= rtol * scale), np.abs(st["obs_mean"] - w.obs_mean).max()
    assert np.allclose(st["obs_var"], w.obs_var, rtol=20 * rtol, atol=1e-7)
    assert np.isclose(st["ret_mean"], w.ret_mean, rtol=20 * rtol, atol=1e-5) and np.isclose(st["ret_var"], w.ret_var, rtol=20 * rtol, atol=1e-7)


# ---- 1: random-action stream -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,E", [("pendulum", 50), ("mountaincar", 33), ("pendulum_scaled", 64), ("reacher3", 37), ("wide", 70), ("wide300", 530), ("pendulum", 1100)])
@pytest.mark.parametrize("norm_obs,norm_reward", [(1, 1), (1, 0), (0, 1)])
def test_random_action_stream_equals_the_numpy_wrapper_over_the_raw_ring(pkg, wide_co, name, E, norm_obs, norm_reward):
    T, k, T_lim = 7, 2, 5
    kw = dict(norm_obs=norm_obs, norm_reward=norm_reward, clip_obs=1.25, clip_reward=0.75, gamma=0.9, epsilon=1e-6)
    a, _ = make(pkg, name, E, T_lim, wide_co)
    b, _ = make(pkg, name, E, T_lim, wide_co)
    b.normalize_enable(**kw)
    for h in (a, b):
        h.env_reset(11)
        for _ in range(k):
            h.collect_rollout(T, True)
    ra, rb = tm(ring(pkg, a), E), tm(ring(pkg, b), E)
    assert ra["trunc"].any() and not ra["trunc"].all()
    for f in ("act", "term", "trunc"):
        assert np.array_equal(ra[f], rb[f]), f
    w = ref.Wrapper(E, a.D, **kw)
    exp = ref.replay_through(w, ra, a.env_observe(), T, k)
    assert np.allclose(rb["obs"], exp["obs"], rtol=3e-5, atol=3e-5), np.abs(rb["obs"] - exp["obs"]).max()
    assert np.allclose(rb["next"], exp["next"], rtol=3e-5, atol=3e-5), np.abs(rb["next"] - exp["next"]).max()
    assert np.allclose(rb["rew"], exp["rew"], rtol=3e-5, atol=3e-5), np.abs(rb["rew"] - exp["rew"]).max()
    st = b.norm_get_stats()
    assert st["obs_count"] == (E * (T + 1) * k if norm_obs else 0) and st["ret_count"] == (E * T * k if norm_reward else 0)
    assert_stats(st, w)
    if norm_obs:                                                       # the clips are hit and held
        assert np.abs(rb["obs"]).max() == F(1.25) and np.abs(rb["next"]).max() <= F(1.25)
    else:
        assert np.array_equal(rb["obs"], ra["obs"]) and np.array_equal(rb["next"], ra["next"])
    if norm_reward:
        assert np.abs(rb["rew"]).max() == F(0.75)
    else:
        assert np.array_equal(rb["rew"], ra["rew"])
    obs, rew = b.norm_get_original()
    assert np.array_equal(obs, a.env_observe()) and np.array_equal(rew, ra["rew"][-1])
    assert np.allclose(b.norm_get_returns(), w.returns, rtol=3e-5, atol=3e-5)
    assert np.allclose(b.env_observe(), w.normalize_obs(obs), rtol=3e-5, atol=3e-5)      # a peek: nothing moved
    st2 = b.norm_get_stats()
    assert all(np.array_equal(st[q], st2[q]) for q in st)
    c, _ = make(pkg, name, E, T_lim, wide_co)                          # two runs, the same bits
    c.normalize_enable(**kw); c.env_reset(11)
    for _ in range(k):
        c.collect_rollout(T, True)
    assert_rings_equal(ring(pkg, b), ring(pkg, c))
    stc = c.norm_get_stats()
    assert all(np.array_equal(st[q], stc[q]) for q in st)


# ---- 2: policy-driven steps -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,E", [("pendulum", 19), ("reacher3", 21)])
def test_policy_steps_reproduce_from_the_originals(pkg, name, E):
    h, layer = make(pkg, name, E, 4)
    h.set_params(init_params(pkg, layer))
    kw = dict(clip_obs=2.0, clip_reward=1.5, gamma=0.95)
    h.normalize_enable(**kw); h.env_reset(3)
    w = ref.Wrapper(E, h.D, **kw)
    raw_prev = h.norm_get_original()[0]
    rng = np.random.default_rng(5)
    for step in range(9):
        noise = rng.normal(0, 1, (E, h.A)).astype(F)
        h.set_collect_noise(noise)
        h.collect_rollout(1, False)
        r = {q: v[-E:] for q, v in ring(pkg, h).items()}
        cur = w.observe(raw_prev)                                      # the observe the collection begins with: the second update over these observations
        assert np.allclose(r["obs"], cur, rtol=3e-5, atol=3e-5)
        raw_act, _ = h.predict_actions(r["obs"], deterministic=False, noise=noise)
        assert np.allclose(r["act"], raw_act, rtol=1e-4, atol=1e-5)
        raw_next, raw_rew = h.norm_get_original()
        rn, _ = w.act(raw_rew, r["term"], r["trunc"], raw_next)
        nxt = w.observe(raw_next)
        assert np.allclose(r["rew"], rn, rtol=3e-5, atol=3e-5)
        keep = ~r["trunc"].astype(bool)
        assert np.allclose(r["next"][keep], nxt[keep], rtol=3e-5, atol=3e-5)
        assert np.abs(r["next"]).max() <= F(2.0)
        assert_stats(h.norm_get_stats(), w)
        raw_prev = raw_next
    assert h.norm_get_stats()["obs_count"] == 2 * 9 * E


# ---- 3: frozen statistics, round trip, reset -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pendulum", "reacher3"])
def test_set_get_round_trip_frozen_collection_and_reset(pkg, name):
    E, T = 23, 6
    h, _ = make(pkg, name, E, 4)
    kw = dict(clip_obs=0.8, clip_reward=0.6)
    h.normalize_enable(**kw); h.env_reset(2)
    h.collect_rollout(T, True)
    assert h.norm_get_returns().any()
    rng = np.random.default_rng(0)
    new = dict(obs_mean=rng.normal(0, 1, h.D).astype(F), obs_var=rng.uniform(0.5, 2, h.D).astype(F), obs_count=12345, ret_mean=0.25, ret_var=1.75, ret_count=777)
    h.norm_set_stats(**new)
    st = h.norm_get_stats()
    assert all(np.array_equal(np.asarray(st[q]), np.asarray(new[q])) for q in new)
    h.normalize_set_training(False)
    n0 = h.replay_size(); ret0 = h.norm_get_returns()
    h.collect_rollout(T, True)
    st2 = h.norm_get_stats()
    assert all(np.array_equal(np.asarray(st2[q]), np.asarray(new[q])) for q in new)
    r = {q: v[n0:] for q, v in ring(pkg, h).items()}
    w = ref.Wrapper(E, h.D, training=False, **kw); w.set_stats(new)
    assert np.abs(r["obs"]).max() == F(0.8) and np.abs(r["rew"]).max() <= F(0.6)
    obs, rew = h.norm_get_original()
    assert np.allclose(r["next"][-E:][~r["trunc"][-E:].astype(bool)], w.normalize_obs(obs)[~r["trunc"][-E:].astype(bool)], rtol=3e-5, atol=3e-5)
    assert np.allclose(r["rew"][-E:], w.act(rew, r["term"][-E:], r["trunc"][-E:], obs)[0], rtol=3e-5, atol=3e-5)
    alive = ~(r["term"] | r["trunc"]).reshape(T, E).any(0).astype(bool)
    assert np.array_equal(h.norm_get_returns()[alive], ret0[alive])   # frozen: the recursion stands still (finished envs still go to zero)
    h.env_reset(2)
    assert not h.norm_get_returns().any()
    st3 = h.norm_get_stats()
    assert all(np.array_equal(np.asarray(st3[q]), np.asarray(new[q])) for q in new)


# ---- 4: evaluation ---------------------------------------------------------------------------------------------------------------------------------------------------
def _snapshot(pkg, h):
    st = h.norm_get_stats()
    return dict(ring=ring(pkg, h), st=st, ret=h.norm_get_returns(), orig=h.norm_get_original(), obs=h.env_observe())


def _same(a, b):
    assert_rings_equal(a["ring"], b["ring"])
    assert all(np.array_equal(np.asarray(a["st"][q]), np.asarray(b["st"][q])) for q in a["st"])
    assert np.array_equal(a["ret"], b["ret"]) and np.array_equal(a["orig"][0], b["orig"][0]) and np.array_equal(a["orig"][1], b["orig"][1]) and np.array_equal(a["obs"], b["obs"])


@pytest.mark.parametrize("name", ["pendulum", "reacher3"])
def test_evaluation_leaves_the_wrapper_alone_and_uses_the_frozen_statistics(pkg, monkeypatch, name):
    E, T_lim = 12, 20
    hs = []
    for _ in range(2):
        h, layer = make(pkg, name, E, T_lim)
        h.set_params(init_params(pkg, layer)); h.normalize_enable(clip_obs=5.0); h.env_reset(4)
        h.collect_rollout(3, True); h.collect_rollout(5, False)
        hs.append(h)
    a, b = hs
    stats, er, el = a.evaluate_agent(15, True, seed=99)
    _same(_snapshot(pkg, a), _snapshot(pkg, b))
    with pytest.raises(pkg.DrilError):
        a.evaluate_agent(0, True)
    _same(_snapshot(pkg, a), _snapshot(pkg, b))
    for h in (a, b):
        h.collect_rollout(4, False)
    _same(_snapshot(pkg, a), _snapshot(pkg, b))
    monkeypatch.setenv("DRIL_SAC_EVAL_POLL", "1")
    try:
        p, layer = make(pkg, name, E, T_lim)
    finally:
        monkeypatch.delenv("DRIL_SAC_EVAL_POLL")
    st = b.norm_get_stats()
    flat = init_params(pkg, layer)
    p.set_params(flat); p.normalize_enable(clip_obs=5.0, training=False)
    p.norm_set_stats(**st)
    b.normalize_set_training(False)
    s_b, er_b, el_b = b.evaluate_agent(15, True, seed=99)
    s_p, er_p, el_p = p.evaluate_agent(15, True, seed=99)
    assert np.array_equal(er_b, er_p) and np.array_equal(el_b, el_p) and s_b == s_p
    # the same statistics folded into the first layer of a handle WITHOUT the wrapper: W1' = W1 / sqrt(var + eps), b1' = b1 - W1' mean (clip_obs far away)
    q, layer = make(pkg, name, E, T_lim)
    ps = pkg.sac_unflatten_params(flat, layer.initialparameters(np.random.default_rng(0)))
    big, _ = make(pkg, name, E, T_lim)
    big.set_params(flat); big.normalize_enable(clip_obs=1e9, training=False); big.norm_set_stats(**st)
    l1 = ps["actor_head"]["layer_1"]
    sd = np.sqrt(st["obs_var"].astype(np.float64) + 1e-8)
    w1 = l1["weight"].astype(np.float64) / sd[None, :]
    l1["bias"] = (l1["bias"].astype(np.float64).reshape(-1) - w1 @ st["obs_mean"].astype(np.float64)).astype(F).reshape(l1["bias"].shape)
    l1["weight"] = w1.astype(F)
    q.set_params(pkg.sac_flatten_params(ps))
    s_q, er_q, el_q = q.evaluate_agent(15, True, seed=99)
    s_big, er_big, el_big = big.evaluate_agent(15, True, seed=99)
    assert np.array_equal(el_q, el_big)
    assert np.allclose(er_q, er_big, rtol=2e-2, atol=2e-2), (er_q, er_big)


# ---- 5: train paths --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pendulum", "reacher3"])
def test_iterate_equals_collect_plus_update_with_the_wrapper_on(pkg, name):
    E, k = 16, 5
    hs = []
    for _ in range(2):
        h, layer = make(pkg, name, E, 6, train_freq=2, gradient_steps=1)
        h.set_params(init_params(pkg, layer)); h.normalize_enable(); h.env_reset(8)
        h.collect_rollout(2, True)
        hs.append(h)
    a, b = hs
    a.iterate(k)
    for _ in range(k):
        b.collect_rollout(2, False); b.update(1)
    assert np.array_equal(a.get_params(), b.get_params())
    _same(_snapshot(pkg, a), _snapshot(pkg, b))
    assert a.norm_get_stats()["obs_count"] == E * 3 * (k + 1)


def test_sac_train_over_wrapped_envs_and_checkpoint_round_trip(pkg, tmp_path):
    E = 8
    env = pkg.NormalizeWrapperEnv(pkg.MonitorWrapperEnv(pkg.DeviceParallelEnv(pkg.PendulumEnv(max_steps=20), E)), clip_obs=5.0)
    alg = pkg.SAC(batch_size=16, buffer_capacity=4096, start_steps=64)
    agent = pkg.SACAgent(pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(32, 32)), alg, seed=1)
    agent, rb, ts, _ = pkg.sac_train_(agent, env, alg, E * 60)
    st = rb.handle.norm_get_stats()
    assert st["obs_count"] > 0 and st["ret_count"] > 0 and np.isfinite(ts["critic_losses"]).all() and np.isfinite(ts["actor_losses"]).all()
    rew_mean, len_mean, n = rb.handle.monitor_stats()
    assert n > 0 and len_mean == 20 and rew_mean < -20                 # raw Pendulum returns, not the normalised (clipped) ones
    assert np.abs(rb.handle.replay(pkg._capi.RB_OBSERVATIONS)).max() <= 5.0
    fp = pkg.checkpoint.save_normalization_stats(rb.handle, tmp_path / "norm", clip_obs=5.0)
    fresh, _ = make(pkg, "pendulum", E, 20)
    fresh.normalize_enable(clip_obs=5.0)
    pkg.checkpoint.load_normalization_stats_(fresh, fp)
    st2 = fresh.norm_get_stats()
    assert all(np.array_equal(np.asarray(st[q]), np.asarray(st2[q])) for q in st)
    out = pkg.sac_evaluate_agent(agent, env, n_eval_episodes=8, normalize_stats=rb.handle)
    assert np.isfinite(out["mean_reward"]) and out["mean_length"] == 20
    # a plug-in gets the wrapper through the keyword
    menv = pkg.DeviceModuleEnv(_co("reacher3"), E, max_steps=25)
    magent = pkg.SACAgent(pkg.SACLayer(menv.observation_space(), menv.action_space(), hidden_dims=(32, 32)), alg, seed=1)
    magent, mrb, mts, _ = pkg.sac_train_(magent, menv, alg, E * 60, normalize=dict(clip_obs=5.0))
    mst = mrb.handle.norm_get_stats()
    assert mst["obs_count"] > 0 and mst["obs_mean"].shape == (12,) and np.isfinite(mts["critic_losses"]).all()
    out = pkg.sac_evaluate_agent(magent, menv, n_eval_episodes=8, normalize=dict(clip_obs=5.0), normalize_stats=mst)
    assert np.isfinite(out["mean_reward"])


def test_collect_continue_is_one_collection_and_callbacks_train_like_the_plain_loop(pkg):
    """step-granular drivers: collect_rollout(1) + (n - 1) x collect_continue(1) is collect_rollout(n) bit for bit (one opening observe), and sac_train_ with a no-op
    on_step callback over a NormalizeWrapperEnv ends with the statistics, ring and weights of the callback-less run"""
    E, n = 13, 5
    hs = []
    for _ in range(2):
        h, layer = make(pkg, "reacher3", E, 4)
        h.set_params(init_params(pkg, layer)); h.normalize_enable(clip_obs=3.0); h.env_reset(5)
        hs.append(h)
    a, b = hs
    with pytest.raises(pkg.DrilError) as ei:
        b.collect_continue(1, True)                                   # nothing in progress after a reset
    assert ei.value.code == pkg._capi.ERR_NOT_INITIALISED
    for use_random in (True, False):
        a.collect_rollout(n, use_random)
        b.collect_rollout(1, use_random)
        for _ in range(n - 1):
            b.collect_continue(1, use_random)
    _same(_snapshot(pkg, a), _snapshot(pkg, b))
    assert a.norm_get_stats()["obs_count"] == 2 * E * (n + 1)
    b.norm_set_stats(**b.norm_get_stats())
    with pytest.raises(pkg.DrilError):
        b.collect_continue(1, False)                                  # set_stats ends the collection in progress

    class Quiet:
        steps = 0

        def on_step(self, loc):
            Quiet.steps += 1
            return True

    def run(cbs):
        env = pkg.NormalizeWrapperEnv(pkg.MonitorWrapperEnv(pkg.DeviceParallelEnv(pkg.PendulumEnv(max_steps=10), 8, seed=3)), clip_obs=4.0, gamma=0.9)
        alg = pkg.SAC(batch_size=16, buffer_capacity=2048, start_steps=40, train_freq=3, gradient_steps=2)
        agent = pkg.SACAgent(pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(32, 32)), alg, seed=1)
        out = pkg.sac_train_(agent, env, alg, 8 * 40, callbacks=cbs)
        return out[0], out[1]
    ag0, rb0 = run(None)
    ag1, rb1 = run([Quiet()])
    assert Quiet.steps == 5 + 11 * 3
    st0, st1 = rb0.handle.norm_get_stats(), rb1.handle.norm_get_stats()
    assert all(np.array_equal(np.asarray(st0[q]), np.asarray(st1[q])) for q in st0)
    assert_rings_equal(ring(pkg, rb0.handle), ring(pkg, rb1.handle))
    assert np.array_equal(pkg.sac_flatten_params(ag0.parameters), pkg.sac_flatten_params(ag1.parameters))
    # collections: 5 start steps, then (40 - 5) / 3 = 11 (+ 1 = 12 iterations in all) of 3: every collection observes n + 1 times
    assert st0["obs_count"] == 8 * ((5 + 1) + 11 * (3 + 1)) and st0["ret_count"] == 8 * (5 + 11 * 3)


def test_enable_again_keeps_the_statistics_whatever_training_says_and_the_handle_knows_its_keywords(pkg, tmp_path):
    E = 9
    h, _ = make(pkg, "pendulum", E, 5)
    kw = dict(clip_obs=2.5, clip_reward=1.5, gamma=0.9, epsilon=1e-6)
    h.normalize_enable(**kw); h.env_reset(1); h.collect_rollout(4, True)
    st = h.norm_get_stats(); ret = h.norm_get_returns(); obs = h.env_observe()
    h.normalize_set_training(False)
    assert h.normalize_config() == dict(training=False, norm_obs=True, norm_reward=True, clip_obs=2.5, clip_reward=1.5, gamma=np.float32(0.9), epsilon=np.float32(1e-6))
    h.normalize_enable(**kw)                                           # what a second sac_train_ on this handle does: training back on, nothing thrown away
    assert h.normalize_config()["training"] is True
    st2 = h.norm_get_stats()
    assert all(np.array_equal(np.asarray(st[q]), np.asarray(st2[q])) for q in st) and np.array_equal(ret, h.norm_get_returns()) and np.array_equal(obs, h.env_observe())
    h.collect_continue(1, True)                                        # the current observation stayed valid
    fp = pkg.checkpoint.save_normalization_stats(h, tmp_path / "n")
    d = np.load(fp)
    assert float(d["clip_obs"]) == 2.5 and float(d["clip_reward"]) == 1.5 and np.float32(d["gamma"]) == np.float32(0.9) and np.float32(d["epsilon"]) == np.float32(1e-6)
    h.normalize_enable(**{**kw, "clip_obs": 3.0})                      # another wrapper: fresh
    assert h.norm_get_stats()["obs_count"] == 0 and not h.norm_get_returns().any()


def test_evaluating_a_normalised_env_without_statistics_warns(pkg):
    env = pkg.NormalizeWrapperEnv(pkg.DeviceParallelEnv(pkg.PendulumEnv(max_steps=10), 4))
    alg = pkg.SAC(batch_size=16, buffer_capacity=256)
    agent = pkg.SACAgent(pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(32, 32)), alg, seed=1)
    with pytest.warns(RuntimeWarning, match="fresh statistics"):
        pkg.sac_evaluate_agent(agent, env, n_eval_episodes=4)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pkg.sac_evaluate_agent(agent, env, n_eval_episodes=4, normalize_stats="fresh")


# ---- 6: off means off, refusals --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pendulum", "reacher3"])
def test_a_disabled_wrapper_leaves_no_trace(pkg, name):
    E = 20
    a, layer = make(pkg, name, E, 5)
    b, _ = make(pkg, name, E, 5)
    flat = init_params(pkg, layer)
    for h in (a, b):
        h.set_params(flat); h.env_reset(6); h.collect_rollout(2, True)
    b.normalize_enable(); b.normalize_enable(False); b.normalize_enable(False)
    for h in (a, b):
        h.collect_rollout(6, False); h.update(2)
    assert_rings_equal(ring(pkg, a), ring(pkg, b))
    assert np.array_equal(a.get_params(), b.get_params())
    c = pkg._capi
    for call in (b.norm_get_stats, b.norm_get_original, b.norm_get_returns, lambda: b.normalize_set_training(True),
                 lambda: b.norm_set_stats(np.zeros(b.D, F), np.ones(b.D, F), 0, 0.0, 1.0, 0)):
        with pytest.raises(pkg.DrilError) as ei:
            call()
        assert ei.value.code == c.ERR_NOT_INITIALISED and "NormalizeWrapperEnv is off" in str(ei.value)
    for bad in (dict(clip_obs=-1.0), dict(clip_reward=-0.5), dict(epsilon=-1e-3)):
        with pytest.raises(pkg.DrilError) as ei:
            b.normalize_enable(**bad)
        assert ei.value.code == c.ERR_INVALID_ARG
    b.normalize_enable()
    with pytest.raises(pkg.DrilError) as ei:
        b.norm_set_stats(np.zeros(b.D, F), np.ones(b.D, F), -1, 0.0, 1.0, 0)
    assert ei.value.code == c.ERR_INVALID_ARG


def test_external_handles_are_refused(pkg):
    capi = pkg._capi
    cfg = capi.DrilSacConfig()
    lib = capi.load_library()
    assert lib.dril_sac_config_default(cfg, capi.ENV_EXTERNAL) == capi.OK
    cfg.n_envs, cfg.ext_obs_dim, cfg.ext_action_dim, cfg.ext_action_low, cfg.ext_action_high = 4, 5, 2, -1.0, 1.0
    cfg.hidden1 = cfg.hidden2 = 32; cfg.batch_size = 8; cfg.buffer_capacity = 64
    h = pkg.SacHandle(cfg)
    with pytest.raises(pkg.DrilError) as ei:
        h.normalize_enable()
    assert ei.value.code == capi.ERR_UNSUPPORTED and "host" in str(ei.value)
    with pytest.raises(pkg.DrilError) as ei:
        h.norm_get_stats()
    assert ei.value.code == capi.ERR_UNSUPPORTED
