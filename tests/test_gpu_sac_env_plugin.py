"""GPU (-m gpu): SAC on device env plug-ins (dril_sac_create_with_env_module) through the C ABI.

  * the Pendulum twin plug-in against built-in Pendulum on its four-launch collection: replay ring bit-identical, three updates within the tolerances of test_gpu_sac.py;
  * the fused head-and-push kernel against the plain three launches (DRIL_SAC_NO_FUSED_HEAD_PUSH=1): every ring field identical;
  * per-dimension Box bounds on a plug-in compiled here whose observation IS the action it received;
  * reacher3's physics and the ring's truncation semantics against the NumPy float32 twin of tests/test_env_plugin.py;
  * determinism, train / iterate, a learning check, the refusals (all decided on the host before a launch).
The A/B switches are latched when a handle is created, so they are set around the creation only (as test_gpu_sac.py does)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_env_plugin import _reacher_obs, _reacher_step

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ENVS = ROOT / "examples" / "envs"
GENCO = ["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "--no-gpu-bundle-output", "-O3", "-fno-slp-vectorize", "-std=c++17", "-I", str(ROOT / "include")]
F = np.float32


def _co(name):
    p = ENVS / f"{name}_plugin.hsaco"
    assert p.exists(), f"{p}: built by the default target of dril.jl_amd/csrc/Makefile"
    return p


def make_module(pkg, path, E, hidden=(32, 32), B=16, cap=4096, seed=7, max_steps=0, act="relu", **alg_kw):
    info = pkg.describe_env_module(path)
    env = pkg.host.ModuleEnv(str(path), info, max_steps or info["episode_len"])
    alg = pkg.SAC(batch_size=B, buffer_capacity=cap, **alg_kw)
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=hidden, activation=act)
    return pkg.SacHandle(pkg.make_sac_config(env, E, alg, layer, seed=seed), env_module=path), layer, alg


def init_params(pkg, layer, seed=0, scale_out=30.0):
    ps = layer.initialparameters(np.random.default_rng(seed))
    ps["actor_head"]["layer_3"]["weight"] *= scale_out
    rng = np.random.default_rng(seed + 1)
    for head in (ps["actor_head"], ps["critic_head"]["layer_1"], ps["critic_head"]["layer_2"]):
        for l in head.values():
            l["bias"] = rng.normal(0, 0.1, l["bias"].shape).astype(F)
    ps["log_std"] = np.full_like(ps["log_std"], -1.0)
    return pkg.sac_flatten_params(ps)


def ring(pkg, h):
    c = pkg._capi
    return {k: h.replay(w) for k, w in (("obs", c.RB_OBSERVATIONS), ("act", c.RB_ACTIONS), ("rew", c.RB_REWARDS), ("term", c.RB_TERMINATED),
                                        ("trunc", c.RB_TRUNCATED), ("next", c.RB_NEXT_OBSERVATIONS))}


def assert_rings_equal(a, b):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def to_env(raw, low, high):
    """to_env(TanhScaleAdapter): scale_to_space(tanh(raw)), the kernels' float32 operation order"""
    return np.tanh(raw.astype(F)).astype(F) * (high - low) / F(2) + (low + high) / F(2)


# ---- the Pendulum twin against the built-in env ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,hidden,fused_plugin", [(8, (32, 32), True), (8, (32, 32), False), (1024, (512, 512), True)])   # 1 024 envs: the f16-piece collection forward on both sides
def test_pendulum_twin_equals_the_builtin_through_collection_and_updates(pkg, monkeypatch, E, hidden, fused_plugin):
    T_lim, steps, B = 5, 11, 16
    cap = 8 * E                                                        # 13 steps of E rows in all: the ring wraps, and every env crosses its time limit twice
    env = pkg.PendulumEnv(max_steps=T_lim)
    alg = pkg.SAC(batch_size=B, buffer_capacity=cap)
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=hidden)
    monkeypatch.setenv("DRIL_SAC_NO_FUSED_COLLECT", "1")               # the built-in on head -> step -> observe -> push, four launches
    b = pkg.SacHandle(pkg.make_sac_config(env, E, alg, layer, seed=7))
    monkeypatch.delenv("DRIL_SAC_NO_FUSED_COLLECT")
    if not fused_plugin:
        monkeypatch.setenv("DRIL_SAC_NO_FUSED_HEAD_PUSH", "1")
    m, mlayer, _ = make_module(pkg, _co("pendulum"), E, hidden=hidden, B=B, cap=cap, seed=7, max_steps=T_lim)
    monkeypatch.delenv("DRIL_SAC_NO_FUSED_HEAD_PUSH", raising=False)
    assert (m.D, m.A, m.P) == (b.D, b.A, b.P) and mlayer.parameterlength() == layer.parameterlength()
    info = m.env_module_info()
    assert info["name"].startswith("Pendulum") and tuple(info["action_low"]) == (-2.0,) and tuple(info["action_high"]) == (2.0,)
    flat = init_params(pkg, layer)
    rng = np.random.default_rng(3)
    nz_rand, nz_pol = rng.random((2, E, 1)).astype(F), rng.normal(0, 1, (steps, E, 1)).astype(F)
    for x in (b, m):
        x.set_params(flat); x.env_reset(11)
        x.set_collect_noise(nz_rand); x.collect_rollout(2, True)       # the start phase: rand(action_space)
        assert x.replay_size() == 2 * E
        x.set_collect_noise(nz_pol); x.collect_rollout(steps, False)
        assert x.replay_size() == cap
    rb, rm = ring(pkg, b), ring(pkg, m)
    assert rb["trunc"].sum() >= E and rb["term"].sum() == 0            # (the ring keeps the last 8 of 13 steps: one time limit of every env is among them)
    assert_rings_equal(rb, rm)
    assert np.array_equal(b.env_observe(), m.env_observe())
    # three gradient steps on injected batches: the same kernels on the same ring
    idx = rng.integers(0, cap, (3, B)).astype(np.int64)
    nz = [rng.normal(0, 1, (3, B, 1)).astype(F) for _ in range(3)]
    out = []
    for x in (b, m):
        x.set_batches(3, idx, *nz)
        st = x.update(3)
        out.append((st, x.last_grads(), x.get_params(), x.get_target_params(), x.get_log_ent_coef()))
    (sb, gb, pb, tb, lb), (sm, gm, pm, tm, lm) = out
    for s1, s2 in zip(sb, sm):
        for k in ("actor_loss", "critic_loss", "entropy_loss", "mean_q_values", "entropy_coefficient", "grad_norm"):
            assert abs(getattr(s1, k) - getattr(s2, k)) <= 1e-4 * max(1.0, abs(getattr(s1, k))), k
    for g1, g2 in zip(gb, gm):
        np.testing.assert_allclose(g2, g1, rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(pm, pb, rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(tm, tb, rtol=2e-4, atol=2e-6)
    assert abs(lm - lb) <= 1e-6
    assert not np.array_equal(pb, flat)


# ---- the fused head-and-push kernel against the plain three launches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,hidden", [(37, (32, 32)), (300, (64, 36))])   # ragged against the 16-env head blocks and the 64-env push blocks; H2 % 4 == 0 (mu inside the head)
def test_fused_head_and_push_equals_the_three_launch_form(pkg, monkeypatch, E, hidden):
    cap = 5 * E + 3                                                    # the wrap falls inside a step's rows
    fused, layer, _ = make_module(pkg, _co("reacher3"), E, hidden=hidden, cap=cap, seed=5, max_steps=4)
    monkeypatch.setenv("DRIL_SAC_NO_FUSED_HEAD_PUSH", "1")
    plain, _, _ = make_module(pkg, _co("reacher3"), E, hidden=hidden, cap=cap, seed=5, max_steps=4)
    monkeypatch.delenv("DRIL_SAC_NO_FUSED_HEAD_PUSH")
    flat = init_params(pkg, layer, scale_out=3.0)
    sizes = []
    for x in (fused, plain):
        x.set_params(flat); x.env_reset(9)
        x.collect_rollout(1, True); sizes.append(x.replay_size())     # one step: nothing pending inside the call
        x.collect_rollout(3, False); sizes.append(x.replay_size())
    assert sizes == [E, 4 * E] * 2
    assert_rings_equal(ring(pkg, fused), ring(pkg, plain))
    for x in (fused, plain):
        x.collect_rollout(4, False)                                   # wraps: 8 E rows into 5 E + 3 slots
        assert x.replay_size() == cap
    rf, rp = ring(pkg, fused), ring(pkg, plain)
    assert_rings_equal(rf, rp)
    assert rf["trunc"].any() and np.isfinite(rf["next"]).all() and np.abs(rf["act"]).max() <= 1.0
    assert np.array_equal(fused.env_observe(), plain.env_observe())
    # the newest E rows are the last step's: their next observation is what the env shows now, except where that step was truncated
    last = slice(cap - E, cap)
    keep = rf["trunc"][last] == 0
    assert np.array_equal(rf["next"][last][keep], fused.env_observe()[keep])


# ---- per-dimension bounds ----------------------------------------------------------------------------------------------------------------------------------------
_ECHO = '''#include "device/dril_env_plugin.h"
struct Echo {{
    static constexpr int S = {A}, D = {A}, A = {A};
    static constexpr bool discrete = {discrete};
    static constexpr int episode_len = 50;
    static constexpr float action_low[A] = {{{low}}}, action_high[A] = {{{high}}};
    static constexpr const char* name = "Echo";
    DRIL_ENV_FN static void reset(const DrilEnvRng& rng, float* st) {{ for (int i = 0; i < S; ++i) st[i] = 0.0f; }}
    DRIL_ENV_FN static void observe(const float* st, float* obs) {{ for (int i = 0; i < D; ++i) obs[i] = st[i]; }}
    DRIL_ENV_FN static float step(float* st, const float* act_f, int act_i, bool* terminated) {{
        float s = 0.0f;
        for (int i = 0; i < S; ++i) {{ st[i] = {act}; s = s + st[i]; }}
        *terminated = false;
        return s;
    }}
}};
DRIL_ENV_PLUGIN(Echo)
'''


def build_echo(tmp_path, name, low, high, discrete=False, extra=()):
    """a plug-in whose state and observation are the action it received (after the wrapper's ClampAdapter), reward = their sum"""
    A = len(low)
    src = tmp_path / f"{name}.hip"
    src.write_text(_ECHO.format(A=A, discrete="true" if discrete else "false", low=", ".join(f"{v}f" for v in low), high=", ".join(f"{v}f" for v in high),
                                act="(float)act_i" if discrete else "act_f[i]"))
    out = tmp_path / f"{name}.hsaco"
    subprocess.run([*GENCO, *extra, str(src), "-o", str(out)], check=True)
    return out


def test_per_dimension_bounds_reach_the_env_and_the_start_phase_is_uniform_in_each_box(pkg, tmp_path):
    low, high = np.array([-1.0, -0.5, 0.0], F), np.array([1.0, 2.0, 3.0], F)
    co = build_echo(tmp_path, "echo3", low, high)
    E, steps = 256, 16
    h, layer, _ = make_module(pkg, co, E, hidden=(32, 32), cap=2 * E * steps, seed=2)
    info = h.env_module_info()
    assert np.array_equal(info["action_low"], low) and np.array_equal(info["action_high"], high) and (h.D, h.A) == (3, 3)
    h.set_params(init_params(pkg, layer, scale_out=300.0)); h.env_reset(1)
    # the start phase: rand(action_space) per dimension; the stored action is the env-space action (off_policy_collection.jl:50-53,72) and the env echoes it
    h.collect_rollout(steps, True)
    r = ring(pkg, h)
    assert np.array_equal(r["act"], r["next"]) and (r["act"] >= low).all() and (r["act"] <= high).all()
    n, width = E * steps, high - low
    # 4 096 uniforms per dimension: the mean's standard deviation is width / sqrt(12 n) = 0.0045 width (margin 0.02 width = 4.4 sigma); the extremes fall
    # within 0.01 width of the bounds except with probability 2 (0.99)^4096 < 1e-17
    assert (np.abs(r["act"].mean(0) - (low + high) / 2) < 0.02 * width).all()
    assert (r["act"].min(0) < low + 0.01 * width).all() and (r["act"].max(0) > high - 0.01 * width).all()
    assert np.allclose(r["rew"], r["act"].sum(1), atol=1e-6)
    # the policy phase: the ring keeps the squashed sample, the env received to_env(TanhScaleAdapter) of it, per dimension
    nz = np.random.default_rng(4).normal(0, 1, (steps, E, 3)).astype(F)
    h.set_collect_noise(nz); h.collect_rollout(steps, False)
    r = ring(pkg, h)
    raw, got = r["act"][n:], r["next"][n:]
    assert np.abs(raw).max() <= 1.0 and np.abs(raw).max() > 0.9         # (a policy that uses its range)
    np.testing.assert_allclose(got, to_env(raw, low, high), rtol=0, atol=2e-6)
    assert (got > low).all() and (got < high).all()
    assert (got.max(0) > low + 0.8 * width).all() and (got.min(0) < low + 0.2 * width).all()   # tanh(tanh(.)) spans (0.12, 0.88) of each box
    # the host-batch verbs read the same table
    obs = np.random.default_rng(5).uniform(-1, 1, (40, 3)).astype(F)
    raw2, env2 = h.predict_actions(obs, True)
    np.testing.assert_allclose(env2, to_env(raw2, low, high), rtol=0, atol=2e-6)


# ---- reacher3: physics and the ring's truncation semantics -------------------------------------------------------------------------------------------------------
def test_reacher3_ring_follows_the_numpy_twin_and_keeps_the_terminal_observation(pkg):
    E, T_lim = 6, 7
    h, layer, _ = make_module(pkg, _co("reacher3"), E, hidden=(32, 32), cap=64 * E, seed=3, max_steps=T_lim)
    h.set_params(init_params(pkg, layer, scale_out=3.0)); h.env_reset(21)
    first = h.env_observe()
    h.collect_rollout(2 * T_lim, False)
    r = {k: v.reshape(2 * T_lim, E, *v.shape[1:]) for k, v in ring(pkg, h).items()}
    assert np.array_equal(r["obs"][0], first)
    one, mone = np.ones(3, F), -np.ones(3, F)
    for t in range(2 * T_lim):
        st = r["obs"][t][:, :9]                                        # reacher3 shows its whole state: p, v, g (and p - g)
        nst, rew, out = _reacher_step(st, to_env(r["act"][t], mone, one))
        np.testing.assert_allclose(r["rew"][t], rew, rtol=1e-5, atol=1e-6)
        assert not out.any() and not r["term"][t].any()               # |p| <= 2 over fourteen steps from |p| <= 0.5
        trunc = (t + 1) % T_lim == 0
        assert (r["trunc"][t] == int(trunc)).all()
        # the next observation of a row: the state after the step — for a truncated row that is the TERMINAL observation, not the fresh episode's
        np.testing.assert_allclose(r["next"][t], _reacher_obs(nst), rtol=1e-5, atol=1e-6)
        if t + 1 < 2 * T_lim:
            if trunc:
                assert (r["obs"][t + 1][:, 3:6] == 0).all() and not np.allclose(r["obs"][t + 1], r["next"][t])   # a fresh episode: v = 0, new p and g
            else:
                assert np.array_equal(r["obs"][t + 1], r["next"][t])
    now = h.env_observe()                                              # the collection ended on a truncation: the env shows the fresh episode
    assert (now[:, 3:6] == 0).all() and not np.allclose(now, r["next"][-1])


# ---- determinism, the training verbs, learning -------------------------------------------------------------------------------------------------------------------
def test_determinism_train_and_iterate_run_on_a_plugin_handle(pkg):
    E = 16
    kw = dict(hidden=(64, 64), B=32, cap=4096, seed=4, start_steps=64, gradient_steps=2)
    rings, params = [], []
    for _ in range(2):
        h, layer, _ = make_module(pkg, _co("reacher3"), E, **kw)
        h.set_params(init_params(pkg, layer, scale_out=1.0)); h.env_reset(4)
        stats, fps, n_upd, iters, total = h.train(64 + 20 * E)
        assert (n_upd, iters, total) == (2 * 21, 21, 64 + 20 * E) and h.replay_size() == total and len(fps) == iters and (fps > 0).all()
        st2, fps2 = h.iterate(5)
        assert len(st2) == 10 and h.replay_size() == total + 5 * E
        assert all(np.isfinite([s.actor_loss, s.critic_loss, s.entropy_loss, s.grad_norm]).all() for s in stats + st2)
        rings.append(ring(pkg, h)); params.append(h.get_params())
        prof = h.profile()
        assert prof["updates"] == 0 or prof["update_ms"] >= 0
    assert_rings_equal(rings[0], rings[1])
    assert np.array_equal(params[0], params[1])


def episode_returns(h, E, T=100, seed=123):
    """mean return of one episode per env under the current policy: reset, T = time limit steps, the rewards of the newest T * E ring rows"""
    h.env_reset(seed)
    h.collect_rollout(T, False)
    rew = h.replay(0 + 2)[-T * E:].reshape(T, E)                      # DRIL_RB_REWARDS
    return float(rew.sum(0).mean())


def test_sac_learns_reacher3(pkg):
    """examples/sac_device_plugin.py at a third of its length.  Measured on one MI355X: the untrained policy's episode return is -106.6, -20.1 after these 10 000
    env steps (the example's 30 000: -15.8); asked for here: above -45, and 50 better than the untrained policy"""
    E = 16
    h, layer, _ = make_module(pkg, _co("reacher3"), E, hidden=(64, 64), B=256, cap=100_000, seed=0, start_steps=1600, gradient_steps=8, learning_rate=1e-3)
    h.set_params(pkg.sac_flatten_params(layer.initialparameters(np.random.default_rng(0))))
    before = episode_returns(h, E)
    h.env_reset(0)
    h.train(10_000)
    after = episode_returns(h, E)
    print(f"[sac reacher3] episode return {before:.1f} -> {after:.1f}")
    assert after > -45.0 and after > before + 50.0, (before, after)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_decided_on_the_host_and_leave_a_healthy_handle_healthy(pkg, tmp_path):
    capi = pkg._capi
    healthy, layer, _ = make_module(pkg, _co("reacher3"), 8, cap=256)
    healthy.set_params(init_params(pkg, layer, scale_out=1.0)); healthy.env_reset(1)

    def still_collects():
        n = healthy.replay_size()
        healthy.collect_rollout(2, False)
        assert healthy.replay_size() == min(256, n + 16) and np.isfinite(healthy.replay(capi.RB_REWARDS)).all()

    def refused(path, word, E=4):
        cfg = capi.DrilSacConfig()
        assert capi.load_library().dril_sac_config_default(cfg, capi.ENV_MODULE) == capi.OK
        cfg.n_envs, cfg.hidden1, cfg.hidden2, cfg.batch_size, cfg.buffer_capacity = E, 32, 32, 8, 64
        with pytest.raises(pkg.DrilError) as e:
            pkg.SacHandle(cfg, env_module=path)
        assert e.value.code == capi.ERR_UNSUPPORTED and word in str(e.value), str(e.value)
        still_collects()

    refused(_co("cartpole"), "Discrete")                                                   # SAC needs a Box
    refused(build_echo(tmp_path, "flat_dim", [-1.0, 0.5], [1.0, 0.5]), "action_low")      # ClampAdapter's "no clamp" convention: no finite Box to scale into
    refused(build_echo(tmp_path, "wide", [-1.0] * 17, [1.0] * 17), "17 action dims")      # above the SAC kernels' 16
    refused(build_echo(tmp_path, "abi2", [-1.0], [1.0], extra=("-DDRIL_ENV_PLUGIN_ABI=2u",)), "ABI 2")
    # 16 action dims is the limit, not beyond it
    ok, l16, _ = make_module(pkg, build_echo(tmp_path, "sixteen", [-1.0] * 16, [float(i + 1) for i in range(16)]), 4, cap=64)
    ok.set_params(init_params(pkg, l16, scale_out=1.0)); ok.env_reset(0); ok.collect_rollout(3, False)
    assert ok.replay_size() == 12 and (np.abs(ok.replay(capi.RB_NEXT_OBSERVATIONS)) <= np.arange(1, 17)).all()
    # the env is not on the host: the host-env verb stays refused on a plug-in handle; a built-in handle has no plug-in to describe
    z = np.zeros((8, 12), F)
    with pytest.raises(pkg.DrilError) as e:
        healthy.ext_push(z, np.zeros((8, 3), F), np.zeros(8, F), np.zeros(8, np.uint8), np.zeros(8, np.uint8), z)
    assert e.value.code == capi.ERR_UNSUPPORTED and "plug-in" in str(e.value)
    env = pkg.PendulumEnv()
    b = pkg.SacHandle(pkg.make_sac_config(env, 4, pkg.SAC(batch_size=8, buffer_capacity=64), pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(32, 32))))
    with pytest.raises(pkg.DrilError) as e:
        b.env_module_info()
    assert e.value.code == capi.ERR_UNSUPPORTED
    still_collects()
