"""GPU (-m gpu): the one-launch update of a generic handle — dril_update_fused_enable, ppo_update_generic_small_kernel (docs/generic_update.md) — through pkg.Handle on
DRIL_ENV_EXTERNAL and forced-generic handles whose rollout buffer is set by set_buffer, and on the reacher3 plug-in.  Cases, inputs, the float64 restatement and
the bounds: tests/generic_update_cases.py (held to its own terms on the CPU by tests/test_generic_update_cases.py).  The oracle and float64 references are computed
once per process and shared.  Nothing here tries to make the device fault: what the kernel cannot hold is refused on the host before anything is launched."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import generic_update_cases as G

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _handle(pkg, r, fused, cfg=None):
    h = pkg.Handle(cfg or r["cfg"])
    h.set_params(r["flat"])
    G.load(h, pkg._capi, r["bufs"], r["perm"])
    if fused:
        h.update_fused_enable(True)
        assert h.update_fused_info()["enabled"] and h.update_fused_info()["available"]
    return h


def _state(h):
    s = h.get_optimizer_state()
    return h.get_params(), s["m"], s["v"], np.asarray(s["beta_powers"], np.float32), s["steps"]


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == np.float32 else x, np.asarray(y).view(np.uint32) if np.asarray(y).dtype == np.float32 else y)
               for x, y in zip(a, b))


def _triple(s):
    return (s.n_updates, s.early_stopped, s.nan_or_inf)


# ---- 1. one optimiser step against float64 ----
@pytest.mark.parametrize("c", G.ONE_STEP, ids=lambda c: c["name"])
def test_one_optimiser_step_against_float64(pkg, oracle_mod, c):
    r = G.reference(oracle_mod, pkg._capi, c, with_f32=True)
    so = r["stats"]
    hf, hs = _handle(pkg, r, True), _handle(pkg, r, False)
    sf, ss = hf.ppo_update(), hs.ppo_update()
    info = hf.update_fused_info()
    assert (info["last_update_path"], info["last_update_launches"]) == (1, 1) and hs.update_fused_info()["last_update_path"] == 0
    assert "ppo_update_generic_small_kernel" in hf.grad_kernel_info()
    assert _triple(sf) == _triple(so) == (1, 0, 0)
    r_dev, r_orc, r_f32 = G.distances(r, hf.get_params()); r_step = G.distances(r, hs.get_params())[0]
    print(f"[{c['name']}] distance of the update from float64: one launch {r_dev:.2e}, per step {r_step:.2e}, oracle {r_orc:.2e}, Float32 loop {r_f32:.2e}; "
          f"loss {sf.loss:.7f} vs {so.loss:.7f}, grad_norm {sf.grad_norm:.6f} vs {so.grad_norm:.6f}")
    assert sf.loss == pytest.approx(so.loss, rel=G.LOSS_REL, abs=G.LOSS_ABS) and sf.grad_norm == pytest.approx(so.grad_norm, rel=G.GNORM_REL)
    np.testing.assert_allclose(hf.get_params(), r["params"], rtol=G.PARAM_RTOL, atol=G.PARAM_ATOL)
    assert r_dev <= G.yardstick_bound(r_f32, r_orc)
    hf.close(); hs.close()


# ---- 2. control flow ----
@pytest.mark.parametrize("c", G.CONTROL + ["kl-mid"], ids=lambda c: c if isinstance(c, str) else c["name"])
def test_control_flow(pkg, oracle_mod, c):
    if c == "kl-mid":
        c, s_star = G.kl_mid_case(oracle_mod, pkg._capi)
    r = G.reference(oracle_mod, pkg._capi, c)
    so = r["stats"]
    h = _handle(pkg, r, True)
    sh = h.ppo_update()
    assert _triple(sh) == _triple(so)
    if c["name"].startswith("kl-stop-mid"):
        assert _triple(sh) == (s_star, 1, 0)
    if c["kw"].get("has_target_kl") and c["name"].startswith("kl-stop-before"):
        assert sh.early_stopped == 1 and sh.n_updates <= 1
    if so.n_updates:
        assert sh.loss == pytest.approx(so.loss, rel=G.LOSS_REL, abs=G.LOSS_ABS) and sh.grad_norm == pytest.approx(so.grad_norm, rel=G.GNORM_REL)
    np.testing.assert_allclose(h.get_params(), r["params"], rtol=G.PARAM_RTOL, atol=G.PARAM_ATOL)
    assert h.get_optimizer_state()["steps"] == so.n_updates
    if c["epochs"] == 0:
        assert np.array_equal(h.get_params(), r["flat"]) and h.update_fused_info()["last_update_launches"] == 0
    else:
        assert h.update_fused_info()["last_update_path"] == 1
    h.close()


# ---- 3. launch boundaries ----
def test_launch_boundaries_do_not_change_a_bit(pkg, oracle_mod, monkeypatch):
    c = G.CHUNKS
    r = G.reference(oracle_mod, pkg._capi, c)
    one = _handle(pkg, r, True)
    monkeypatch.setenv("DRIL_DEBUG", "1"); monkeypatch.setenv("DRIL_SMALL_CHUNK", "3")
    cut = _handle(pkg, r, True)
    monkeypatch.delenv("DRIL_SMALL_CHUNK"); monkeypatch.delenv("DRIL_DEBUG")
    assert (one.update_fused_info()["steps_per_launch"] >= 14, cut.update_fused_info()["steps_per_launch"]) == (True, 3)
    for rnd in range(2):                                                             # the second round starts from the first one's state: Adam parity 14, moments non-zero
        s1, s3 = one.ppo_update(), cut.ppo_update()
        assert _triple(s1) == _triple(s3) == (14, 0, 0)
        assert (one.update_fused_info()["last_update_launches"], cut.update_fused_info()["last_update_launches"]) == (1, 5)
        a, b = _state(one), _state(cut)
        assert _same_bits(a, b) and a[4] == 14 * (rnd + 1)
        assert np.array_equal(one.step_stats(14).view(np.uint32), cut.step_stats(14).view(np.uint32))
        assert (one.step_stats(14)[:, 9] == 1.0).all()
        if rnd == 0:
            np.testing.assert_allclose(a[0], r["params"], rtol=G.SHORT_RTOL, atol=G.SHORT_ATOL)
            again = _handle(pkg, r, True); again.ppo_update()                        # the same state run a second time: the same bits
            assert _same_bits(_state(again), a) and np.array_equal(again.step_stats(14).view(np.uint32), one.step_stats(14).view(np.uint32))
            again.close()
    one.close(); cut.close()


# ---- 4. the README shape ----
def test_readme_shape_short_and_full(pkg, oracle_mod):
    capi = pkg._capi
    rs = G.reference(oracle_mod, capi, G.README_SHORT)
    h2 = _handle(pkg, rs, True)
    s2 = h2.ppo_update()
    assert s2.n_updates == rs["stats"].n_updates == 256
    print(f"[readme] first 256 optimiser steps: max abs parameter difference {np.abs(h2.get_params() - rs['params']).max():.2e}")
    np.testing.assert_allclose(h2.get_params(), rs["params"], rtol=G.SHORT_RTOL, atol=G.SHORT_ATOL)
    h2.close()
    r = G.reference(oracle_mod, capi, G.README, with_f32=True)
    h, hs = _handle(pkg, r, True), _handle(pkg, r, False)
    sh = h.ppo_update(); hs.ppo_update()
    info = h.update_fused_info()
    assert sh.n_updates == r["stats"].n_updates == 1280 and not sh.early_stopped
    assert (info["last_update_path"], info["last_update_launches"]) == (1, 1) and info["steps_per_launch"] >= 1280
    r_dev, r_orc, r_f32 = G.distances(r, h.get_params()); r_step = G.distances(r, hs.get_params())[0]
    print(f"[readme] distance of the 1 280-step update from the float64 loop: one launch {r_dev:.2e}, per step {r_step:.2e}, oracle {r_orc:.2e}, Float32 loop {r_f32:.2e}")
    assert r_dev <= G.yardstick_bound(r_f32, r_orc)
    h.close(); hs.close()


# ---- 5. launch count ----
def test_launches_do_not_grow_with_the_epochs(pkg, oracle_mod):
    out = []
    for c in G.COUNT:
        r = G.reference(oracle_mod, pkg._capi, c)
        h = _handle(pkg, r, True); s = h.ppo_update()
        assert _triple(s) == _triple(r["stats"])
        np.testing.assert_allclose(h.get_params(), r["params"], rtol=G.SHORT_RTOL, atol=G.SHORT_ATOL)
        out.append((s.n_updates, h.update_fused_info()["last_update_launches"])); h.close()
    assert out[1][0] == 4 * out[0][0] and out[0][1] == out[1][1] == 1


# ---- 6. either route may follow the other ----
def test_fused_per_step_fused_on_one_handle(pkg, oracle_mod):
    capi = pkg._capi; c = G.SEQUENCE
    r = G.reference(oracle_mod, capi, c)                                             # (its oracle has run one update; a fresh one runs all three)
    o = oracle_mod.Oracle(r["cfg"]); o.set_params(r["flat"])
    h = _handle(pkg, r, False)
    steps = 0
    for k, fused in enumerate((True, False, True)):
        perm = G.make_perm(c, salt=k + 1)
        G.load(o, capi, r["bufs"], perm); h.set_permutation(perm)
        h.update_fused_enable(fused)
        sh, so = h.ppo_update(), o.ppo_update()
        assert h.update_fused_info()["last_update_path"] == int(fused) and _triple(sh) == _triple(so)
        steps += so.n_updates
        np.testing.assert_allclose(h.get_params(), o.get_params(), rtol=G.SHORT_RTOL, atol=G.SHORT_ATOL)
        st = h.get_optimizer_state()
        assert st["steps"] == steps
        exp = [np.float32(r["cfg"].adam_beta1), np.float32(r["cfg"].adam_beta2)]         # Optimisers.Adam's beta powers before step `steps + 1`, carried in Float32 as the oracle does
        for _ in range(steps):
            exp = [np.float32(exp[0] * np.float32(r["cfg"].adam_beta1)), np.float32(exp[1] * np.float32(r["cfg"].adam_beta2))]
        assert st["beta_powers"][0] == pytest.approx(float(exp[0]), rel=1e-6) and st["beta_powers"][1] == pytest.approx(float(exp[1]), rel=1e-6)
    h.close()


# ---- 7. off means off ----
@pytest.mark.parametrize("forced", [False, True], ids=["external", "forced-generic-cartpole"])
def test_off_means_off(pkg, oracle_mod, monkeypatch, forced):
    capi = pkg._capi
    if forced:                                                                       # a fused-shape built-in pushed onto the generic kernels
        monkeypatch.setenv("DRIL_FORCE_GENERIC", "1")
        cfg = capi.default_config(capi.ENV_CARTPOLE); cfg.n_envs, cfg.n_steps, cfg.batch_size, cfg.epochs, cfg.episode_len = 4, 16, 16, 2, 20

        def make():
            h = pkg.Handle(cfg); h.set_params((np.random.default_rng(3).standard_normal(h.P) * 0.3).astype(np.float32)); h.env_reset(5); h.collect_rollout(); return h
    else:
        r = G.reference(oracle_mod, capi, G.SEQUENCE)
        make = lambda: _handle(pkg, r, False)
    a, b, f = make(), make(), make()
    a.update_fused_enable(True); a.update_fused_enable(False)
    f.update_fused_enable(True)
    assert not a.update_fused_info()["enabled"] and a.update_fused_info()["available"]
    sa, sb, sf = a.ppo_update(), b.ppo_update(), f.ppo_update()
    assert _same_bits(_state(a), _state(b)) and a.update_fused_info()["last_update_path"] == 0 and f.update_fused_info()["last_update_path"] == 1
    assert _triple(sf) == _triple(sb)
    np.testing.assert_allclose(f.get_params(), b.get_params(), rtol=G.SHORT_RTOL, atol=G.SHORT_ATOL)   # the two routes agree like device and oracle do
    for h in (a, b, f):
        h.close()


# ---- 8. refusals ----
def _refusal_cfgs(pkg):
    capi = pkg._capi
    base = G.case("refuse", 5, 3, True, [16, 24], "tanh", 8, 4, 8, epochs=1)
    fused_shape = capi.default_config(capi.ENV_CARTPOLE); fused_shape.n_envs, fused_shape.n_steps, fused_shape.batch_size, fused_shape.epochs = 4, 8, 8, 1
    wide = G.case("refuse-wide", 5, 3, True, [65], "tanh", 8, 4, 8)
    over = G.case("refuse-p", 16, 8, False, [63, 49, 26], "tanh", 8, 4, 8)             # inside every other cap, one float over the P cap
    assert G.param_count(over) == 11264 + 1
    return dict(fused_shape=fused_shape, batch_1=G.make_cfg(capi, dict(base, B=1)), batch_65=G.make_cfg(capi, dict(base, B=65, E=5, T=13)), params_over=G.make_cfg(capi, over),
                width_over=G.make_cfg(capi, wide), loopback=G.make_cfg(capi, base))


@pytest.mark.parametrize("which", ["fused_shape", "batch_1", "batch_65", "params_over", "width_over", "loopback"])
def test_refusals_leave_the_handle_as_it_was(pkg, which):
    capi = pkg._capi
    cfg = _refusal_cfgs(pkg)[which]

    def make():
        h = pkg.Handle(cfg)
        if which == "loopback":
            pkg.Handle.comm_loopback([h])
        rng = np.random.default_rng(4); N = cfg.n_envs * cfg.n_steps
        h.set_params((rng.standard_normal(h.P) * 0.3).astype(np.float32))
        if which == "fused_shape":
            h.env_reset(1); h.collect_rollout()
        else:
            act = (rng.integers(0, h.A, N) + cfg.action_start).astype(np.int32) if h.discrete else rng.normal(0, 1, (N, h.A)).astype(np.float32)
            for w, arr in ((capi.BUF_OBSERVATIONS, rng.standard_normal((N, h.D)).astype(np.float32)), (capi.BUF_ACTIONS, act), (capi.BUF_ADVANTAGES, rng.standard_normal(N).astype(np.float32)),
                           (capi.BUF_RETURNS, rng.standard_normal(N).astype(np.float32)), (capi.BUF_VALUES, rng.standard_normal(N).astype(np.float32)),
                           (capi.BUF_LOGPROBS, (-1.0 + 0.1 * rng.standard_normal(N)).astype(np.float32))):
                h.set_buffer(w, arr)
        return h
    a, b = make(), make()
    if which == "params_over":
        assert a.P == a.update_fused_info()["max_params"] + 1
    with pytest.raises(pkg.DrilError) as e:
        a.update_fused_enable(True)
    info = a.update_fused_info()
    assert e.value.code == capi.ERR_UNSUPPORTED and info["reason"] and info["reason"][:120] in str(e.value) and not info["available"] and not info["enabled"]
    if which == "batch_1":                                                           # (one sample: std of one element is NaN, ppo.jl:350-356 — both handles report it alike)
        ra, rb = (h.lib.dril_ppo_update(h._h, C.byref(capi.DrilPPOStats())) for h in (a, b))
        assert ra == rb
    else:
        a.ppo_update(); b.ppo_update()
    assert _same_bits(_state(a), _state(b)) and a.update_fused_info()["last_update_path"] == 0
    a.close(); b.close()


# ---- 9. non-finite input ----
def test_a_nan_advantage_ends_the_update_like_the_per_step_route(pkg, oracle_mod):
    capi = pkg._capi; c = G.NAN_CASE
    cfg = G.make_cfg(capi, c)
    o = oracle_mod.Oracle(cfg); flat = G.make_params(c); o.set_params(flat)
    bufs = G.make_data(capi, c, o); perm = G.make_perm(c)
    adv = bufs[capi.BUF_ADVANTAGES].copy(); adv[int(perm[0, 19])] = np.nan; bufs[capi.BUF_ADVANTAGES] = adv      # in the third minibatch of the first epoch
    r = dict(cfg=cfg, flat=flat, bufs=bufs, perm=perm)
    out = []
    for fused in (True, False):
        h = _handle(pkg, r, fused); st = capi.DrilPPOStats()
        rc = h.lib.dril_ppo_update(h._h, C.byref(st))
        out.append((rc, _triple(st), h.get_params(), h.get_optimizer_state()["steps"])); h.close()
    (rcf, tf, pf, nf), (rcs, ts, ps, ns) = out
    assert rcf == rcs == capi.ERR_NAN_IN_GRADS and tf == ts == (2, 0, 1) and nf == ns == 2
    np.testing.assert_allclose(pf, ps, rtol=G.SHORT_RTOL, atol=G.SHORT_ATOL)
    assert np.isfinite(pf).all()


# ---- 10. end to end on a plug-in ----
def test_reacher3_trains_with_the_fused_update(pkg):
    """the configuration and the pass mark of tests/test_gpu_env_plugin.py::test_reacher3_training_improves_the_episode_return, at the batch size the verb is for (64,
    the reference's default, where that test has 1600)"""
    co = ROOT / "examples" / "envs" / "reacher3_plugin.hsaco"
    assert co.exists(), f"{co}: built by the default target of dril.jl_amd/csrc/Makefile"
    env = pkg.MonitorWrapperEnv(pkg.DeviceModuleEnv(co, 64, seed=0), stats_window=64)
    alg = pkg.PPO(n_steps=100, batch_size=64, epochs=10, learning_rate=1e-3)
    agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space()), alg, seed=0)
    seen = []

    class Log:
        def on_rollout_end(self, loc):
            seen.append(loc["env"].handle.monitor_stats()[0]); return True
    pkg.train_(agent, env, alg, 64 * 100 * 40, callbacks=[Log()], fused_update=True)
    info = env.handle.update_fused_info()
    assert info["enabled"] and (info["last_update_path"], info["last_update_launches"]) == (1, 1) and agent.gradient_updates == 40 * 1000
    assert len(seen) == 40 and np.isfinite(seen).all()
    assert seen[-1] > seen[0] + 100.0, (seen[0], seen[-1])
