"""GPU (-m gpu): device env plug-ins (DRIL_ENV_MODULE) — a user's env compiled into a gfx950 code object (include/device/dril_env_plugin.h), loaded with the HIP
module API and stepped by its own kernels where a built-in kind's env kernels would run.

Checkers: (1) the built-in CartPole / Pendulum, whose TWINS examples/envs/{cartpole,pendulum}_plugin.hip restate (the built-ins are pinned by the CPU oracle in the
other GPU tests), bit for bit; (2) a NumPy float32 restatement of examples/envs/reacher3_plugin.hip; (3) a DRIL_ENV_EXTERNAL handle fed step by step from a second
plug-in handle's env verbs (the construction of test_external_matches_the_fused_cartpole_path): the collection loop against the step-granular verbs.
Nothing here tries to make the device fault: a malformed module is refused by the host-side checks and the descriptor check before anything of it is launched."""
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ENVS = ROOT / "examples" / "envs"
ALL_BUFS = range(10)


def _co(name):
    p = ENVS / f"{name}_plugin.hsaco"
    assert p.exists(), f"{p}: built by the default target of dril.jl_amd/csrc/Makefile"
    return p


def _cfg(pkg, kind, **kw):
    c = pkg._capi.default_config(kind)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _params(P, seed, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(P) * scale).astype(np.float32)


def _stats(s):
    return tuple(getattr(s, n) for n, _ in type(s)._fields_)


def test_describe_the_three_examples(pkg):
    c, p, r = (pkg.describe_env_module(_co(n)) for n in ("cartpole", "pendulum", "reacher3"))
    assert (c["state_dim"], c["obs_dim"], c["action_dim"], c["discrete"], c["episode_len"]) == (4, 4, 2, True, 500) and "CartPole" in c["name"]
    assert (p["state_dim"], p["obs_dim"], p["action_dim"], p["discrete"], p["episode_len"]) == (2, 3, 1, False, 200)
    assert p["action_low"].tolist() == [-2.0] and p["action_high"].tolist() == [2.0]
    assert (r["state_dim"], r["obs_dim"], r["action_dim"], r["discrete"], r["episode_len"], r["name"]) == (9, 12, 3, False, 100, "Reacher3")
    assert r["action_low"].tolist() == [-1.0] * 3 and r["action_high"].tolist() == [1.0] * 3 and r["plugin_abi"] == 1
    h = pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, n_envs=4, n_steps=2, batch_size=8), env_module=_co("reacher3"))
    assert (h.D, h.A, h.discrete) == (12, 3, False) and h.env_module_info()["name"] == "Reacher3"
    net = lambda out: 12 * 64 + 64 + 64 * 64 + 64 + 64 * out + out
    assert h.P == net(3) + net(1) + 3


@pytest.mark.parametrize("name,kind", [("cartpole", 0), ("pendulum", 1)])
def test_twin_env_verbs_are_bit_identical_to_the_builtin(pkg, name, kind):
    """the same expressions compiled inside libdril_hip.so and on their own into a code object: reset states, observations, rewards, flags, terminal observations,
    auto-reset episodes and the raw state agree to the bit over > 500 steps with terminations (CartPole) and truncations (both)"""
    capi = pkg._capi
    E, L = 32, 60
    b = pkg.Handle(_cfg(pkg, kind, n_envs=E, n_steps=2, batch_size=E, episode_len=L))
    m = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=E, n_steps=2, batch_size=E, episode_len=L), env_module=_co(name))
    b.env_reset(5); m.env_reset(5)
    rng = np.random.default_rng(0)
    n_term = n_trunc = 0
    for t in range(520):
        assert np.array_equal(b.env_observe(), m.env_observe()), t
        if kind == 0:
            act = rng.integers(1, 3, E).astype(np.int32)
            act[: E // 2] = 1 + (t // 7) % 2                      # half the envs are pushed one way for a while: poles fall; the rest survive to the time limit
            act[E // 2:] = 1 + t % 2
        else:
            act = rng.uniform(-3, 3, (E, 1)).astype(np.float32)    # beyond Box(-2, 2): the ClampAdapter of the wrapper is exercised
        rb, tb, ub, ob = b.env_step(act); rm, tm, um, om = m.env_step(act)
        assert np.array_equal(rb, rm) and np.array_equal(tb, tm) and np.array_equal(ub, um), t
        assert np.array_equal(ob[ub], om[um]), t
        n_term += int(tb.sum()); n_trunc += int(ub.sum())
        sb, cb = b.env_get_state(); sm, cm = m.env_get_state()
        assert np.array_equal(sb, sm) and np.array_equal(cb, cm), t
    assert n_trunc > 0 and (kind != 0 or n_term > 0)


@pytest.mark.parametrize("name,kind", [("cartpole", 0), ("pendulum", 1)])
@pytest.mark.parametrize("hidden", [(64, 64), (48, 80)])
def test_twin_collection_and_update_equal_the_builtin_on_the_generic_kernels(pkg, monkeypatch, name, kind, hidden):
    """the plug-in collection loop (policy -> plug-in step) against collect_rollout_stepwise of the built-in on the same generic kernels (DRIL_FORCE_GENERIC for the
    fused shape): injected noise and DataLoader order, two iterations, every buffer field to the bit, the update's statistics and parameters equal"""
    capi = pkg._capi
    E, T = 64, 24
    kw = dict(n_envs=E, n_steps=T, batch_size=E * T // 2, epochs=2, episode_len=9, seed=3, hidden1=hidden[0], hidden2=hidden[1], monitor_window=50)
    monkeypatch.setenv("DRIL_FORCE_GENERIC", "1")
    b = pkg.Handle(_cfg(pkg, kind, **kw))
    monkeypatch.delenv("DRIL_FORCE_GENERIC")
    m = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, **kw), env_module=_co(name))
    assert m.P == b.P
    flat = _params(b.P, 3, 0.4)
    for h in (b, m):
        h.set_params(flat); h.env_reset(11)
    for it in range(2):
        rng = np.random.default_rng(10 + it)
        nz = rng.random(E * T) if kind == 0 else (rng.standard_normal((E * T, 1)) * 2).astype(np.float32)
        perm = np.stack([rng.permutation(E * T) for _ in range(2)]).astype(np.int64)
        for h in (b, m):
            h.set_noise(nz); h.collect_rollout()
        for which in ALL_BUFS:
            assert np.array_equal(b.buffer(which), m.buffer(which)), (it, which)
        assert (m.buffer(capi.BUF_FLAGS) & 2).any()
        assert b.monitor_stats() == m.monitor_stats()
        for h in (b, m):
            h.set_permutation(perm)
        sb, sm = b.ppo_update(), m.ppo_update()
        assert _stats(sb) == _stats(sm) and sb.n_updates == 4
        assert np.array_equal(b.get_params(), m.get_params())
    assert "generic" in m.grad_kernel_info().lower() or m.grad_kernel_info() == b.grad_kernel_info()


# ---- reacher3: an env the built-in kinds cannot express --------------------------------------------------------------------------------------------
def _reacher_step(st, act):
    """NumPy float32 twin of Reacher3::step + observe (examples/envs/reacher3_plugin.hip), one statement per product / sum like the source"""
    f = np.float32
    st = st.astype(f).copy(); a = np.clip(act.astype(f), f(-1), f(1))
    dist2 = np.zeros(len(st), f); act2 = np.zeros(len(st), f); out = np.zeros(len(st), bool)
    for i in range(3):
        push = f(0.1) * a[:, i]
        v = (st[:, 3 + i] + push) * f(0.95)
        move = f(0.1) * v
        p = st[:, i] + move
        st[:, i] = p; st[:, 3 + i] = v
        d = p - st[:, 6 + i]
        dist2 = dist2 + d * d
        act2 = act2 + a[:, i] * a[:, i]
        out |= (p < f(-2)) | (p > f(2))
    return st, -dist2 - f(0.01) * act2, out


def _reacher_obs(st):
    return np.concatenate([st, st[:, 0:3] - st[:, 6:9]], axis=1).astype(np.float32)


def test_reacher3_physics_matches_the_numpy_twin(pkg):
    capi = pkg._capi
    E = 48
    h = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=E, n_steps=2, batch_size=E), env_module=_co("reacher3"))
    h.env_reset(3)
    st0, sc0 = h.env_get_state()
    assert st0.shape == (E, 9) and not sc0.any()
    assert (np.abs(st0[:, 0:3]) <= 0.5).all() and not st0[:, 3:6].any() and (np.abs(st0[:, 6:9]) <= 1).all() and len(np.unique(st0[:, 6])) == E
    rng = np.random.default_rng(1)
    st = rng.uniform(-1.9, 1.9, (E, 9)).astype(np.float32)
    h.env_set_state(st, np.zeros(E, np.int32))
    np.testing.assert_array_equal(h.env_observe(), _reacher_obs(st))
    for t in range(40):
        act = rng.uniform(-1.5, 1.5, (E, 3)).astype(np.float32)
        want_st, want_r, want_out = _reacher_step(st, act)
        rew, term, trunc, _ = h.env_step(act)
        np.testing.assert_allclose(rew, want_r, rtol=2e-6, atol=2e-6)          # the device may contract a product into an FMA; NumPy rounds every product
        assert np.array_equal(term, want_out) or np.abs(np.abs(want_st[:, 0:3]) - 2).min() < 1e-5
        got, _ = h.env_get_state()
        live = ~term
        np.testing.assert_allclose(got[live], want_st[live], rtol=2e-6, atol=2e-6)
        assert not trunc.any()
        st = got


def _reacher_pair(pkg, E, T, **kw):
    capi = pkg._capi
    cm = _cfg(pkg, capi.ENV_MODULE, n_envs=E, n_steps=T, batch_size=E * T // 2, epochs=2, seed=7, **kw)
    return cm


def test_reacher3_collection_matches_an_external_handle_fed_from_the_env_verbs(pkg):
    capi = pkg._capi
    E, T, L = 32, 40, 13
    cm = _reacher_pair(pkg, E, T, episode_len=L)
    cx = _cfg(pkg, capi.ENV_EXTERNAL, n_envs=E, n_steps=T, batch_size=E * T // 2, epochs=2, seed=7, ext_obs_dim=12, ext_action_dim=3, ext_discrete=0,
              ext_action_low=-1.0, ext_action_high=1.0)
    col, sim, ext = pkg.Handle(cm, env_module=_co("reacher3")), pkg.Handle(cm, env_module=_co("reacher3")), pkg.Handle(cx)
    assert col.P == ext.P
    flat = _params(col.P, 5, 0.3)
    for h in (col, sim, ext):
        h.set_params(flat)
    nz = np.random.default_rng(2).standard_normal((E * T, 3)).astype(np.float32)
    col.env_reset(11); sim.env_reset(11)
    col.set_noise(nz); col.collect_rollout()
    ext.set_noise(nz)
    for t in range(T):
        raw, ea = ext.ext_act(sim.env_observe())
        rew, term, trunc, tobs = sim.env_step(raw)             # the plug-in wrapper clamps the raw action itself
        ext.ext_record(rew, term, trunc, tobs)
    ext.ext_finish(sim.env_observe())
    fl = col.buffer(capi.BUF_FLAGS)
    assert (fl & 2).any()
    for which in (capi.BUF_OBSERVATIONS, capi.BUF_ACTIONS, capi.BUF_REWARDS, capi.BUF_FLAGS, capi.BUF_LOGPROBS, capi.BUF_VALUES, capi.BUF_LAST_VALUES):
        assert np.array_equal(col.buffer(which), ext.buffer(which)), which
    tr = (fl & 2) != 0                                          # the external path evaluates V(terminal_observation) on the truncated rows alone (another batch shape)
    np.testing.assert_allclose(col.buffer(capi.BUF_BOOTSTRAP)[tr], ext.buffer(capi.BUF_BOOTSTRAP)[tr], atol=2e-5, rtol=2e-5)
    for which in (capi.BUF_ADVANTAGES, capi.BUF_RETURNS):
        np.testing.assert_allclose(col.buffer(which), ext.buffer(which), atol=2e-4, rtol=2e-4)
        ext.set_buffer(which, col.buffer(which))
    assert np.array_equal(col.env_get_state()[0], sim.env_get_state()[0])
    perm = np.stack([np.random.default_rng(e).permutation(E * T) for e in range(2)]).astype(np.int64)
    col.set_permutation(perm); ext.set_permutation(perm)
    sc, sx = col.ppo_update(), ext.ppo_update()
    assert sc.n_updates == sx.n_updates == 4 and sc.loss == pytest.approx(sx.loss, rel=1e-5)
    np.testing.assert_allclose(col.get_params(), ext.get_params(), rtol=1e-5, atol=1e-7)


def test_reacher3_monitor_evaluate_and_determinism(pkg):
    capi = pkg._capi
    E, T, L = 16, 64, 10
    cm = _reacher_pair(pkg, E, T, episode_len=L, monitor_window=1000)
    a, b = pkg.Handle(cm, env_module=_co("reacher3")), pkg.Handle(cm, env_module=_co("reacher3"))
    flat = _params(a.P, 1, 0.2)
    for h in (a, b):
        h.set_params(flat); h.env_reset(4); h.collect_rollout()
    for which in ALL_BUFS:
        assert np.array_equal(a.buffer(which), b.buffer(which)), which       # two collections from the same seed
    rew, fl = a.buffer(capi.BUF_REWARDS).reshape(T, E), a.buffer(capi.BUF_FLAGS).reshape(T, E)
    rets, lens = [], []
    cur_r, cur_l = np.zeros(E, np.float32), np.zeros(E, np.int64)
    for t in range(T):
        cur_r += rew[t]; cur_l += 1
        for e in np.nonzero(fl[t])[0]:
            rets.append(cur_r[e]); lens.append(cur_l[e]); cur_r[e] = 0; cur_l[e] = 0
    r_mean, l_mean, n = a.monitor_stats()
    assert n == len(rets) > E and l_mean == pytest.approx(np.mean(lens)) and r_mean == pytest.approx(np.mean(rets), rel=1e-5)
    s1, r1, l1 = a.evaluate_agent(12, True); s2, r2, l2 = a.evaluate_agent(12, True)
    assert np.array_equal(r1, r2) and np.array_equal(l1, l2) and s1["n_steps"] == s2["n_steps"] and (l1 <= L).all() and np.isfinite(r1).all()


def test_reacher3_training_improves_the_episode_return(pkg):
    """train_ through the public Python surface: DeviceModuleEnv + MonitorWrapperEnv + Agent — the configuration of examples/ppo_device_plugin.py 64 40.  One real run
    of it on an MI355X: the mean episode return over the monitor window went from -221.1 after the first rollout to -25.8 after the fortieth (monotone up to noise of
    about 5); the margin asked for here is 100."""
    env = pkg.MonitorWrapperEnv(pkg.DeviceModuleEnv(_co("reacher3"), 64, seed=0), stats_window=64)
    assert env.observation_space().shape == (12,) and env.action_space().shape == (3,)
    alg = pkg.PPO(n_steps=100, batch_size=1600, epochs=10, learning_rate=1e-3)
    agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space()), alg, seed=0)
    seen = []

    class Log:
        def on_rollout_end(self, loc):
            seen.append(loc["env"].handle.monitor_stats()[0]); return True
    pkg.train_(agent, env, alg, 64 * 100 * 40, callbacks=[Log()])
    assert len(seen) == 40 and np.isfinite(seen).all()
    assert seen[-1] > seen[0] + 100.0, (seen[0], seen[-1])
    with pytest.raises(pkg.DrilError) as e:
        pkg.NormalizeWrapperEnv(pkg.DeviceModuleEnv(_co("reacher3"), 4))
    assert e.value.code == pkg._capi.ERR_UNSUPPORTED and "NormalizeWrapperEnv" in str(e.value)


def test_two_loopback_ranks_own_the_global_env_indices(pkg):
    """world_size 2: rank 1's envs are envs E .. 2E-1 of a single handle over 2E envs (the env seed is seed + global index)"""
    capi = pkg._capi
    E, T = 8, 12
    kw = dict(n_steps=T, batch_size=2 * E * T, epochs=1, episode_len=5, seed=9)
    one = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=2 * E, **kw), env_module=_co("reacher3"))
    hs = [pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=E, rank=r, world_size=2, **kw), env_module=_co("reacher3")) for r in range(2)]
    pkg.Handle.comm_loopback(hs)
    flat = _params(one.P, 2, 0.2)
    one.set_params(flat); one.env_reset(21); one.collect_rollout()
    out, err = [None, None], [None, None]

    def run(r):
        try:
            hs[r].set_params(flat); hs[r].env_reset(21); hs[r].collect_rollout()
            out[r] = {w: hs[r].buffer(w) for w in (capi.BUF_OBSERVATIONS, capi.BUF_ACTIONS, capi.BUF_REWARDS, capi.BUF_FLAGS)}
        except BaseException as ex:   # noqa: BLE001 - re-raised below
            err[r] = ex
    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in ts]; [t.join() for t in ts]
    for ex in err:
        if ex is not None:
            raise ex
    for w, width in ((capi.BUF_OBSERVATIONS, 12), (capi.BUF_ACTIONS, 3), (capi.BUF_REWARDS, 1), (capi.BUF_FLAGS, 1)):
        whole = one.buffer(w).reshape(T, 2 * E, width)
        for r in range(2):
            assert np.array_equal(out[r][w].reshape(T, E, width), whole[:, r * E:(r + 1) * E]), (w, r)


def test_refusals_by_status_and_message(pkg, tmp_path):
    import ctypes as C
    capi = pkg._capi
    lib = capi.load_library()
    with pytest.raises(pkg.DrilError) as e:
        pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=4, n_steps=2, batch_size=8, norm_obs=1), env_module=_co("reacher3"))
    assert e.value.code == capi.ERR_UNSUPPORTED and "NormalizeWrapperEnv" in str(e.value)
    h = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=4, n_steps=2, batch_size=8), env_module=_co("reacher3"))
    for call in (lambda: h.ext_act(np.zeros((4, 12), np.float32)), lambda: h.ext_finish(np.zeros((4, 12), np.float32)), h.norm_get_stats, h.norm_get_original):
        with pytest.raises(pkg.DrilError) as e:
            call()
        assert e.value.code == capi.ERR_UNSUPPORTED and str(e.value)
    sc = capi.DrilSacConfig(); sc.abi_version = capi.SAC_ABI_VERSION; sc.env_kind = capi.ENV_MODULE
    hp = C.c_void_p()
    assert lib.dril_sac_create(C.byref(sc), C.byref(hp)) == capi.ERR_UNSUPPORTED and b"plug-in" in lib.dril_sac_last_error(None)
    builtin = pkg.Handle(_cfg(pkg, 0, n_envs=4, n_steps=2, batch_size=8))
    with pytest.raises(pkg.DrilError) as e:
        builtin.env_module_info()
    assert e.value.code == capi.ERR_UNSUPPORTED
    # a code object compiled against another plug-in ABI number is refused when the handle is created, before anything of it is launched
    other = tmp_path / "abi99.hsaco"
    subprocess.run(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "--no-gpu-bundle-output", "-O3", "-DDRIL_ENV_PLUGIN_ABI=99u", "-I", str(ROOT / "include"),
                    str(ENVS / "reacher3_plugin.hip"), "-o", str(other)], check=True)
    with pytest.raises(pkg.DrilError) as e:
        pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=4, n_steps=2, batch_size=8), env_module=other)
    assert e.value.code == capi.ERR_UNSUPPORTED and "ABI 99" in str(e.value)
    with pytest.raises(pkg.DrilError) as e:
        pkg.describe_env_module(other)
    assert "ABI 99" in str(e.value)
    # a code object that is not a plug-in at all: no descriptor symbol
    src = tmp_path / "plain.hip"
    src.write_text('#include <hip/hip_runtime.h>\nextern "C" __global__ void k(float* x) { x[0] = 1.f; }\n')
    subprocess.run(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "--no-gpu-bundle-output", str(src), "-o", str(tmp_path / "plain.hsaco")], check=True)
    with pytest.raises(pkg.DrilError) as e:
        pkg.describe_env_module(tmp_path / "plain.hsaco")
    assert e.value.code == capi.ERR_UNSUPPORTED and "dril_env_plugin_desc" in str(e.value)
    # a refused module leaves no error behind for the next launch of another handle (the launchers check the runtime's last error after each launch)
    cx = _cfg(pkg, capi.ENV_EXTERNAL, n_envs=2, n_steps=2, batch_size=2, ext_obs_dim=6, ext_action_dim=3, ext_discrete=1)
    hx = pkg.Handle(cx); hx.set_params(_params(hx.P, 0))
    assert np.isfinite(hx.predict_values(np.zeros((5, 6), np.float32))).all()
