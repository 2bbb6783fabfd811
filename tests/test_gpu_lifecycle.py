"""GPU (-m gpu): every allocation a handle or a population makes goes back when it is closed.  The measure is dril_debug_device_bytes_live: the bytes of device and
pinned memory held through the owning buffers of dril.jl_amd/csrc/dril_devmem.h, process-wide.  Each case reads it, creates, exercises the verbs that allocate lazily,
closes, and asserts the counter equals its first reading exactly (hipMemGetInfo would see the other tenants of the card).

Shapes are the smallest that still reach the lazy allocations: n_envs 8, n_steps 8, batch_size 16, epochs 1, hidden [64, 64] unless a case says otherwise.

Owners these cases do not reach: the RCCL / loopback data-parallel rows (rms_red, pn_red on world_size > 1), epoch_tables / epoch_stats / epoch_index (minibatches above the
small path with normalize_advantage), SAC's it_stamps (cfg.profile_events) and a generic-shape handle's gen_tmp.  Not counted at all, by design: the envs' own arrays
(DeviceEnvs) and deployment policies.

Two statements are worded for the grow-only buffers a handle keeps: the external handle's wrappers give back exactly what switching them on took (the literal "as before
they were switched on" holds only with nothing lazily allocated in between, and is asserted for that), and the population is measured on its second join, after the first
has grown the members' own evaluation buffers.  The two external-handle cases use torch device tensors; the first of them pays torch's start-up (about 11 s measured, once
per session), the cases themselves take well under a second."""
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
F = np.float32
E, T, B = 8, 8, 16
NKW = dict(clip_obs=5.0, clip_reward=5.0, gamma=0.9, epsilon=1e-6)


def _live(pkg) -> int:
    return int(pkg._capi.load_library().dril_debug_device_bytes_live())


def _cfg(pkg, kind, **kw):
    c = pkg._capi.default_config(kind)
    for k, v in {**dict(n_envs=E, n_steps=T, batch_size=B, epochs=1, hidden1=64, hidden2=64), **kw}.items():
        setattr(c, k, v)
    return c


def _params(h, seed=0):
    h.set_params((np.random.default_rng(seed).standard_normal(h.P) * 0.1).astype(F))


def _co(name):
    return str(ROOT / "examples" / "envs" / f"{name}.hsaco")


class _Spaces:
    """what make_sac_config reads of an external env"""

    def __init__(self, pkg, D, A):
        self.kind, self._o, self._a = pkg._capi.ENV_EXTERNAL, pkg.Box(low=(-10.0,) * D, high=(10.0,) * D), pkg.Box(low=(-1.0,) * A, high=(1.0,) * A)

    def observation_space(self):
        return self._o

    def action_space(self):
        return self._a


def test_ppo_cartpole_with_monitor(pkg):
    capi, rng = pkg._capi, np.random.default_rng(1)
    base = _live(pkg)
    h = pkg.Handle(_cfg(pkg, capi.ENV_CARTPOLE, monitor_window=4))
    assert _live(pkg) > base
    _params(h); h.env_reset(3)
    h.collect_rollout(); h.ppo_update()                                             # the persistent small path: small_xchg, epoch_keys, step_stats
    h.set_noise(rng.random(h.N)); h.collect_rollout()                                # noise_dev
    h.set_permutation(rng.permutation(h.N)); h.ppo_update()                           # perm_dev
    obs = rng.standard_normal((5, h.D)).astype(F)
    act, val, lp = h.policy_forward(obs)                                             # policy_host's temporaries
    h.ppo_loss_grad(obs, act, val, val, lp, val)                                     # dril_ppo_loss_grad's
    h.evaluate_agent_device(2)                                                       # eval_snap, eval_cur_*, eval_counter (+ pinned word), eval_events; the monitor set aside and put back
    h.collect_trajectory_device(2, max_steps=6)                                      # traj_blob
    assert h.monitor_stats() is not None                                             # the monitor is the handle's again
    h.close()
    assert _live(pkg) == base


def test_ppo_pendulum_wide_normalising(pkg):
    capi = pkg._capi
    base = _live(pkg)
    h = pkg.Handle(_cfg(pkg, capi.ENV_PENDULUM, hidden1=128, hidden2=128, norm_obs=1, norm_reward=1, norm_training=1, batch_size=64))
    _params(h); h.env_reset(3)
    h.collect_rollout(); h.ppo_update()                                             # the W2 images, retry_snap, step_stats
    h.close()
    assert _live(pkg) == base


def test_ppo_external_handle_on_device_tensors(pkg):
    import torch
    capi, dev = pkg._capi, "cuda"
    D, A = 5, 2
    gen = torch.Generator(device="cpu").manual_seed(0)
    up = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    base = _live(pkg)
    h = pkg.Handle(_cfg(pkg, capi.ENV_EXTERNAL, ext_obs_dim=D, ext_action_dim=A, ext_discrete=0, ext_action_low=-1.0, ext_action_high=1.0, batch_size=E))
    _params(h)
    plain = _live(pkg)
    h.ext_normalize_enable(**NKW); h.ext_monitor_enable(4); h.ext_normalize_enable(False); h.ext_monitor_enable(0)
    assert _live(pkg) == plain                                                      # both off: the counter of before they were switched on
    h.ext_normalize_enable(**NKW); h.ext_monitor_enable(4)
    took = _live(pkg) - plain
    assert took > 0
    raw, env = torch.empty((E, A), device=dev), torch.empty((E, A), device=dev)
    term, tobs = torch.zeros(E, dtype=torch.uint8, device=dev), up(E, D)
    for t in range(T):
        h.ext_act_device(up(E, D), raw, env)
        trunc = torch.full((E,), int(t % 4 == 3), dtype=torch.uint8, device=dev)
        h.ext_record_device(up(E), term, trunc, tobs)
    h.ext_finish_device(up(E, D))
    for n in (E + 3, 4 * E):                                                         # above n_envs: ext_pred_* and, under the normaliser, ext_pred_obs; then the grow path
        h.predict_actions_device(up(n, D), True, None, torch.empty((n, A), device=dev))
    assert h.ext_wrap_info()["allocations"] == 2
    h.ppo_update()
    torch.cuda.synchronize()
    # the same after a rollout and an update.  What those allocated lazily in between (the scratch of predict_actions_device, the update's tables) is the handle's
    # and stays, so the statement is: switching both off gives back exactly what switching them on took
    used = _live(pkg)
    h.ext_normalize_enable(False); h.ext_monitor_enable(0)
    assert used - _live(pkg) == took
    h.close()
    assert _live(pkg) == base


def test_ppo_plugin_handle_normalize_and_fused_evaluation(pkg):
    capi = pkg._capi
    base = _live(pkg)
    h = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, episode_len=20), env_module=_co("cartpole_plugin"))
    _params(h); h.env_reset(3)
    h.collect_rollout(); h.ppo_update()                                             # the layer-by-layer workspace and the update's tables: grow-only, the handle's
    off = _live(pkg)
    h.normalize_enable(**NKW)
    on = _live(pkg)
    h.collect_rollout()
    h.normalize_enable(False)
    assert _live(pkg) == off
    h.normalize_enable(**{**NKW, "gamma": 0.8})                                       # release and re-allocate
    assert _live(pkg) == on
    h.collect_rollout(); h.ppo_update()
    h.evaluate_agent_device(2, persistent=True)                                      # this code object has no fused evaluation kernel: the step-granular launches
    h.close()
    assert _live(pkg) == base
    f = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, episode_len=20), env_module=_co("cartpole_eval_plugin"))
    _params(f); f.env_reset(3)
    f.normalize_enable(**NKW)
    assert f.evaluate_agent_device(2, persistent=True)[3]["path"] == 2               # the fused path: evalf_blob
    assert f.collect_trajectory_device(2, max_steps=6, persistent=True)[3]["path"] == 2   # ... grown for the recording rows
    f.close()
    assert _live(pkg) == base


def _sac(pkg, env, cap=256):
    alg = pkg.SAC(batch_size=B, buffer_capacity=cap, start_steps=16)
    h = pkg.SacHandle(pkg.make_sac_config(env, E, alg, pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(64, 64)), seed=7))
    h.set_params((np.random.default_rng(5).standard_normal(h.P) * 0.1).astype(F))
    return h


def test_sac_pendulum(pkg):
    rng = np.random.default_rng(2)
    base = _live(pkg)
    h = _sac(pkg, pkg.PendulumEnv())
    h.env_reset(0)
    h.train(64)                                                                      # stats_out / ssq_rows at their first capacity
    plain = _live(pkg)
    h.monitor_enable(4); h.collect_rollout(3)                                        # three rows where the block has train_freq: monitor_begin grows it
    h.monitor_enable(8); h.collect_rollout(1)
    h.monitor_enable(0)
    assert _live(pkg) == plain
    h.normalize_enable(**NKW); h.collect_rollout(2); h.normalize_enable(False)
    assert _live(pkg) == plain
    h.evaluate_agent(2)                                                              # ev_*: allocated by the first evaluation, kept
    h.collect_trajectory(2, max_steps=6)                                             # traj_blob (drained before it is replaced)
    h.set_collect_noise(rng.standard_normal((2, E, h.A)).astype(F)); h.collect_rollout(2)   # collect_noise: freed by the collection that used it
    n = 2
    h.set_batches(n, rng.integers(0, h.replay_size(), n * B), *[rng.standard_normal((n * B, h.A)).astype(F) for _ in range(3)])
    h.update(n)                                                                      # inj_*: freed by the update that used them
    h.set_batches(n, rng.integers(0, h.replay_size(), n * B)); h.set_batches(0)      # ... or by the next injection
    held = _live(pkg)
    h.update(300)                                                                    # above the first statistics capacity: ensure_stats grows both tables
    assert _live(pkg) > held
    h.close()
    assert _live(pkg) == base


def test_sac_external_handle_on_device_tensors(pkg):
    import torch
    dev, D, A = "cuda", 5, 2
    gen = torch.Generator(device="cpu").manual_seed(0)
    up = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    rng = np.random.default_rng(4)
    base = _live(pkg)
    h = _sac(pkg, _Spaces(pkg, D, A))
    plain = _live(pkg)
    stored, env = torch.empty((E, A), device=dev), torch.empty((E, A), device=dev)
    term = torch.zeros(E, dtype=torch.uint8, device=dev)

    def steps(k):
        for t in range(k):
            h.ext_act_device(up(E, D), False, None, stored, env)
            h.ext_push_device(up(E), term, torch.full((E,), int(t % 4 == 3), dtype=torch.uint8, device=dev), up(E, D), up(E, D))

    steps(4)
    h.ext_normalize_enable(**NKW); h.ext_monitor_enable(4)
    assert _live(pkg) > plain
    h.ext_collection_begin(); steps(4)
    h.set_batches(2, rng.integers(0, h.replay_size(), 2 * B))                        # the injected batches outlive update_enqueue: they go with the flush
    h.update_enqueue(2); h.update_enqueue(1)
    assert len(h.flush()) == 3
    torch.cuda.synchronize()
    h.ext_normalize_enable(False); h.ext_monitor_enable(0)
    assert _live(pkg) == plain
    h.set_batches(1, rng.integers(0, h.replay_size(), B)); h.update_enqueue(1)       # closed with injected batches still waiting for a flush
    h.close()
    assert _live(pkg) == base


def test_population_of_two(pkg):
    capi = pkg._capi
    base = _live(pkg)
    hs = []
    for seed in (1, 2):
        h = pkg.Handle(_cfg(pkg, capi.ENV_CARTPOLE, seed=seed)); _params(h, seed); h.env_reset(seed); hs.append(h)
    with pkg.Population(hs) as pop:                                                  # a first round: what the verbs allocate lazily ON the members is the members' and stays
        pop.collect_rollout(); pop.ppo_update(); pop.evaluate(2)
    before = _live(pkg)
    pop = pkg.Population(hs)
    assert _live(pkg) > before                                                       # the launch tables, the exchange words, a pinned home block per member
    pop.collect_rollout(); pop.ppo_update(); pop.evaluate(2)                          # the pinned event area
    pop.close()
    assert _live(pkg) == before
    for h in hs:
        h.close()
    assert _live(pkg) == base


def test_refused_creates_hold_nothing(pkg, tmp_path):
    capi = pkg._capi
    base = _live(pkg)
    with pytest.raises(pkg.DrilError):                                               # past the argument checks: the handle exists when the module fails to load
        pkg.Handle(_cfg(pkg, capi.ENV_MODULE), env_module=str(tmp_path / "no_such_plugin.hsaco"))
    assert _live(pkg) == base
    with pytest.raises(pkg.DrilError):                                               # refused outright
        pkg.Handle(_cfg(pkg, capi.ENV_MODULE, norm_obs=1), env_module=_co("cartpole_plugin"))
    assert _live(pkg) == base
    cfg = capi.DrilSacConfig()
    assert capi.load_library().dril_sac_config_default(cfg, capi.ENV_MODULE) == capi.OK
    cfg.n_envs, cfg.hidden1, cfg.hidden2, cfg.batch_size, cfg.buffer_capacity = E, 64, 64, B, 256
    with pytest.raises(pkg.DrilError):                                               # SAC on a Discrete plug-in: refused after the module is loaded
        pkg.SacHandle(cfg, env_module=_co("cartpole_plugin"))
    assert _live(pkg) == base
