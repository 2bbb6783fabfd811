"""GPU (-m gpu): populations of NORMALISING members (docs/population.md, docs/normalized_rollout.md).  A normalising built-in handle whose one-launch collection is on
(dril_norm_rollout_enable) may join; the members collect through one rollout_norm_pop_kernel launch.  The contract is the one of every population: every bit of a
member equals the same handle, with the opt-in on, driven alone — compared on raw bytes against solo handles created in the same test."""
import numpy as np
import pytest

from test_gpu_population import _assert_same, _bytes, _cfg, _close, _drive, _params, _snap_state
from test_gpu_population_eval import _assert_equal as _assert_eval_equal

pytestmark = pytest.mark.gpu

CARTPOLE, PENDULUM = 0, 1
SHAPE = dict(n_envs=5, n_steps=25, batch_size=24, epochs=3, episode_len=11, monitor_window=10, norm_obs=1, norm_reward=1, norm_training=1)   # N = 125: a ragged last minibatch
MEMBERS = [(11, dict()), (12, dict(learning_rate=1e-3, clip_obs=3.0, norm_gamma=0.9)), (13, dict(learning_rate=1e-4, clip_obs=1.5, clip_reward=2.0, norm_gamma=0.95, norm_epsilon=1e-6))]


def _make(pkg, kind, members, optin=True, **extra):
    hs = []
    for seed, over in members:
        h = pkg.Handle(_cfg(pkg, kind, SHAPE, seed, over, **extra))
        h.set_params(_params(h.P, 100 + seed))
        h.env_reset(seed)
        if optin:
            h.norm_rollout_enable(True)
        hs.append(h)
    return hs


def _norm_state(h):
    """what the wrapper holds beyond _snap_state: statistics, counts, the originals of the last step"""
    s = h.norm_get_stats()
    oo, orw = h.norm_get_original()
    return {**{f"norm_{k}": _bytes(np.asarray(v)) for k, v in s.items()}, "orig_obs": _bytes(oo), "orig_rew": _bytes(orw)}


def _drive_norm(pkg, hs, iters, pop=None, between=None):
    rec = _drive(pkg, hs, iters, pop=pop, between=between)
    for m, h in enumerate(hs):
        rec[m][-1].update(_norm_state(h))
    return rec


@pytest.mark.parametrize("kind", [PENDULUM, CARTPOLE], ids=["pendulum", "cartpole"])
def test_normalising_members_bit_identical(pkg, kind):
    """three members with their own seeds, learning rates, clip_obs and norm_gamma, two iterations: every buffer, parameter, Adam moment, statistic, env state and
    monitor figure equals the handle trained alone with the opt-in; in reversed order too"""
    hs = _make(pkg, kind, MEMBERS)
    solo = _drive_norm(pkg, hs, 2)
    assert all(h.norm_rollout_info()["last_collection_path"] == 1 for h in hs)
    _close(hs)
    for order in ([0, 1, 2], [2, 0, 1]):
        hs = _make(pkg, kind, [MEMBERS[i] for i in order])
        with pkg.Population(hs) as pop:
            rec = _drive_norm(pkg, hs, 2, pop=pop)
            info = pop.info()
        assert all(h.norm_rollout_info()["last_collection_path"] == 1 for h in hs)
        _close(hs)
        for k, m in enumerate(order):
            _assert_same(rec[k], solo[m], f"member {m} at position {k}")
        assert info["total_solo_rollouts"] == 0 and info["total_solo_updates"] == 0
        assert info["total_rollout_launches"] == 2 * (1 + 2 * 3) and info["total_update_launches"] == 2       # per iteration: the members' opening observes and ONE kernel
    assert solo[0][-1]["norm_obs_mean"] != solo[1][-1]["norm_obs_mean"] and solo[0][0]["params"] != solo[1][0]["params"]   # the members really differ


def test_refusals(pkg):
    """a normalising member without the opt-in stays refused; so are mixed norm_* flags and a mixed opt-in"""
    capi = pkg._capi
    def refused(hs, code):
        with pytest.raises(pkg.DrilError) as e:
            pkg.Population(hs)
        assert e.value.code == code, str(e.value)
        _close(hs)
    refused(_make(pkg, PENDULUM, MEMBERS[:2], optin=False), capi.ERR_UNSUPPORTED)
    hs = _make(pkg, PENDULUM, MEMBERS[:2]); hs[1].norm_rollout_enable(False)
    refused(hs, capi.ERR_UNSUPPORTED)
    hs = _make(pkg, PENDULUM, MEMBERS[:1]) + _make(pkg, PENDULUM, MEMBERS[1:2], norm_reward=0)
    refused(hs, capi.ERR_INVALID_ARG)
    hs = _make(pkg, PENDULUM, MEMBERS[:1]) + _make(pkg, PENDULUM, MEMBERS[1:2], norm_training=0)
    refused(hs, capi.ERR_INVALID_ARG)
    plain = dict(norm_obs=0, norm_reward=0, norm_training=0)
    hs = _make(pkg, PENDULUM, MEMBERS[:1], optin=False, **plain) + _make(pkg, PENDULUM, MEMBERS[1:2])
    refused(hs, capi.ERR_INVALID_ARG)


def test_evaluate_between_iterations(pkg):
    """Population.evaluate() of normalising members: each runs the solo verb (frozen statistics) after the batched loop and is counted in solo_members; the result is
    the handle's own evaluate_agent_device, and a population that evaluates between two iterations continues bit-identically"""
    kw = dict(n_eval_episodes=6, deterministic=True)
    hs = _make(pkg, PENDULUM, MEMBERS)
    solo = _drive_norm(pkg, hs, 2)
    _close(hs)
    hs = _make(pkg, PENDULUM, MEMBERS)
    for h in hs:
        h.collect_rollout(); h.ppo_update()
    alone = [h.evaluate_agent_device(**kw) for h in hs]
    _close(hs)
    seen = {}
    def between(it, hs_):
        if it == 1:
            seen["res"] = seen["pop"].evaluate(**kw); seen["info"] = seen["pop"].last_eval_info
    hs = _make(pkg, PENDULUM, MEMBERS)
    with pkg.Population(hs) as pop:
        seen["pop"] = pop
        rec = _drive_norm(pkg, hs, 2, pop=pop, between=between)
    _close(hs)
    _assert_eval_equal(seen["res"], alone)
    assert seen["info"]["solo_members"] == 3 and seen["info"]["batched_members"] == 0
    for m in range(3):
        _assert_same(rec[m], solo[m], f"member {m}, evaluated between the iterations")
