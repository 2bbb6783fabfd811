"""GPU (-m gpu): populations of device env plug-in handles (docs/population.md, "Plug-in members").  A member must be BIT-IDENTICAL to the same handle driven alone
with dril_rollout_fused_enable(h, 1) and dril_update_fused_enable(h, 1): the batched kernels (the plug-in's dril_env_plugin_rollout_pop, the library's
ppo_update_generic_small_pop_kernel) run the solo kernels' device code on the solo path's own argument blocks.  Every comparison is on raw bytes, with the helpers
of tests/test_gpu_population.py; the yardstick is always a set of solo handles with the same configs and both opt-ins on.

The shape is the smallest that reaches every branch: 20 envs are a full and a partial tile of 16, 13 steps under a time limit of 11 give truncations with their
bootstrap pass, batch_size 64 is two sample tiles of 32, N = 260 is four full minibatches and a ragged one of 4, two epochs are ten optimiser steps."""
from pathlib import Path

import numpy as np
import pytest

from test_gpu_population import _assert_same, _bytes, _close, _drive, _params, _refused, _snap_state, _stats

pytestmark = pytest.mark.gpu
ENVS = Path(__file__).resolve().parents[1] / "examples" / "envs"
SHAPE = dict(n_envs=20, n_steps=13, batch_size=64, epochs=2, episode_len=11)
N = SHAPE["n_envs"] * SHAPE["n_steps"]
STEPS = 10
MON = dict(monitor_window=10)
R_MEMBERS = [(11, dict(MON)), (12, dict(learning_rate=1e-3, gamma=0.95, clip_range=0.1, ent_coef=0.01)), (13, dict(MON, learning_rate=2e-3, gamma=0.9, clip_range=0.3, ent_coef=0.02))]
C_MEMBERS = [(21, dict(MON)), (22, dict(learning_rate=1e-3, gamma=0.95, clip_range=0.1, ent_coef=0.01, has_clip_range_vf=1, clip_range_vf=0.2)), (23, dict(MON, learning_rate=2e-3))]
REACHER = dict(name="reacher3_pop", hidden=(64, 64), activation=0)       # Box, D 12, A 3
CARTPOLE = dict(name="cartpole_pop", hidden=(32, 48), activation=1)      # Categorical, relu


def _co(name):
    p = ENVS / f"{name}_plugin.hsaco"
    assert p.exists(), f"{p}: built by the default target of dril.jl_amd/csrc/Makefile"
    return str(p)


def _one(pkg, seed, over, name, hidden, activation, rollout=True, update=True, scaling=False, shape=SHAPE):
    c = pkg._capi.default_config(pkg._capi.ENV_MODULE)
    for k, v in {**shape, **over}.items():
        setattr(c, k, v)
    c.seed, c.n_hidden, c.activation = seed, len(hidden), activation
    for i, w in enumerate(hidden):
        c.hidden[i] = w
    h = pkg.Handle(c, env_module=_co(name))
    if scaling:
        h.scaling_enable(True)
    if rollout:
        h.rollout_fused_enable(True)
    if update:
        h.update_fused_enable(True)
    h.set_params(_params(h.P, 100 + seed))
    h.env_reset(seed)
    return h


def _make(pkg, members, env, **kw):
    return [_one(pkg, seed, over, **env, **kw) for seed, over in members]


_SOLO = {}


def _solo(pkg, key, members, env, iters=2, between=None):
    """the solo yardstick of a member list (both opt-ins on, driven alone), computed once per module and never changed"""
    if key not in _SOLO:
        hs = _make(pkg, members, env)
        _SOLO[key] = _drive(pkg, hs, iters, between=between)
        _close(hs)
    return _SOLO[key]


def _pop_run(pkg, members, env, iters=2, between=None):
    hs = _make(pkg, members, env)
    with pkg.Population(hs) as pop:
        rec = _drive(pkg, hs, iters, pop=pop, between=between)
        info = pop.info()
    _close(hs)
    return rec, info


def _case_one(pkg, key, members, env):
    solo = _solo(pkg, key, members, env)
    rec, info = _pop_run(pkg, members, env)
    for m in range(3):
        _assert_same(rec[m], solo[m], f"member {m}")
        assert solo[m][0]["stats"] != solo[(m + 1) % 3][0]["stats"] and solo[m][0]["buf0"] != solo[(m + 1) % 3][0]["buf0"]   # the members really differ
        assert any(f & 2 for f in solo[m][0]["buf7"]), "no truncation inside the rollout"
    assert info["members"] == 3 and info["total_solo_rollouts"] == 0 and info["total_solo_updates"] == 0
    assert info["total_rollout_launches"] == 2 and info["total_update_launches"] == 2
    # the train verb against dril_train
    hs = _make(pkg, members, env)
    alone = [h.train(2 * N)[0] for h in hs]
    after_alone = [_snap_state(h) for h in hs]
    _close(hs)
    hs = _make(pkg, members, env)
    with pkg.Population(hs) as pop:
        stats, fps = pop.train(2 * N)
        assert len(stats) == 2 and all(f > 0 for row in fps for f in row)
        for m, h in enumerate(hs):
            assert [_stats(stats[i][m]) for i in range(2)] == [_stats(s) for s in alone[m]]
            assert _snap_state(h) == after_alone[m] == {k: solo[m][1][k] for k in after_alone[m]}
        assert pop.info()["last_launches_per_iteration"] == 2.0
    _close(hs)


def test_reacher3_members_bit_identical(pkg):
    """case 1 (fails without the feature: the join is refused): three reacher3 members with their own seeds and run-time hyper-parameters, the monitor on for two"""
    _case_one(pkg, "reacher", R_MEMBERS, REACHER)


def test_cartpole_twin_members_bit_identical(pkg):
    """case 2: the Categorical head, hidden [32, 48] relu, has_clip_range_vf on one member"""
    _case_one(pkg, "cartpole", C_MEMBERS, CARTPOLE)


def test_position_and_company_do_not_matter(pkg):
    """case 3: reversed member order, and one member in the company of two others"""
    solo = _solo(pkg, "reacher", R_MEMBERS, REACHER)
    rec, _ = _pop_run(pkg, R_MEMBERS[::-1], REACHER)
    for m in range(3):
        _assert_same(rec[m], solo[2 - m], f"member {2 - m} at position {m}")
    others = [(41, dict()), (42, dict(MON, learning_rate=5e-4))]
    rec, _ = _pop_run(pkg, [others[0], R_MEMBERS[1], others[1]], REACHER)
    _assert_same(rec[1], solo[1], "member 1 in other company")


def test_launch_boundaries_and_a_member_that_stops_early(pkg, monkeypatch):
    """case 4: three optimiser steps per launch (four launches per iteration) leave the bytes of the one-launch solo handles; a member whose target_kl stops it early
    idles through the later launches while the others finish"""
    members = [R_MEMBERS[0], (12, dict(R_MEMBERS[1][1], has_target_kl=1, target_kl=1e-12)), R_MEMBERS[2]]
    solo = _solo(pkg, "reacher-kl", members, REACHER)
    plain = _solo(pkg, "reacher", R_MEMBERS, REACHER)
    n_upd = [int(np.frombuffer(solo[m][0]["stats"][10], np.int32)[0]) for m in range(3)]
    stopped = [int(np.frombuffer(solo[m][0]["stats"][11], np.int32)[0]) for m in range(3)]
    assert 0 <= n_upd[1] < STEPS and stopped[1] == 1 and n_upd[0] == n_upd[2] == STEPS and stopped[0] == stopped[2] == 0   # on the SOLO handles: the case cannot pass empty
    monkeypatch.setenv("DRIL_DEBUG", "1"); monkeypatch.setenv("DRIL_SMALL_CHUNK", "3")
    rec, info = _pop_run(pkg, members, REACHER)
    for m in range(3):
        _assert_same(rec[m], solo[m], f"member {m}")
    _assert_same(rec[0], plain[0], "member 0 beside a member that stopped")
    assert info["last_update_launches"] == 4 and info["total_update_launches"] == 8 and info["total_solo_updates"] == 0
    rec, info = _pop_run(pkg, R_MEMBERS, REACHER)
    for m in range(3):
        _assert_same(rec[m], plain[m], f"member {m} in launches of three steps")


def test_injected_noise_and_permutation(pkg):
    """case 5: a member given an injected noise table and DataLoader order stays in the batch and equals its solo twin given the same tables"""
    noise = np.random.default_rng(5).standard_normal((N, 3)).astype(np.float32)
    perm = np.stack([np.random.default_rng(60 + e).permutation(N) for e in range(SHAPE["epochs"])]).astype(np.int64)
    def inject(it, hs):
        if it == 0:
            hs[1].set_noise(noise); hs[1].set_permutation(perm)
    hs = _make(pkg, R_MEMBERS, REACHER)
    solo = _drive(pkg, hs, 2, between=inject)
    _close(hs)
    plain = _solo(pkg, "reacher", R_MEMBERS, REACHER)
    assert solo[1][0]["buf1"] != plain[1][0]["buf1"] and solo[1][0]["params"] != plain[1][0]["params"]   # the tables were used
    rec, info = _pop_run(pkg, R_MEMBERS, REACHER, between=inject)
    for m in range(3):
        _assert_same(rec[m], solo[m], f"member {m}")
    _assert_same(rec[0], plain[0], "member 0 beside an injected member")
    assert info["total_solo_rollouts"] == 0 and info["total_solo_updates"] == 0 and info["total_rollout_launches"] == 2


def test_an_opt_in_switched_off_between_calls_runs_that_update_alone(pkg):
    """case 6: a member whose update_fused is switched off between two population calls runs that update on the per-step route, alone, is counted, and equals a solo
    handle driven the same way"""
    def off(it, hs):
        if it == 1:
            hs[1].update_fused_enable(False)
    hs = _make(pkg, R_MEMBERS, REACHER)
    solo = _drive(pkg, hs, 2, between=off)
    _close(hs)
    rec, info = _pop_run(pkg, R_MEMBERS, REACHER, between=off)
    for m in range(3):
        _assert_same(rec[m], solo[m], f"member {m}")
    assert info["total_solo_updates"] == 1 and info["last_solo_updates"] == 1 and info["total_solo_rollouts"] == 0 and info["total_update_launches"] == 2


def test_refusals(pkg):
    """case 7: one refusal per line of the join list; each names the member, and every refused handle still trains alone like an untouched twin"""
    capi = pkg._capi
    r = lambda seed=11, **kw: (lambda: _one(pkg, seed, dict(), **{**REACHER, **kw}))
    makers = {"good0": r(11), "good1": r(12), "no macro": r(name="reacher3_fused"), "fused_rollout off": r(rollout=False), "update_fused off": r(update=False),
              "cartpole twin": lambda: _one(pkg, 21, dict(), **CARTPOLE), "scaled": r(scaling=True)}
    hs = {k: mk() for k, mk in makers.items()}
    msg = _refused(pkg, [hs["good0"], hs["no macro"]], capi.ERR_UNSUPPORTED, 1)
    assert "DRIL_ENV_PLUGIN_ROLLOUT_POP" in msg and "dril_env_rollout_pop.h" in msg, msg
    assert "dril_rollout_fused_enable" in _refused(pkg, [hs["good0"], hs["fused_rollout off"]], capi.ERR_UNSUPPORTED, 1)
    assert "dril_update_fused_enable" in _refused(pkg, [hs["good0"], hs["update_fused off"]], capi.ERR_UNSUPPORTED, 1)
    world = pkg.DeviceModuleEnv(_co("rendezvous3"), 6, seed=3)
    hw = world.bind(pkg.PPO(n_steps=13, batch_size=30, epochs=2))
    _refused(pkg, [hw], capi.ERR_UNSUPPORTED, 0)
    _refused(pkg, [hs["good0"], hw], capi.ERR_UNSUPPORTED, 1)
    assert "mixed code objects" in _refused(pkg, [hs["good0"], hs["cartpole twin"]], capi.ERR_INVALID_ARG, 1)
    c = capi.default_config(0)                                                                   # a built-in CartPole handle that is eligible on its own
    for k, v in SHAPE.items():
        setattr(c, k, v)
    builtin = pkg.Handle(c); builtin.set_params(_params(builtin.P, 1)); builtin.env_reset(1)
    assert "mixed members" in _refused(pkg, [hs["good0"], builtin], capi.ERR_INVALID_ARG, 1)
    assert "mixed members" in _refused(pkg, [builtin, hs["good0"]], capi.ERR_INVALID_ARG, 1)
    assert "mixed scaling" in _refused(pkg, [hs["good0"], hs["scaled"]], capi.ERR_INVALID_ARG, 1)
    with pkg.Population([hs["good0"], hs["good1"]]):                                             # the two good ones do join
        pass
    for k, mk in makers.items():                                                                  # every handle was left as it was
        twin = mk()
        _assert_same(_drive(pkg, [hs[k]], 1)[0], _drive(pkg, [twin], 1)[0], f"refused handle '{k}'")
        twin.close(); hs[k].close()
    builtin.close(); hw.close()


def test_evaluation_runs_per_member_and_leaves_nothing_behind(pkg):
    """case 8: Population.evaluate(3) on plug-in members equals evaluate_agent_device per member (they are counted as members that ran alone), and an iteration
    afterwards equals the iteration without the evaluation"""
    solo = _solo(pkg, "reacher", R_MEMBERS, REACHER)
    hs = _make(pkg, R_MEMBERS, REACHER)
    want = [h.evaluate_agent_device(3) for h in hs]
    with pkg.Population(hs) as pop:
        got = pop.evaluate(3)
        assert pop.last_eval_info["solo_members"] == 3 and pop.last_eval_info["batched_members"] == 0
        for m in range(3):
            assert got[m][0] == want[m][0] and _bytes(got[m][1]) == _bytes(want[m][1]) and _bytes(got[m][2]) == _bytes(want[m][2]), m
        rec = _drive(pkg, hs, 1, pop=pop)
    for m in range(3):
        _assert_same(rec[m], solo[m][:1], f"member {m} after an evaluation")
    _close(hs)


def test_train_population_python(pkg):
    """case 9: train_population_(..., fused_update=True) on three agents equals three train_(..., fused_update=True) calls"""
    algs = [pkg.PPO(n_steps=13, batch_size=64, epochs=2), pkg.PPO(n_steps=13, batch_size=64, epochs=2, learning_rate=1e-3, gamma=0.95, ent_coef=0.01),
            pkg.PPO(n_steps=13, batch_size=64, epochs=2, clip_range=0.1)]
    def fresh():
        envs = [pkg.DeviceModuleEnv(_co("reacher3_pop"), 20, seed=80 + i, max_steps=11, fused_rollout=True) for i in range(3)]
        agents = [pkg.Agent(pkg.ActorCriticLayer(envs[i].observation_space(), envs[i].action_space()), algs[i], seed=90 + i) for i in range(3)]
        return agents, envs
    agents_a, envs_a = fresh()
    alone = [pkg.train_(a, e, g, 2 * N, fused_update=True) for a, e, g in zip(agents_a, envs_a, algs)]
    agents_p, envs_p = fresh()
    together = pkg.train_population_(agents_p, envs_p, algs, 2 * N, fused_update=True)
    assert len(together) == 3
    for i in range(3):
        ls_a, ls_p = alone[i][0], together[i][0]
        assert ls_a.keys() == ls_p.keys()
        for k in ls_a:
            if k != "fps":
                assert _bytes(np.asarray(ls_a[k], np.float32)) == _bytes(np.asarray(ls_p[k], np.float32)), (i, k)
        assert len(ls_p["fps"]) == 2 and all(f > 0 for f in ls_p["fps"])
        assert _bytes(pkg.flatten_params(agents_a[i].train_state.parameters)) == _bytes(pkg.flatten_params(agents_p[i].train_state.parameters))
        oa, op = agents_a[i].train_state.optimizer_state, agents_p[i].train_state.optimizer_state
        assert _bytes(oa["m"]) == _bytes(op["m"]) and _bytes(oa["v"]) == _bytes(op["v"]) and oa["steps"] == op["steps"] and oa["beta_powers"] == op["beta_powers"]
        assert agents_a[i].gradient_updates == agents_p[i].gradient_updates == 2 * STEPS and agents_a[i].steps_taken == agents_p[i].steps_taken
    agents_q, envs_q = fresh()
    with pytest.raises(pkg.DrilError, match="dril_update_fused_enable"):                         # without the opt-in the library's refusal comes through
        pkg.train_population_(agents_q, envs_q, algs, 2 * N)
    for e in envs_a + envs_p + envs_q:
        e.handle.close()


def test_lifecycle(pkg):
    """case 10: what the population allocates for plug-in members goes back when it is closed (measured on the second join), and the members' with them"""
    live = lambda: int(pkg._capi.load_library().dril_debug_device_bytes_live())
    base = live()
    hs = _make(pkg, R_MEMBERS[:2], REACHER)
    with pkg.Population(hs) as pop:                                                               # a first round: what the verbs allocate lazily ON the members stays theirs
        pop.collect_rollout(); pop.ppo_update(); pop.evaluate(2)
    before = live()
    pop = pkg.Population(hs)
    assert live() > before
    pop.collect_rollout(); pop.ppo_update(); pop.evaluate(2)
    pop.close()
    assert live() == before
    _close(hs)
    assert live() == base
