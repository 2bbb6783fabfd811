"""GPU (-m gpu): dril_population_evaluate_device (docs/population.md, "Evaluation").  A member's evaluation inside the batched launches must be BYTE-IDENTICAL to
dril_evaluate_agent_device on the same handle alone, and must leave nothing behind.  Every comparison below is on raw bytes (no tolerance); the yardstick is always
Handle.evaluate_agent_device on a second set of handles created in the same test with the same configs, parameters and resets — the solo verb."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CARTPOLE, PENDULUM, ACROBOT = 0, 1, 6
M_PLAIN = dict()
M_OWN = dict(learning_rate=1e-3, clip_range=0.1, ent_coef=0.01, vf_coef=0.7, gamma=0.95, gae_lambda=0.9)
M_NOCLIP = dict(has_max_grad_norm=0, clip_range_vf=0.2, has_clip_range_vf=1)
MEMBERS = [(11, M_PLAIN), (12, M_OWN), (13, M_NOCLIP)]                                            # (seed, overrides)
PARAM_BASE = 400   # member with seed s holds _params(P, PARAM_BASE + s).  Picked with the SOLO verb so that the CartPole members of test 1 need different numbers of
                   # launches in all six cases (with 100 the deterministic members all finish after the same launch and no member ever sits out with T = 0)


def _shape(n_envs, **kw):
    return {**dict(n_envs=n_envs, n_steps=8, batch_size=16, epochs=2, episode_len=40), **kw}


def _cfg(pkg, kind, shape, seed, over, **extra):
    c = pkg._capi.default_config(kind)
    for k, v in {**shape, **over, **extra}.items():
        setattr(c, k, v)
    c.seed = seed
    return c


def _params(P, seed, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(P) * scale).astype(np.float32)


def _make(pkg, kind, shape, members, base=PARAM_BASE, **extra):
    hs = []
    for seed, over in members:
        h = pkg.Handle(_cfg(pkg, kind, shape, seed, over, **extra))
        h.set_params(_params(h.P, base + seed))
        h.env_reset(seed)
        hs.append(h)
    return hs


def _close(hs):
    for h in hs:
        h.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _res(r):
    """one member's (stats, episode rewards, episode lengths, info) as comparable bytes / ints"""
    stats, er, el, info = r
    return (tuple((k, np.float64(stats[k]).tobytes()) for k in ("mean_reward", "std_reward", "mean_length", "std_length")), int(stats["n_steps"]),
            _bytes(np.asarray(er, np.float32)), _bytes(np.asarray(el, np.int32)), tuple(sorted(info.items())))


def _solo_eval(hs, **kw):
    return [h.evaluate_agent_device(**kw) for h in hs]


def _assert_equal(pop_res, solo_res):
    assert len(pop_res) == len(solo_res)
    for m, (a, b) in enumerate(zip(pop_res, solo_res)):
        ra, rb = _res(a), _res(b)
        bad = [name for name, x, y in zip(("stats", "n_steps", "episode_rewards", "episode_lengths", "member_info"), ra, rb) if x != y]
        assert not bad, f"member {m}: {bad} differ from the solo verb: {a} against {b}"


@pytest.mark.parametrize("n_envs", [4, 33, 129])
@pytest.mark.parametrize("deterministic", [1, 0])
@pytest.mark.parametrize("kind", [CARTPOLE, PENDULUM, ACROBOT], ids=["cartpole", "pendulum", "acrobot"])
def test_equal_to_solo(pkg, kind, deterministic, n_envs):
    """test 1: three members with their own seeds, parameters and hyper-parameters; a poll of 3 steps lets them finish in different launches.  4 envs: one wave with
    28 invalid lanes; 33: a second wave with a single valid env; 129: a second block with one env"""
    kw = dict(n_eval_episodes=10, deterministic=bool(deterministic), poll_steps=3)
    solo_hs = _make(pkg, kind, _shape(n_envs), MEMBERS)
    solo = _solo_eval(solo_hs, **kw)
    _close(solo_hs)
    hs = _make(pkg, kind, _shape(n_envs), MEMBERS)
    with pkg.Population(hs) as pop:
        res = pop.evaluate(**kw)
        info = pop.last_eval_info
    _close(hs)
    print(f"[population eval] kind {kind} det {deterministic} E {n_envs}: steps_enqueued {[r[3]['steps_enqueued'] for r in res]} info {info}")
    _assert_equal(res, solo)
    assert info["batched_members"] == 3 and info["solo_members"] == 0 and info["launches"] == info["looks"]
    assert info["launches"] == max(r[3]["launches"] for r in res)
    assert all(r[3]["path"] == 1 for r in res)
    if kind == CARTPOLE:
        assert len({r[3]["steps_enqueued"] for r in res}) > 1, "every member finished in the same launch: the T = 0 path did not run"


def test_more_episodes_than_envs(pkg):
    """test 2: 37 episodes on 33 envs — several episodes per env, the event list close to n + E K — with the default poll (the default K)"""
    kw = dict(n_eval_episodes=37, deterministic=True)
    solo_hs = _make(pkg, CARTPOLE, _shape(33), MEMBERS)
    solo = _solo_eval(solo_hs, **kw)
    _close(solo_hs)
    hs = _make(pkg, CARTPOLE, _shape(33), MEMBERS)
    with pkg.Population(hs) as pop:
        res = pop.evaluate(**kw)
        info = pop.last_eval_info
    _close(hs)
    print(f"[population eval] 37 episodes on 33 envs: events {[r[3]['events'] for r in res]} steps {[r[3]['steps_enqueued'] for r in res]}")
    _assert_equal(res, solo)
    assert all(r[3]["events"] >= 37 and len(r[1]) == 37 for r in res) and info["batched_members"] == 3


def test_common_seed(pkg):
    """test 3: with seed=123 two members holding identical parameters return identical results, and each equals the solo call with seed=123"""
    members = [(21, M_PLAIN), (22, M_OWN)]
    kw = dict(n_eval_episodes=10, deterministic=False, seed=123, poll_steps=3)
    def make():
        hs = _make(pkg, CARTPOLE, _shape(4), members)
        flat = _params(hs[0].P, 500)
        for h in hs:
            h.set_params(flat)
        return hs
    solo_hs = make()
    solo = _solo_eval(solo_hs, **kw)
    _close(solo_hs)
    hs = make()
    with pkg.Population(hs) as pop:
        res = pop.evaluate(**kw)
        res_own = pop.evaluate(n_eval_episodes=10, deterministic=False, poll_steps=3)             # without the common seed the members' own seeds are in force
    _close(hs)
    _assert_equal(res, solo)
    assert _res(res[0]) == _res(res[1])
    assert _res(res_own[0])[2:4] != _res(res_own[1])[2:4]


def _snap_rollout(pkg, h):
    capi = pkg._capi
    return {f"buf{w}": _bytes(h.buffer(w)) for w in (capi.BUF_OBSERVATIONS, capi.BUF_ACTIONS, capi.BUF_REWARDS, capi.BUF_ADVANTAGES, capi.BUF_RETURNS, capi.BUF_LOGPROBS,
                                                     capi.BUF_VALUES, capi.BUF_FLAGS, capi.BUF_BOOTSTRAP, capi.BUF_LAST_VALUES)}


def _snap_state(h):
    o = h.get_optimizer_state()
    st, sc = h.env_get_state()
    out = {"params": _bytes(h.get_params()), "m": _bytes(o["m"]), "v": _bytes(o["v"]), "beta_powers": _bytes(np.asarray(o["beta_powers"], np.float32)), "steps": o["steps"],
           "env_state": _bytes(st), "env_steps": _bytes(sc), "f32": tuple(sorted(h.f32_fallback_info().items()))}
    if h.cfg.monitor_window > 0:
        out["monitor"] = _bytes(np.asarray(h.monitor_stats(), np.float64))
    return out


def _ppo_stats(st):
    return tuple((np.float32 if t is C.c_float else np.int32)(getattr(st, k)).tobytes() for k, t in st._fields_)


def _train3(pkg, evaluate):
    """three iterations of collect + update through a population; `evaluate`: evaluate() before every iteration, and a sampling evaluation before the third"""
    shape = dict(n_envs=4, n_steps=25, batch_size=24, epochs=3, episode_len=11, monitor_window=10)
    hs = _make(pkg, CARTPOLE, shape, MEMBERS)
    rec = [[] for _ in hs]
    with pkg.Population(hs) as pop:
        for it in range(3):
            if evaluate:
                res = pop.evaluate(n_eval_episodes=5)
                assert all(len(r[1]) == 5 for r in res)
                if it == 2:
                    pop.evaluate(n_eval_episodes=5, deterministic=False)
            pop.collect_rollout()
            rolls = [_snap_rollout(pkg, h) for h in hs]
            sts = pop.ppo_update()
            for m, h in enumerate(hs):
                rec[m].append({**rolls[m], **_snap_state(h), "stats": _ppo_stats(sts[m])})
    _close(hs)
    return rec


def test_nothing_left_behind(pkg):
    """test 4: a population that evaluates before every iteration (and once more, sampling, before the third) trains byte-equal to one that never evaluates"""
    plain, with_eval = _train3(pkg, False), _train3(pkg, True)
    for m in range(3):
        for it in range(3):
            x, y = plain[m][it], with_eval[m][it]
            assert x.keys() == y.keys() and "monitor" in x
            bad = [k for k in x if x[k] != y[k]]
            assert not bad, f"member {m}, iteration {it}: {bad} differ after an evaluation"


def test_member_on_exact_f32_forward(pkg):
    """test 5: a member whose actor's W2 holds a 400 evaluates alone through the solo verb; the others stay in the batch; all three equal their solo handles"""
    kw = dict(n_eval_episodes=10, deterministic=True, poll_steps=3)
    def make():
        hs = _make(pkg, CARTPOLE, _shape(4), MEMBERS)
        flat = hs[1].get_params().copy()
        flat[hs[1].D * 64 + 64 + 5] = 400.0                                                       # one entry of the actor's W2 (flat layout: W1, b1, W2, ...)
        hs[1].set_params(flat)
        assert hs[1].f32_fallback_info()["forward_exact_f32"] == 1
        return hs
    solo_hs = make()
    solo = _solo_eval(solo_hs, **kw)
    _close(solo_hs)
    hs = make()
    with pkg.Population(hs) as pop:
        res = pop.evaluate(**kw)
        info = pop.last_eval_info
    _close(hs)
    _assert_equal(res, solo)
    assert info["solo_members"] == 1 and info["batched_members"] == 2
    assert res[1][3]["path"] == solo[1][3]["path"]


def test_force_step_granular(pkg):
    """test 6: force_step_granular sends every member through the solo verb's step-granular launches (path 0)"""
    kw = dict(n_eval_episodes=6, deterministic=True, poll_steps=3, force_step_granular=True)
    solo_hs = _make(pkg, CARTPOLE, _shape(4), MEMBERS)
    solo = _solo_eval(solo_hs, **kw)
    _close(solo_hs)
    hs = _make(pkg, CARTPOLE, _shape(4), MEMBERS)
    with pkg.Population(hs) as pop:
        res = pop.evaluate(**kw)
        info = pop.last_eval_info
    _close(hs)
    _assert_equal(res, solo)
    assert all(r[3]["path"] == 0 for r in res)
    assert info["solo_members"] == 3 and info["batched_members"] == 0 and info["launches"] == 0 and info["looks"] == 0


def test_refusals(pkg):
    """test 7: n_eval_episodes = 0 and poll_steps = -1 are DRIL_ERR_INVALID_ARG with no member touched; a following valid call equals solo"""
    capi = pkg._capi
    kw = dict(n_eval_episodes=10, deterministic=True, poll_steps=3)
    solo_hs = _make(pkg, CARTPOLE, _shape(4), MEMBERS)
    solo = _solo_eval(solo_hs, **kw)
    _close(solo_hs)
    hs = _make(pkg, CARTPOLE, _shape(4), MEMBERS)
    with pkg.Population(hs) as pop:
        for bad in (dict(n_eval_episodes=0), dict(n_eval_episodes=10, poll_steps=-1)):
            with pytest.raises(pkg.DrilError) as e:
                pop.evaluate(**bad)
            assert e.value.code == capi.ERR_INVALID_ARG, e.value
            _assert_equal(pop.evaluate(**kw), solo)
        o = capi.DrilEvalOptions()
        assert pop.lib.dril_eval_options_default(C.byref(o)) == 0
        st = (capi.DrilEvalStats * 3)()
        assert pop.lib.dril_population_evaluate_device(pop._p, None, st, None, None, None, None) == capi.ERR_INVALID_ARG      # null options
        assert pop.lib.dril_population_evaluate_device(pop._p, C.byref(o), None, None, None, None, None) == capi.ERR_INVALID_ARG   # null out
        assert pop.lib.dril_population_evaluate_device(None, C.byref(o), st, None, None, None, None) == capi.ERR_INVALID_ARG  # null population
        assert pop.lib.dril_population_evaluate_device(pop._p, C.byref(o), st, None, None, None, None) == 0                  # every optional output may be NULL
        _assert_equal(pop.evaluate(**kw), solo)
    _close(hs)


def test_python_forms(pkg):
    """test 8: evaluate_population(agents, envs) returns per agent what evaluate_agent(agent, env, isolated=True) returns (the floats compared as bytes), and
    train_population_ afterwards equals training without the evaluation"""
    algs = [pkg.PPO(n_steps=25, batch_size=24, epochs=3), pkg.PPO(n_steps=25, batch_size=24, epochs=3, learning_rate=1e-3, gamma=0.95, ent_coef=0.01),
            pkg.PPO(n_steps=25, batch_size=24, epochs=3, clip_range=0.1)]
    def fresh():
        envs = [pkg.DeviceParallelEnv(pkg.CartPoleEnv(), 4, seed=80 + i) for i in range(3)]
        agents = []
        for i in range(3):
            layer = pkg.ActorCriticLayer(pkg.CartPoleEnv().observation_space(), pkg.CartPoleEnv().action_space())
            agents.append(pkg.Agent(layer, algs[i], seed=90 + i))
        return agents, envs
    keys = ("mean_reward", "std_reward", "mean_length", "std_length")
    as_bytes = lambda d: tuple((k, np.float64(d[k]).tobytes()) for k in keys)
    agents_a, envs_a = fresh()
    alone = [pkg.evaluate_agent(a, e, isolated=True) for a, e in zip(agents_a, envs_a)]
    agents_p, envs_p = fresh()
    together = pkg.evaluate_population(agents_p, envs_p)
    assert len(together) == 3 and all(tuple(d) == keys for d in together)
    assert [as_bytes(d) for d in together] == [as_bytes(d) for d in alone]
    assert len({as_bytes(d) for d in together}) > 1                                               # the agents really differ
    # training afterwards: the evaluated population against one that never evaluated
    agents_n, envs_n = fresh()
    trained_n = pkg.train_population_(agents_n, envs_n, algs, 200)
    trained_p = pkg.train_population_(agents_p, envs_p, algs, 200)
    for i in range(3):
        for k in trained_n[i][0]:
            if k != "fps":
                assert _bytes(np.asarray(trained_n[i][0][k], np.float32)) == _bytes(np.asarray(trained_p[i][0][k], np.float32)), (i, k)
        assert _bytes(pkg.flatten_params(agents_n[i].train_state.parameters)) == _bytes(pkg.flatten_params(agents_p[i].train_state.parameters))
    # handles already joined: through the caller's population
    hs = [e.handle for e in envs_p]
    with pkg.Population(hs) as pop:
        again = pkg.evaluate_population(agents_p, envs_p, population=pop)
        each = [pkg.evaluate_agent(a, e, isolated=True) for a, e in zip(agents_p, envs_p)]
        assert [as_bytes(d) for d in again] == [as_bytes(d) for d in each]
    for e in envs_a + envs_p + envs_n:
        e.handle.close()
