"""GPU (-m gpu): populations (dril_population_*, docs/population.md).  A member of a population must be BIT-IDENTICAL to the same handle driven alone: the batched
kernels run the solo kernels' device code on the solo path's own arguments.  Every comparison below is on raw bytes (no tolerance); the yardstick is always a set
of solo handles created with the same configs in the same test and driven with dril_collect_rollout + dril_ppo_update or dril_train."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CARTPOLE, PENDULUM, ACROBOT = 0, 1, 6
SHAPE1 = dict(n_envs=4, n_steps=25, batch_size=24, epochs=3, episode_len=11, monitor_window=10)   # N = 100: a ragged last minibatch of 4
M_PLAIN = dict()
M_OWN = dict(learning_rate=1e-3, clip_range=0.1, ent_coef=0.01, vf_coef=0.7, gamma=0.95, gae_lambda=0.9)
M_NOCLIP = dict(has_max_grad_norm=0, clip_range_vf=0.2, has_clip_range_vf=1)
CASE1 = [(11, M_PLAIN), (12, M_OWN), (13, M_NOCLIP)]                                              # (seed, overrides)


def _cfg(pkg, kind, shape, seed, over, **extra):
    c = pkg._capi.default_config(kind)
    for k, v in {**shape, **over, **extra}.items():
        setattr(c, k, v)
    c.seed = seed
    return c


def _params(P, seed, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(P) * scale).astype(np.float32)


def _make(pkg, kind, shape, members, **extra):
    hs = []
    for seed, over in members:
        h = pkg.Handle(_cfg(pkg, kind, shape, seed, over, **extra))
        h.set_params(_params(h.P, 100 + seed))
        h.env_reset(seed)
        hs.append(h)
    return hs


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _stats(st):
    """every field of dril_ppo_stats as bytes (ten floats, then n_updates, early_stopped, nan_or_inf, f32_path)"""
    return tuple((np.float32 if t is C.c_float else np.int32)(getattr(st, k)).tobytes() for k, t in st._fields_)


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


def _drive(pkg, hs, iters, pop=None, between=None):
    """`iters` iterations of collect + update over the handles: alone, or through the population.  Returns per member the list of per-iteration records."""
    rec = [[] for _ in hs]
    for it in range(iters):
        if between:
            between(it, hs)
        if pop is None:
            for h in hs:
                h.collect_rollout()
        else:
            pop.collect_rollout()
        rolls = [_snap_rollout(pkg, h) for h in hs]
        sts = [h.ppo_update() for h in hs] if pop is None else pop.ppo_update()
        for m, h in enumerate(hs):
            rec[m].append({**rolls[m], **_snap_state(h), "stats": _stats(sts[m])})
    return rec


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for it, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        bad = [k for k in x if x[k] != y[k]]
        assert not bad, f"{what}, iteration {it}: {bad} differ from the solo handle"


def _close(hs):
    for h in hs:
        h.close()


_SOLO = {}


def _solo(pkg, key, kind, shape, members, iters, between=None, **extra):
    """the solo yardstick of a member list, computed once per module and never changed"""
    if key not in _SOLO:
        hs = _make(pkg, kind, shape, members, **extra)
        _SOLO[key] = _drive(pkg, hs, iters, between=between)
        _close(hs)
    return _SOLO[key]


def _pop_run(pkg, kind, shape, members, iters, between=None, check=None, **extra):
    hs = _make(pkg, kind, shape, members, **extra)
    with pkg.Population(hs) as pop:
        rec = _drive(pkg, hs, iters, pop=pop, between=between)
        info = pop.info()
        if check:
            check(pop, hs)
    _close(hs)
    return rec, info


def test_heterogeneous_members_bit_identical(pkg):
    """case 1: three members with their own seeds and run-time hyper-parameters, the monitor on, two iterations; and dril_population_train against dril_train"""
    solo = _solo(pkg, "case1", CARTPOLE, SHAPE1, CASE1, 2)
    rec, info = _pop_run(pkg, CARTPOLE, SHAPE1, CASE1, 2)
    for m in range(3):
        _assert_same(rec[m], solo[m], f"member {m}")
        assert solo[m][0]["stats"] != solo[(m + 1) % 3][0]["stats"]                               # the members really differ
    assert info["members"] == 3 and info["total_solo_rollouts"] == 0 and info["total_solo_updates"] == 0
    assert info["total_rollout_launches"] == 2 and info["total_update_launches"] == 2
    # the train verb: [iteration][member] statistics and the state left behind
    N = SHAPE1["n_envs"] * SHAPE1["n_steps"]
    hs = _make(pkg, CARTPOLE, SHAPE1, CASE1)
    alone = [h.train(2 * N)[0] for h in hs]
    after_alone = [_snap_state(h) for h in hs]
    _close(hs)
    hs = _make(pkg, CARTPOLE, SHAPE1, CASE1)
    with pkg.Population(hs) as pop:
        stats, fps = pop.train(2 * N)
        assert len(stats) == 2 and all(f > 0 for row in fps for f in row)
        for m, h in enumerate(hs):
            assert [_stats(stats[i][m]) for i in range(2)] == [_stats(s) for s in alone[m]]
            assert _snap_state(h) == after_alone[m] == {k: solo[m][1][k] for k in after_alone[m]}
        assert pop.info()["last_launches_per_iteration"] == 2.0
    _close(hs)


@pytest.mark.parametrize("kind,P,shape", [(PENDULUM, 9, dict(n_envs=40, n_steps=16, batch_size=64, epochs=2, episode_len=9)),
                                          (ACROBOT, 2, dict(n_envs=4, n_steps=16, batch_size=16, epochs=2, episode_len=9))], ids=["pendulum-P9-E40", "acrobot-P2"])
def test_two_xcd_groups_and_two_env_tiles(pkg, kind, P, shape):
    """case 2: nine members fill one group of 16 blocks and start a second, 40 envs are two tiles of the rollout grid (Gaussian head, D = 3); Acrobot has D = 6"""
    members = [(20 + m, [M_PLAIN, M_OWN, M_NOCLIP][m % 3]) for m in range(P)]
    hs = _make(pkg, kind, shape, members)
    solo = _drive(pkg, hs, 2)
    _close(hs)
    rec, info = _pop_run(pkg, kind, shape, members, 2)
    for m in range(P):
        _assert_same(rec[m], solo[m], f"member {m}")
    assert info["total_solo_rollouts"] == 0 and info["total_solo_updates"] == 0 and info["total_update_launches"] == 2


def test_members_stop_at_different_steps(pkg, oracle_mod):
    """case 3: one member's target_kl stops its loop strictly inside the update (value picked on the CPU oracle, which runs the same update); the others run to the end"""
    shape = dict(n_envs=4, n_steps=25, batch_size=24, epochs=3, episode_len=11)
    total = 5 * 3
    picked = None
    for tk in [2.0 ** -k for k in range(4, 24)]:
        cfg = _cfg(pkg, CARTPOLE, shape, 31, dict(learning_rate=3e-3, target_kl=tk, has_target_kl=1))
        o = oracle_mod.Oracle(cfg)
        o.set_params(_params(o.P, 131)); o.env_reset(31); o.collect_rollout()
        st = o.ppo_update()
        if st.early_stopped == 1 and 0 < st.n_updates < total:
            if picked is None or abs(st.n_updates - total // 2) < abs(picked[1] - total // 2):
                picked = (tk, st.n_updates)
    assert picked is not None, "no target_kl stops the oracle strictly inside the update"
    members = [(30, M_PLAIN), (31, dict(learning_rate=3e-3, target_kl=picked[0], has_target_kl=1)), (32, M_OWN)]
    hs = _make(pkg, CARTPOLE, shape, members)
    solo = _drive(pkg, hs, 1)
    st = hs[1].get_optimizer_state()
    _close(hs)
    n_upd = [int(np.frombuffer(solo[m][0]["stats"][10], np.int32)[0]) for m in range(3)]
    stopped = [int(np.frombuffer(solo[m][0]["stats"][11], np.int32)[0]) for m in range(3)]
    print(f"[population] target_kl {picked[0]:.3e}: oracle stops after {picked[1]}, the device after {n_upd[1]} of {total}")
    assert 0 < n_upd[1] < total and stopped[1] == 1 and st["steps"] == n_upd[1]                   # on the SOLO handle: the case cannot pass empty
    assert n_upd[0] == n_upd[2] == total and stopped[0] == stopped[2] == 0
    rec, info = _pop_run(pkg, CARTPOLE, shape, members, 1)
    for m in range(3):
        _assert_same(rec[m], solo[m], f"member {m}")
    assert info["total_solo_updates"] == 0


def test_launch_boundaries(pkg, monkeypatch):
    """case 4: at most DRIL_SMALL_CHUNK optimiser steps per launch: 15 steps in launches of 3 equal the one-launch population (and with it the solo handles)"""
    solo = _solo(pkg, "case1", CARTPOLE, SHAPE1, CASE1, 2)
    monkeypatch.setenv("DRIL_DEBUG", "1"); monkeypatch.setenv("DRIL_SMALL_CHUNK", "3")
    rec, info = _pop_run(pkg, CARTPOLE, SHAPE1, CASE1, 2)
    for m in range(3):
        _assert_same(rec[m], solo[m], f"member {m}")
    assert info["total_update_launches"] == 2 * 5 and info["last_update_launches"] == 5


def test_position_and_company_do_not_matter(pkg):
    """case 5: the member (seed 12, its own hyper-parameters) gives the same bytes as member 0 of P = 1, member 2 of P = 3 and member 8 of P = 9"""
    me = CASE1[1]
    solo = _solo(pkg, "case1", CARTPOLE, SHAPE1, CASE1, 2)[1]
    for P in (1, 3, 9):
        members = [(40 + m, [M_PLAIN, M_NOCLIP][m % 2]) for m in range(P - 1)] + [me]
        rec, _ = _pop_run(pkg, CARTPOLE, SHAPE1, members, 2)
        _assert_same(rec[P - 1], solo, f"member {P - 1} of {P}")


CASE6 = CASE1 + [(14, M_OWN), (15, M_PLAIN)]


def test_more_than_one_launch_per_verb(pkg, monkeypatch):
    """case 6: a cap of two members per update launch (debug switch, read at join): five members update in three launches, and nothing else changes"""
    solo = _solo(pkg, "case6", CARTPOLE, SHAPE1, CASE6, 2)
    monkeypatch.setenv("DRIL_DEBUG", "1"); monkeypatch.setenv("DRIL_POP_CAP", "2")
    rec, info = _pop_run(pkg, CARTPOLE, SHAPE1, CASE6, 2)
    for m in range(5):
        _assert_same(rec[m], solo[m], f"member {m}")
    assert info["cap"] == 2 and info["last_update_launches"] == 3 and info["total_update_launches"] == 6
    assert info["last_rollout_launches"] == 0 and info["total_rollout_launches"] == 2           # (the last call was an update; a collection is always one launch)
    assert info["total_solo_updates"] == 0


def test_launch_accounting(pkg):
    """case 7: nine eligible members: one iteration of dril_population_train is one batched rollout launch and one batched update launch, nobody runs alone and
    the members' own rollout / update launch counters (dril_profile_launches) do not move"""
    capi = pkg._capi
    members = [(50 + m, M_PLAIN) for m in range(9)]
    hs = _make(pkg, CARTPOLE, SHAPE1, members, profile_events=1)
    launches = lambda h, k: h.profile()[h.lib.dril_kernel_name(k).decode()]
    def count(h, k):
        n = C.c_int64()
        assert h.lib.dril_profile_launches(h._h, k, C.byref(n)) == 0
        return n.value
    with pkg.Population(hs) as pop:
        before = [(count(h, capi.K_ROLLOUT), count(h, capi.K_PPO_GRAD)) for h in hs]
        stats, _ = pop.train(SHAPE1["n_envs"] * SHAPE1["n_steps"])
        info = pop.info()
        assert len(stats) == 1 and all(s.n_updates == 15 for s in stats[0])
        assert info["cap"] >= 9 and info["last_rollout_launches"] == 1 and info["last_update_launches"] == 1
        assert info["last_solo_rollouts"] == 0 and info["last_solo_updates"] == 0 and info["last_launches_per_iteration"] == 2.0
        assert info["last_rollout_ms"] > 0 and info["last_update_ms"] > 0
        assert [(count(h, capi.K_ROLLOUT), count(h, capi.K_PPO_GRAD)) for h in hs] == before
        assert all(count(h, capi.K_GAE) == 1 for h in hs)                                         # the per-member launches are the members' own
    hs[0].collect_rollout(); hs[0].ppo_update()                                                   # after the population the counters move again
    assert (count(hs[0], capi.K_ROLLOUT), count(hs[0], capi.K_PPO_GRAD)) == (before[0][0] + 1, before[0][1] + 1)
    _close(hs)


def test_injected_noise_and_permutation(pkg):
    """case 8: a member given an injected noise table and an injected DataLoader order equals its solo twin given the same tables; the batched launch carries both
    (they are arguments of the kernels), info reports that nobody ran alone, and the other members are unaffected"""
    N = SHAPE1["n_envs"] * SHAPE1["n_steps"]
    noise = np.random.default_rng(5).random(N)
    perm = np.stack([np.random.default_rng(60 + e).permutation(N) for e in range(SHAPE1["epochs"])]).astype(np.int64)
    def inject(it, hs):
        if it == 0:
            hs[1].set_noise(noise); hs[1].set_permutation(perm)
    hs = _make(pkg, CARTPOLE, SHAPE1, CASE1)
    solo = _drive(pkg, hs, 2, between=inject)
    _close(hs)
    plain = _solo(pkg, "case1", CARTPOLE, SHAPE1, CASE1, 2)
    assert solo[1][0]["buf1"] != plain[1][0]["buf1"] and solo[1][0]["params"] != plain[1][0]["params"]   # the tables were used
    rec, info = _pop_run(pkg, CARTPOLE, SHAPE1, CASE1, 2, between=inject)
    for m in range(3):
        _assert_same(rec[m], solo[m], f"member {m}")
    _assert_same(rec[0], plain[0], "member 0 beside an injected member")
    _assert_same(rec[2], plain[2], "member 2 beside an injected member")
    assert info["total_solo_rollouts"] == 0 and info["total_solo_updates"] == 0 and info["total_rollout_launches"] == 2


def test_verbs_between_calls(pkg):
    """case 9: dril_evaluate_agent_device and dril_policy_from_handle on a member between two population iterations work and leave the next iteration bit-equal to a
    solo run that made the same calls; dril_set_learning_rate on one member between the iterations is honoured"""
    seen = {}
    def between(it, hs):
        if it == 1:
            ev = hs[0].evaluate_agent_device(3, deterministic=True, seed=7)
            pol = pkg.NeuralPolicy.from_handle(hs[2])
            seen.setdefault("eval", []).append((_bytes(np.asarray(ev[1])), _bytes(np.asarray(ev[2]))))
            pol.close()
            hs[1].set_learning_rate(5e-3)
    hs = _make(pkg, CARTPOLE, SHAPE1, CASE1)
    solo = _drive(pkg, hs, 2, between=between)
    _close(hs)
    plain = _solo(pkg, "case1", CARTPOLE, SHAPE1, CASE1, 2)
    assert solo[1][1]["params"] != plain[1][1]["params"]                                          # the new learning rate changed the solo run
    rec, info = _pop_run(pkg, CARTPOLE, SHAPE1, CASE1, 2, between=between)
    for m in range(3):
        _assert_same(rec[m], solo[m], f"member {m}")
    assert seen["eval"][0] == seen["eval"][1] and info["total_solo_updates"] == 0


def _refused(pkg, hs, code, index):
    lib = hs[0].lib if hs and hs[0] is not None else pkg._capi.load_library()
    arr = (C.c_void_p * max(len(hs), 1))(*[None if h is None else h._h for h in hs])
    p = C.c_void_p()
    rc = lib.dril_population_join(arr, len(hs), C.byref(p))
    msg = (lib.dril_population_last_error(None) or b"").decode()
    assert rc == code and not p.value, (rc, msg)
    if index is not None:
        assert f"member {index}:" in msg, msg
    return msg


def test_refusals(pkg, monkeypatch):
    """case 10: one refusal per line of the join list; each names the member, and the refused handles still train alone with unchanged results"""
    capi = pkg._capi
    shape = dict(n_envs=4, n_steps=25, batch_size=24, epochs=3, episode_len=11)
    members = [(11, M_PLAIN), (12, M_OWN)]
    hs = _make(pkg, CARTPOLE, shape, members)
    solo = _drive(pkg, hs, 1)
    _close(hs)
    good = _make(pkg, CARTPOLE, shape, members)
    mk = lambda kind=CARTPOLE, **kw: _make(pkg, kind, {**shape, **kw}, [(70, M_PLAIN)])[0]
    bad = {}
    ext = capi.default_config(capi.ENV_EXTERNAL)
    ext.n_envs, ext.n_steps, ext.batch_size, ext.ext_obs_dim, ext.ext_action_dim, ext.ext_discrete = 4, 25, 24, 4, 2, 1
    bad["external"] = (pkg.Handle(ext), capi.ERR_UNSUPPORTED)
    bad["normalising"] = (mk(norm_obs=1, norm_training=1), capi.ERR_UNSUPPORTED)
    bad["wide net"] = (mk(hidden1=128, hidden2=128), capi.ERR_UNSUPPORTED)
    bad["generic net"] = (mk(hidden1=48, hidden2=48), capi.ERR_UNSUPPORTED)
    bad["batch_size > 64"] = (mk(batch_size=100), capi.ERR_UNSUPPORTED)
    bad["world_size > 1"] = (mk(world_size=2, batch_size=48), capi.ERR_UNSUPPORTED)
    bad["mixed kinds"] = (mk(kind=ACROBOT), capi.ERR_INVALID_ARG)
    bad["mixed shapes"] = (mk(n_steps=20), capi.ERR_INVALID_ARG)
    for what, (h, code) in bad.items():
        msg = _refused(pkg, [good[0], h, good[1]], code, 1)
        print(f"[population] {what}: {msg}")
    plugin = pkg.DeviceModuleEnv(str(__import__("pathlib").Path(__file__).resolve().parents[1] / "examples" / "envs" / "cartpole_plugin.hsaco"), 4, seed=3)
    hp = plugin.bind(pkg.PPO(n_steps=25, batch_size=24, epochs=3))
    _refused(pkg, [good[0], hp], capi.ERR_UNSUPPORTED, 1)
    world = pkg.DeviceModuleEnv(str(__import__("pathlib").Path(__file__).resolve().parents[1] / "examples" / "envs" / "rendezvous3_plugin.hsaco"), 6, seed=3)
    hw = world.bind(pkg.PPO(n_steps=25, batch_size=30, epochs=3))
    _refused(pkg, [hw], capi.ERR_UNSUPPORTED, 0)
    _refused(pkg, [good[0], good[1], good[0]], capi.ERR_INVALID_ARG, 2)                          # the same handle twice
    _refused(pkg, [good[0], None], capi.ERR_INVALID_ARG, 1)                                      # a null entry
    _refused(pkg, [], capi.ERR_INVALID_ARG, None)                                                # n < 1
    ndev = __import__("torch").cuda.device_count()
    if ndev > 1:                                                                                  # mixed devices: needs a second device to create the handle on
        other = mk(device=1)
        _refused(pkg, [good[0], other], capi.ERR_INVALID_ARG, 1)
        other.close()
    with pkg.Population([good[0]]) as pop:
        _refused(pkg, [good[1], good[0]], capi.ERR_INVALID_ARG, 1)                                # a handle already in a population
        rc = good[0].lib.dril_destroy(good[0]._h)                                                 # dril_destroy of a joined member is refused
        assert rc == capi.ERR_INVALID_ARG and "population" in good[0].lib.dril_last_error(good[0]._h).decode()
        with pytest.raises(pkg.DrilError):
            good[0].close()
        assert good[0]._h
    # every refused handle was left as it was: the two good ones train alone, bit-equal to handles that never met a population
    rec = _drive(pkg, good, 1)
    for m in range(2):
        _assert_same(rec[m], solo[m], f"refused handle {m}")
    bad["batch_size > 64"][0].collect_rollout(); assert bad["batch_size > 64"][0].ppo_update().n_updates == 3
    _close(good)                                                                                  # after dril_population_destroy, dril_destroy succeeds
    assert not good[0]._h
    for h, _ in bad.values():
        h.close()
    hp.close(); hw.close()


def test_train_population_python(pkg):
    """case 11: train_population_ on three agents returns per-agent learn_stats equal to three train_ calls, with the copied-back parameters and optimiser state equal"""
    algs = [pkg.PPO(n_steps=25, batch_size=24, epochs=3), pkg.PPO(n_steps=25, batch_size=24, epochs=3, learning_rate=1e-3, gamma=0.95, ent_coef=0.01),
            pkg.PPO(n_steps=25, batch_size=24, epochs=3, clip_range=0.1)]
    def fresh():
        envs = [pkg.DeviceParallelEnv(pkg.CartPoleEnv(), 4, seed=80 + i) for i in range(3)]
        agents = []
        for i in range(3):
            layer = pkg.ActorCriticLayer(pkg.CartPoleEnv().observation_space(), pkg.CartPoleEnv().action_space())
            agents.append(pkg.Agent(layer, algs[i], seed=90 + i))
        return agents, envs
    agents_a, envs_a = fresh()
    alone = [pkg.train_(a, e, g, 200) for a, e, g in zip(agents_a, envs_a, algs)]
    agents_p, envs_p = fresh()
    together = pkg.train_population_(agents_p, envs_p, algs, 200)
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
        assert agents_a[i].gradient_updates == agents_p[i].gradient_updates and agents_a[i].steps_taken == agents_p[i].steps_taken
        assert set(pkg.TIMER_SECTIONS) <= set(together[i][1])
    for e in envs_a + envs_p:
        e.handle.close()
