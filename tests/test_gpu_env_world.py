"""GPU (-m gpu): WORLDS — the multi-agent form of a device env plug-in (include/device/dril_env_world.h, DRIL_ENV_PLUGIN_WORLD): N agents, one shared state, one joint
step, agent i of world w = row w N + i (the stacking of MultiAgentParallelEnv).  The two examples examples/envs/rendezvous3_plugin.hip (N = 3, Box) and
ringmeet4_plugin.hip (N = 4, Discrete) on the device.

Checkers: (1) the NumPy float32 twins of tests/env_world_twins.py; (2) a second handle (bit-identity between batch sizes, between worlds, between ranks); (3) a
DRIL_ENV_EXTERNAL handle fed step by step from a second world handle's env verbs (the construction of
test_reacher3_collection_matches_an_external_handle_fed_from_the_env_verbs).  Shapes: W = 5 (the tail of one workgroup), W = 86 with N = 3 (E = 258: world 85 has rows
255..257, across the observe launch's workgroup boundary), W = 65 with N = 4 (E = 260).  Nothing here tries to make the device fault."""
import ctypes as C

import numpy as np
import pytest

import env_world_twins as tw
import sac_normalize_ref as ref
from env_world_twins import TWINS
from test_gpu_dataparallel import _each
from test_gpu_env_plugin import ALL_BUFS, _cfg, _co, _params
from test_gpu_eval_device import assert_bitwise, assert_equal_runs, snapshot
from test_gpu_traj_device import assert_traj, bits, build, feature_policy, host_loop

pytestmark = pytest.mark.gpu
F = np.float32
TOL = dict(rtol=2e-6, atol=2e-6)           # test_reacher3_physics_matches_the_numpy_twin's: the device may contract a product into an FMA; NumPy rounds every product
NAMES = ["rendezvous3", "ringmeet4"]


def mk(pkg, name, W, T=2, **kw):
    twin = TWINS[name]
    E = W * twin.N
    kw = {**dict(n_envs=E, n_steps=T, batch_size=E * T // 2 if (E * T) % 2 == 0 else E * T, epochs=2, seed=7), **kw}
    return pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, **kw), env_module=_co(name))


def rows(twin, raw):
    """(W, N[, A]) -> the handle's (E,) | (E, A)"""
    return raw.reshape(-1) if twin.discrete else raw.reshape(-1, twin.A)


def words_of(oracle_mod):
    def words(key, episode, block):
        w = np.zeros(4, np.uint32)
        oracle_mod.lib().orc_philox(int(key), int(episode), 0, 0, int(block), w.ctypes.data_as(C.c_void_p))
        return w
    return words


def test_describe_the_two_worlds(pkg):
    r, g, c = (pkg.describe_env_module(_co(n)) for n in ("rendezvous3", "ringmeet4", "cartpole"))
    assert (r["agents"], r["state_dim"], r["obs_dim"], r["action_dim"], r["discrete"], r["episode_len"], r["name"]) == (3, 12, 8, 2, False, 50, "Rendezvous3")
    assert (g["agents"], g["state_dim"], g["obs_dim"], g["action_dim"], g["discrete"], g["episode_len"], g["name"]) == (4, 4, 5, 3, True, 40, "RingMeet4")
    assert c["agents"] == 1 and r["plugin_abi"] == g["plugin_abi"] == c["plugin_abi"] == 1 and not r["obs_declared"]
    h = mk(pkg, "rendezvous3", 5)
    assert h.env_module_agents() == 3 and (h.E, h.D, h.A) == (15, 8, 2)
    assert pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, n_envs=4, n_steps=2, batch_size=8), env_module=_co("reacher3")).env_module_agents() == 1
    env = pkg.DeviceModuleEnv(_co("ringmeet4"), 20)
    assert (env.agents_per_world, env.n_worlds) == (4, 5)
    with pytest.raises(ValueError):
        pkg.DeviceModuleEnv(_co("ringmeet4"), 22)


# ---- 1: the env verbs against the NumPy twin ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_env_verbs_match_the_numpy_twin(pkg, oracle_mod, name):
    twin, W = TWINS[name], tw.VERB_CASES[name]
    N, D, E, L, seed = twin.N, twin.D, tw.VERB_CASES[name] * twin.N, tw.VERB_LIMIT, tw.VERB_ENV_SEED
    words = words_of(oracle_mod)
    exact = twin.discrete                                                      # ringmeet4: integer state, exact throughout
    close = (lambda a, b: np.array_equal(a, b)) if exact else (lambda a, b: np.allclose(a, b, **TOL))
    h = mk(pkg, name, W, episode_len=L)
    h.env_reset(seed)
    st, sc = h.env_get_state()
    assert st.shape == (W, twin.S) and sc.shape == (E,) and not sc.any()
    for w in (0, 1, W - 1):
        assert np.array_equal(st[w], twin.fresh(words, seed + w * N, 0)), w    # world w: key seed0 + w N
    rng = np.random.default_rng(tw.VERB_ACTION_SEED)
    episode = np.zeros(W, np.int64); left_out = n_term = n_trunc = 0
    for t in range(tw.VERB_STEPS):
        obs = h.env_observe()
        assert close(obs, twin.obs(st).reshape(E, D)), t                       # (a row per agent: rows 255..257 of rendezvous3 are one world, in two workgroups)
        raw = tw.raw_actions(twin, rng, W)
        want_st, want_r, want_term = twin.step(st, tw.env_actions(twin, raw))
        rew, term, trunc, tobs = h.env_step(rows(twin, raw))
        got, sc_after = h.env_get_state()
        assert close(rew, want_r.reshape(E)), (t, np.abs(rew - want_r.reshape(E)).max())
        assert (rew.reshape(W, N).std(axis=1) > 0).any()                       # each agent its own reward
        term_w, trunc_w = term.reshape(W, N), trunc.reshape(W, N)
        assert (term_w == term_w[:, :1]).all() and (trunc_w == trunc_w[:, :1]).all()        # the world's flags in all N rows
        edge = twin.near_edge(want_st, tw.EDGE_EPS)                            # the twin within 1e-5 of the termination edge: that world's flag is left out
        left_out += int(edge.sum()) * N
        assert np.array_equal(term_w[~edge, 0], want_term[~edge]), t
        want_trunc = sc.reshape(W, N)[:, 0] + 1 >= L
        assert np.array_equal(trunc_w[:, 0], want_trunc), t
        tr = np.repeat(want_trunc, N)
        assert close(tobs[tr], twin.obs(want_st).reshape(E, D)[tr])            # terminal observations of all N rows of a truncated world
        done = term_w[:, 0] | want_trunc
        assert close(got[~done], want_st[~done])
        for w in np.nonzero(done)[0]:
            episode[w] += 1
            assert np.array_equal(got[w], twin.fresh(words, seed + w * N, episode[w])), (t, w)      # episode k of world w restarts from key seed0 + w N, exactly
        assert (sc_after.reshape(W, N) == sc_after.reshape(W, N)[:, :1]).all() and (sc_after.reshape(W, N)[done] == 0).all()
        n_term += int(term_w[:, 0].sum()); n_trunc += int(want_trunc.sum())
        st, sc = got, sc_after
    assert n_trunc > 0 and (twin.discrete or n_term > 0)
    assert left_out <= tw.LEFT_OUT_CAP * tw.VERB_STEPS * E


# ---- 2: the step is joint within a world, and worlds do not see each other --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_one_agents_action_moves_its_own_world_and_no_other(pkg, name):
    twin, W = TWINS[name], 5
    N, D = twin.N, twin.D
    a, b = mk(pkg, name, W), mk(pkg, name, W)
    a.env_reset(4); b.env_reset(4)
    raw = tw.raw_actions(twin, np.random.default_rng(0), W)
    other = raw.copy()
    if twin.discrete:
        raw[2, 1], other[2, 1] = 2, 1                                           # world 2, agent 1: stay | left
    else:
        raw[2, 1], other[2, 1] = (0.9, -0.9), (-0.9, 0.9)
    ra = a.env_step(rows(twin, raw))[0].reshape(W, N); rb = b.env_step(rows(twin, other))[0].reshape(W, N)
    oa, ob = a.env_observe().reshape(W, N, D), b.env_observe().reshape(W, N, D)
    others = [i for i in range(N) if i != 1]
    assert (ra[2, others] != rb[2, others]).any() and (oa[2, others] != ob[2, others]).any()          # the OTHER agents of the world feel it
    keep = [w for w in range(W) if w != 2]
    assert np.array_equal(bits(ra[keep]), bits(rb[keep])) and np.array_equal(bits(oa[keep]), bits(ob[keep]))
    assert np.array_equal(bits(a.env_get_state()[0][keep]), bits(b.env_get_state()[0][keep]))


# ---- 3: batch invariance ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_a_world_does_not_depend_on_how_many_worlds_there_are(pkg, name):
    twin, W = TWINS[name], tw.VERB_CASES[name]
    N = twin.N
    big, small = mk(pkg, name, W, episode_len=7), mk(pkg, name, 5, episode_len=7)
    big.env_reset(9); small.env_reset(9)
    rng = np.random.default_rng(5)
    n_done = 0
    for t in range(30):
        raw = tw.raw_actions(twin, rng, W)
        assert np.array_equal(bits(big.env_observe()[:5 * N]), bits(small.env_observe())), t
        rb, tb, ub, ob = big.env_step(rows(twin, raw)); rs, ts, us, os_ = small.env_step(rows(twin, raw[:5]))
        assert np.array_equal(bits(rb[:5 * N]), bits(rs)) and np.array_equal(tb[:5 * N], ts) and np.array_equal(ub[:5 * N], us) and np.array_equal(bits(ob[:5 * N]), bits(os_)), t
        (sb, cb), (ss, cs) = big.env_get_state(), small.env_get_state()
        assert np.array_equal(bits(sb[:5]), bits(ss)) and np.array_equal(cb[:5 * N], cs), t
        n_done += int((ts | us).sum())
    assert n_done >= 4 * 5 * N                                                  # with resets: every world restarted at least four times


# ---- 4: the collection against an external handle fed from the env verbs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_collection_matches_an_external_handle_fed_from_the_env_verbs(pkg, name):
    capi = pkg._capi
    twin, W, T, L = TWINS[name], 10, 24, 7
    N, D, A = twin.N, twin.D, twin.A
    E = W * N
    col, sim = mk(pkg, name, W, T, episode_len=L), mk(pkg, name, W, T, episode_len=L)
    ext = pkg.Handle(_cfg(pkg, capi.ENV_EXTERNAL, n_envs=E, n_steps=T, batch_size=E * T // 2, epochs=2, seed=7, ext_obs_dim=D, ext_action_dim=A, ext_discrete=int(twin.discrete),
                          ext_action_low=-1.0, ext_action_high=1.0))
    assert col.P == ext.P
    flat = _params(col.P, 5, 0.3)
    for h in (col, sim, ext):
        h.set_params(flat)
    rng = np.random.default_rng(2)
    nz = rng.random(E * T) if twin.discrete else rng.standard_normal((E * T, A)).astype(F)
    col.env_reset(11); sim.env_reset(11)
    col.set_noise(nz); col.collect_rollout()
    ext.set_noise(nz)
    for t in range(T):
        raw, _ = ext.ext_act(sim.env_observe())
        rew, term, trunc, tobs = sim.env_step(raw)             # the world wrapper applies the adapters itself, per agent
        ext.ext_record(rew, term, trunc, tobs)
    ext.ext_finish(sim.env_observe())
    fl = col.buffer(capi.BUF_FLAGS)
    assert (fl & 2).any() and (twin.discrete or (fl & 1).any())                 # some row truncated; on rendezvous3 some row terminated
    flw = fl.reshape(T, W, N)
    assert (flw == flw[:, :, :1]).all()                                         # the world's flags in all N rows of the buffer
    for which in (capi.BUF_OBSERVATIONS, capi.BUF_ACTIONS, capi.BUF_REWARDS, capi.BUF_FLAGS, capi.BUF_LOGPROBS, capi.BUF_VALUES, capi.BUF_LAST_VALUES):
        assert np.array_equal(col.buffer(which), ext.buffer(which)), which
    tr = (fl & 2) != 0
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
    # a world adds no launch: the collection of a classic plug-in handle with the same net, n_envs and n_steps makes as many
    classic = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=E, n_steps=T, batch_size=E * T // 2, epochs=2, seed=7, episode_len=L), env_module=_co("reacher3"))
    classic.set_params(_params(classic.P, 5, 0.3)); classic.env_reset(11); classic.collect_rollout()
    assert col.rollout_fused_info()["last_collection_launches"] == classic.rollout_fused_info()["last_collection_launches"] > 0


# ---- 5: monitor and evaluation --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_monitor_and_evaluation_work_per_row(pkg, name):
    capi = pkg._capi
    twin, W, T, L = TWINS[name], 5, 40, 6
    N = twin.N
    E = W * N
    h = mk(pkg, name, W, T, episode_len=L, monitor_window=1000)
    h.set_params(_params(h.P, 1, 0.2)); h.env_reset(4); h.collect_rollout()
    rew, fl = h.buffer(capi.BUF_REWARDS).reshape(T, E), h.buffer(capi.BUF_FLAGS).reshape(T, E)
    rets, lens = [], []
    cur_r, cur_l = np.zeros(E, F), np.zeros(E, np.int64)
    for t in range(T):
        cur_r += rew[t]; cur_l += 1
        for e in np.nonzero(fl[t])[0]:
            rets.append(cur_r[e]); lens.append(cur_l[e]); cur_r[e] = 0; cur_l[e] = 0
    r_mean, l_mean, n = h.monitor_stats()
    assert n == len(rets) > E and n % N == 0 and l_mean == pytest.approx(np.mean(lens)) and r_mean == pytest.approx(np.mean(rets), rel=1e-5)
    h.ppo_update()
    for det in (True, False):
        before = snapshot(h, False)
        new = h.evaluate_agent_device(4 * N, det)
        assert_bitwise(before, snapshot(h, False))                              # training state bit-identical before and after
        st, sc = h.env_get_state()
        info = assert_equal_runs(h.evaluate_agent(4 * N, det), new, (name, det))      # the old verb on the same handle (it resets the envs: put them back)
        h.env_set_state(st, sc)
        assert info["path"] == 0
        lengths = new[2].reshape(-1, N)
        assert (lengths == lengths[:, :1]).all() and (lengths <= L).all() and np.isfinite(new[1]).all()       # episodes arrive N at a time, equally long
        assert h.evaluate_agent_device(4 * N, det, persistent=True)[3]["path"] == 0      # no fused evaluation on a world: the request is answered by path 0


# ---- 6: NormalizeWrapperEnv around the rows ---------------------------------------------------------------------------------------------------------------------------
def test_rendezvous3_under_normalize_enable_equals_the_numpy_wrapper_over_a_twin_without_it(pkg):
    """the comparison of test_step_verbs_equal_the_numpy_wrapper_over_a_twin_without_it (tests/test_gpu_env_plugin_normalize.py), its tolerance and keywords"""
    twin, W = TWINS["rendezvous3"], 13
    E = W * twin.N
    kw = dict(norm_obs=1, norm_reward=1, clip_obs=1.25, clip_reward=0.75, gamma=0.9, epsilon=1e-6)
    tol = dict(rtol=3e-5, atol=3e-5)
    h, u = mk(pkg, "rendezvous3", W, 4, episode_len=5), mk(pkg, "rendezvous3", W, 4, episode_len=5)
    h.normalize_enable(**kw)
    w = ref.Wrapper(E, h.D, **kw)
    h.env_reset(11); u.env_reset(11)
    rng = np.random.default_rng(3)
    n_trunc = 0
    for t in range(12):
        raw = u.env_observe()
        got, exp = h.env_observe(), w.observe(raw)
        assert np.allclose(got, exp, **tol), (t, np.abs(got - exp).max())
        assert np.array_equal(h.normalize_get_original()[0], raw)
        act = rows(twin, tw.raw_actions(twin, rng, W))
        ru, tu, uu, ou = u.env_step(act); rh, th, uh, oh = h.env_step(act)
        assert np.array_equal(tu, th) and np.array_equal(uu, uh)
        rn, on = w.act(ru, tu, uu, ou)
        assert np.allclose(rh, rn, **tol), (t, np.abs(rh - rn).max())
        assert np.allclose(oh[uu], on[uu], **tol)
        assert np.array_equal(h.normalize_get_original()[1], ru)
        assert np.allclose(h.normalize_get_returns(), w.returns, **tol)
        n_trunc += int(uu.sum())
    assert n_trunc > 0 and h.normalize_get_stats()["obs_count"] == 12 * E


# ---- 7: trajectories record whole worlds ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("rendezvous3", 1), ("rendezvous3", 2), ("ringmeet4", 1), ("ringmeet4", 2)])
def test_trajectories_of_whole_worlds_equal_a_reconstruction_from_the_env_verbs(pkg, name, k):
    capi = pkg._capi
    twin, W = TWINS[name], 5
    L = 50 if name == "rendezvous3" else 12                                     # rendezvous3: long enough for the policy below to drive every world out of the arena
    N, D = twin.N, twin.D
    M = k * N
    h, sim = mk(pkg, name, W, 4, episode_len=L, monitor_window=20), mk(pkg, name, W, 4, episode_len=L)
    # rendezvous3: every agent pushes along x away from the origin, so the worlds terminate (|x| > 3) before the time limit; ringmeet4: random parameters, truncations
    flat = feature_policy(h, (64, 64), 0, 100.0, (3.0, 0.0)) if name == "rendezvous3" else _params(h.P, 3, 0.5)
    h.set_params(flat); sim.set_params(flat)
    h.env_reset(2); h.collect_rollout()
    before = snapshot(h, False)
    trajs, lengths, flags, info = h.collect_trajectory_device(M, seed=31)
    assert_bitwise(before, snapshot(h, False))                                  # training state is put back
    assert info["path"] == 0 and len(trajs) == M
    assert h.collect_trajectory_device(M, seed=31, persistent=True)[3]["path"] == 0
    bounds = None if twin.discrete else (np.full(twin.A, -1, F), np.full(twin.A, 1, F))
    loop = host_loop(sim, 31, L, bounds)
    lw = lengths.reshape(k, N)
    assert (lw == lw[:, :1]).all() and (flags.reshape(k, N) == flags.reshape(k, N)[:, :1]).all()      # the agents of a world end together
    for m in range(M):
        want = build(loop, m)
        assert flags[m] == want[4] and lengths[m] == len(want[2])
        assert_traj(trajs[m], want, (name, m))                                  # observations, actions, rewards; the terminal observation where truncated
        if flags[m] & capi.TRAJ_TERMINATED:                                     # the terminal state of a terminated world, for every one of its agents: the twin's
            Lm, w = lengths[m], m // N
            after = twin.step(loop["state"][Lm - 1], tw.env_actions(twin, loop["act"][Lm - 1].reshape((W, N) if twin.discrete else (W, N, -1))))[0]
            final = twin.obs(after)[w, m % N]
            assert np.allclose(trajs[m][0][Lm], final, **TOL), (name, m)
    if name == "rendezvous3":
        assert (flags & capi.TRAJ_TERMINATED).any()
    with pytest.raises(pkg.DrilError) as e:
        h.collect_trajectory_device(N + 1, seed=31)
    assert e.value.code == capi.ERR_INVALID_ARG and "multiple of" in str(e.value) and str(N + 1) in str(e.value)
    assert_bitwise(before, snapshot(h, False))


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_status_and_message_leave_the_handle_usable(pkg):
    capi = pkg._capi
    with pytest.raises(pkg.DrilError) as e:
        pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=16, n_steps=2, batch_size=16), env_module=_co("rendezvous3"))
    assert e.value.code == capi.ERR_INVALID_ARG and "16" in str(e.value) and "3" in str(e.value) and "multiple" in str(e.value)
    a, b = mk(pkg, "rendezvous3", 5, 8, episode_len=5), mk(pkg, "rendezvous3", 5, 8, episode_len=5)
    for call in (lambda: a.scaling_enable(True), lambda: a.rollout_fused_enable(True)):
        with pytest.raises(pkg.DrilError) as e:
            call()
        assert e.value.code == capi.ERR_UNSUPPORTED and "world" in str(e.value)
    info = a.evaluate_fused_info()
    assert not info["available"] and "world" in info["reason"]
    assert not a.rollout_fused_info()["available"] and not a.rollout_fused_info()["enabled"]
    from test_gpu_sac_env_plugin import make_module
    with pytest.raises(pkg.DrilError) as e:                                     # SAC on worlds is not built: refused at create, for any row count
        make_module(pkg, _co("rendezvous3"), 6)
    assert e.value.code == capi.ERR_UNSUPPORTED and "world" in str(e.value) and "PPO" in str(e.value)
    flat = _params(a.P, 2, 0.2)
    for h in (a, b):
        h.set_params(flat); h.env_reset(21); h.collect_rollout()
    for which in ALL_BUFS:
        assert np.array_equal(a.buffer(which), b.buffer(which), equal_nan=True), which       # the refused handle collects, with an unchanged result
    with pytest.raises(pkg.DrilError) as e:                                     # the rows of a world share the world's step count
        st, sc = a.env_get_state(); sc[1] += 1; a.env_set_state(st, sc)
    assert e.value.code == capi.ERR_INVALID_ARG and "step count" in str(e.value)


# ---- 9: two loopback ranks ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_two_loopback_ranks_own_the_global_rows(pkg, name):
    """world_size 2: rank 1's W / 2 worlds are worlds W / 2 .. W - 1 of a single handle over W worlds (a world's key is the global row index of its agent 0)"""
    capi = pkg._capi
    twin, W, T = TWINS[name], 8, 12
    N, D = twin.N, twin.D
    E = W * N
    kw = dict(n_steps=T, batch_size=E * T, epochs=1, episode_len=5, seed=9)
    one = pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=E, **kw), env_module=_co(name))
    hs = [pkg.Handle(_cfg(pkg, capi.ENV_MODULE, n_envs=E // 2, rank=r, world_size=2, **kw), env_module=_co(name)) for r in range(2)]
    pkg.Handle.comm_loopback(hs)
    flat = _params(one.P, 2, 0.2)
    one.set_params(flat); one.env_reset(21); one.collect_rollout()
    fields = ((capi.BUF_OBSERVATIONS, D), (capi.BUF_ACTIONS, 1 if twin.discrete else twin.A), (capi.BUF_REWARDS, 1), (capi.BUF_FLAGS, 1))

    def run(r, h):
        h.set_params(flat); h.env_reset(21); h.collect_rollout()
        return {w: h.buffer(w) for w, _ in fields}
    out = _each(hs, run)
    for w, width in fields:
        whole = one.buffer(w).reshape(T, E, width)
        for r in range(2):
            assert np.array_equal(out[r][w].reshape(T, E // 2, width), whole[:, r * (E // 2):(r + 1) * (E // 2)]), (w, r)


# ---- 10: training through the public Python surface ---------------------------------------------------------------------------------------------------------------------
TRAIN_ITERATIONS = 30


def test_rendezvous3_training_improves_the_episode_return(pkg):
    """train_ through the public Python surface: DeviceModuleEnv + MonitorWrapperEnv + Agent — the configuration of examples/ppo_device_world.py 66 30.  One real run
    of it on an MI355X: the mean episode return per agent over the monitor window went from -303.6 after the first rollout to -189.1 after the thirtieth (upwards
    with a noise of about 40 between neighbouring iterations: 22 worlds fill the window); the margin asked for here is 57, half of that improvement of 114.4."""
    env = pkg.MonitorWrapperEnv(pkg.DeviceModuleEnv(_co("rendezvous3"), 66, seed=0), stats_window=66)
    assert env.observation_space().shape == (8,) and env.action_space().shape == (2,)
    alg = pkg.PPO(n_steps=100, batch_size=1650, epochs=10, learning_rate=1e-3)
    agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space()), alg, seed=0)
    seen = []

    class Log:
        def on_rollout_end(self, loc):
            seen.append(loc["env"].handle.monitor_stats()[0]); return True
    pkg.train_(agent, env, alg, 66 * 100 * TRAIN_ITERATIONS, callbacks=[Log()])
    print("rendezvous3 monitor mean per iteration:", [round(float(x), 2) for x in seen])
    assert len(seen) == TRAIN_ITERATIONS and np.isfinite(seen).all()
    assert seen[-1] > seen[0] + TRAIN_MARGIN, (seen[0], seen[-1])


TRAIN_MARGIN = 57.0                         # half of the measured improvement (the docstring above)
