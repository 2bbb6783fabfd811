"""GPU (-m gpu): path 2 of dril_evaluate_agent_device / dril_collect_trajectory_device — the fused evaluation kernel of a device env plug-in
(include/device/dril_env_evaluate.h), K env steps per launch and one library launch over the rows it leaves.

Yardsticks: (a) the fused rollout of the same code object (merged and oracle-checked): a stochastic path-2 evaluation must reproduce, bit for bit, the episodes formed
on the host from BUF_REWARDS / BUF_FLAGS of a fused collection after the same reset; (b) path 0 on the same handle — another f32-equivalent arithmetic of the actor, so
the rule of test_fused_matches_the_step_granular_collection holds: envs whose lengths or end flags differ are left out, at most 2 % of them, each explained by a
boundary within 1e-5 (reacher3) or a logit near-tie below 1e-4 (cartpole); (c) the env verbs of a plain twin replaying the recorded actions.
Nothing here tries to make the device fault: every refusal is a host-side check made before anything is launched."""
import threading

import numpy as np
import pytest

import fused_evaluate_helpers as V
from test_gpu_env_plugin import _reacher_step
from test_gpu_env_plugin_fused import _cfg, _co, _params
from test_gpu_eval_device import assert_bitwise, snapshot, stats_equal

pytestmark = pytest.mark.gpu
f32 = np.float32
K_DEFAULT = 64                                                                 # kEvalPollPersistent (dril_eval.hip)


def _make(pkg, name, E, L, scaling=False, hidden=None, **kw):
    c = dict(n_envs=E, n_steps=kw.pop("n_steps", 4), episode_len=L, **kw)
    c.setdefault("batch_size", E * c["n_steps"])
    if hidden is not None:
        c["hidden"] = hidden
    h = pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, **c), env_module=_co(name))
    if scaling:
        h.scaling_enable(True)
    return h


# ---- 1: the path is taken where the kernel is, and nowhere else (fails without the feature) ---------------------------------------------------------------------
@pytest.mark.parametrize("name,scaling", [("cartpole_eval", False), ("pendulum_eval", True), ("reacher3_eval", False)])
def test_the_request_reaches_path_2_with_two_launches_per_k_steps(pkg, name, scaling):
    E, L = 37, 13
    h = _make(pkg, name, E, L, scaling)
    h.set_params(_params(h.P, 5, 0.3)); h.env_reset(11)
    info = h.evaluate_fused_info()
    assert info["available"] and info["reason"] == "" and (info["tile"], info["threads"], info["max_width"]) == (16, 256, 256)
    for k in (0, 1, 7):
        K = k or min(K_DEFAULT, L)
        *_, ei = h.evaluate_agent_device(E, True, poll_steps=k, persistent=True)
        assert ei["path"] == 2 and ei["steps_enqueued"] % K == 0 and ei["launches"] == 2 * ei["steps_enqueued"] // K, (k, ei)
        *_, ti = h.collect_trajectory_device(E, poll_steps=k, persistent=True)
        assert ti["path"] == 2 and ti["launches"] == 2 * -(-ti["steps_enqueued"] // K) and ti["steps_enqueued"] <= L, (k, ti)
    assert h.evaluate_agent_device(E, True)[3]["path"] == 0 and h.collect_trajectory_device(E)[3]["path"] == 0                       # without the request: as ever
    assert h.evaluate_agent_device(E, True, force_step_granular=True, persistent=True)[3]["path"] == 0                                 # force_step_granular wins


@pytest.mark.parametrize("name", ["reacher3", "reacher3_fused"])
def test_code_objects_without_the_kernel_answer_as_before(pkg, name):
    h = _make(pkg, name, 24, 13)
    h.set_params(_params(h.P, 5, 0.3)); h.env_reset(11)
    info = h.evaluate_fused_info()
    assert not info["available"] and "DRIL_ENV_PLUGIN_EVALUATE" in info["reason"] and info["tile"] == 0
    want = h.evaluate_agent_device(30, True)
    got = h.evaluate_agent_device(30, True, persistent=True)
    assert got[3]["path"] == 0 and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert h.collect_trajectory_device(5, persistent=True)[3]["path"] == 0


# ---- 2: the exact yardstick: the fused rollout's rewards and flags --------------------------------------------------------------------------------------------
def _host_episodes(rew, fl, n_eval):
    """evaluation.jl:95-121 on the rows of a collection: float32 sums in step order, episodes in (step, env) order"""
    T, E = rew.shape
    cur_r, cur_l, er, el = np.zeros(E, f32), np.zeros(E, np.int64), [], []
    for t in range(T):
        cur_r += rew[t]; cur_l += 1
        for e in np.flatnonzero(fl[t]):
            er.append(cur_r[e]); el.append(cur_l[e]); cur_r[e] = 0; cur_l[e] = 0
    assert len(er) >= n_eval
    return np.asarray(er[:n_eval], f32), np.asarray(el[:n_eval], np.int32)


@pytest.mark.parametrize("name,scaling", [("cartpole_eval", False), ("pendulum_eval", True), ("reacher3_eval", False)])
def test_stochastic_episodes_equal_those_of_a_fused_collection_bitwise(pkg, name, scaling):
    capi = pkg._capi
    E, L = 37, 13
    T = 3 * L
    h = _make(pkg, name, E, L, scaling)
    twin = _make(pkg, name, E, L, scaling, n_steps=T)
    twin.rollout_fused_enable(True)
    flat = _params(h.P, 5, 0.3)
    for x in (h, twin):
        x.set_params(flat); x.env_reset(11)
    twin.env_reset(23); twin.collect_rollout()                                # the collection runs after env_reset with the evaluation's seed
    rew, fl = twin.buffer(capi.BUF_REWARDS).reshape(T, E), twin.buffer(capi.BUF_FLAGS).reshape(T, E)
    for n in (E, 3 * E // 2):
        want_r, want_l = _host_episodes(rew, fl, n)
        for k in (1, 7, 0):
            st, er, el, info = h.evaluate_agent_device(n, False, seed=23, poll_steps=k, persistent=True)
            assert info["path"] == 2
            assert np.array_equal(er.view(np.uint32), want_r.view(np.uint32)) and np.array_equal(el, want_l), (name, n, k)
    # independence of E: envs [16, 24) alone, seeded with their global indices
    part = _make(pkg, name, 8, L, scaling)
    part.set_params(flat); part.env_reset(1)
    want_r, want_l = _host_episodes(rew[:, 16:24], fl[:, 16:24], 12)
    _, er, el, info = part.evaluate_agent_device(12, False, seed=23 + 16, persistent=True)
    assert info["path"] == 2 and np.array_equal(er.view(np.uint32), want_r.view(np.uint32)) and np.array_equal(el, want_l)


# ---- 3: against path 0 on the same handle ------------------------------------------------------------------------------------------------------------------------
def _compare_paths(pkg, h, name, ref, got, flat, hidden=(64, 64)):
    """rule 3 of the issue on two recordings (trajs, lengths, flags) of the same handle: path 0 (ref) is the yardstick"""
    (tr, lr, fr), (tg, lg, fg) = ref, got
    E = len(lr)
    same = (lr == lg) & (fr == fg)
    print(f"[{name}] envs left out: {(~same).sum()} of {E}")
    assert (~same).mean() <= 0.02, f"{(~same).sum()} of {E} envs differ in length or end flags"
    for e in np.flatnonzero(~same):
        (o0, a0, _), (o2, a2, _) = tr[e], tg[e]
        n = min(lr[e], lg[e])
        d = [t for t in range(n) if not (np.allclose(o0[t], o2[t], atol=2e-5, rtol=2e-5) and np.allclose(a0[t], a2[t], atol=5e-5, rtol=5e-5))]
        t = d[0] if d else n - 1                                               # the first differing step: the step at which the shorter one ended
        if name.startswith("reacher3"):
            pos = _reacher_step(o2[t:t + 1, :9], a2[t:t + 1])[0][0, :3]
            assert np.abs(np.abs(pos) - 2).min() < 1e-5, (e, t, pos)
        else:
            z = np.sort(V.actor_forward(flat, 4, hidden, 2, 0, o2[t:t + 1]), axis=1)[0]
            assert z[-1] - z[-2] < 1e-4, (e, t, z)
    worst = [0.0, 0.0, 0.0]
    for e in np.flatnonzero(same):
        (o0, a0, r0), (o2, a2, r2) = tr[e], tg[e]
        np.testing.assert_allclose(o2, o0, atol=2e-5, rtol=2e-5); np.testing.assert_allclose(r2, r0, atol=1e-4, rtol=1e-4)
        np.testing.assert_allclose(np.asarray(a2, np.float64), np.asarray(a0, np.float64), atol=5e-5, rtol=5e-5)
        worst = [max(worst[0], np.abs(o2 - o0).max()), max(worst[1], np.abs(r2 - r0).max()), max(worst[2], np.abs(np.asarray(a2, np.float64) - a0).max())]
    print(f"[{name}] max |diff| observations {worst[0]:.3e} rewards {worst[1]:.3e} actions {worst[2]:.3e}")
    return same


@pytest.mark.parametrize("name,L", [("reacher3_eval", 13), ("reacher3_eval", 40), ("cartpole_eval", 60)])
@pytest.mark.parametrize("det", [True, False])
def test_recordings_match_path_0_on_the_same_handle(pkg, name, L, det):
    """collect_trajectory with M = E = 256 on both paths of one handle.  Both verbs bring their own reset!(env), so a start at |p| = 1.9 cannot be handed to them: from
    reacher3's own reset (|p| <= 0.5, v = 0) no env can reach the +-2 boundary within 13 steps (13 steps of full push move it by 0.72), so the L = 13 case holds
    truncated episodes only, and the terminated ones — with the check of their final row — come from the same env at L = 40 and from cartpole, whose time limit is set to the median episode length of the yardstick path so that both kinds of ending occur"""
    capi = pkg._capi
    E = 256
    h = _make(pkg, name, E, L)
    flat = _params(h.P, 5, 0.3)
    h.set_params(flat); h.env_reset(11)
    if name.startswith("cartpole"):                                            # a time limit at the median of the yardstick's own episode lengths: poles that fall before it, and poles cut by it
        L = max(2, int(np.median(h.collect_trajectory_device(E, deterministic=det, seed=31)[1])))
        h = _make(pkg, name, E, L)
        h.set_params(flat); h.env_reset(11)
    ref = h.collect_trajectory_device(E, deterministic=det, seed=31)
    got = h.collect_trajectory_device(E, deterministic=det, seed=31, persistent=True)
    assert ref[3]["path"] == 0 and got[3]["path"] == 2
    same = _compare_paths(pkg, h, name, ref[:3], got[:3], flat)
    fl = got[2][same]
    assert (fl & capi.TRAJ_TRUNCATED).any(), "no truncated env among the recorded ones"
    if L == 13:
        assert not (fl & capi.TRAJ_TERMINATED).any()                           # (see above: not reachable)
        return
    assert (fl & capi.TRAJ_TERMINATED).any(), "no terminated env among the recorded ones"
    # the final row of a terminated episode: a fixed_length_episodes twin (it masks the termination and nothing else) stepped once from the recorded state
    twin = _make(pkg, name, E, L, fixed_length_episodes=1)
    twin.set_params(flat); twin.env_reset(31)
    term = np.flatnonzero((got[2] & capi.TRAJ_TERMINATED) != 0)[:8]
    S = twin.env_get_state()[0].shape[1]
    for e in term:
        o, a, _ = got[0][e]
        n = got[1][e]
        st, sc = twin.env_get_state()
        st[e] = o[n - 1][:S]; sc[:] = 0                                         # reacher3 / cartpole: the state is the observation's first S entries
        twin.env_set_state(st, sc)
        act = np.zeros((E,) + a.shape[1:], a.dtype) + (1 if name.startswith("cartpole") else 0)
        act[e] = a[n - 1]
        twin.env_step(act)
        np.testing.assert_allclose(twin.env_observe()[e], o[n], atol=2e-6, rtol=2e-6)


# ---- 4: replay -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scaling", [("reacher3_eval", False), ("cartpole_eval", False), ("pendulum_eval", True)])
def test_recorded_actions_replayed_through_the_env_verbs(pkg, name, scaling):
    """a plain twin (no scaling: the recording holds original observations and the actions the physics received) stepped with the recorded actions"""
    capi = pkg._capi
    E, L = 37, 13
    h = _make(pkg, name, E, L, scaling)
    h.set_params(_params(h.P, 5, 0.3)); h.env_reset(1)
    trajs, lengths, flags, info = h.collect_trajectory_device(E, seed=31, persistent=True, final_original=True)
    assert info["path"] == 2
    plain = _make(pkg, name, E, L)
    plain.env_reset(31)
    np.testing.assert_allclose(plain.env_observe(), np.stack([t[0][0] for t in trajs]), atol=2e-6, rtol=2e-6)
    alive = np.ones(E, bool)
    for t in range(int(lengths.max())):
        a0 = trajs[0][1]
        act = np.zeros((E,) + a0.shape[1:], a0.dtype) + (1 if h.discrete else 0)
        for e in np.flatnonzero(alive):
            act[e] = trajs[e][1][t]
        rew, term, trunc, _ = plain.env_step(act)
        nxt = plain.env_observe()
        for e in np.flatnonzero(alive):
            np.testing.assert_allclose(rew[e], trajs[e][2][t], atol=2e-6, rtol=2e-6)
            done = bool(term[e] or trunc[e])
            assert done == (t + 1 == lengths[e]), (e, t)
            if done:
                assert flags[e] == (int(term[e]) | int(trunc[e]) << 1)
                alive[e] = False
            else:
                np.testing.assert_allclose(nxt[e], trajs[e][0][t + 1], atol=2e-6, rtol=2e-6)
    assert not alive.any()


# ---- 5: the frozen normaliser ---------------------------------------------------------------------------------------------------------------------------------------
def test_frozen_normaliser_is_read_and_left_alone(pkg):
    E, L = 256, 13
    h = _make(pkg, "reacher3_eval", E, L, n_steps=8)
    h.normalize_enable(clip_obs=1.25, clip_reward=0.75, gamma=0.9, epsilon=1e-6)
    flat = _params(h.P, 5, 0.3)
    h.set_params(flat); h.env_reset(4); h.collect_rollout()                     # one training collection: statistics with mean != 0 and var != 1
    before = (h.normalize_get_stats(), h.normalize_get_returns(), h.normalize_config())
    assert np.abs(before[0]["obs_mean"]).min() > 0 and np.abs(before[0]["obs_var"] - 1).min() > 0 and before[2]["training"] is True
    ref = h.collect_trajectory_device(E, seed=31)
    got = h.collect_trajectory_device(E, seed=31, persistent=True)
    assert ref[3]["path"] == 0 and got[3]["path"] == 2
    raw = np.concatenate([t[0][:-1] for t in got[0]])                           # the clip bites on what the actor saw
    z = (raw - before[0]["obs_mean"]) / np.sqrt(before[0]["obs_var"] + f32(1e-6))
    assert (np.abs(z) > 1.25).any() and (np.abs(z) < 1.25).any()
    _compare_paths(pkg, h, "reacher3_eval", ref[:3], got[:3], flat)
    ev2 = h.evaluate_agent_device(E, True, seed=31, persistent=True)         # raw returns (the rule for plug-ins): the sums of the recorded raw rewards
    assert ev2[3]["path"] == 2
    order = np.argsort(got[1], kind="stable")                                  # every env ends once within L: (step, env) order
    want = np.asarray([np.add.accumulate(got[0][e][2].astype(f32), dtype=f32)[-1] for e in order], f32)
    assert np.array_equal(ev2[2], got[1][order]) and np.array_equal(ev2[1].view(np.uint32), want.view(np.uint32))
    after = (h.normalize_get_stats(), h.normalize_get_returns(), h.normalize_config())
    assert stats_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and after[2]["training"] is True
    # statistics (0, 1) and a clip that never bites: the un-normalised path 2, bit for bit
    ident = _make(pkg, "reacher3_eval", E, L)
    ident.normalize_enable(clip_obs=1e9, clip_reward=1e9, gamma=0.9, epsilon=1e-8)
    plain = _make(pkg, "reacher3_eval", E, L)
    outs = []
    for x in (ident, plain):
        x.set_params(flat); x.env_reset(4)
        outs.append(x.collect_trajectory_device(E, seed=31, persistent=True))
        assert outs[-1][3]["path"] == 2
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    for (o0, a0, r0), (o1, a1, r1) in zip(outs[0][0], outs[1][0]):
        assert np.array_equal(o0.view(np.uint32), o1.view(np.uint32)) and np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(r0.view(np.uint32), r1.view(np.uint32))


# ---- 6: isolation ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalised", [False, True])
def test_path_2_between_training_iterations_changes_nothing(pkg, normalised):
    E = 24
    kw = dict(monitor_window=30, epochs=2, seed=5, n_steps=16, batch_size=96)

    def mk():
        h = _make(pkg, "reacher3_eval", E, 12, **kw)
        if normalised:
            h.normalize_enable(clip_obs=1.25, clip_reward=0.75, gamma=0.9, epsilon=1e-6)
        return h
    a, b = mk(), mk()
    flat = _params(a.P, 21, 0.2)
    calls = []

    def visit(h):
        for det in (True, False):
            calls.append(h.evaluate_agent_device(7, det, seed=1000 + len(calls), persistent=True)[3]["path"])
            calls.append(h.collect_trajectory_device(5, deterministic=det, seed=1000 + len(calls), persistent=True)[3]["path"])

    def snap(h):
        s = snapshot(h, False)
        if normalised:
            s["pn"] = (h.normalize_get_stats(), h.normalize_get_returns(), h.normalize_get_original(), h.normalize_config())
        return s

    def check(x, y):
        assert_bitwise(x, y)
        if normalised:
            assert stats_equal(x["pn"][0], y["pn"][0]) and np.array_equal(x["pn"][1], y["pn"][1]) and x["pn"][3] == y["pn"][3]
            assert all(np.array_equal(p, q) for p, q in zip(x["pn"][2], y["pn"][2]))
    for h, with_calls in ((a, False), (b, True)):
        h.set_params(flat); h.env_reset(13)
        if with_calls:
            visit(h)
        for _ in range(2):
            h.collect_rollout(); h.ppo_update()
            if with_calls:
                visit(h)
    assert len(calls) == 12 and set(calls) == {2}
    assert a.monitor_stats()[2] > 0
    check(snap(a), snap(b))
    a.collect_rollout(); b.collect_rollout(); a.ppo_update(); b.ppo_update()    # and what follows is the same too
    check(snap(a), snap(b))


def test_a_never_reset_handle_and_two_loopback_ranks(pkg):
    capi = pkg._capi
    E, L = 24, 13
    h = _make(pkg, "reacher3_eval", E, L)
    ref = _make(pkg, "reacher3_eval", E, L)
    flat = _params(h.P, 5, 0.3)
    h.set_params(flat); ref.set_params(flat); ref.env_reset(3)
    want = ref.evaluate_agent_device(30, False, persistent=True)
    got = h.evaluate_agent_device(30, False, seed=3, persistent=True)
    assert got[3]["path"] == 2 and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert h.collect_trajectory_device(3, seed=3, persistent=True)[3]["path"] == 2
    with pytest.raises(pkg.DrilError) as e:
        h.collect_rollout()
    assert e.value.code == capi.ERR_NOT_INITIALISED and "before dril_env_reset" in str(e.value)
    hs = [_make(pkg, "reacher3_eval", E, L, rank=r, world_size=2, batch_size=2 * E, seed=11) for r in range(2)]
    pkg.Handle.comm_loopback(hs)
    out, err = [None, None], [None, None]

    def run(r):
        try:
            hs[r].set_params(flat); hs[r].env_reset(21)
            calls = hs[r].comm_allreduce_calls()
            res = (hs[r].evaluate_agent_device(30, False, persistent=True), hs[r].collect_trajectory_device(E, deterministic=False, persistent=True))
            out[r] = (res, hs[r].comm_allreduce_calls() - calls)
        except BaseException as ex:   # noqa: BLE001 - re-raised below
            err[r] = ex
    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in ts]; [t.join() for t in ts]
    for ex in err:
        if ex is not None:
            raise ex
    for r in range(2):
        (ev, tj), calls = out[r]
        assert calls == 0 and ev[3]["path"] == 2 and tj[3]["path"] == 2
        one = _make(pkg, "reacher3_eval", E, L, seed=11)                       # the same global env indices in a handle of its own
        one.set_params(flat); one.env_reset(21 + r * E)
        w_ev, w_tj = one.evaluate_agent_device(30, False, persistent=True), one.collect_trajectory_device(E, deterministic=False, persistent=True)
        assert np.array_equal(ev[1], w_ev[1]) and np.array_equal(ev[2], w_ev[2])
        assert np.array_equal(tj[1], w_tj[1]) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(tj[0], w_tj[0]))


# ---- 7: further checks ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_max_steps_final_original_and_independence_of_m(pkg):
    capi = pkg._capi
    E, L = 64, 13
    h = _make(pkg, "pendulum_eval", E, L, scaling=True)
    h.set_params(_params(h.P, 5, 0.3)); h.env_reset(1)
    full = {}
    for max_steps in (1, 5, None):
        for final in (False, True):
            trajs, lengths, flags, info = h.collect_trajectory_device(E, max_steps, seed=31, final_original=final, persistent=True)
            assert info["path"] == 2 and info["capacity"] == (max_steps or L) and info["steps_enqueued"] <= info["capacity"]
            assert (lengths == (max_steps or L)).all() and (flags == (capi.TRAJ_MAX_STEPS if max_steps else capi.TRAJ_TRUNCATED)).all()   # Pendulum never terminates
            full[max_steps, final] = trajs
            for M in (1, 37):
                part, pl, pf, _ = h.collect_trajectory_device(M, max_steps, seed=31, final_original=final, persistent=True)
                assert np.array_equal(pl, lengths[:M]) and np.array_equal(pf, flags[:M])
                assert all(np.array_equal(x[i], y[i]) for x, y in zip(part, trajs) for i in range(3)), (max_steps, final, M)
        a, b = full[max_steps, False], full[max_steps, True]
        lo, hi = h.env_module_obs_space()["low"], h.env_module_obs_space()["high"]
        for (o0, a0, r0), (o1, a1, r1) in zip(a, b):                           # final_original unscales the last row and nothing else
            assert np.array_equal(o0[:-1], o1[:-1]) and np.array_equal(a0, a1) and np.array_equal(r0, r1)
            np.testing.assert_allclose(o1[-1], (o0[-1] + 1) * (hi - lo) / 2 + lo, atol=2e-6, rtol=2e-6)
            assert np.abs(o0[-1]).max() <= 1 + 1e-6
    for t5, tn in zip(full[5, False], full[None, False]):                      # a cut trajectory is the prefix of the uncut one
        assert np.array_equal(t5[0][:5], tn[0][:5]) and np.array_equal(t5[1], tn[1][:5]) and np.array_equal(t5[2], tn[2][:5])


def test_info_verb_reasons_and_the_python_mirror(pkg):
    capi = pkg._capi
    builtin = pkg.Handle(_cfg(pkg, 0, n_envs=8, n_steps=4, batch_size=32))
    info = builtin.evaluate_fused_info()
    assert not info["available"] and "device env plug-in" in info["reason"]
    builtin.env_reset(1)
    assert builtin.evaluate_agent_device(4, True, persistent=True)[3]["path"] == 1        # a built-in kind keeps its own persistent kernel
    wide = _make(pkg, "reacher3_eval", 8, 13, hidden=(300, 64))
    info = wide.evaluate_fused_info()
    assert not info["available"] and "300" in info["reason"] and "DRIL_ENV_ROLLOUT_MAX_WIDTH" in info["reason"] and info["max_width"] == 256
    wide.set_params(_params(wide.P, 5, 0.1)); wide.env_reset(1)
    assert wide.evaluate_agent_device(4, True, persistent=True)[3]["path"] == 0           # path 0, never an error
    disc = _make(pkg, "cartpole_eval", 8, 13)
    with pytest.raises(pkg.DrilError) as e:
        disc.scaling_enable(True)
    assert e.value.code == capi.ERR_UNSUPPORTED


def test_python_mirror(pkg):
    """evaluate_agent / collect_trajectory with persistent=True on a device plug-in env return what the handle's verbs return on path 2"""
    env = pkg.host.DeviceModuleEnv(_co("reacher3_eval"), 16, seed=3)
    agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space()), pkg.PPO(n_steps=16, batch_size=128, epochs=1), seed=0)
    h = env.bind(agent.alg, agent.layer)
    assert h.evaluate_fused_info()["available"]
    obs, act, rew = pkg.collect_trajectory(agent, env, seed=9, persistent=True)
    trajs, _, _, info = h.collect_trajectory_device(1, seed=9, persistent=True)
    assert info["path"] == 2 and np.array_equal(obs, trajs[0][0]) and np.array_equal(act, trajs[0][1]) and np.array_equal(rew, trajs[0][2])
    stats = pkg.evaluate_agent(agent, env, n_eval_episodes=20, isolated=True, persistent=True)
    want = h.evaluate_agent_device(20, True, persistent=True)
    assert want[3]["path"] == 2 and stats["mean_reward"] == want[0]["mean_reward"] and stats["mean_length"] == want[0]["mean_length"]
