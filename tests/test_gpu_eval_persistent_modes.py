"""GPU (-m gpu): the two opt-in modes of the persistent evaluate kernel (docs/evaluation.md) — evaluation under a frozen cfg.norm_* normaliser and the trajectory
recording inside the kernel — every check through pkg.Handle, everything compared BITWISE.

Checkers: (1) the step-granular form of the same verb on the same handle (force_step_granular = 1 / persistent = False), whose kernels the modes do not touch;
(2) for the evaluation, dril_evaluate_agent on a twin with norm_training = 0 and the same statistics; (3) for what a call must NOT do, readings before and after
it and a twin that trained without any such call.

Sizes: E = 130 (two workgroups; the last wave holds two valid lanes) and E = 24 (one partial wave), n_steps <= 8.  Time limits are 15 (60 for CartPole) wherever
the test does not need terminations.  The trajectory cases of the kinds that can terminate need BOTH terminated and truncated recorded envs, which is asserted; with
the policies of tests/test_gpu_traj_device.py MountainCar, MountainCarContinuous and Acrobot first terminate after 70 - 170 steps, so there the time limit is taken
as that test takes it — the median first-episode length of the 37 recorded envs under a long limit (about 150 / 85 / 80 steps) — and not kept below 60: a limit of
60 would leave those cases without a single termination.  Such a case still takes well under a second."""
import math
import threading

import numpy as np
import pytest

from test_gpu_env_plugin import _cfg, _co, _params
from test_gpu_eval_device import assert_bitwise, assert_equal_runs, limit as eval_limit, nudged_params, snapshot, stats_equal, STAT_KEYS
from test_gpu_traj_device import LONG, TERM, TRUNC, CUT, bits, policy_for, same_trajs

pytestmark = pytest.mark.gpu
F = np.float32
SEED = 13
K_PERSISTENT = 64                                                                  # the persistent forms' default poll interval, capped by the time limit
NORM_MODES = {"obs": dict(norm_obs=1, norm_reward=0), "reward": dict(norm_obs=0, norm_reward=1), "both": dict(norm_obs=1, norm_reward=1)}
STATS = dict(obs_mean=F([0.1, -0.2, 0.5]), obs_var=F([0.5, 0.6, 8.0]), obs_count=100, ret_mean=0.0, ret_var=50.0, ret_count=100)   # Pendulum, where a test sets them


def clips(kind):
    """small enough to bite (asserted where used): a normalised observation has about unit variance, so 0.5 cuts a good part of them; Pendulum's rewards reach -16
    against a returns' deviation of about that size; CartPole's / Acrobot's are +-1 against a deviation of the discounted return of at most 1 / (1 - gamma) = 100"""
    return dict(clip_obs=0.5, clip_reward=0.3 if kind in (1, 2) else 0.005)


def make(pkg, kind, hidden, E, episode_len=None, flat=None, reset=SEED, **kw):
    cfg = _cfg(pkg, kind, n_envs=E, n_steps=kw.pop("n_steps", 4), episode_len=episode_len or eval_limit(kind), batch_size=kw.pop("batch_size", E),
               hidden1=hidden[0], hidden2=hidden[1], **kw)
    h = pkg.Handle(cfg)
    h.set_params(nudged_params(h, hidden) if flat is None else flat)
    if reset is not None:
        h.env_reset(reset)
    return h


def trained(pkg, kind, hidden, E, **kw):
    """a handle whose normaliser trains, after two collections: the statistics are not the initial ones"""
    a = make(pkg, kind, hidden, E, norm_training=1, **kw)
    a.collect_rollout(); a.collect_rollout()
    st = a.norm_get_stats()
    if kw.get("norm_obs"):
        assert st["obs_count"] > 0 and not np.allclose(st["obs_var"], 1.0)
    if kw.get("norm_reward"):
        assert st["ret_count"] > 0 and st["ret_var"] != 1.0
    return a, st


def frozen_twin(pkg, st, kind, hidden, E, **kw):
    b = make(pkg, kind, hidden, E, norm_training=0, **kw)
    b.norm_set_stats(st["obs_mean"], st["obs_var"], st["obs_count"], st["ret_mean"], st["ret_var"], st["ret_count"])
    return b


def readings(h):
    """what a call must leave as it was, as far as the handle shows it: the statistics in force and their counts, the raw per-step arrays, env state and step counts,
    the monitor's window (the other half, the parities and `returns` show in what training computes next: the twin test below)"""
    return h.norm_get_stats(), h.norm_get_original(), h.env_get_state(), h.monitor_stats() if h.cfg.monitor_window > 0 else ()


def same_readings(a, b):
    return stats_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2])) \
        and np.array_equal(a[3], b[3], equal_nan=True)


def same_eval(a, b, where):
    (sa, ra, la, _), (sb, rb, lb, _) = a, b
    assert np.array_equal(la, lb), (where, la, lb)
    assert np.array_equal(bits(ra), bits(rb)), (where, ra, rb)
    for k in STAT_KEYS:
        assert sa[k] == sb[k] or (math.isnan(sa[k]) and math.isnan(sb[k])), (where, k, sa[k], sb[k])


def same_recordings(a, b, where):
    (ta, la, fa, _), (tb, lb, fb, _) = a, b
    assert np.array_equal(la, lb) and np.array_equal(fa, fb), (where, la, lb, fa, fb)
    same_trajs(ta, tb, len(ta), where)


# ---- 1: what fails without the feature -------------------------------------------------------------------------------------------------------------------------------------
def test_the_requests_reach_the_persistent_kernel(pkg):
    h = make(pkg, 1, (64, 64), 130, norm_obs=1, norm_reward=1)
    s, r, l, info = h.evaluate_agent_device(10, True, persistent=True)
    assert info["path"] == 1 and info["launches"] == 1 and len(r) == 10
    assert h.evaluate_agent_device(10, True)[3]["path"] == 0                           # the default is today's rule
    h.close()
    h = make(pkg, 0, (64, 64), 130)
    trajs, lengths, flags, info = h.collect_trajectory_device(37, persistent=True)
    assert info["path"] == 1 and info["launches"] == 1 and len(trajs) == 37 and (lengths >= 1).all()
    assert h.collect_trajectory_device(37)[3]["path"] == 0
    h.close()


# ---- 2: evaluation under a frozen normaliser ---------------------------------------------------------------------------------------------------------------------------------
EVAL_HANDLES = [(0, (64, 64)), (1, (64, 64)), (6, (64, 64)), (1, (128, 128)), (1, (256, 256)), (2, (64, 64))]


@pytest.mark.parametrize("E", [130, 24])
@pytest.mark.parametrize("kind,hidden", EVAL_HANDLES)
def test_evaluation_under_a_frozen_normaliser_equals_both_step_granular_forms(pkg, kind, hidden, E):
    for mode, nkw in NORM_MODES.items():
        for monitor in (0, 30):
            kw = dict(monitor_window=monitor, **nkw, **clips(kind))
            a, st = trained(pkg, kind, hidden, E, **kw)
            b = frozen_twin(pkg, st, kind, hidden, E, **kw)
            # the clips bite: from the statistics and a raw recording of the very episodes the deterministic evaluation runs (the seed in force)
            rec = a.collect_trajectory_device(E)[0]
            eps = a.cfg.norm_epsilon
            if nkw["norm_obs"]:
                z = np.concatenate([(o[:-1] - st["obs_mean"]) / np.sqrt(st["obs_var"] + F(eps)) for o, _, _ in rec])
                assert (np.abs(z) > kw["clip_obs"]).any() and (np.abs(z) < kw["clip_obs"]).any(), (kind, mode, "no observation is clipped")
            if nkw["norm_reward"]:
                rn = np.concatenate([r for _, _, r in rec]) / np.sqrt(F(st["ret_var"]) + F(eps))
                assert (np.abs(rn) > kw["clip_reward"]).any(), (kind, mode, "no reward is clipped", float(np.abs(rn).max()))
            before = readings(a)
            for det in (True, False):
                for n in (10, 60, 1):
                    where = (kind, hidden, E, mode, monitor, det, n)
                    new = a.evaluate_agent_device(n, det, persistent=True)
                    assert new[3]["path"] == 1 and new[3]["launches"] * min(K_PERSISTENT, a.cfg.episode_len) == new[3]["steps_enqueued"], (where, new[3])
                    assert same_readings(before, readings(a)), where
                    forced = a.evaluate_agent_device(n, det, persistent=True, force_step_granular=True)
                    assert forced[3]["path"] == 0 and forced[3]["launches"] == 6 * forced[3]["steps_enqueued"]   # force_step_granular wins; six launches per env step
                    same_eval(new, forced, where)
                    assert_equal_runs(b.evaluate_agent(n, det), new, where)            # the old verb on the twin that does not train
                    if n == 1:
                        assert math.isnan(new[0]["std_reward"])
            if kind == 0:
                assert len(set(a.evaluate_agent_device(60, True, persistent=True)[2].tolist())) > 1   # poles fall at different steps: the lengths say something
            assert same_readings(before, readings(a))
            a.close(); b.close()


# ---- 3: both forwards -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [(64, 64), (256, 256)])
def test_both_forwards(pkg, monkeypatch, hidden):
    """the f16-piece forward (default) and the exact f32 one (DRIL_GRAD_VARIANT=0, latched at create: "exact f32 everywhere"), in both modes of the kernel.
    Parameters of scale 0.1: the actor's mean stays inside Pendulum's Box(-2, 2), so the last bits of the forward reach the env (the nudged ones of scale 0.5
    saturate the clamp, after which both forwards act alike)"""
    kw = dict(norm_obs=1, norm_reward=1, **clips(1))
    out = {}
    flat = None
    for fwd in ("f16", "f32"):
        if fwd == "f32":
            monkeypatch.setenv("DRIL_GRAD_VARIANT", "0")
        h = make(pkg, 1, hidden, 130, **kw)
        monkeypatch.delenv("DRIL_GRAD_VARIANT", raising=False)
        flat = _params(h.P, 21, 0.1) if flat is None else flat
        h.set_params(flat); h.norm_set_stats(**STATS)
        seen = []
        for det in (True, False):
            new, old = h.evaluate_agent_device(60, det, persistent=True), h.evaluate_agent_device(60, det, force_step_granular=True)
            assert (new[3]["path"], old[3]["path"]) == (1, 0)
            same_eval(new, old, (fwd, hidden, det))
            rn, ro = h.collect_trajectory_device(37, deterministic=det, persistent=True), h.collect_trajectory_device(37, deterministic=det)
            assert (rn[3]["path"], ro[3]["path"]) == (1, 0)
            same_recordings(rn, ro, (fwd, hidden, det))
            seen += [new[1]] + [t[1].ravel() for t in rn[0]]
        out[fwd] = np.concatenate(seen)
        h.close()
    assert out["f16"].shape == out["f32"].shape and not np.array_equal(bits(out["f16"]), bits(out["f32"]))   # two arithmetics: the selection did select (120 returns, 888 actions)


# ---- 4: nothing is left behind ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_persistent_calls_between_training_iterations_change_nothing(pkg):
    """A: env_reset, collect, update, collect, update.  B: the same with persistent evaluations and recordings, deterministic and stochastic, under other seeds, after
    the reset and after each update.  Everything training continues from is bitwise equal afterwards, and after one more collection and update (statistics of both
    halves, parities, counts, `returns`, the training flag: whatever differed would show in the next merge)"""
    E = 24
    kw = dict(monitor_window=30, epochs=2, seed=5, n_steps=8, batch_size=96, norm_obs=1, norm_reward=1, norm_training=1, **clips(1))
    a, b = (make(pkg, 1, (64, 64), E, episode_len=12, reset=None, **kw) for _ in range(2))
    flat = nudged_params(a, (64, 64))
    calls = []

    def visit(h):
        for det in (True, False):
            calls.append(h.evaluate_agent_device(7, det, seed=1000 + len(calls), persistent=True))
            assert calls[-1][3]["path"] == 1
            calls.append(h.collect_trajectory_device(E, deterministic=det, seed=1000 + len(calls), max_steps=5 if det else None, persistent=True))
            assert calls[-1][3]["path"] == 1

    for h, visits in ((a, False), (b, True)):
        h.set_params(flat); h.env_reset(13)
        if visits:
            visit(h)
        for _ in range(2):
            h.collect_rollout(); h.ppo_update()
            if visits:
                visit(h)
    assert len(calls) == 12 and a.monitor_stats()[2] > 0
    assert_bitwise(snapshot(a, True), snapshot(b, True))
    for h in (a, b):
        h.collect_rollout(); h.ppo_update()
    assert_bitwise(snapshot(a, True), snapshot(b, True))
    a.close(); b.close()


# ---- 5: trajectories ------------------------------------------------------------------------------------------------------------------------------------------------------------
def traj_handle(pkg, kind, hidden, E, limit, norm=False, **kw):
    nkw = dict(norm_obs=1, norm_reward=1, norm_training=1, n_steps=8, batch_size=8 * E, **clips(kind)) if norm else {}
    h = make(pkg, kind, hidden, E, episode_len=limit, **nkw, **kw)
    h.set_params(policy_for(h, kind, hidden))                                          # tests/test_gpu_traj_device.py's policies: the kinds that can terminate do
    if norm:
        h.collect_rollout(); h.collect_rollout()
        assert not np.allclose(h.norm_get_stats()["obs_var"], 1.0)
    return h


def median_limit(pkg, kind, hidden, E, **kw):
    """tests/test_gpu_traj_device.py's rule: the median first-episode length of the recorded envs under a long limit, so that some terminate before it"""
    h = traj_handle(pkg, kind, hidden, E, LONG[kind], **kw)
    lens = np.sort(h.collect_trajectory_device(min(37, E), seed=SEED)[1])
    h.close()
    limit = int(lens[len(lens) // 2])
    assert lens[0] < limit < LONG[kind], (kind, lens)
    return limit


TRAJ_CASES = [(k, (64, 64), 130, {}) for k in (0, 1, 3, 4, 6, 2, 7)] + [(0, (256, 256), 130, {}), (0, (64, 64), 130, dict(action_start=0)), (0, (64, 64), 130, dict(action_start=1)),
                                                                           (1, (64, 64), 130, dict(norm=True)), (0, (64, 64), 24, {}), (1, (64, 64), 24, dict(norm=True))]


@pytest.mark.parametrize("kind,hidden,E,kw", TRAJ_CASES)
def test_recordings_inside_the_kernel_equal_the_step_granular_verb(pkg, kind, hidden, E, kw):
    limit = median_limit(pkg, kind, hidden, E, **kw) if kind in LONG else 12
    h = traj_handle(pkg, kind, hidden, E, limit, **kw)
    before = readings(h) if kw.get("norm") else None
    K = min(K_PERSISTENT, limit)
    full = {}
    for M in (1, min(37, E), E):
        for max_steps in (None, 5, 1):
            for final_original in (False, True):
                for det in (True, False):
                    where = (kind, hidden, E, M, max_steps, final_original, det)
                    args = dict(max_steps=max_steps, deterministic=det, seed=SEED, final_original=final_original)
                    new, old = h.collect_trajectory_device(M, persistent=True, **args), h.collect_trajectory_device(M, **args)
                    assert (new[3]["path"], old[3]["path"]) == (1, 0), where
                    same_recordings(new, old, where)
                    ni, oi = new[3], old[3]
                    assert (ni["capacity"], ni["longest"], ni["cut_by_max_steps"]) == (oi["capacity"], oi["longest"], oi["cut_by_max_steps"])
                    assert ni["longest"] <= ni["steps_enqueued"] <= ni["capacity"] and ni["launches"] == -(-ni["steps_enqueued"] // K), (where, ni)   # never a step past Tcap
                    assert oi["launches"] == (11 if kw.get("norm") else 8) * oi["steps_enqueued"]      # the step-granular form is the parent's
                    if max_steps:
                        assert (new[2] == CUT).any() and new[1].max() <= max_steps
                    elif M > 1 and det and not final_original:
                        flags = new[2][:37]
                        if kind in LONG:                                               # a comparison that never met a termination, or never a time limit, proves little
                            assert ((flags & TERM) != 0).any() and ((flags & TRUNC) != 0).any(), (where, flags)
                        else:
                            assert (flags == TRUNC).all()
                    if max_steps is None and not final_original:
                        full.setdefault(det, {})[M] = new
    for det, by_m in full.items():                                                     # the trajectory of env m does not depend on M ...
        for M, run in by_m.items():
            same_trajs(run[0], by_m[E][0], M, ("independent of M", kind, det, M))
        for poll in (1, 7):                                                            # ... nor on the poll interval
            run = h.collect_trajectory_device(min(37, E), deterministic=det, seed=SEED, poll_steps=poll, persistent=True)
            same_recordings(run, by_m[min(37, E)], ("poll", kind, det, poll))
            assert run[3]["path"] == 1 and run[3]["launches"] == -(-run[3]["steps_enqueued"] // poll) and run[3]["steps_enqueued"] <= limit
    if h.discrete:
        acts = np.concatenate([t[1] for t in full[False][E][0]])
        assert acts.min() >= h.cfg.action_start and acts.max() <= h.cfg.action_start + h.A - 1 and len(np.unique(acts)) > 1
    if kind in (2, 7):                                                                 # the final row is the wrapper's unless final_original; the rows below it never are
        a0 = h.collect_trajectory_device(1, seed=SEED, persistent=True)[0][0][0]
        a1 = h.collect_trajectory_device(1, seed=SEED, persistent=True, final_original=True)[0][0][0]
        assert np.array_equal(bits(a0[:-1]), bits(a1[:-1])) and not np.array_equal(bits(a0[-1]), bits(a1[-1]))
    if before is not None:
        assert same_readings(before, readings(h))
    h.close()


# ---- 6: fallbacks -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["generic", "plugin"])
def test_where_the_kernel_does_not_apply_the_request_changes_nothing(pkg, which):
    E = 24
    if which == "generic":
        h = make(pkg, 0, (32, 48), E)
    else:
        h = pkg.Handle(_cfg(pkg, pkg._capi.ENV_MODULE, n_envs=E, n_steps=4, batch_size=E * 4, episode_len=15), env_module=_co("reacher3"))
        h.set_params(nudged_params(h, (64, 64))); h.env_reset(SEED)
    for det in (True, False):
        new, old = h.evaluate_agent_device(30, det, persistent=True), h.evaluate_agent_device(30, det)
        assert (new[3]["path"], old[3]["path"]) == (0, 0) and new[3] == old[3]
        same_eval(new, old, (which, det))
        new, old = h.collect_trajectory_device(E, deterministic=det, persistent=True), h.collect_trajectory_device(E, deterministic=det)
        assert (new[3]["path"], old[3]["path"]) == (0, 0) and new[3] == old[3]
        same_recordings(new, old, (which, det))
    h.close()


def test_external_envs_keep_their_refusal_and_the_default_launch_counts_are_the_parents(pkg):
    capi = pkg._capi
    ext = pkg.Handle(_cfg(pkg, capi.ENV_EXTERNAL, n_envs=2, n_steps=2, batch_size=2, ext_obs_dim=6, ext_action_dim=3, ext_discrete=1))
    for verb in (ext.evaluate_agent_device, ext.collect_trajectory_device):
        msgs = []
        for persistent in (False, True):
            with pytest.raises(pkg.DrilError) as e:
                verb(1, persistent=persistent)
            assert e.value.code == capi.ERR_UNSUPPORTED
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1]
    ext.close()
    # persistent=False: per env step three launches (policy, step, observe) on a fused shape, six under cfg.norm_*; the recording eight / eleven; path 1 one per K
    for norm, per_eval, per_traj in ((False, 3, 8), (True, 6, 11)):
        h = make(pkg, 1, (64, 64), 24, **(dict(norm_obs=1, norm_reward=1) if norm else {}))
        i = h.evaluate_agent_device(30, True, force_step_granular=True)[3]
        assert i["path"] == 0 and i["launches"] == per_eval * i["steps_enqueued"]
        i = h.evaluate_agent_device(30, True)[3]
        assert (i["path"], i["launches"]) == ((0, per_eval * i["steps_enqueued"]) if norm else (1, 2))   # (30 episodes of 24 envs: two time limits of 15 steps = two launches)
        i = h.collect_trajectory_device(24)[3]
        assert i["path"] == 0 and i["launches"] == per_traj * i["steps_enqueued"]
        h.close()


# ---- 7: data-parallel -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_ranks_run_the_persistent_forms_on_their_own_envs_without_an_all_reduce(pkg):
    E = 24
    common = dict(n_steps=4, episode_len=15, seed=11, norm_obs=1, norm_reward=1, norm_training=1, **clips(1))
    hs = [pkg.Handle(_cfg(pkg, 1, n_envs=E, rank=r, world_size=2, batch_size=2 * E, **common)) for r in range(2)]
    pkg.Handle.comm_loopback(hs)
    flat = nudged_params(hs[0], (64, 64))
    out, err = [None, None], [None, None]

    def run(r):
        try:
            hs[r].set_params(flat); hs[r].env_reset(21); hs[r].norm_set_stats(**STATS)
            calls = hs[r].comm_allreduce_calls()
            res = [(hs[r].evaluate_agent_device(30, det, persistent=True), hs[r].collect_trajectory_device(E, deterministic=det, persistent=True)) for det in (True, False)]
            out[r] = (res, hs[r].comm_allreduce_calls() - calls)
        except BaseException as ex:   # noqa: BLE001 - re-raised below
            err[r] = ex
    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in ts]; [t.join() for t in ts]
    for ex in err:
        if ex is not None:
            raise ex
    for r in range(2):
        res, calls = out[r]
        assert calls == 0
        one = pkg.Handle(_cfg(pkg, 1, n_envs=E, batch_size=E, **common))               # the same global env indices in a handle of its own
        one.set_params(flat); one.env_reset(21 + r * E); one.norm_set_stats(**STATS)
        for (ev, tr), det in zip(res, (True, False)):
            assert ev[3]["path"] == 1 and tr[3]["path"] == 1
            same_eval(ev, one.evaluate_agent_device(30, det, force_step_granular=True), (r, det))
            same_recordings(tr, one.collect_trajectory_device(E, deterministic=det), (r, det))
        one.close()
    assert not np.array_equal(bits(out[0][0][0][0][1]), bits(out[1][0][0][0][1]))      # the ranks own different envs


# ---- 8: the host mirror ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_host_mirror_takes_the_keyword(pkg):
    env = pkg.MonitorWrapperEnv(pkg.DeviceParallelEnv(pkg.CartPoleEnv(max_steps=60), 32, seed=3), 20)
    agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space()), pkg.PPO(n_steps=8, batch_size=128, epochs=1), seed=0)
    assert pkg.evaluate_agent(agent, env, n_eval_episodes=12, isolated=True, persistent=True) == pkg.evaluate_agent(agent, env, n_eval_episodes=12, isolated=True)
    a, b = pkg.collect_trajectory(agent, env, persistent=True), pkg.collect_trajectory(agent, env)
    assert all(np.array_equal(bits(np.asarray(x)), bits(np.asarray(y))) for x, y in zip(a, b))
