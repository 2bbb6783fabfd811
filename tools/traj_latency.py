#!/usr/bin/env python3
"""Per-env-step cost of collect_trajectory on a PPO handle (dril_collect_trajectory_device) at E = 64 / 1 024 / 16 384 and M = 1 / E recorded envs, in its two forms — the
step-granular launches with shadow envs, and on request (persistent = True) the recording inside the persistent evaluate kernel — next to two baselines on the same
handle in the same process at E = 1 024: the step-granular evaluation (dril_evaluate_agent_device, force_step_granular = 1, n = E) and the host loop a caller had to
write before (dril_env_observe / dril_predict_actions / dril_env_step per step, one time limit of steps).
  CartPole  (time limit 500, real episodes: poles fall)   built-in kind, hidden [64,64]
  Pendulum  (time limit 200)                              built-in kind, hidden [64,64]
  Pendulum under cfg.norm_obs / cfg.norm_reward           the same, wrapped (statistics frozen for the call)
  reacher3 plug-in (time limit 100)                       generic kernels; no persistent form (the request falls back)
  reacher3_eval: the same env with DRIL_ENV_PLUGIN_EVALUATE  path 0 against path 2 (the recording mode of the plug-in's own evaluation kernel) on the same handle
The wall time of the whole call — reset, every enqueued step, the looks at the counter, the copy-out and reorder, the restore of the training envs — is divided by the
steps that count: the longest recorded trajectory (the verb), stats.n_steps (the evaluation), the steps taken (the host loop).  Median (min .. max) over the calls
after warm-up; the host loop is timed over fewer calls (a fifth), it is the slow one.
usage: python tools/traj_latency.py [calls=20] [env ...]      env: cartpole pendulum pendulum_norm reacher3 reacher3_eval"""
import sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g

pkg = g.load_package()
capi = pkg._capi
R = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ENVS = sys.argv[2:] or ["cartpole", "pendulum", "pendulum_norm", "reacher3", "reacher3_eval"]
WARM, SIZES, E_BASELINES = 3, (64, 1024, 16384), 1024
REACHER = ROOT / "examples" / "envs" / "reacher3_plugin.hsaco"
KIND = {"cartpole": (capi.ENV_CARTPOLE, None), "pendulum": (capi.ENV_PENDULUM, None), "pendulum_norm": (capi.ENV_PENDULUM, None), "reacher3": (capi.ENV_MODULE, REACHER),
        "reacher3_eval": (capi.ENV_MODULE, REACHER.with_name("reacher3_eval_plugin.hsaco"))}


def handle_for(name, E):
    kind, module = KIND[name]
    cfg = capi.default_config(kind)
    cfg.n_envs, cfg.n_steps, cfg.batch_size, cfg.epochs = E, 32, min(E * 32, 4096), 1
    if name == "pendulum_norm":
        cfg.norm_obs = cfg.norm_reward = cfg.norm_training = 1
    h = pkg.Handle(cfg, env_module=module)
    h.set_params((np.random.default_rng(0).standard_normal(h.P) * 0.3).astype(np.float32))
    h.env_reset(1)
    if name == "pendulum_norm":
        h.collect_rollout()                      # statistics that are not the initial ones
    return h


def timed(call, reps):
    wall, last = [], None
    for r in range(reps + WARM):
        a = time.perf_counter(); steps, last = call(); b = time.perf_counter()
        if r >= WARM:
            wall.append((b - a) / steps * 1e6)
    w = np.asarray(wall)
    return f"{np.median(w):8.1f} ({w.min():.1f} .. {w.max():.1f})", last


def host_loop(h, steps):
    lo, hi = (None, None) if h.discrete else (-1.0, 1.0) if h.cfg.env_kind == capi.ENV_MODULE else (-2.0, 2.0)
    h.env_reset(1)
    obs = h.env_observe(update_stats=False)
    for _ in range(steps):
        raw = h.predict_actions(obs, deterministic=True)
        h.env_step(raw if lo is None else np.clip(raw, lo, hi))
        obs = h.env_observe(update_stats=False)
    return steps, None


def measure(name, E):
    h = handle_for(name, E)
    limit = h.cfg.episode_len if h.cfg.episode_len else h.env_module_info()["episode_len"]
    print(f"== {name}  E = {E}, time limit {limit}", flush=True)
    for M in (1, E):
        for persistent in (False, True):
            def verb():
                _, lengths, _, info = h.collect_trajectory_device(M, persistent=persistent)
                return int(lengths.max()), info
            s, info = timed(verb, R)
            form = {0: "step-granular", 1: "persistent   ", 2: "path 2       "}[info["path"]]
            print(f"   dril_collect_trajectory_device  M = {M:5d}  {form}  {s} us / env step over {info['longest']} steps, {info['steps_enqueued']} enqueued, {info['launches']} launches", flush=True)
            if persistent and info["path"] == 0:
                print("      (no persistent form on this handle: the request fell back)", flush=True)
    if E != E_BASELINES:
        h.close()
        return

    def evaluation():
        st, _, _, info = h.evaluate_agent_device(E, True, force_step_granular=True)
        return st["n_steps"], info
    s, info = timed(evaluation, R)
    print(f"   dril_evaluate_agent_device, step-granular   {s} us / env step, {info['steps_enqueued']} enqueued, {info['launches']} launches", flush=True)
    s, _ = timed(lambda: host_loop(h, limit), max(1, R // 5))
    print(f"   host loop (observe / predict / step)        {s} us / env step over {limit} steps", flush=True)
    h.close()


for name in ENVS:
    for E in SIZES:
        measure(name, E)
