#!/usr/bin/env python3
"""Per-env-step cost of evaluate_agent on a PPO handle: the per-step host loop (dril_evaluate_agent) against the device-resident verb (dril_evaluate_agent_device)
on its two paths and at several poll intervals K, next to a collection step of the same handle.
  CartPole  (time limit 500, real episodes: poles fall)   built-in kind, hidden [64,64]: both paths
  Pendulum  (time limit 200)                              built-in kind, hidden [64,64]: both paths
  Pendulum under cfg.norm_obs / cfg.norm_reward           the same, wrapped: step-granular by default (six launches per env step), the persistent kernel on request
                                                          (persistent = True: the frozen statistics are an argument of the kernel)
  reacher3 plug-in (time limit 100)                       step-granular path only
  reacher3_eval: the same env with DRIL_ENV_PLUGIN_EVALUATE  path 0 against path 2 (the plug-in's own evaluation kernel) on the same handle in the same process
E = 64 / 1 024 / 16 384, one process, n_eval = E (for Pendulum / reacher3 exactly one time limit of env steps).  The wall time of the whole call — reset, every
enqueued step (those past the last counted episode included), the polls, the event copy, the restore of the training envs — is divided by the counted steps
(stats.n_steps).  The calls are synchronous, so the wall time contains the device time.  Median (min .. max) over the calls after warm-up.
The collection figure: wall time of dril_collect_rollout (n_steps = 32, drained) / 32.
usage: python tools/ppo_eval_latency.py [evaluations=20] [env ...]      env: cartpole pendulum pendulum_norm reacher3 reacher3_eval"""
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
WARM, T = 3, 32
REACHER = ROOT / "examples" / "envs" / "reacher3_plugin.hsaco"
KIND = {"cartpole": (capi.ENV_CARTPOLE, None), "pendulum": (capi.ENV_PENDULUM, None), "pendulum_norm": (capi.ENV_PENDULUM, None), "reacher3": (capi.ENV_MODULE, REACHER),
        "reacher3_eval": (capi.ENV_MODULE, REACHER.with_name("reacher3_eval_plugin.hsaco"))}
K_PERSISTENT = (8, 32, 64, 128, 0)          # candidates of the persistent path (0 = the library's default)


def handle_for(name, E):
    kind, module = KIND[name]
    cfg = capi.default_config(kind)
    cfg.n_envs, cfg.n_steps, cfg.batch_size, cfg.epochs = E, T, min(E * T, 4096), 1
    if name == "pendulum_norm":
        cfg.norm_obs = cfg.norm_reward = cfg.norm_training = 1
    h = pkg.Handle(cfg, env_module=module)
    h.set_params((np.random.default_rng(0).standard_normal(h.P) * 0.3).astype(np.float32))
    h.env_reset(1)
    if name == "pendulum_norm":
        h.collect_rollout()                      # statistics that are not the initial ones
    return h


def timed(call):
    wall, steps, info = [], 0, None
    for r in range(R + WARM):
        a = time.perf_counter(); out = call(); b = time.perf_counter()
        steps = out[0]["n_steps"]; info = out[3] if len(out) > 3 else None
        if r >= WARM:
            wall.append((b - a) / steps * 1e6)
    w = np.asarray(wall)
    return f"{np.median(w):8.1f} ({w.min():.1f} .. {w.max():.1f})", steps, info


def measure(name, E):
    h = handle_for(name, E)
    print(f"== {name}  E = {E}", flush=True)
    s, steps, _ = timed(lambda: h.evaluate_agent(E, True))
    print(f"   host loop (dril_evaluate_agent)              {s} us / env step over {steps} steps", flush=True)
    for K in (0, 1):
        s, steps, info = timed(lambda: h.evaluate_agent_device(E, True, poll_steps=K, force_step_granular=True))
        print(f"   device, step-granular  K = {'default' if not K else K:>7}          {s} us / env step over {steps} steps, {info['steps_enqueued']} enqueued, {info['launches']} launches", flush=True)
        assert info["path"] == 0
    if KIND[name][1] is None:
        for K in K_PERSISTENT:
            s, steps, info = timed(lambda: h.evaluate_agent_device(E, True, poll_steps=K, persistent=name == "pendulum_norm"))
            print(f"   device, persistent     K = {'default' if not K else K:>7}          {s} us / env step over {steps} steps, {info['steps_enqueued']} enqueued, {info['launches']} launches", flush=True)
            assert info["path"] == 1
    if name == "reacher3_eval":
        for K in (8, 32, 0):
            s, steps, info = timed(lambda: h.evaluate_agent_device(E, True, poll_steps=K, persistent=True))
            print(f"   device, path 2         K = {'default' if not K else K:>7}          {s} us / env step over {steps} steps, {info['steps_enqueued']} enqueued, {info['launches']} launches", flush=True)
            assert info["path"] == 2
    h.env_reset(1)
    col = []
    for r in range(5 + WARM):
        h.synchronize(); a = time.perf_counter(); h.collect_rollout(); h.synchronize(); b = time.perf_counter()
        if r >= WARM:
            col.append((b - a) / T * 1e6)
    print(f"   dril_collect_rollout                         {np.median(col):8.1f} ({min(col):.1f} .. {max(col):.1f}) us / env step (wall, {T} steps)", flush=True)
    h.close()


for name in ENVS:
    for E in (64, 1024, 16384):
        measure(name, E)
