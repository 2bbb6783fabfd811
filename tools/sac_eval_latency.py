#!/usr/bin/env python3
"""Per-env-step cost of a device-resident evaluation (dril_sac_evaluate_agent) against the poll interval, next to a collection step of the same handle:
  built-in Pendulum (T = 200)      actor hidden layers + sac_eval_env_kernel per env step
  reacher3 plug-in  (T = 100)      actor hidden layers + head + the plug-in's step + sac_eval_account_kernel per env step
each with the default poll interval K = min(T, 32) and with DRIL_SAC_EVAL_POLL=1 (the host reads the event counter after every step), hidden [64,64],
E = 64 / 1 024 / 16 384, one process.  n_eval = E, so an evaluation is exactly one time limit of env steps; the wall time of the whole call (reset, every enqueued
step — the ones past the last counted episode included — the event copy, the restore of the training envs) is divided by that number.  The call is synchronous,
so its wall time contains the device time.  The collection figure is the library's HIP-event time of dril_sac_collect_rollout(32) per step (cfg.profile_events).
Median and min..max over the evaluations after warm-up.
usage: python tools/sac_eval_latency.py [evaluations=20]"""
import os, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g

pkg = g.load_package()
R = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WARM, HIDDEN = 3, (64, 64)
REACHER = ROOT / "examples" / "envs" / "reacher3_plugin.hsaco"


def handle_for(env, E, module, poll):
    alg = pkg.SAC(batch_size=256, buffer_capacity=max(64 * E, 4096))
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=HIDDEN)
    if poll:
        os.environ["DRIL_SAC_EVAL_POLL"] = str(poll)               # latched when the handle is created
    try:
        h = pkg.SacHandle(pkg.make_sac_config(env, E, alg, layer, seed=0, profile_events=True), env_module=module)
    finally:
        os.environ.pop("DRIL_SAC_EVAL_POLL", None)
    h.set_params(pkg.sac_flatten_params(layer.initialparameters(np.random.default_rng(0))))
    return h


def measure(label, E, env, module, poll):
    h = handle_for(env, E, module, poll)
    wall = []
    for r in range(R + WARM):
        a = time.perf_counter(); stats, _, _ = h.evaluate_agent(E, True, seed=1); b = time.perf_counter()
        if r >= WARM:
            wall.append((b - a) / stats["n_steps"] * 1e6)
    h.env_reset(1)
    col = []
    for r in range(5 + WARM):
        h.profile_reset(); h.collect_rollout(32, False)
        if r >= WARM:
            col.append(h.profile()["collect_ms"] / 32 * 1e3)
    w = np.asarray(wall)
    print(f"E = {E:6d}  {label:18s} poll {'default' if not poll else poll:>7}  evaluation {np.median(w):7.1f} us / env step ({w.min():.1f} .. {w.max():.1f}) over {stats['n_steps']} steps"
          f"   collection step {np.median(col):6.1f} us (HIP events)", flush=True)
    h.close()


for E in (64, 1024, 16384):
    for poll in (0, 1):
        measure("built-in Pendulum", E, pkg.PendulumEnv(), None, poll)
        measure("reacher3 plug-in", E, pkg.host.ModuleEnv("", pkg.describe_env_module(REACHER), 100), REACHER, poll)
