#!/usr/bin/env python3
"""Per-env-step cost of collect_trajectory on a SAC handle (dril_sac_collect_trajectory) at E = 64 / 1 024 and M = 1 / E recorded envs, next to dril_sac_evaluate_agent
(n = E episodes) on the same handle in the same process.
  Pendulum  (time limit 200)          built-in kind: one env launch per step (sac_traj_env_kernel), no shadow envs
  reacher3 plug-in (time limit 100)   head, the plug-in's step, and over M envs a state copy, the shadow step, the shadow observe, sac_traj_record_kernel
Hidden [64,64].  The wall time of the whole call — reset, every enqueued step, the looks at the counter, the copy-out and reorder, the restore of the training envs — is
divided by the steps that count: the longest recorded trajectory (the verb), stats.n_steps (the evaluation).  Median (min .. max) over the calls after warm-up.
usage: python tools/sac_traj_latency.py [calls=20] [env ...]      env: pendulum reacher3"""
import sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g

pkg = g.load_package()
R = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ENVS = sys.argv[2:] or ["pendulum", "reacher3"]
WARM, SIZES = 3, (64, 1024)
REACHER = ROOT / "examples" / "envs" / "reacher3_plugin.hsaco"


def handle_for(name, E):
    if name == "reacher3":
        info = pkg.describe_env_module(REACHER)
        env, module = pkg.host.ModuleEnv(str(REACHER), info, info["episode_len"]), REACHER
    else:
        env, module = pkg.PendulumEnv(), None
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(64, 64))
    h = pkg.SacHandle(pkg.make_sac_config(env, E, pkg.SAC(batch_size=64, buffer_capacity=max(E, 64)), layer, seed=1), env_module=module)
    h.set_params(pkg.sac_flatten_params(layer.initialparameters(np.random.default_rng(0))))
    h.env_reset(1)
    return h, env.max_steps


def timed(call, reps):
    wall, last = [], None
    for r in range(reps + WARM):
        a = time.perf_counter(); steps, last = call(); b = time.perf_counter()
        if r >= WARM:
            wall.append((b - a) / steps * 1e6)
    w = np.asarray(wall)
    return f"{np.median(w):8.1f} ({w.min():.1f} .. {w.max():.1f})", last


def measure(name, E):
    h, limit = handle_for(name, E)
    print(f"== {name}  E = {E}, time limit {limit}", flush=True)
    for M in (1, E):
        def verb():
            _, lengths, _, info = h.collect_trajectory(M)
            return int(lengths.max()), info
        s, info = timed(verb, R)
        print(f"   dril_sac_collect_trajectory  M = {M:5d}  {s} us / env step over {info['longest']} steps, {info['steps_enqueued']} enqueued, {info['launches']} launches", flush=True)

    def evaluation():
        st, _, _ = h.evaluate_agent(E, True)
        return st["n_steps"], None
    s, _ = timed(evaluation, R)
    print(f"   dril_sac_evaluate_agent      n = {E:5d}  {s} us / env step", flush=True)
    h.close()


for name in ENVS:
    for E in SIZES:
        measure(name, E)
