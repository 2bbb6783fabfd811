#!/usr/bin/env python3
"""Latency of a deployment policy (include/dril_policy.h) next to predict_actions of the training handle it was taken from: same parameters, same process, same observations.

Per shape and batch size: median wall time of NeuralPolicy.act (pinned staging, one copy in, device work, one copy out, one stream wait), median HIP-event time of that
device work alone, both for policy_act_kernel and for the layer-contraction path (set_threshold forces either), and median wall time of Handle.predict_actions /
SacHandle.predict_actions.  One process, every number after a warm-up; prints one markdown table (docs/deployment.md holds a copy as measured).

usage: python tools/policy_latency.py [calls=300] [warmup=30]"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g

pkg = g.load_package()
cap = pkg._capi
CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 300
WARM = int(sys.argv[2]) if len(sys.argv) > 2 else 30
BATCHES = (1, 16, 256, 4096)


def ppo_handle(kind, hidden, act=0, module=None):
    c = cap.default_config(kind)
    c.n_envs, c.n_steps, c.batch_size, c.epochs = 64, 4, 256, 1
    if len(hidden) == 2 and act == 0:
        c.hidden1, c.hidden2 = hidden
    else:
        c.n_hidden, c.activation = len(hidden), act
        for i, w in enumerate(hidden):
            c.hidden[i] = w
    return pkg.Handle(c, env_module=module)


def sac_handle(hidden):
    env = pkg.PendulumEnv()
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=hidden)
    return pkg.SacHandle(pkg.make_sac_config(env, 64, pkg.SAC(batch_size=64, buffer_capacity=4096), layer, seed=1))


def median_us(fn, calls=CALLS, warm=WARM, also=None):
    for _ in range(warm):
        fn()
    wall, extra = [], []
    for _ in range(calls):
        t0 = time.perf_counter(); fn(); wall.append((time.perf_counter() - t0) * 1e6)
        if also is not None:
            extra.append(also() * 1e3)
    return statistics.median(wall), (statistics.median(extra) if extra else float("nan"))


SHAPES = (
    ("[64,64] tanh D=4 (CartPole, fused policy_kernel)", lambda: ppo_handle(cap.ENV_CARTPOLE, (64, 64))),
    ("[256,256] tanh D=3 (Pendulum, fused policy_kernel)", lambda: ppo_handle(cap.ENV_PENDULUM, (256, 256))),
    ("[512,512] relu D=3 (SAC Pendulum)", lambda: sac_handle((512, 512))),
    ("[128,128,128] gelu D=12 (reacher3 plug-in, generic path)", lambda: ppo_handle(cap.ENV_MODULE, (128, 128, 128), 6, ROOT / "examples" / "envs" / "reacher3_plugin.hsaco")),
)

print(f"median of {CALLS} calls after {WARM}; microseconds; wall = Python call to return, event = HIP events around the device work\n")
print("| shape | B | policy kernel wall | kernel event | policy contractions wall | contractions event | handle predict_actions wall |")
print("|---|---:|---:|---:|---:|---:|---:|")
for name, make in SHAPES:
    h = make()
    h.set_params((np.random.default_rng(0).standard_normal(h.P) * 0.2).astype(np.float32))
    p = pkg.NeuralPolicy.from_handle(h)
    p.kernel_time(True)
    for B in BATCHES:
        obs = np.random.default_rng(B).standard_normal((B, p.D)).astype(np.float32)
        p.set_threshold(1 << 30)
        kw, ke = median_us(lambda: p.act(obs, True), also=lambda: p.kernel_time(True))
        p.set_threshold(1) if B > 1 else None
        gw, ge = (median_us(lambda: p.act(obs, True), also=lambda: p.kernel_time(True)) if B > 1 else (float("nan"), float("nan")))
        hw, _ = median_us(lambda: h.predict_actions(obs, deterministic=True))
        print(f"| {name} | {B} | {kw:.1f} | {ke:.1f} | {gw:.1f} | {ge:.1f} | {hw:.1f} |", flush=True)
    p.close(); h.close()
