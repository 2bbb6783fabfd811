#!/usr/bin/env python3
"""Per-env-step cost of a SAC collection (dril_sac_collect_rollout, policy actions) over a device env plug-in, next to the built-in env and to the same env on the host:
  (a) reacher3 plug-in, fused        actor hidden layers + sac_collect_head_push_kernel + the plug-in's step per env step, one trailing push per collection
  (b) reacher3 plug-in, plain        DRIL_SAC_NO_FUSED_HEAD_PUSH=1: actor hidden layers + head + the plug-in's step + push
  (c) Pendulum twin plug-in          (fused)
  (d) built-in Pendulum              actor hidden layers + sac_collect_env_kernel (head, step, observe and push in one launch)
  (e) reacher3 on the host           the same physics in NumPy behind dril_sac_predict_actions + dril_sac_ext_push (DRIL_ENV_EXTERNAL): a PCIe round trip and a drain per step
hidden [64,64], T = 32 steps per collection, E = 64 / 1 024 / 16 384, one process.  Per collection: wall time around the call and the library's HIP-event time
(cfg.profile_events); median and min..max over the collections after warm-up, divided by T.  (e) has no HIP-event figure: its time is spent between device calls.
usage: python tools/sac_plugin_latency.py [collections=20]"""
import os, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g

pkg = g.load_package(); capi = pkg._capi
R = int(sys.argv[1]) if len(sys.argv) > 1 else 20
T, WARM, HIDDEN = 32, 3, (64, 64)
ENVS = ROOT / "examples" / "envs"
F = np.float32


def handle_for(env, E, module=None, plain=False):
    alg = pkg.SAC(batch_size=256, buffer_capacity=max(4 * T * E, 4096))
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=HIDDEN)
    if plain:
        os.environ["DRIL_SAC_NO_FUSED_HEAD_PUSH"] = "1"
    h = pkg.SacHandle(pkg.make_sac_config(env, E, alg, layer, seed=0, profile_events=True), env_module=module)
    os.environ.pop("DRIL_SAC_NO_FUSED_HEAD_PUSH", None)
    h.set_params(pkg.sac_flatten_params(layer.initialparameters(np.random.default_rng(0))))
    return h


def report(label, E, wall, dev):
    w = np.asarray(wall)
    line = f"E = {E:6d}  {label:30s} wall {np.median(w):8.1f} us / env step ({w.min():.1f} .. {w.max():.1f})"
    if dev:
        d = np.asarray(dev)
        line += f"   HIP events {np.median(d):7.1f} us ({d.min():.1f} .. {d.max():.1f})"
    print(line, flush=True)


def device(label, E, env, module=None, plain=False):
    h = handle_for(env, E, module, plain)
    h.env_reset(1)
    wall, dev = [], []
    for r in range(R + WARM):
        h.profile_reset()
        a = time.perf_counter(); h.collect_rollout(T, False); b = time.perf_counter()
        if r >= WARM:
            wall.append((b - a) / T * 1e6); dev.append(h.profile()["collect_ms"] / T * 1e3)
    report(label, E, wall, dev)
    h.close()


class HostReacher3:
    """E copies of examples/envs/reacher3_plugin.hip in NumPy float32, with the library's transition (time limit, terminal observation, auto-reset)"""

    def __init__(self, E, rng):
        self.E, self.rng, self.T = E, rng, 100
        self.st = np.zeros((E, 9), F); self.sc = np.zeros(E, np.int32)
        self.reset(np.ones(E, bool))

    def reset(self, where):
        n = int(where.sum())
        self.st[where, 0:3] = self.rng.random((n, 3), F) - F(0.5); self.st[where, 3:6] = 0; self.st[where, 6:9] = self.rng.random((n, 3), F) * F(2) - F(1)
        self.sc[where] = 0

    def obs(self):
        return np.concatenate([self.st, self.st[:, 0:3] - self.st[:, 6:9]], axis=1)

    def step(self, act):
        a = np.clip(act, F(-1), F(1))
        v = (self.st[:, 3:6] + F(0.1) * a) * F(0.95); p = self.st[:, 0:3] + F(0.1) * v
        self.st[:, 0:3] = p; self.st[:, 3:6] = v
        d = p - self.st[:, 6:9]
        rew = -(d * d).sum(1) - F(0.01) * (a * a).sum(1)
        term = (np.abs(p) > 2).any(1)
        self.sc += 1
        trunc = self.sc >= self.T
        tobs = self.obs()
        self.reset(term | trunc)
        return rew.astype(F), term.astype(np.uint8), trunc.astype(np.uint8), tobs


def host(label, E):
    info = pkg.describe_env_module(ENVS / "reacher3_plugin.hsaco")
    spaces = pkg.host.ModuleEnv("", info, info["episode_len"])

    class Ext:                                                      # the spaces of a HostParallelEnv: all make_sac_config reads
        kind = capi.ENV_EXTERNAL
        observation_space, action_space = spaces.observation_space, spaces.action_space
    h = handle_for(Ext(), E)
    env = HostReacher3(E, np.random.default_rng(1))
    obs = env.obs()
    wall = []
    for r in range(R + WARM):
        a = time.perf_counter()
        for _ in range(T):
            stored, env_act = h.predict_actions(obs)
            rew, term, trunc, tobs = env.step(env_act)
            nobs = env.obs()
            h.ext_push(obs, stored, rew, term, trunc, nobs, tobs if trunc.any() else None)
            obs = nobs
        b = time.perf_counter()
        if r >= WARM:
            wall.append((b - a) / T * 1e6)
    report(label, E, wall, None)
    h.close()


for E in (64, 1024, 16384):
    device("(a) reacher3 plug-in, fused", E, pkg.host.ModuleEnv("", pkg.describe_env_module(ENVS / "reacher3_plugin.hsaco"), 100), ENVS / "reacher3_plugin.hsaco")
    device("(b) reacher3 plug-in, plain", E, pkg.host.ModuleEnv("", pkg.describe_env_module(ENVS / "reacher3_plugin.hsaco"), 100), ENVS / "reacher3_plugin.hsaco", plain=True)
    device("(c) Pendulum twin plug-in", E, pkg.host.ModuleEnv("", pkg.describe_env_module(ENVS / "pendulum_plugin.hsaco"), 200), ENVS / "pendulum_plugin.hsaco")
    device("(d) built-in Pendulum", E, pkg.PendulumEnv())
    host("(e) reacher3 on the host", E)
