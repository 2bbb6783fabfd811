#!/usr/bin/env python3
"""What NormalizeWrapperEnv / MonitorWrapperEnv on a DRIL_ENV_EXTERNAL SAC handle cost the device-array verbs (dril_sac_ext_normalize_enable /
dril_sac_ext_monitor_enable, docs/sac.md last section): time per env step of dril_sac_ext_collection_begin + dril_sac_ext_act_device + dril_sac_ext_push_device on
scripted device arrays (no env is stepped, no gradient step), in us.

  off            no wrapper: the handle enqueues what it did before the wrappers existed
  normalise      dril_sac_ext_normalize_enable (training, both halves), a collection per step (train_freq = 1: every act is an opening act)
  normalise+mon  and dril_sac_ext_monitor_enable(100)
Two figures per cell, from two handles: `wall` — host clock over a run of 200 steps closed by one dril_sac_flush, the only host wait, on a handle WITHOUT
cfg.profile_events (what a training run enqueues) — and `event` — the HIP-event time of what act and push enqueue (a second handle with cfg.profile_events,
dril_sac_profile_get), which leaves out the gaps between launches of different calls; recording the four events costs that handle about 30 us of wall time per step.  Every eighth step passes terminal
observations.  obs [D], Box(1), hidden [64, 64] (the shape of examples/sac_torch_envs.py).  After one warm-up run per column, 5 runs per column ALTERNATING in one
process; median (min .. max).

usage: python tools/sac_ext_norm_latency.py [--lib PATH] [--sizes E,E,...] [--dims D,D,...]
  --lib PATH   time the `off` column of ANOTHER build of libdril_hip.so (the parent commit's: it has the device verbs and not the wrappers, and records no events on
               them, so its `event` figure is absent) with the same loop"""
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as g   # noqa: E402
import hip_mem                # noqa: E402  (device memory through ctypes on the HIP runtime: no torch needed)

pkg = g.load_package(); capi = pkg._capi
A, H, STEPS, RUNS = 1, 64, 200, 5


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


other = arg("--lib", None)
Handle = pkg.SacHandle
if other:                                                                            # another build: every verb it exports is typed (it lacks the newer ones)
    lib = C.CDLL(str(other))
    for name, (res, args) in capi._SIG.items():
        if hasattr(lib, name):
            fn = getattr(lib, name); fn.restype, fn.argtypes = res, args

    class Handle(pkg.SacHandle):
        @classmethod
        def _load(cls):
            return lib
sizes = [int(x) for x in arg("--sizes", "64,1024,4096,65536").split(",")]
dims = [int(x) for x in arg("--dims", "3,64,300").split(",")]
columns = ("off",) if other else ("off", "normalise", "normalise+mon")
fmt = lambda xs: f"{statistics.median(xs):6.1f} ({min(xs):5.1f} .. {max(xs):6.1f})"


class _Spaces:
    kind = capi.ENV_EXTERNAL

    def __init__(self, D):
        self.D = D

    def observation_space(self):
        return pkg.Box(low=(-10.0,) * self.D, high=(10.0,) * self.D)

    def action_space(self):
        return pkg.Box(low=(-2.0,) * A, high=(2.0,) * A)


def make(E, D, column, profile):
    env = _Spaces(D)
    alg = pkg.SAC(batch_size=256, buffer_capacity=max(8 * E, 4096))
    h = Handle(pkg.make_sac_config(env, E, alg, pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(H, H)), seed=1, profile_events=profile))
    h.set_params((np.random.default_rng(0).standard_normal(h.P) * 0.2).astype(np.float32))
    if column != "off":
        h.ext_normalize_enable()
    if column == "normalise+mon":
        h.ext_monitor_enable(100)
    return h


def run(h, dev, wrapped):
    """STEPS env steps -> (wall us per env step with the clock stopped after the drain, HIP-event us per env step or nan)"""
    d_obs, d_rew, d_fl, d_tr, d_env, s = dev
    h.profile_reset()
    t0 = time.perf_counter()
    for t in range(STEPS):
        if wrapped:
            h.ext_collection_begin()
        h.ext_act_device(d_obs, False, None, None, d_env, s.ptr)
        if t % 8 == 7:
            h.ext_push_device(d_rew, d_fl, d_tr, d_obs, d_obs, s.ptr)
        else:
            h.ext_push_device(d_rew, d_fl, d_fl, d_obs, None, s.ptr)
    h.flush()
    wall = (time.perf_counter() - t0) / STEPS * 1e6
    assert h.ext_device_info()["host_syncs"] == 0
    p = h.profile()
    return wall, (p["collect_ms"] / p["collect_steps"] * 1e3 if p["collect_steps"] else float("nan"))


print("| E | D | " + " | ".join(f"{c}: wall | {c}: event" for c in columns) + " |")
print("|---|---|" + "---|---|" * len(columns))
for E in sizes:
    for D in dims:
        rng = np.random.default_rng(E + D)
        obs = rng.standard_normal((E, D)).astype(np.float32); rew = rng.standard_normal(E).astype(np.float32); fl = np.zeros(E, np.uint8)
        tr = fl.copy(); tr[::7] = 1
        s = hip_mem.Stream()
        dev = tuple(hip_mem.to_device(x) for x in (obs, rew, fl, tr)) + (hip_mem.empty((E, A), np.float32), s)
        hs = {(col, prof): make(E, D, col, prof) for col in columns for prof in ((False,) if other else (False, True))}
        for (col, prof), h in hs.items():
            run(h, dev, col != "off")                                                # warm-up
        wall, ev = {col: [] for col in columns}, {col: [float("nan")] if other else [] for col in columns}
        for _ in range(RUNS):
            for (col, prof), h in hs.items():                                        # alternating
                w, e = run(h, dev, col != "off")
                if prof:
                    ev[col].append(e)
                else:
                    wall[col].append(w)
        print(f"| {E} | {D} | " + " | ".join(f"{fmt(wall[col])} | {fmt(ev[col])}" for col in columns) + " |", flush=True)
        for h in hs.values():
            h.close()
