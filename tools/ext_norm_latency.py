#!/usr/bin/env python3
"""What NormalizeWrapperEnv / MonitorWrapperEnv on a DRIL_ENV_EXTERNAL handle cost the device-array verbs (dril_ext_normalize_enable / dril_ext_monitor_enable,
docs/external_envs.md section 10, "Wrappers on device-resident arrays"): wall time per env step of dril_ext_act_device + dril_ext_record_device on scripted device arrays (no env is stepped), in us.

  off            no wrapper: the handle enqueues what it did before the wrappers existed
  normalise      dril_ext_normalize_enable (training, both halves)
  normalise+mon  and dril_ext_monitor_enable(100)
Every eighth step passes terminal observations (the extra critic forward).  obs [D], Box(4), hidden [64,64]; rollouts of T = 10 steps, so a run of 200 steps is 20
rollouts, each closed by dril_ext_finish_device: its drain is the only host wait, and the clock stops after the last one.  After one warm-up run per column, 5 runs
per column ALTERNATING in one process; median (min .. max).

usage: python tools/ext_norm_latency.py [--lib PATH] [--sizes E,E,...] [--dims D,D,...]
  --lib PATH   time the `off` column of ANOTHER build of libdril_hip.so (the parent commit's: it has the device verbs and not the wrappers) with the same loop"""
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
A, H, T, STEPS, RUNS = 4, 64, 10, 200, 5


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


other = arg("--lib", None)
lib = None
if other:                                                                            # another build: every verb it exports is typed (it may lack the newer ones)
    lib = C.CDLL(str(other))
    for name, (res, args) in capi._SIG.items():
        if hasattr(lib, name):
            fn = getattr(lib, name); fn.restype, fn.argtypes = res, args
sizes = [int(x) for x in arg("--sizes", "64,4096,65536").split(",")]
dims = [int(x) for x in arg("--dims", "3,64,300").split(",")]
columns = ("off",) if other else ("off", "normalise", "normalise+mon")
fmt = lambda xs: f"{statistics.median(xs):7.1f} ({min(xs):6.1f} .. {max(xs):7.1f})"


def make(E, D, column):
    c = capi.default_config(capi.ENV_EXTERNAL)
    c.ext_obs_dim, c.ext_action_dim, c.ext_discrete, c.hidden1, c.hidden2 = D, A, 0, H, H
    c.ext_action_low, c.ext_action_high = -1.0, 1.0
    c.n_envs, c.n_steps, c.batch_size, c.epochs = E, T, max(64, E * T // 32), 1
    h = pkg.Handle(c, lib) if lib is not None else pkg.Handle(c)
    h.set_params((np.random.default_rng(0).standard_normal(h.P) * 0.2).astype(np.float32))
    if column != "off":
        h.ext_normalize_enable()
    if column == "normalise+mon":
        h.ext_monitor_enable(100)
    return h


def run(h, dev):
    """STEPS env steps -> us per env step, the clock stopped after the last drain"""
    d_obs, d_rew, d_fl, d_tr, d_raw, d_env, s = dev
    t0 = time.perf_counter()
    for r in range(STEPS // T):
        for t in range(T):
            h.ext_act_device(d_obs, d_raw, d_env, s.ptr)
            if (r * T + t) % 8 == 7:
                h.ext_record_device(d_rew, d_fl, d_tr, d_obs, s.ptr)
            else:
                h.ext_record_device(d_rew, d_fl, d_fl, None, s.ptr)
        h.ext_finish_device(d_obs, s.ptr)
        info = h.ext_device_info()
        assert info["host_syncs"] == 0 and info["steps_device"] == T, info
    return (time.perf_counter() - t0) / STEPS * 1e6


print("| E | D | " + " | ".join(columns) + " |")
print("|---|---|" + "---|" * len(columns))
for E in sizes:
    for D in dims:
        rng = np.random.default_rng(E + D)
        obs = rng.standard_normal((E, D)).astype(np.float32); rew = rng.standard_normal(E).astype(np.float32); fl = np.zeros(E, np.uint8)
        tr = fl.copy(); tr[::7] = 1
        s = hip_mem.Stream()
        dev = tuple(hip_mem.to_device(x) for x in (obs, rew, fl, tr)) + (hip_mem.empty((E, A), np.float32), hip_mem.empty((E, A), np.float32), s)
        hs = {col: make(E, D, col) for col in columns}
        for col in columns:
            run(hs[col], dev)                                                        # warm-up
        us = {col: [] for col in columns}
        for _ in range(RUNS):
            for col in columns:                                                      # alternating
                us[col].append(run(hs[col], dev))
        print(f"| {E} | {D} | " + " | ".join(fmt(us[col]) for col in columns) + " |", flush=True)
        for h in hs.values():
            h.close()
