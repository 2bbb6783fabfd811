#!/usr/bin/env python3
"""SAC over external envs whose arrays are on the device: wall time per env step of {act + push + gradient_steps updates}, the host verbs beside the device verbs,
in the same process and run.

  host verbs     dril_sac_predict_actions + dril_sac_ext_push + dril_sac_update on host arrays: the loop of _sac_train_host (three host waits and two PCIe round
                 trips per env step)
  device verbs   dril_sac_ext_act_device + dril_sac_ext_push_device + dril_sac_update_enqueue on device arrays, dril_sac_flush when the pending table would
                 overflow and once at the end of the window — the clock stops after that drain, so the figure is work done, not work enqueued
The env is scripted device / host arrays (no simulator): obs [3], Box(-2, 2) of one dimension, hidden [512, 512], batch 256.  Per cell: a warm-up window, then 5 runs of
STEPS env steps each, host and device alternating; the median run's wall time / STEPS in microseconds (min .. max of the 5).
usage: python tools/sac_ext_latency.py [--steps 200]"""
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
D, A, HID, BATCH, RUNS = 3, 1, (512, 512), 256, 5
STEPS = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 200
clock = time.perf_counter
fmt = lambda xs: f"{statistics.median(xs) * 1e6 / STEPS:7.1f} ({min(xs) * 1e6 / STEPS:6.1f} .. {max(xs) * 1e6 / STEPS:6.1f})"


class _Spaces:
    kind = capi.ENV_EXTERNAL

    def observation_space(self):
        return pkg.Box(low=(-1.0, -1.0, -8.0), high=(1.0, 1.0, 8.0))

    def action_space(self):
        return pkg.Box(low=(-2.0,), high=(2.0,))


def make(E, gs):
    env = _Spaces()
    alg = pkg.SAC(batch_size=BATCH, buffer_capacity=max(100_000, 4 * E), gradient_steps=gs)
    h = pkg.SacHandle(pkg.make_sac_config(env, E, alg, pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=HID), seed=1))
    h.set_params((np.random.default_rng(0).standard_normal(h.P) * 0.05).astype(np.float32))
    return h


print(f"| E | gradient_steps | host verbs, us / env step | device verbs, us / env step | host / device | launches per act + push | flushes per {STEPS} steps |")
print("|---|---|---|---|---|---|---|")
for E in (64, 4096):
    rng = np.random.default_rng(E)
    obs, nobs = (rng.uniform(-1, 1, (E, D)).astype(np.float32) for _ in range(2))
    rew, fl = rng.standard_normal(E).astype(np.float32), np.zeros(E, np.uint8)
    s = hip_mem.Stream()
    d_obs, d_nobs, d_rew, d_fl = (hip_mem.to_device(x) for x in (obs, nobs, rew, fl))
    d_env = hip_mem.empty((E, A), np.float32)
    for gs in (1, 8):
        hh, hd = make(E, gs), make(E, gs)

        def host_window(n):
            a = clock()
            for _ in range(n):
                stored, _ = hh.predict_actions(obs)
                hh.ext_push(obs, stored, rew, fl, fl, nobs)
                hh.update(gs)
            return clock() - a

        def device_window(n):
            cap, pending = capi.SAC_PENDING_CAPACITY, 0
            a = clock()
            for _ in range(n):
                hd.ext_act_device(d_obs, False, None, None, d_env, s.ptr)
                hd.ext_push_device(d_rew, d_fl, d_fl, d_nobs, None, s.ptr)
                if pending + gs > cap:
                    hd.flush(); pending = 0
                hd.update_enqueue(gs); pending += gs
            hd.flush()
            s.synchronize()
            return clock() - a

        host_window(20); device_window(20)                                            # warm-up: code objects, scratch, the pending table
        i0 = hd.ext_device_info()
        th, td = [], []
        for _ in range(RUNS):
            th.append(host_window(STEPS)); td.append(device_window(STEPS))
        i1 = hd.ext_device_info()
        assert i1["host_syncs"] == 0 and i1["steps_device"] - i0["steps_device"] == RUNS * STEPS, i1
        print(f"| {E} | {gs} | {fmt(th)} | {fmt(td)} | {statistics.median(th) / statistics.median(td):.2f} | "
              f"{(i1['launches'] - i0['launches']) / (RUNS * STEPS):.0f} | {(i1['flushes'] - i0['flushes']) / RUNS:.0f} |", flush=True)
        hh.close(); hd.close()
