#!/usr/bin/env python3
"""External-env boundary cost (DRIL_ENV_EXTERNAL): the library's share of one env step, host verbs beside device verbs, in the same process and run.

  host verbs     dril_ext_act / dril_ext_record on host arrays: wall time of the call (obs in over PCIe, forward + sampling, actions back, one drain; record: the
                 staging copy, and on a truncation step the gather / critic forward / two drains)
  device verbs   dril_ext_act_device / dril_ext_record_device on device arrays.  Two figures per verb: `enqueue` = wall time of the call (it returns without
                 waiting), `done` = call + a drain of the caller's stream by THIS TOOL, i.e. the time until the actions could be consumed — the figure to hold
                 against the host verb, whose call includes its drain.  `record+tobs`: a step in which d_terminal_obs is passed (the extra critic forward over all E).
obs [24], Box(4), hidden [64,64]; per verb the median (min .. max) in us over the T = 64 steps of the second rollout (the first warms up).  No env is stepped.
usage: python tools/ext_latency.py [--update]      (--update: also time one PPO update, as the tool did before)"""
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
D, A, H, T = 24, 4, 64, 64
fmt = lambda xs: f"{statistics.median(xs) * 1e6:6.1f} ({min(xs) * 1e6:5.1f} .. {max(xs) * 1e6:6.1f})"
clock = time.perf_counter
print("| E | host act | host record | host record, truncated | device act: enqueue | device act: done | device record: enqueue | device record: done | device record+tobs: done |")
print("|---|---|---|---|---|---|---|---|---|")
for E in (64, 1024, 16384):
    c = capi.default_config(capi.ENV_EXTERNAL)
    c.ext_obs_dim, c.ext_action_dim, c.ext_discrete, c.hidden1, c.hidden2 = D, A, 0, H, H
    c.ext_action_low, c.ext_action_high = -1.0, 1.0
    c.n_envs, c.n_steps, c.batch_size, c.epochs = E, T, max(64, E * T // 32), 2
    h = pkg.Handle(c)
    rng = np.random.default_rng(0)
    h.set_params((rng.standard_normal(h.P) * 0.2).astype(np.float32))
    obs = rng.standard_normal((E, D)).astype(np.float32); rew = np.zeros(E, np.float32); fl = np.zeros(E, np.uint8)
    tr = fl.copy(); tr[::7] = 1
    s = hip_mem.Stream()
    d_obs, d_rew, d_fl, d_tr = (hip_mem.to_device(x) for x in (obs, rew, fl, tr))
    d_raw, d_env = hip_mem.empty((E, A), np.float32), hip_mem.empty((E, A), np.float32)
    for rep in range(2):                                                             # host verbs
        act, rec, rec_tr = [], [], []
        for t in range(T):
            a = clock(); h.ext_act(obs); b = clock(); act.append(b - a)
            if t % 8 == 7:
                h.ext_record(rew, fl, tr, obs); rec_tr.append(clock() - b)
            else:
                h.ext_record(rew, fl, fl); rec.append(clock() - b)
        h.ext_finish(obs)
    for rep in range(2):                                                             # device verbs
        d_act_q, d_act, d_rec_q, d_rec, d_rec_tr = [], [], [], [], []
        for t in range(T):
            a = clock(); h.ext_act_device(d_obs, d_raw, d_env, s.ptr); b = clock(); s.synchronize(); e = clock()
            d_act_q.append(b - a); d_act.append(e - a)
            a = clock()
            if t % 8 == 7:
                h.ext_record_device(d_rew, d_fl, d_tr, d_obs, s.ptr); s.synchronize(); d_rec_tr.append(clock() - a)
            else:
                h.ext_record_device(d_rew, d_fl, d_fl, None, s.ptr); b = clock(); s.synchronize(); e = clock()
                d_rec_q.append(b - a); d_rec.append(e - a)
        h.ext_finish_device(d_obs, s.ptr)
        info = h.ext_device_info()
        assert info["host_syncs"] == 0 and info["steps_device"] == T, info
    print(f"| {E} | " + " | ".join(fmt(x) for x in (act, rec, rec_tr, d_act_q, d_act, d_rec_q, d_rec, d_rec_tr)) + " |", flush=True)
    if "--update" in sys.argv:
        a = clock(); st = h.ppo_update(); t_upd = clock() - a
        print(f"    update {t_upd * 1e3:7.2f} ms for {st.n_updates} optimiser steps ({t_upd / max(st.n_updates, 1) * 1e6:6.1f} us each); launches of the last device rollout: {info['launches']}")
    h.close()
