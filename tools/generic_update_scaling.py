#!/usr/bin/env python3
"""The one-launch update of a generic handle (dril_update_fused_enable, ppo_update_generic_small_kernel) against the per-step route of the same handle: wall time
of dril_ppo_update at the README shape (4 envs x 2048 steps, 10 epochs) on the reacher3 plug-in, CartPole under DRIL_FORCE_GENERIC, a built-in at [32,48] relu and
four-layer nets at the kernel's parameter cap, each at batch_size 64 and 32, then batch_size 8 — the same process, the two forms alternating, WARMUP updates, then the median of REPS with
min and max — and the HIP-event time of the update (cfg.profile_events, the sum over the bracketed kernel classes) on handles of their own.  One row times the whole
dril_train iteration.

usage: tools/generic_update_scaling.py [--out profiles/generic_update_scaling.json] [--reps 10] [--warmup 3]
Prints a markdown table (docs/generic_update.md) and writes the raw numbers as JSON.  Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "generic_update_scaling.json"))
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()
pkg = g.load_package()
capi = pkg._capi
E, T, EPOCHS = 4, 2048, 10
N = E * T
med = statistics.median
REACHER = ROOT / "examples" / "envs" / "reacher3_plugin.hsaco"


def base_cfg(kind, B, hidden, act, events):
    c = capi.default_config(kind)
    c.n_envs, c.n_steps, c.batch_size, c.epochs, c.seed, c.profile_events = E, T, B, EPOCHS, 7, int(events)
    c.n_hidden, c.activation = len(hidden), act
    for l, w in enumerate(hidden):
        c.hidden[l] = w
    c.hidden1, c.hidden2 = hidden[0], hidden[min(1, len(hidden) - 1)]
    return c


def make(shape, B, optin, events=False):
    """a handle of the shape with one rollout in its buffer"""
    kind, hidden, act = shape["kind"], shape["hidden"], shape["act"]
    if shape.get("force_generic"):
        os.environ["DRIL_FORCE_GENERIC"] = "1"
    try:
        if kind == "reacher3":
            h = pkg.Handle(base_cfg(capi.ENV_MODULE, B, hidden, act, events), env_module=REACHER)
        elif kind == "external":
            c = base_cfg(capi.ENV_EXTERNAL, B, hidden, act, events)
            c.ext_obs_dim, c.ext_action_dim, c.ext_discrete, c.ext_action_low, c.ext_action_high = shape["D"], shape["A"], 0, -1.0, 1.0
            h = pkg.Handle(c)
        else:
            h = pkg.Handle(base_cfg(getattr(capi, "ENV_" + kind.upper()), B, hidden, act, events))
    finally:
        os.environ.pop("DRIL_FORCE_GENERIC", None)
    rng = np.random.default_rng(3)
    h.set_params((rng.standard_normal(h.P) * 0.1).astype(np.float32))
    if kind == "external":
        for w, arr in ((capi.BUF_OBSERVATIONS, rng.standard_normal((N, h.D))), (capi.BUF_ACTIONS, rng.normal(0, 1, (N, h.A))), (capi.BUF_ADVANTAGES, rng.standard_normal(N)),
                       (capi.BUF_RETURNS, rng.standard_normal(N)), (capi.BUF_VALUES, rng.standard_normal(N))):
            h.set_buffer(w, arr.astype(np.float32))
        lp = h.evaluate_actions(h.buffer(capi.BUF_OBSERVATIONS), h.buffer(capi.BUF_ACTIONS))[1]
        h.set_buffer(capi.BUF_LOGPROBS, (lp + 0.1 * rng.standard_normal(N)).astype(np.float32))
    else:
        h.env_reset(7); h.collect_rollout()
    if optin:
        h.update_fused_enable(True)
    return h


def timed(f):
    t0 = time.perf_counter(); r = f(); return 1e3 * (time.perf_counter() - t0), r


def event_ms(h, calls=2):
    h.profile_reset()
    for _ in range(calls):
        h.ppo_update()
    return sum(p["total_ms"] for name, p in h.profile().items() if name not in ("rollout_kernel", "gae_kernel")) / calls


SHAPES = [
    dict(name="reacher3 plug-in [64,64] tanh", kind="reacher3", hidden=(64, 64), act=0),
    dict(name="CartPole, DRIL_FORCE_GENERIC [64,64] tanh", kind="cartpole", hidden=(64, 64), act=0, force_generic=True),
    dict(name="Pendulum [32,48] relu", kind="pendulum", hidden=(32, 48), act=1),
    dict(name="external D=16 A=8 [40,40,40,36] tanh (P = 11 213)", kind="external", hidden=(40, 40, 40, 36), act=0, D=16, A=8),
    dict(name="external D=16 A=8 [40,40,40,36] gelu (P = 11 213)", kind="external", hidden=(40, 40, 40, 36), act=6, D=16, A=8),
]
rows = []
for shape, B in [(s, 64) for s in SHAPES] + [(s, 32) for s in SHAPES] + [(SHAPES[0], 8)]:
    one, step = make(shape, B, True), make(shape, B, False)
    t_one, t_step, n_upd = [], [], 0
    for it in range(a.warmup + a.reps):
        (x, so), (y, ss) = timed(one.ppo_update), timed(step.ppo_update)
        assert so.n_updates == ss.n_updates and not so.nan_or_inf
        n_upd = so.n_updates
        if it >= a.warmup:
            t_one.append(x); t_step.append(y)
    info = one.update_fused_info()
    assert info["last_update_path"] == 1 and step.update_fused_info()["last_update_path"] == 0
    one.close(); step.close()
    eo, es = make(shape, B, True, events=True), make(shape, B, False, events=True)
    ev_one, ev_step = event_ms(eo), event_ms(es)
    P_shape = es.P
    # launches of the per-step route, read off generic_ppo_grad / run_backward_both / ppo_step: per optimiser step the gather, nh + 1 forward layers, the loss head,
    # 2 nh + 1 reverse stages, grad_reduce_kernel and adam_kernel; per epoch the moments pass (2 <= minibatches <= 2048)
    nh, nb = len(shape["hidden"]), -(-N // B)
    step_launches = n_upd * (3 * nh + 6) + (EPOCHS if 2 <= nb <= 2048 else 2 * n_upd)
    eo.close(); es.close()
    us = lambda ms: 1e3 * ms / n_upd
    rows.append(dict(shape=shape["name"], batch_size=B, P=P_shape, optimiser_steps=n_upd, one_launch_ms=med(t_one), one_launch_min=min(t_one), one_launch_max=max(t_one),
                     per_step_ms=med(t_step), per_step_min=min(t_step), per_step_max=max(t_step), one_launch_us_per_step=us(med(t_one)), per_step_us_per_step=us(med(t_step)),
                     one_launch_event_ms=ev_one, per_step_event_ms=ev_step, one_launch_launches=int(info["last_update_launches"]), per_step_launches=int(step_launches),
                     steps_per_launch=int(info["steps_per_launch"]), one_launch_ms_all=t_one, per_step_ms_all=t_step))
    print(f"{shape['name']} B={B}: one launch {rows[-1]['one_launch_ms']:.2f} ms ({rows[-1]['one_launch_us_per_step']:.1f} us/step), per step {rows[-1]['per_step_ms']:.2f} ms "
          f"({rows[-1]['per_step_us_per_step']:.1f} us/step)", file=sys.stderr, flush=True)

# the whole dril_train iteration (collection + GAE + update) of the README shape on the plug-in
one, step = make(SHAPES[0], 64, True), make(SHAPES[0], 64, False)
t_one, t_step = [], []
for it in range(a.warmup + a.reps):
    x, y = timed(lambda: one.train(N))[0], timed(lambda: step.train(N))[0]
    if it >= a.warmup:
        t_one.append(x); t_step.append(y)
one.close(); step.close()
train_row = dict(shape=SHAPES[0]["name"], batch_size=64, one_launch_ms=med(t_one), one_launch_min=min(t_one), one_launch_max=max(t_one), per_step_ms=med(t_step), per_step_min=min(t_step),
                 per_step_max=max(t_step), one_launch_ms_all=t_one, per_step_ms_all=t_step)

print("| shape | B | optimiser steps | one launch, ms (min - max) | per step, ms (min - max) | speed-up | us / step: one launch | per step | events: one launch, ms | per step, ms | launches |")
print("|:--|--:|--:|--:|--:|--:|--:|--:|--:|--:|--:|")
for r in rows:
    print(f"| {r['shape']} | {r['batch_size']} | {r['optimiser_steps']} | {r['one_launch_ms']:.2f} ({r['one_launch_min']:.2f} - {r['one_launch_max']:.2f}) | "
          f"{r['per_step_ms']:.2f} ({r['per_step_min']:.2f} - {r['per_step_max']:.2f}) | {r['per_step_ms'] / r['one_launch_ms']:.2f} | {r['one_launch_us_per_step']:.1f} | {r['per_step_us_per_step']:.1f} | "
          f"{r['one_launch_event_ms']:.2f} | {r['per_step_event_ms']:.2f} | {r['one_launch_launches']} vs {r['per_step_launches']} |")
print()
print(f"dril_train, one iteration, {train_row['shape']}, B = 64: one launch {train_row['one_launch_ms']:.2f} ms ({train_row['one_launch_min']:.2f} - {train_row['one_launch_max']:.2f}), "
      f"per step {train_row['per_step_ms']:.2f} ms ({train_row['per_step_min']:.2f} - {train_row['per_step_max']:.2f}), speed-up {train_row['per_step_ms'] / train_row['one_launch_ms']:.2f}")
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text(json.dumps(dict(shape=dict(n_envs=E, n_steps=T, epochs=EPOCHS), warmup=a.warmup, reps=a.reps, rows=rows, train_iteration=train_row), indent=1) + "\n")
