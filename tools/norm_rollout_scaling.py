#!/usr/bin/env python3
"""The one-launch collection of a normalising built-in handle (dril_norm_rollout_enable, rollout_norm_kernel) against the step-granular collection of the same
handle: wall time of dril_collect_rollout on Pendulum and CartPole, norm_obs = norm_reward = 1, T = 2048, at E = 4 .. 128 envs — the same process, the two forms
alternating, WARMUP collections, then the median of REPS with min and max — and the HIP-event time of the collection (cfg.profile_events) in calls of their own.
Population rows: P members of the README shape (Pendulum, 4 envs x 2048 steps, batch 64, 10 epochs) under the normaliser, dril_population_train against
P x dril_train with and without the opt-in.

usage: tools/norm_rollout_scaling.py [--out profiles/norm_rollout_scaling.json] [--reps 10] [--warmup 3] [--envs 4,8,32,64,128] [--members 1,8,64]
Prints two markdown tables (docs/normalized_rollout.md) and writes the raw numbers as JSON.  Needs an MI355X."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "norm_rollout_scaling.json"))
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--envs", default="4,8,32,64,128")
ap.add_argument("--members", default="1,8,64")
a = ap.parse_args()
pkg = g.load_package()
capi = pkg._capi
T = 2048
KINDS = {"Pendulum": (capi.ENV_PENDULUM, pkg.PendulumEnv), "CartPole": (capi.ENV_CARTPOLE, pkg.CartPoleEnv)}
med = statistics.median


def handle(kind, E, seed, optin):
    c = capi.default_config(KINDS[kind][0])
    c.n_envs, c.n_steps, c.batch_size, c.epochs, c.seed, c.profile_events = E, T, 64, 10, seed, 1
    c.norm_obs = c.norm_reward = c.norm_training = 1
    h = pkg.Handle(c)
    env = KINDS[kind][1]()
    layer = pkg.ActorCriticLayer(env.observation_space(), env.action_space())
    h.set_params(pkg.flatten_params(layer.initialparameters(np.random.default_rng(seed))))
    h.env_reset(seed)
    if optin:
        h.norm_rollout_enable(True)
    return h


def timed(f):
    t0 = time.perf_counter(); f(); return 1e3 * (time.perf_counter() - t0)


def event_ms(h, calls=3):
    h.profile_reset()
    for _ in range(calls):
        h.collect_rollout()
    p = h.profile()[h.lib.dril_kernel_name(capi.K_ROLLOUT).decode()]
    return p["total_ms"] / max(p["launches"], 1)


rows = []
for kind in KINDS:
    for E in [int(x) for x in a.envs.split(",")]:
        one, step = handle(kind, E, 7, True), handle(kind, E, 7, False)
        t_one, t_step = [], []
        for it in range(a.warmup + a.reps):
            x, y = timed(one.collect_rollout), timed(step.collect_rollout)
            if it >= a.warmup:
                t_one.append(x); t_step.append(y)
        io, is_ = one.norm_rollout_info(), step.norm_rollout_info()
        same = all((one.buffer(w).view(np.uint8) == step.buffer(w).view(np.uint8)).all() for w in (capi.BUF_OBSERVATIONS, capi.BUF_ACTIONS, capi.BUF_REWARDS, capi.BUF_LOGPROBS, capi.BUF_FLAGS))
        ev_one, ev_step = event_ms(one), event_ms(step)
        rows.append(dict(env=kind, n_envs=E, n_steps=T, one_launch_ms=med(t_one), one_launch_min=min(t_one), one_launch_max=max(t_one), step_granular_ms=med(t_step),
                         step_granular_min=min(t_step), step_granular_max=max(t_step), one_launch_event_ms=ev_one, step_granular_event_ms=ev_step,
                         one_launch_launches=io["last_collection_launches"], step_granular_launches=is_["last_collection_launches"], path=io["last_collection_path"], bit_equal=bool(same),
                         one_launch_ms_all=t_one, step_granular_ms_all=t_step))
        print(f"{kind} E={E}: one launch {rows[-1]['one_launch_ms']:.2f} ms, step-granular {rows[-1]['step_granular_ms']:.2f} ms", file=sys.stderr, flush=True)
        one.close(); step.close()

pop_rows = []
E0, N0 = 4, 4 * T
for P in [int(x) for x in a.members.split(",")]:
    joined, solo, plain = ([handle("Pendulum", E0, 1000 + m, o) for m in range(P)] for o in (True, True, False))
    t_pop, t_ser, t_plain = [], [], []
    with pkg.Population(joined) as pop:
        for it in range(a.warmup + a.reps):
            x = timed(lambda: pop.train(N0))
            y = timed(lambda: [h.train(N0) for h in solo])
            z = timed(lambda: [h.train(N0) for h in plain])
            if it >= a.warmup:
                t_pop.append(x); t_ser.append(y); t_plain.append(z)
        info = pop.info()
    same = all((x.get_params() == y.get_params()).all() for x, y in zip(solo, joined))
    for h in joined + solo + plain:
        h.close()
    pop_rows.append(dict(P=P, population_ms=med(t_pop), serial_one_launch_ms=med(t_ser), serial_step_granular_ms=med(t_plain), rollout_launches_per_iteration=info["last_rollout_launches"],
                         update_launches_per_iteration=info["last_update_launches"], members_run_solo=info["total_solo_rollouts"] + info["total_solo_updates"], bit_equal=bool(same),
                         population_ms_all=t_pop, serial_one_launch_ms_all=t_ser, serial_step_granular_ms_all=t_plain))
    print(f"P={P}: population {pop_rows[-1]['population_ms']:.2f} ms, P x dril_train {pop_rows[-1]['serial_one_launch_ms']:.2f} ms (opt-in) / {pop_rows[-1]['serial_step_granular_ms']:.2f} ms (step-granular)", file=sys.stderr, flush=True)

print("| env | E | one launch, ms (min - max) | step-granular, ms (min - max) | speed-up | events: one launch, ms | events: step-granular, ms | launches | bit-equal |")
print("|:--|--:|--:|--:|--:|--:|--:|--:|:--|")
for r in rows:
    print(f"| {r['env']} | {r['n_envs']} | {r['one_launch_ms']:.2f} ({r['one_launch_min']:.2f} - {r['one_launch_max']:.2f}) | {r['step_granular_ms']:.2f} ({r['step_granular_min']:.2f} - {r['step_granular_max']:.2f}) | "
          f"{r['step_granular_ms'] / r['one_launch_ms']:.1f} | {r['one_launch_event_ms']:.2f} | {r['step_granular_event_ms']:.2f} | {r['one_launch_launches']} vs {r['step_granular_launches']} | {'yes' if r['bit_equal'] else 'NO'} |")
print()
print("| P | population, ms / iteration | P x dril_train with the opt-in, ms | P x dril_train step-granular, ms | speed-up over the opt-in | over step-granular | collection launches | run solo | bit-equal |")
print("|--:|--:|--:|--:|--:|--:|--:|--:|:--|")
for r in pop_rows:
    print(f"| {r['P']} | {r['population_ms']:.2f} | {r['serial_one_launch_ms']:.2f} | {r['serial_step_granular_ms']:.2f} | {r['serial_one_launch_ms'] / r['population_ms']:.2f} | "
          f"{r['serial_step_granular_ms'] / r['population_ms']:.2f} | {r['rollout_launches_per_iteration']} | {r['members_run_solo']} | {'yes' if r['bit_equal'] else 'NO'} |")
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text(json.dumps(dict(shape=dict(n_steps=T, norm_obs=1, norm_reward=1, batch_size=64, epochs=10), warmup=a.warmup, reps=a.reps, rows=rows, population_rows=pop_rows), indent=1) + "\n")
