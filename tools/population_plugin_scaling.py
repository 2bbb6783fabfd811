#!/usr/bin/env python3
"""Populations of device env plug-in handles (docs/population.md, "Plug-in members") against the same handles trained one after the other: wall time of one
iteration (collection + GAE + update) on the reacher3 plug-in at the README shape (4 envs x 2048 steps, 10 epochs, hidden [64,64] tanh), batch_size 64 and 32,
P members —
  * dril_population_train on P members (one dril_env_plugin_rollout_pop launch + one ppo_update_generic_small_pop_kernel launch per chunk),
  * P x dril_train with both opt-ins on (dril_rollout_fused_enable + dril_update_fused_enable: the members' own solo route),
  * P x dril_train on the default routes (step-granular collection, per-step update)
— in the same process, the three forms alternating, WARMUP iterations, then the median of REPS with min and max; and the HIP-event time of the two batched kernels
(cfg.profile_events) on a population of its own.  The members of the population and the opt-in solo handles start from the same seeds and parameters: their
parameters are compared byte for byte at the end.

usage: tools/population_plugin_scaling.py [--out profiles/population_plugin_scaling.json] [--members 1,8,64] [--batch 64,32] [--reps 10] [--warmup 3]
Prints a markdown table (docs/population.md) and writes the raw numbers as JSON.  Needs an MI355X."""
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
ap.add_argument("--out", default=str(ROOT / "profiles" / "population_plugin_scaling.json"))
ap.add_argument("--members", default="1,8,64")
ap.add_argument("--batch", default="64,32")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()
pkg = g.load_package()
capi = pkg._capi
E, T, EPOCHS, HIDDEN = 4, 2048, 10, (64, 64)
N = E * T
med = statistics.median
CO = ROOT / "examples" / "envs" / "reacher3_pop_plugin.hsaco"
SPREAD = 0.03   # the box-to-box spread the README records


def make(B, P, optin, events=False):
    hs = []
    for m in range(P):
        c = capi.default_config(capi.ENV_MODULE)
        c.n_envs, c.n_steps, c.batch_size, c.epochs, c.seed, c.profile_events = E, T, B, EPOCHS, 7 + m, int(events)
        c.n_hidden, c.activation = len(HIDDEN), 0
        for l, w in enumerate(HIDDEN):
            c.hidden[l] = w
        h = pkg.Handle(c, env_module=str(CO))
        if optin:
            h.rollout_fused_enable(True); h.update_fused_enable(True)
        h.set_params((np.random.default_rng(100 + m).standard_normal(h.P) * 0.1).astype(np.float32))
        h.env_reset(7 + m)
        hs.append(h)
    return hs


def timed(f):
    t0 = time.perf_counter(); f(); return 1e3 * (time.perf_counter() - t0)


rows = []
for B in [int(x) for x in a.batch.split(",")]:
    for P in [int(x) for x in a.members.split(",")]:
        members, opt, dflt = make(B, P, True), make(B, P, True), make(B, P, False)
        t_pop, t_opt, t_def = [], [], []
        with pkg.Population(members) as pop:
            for it in range(a.warmup + a.reps):
                x = timed(lambda: pop.train(N))
                y = timed(lambda: [h.train(N) for h in opt])
                z = timed(lambda: [h.train(N) for h in dflt])
                if it >= a.warmup:
                    t_pop.append(x); t_opt.append(y); t_def.append(z)
            info = pop.info()
        equal = all(np.array_equal(m.get_params().view(np.uint32), s.get_params().view(np.uint32)) for m, s in zip(members, opt))
        for h in members + opt + dflt:
            h.close()
        ev = make(B, P, True, events=True)
        with pkg.Population(ev) as pop:
            pop.train(N); pop.train(N)
            ei = pop.info()
        for h in ev:
            h.close()
        best = min(med(t_opt), med(t_def))
        rows.append(dict(batch_size=B, members=P, optimiser_steps=EPOCHS * -(-N // B), population_ms=med(t_pop), population_min=min(t_pop), population_max=max(t_pop),
                         solo_optin_ms=med(t_opt), solo_optin_min=min(t_opt), solo_optin_max=max(t_opt), solo_default_ms=med(t_def), solo_default_min=min(t_def),
                         solo_default_max=max(t_def), speedup_vs_faster_yardstick=best / med(t_pop), rollout_kernel_ms=ei["last_rollout_ms"], update_kernel_ms=ei["last_update_ms"],
                         rollout_launches=int(info["last_rollout_launches"]), update_launches=int(info["last_update_launches"]), run_solo=int(info["total_solo_rollouts"] + info["total_solo_updates"]),
                         bit_equal=bool(equal), population_ms_all=t_pop, solo_optin_ms_all=t_opt, solo_default_ms_all=t_def))
        r = rows[-1]
        print(f"B={B} P={P}: population {r['population_ms']:.2f} ms, P x opt-in {r['solo_optin_ms']:.2f} ms, P x default {r['solo_default_ms']:.2f} ms, kernels {r['rollout_kernel_ms']:.2f} + "
              f"{r['update_kernel_ms']:.2f} ms, bit-equal {equal}", file=sys.stderr, flush=True)

print("| B | P | population, ms (min - max) | P x dril_train, opt-ins on, ms (min - max) | P x dril_train, default routes, ms (min - max) | speed-up over the faster | rollout kernel, ms | update kernel, ms | launches | run solo | bit-equal |")
print("|--:|--:|--:|--:|--:|--:|--:|--:|--:|--:|:--|")
for r in rows:
    print(f"| {r['batch_size']} | {r['members']} | {r['population_ms']:.2f} ({r['population_min']:.2f} - {r['population_max']:.2f}) | {r['solo_optin_ms']:.2f} ({r['solo_optin_min']:.2f} - {r['solo_optin_max']:.2f}) | "
          f"{r['solo_default_ms']:.2f} ({r['solo_default_min']:.2f} - {r['solo_default_max']:.2f}) | {r['speedup_vs_faster_yardstick']:.2f} | {r['rollout_kernel_ms']:.2f} | {r['update_kernel_ms']:.2f} | "
          f"{r['rollout_launches']} + {r['update_launches']} | {r['run_solo']} | {'yes' if r['bit_equal'] else 'NO'} |")
verdict = {}
for r in rows:
    if r["members"] == 8:
        verdict[f"P=8 B={r['batch_size']} beats the faster yardstick by more than {SPREAD:.0%}"] = bool(r["speedup_vs_faster_yardstick"] > 1 + SPREAD)
    if r["members"] == 1:
        verdict[f"P=1 B={r['batch_size']} within {SPREAD:.0%} of the solo opt-in iteration"] = bool(abs(r["population_ms"] / r["solo_optin_ms"] - 1) <= SPREAD)
print()
for k, v in verdict.items():
    print(f"{k}: {'holds' if v else 'MISSED'}")
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text(json.dumps(dict(shape=dict(n_envs=E, n_steps=T, epochs=EPOCHS, hidden=list(HIDDEN), plugin="reacher3"), warmup=a.warmup, reps=a.reps, rows=rows, pass_rule=verdict), indent=1) + "\n")
