#!/usr/bin/env python3
"""Population scaling on the README quick-start shape (CartPole, 4 envs x 2048 steps, batch 64, 10 epochs): wall time per iteration of dril_population_train for
P members against the same P handles trained one after the other with dril_train, in the same process and alternating the two forms; plus the HIP-event time of
the two batched kernels (cfg.profile_events).  Host clock around calls that end in a synchronise; WARMUP iterations, then the median of REPS.

usage: tools/population_scaling.py [--out profiles/population_scaling.json] [--reps 10] [--warmup 3] [--sizes 1,2,4,8,16,32,64]
Prints a markdown table (docs/population.md) and writes the raw numbers as JSON.  Needs an MI355X."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "population_scaling.json"))
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sizes", default="1,2,4,8,16,32,64")
a = ap.parse_args()
pkg = g.load_package()
capi = pkg._capi
E, T = 4, 2048
N = E * T


def handles(P, seed0):
    hs = []
    for m in range(P):
        c = capi.default_config(capi.ENV_CARTPOLE)
        c.n_envs, c.n_steps, c.batch_size, c.epochs, c.seed, c.profile_events = E, T, 64, 10, seed0 + m, 1
        h = pkg.Handle(c)
        layer = pkg.ActorCriticLayer(pkg.CartPoleEnv().observation_space(), pkg.CartPoleEnv().action_space())
        h.set_params(pkg.flatten_params(layer.initialparameters(__import__("numpy").random.default_rng(seed0 + m))))
        h.env_reset(seed0 + m)
        hs.append(h)
    return hs


rows = []
for P in [int(x) for x in a.sizes.split(",")]:
    solo, joined = handles(P, 1000), handles(P, 1000)
    t_pop, t_ser, ms_roll, ms_upd, solo_members = [], [], [], [], 0
    with pkg.Population(joined) as pop:
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            pop.train(N)
            t1 = time.perf_counter()
            for h in solo:
                h.train(N)
            t2 = time.perf_counter()
            if it >= a.warmup:
                i = pop.info()
                t_pop.append(t1 - t0); t_ser.append(t2 - t1); ms_roll.append(i["last_rollout_ms"]); ms_upd.append(i["last_update_ms"])
                solo_members += i["last_solo_rollouts"] + i["last_solo_updates"]
        info = pop.info()
    same = all((x.get_params() == y.get_params()).all() for x, y in zip(solo, joined))
    for h in solo + joined:
        h.close()
    med = statistics.median
    rows.append(dict(P=P, population_ms=1e3 * med(t_pop), serial_ms=1e3 * med(t_ser), rollout_kernel_ms=med(ms_roll), update_kernel_ms=med(ms_upd), cap=info["cap"],
                     update_launches_per_iteration=info["last_update_launches"], members_run_solo=solo_members, bit_equal=bool(same),
                     population_ms_all=[1e3 * t for t in t_pop], serial_ms_all=[1e3 * t for t in t_ser]))
    print(f"P={P}: population {rows[-1]['population_ms']:.2f} ms, serial {rows[-1]['serial_ms']:.2f} ms per iteration", file=sys.stderr, flush=True)
print("| P | population, ms / iteration | P x dril_train, ms | speed-up | rollout kernel, ms | update kernel, ms | host + small launches, ms | update launches | run solo | bit-equal |")
print("|--:|--:|--:|--:|--:|--:|--:|--:|--:|:--|")
for r in rows:
    rest = r["population_ms"] - r["rollout_kernel_ms"] - r["update_kernel_ms"]
    print(f"| {r['P']} | {r['population_ms']:.2f} | {r['serial_ms']:.2f} | {r['serial_ms'] / r['population_ms']:.2f} | {r['rollout_kernel_ms']:.2f} | {r['update_kernel_ms']:.2f} | {rest:.2f} | "
          f"{r['update_launches_per_iteration']} | {r['members_run_solo']} | {'yes' if r['bit_equal'] else 'NO'} |")
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text(json.dumps(dict(shape=dict(env="CartPole", n_envs=E, n_steps=T, batch_size=64, epochs=10), warmup=a.warmup, reps=a.reps, rows=rows), indent=1) + "\n")
