#!/usr/bin/env python3
"""Population evaluation scaling on the README quick-start shape (CartPole, 4 envs, PPO defaults): wall time of one dril_population_evaluate_device call on P
members against the same P handles evaluated one after the other with dril_evaluate_agent_device, in the same process and alternating the two forms.  The members
are first trained for TRAIN iterations (as one population; the solo handles take the same parameters) so that episodes run to the 500-step limit; n_eval_episodes = 10,
the default K.  Host clock around calls that end in a synchronise; WARMUP calls, then the median of REPS (all samples are kept in the JSON).  kernel_ms is the
HIP-event time of the batched launches, taken in calls of their own on handles with cfg.profile_events (the timed handles have it off).

usage: tools/population_eval_scaling.py [--out profiles/population_eval_scaling.json] [--reps 10] [--warmup 3] [--train 30] [--sizes 1,2,4,8,16,32,64]
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
ap.add_argument("--out", default=str(ROOT / "profiles" / "population_eval_scaling.json"))
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--train", type=int, default=30)
ap.add_argument("--sizes", default="1,2,4,8,16,32,64")
a = ap.parse_args()
pkg = g.load_package()
capi = pkg._capi
np = __import__("numpy")
E, T, N_EVAL = 4, 2048, 10
N = E * T


def handles(P, seed0, profile_events=0):
    hs = []
    for m in range(P):
        c = capi.default_config(capi.ENV_CARTPOLE)
        c.n_envs, c.n_steps, c.batch_size, c.epochs, c.seed, c.profile_events = E, T, 64, 10, seed0 + m, profile_events
        h = pkg.Handle(c)
        layer = pkg.ActorCriticLayer(pkg.CartPoleEnv().observation_space(), pkg.CartPoleEnv().action_space())
        h.set_params(pkg.flatten_params(layer.initialparameters(np.random.default_rng(seed0 + m))))
        h.env_reset(seed0 + m)
        hs.append(h)
    return hs


def as_bytes(r):
    return (tuple(np.float64(r[0][k]).tobytes() for k in ("mean_reward", "std_reward", "mean_length", "std_length")), r[1].tobytes(), r[2].tobytes(), tuple(sorted(r[3].items())))


rows = []
for P in [int(x) for x in a.sizes.split(",")]:
    solo, joined = handles(P, 1000), handles(P, 1000)
    t_pop, t_ser, ms_k, launches, solo_members = [], [], [], [], 0
    with pkg.Population(joined) as pop:
        if a.train > 0:
            pop.train(a.train * N)
        for x, y in zip(solo, joined):                                     # the solo handles evaluate the same trained parameters
            x.set_params(y.get_params())
        same = True
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            rp = pop.evaluate(N_EVAL)
            t1 = time.perf_counter()
            rs = [h.evaluate_agent_device(N_EVAL) for h in solo]
            t2 = time.perf_counter()
            same = same and all(as_bytes(x) == as_bytes(y) for x, y in zip(rp, rs))
            if it >= a.warmup:
                i = pop.last_eval_info
                t_pop.append(t1 - t0); t_ser.append(t2 - t1); launches.append(i["launches"]); solo_members += i["solo_members"]
        mean_len = [r[0]["mean_length"] for r in rp]
    # kernel_ms in calls of their own, on a third set of handles with cfg.profile_events: the event records around every batched launch are host work the solo verb
    # does not do, so the timed calls above run without them
    profiled = handles(P, 1000, profile_events=1)
    for x, y in zip(profiled, joined):
        x.set_params(y.get_params())
    with pkg.Population(profiled) as pop:
        for it in range(a.warmup + a.reps):
            rq = pop.evaluate(N_EVAL)
            same = same and all(as_bytes(x) == as_bytes(y) for x, y in zip(rq, rp))
            if it >= a.warmup:
                ms_k.append(pop.last_eval_info["kernel_ms"])
    for h in solo + joined + profiled:
        h.close()
    med = statistics.median
    rows.append(dict(P=P, population_ms=1e3 * med(t_pop), serial_ms=1e3 * med(t_ser), population_ms_min=1e3 * min(t_pop), population_ms_max=1e3 * max(t_pop),
                     serial_ms_min=1e3 * min(t_ser), serial_ms_max=1e3 * max(t_ser), kernel_ms=med(ms_k), launches=int(med(launches)), members_run_solo=solo_members,
                     equal_to_solo=bool(same), mean_episode_length=mean_len, population_ms_all=[1e3 * t for t in t_pop], serial_ms_all=[1e3 * t for t in t_ser]))
    print(f"P={P}: population {rows[-1]['population_ms']:.3f} ms, serial {rows[-1]['serial_ms']:.3f} ms per call", file=sys.stderr, flush=True)
print("| P | population, ms / call (min – max) | P x dril_evaluate_agent_device, ms (min – max) | ratio | launches | kernel_ms | run solo | equal to solo |")
print("|--:|--:|--:|--:|--:|--:|--:|:--|")
for r in rows:
    print(f"| {r['P']} | {r['population_ms']:.3f} ({r['population_ms_min']:.3f} – {r['population_ms_max']:.3f}) | {r['serial_ms']:.3f} ({r['serial_ms_min']:.3f} – {r['serial_ms_max']:.3f}) | "
          f"{r['serial_ms'] / r['population_ms']:.2f} | {r['launches']} | {r['kernel_ms']:.3f} | {r['members_run_solo']} | {'yes' if r['equal_to_solo'] else 'NO'} |")
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text(json.dumps(dict(shape=dict(env="CartPole", n_envs=E, n_steps=T, batch_size=64, epochs=10, n_eval_episodes=N_EVAL, trained_iterations=a.train),
                                       warmup=a.warmup, reps=a.reps, rows=rows), indent=1) + "\n")
