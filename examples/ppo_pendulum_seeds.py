#!/usr/bin/env python3
"""Continuous control at the reference's own scale — Pendulum, 4 envs, `PPO()` defaults, `NormalizeWrapperEnv(MonitorWrapperEnv(env))` — for ten seeds as ONE
population.  `fused_rollout=True` on the wrapper (dril_norm_rollout_enable, docs/normalized_rollout.md) makes a normalised collection one launch instead of three per
env step, which is also what lets normalising agents join a population: every iteration of all ten agents is the seeds' opening observes, one batched rollout
launch and one batched update launch, and every agent ends bit-identical to its own `train_` call.

usage: python examples/ppo_pendulum_seeds.py [iterations=30] [seeds=10] [--serial]      (--serial: also time the same agents trained one after the other)"""
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import __graft_entry__ as g

pkg = g.load_package()
args = [a for a in sys.argv[1:] if not a.startswith("--")]
iters = int(args[0]) if len(args) > 0 else 30
seeds = int(args[1]) if len(args) > 1 else 10
alg = pkg.PPO()


def fresh():
    envs = [pkg.NormalizeWrapperEnv(pkg.MonitorWrapperEnv(pkg.DeviceParallelEnv(pkg.PendulumEnv(), 4, seed=s), 100), fused_rollout=True) for s in range(seeds)]
    agents = [pkg.Agent(pkg.ActorCriticLayer(e.observation_space(), e.action_space()), alg, seed=s) for s, e in enumerate(envs)]
    return agents, envs


max_steps = iters * alg.n_steps * 4
agents, envs = fresh()
t0 = time.perf_counter()
results = pkg.train_population_(agents, envs, [alg] * seeds, max_steps)
t_pop = time.perf_counter() - t0
print(f"population of {seeds} normalised seeds, {iters} iterations: {t_pop:.2f} s wall ({results[0][1]['training_loop']:.2f} s in the training loop)")
evs = pkg.evaluate_population(agents, envs, n_eval_episodes=10)   # normalising members evaluate one after the other, on frozen statistics (docs/population.md, "Evaluation")
for s, (ev, env) in enumerate(zip(evs, envs)):
    info = env.handle.norm_rollout_info()
    print(f"  seed {s}: mean reward {ev['mean_reward']:.1f} +- {ev['std_reward']:.1f}, last loss {results[s][0]['losses'][-1]:.4f}, "
          f"collection path {info['last_collection_path']} in {info['last_collection_launches']} launches")
if "--serial" in sys.argv:
    agents2, envs2 = fresh()
    t0 = time.perf_counter()
    for a, e in zip(agents2, envs2):
        pkg.train_(a, e, alg, max_steps)
    t_ser = time.perf_counter() - t0
    same = all((pkg.flatten_params(a.train_state.parameters) == pkg.flatten_params(b.train_state.parameters)).all() for a, b in zip(agents, agents2))
    print(f"the same {seeds} agents with {seeds} serial train_ calls: {t_ser:.2f} s wall ({t_ser / t_pop:.2f} x the population); parameters bit-equal: {same}")
