#!/usr/bin/env python3
"""The reference README quick-start (4 envs, `PPO()` defaults: 2048 steps, batch 64, 10 epochs) for ten seeds as ONE population: every iteration of all ten
agents is one batched rollout launch and one batched update launch (docs/population.md), and every agent ends bit-identical to its own `train_` call.  The seeds are then judged with `evaluate_population`: one batched
launch and one look at the counters per K env steps for all of them.

usage: python examples/ppo_cartpole_seeds.py [iterations=30] [seeds=10] [--serial]      (--serial: also time the same agents trained and evaluated one after the other)"""
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
    envs = [pkg.DeviceParallelEnv(pkg.CartPoleEnv(max_steps=500), 4, seed=s) for s in range(seeds)]
    agents = [pkg.Agent(pkg.ActorCriticLayer(e.observation_space(), e.action_space()), alg, seed=s) for s, e in enumerate(envs)]
    return agents, envs


max_steps = iters * alg.n_steps * 4
agents, envs = fresh()
t0 = time.perf_counter()
results = pkg.train_population_(agents, envs, [alg] * seeds, max_steps)
t_pop = time.perf_counter() - t0
print(f"population of {seeds} seeds, {iters} iterations: {t_pop:.2f} s wall ({results[0][1]['training_loop']:.2f} s in the training loop)")
t0 = time.perf_counter()
evs = pkg.evaluate_population(agents, envs, n_eval_episodes=10)   # all seeds in one batched launch per K env steps (docs/population.md, "Evaluation")
t_eval = time.perf_counter() - t0
print(f"evaluation of the {seeds} seeds as one population: {1e3 * t_eval:.1f} ms wall")
for s, ev in enumerate(evs):
    print(f"  seed {s}: mean reward {ev['mean_reward']:.1f} +- {ev['std_reward']:.1f}, last loss {results[s][0]['losses'][-1]:.4f}")
if "--serial" in sys.argv:
    t0 = time.perf_counter()
    each = [pkg.evaluate_agent(agent, env, n_eval_episodes=10, isolated=True) for agent, env in zip(agents, envs)]
    t_each = time.perf_counter() - t0
    print(f"the same evaluation, one evaluate_agent(isolated=True) per seed: {1e3 * t_each:.1f} ms wall ({t_each / t_eval:.2f} x the population); results equal: {each == evs}")
if "--serial" in sys.argv:
    agents2, envs2 = fresh()
    t0 = time.perf_counter()
    for a, e in zip(agents2, envs2):
        pkg.train_(a, e, alg, max_steps)
    t_ser = time.perf_counter() - t0
    same = all((pkg.flatten_params(a.train_state.parameters) == pkg.flatten_params(b.train_state.parameters)).all() for a, b in zip(agents, agents2))
    print(f"the same {seeds} agents with {seeds} serial train_ calls: {t_ser:.2f} s wall ({t_ser / t_pop:.2f} x the population); parameters bit-equal: {same}")
