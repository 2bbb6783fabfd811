#!/usr/bin/env python3
"""Ten seeds of PPO on a user's own device env — the reacher3 plug-in (examples/envs/reacher3_pop_plugin.hip) — as ONE population: every iteration of all ten
agents is one launch of the plug-in's dril_env_plugin_rollout_pop and one launch of ppo_update_generic_small_pop_kernel (docs/population.md, "Plug-in members"),
and every agent ends bit-identical to its own `train_(..., fused_update=True)` call on `DeviceModuleEnv(path, n, fused_rollout=True)`.

usage: python examples/ppo_device_plugin_seeds.py [iterations=10] [seeds=10] [--serial]      (--serial: also time the same agents trained one after the other)"""
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import __graft_entry__ as g

pkg = g.load_package()
args = [a for a in sys.argv[1:] if not a.startswith("--")]
iters = int(args[0]) if len(args) > 0 else 10
seeds = int(args[1]) if len(args) > 1 else 10
alg = pkg.PPO()
co = Path(__file__).resolve().parent / "envs" / "reacher3_pop_plugin.hsaco"      # built by the default target of dril.jl_amd/csrc/Makefile


def fresh():
    envs = [pkg.DeviceModuleEnv(co, 4, seed=s, fused_rollout=True) for s in range(seeds)]
    agents = [pkg.Agent(pkg.ActorCriticLayer(e.observation_space(), e.action_space()), alg, seed=s) for s, e in enumerate(envs)]
    return agents, envs


max_steps = iters * alg.n_steps * 4
agents, envs = fresh()
t0 = time.perf_counter()
results = pkg.train_population_(agents, envs, [alg] * seeds, max_steps, fused_update=True)
t_pop = time.perf_counter() - t0
print(f"population of {seeds} seeds, {iters} iterations: {t_pop:.2f} s wall ({results[0][1]['training_loop']:.2f} s in the training loop)")
evs = pkg.evaluate_population(agents, envs, n_eval_episodes=10)                  # plug-in members are evaluated one by one inside the call
for s, ev in enumerate(evs):
    print(f"  seed {s}: mean reward {ev['mean_reward']:.2f} +- {ev['std_reward']:.2f}, last loss {results[s][0]['losses'][-1]:.4f}")
if "--serial" in sys.argv:
    agents2, envs2 = fresh()
    t0 = time.perf_counter()
    for a, e in zip(agents2, envs2):
        pkg.train_(a, e, alg, max_steps, fused_update=True)
    t_ser = time.perf_counter() - t0
    same = all((pkg.flatten_params(a.train_state.parameters) == pkg.flatten_params(b.train_state.parameters)).all() for a, b in zip(agents, agents2))
    print(f"the same {seeds} agents with {seeds} serial train_ calls: {t_ser:.2f} s wall ({t_ser / t_pop:.2f} x the population); parameters bit-equal: {same}")
