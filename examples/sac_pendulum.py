#!/usr/bin/env python3
"""SAC on Pendulum-v1 on the device path (reference: src/algorithms/sac.jl; BASELINE.json configs[4] uses n_envs = 4096):

    env = MultiThreadedParallelEnv([PendulumEnv() for _ in 1:n]) -> DeviceParallelEnv(PendulumEnv(), n)
    alg = SAC();  layer = SACLayer(observation_space(env), action_space(env));  agent = Agent(layer, alg)
    agent, replay_buffer, training_stats, to = train!(agent, env, alg, max_steps)

usage: python examples/sac_pendulum.py [n_envs=64] [env_steps=200000] [--trajectory]
--trajectory: after training, collect_trajectory(agent, env) records one episode of the deterministic policy on the device and prints its length, its return and
its first rows"""
import sys
from pathlib import Path
import numpy as np
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import __graft_entry__ as g

pkg = g.load_package()
show_trajectory = "--trajectory" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--trajectory"]
n_envs = int(argv[0]) if len(argv) > 0 else 64
max_steps = int(argv[1]) if len(argv) > 1 else 200_000
env = pkg.DeviceParallelEnv(pkg.PendulumEnv(max_steps=200), n_envs, seed=0)
alg = pkg.SAC(start_steps=5000, buffer_capacity=200_000, gradient_steps=max(1, n_envs // 8))
agent = pkg.SACAgent(pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(256, 256)), alg, seed=0)
env = pkg.MonitorWrapperEnv(env, 100)                                     # MonitorWrapperEnv(env, 100): episode statistics of the training episodes
before = pkg.sac_evaluate_agent(agent, env)                               # evaluate_agent(agent, env): ten episodes of the deterministic policy
agent, rb, stats, timer = pkg.sac_train_(agent, env, alg, max_steps)
after = pkg.sac_evaluate_agent(agent, env)
ep_rew_mean, ep_len_mean, n_ep = rb.handle.monitor_stats()
print(f"{agent.steps_taken} env steps, {agent.gradient_updates} gradient steps in {timer['training_loop']:.1f} s")
print(f"evaluate_agent (10 episodes, deterministic): mean return {before['mean_reward']:.1f} +- {before['std_reward']:.1f} before -> {after['mean_reward']:.1f} +- {after['std_reward']:.1f} after")
print(f"monitor: env/ep_rew_mean {ep_rew_mean:.1f}, env/ep_len_mean {ep_len_mean:.1f} over the last {n_ep} training episodes")
print(f"critic loss {np.mean(stats['critic_losses'][:50]):.3f} -> {np.mean(stats['critic_losses'][-50:]):.3f}; entropy coefficient {stats['entropy_coefficients'][-1]:.3f}")
if show_trajectory:                                                       # collect_trajectory(agent, env): original observations, env actions, raw rewards
    obs, act, rew = pkg.sac_collect_trajectory(agent, env)
    print(f"collect_trajectory: one episode of {len(rew)} steps, return {rew.sum():.1f}")
    print("   t   cos(theta) sin(theta)  theta_dot     torque     reward")
    for t in range(min(5, len(rew))):
        print(f"{t:4d}   {obs[t, 0]:10.4f} {obs[t, 1]:10.4f} {obs[t, 2]:10.4f} {act[t, 0]:10.4f} {rew[t]:10.4f}")
    print(f"   final observation {np.array2string(obs[-1], precision=4)}")
