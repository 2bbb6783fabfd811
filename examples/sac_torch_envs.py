#!/usr/bin/env python3
"""SAC on a batched env written in PyTorch-ROCm tensor ops: observations, actions, rewards and flags never leave the GPU.

    env = DeviceArrayParallelEnv(TorchPendulums(1024), stream=lambda: torch.cuda.current_stream().cuda_stream)
    sac_train_(agent, env, alg, max_steps)

The twin of examples/ppo_torch_envs.py (the env is that file's TorchPendulums).  The library takes the tensors through __cuda_array_interface__
(dril_sac_ext_act_device / dril_sac_ext_push_device / dril_sac_update_enqueue): every call of an iteration enqueues on the device and returns, the start phase's
random actions are drawn on the device, and the host waits only in dril_sac_flush — when the pending statistics table is full and at the end (docs/sac.md,
"SAC on device-resident env arrays").

usage: python examples/sac_torch_envs.py [--envs 1024] [--iterations 2000] [--gradient-steps 1]"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from ppo_torch_envs import TorchPendulums, pkg   # noqa: E402  (examples/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--gradient-steps", type=int, default=1)
    a = ap.parse_args()
    E = a.envs
    stream = lambda: torch.cuda.current_stream().cuda_stream
    env = pkg.DeviceArrayParallelEnv(TorchPendulums(E), stream=stream)
    alg = pkg.SAC(start_steps=4 * E, train_freq=1, gradient_steps=a.gradient_steps, batch_size=256, buffer_capacity=max(200 * E, 100_000), learning_rate=1e-3)
    agent = pkg.SACAgent(pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(64, 64)), alg, seed=0)
    episodes = min(E, 256)
    before = pkg.sac_evaluate_agent(agent, pkg.DeviceArrayParallelEnv(TorchPendulums(E, seed=1), stream=stream), n_eval_episodes=episodes)["mean_reward"]
    max_steps = alg.start_steps + (a.iterations - 1) * E                              # the start phase is the first iteration
    agent, rb, stats, timer = pkg.sac_train_(agent, env, alg, max_steps)
    info = rb.handle.ext_device_info()
    after = pkg.sac_evaluate_agent(agent, pkg.DeviceArrayParallelEnv(TorchPendulums(E, seed=1), stream=stream), n_eval_episodes=episodes)["mean_reward"]
    print(f"before: mean return {before:9.1f}")
    print(f"after {timer['iterations']} iterations ({timer['training_loop']:.1f} s, {agent.gradient_updates} gradient steps): mean return {after:9.1f}")
    print(f"steps_device={info['steps_device']} steps_host={info['steps_host']} host_syncs={timer['host_syncs']} flushes={timer['flushes']} "
          f"launches_per_step={info['launches'] / max(info['steps_device'], 1):.1f} replay={rb.handle.replay_size()}")
    rb.handle.close()


if __name__ == "__main__":
    main()
