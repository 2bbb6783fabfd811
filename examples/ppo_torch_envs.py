#!/usr/bin/env python3
"""PPO on a batched env written in PyTorch-ROCm tensor ops: observations, rewards and flags never leave the GPU.

    env = DeviceArrayParallelEnv(TorchPendulums(1024), stream=lambda: torch.cuda.current_stream().cuda_stream)
    train_(agent, env, alg, max_steps)

The library takes the tensors through __cuda_array_interface__ (dril_ext_act_device / dril_ext_record_device / dril_ext_finish_device): every call of a
rollout enqueues on the device and returns, the one host wait is the last call's (docs/external_envs.md section 10, "Device-resident arrays").

--normalize / --monitor put NormalizeWrapperEnv / MonitorWrapperEnv around the env: the library's own wrappers on the device arrays (dril_ext_normalize_enable /
dril_ext_monitor_enable, docs/external_envs.md section 10, "Wrappers on device-resident arrays") — running statistics, clipped normalised observations and rewards, episode statistics of the raw
rewards — and the rollout still makes no host wait before its last call.

usage: python examples/ppo_torch_envs.py [n_envs=1024] [iterations=30] [--normalize] [--monitor]"""
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import __graft_entry__ as g   # noqa: E402

pkg = g.load_package()


class TorchPendulums:
    """E pendulums as three tensors: observation (cos th, sin th, th'), one torque in Box(-2, 2), reward -(th^2 + 0.1 th'^2 + 0.001 u^2), 200-step episodes"""

    def __init__(self, n_envs, seed=0, device="cuda", max_steps=200):
        self.n_envs, self.dev, self.max_steps = n_envs, torch.device(device), max_steps
        self.gen = torch.Generator(device=self.dev); self.gen.manual_seed(seed)
        self.th = torch.empty(n_envs, device=self.dev); self.thdot = torch.empty(n_envs, device=self.dev); self.t = torch.zeros(n_envs, dtype=torch.int32, device=self.dev)
        self.reset_()

    def observation_space(self):
        return pkg.Box(low=(-1.0, -1.0, -8.0), high=(1.0, 1.0, 8.0))

    def action_space(self):
        return pkg.Box(low=(-2.0,), high=(2.0,))

    def _draw(self, n, lo, hi):
        return torch.rand(n, device=self.dev, generator=self.gen) * (hi - lo) + lo

    def reset_(self):
        self.th[:] = self._draw(self.n_envs, -math.pi, math.pi); self.thdot[:] = self._draw(self.n_envs, -1.0, 1.0); self.t.zero_()

    def observe(self):
        return torch.stack([torch.cos(self.th), torch.sin(self.th), self.thdot], dim=1).contiguous()

    def act_(self, actions):                                                         # actions: (E, 1) f32, already clamped to the Box on the device
        u = actions[:, 0]
        th = torch.remainder(self.th + math.pi, 2 * math.pi) - math.pi
        reward = -(th ** 2 + 0.1 * self.thdot ** 2 + 0.001 * u ** 2)
        self.thdot = torch.clamp(self.thdot + (15.0 * torch.sin(self.th) + 3.0 * u) * 0.05, -8.0, 8.0)
        self.th = self.th + self.thdot * 0.05
        self.t += 1
        truncated = self.t >= self.max_steps
        terminated = torch.zeros_like(truncated)
        terminal_obs = self.observe()                                                # the pre-reset observation of every env: the library keeps V of the truncated ones
        n = self.n_envs                                                              # auto-reset without a host round trip: draw for all, keep where truncated
        self.th = torch.where(truncated, self._draw(n, -math.pi, math.pi), self.th); self.thdot = torch.where(truncated, self._draw(n, -1.0, 1.0), self.thdot)
        self.t = torch.where(truncated, torch.zeros_like(self.t), self.t)
        return reward, terminated, truncated, terminal_obs


def mean_return(agent, env, episodes):
    return pkg.evaluate_agent(agent, env, n_eval_episodes=episodes, deterministic=True)["mean_reward"]


def make_env(n_envs, normalize=False, monitor=False, max_steps=200):
    env = pkg.DeviceArrayParallelEnv(TorchPendulums(n_envs, max_steps=max_steps), stream=lambda: torch.cuda.current_stream().cuda_stream)
    if monitor:
        env = pkg.MonitorWrapperEnv(env, 100)                                        # inside the normaliser: raw returns
    if normalize:
        env = pkg.NormalizeWrapperEnv(env, gamma=0.95)
    return env


def main():
    flags = {a for a in sys.argv[1:] if a.startswith("--")}
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n_envs = int(args[0]) if len(args) > 0 else 1024
    iters = int(args[1]) if len(args) > 1 else 30
    env = make_env(n_envs, normalize="--normalize" in flags, monitor="--monitor" in flags)
    alg = pkg.PPO(n_steps=200, batch_size=n_envs * 200 // 8, epochs=8, learning_rate=1e-3, gamma=0.95)
    agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space(), hidden_dims=(64, 64)), alg, seed=0)
    print(f"before: mean return {mean_return(agent, env, n_envs):9.1f}")
    stats, timer = pkg.train_(agent, env, alg, iters * alg.n_steps * n_envs)
    info = env.handle.ext_device_info()
    print(f"after {iters} iterations ({timer['training_loop']:.1f} s, rollouts {timer['collect_rollout']:.1f} s, updates {timer['epoch loop']:.2f} s): mean return {mean_return(agent, env, n_envs):9.1f}; "
          f"last rollout: {info['steps_device']} steps through the device verbs, {info['host_syncs']} host waits before its last call, {info['launches']} launches")
    if "--monitor" in flags:
        print("monitor window: mean return %.1f, mean length %.1f over %d episodes" % env.monitor_stats())
    if "--normalize" in flags:
        st = env.handle.ext_normalize_get_stats()
        print(f"normaliser: {st['obs_count']} observations, mean {st['obs_mean'].round(3)}, var {st['obs_var'].round(3)}; return variance {st['ret_var']:.3f}")


if __name__ == "__main__":
    main()
