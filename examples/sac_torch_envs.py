#!/usr/bin/env python3
"""SAC on a batched env written in PyTorch-ROCm tensor ops: observations, actions, rewards and flags never leave the GPU.

    env = DeviceArrayParallelEnv(TorchPendulums(1024), stream=lambda: torch.cuda.current_stream().cuda_stream)
    sac_train_(agent, env, alg, max_steps)

The twin of examples/ppo_torch_envs.py (the env is that file's TorchPendulums).  The library takes the tensors through __cuda_array_interface__
(dril_sac_ext_act_device / dril_sac_ext_push_device / dril_sac_update_enqueue): every call of an iteration enqueues on the device and returns, the start phase's
random actions are drawn on the device, and the host waits only in dril_sac_flush — when the pending statistics table is full and at the end (docs/sac.md,
"SAC on device-resident env arrays").

--normalize / --monitor wrap the env as NormalizeWrapperEnv(MonitorWrapperEnv(env, 100)): the handle's own wrappers on the device (dril_sac_ext_normalize_enable /
dril_sac_ext_monitor_enable), with which the loop stays free of host waits; the evaluations then run under the training statistics, frozen.

usage: python examples/sac_torch_envs.py [--envs 1024] [--iterations 2000] [--gradient-steps 1] [--normalize] [--monitor] [--profile]"""
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
    ap.add_argument("--normalize", action="store_true", help="NormalizeWrapperEnv around the env, on the device")
    ap.add_argument("--monitor", action="store_true", help="MonitorWrapperEnv(env, 100) around the env, on the device")
    ap.add_argument("--profile", action="store_true", help="HIP events around what act and push enqueue (cfg.profile_events): prints their time per env step")
    a = ap.parse_args()
    E = a.envs
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def make(seed=0):
        e = pkg.DeviceArrayParallelEnv(TorchPendulums(E, seed=seed), stream=stream, profile_events=a.profile)
        if a.monitor and seed == 0:
            e = pkg.MonitorWrapperEnv(e, 100)
        return pkg.NormalizeWrapperEnv(e) if a.normalize else e

    env = make()
    alg = pkg.SAC(start_steps=4 * E, train_freq=1, gradient_steps=a.gradient_steps, batch_size=256, buffer_capacity=max(200 * E, 100_000), learning_rate=1e-3)
    agent = pkg.SACAgent(pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(64, 64)), alg, seed=0)
    episodes = min(E, 256)
    before = pkg.sac_evaluate_agent(agent, make(1), n_eval_episodes=episodes, normalize_stats="fresh")["mean_reward"]   # an untrained agent: fresh statistics
    max_steps = alg.start_steps + (a.iterations - 1) * E                              # the start phase is the first iteration
    agent, rb, stats, timer = pkg.sac_train_(agent, env, alg, max_steps)
    info = rb.handle.ext_device_info()
    after = pkg.sac_evaluate_agent(agent, make(1), n_eval_episodes=episodes, normalize_stats=rb.handle)["mean_reward"]  # the training statistics, frozen; raw returns
    print(f"before: mean return {before:9.1f}")
    print(f"after {timer['iterations']} iterations ({timer['training_loop']:.1f} s, {agent.gradient_updates} gradient steps): mean return {after:9.1f}")
    print(f"steps_device={info['steps_device']} steps_host={info['steps_host']} host_syncs={timer['host_syncs']} flushes={timer['flushes']} "
          f"launches_per_step={info['launches'] / max(info['steps_device'], 1):.1f} replay={rb.handle.replay_size()}")
    prof = rb.handle.profile()                                                        # HIP events around what act and push enqueue (profile_events; read by the flushes)
    if prof["collect_steps"]:
        print(f"act + push: {prof['collect_ms'] / prof['collect_steps'] * 1e3:.1f} us of HIP-event time per env step over {prof['collect_steps']} steps")
    if a.normalize:
        st = rb.handle.ext_normalize_get_stats()
        print(f"normalize: obs_count={st['obs_count']} ret_count={st['ret_count']} obs_mean={st['obs_mean'].round(3).tolist()} ret_var={st['ret_var']:.3f}")
    if a.monitor:
        r, l, n = env.monitor_stats()
        print(f"monitor: ep_rew_mean={r:.1f} ep_len_mean={l:.1f} over {n} episodes")
    if a.normalize or a.monitor:
        wi = rb.handle.ext_wrap_info()
        print(f"wrappers: launches added per act {wi['launches_act'] / max(info['steps_device'], 1):.2f}, per push {wi['launches_push'] / max(info['steps_device'], 1):.2f}, allocations={wi['allocations']}")
    rb.handle.close()


if __name__ == "__main__":
    main()
