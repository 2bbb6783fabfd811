#!/usr/bin/env python3
"""SAC on the caller's OWN env, living on the device: examples/envs/reacher3_plugin.hip (a point mass in 3-D pushed towards a per-episode random target; 12
observation dims, a three-dimensional force Box) is compiled by the library's Makefile into a gfx950 code object; the library loads it
(dril_sac_create_with_env_module) and steps it with its own kernels between the actor's forward and the replay ring.  No host env anywhere in the loop:
off-policy collection, the ring and every gradient step stay on the device.  The PPO twin of this file is examples/ppo_device_plugin.py.

usage: python examples/sac_device_plugin.py [--normalize] [--scaling] [n_envs=16] [max_steps=30000]
--scaling trains under ScalingWrapperEnv (dril_sac_scaling_enable: the plug-in's own _scaled kernels; observations in the ring and the actions the adapters
produce live in Box(-1, 1)).
--normalize trains through NormalizeWrapperEnv on the device (sac_train_(..., normalize=dict()): running statistics of the 12 mixed-scale observation dims and of
the discounted returns, normalised rows in the ring) and evaluates with the training statistics, frozen; the final statistics are printed."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g

pkg = g.load_package()
args = [a for a in sys.argv[1:] if a not in ("--normalize", "--scaling")]
normalize = dict() if "--normalize" in sys.argv[1:] else None                # the reference's keyword defaults (normalizeWrapperEnv.jl:71-80)
n_envs = int(args[0]) if len(args) > 0 else 16
max_steps = int(args[1]) if len(args) > 1 else 30000
code_object = ROOT / "examples" / "envs" / "reacher3_plugin.hsaco"        # built by `make -C dril.jl_amd/csrc` (__graft_entry__.build())
info = pkg.describe_env_module(code_object)
print("env:", info)
env = pkg.DeviceModuleEnv(code_object, n_envs, seed=0, scaling="--scaling" in sys.argv[1:])
alg = pkg.SAC(learning_rate=1e-3, buffer_capacity=100_000, start_steps=100 * n_envs, batch_size=256, gradient_steps=8)
agent = pkg.SACAgent(pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(64, 64)), alg, seed=0)
env = pkg.MonitorWrapperEnv(env, 100)                                     # sac_train_ switches MonitorWrapperEnv on around the handle's envs: ep_rew_mean of the training episodes
before = pkg.sac_evaluate_agent(agent, env, n_eval_episodes=n_envs, normalize=normalize, normalize_stats="fresh" if normalize is not None else None)   # evaluate_agent: deterministic policy, episode accounting on the device, no training data touched
agent, rb, stats, timer = pkg.sac_train_(agent, env, alg, max_steps, normalize=normalize)
after = pkg.sac_evaluate_agent(agent, env, n_eval_episodes=n_envs, normalize=normalize, normalize_stats=rb.handle if normalize is not None else None)
ep_rew_mean, ep_len_mean, n_ep = rb.handle.monitor_stats()
print(f"trained {agent.steps_taken} env steps, {agent.gradient_updates} gradient steps in {timer['training_loop']:.2f} s; "
      f"critic loss {stats['critic_losses'][-1]:.4f}, entropy coefficient {stats['entropy_coefficients'][-1]:.4f}")
print(f"evaluate_agent ({n_envs} episodes, deterministic): mean return {before['mean_reward']:.1f} +- {before['std_reward']:.1f} before -> "
      f"{after['mean_reward']:.1f} +- {after['std_reward']:.1f} after (mean length {after['mean_length']:.0f})")
print(f"monitor: env/ep_rew_mean {ep_rew_mean:.1f}, env/ep_len_mean {ep_len_mean:.1f} over the last {n_ep} training episodes")
if normalize is not None:
    st = rb.handle.norm_get_stats()
    print(f"NormalizeWrapperEnv: obs_count {st['obs_count']}, ret_count {st['ret_count']}, ret_var {st['ret_var']:.4f}\n  obs_mean {st['obs_mean'].round(3)}\n  obs_std  {(st['obs_var'] ** 0.5).round(3)}")
