#!/usr/bin/env python3
"""PPO on the caller's OWN env, living on the device: examples/envs/reacher3_plugin.hip (a point mass in 3-D pushed towards a per-episode random target; 12
observation dims, 3 action dims — nothing the built-in kinds can express) is compiled by the library's Makefile into a gfx950 code object; the library loads
it (DRIL_ENV_MODULE) and steps it with its own kernels.  No host env anywhere in the loop.

usage: python examples/ppo_device_plugin.py [n_envs=256] [iterations=30] [--normalize] [--scaling] [--fused] [--persistent-eval] [--fused-update]
--scaling: ScalingWrapperEnv around every env (dril_scaling_enable: the plug-in's own _scaled kernels; the agent sees Box(-1, 1) observations and actions)
--fused: every collection is ONE launch of the plug-in's own rollout kernel (examples/envs/reacher3_fused_plugin.hip = the same env + DRIL_ENV_PLUGIN_ROLLOUT;
  dril_rollout_fused_enable) instead of six or more launches per env step; not together with --normalize
--persistent-eval: the evaluations run through the plug-in's own evaluation kernel (examples/envs/reacher3_eval_plugin.hip = the fused twin + DRIL_ENV_PLUGIN_EVALUATE):
  two launches per K env steps instead of eight or more per step (docs/evaluation.md, path 2); works with --normalize (frozen statistics) and --scaling
--fused-update: every optimiser step of an update inside ONE launch of ppo_update_generic_small_kernel (dril_update_fused_enable, docs/generic_update.md) instead of
  twelve launches per step; it is for the reference's own scale, so the run uses PPO()'s batch_size = 64 (try: 4 30 --fused-update)
--normalize: NormalizeWrapperEnv around the plug-in envs with the reference's default keywords (dril_normalize_enable: observation and reward statistics on the device)"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g

pkg = g.load_package()
normalize, scaling, fused, persistent, fused_update = ("--" + f in sys.argv for f in ("normalize", "scaling", "fused", "persistent-eval", "fused-update"))
args = [a for a in sys.argv[1:] if a not in ("--normalize", "--scaling", "--fused", "--persistent-eval", "--fused-update")]
n_envs = int(args[0]) if len(args) > 0 else 256
iters = int(args[1]) if len(args) > 1 else 30
code_object = ROOT / "examples" / "envs" / ("reacher3_eval_plugin.hsaco" if persistent else "reacher3_fused_plugin.hsaco" if fused else "reacher3_plugin.hsaco")        # built by `make -C dril.jl_amd/csrc` (__graft_entry__.build())
print("env:", pkg.describe_env_module(code_object))
env = pkg.MonitorWrapperEnv(pkg.DeviceModuleEnv(code_object, n_envs, seed=0, normalize={} if normalize else None, scaling=scaling, fused_rollout=fused), stats_window=n_envs)
alg = pkg.PPO(n_steps=100, batch_size=64 if fused_update else n_envs * 100 // 4, epochs=10, learning_rate=1e-3)
agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space()), alg, seed=0)


class PrintReturn:
    def on_rollout_end(self, loc):
        r, l, n = loc["env"].handle.monitor_stats()
        print(f"iteration {loc['i']:3d}: episode return {r:8.3f}  length {l:6.1f}  ({n} episodes in the window)  rollout {loc['fps']:.3g} env-steps/s")
        return True


# isolated=True: evaluated on the device, the training envs, the monitor's window and (under --normalize) the statistics left as they were (docs/evaluation.md)
print("evaluate_agent before:", pkg.evaluate_agent(agent, env, n_eval_episodes=20, isolated=True, persistent=persistent))
stats, timer = pkg.train_(agent, env, alg, iters * alg.n_steps * n_envs, callbacks=[PrintReturn()], fused_update=fused_update)
print(f"trained {iters} iterations in {timer['training_loop']:.2f} s; last loss {stats['losses'][-1]:.4f}")
print("evaluate_agent after: ", pkg.evaluate_agent(agent, env, n_eval_episodes=20, isolated=True, persistent=persistent))        # under --normalize: the training statistics, frozen; raw episode returns
if fused_update:
    print("fused update:", env.handle.update_fused_info())
if persistent:
    print("fused evaluation:", env.handle.evaluate_fused_info())
if normalize:
    st = env.handle.normalize_get_stats()
    print(f"obs_rms over {st['obs_count']} observations: mean {st['obs_mean'].round(3)}  var {st['obs_var'].round(3)};  ret_rms var {st['ret_var']:.4f} over {st['ret_count']}")
