#!/usr/bin/env python3
"""PPO on a multi-agent WORLD living on the device: examples/envs/rendezvous3_plugin.hip (three point agents in the plane that share one state and are rewarded for
meeting; include/device/dril_env_world.h) is compiled by the library's Makefile into a gfx950 code object.  The library sees agent i of world w as row 3 w + i — the
stacking of the reference's MultiAgentParallelEnv — so ONE shared policy acts for every agent of every world, and the rollout buffer, GAE, the update and
MonitorWrapperEnv work per row as for any device env.  No host env anywhere in the loop.

usage: python examples/ppo_device_world.py [n_envs=66] [iterations=30]        (n_envs counts rows: a multiple of 3)"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g

pkg = g.load_package()
n_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 66
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 30
code_object = ROOT / "examples" / "envs" / "rendezvous3_plugin.hsaco"              # built by `make -C dril.jl_amd/csrc` (__graft_entry__.build())
print("env:", pkg.describe_env_module(code_object))
module = pkg.DeviceModuleEnv(code_object, n_envs, seed=0)
print(f"{module.n_worlds} worlds of {module.agents_per_world} agents = {n_envs} rows")
env = pkg.MonitorWrapperEnv(module, stats_window=n_envs)
alg = pkg.PPO(n_steps=100, batch_size=n_envs * 100 // 4, epochs=10, learning_rate=1e-3)
agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space()), alg, seed=0)


class PrintReturn:
    def on_rollout_end(self, loc):
        r, l, n = loc["env"].handle.monitor_stats()
        print(f"iteration {loc['i']:3d}: episode return per agent {r:8.3f}  length {l:6.1f}  ({n} episodes in the window)  rollout {loc['fps']:.3g} env-steps/s")
        return True


print("evaluate_agent before:", pkg.evaluate_agent(agent, env, n_eval_episodes=21, isolated=True))
stats, timer = pkg.train_(agent, env, alg, iters * alg.n_steps * n_envs, callbacks=[PrintReturn()])
print(f"trained {iters} iterations in {timer['training_loop']:.2f} s; last loss {stats['losses'][-1]:.4f}")
print("evaluate_agent after: ", pkg.evaluate_agent(agent, env, n_eval_episodes=21, isolated=True))
trajs = pkg.collect_trajectory(agent, env, n_trajectories=module.agents_per_world)                # one whole world: a trajectory per agent, equally long
print("one world's trajectory:", [len(r) for _, _, r in trajs], "steps per agent")
