#!/usr/bin/env python3
"""Per-env-step cost of a collection with a device env plug-in (DRIL_ENV_MODULE) next to the built-in env on the same generic kernels:
  (a) the CartPole twin plug-in        policy launches + ONE plug-in step launch per env step
  (b) built-in CartPole, DRIL_FORCE_GENERIC=1   policy launches + norm_step_kernel + norm_apply_kernel
  (c) reacher3 plug-in (D = 12, S = 9, A = 3)
  (d) reacher3 plug-in under NormalizeWrapperEnv (dril_normalize_enable)   (c) + norm_moments_kernel<64> + ppo_norm_apply_kernel per env step
hidden [64,64], T = 32 steps per rollout, E = 64 .. 65 536.  Per rollout: wall time around dril_collect_rollout and the library's HIP-event time of the
rollout class (cfg.profile_events); median and min..max over the rollouts after warm-up, divided by T.   usage: python tools/env_plugin_latency.py [rollouts=20] [--fused]
--fused: instead of (a) - (d), the FUSED rollout (dril_rollout_fused_enable; examples/envs/*_fused_plugin.hip) next to the step-granular collection of the same code
object, on the same handle in the same process: the CartPole twin and reacher3 at hidden [64,64], and one reacher3 row at [256,256]"""
import os, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g

pkg = g.load_package(); capi = pkg._capi
FUSED = "--fused" in sys.argv
_args = [a for a in sys.argv[1:] if a != "--fused"]
R = int(_args[0]) if _args else 20
T = 32


def measure(label, kind, E, module=None, force_generic=False, normalize=False, hidden=64, fused=None):
    """fused: None = a handle of its own, step-granular; True = both paths on ONE handle, step-granular first"""
    c = capi.default_config(kind)
    c.n_envs, c.n_steps, c.batch_size, c.epochs, c.profile_events, c.hidden1, c.hidden2 = E, T, E * T, 1, 1, hidden, hidden
    if force_generic:
        os.environ["DRIL_FORCE_GENERIC"] = "1"
    h = pkg.Handle(c, env_module=module)
    os.environ.pop("DRIL_FORCE_GENERIC", None)
    if normalize:
        h.normalize_enable()
    h.set_params((np.random.default_rng(0).standard_normal(h.P) * 0.2).astype(np.float32))
    h.env_reset(1)
    for on in ((False, True) if fused else (False,)):
        if fused:
            h.rollout_fused_enable(on)
        wall, dev = [], []
        for r in range(R + 3):
            h.profile_reset()
            a = time.perf_counter(); h.collect_rollout(); b = time.perf_counter()
            if r >= 3:
                wall.append((b - a) / T * 1e6); dev.append(h.profile()["rollout_kernel"]["total_ms"] / T * 1e3)
        w, d = np.asarray(wall), np.asarray(dev)
        name = label + ((", fused" if on else ", step-granular") if fused else "")
        print(f"E = {E:6d}  {name:42s} wall {np.median(w):7.1f} us / env step ({w.min():.1f} .. {w.max():.1f})   HIP events {np.median(d):7.1f} us ({d.min():.1f} .. {d.max():.1f})   "
              f"{E / np.median(d):9.1f} env-steps/us", flush=True)
    h.close()


if FUSED:
    envs = ROOT / "examples" / "envs"
    for E in (64, 1024, 16384, 65536):
        measure("CartPole twin [64,64]", capi.ENV_MODULE, E, module=envs / "cartpole_fused_plugin.hsaco", fused=True)
        measure("reacher3 [64,64]", capi.ENV_MODULE, E, module=envs / "reacher3_fused_plugin.hsaco", fused=True)
    for E in (1024, 65536):
        measure("reacher3 [256,256]", capi.ENV_MODULE, E, module=envs / "reacher3_fused_plugin.hsaco", hidden=256, fused=True)
    sys.exit(0)
for E in (64, 1024, 16384, 65536):
    measure("(a) CartPole twin plug-in", capi.ENV_MODULE, E, module=ROOT / "examples" / "envs" / "cartpole_plugin.hsaco")
    measure("(b) built-in CartPole, generic", capi.ENV_CARTPOLE, E, force_generic=True)
    measure("(c) reacher3 plug-in", capi.ENV_MODULE, E, module=ROOT / "examples" / "envs" / "reacher3_plugin.hsaco")
    measure("(d) reacher3 plug-in, normalised", capi.ENV_MODULE, E, module=ROOT / "examples" / "envs" / "reacher3_plugin.hsaco", normalize=True)
