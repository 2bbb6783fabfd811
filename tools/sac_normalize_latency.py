#!/usr/bin/env python3
"""Per-step collection time of a SAC handle with NormalizeWrapperEnv on against off (docs/sac.md, "NormalizeWrapperEnv"), policy actions, warmed up, the two
settings alternating on one device, from dril_sac_profile_get:
  long   one dril_sac_collect_rollout of --steps steps (HIP events): the collection's opening observe amortised to nothing;
  tf1    dril_sac_iterate at train_freq = 1 without gradient steps (in-stream stamps): every env step is a collection of its own, so the wrapper's opening observe
         (moments + apply) runs per step — the shape dril_sac_train / sac_train_ have at the default train_freq.
--wide D also times a plug-in with D observation dims compiled here (the column-per-thread branch of the moments kernel).
    python tools/sac_normalize_latency.py [--steps 200] [--reps 5] [--wide 512]"""
import argparse
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g  # noqa: E402


_WIDE = '''#include "device/dril_env_plugin.h"
struct Wide {
    static constexpr int S = 2, D = WIDE_D, A = 1;
    static constexpr bool discrete = false;
    static constexpr int episode_len = 200;
    static constexpr float action_low[A] = {-1.0f}, action_high[A] = {1.0f};
    static constexpr const char* name = "Wide";
    DRIL_ENV_FN static void reset(const DrilEnvRng& rng, float* st) { const DrilEnvWords r = rng.words(0); st[0] = DrilEnvRng::u01(r.w[0]) * 2.0f - 1.0f; st[1] = DrilEnvRng::u01(r.w[1]) - 0.5f; }
    DRIL_ENV_FN static void observe(const float* st, float* obs) { for (int i = 0; i < D; ++i) obs[i] = (float)(1 + i % 7) * st[i & 1] + (float)(i % 11); }
    DRIL_ENV_FN static float step(float* st, const float* act_f, int act_i, bool* terminated) {
        st[0] = 0.9f * st[0] + 0.3f * act_f[0]; st[1] = 0.8f * st[1] + 0.1f * st[0]; *terminated = false; return -st[0] * st[0];
    }
};
DRIL_ENV_PLUGIN(Wide)
'''
PLUGINS = {"reacher3": ROOT / "examples" / "envs" / "reacher3_plugin.hsaco"}


def build_wide(D, tmp):
    src = Path(tmp) / "wide.hip"; src.write_text(_WIDE)
    out = Path(tmp) / f"wide{D}.hsaco"
    subprocess.run(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "--no-gpu-bundle-output", "-O3", "-fno-slp-vectorize", "-std=c++17", f"-DWIDE_D={D}",
                    "-I", str(ROOT / "include"), str(src), "-o", str(out)], check=True)
    PLUGINS[f"wide{D}"] = out


def handle(pkg, name, E, tf1):
    if name == "pendulum":
        env = pkg.PendulumEnv()
        path = None
    else:
        path = PLUGINS[name]
        env = pkg.host.ModuleEnv(str(path), pkg.describe_env_module(path), 0)
    alg = pkg.SAC(buffer_capacity=1 << 18, train_freq=1, gradient_steps=0) if tf1 else pkg.SAC(buffer_capacity=1 << 18)
    layer = pkg.SACLayer(env.observation_space(), env.action_space())
    h = pkg.SacHandle(pkg.make_sac_config(env, E, alg, layer, seed=1, profile_events=True), env_module=path)
    h.set_params(pkg.sac_flatten_params(layer.initialparameters(np.random.default_rng(0))))
    h.env_reset(1)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--wide", type=int, default=0)
    a = ap.parse_args()
    pkg = g.load_package()
    names = ["pendulum", "reacher3"]
    tmp = tempfile.TemporaryDirectory()
    if a.wide:
        build_wide(a.wide, tmp.name); names.append(f"wide{a.wide}")
    for name, E, tf1 in [(n, E, m) for n in names for E in (64, 4096) for m in (False, True)]:
        if True:
            hs = {"off": handle(pkg, name, E, tf1), "on": handle(pkg, name, E, tf1)}
            hs["on"].normalize_enable()
            us = {k: [] for k in hs}
            for h in hs.values():
                h.collect_rollout(1, True)                              # (dril_sac_iterate wants a non-empty ring only when it updates; harmless)
            for rep in range(a.reps + 1):
                for k, h in hs.items():
                    h.profile_reset()
                    if tf1:
                        h.iterate(a.steps, want_stats=False)
                    else:
                        h.collect_rollout(a.steps, False)
                    p = h.profile()
                    if rep:                                             # the first round warms up
                        us[k].append(1e3 * p["collect_ms"] / p["collect_steps"])
            print(f"{name:9s} E={E:5d} {'tf1 ' if tf1 else 'long'}  off {np.median(us['off']):7.2f} us/step [{min(us['off']):.2f} .. {max(us['off']):.2f}]   "
                  f"on {np.median(us['on']):7.2f} us/step [{min(us['on']):.2f} .. {max(us['on']):.2f}]   +{np.median(us['on']) - np.median(us['off']):.2f} us", flush=True)
            for h in hs.values():
                h.close()


if __name__ == "__main__":
    main()
