"""Shared by tests/test_env_plugin_evaluate.py (CPU) and tests/test_gpu_env_plugin_evaluate.py (GPU): the argument block of a plug-in's fused evaluation
(include/device/dril_env_evaluate.h) for ctypes, a host build driven launch by launch, the library's per-trajectory rule over the K rows of a launch
(dril_traj_record.h: traj_record_lane_rows) compiled with g++, and a NumPy forward of the actor."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import fused_rollout_helpers as F
from test_env_plugin import Args, Desc

ROOT = Path(__file__).resolve().parents[1]
_PV = C.c_void_p
f32 = np.float32


class EvaluateDesc(C.Structure):
    """struct DrilEnvEvaluateDesc"""
    _fields_ = [("abi_version", C.c_uint32), ("args_size", C.c_uint32), ("tile", C.c_int32), ("threads", C.c_int32), ("max_width", C.c_int32), ("has_scaled", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class EvaluateArgs(C.Structure):
    """struct DrilEnvEvaluateArgs"""
    _fields_ = [("r", F.RolloutArgs), ("shadow", Args), ("deterministic", C.c_int32), ("n_record", C.c_int32), ("norm_eps", C.c_float), ("norm_clip", C.c_float),
                ("norm_mean", _PV), ("norm_var", _PV), ("rec_obs0", _PV), ("rec_act", _PV), ("rec_obs", _PV)]


class HostEvaluate:
    """E envs of an _eval plug-in's host build, stepped by dril_env_plugin_host_evaluate launch by launch; norm: None or (mean, var, eps, clip)"""

    def __init__(self, lib, E, episode_len=0, hidden=(64, 64), activation=0, action_start=1, scaled=False, norm=None, M=0):
        self.lib, self.E, self.hidden, self.activation, self.scaled, self.norm, self.M = lib, E, tuple(hidden), activation, scaled, norm, M
        d = self.desc = Desc.in_dll(lib, "dril_env_plugin_desc")
        self.edesc = EvaluateDesc.in_dll(lib, "dril_env_plugin_evaluate_desc")
        assert self.edesc.abi_version == 1 and self.edesc.args_size == C.sizeof(EvaluateArgs)
        self.S, self.D, self.A, self.discrete = d.S, d.D, d.A, bool(d.discrete)
        self.W = 1 if self.discrete else self.A
        self.Pa, self.Pc = F.net_size(self.D, hidden, self.A), F.net_size(self.D, hidden, 1)
        self.P = self.Pa + self.Pc + (0 if self.discrete else self.A)
        self.base = dict(E=E, episode_len=episode_len or d.episode_len, fixed_len=0, action_start=action_start)
        self.state = np.zeros((E, d.S), f32); self.sc = np.zeros(E, np.int32); self.ep = np.zeros(E, np.uint32); self.gs = np.zeros(E, np.uint32)
        self.obs = np.zeros((E, self.D), f32); self.act = np.zeros((E, self.W), np.uint32)
        self.sh_state = np.zeros((max(M, 1), d.S), f32); self.sh_sc = np.zeros(max(M, 1), np.int32); self.sh_ep = np.zeros(max(M, 1), np.uint32); self.sh_gs = np.zeros(max(M, 1), np.uint32)
        self.params = None; self.seed = 0

    def set_params(self, flat):
        self.params = np.ascontiguousarray(flat, f32); assert self.params.size == self.P

    def _env_args(self):
        p = lambda a: a.ctypes.data_as(_PV)
        return Args(**self.base, seed0=self.seed, state=p(self.state), step_count=p(self.sc), episode=p(self.ep), gstep=p(self.gs), obs=p(self.obs))

    def env_reset(self, seed):
        self.seed = seed
        self.lib.dril_env_plugin_host_reset(C.byref(self._env_args()))

    def launch(self, K, deterministic):
        """one launch of K env steps: rew (K, E), flags (K, E), obs0 (M, D), act (K, M, W) u32, obs (K, M, D)"""
        p = lambda a: a.ctypes.data_as(_PV)
        E, M = self.E, self.M
        rew = np.full((K, E), np.nan, f32); flags = np.full((K, E), 0xEE, np.uint8)
        obs0 = np.full((max(M, 1), self.D), np.nan, f32); ract = np.full((K, max(M, 1), self.W), 0xABCD, np.uint32); robs = np.full((K, max(M, 1), self.D), np.nan, f32)
        g = EvaluateArgs()
        g.r = F.RolloutArgs(env=self._env_args(), T=K, n_hidden=len(self.hidden), activation=self.activation, n_params=self.P, actor_off=0, critic_off=0, log_std_off=self.Pa + self.Pc,
                            params=p(self.params), act=p(self.act), rew=p(rew), flags=p(flags))
        for i, h in enumerate(self.hidden):
            g.r.hidden[i] = h
        g.deterministic, g.n_record = int(deterministic), M
        if self.norm is not None:
            mean, var, eps, clip = self.norm
            self._stats = (np.ascontiguousarray(mean, f32), np.ascontiguousarray(var, f32))
            g.norm_mean, g.norm_var, g.norm_eps, g.norm_clip = p(self._stats[0]), p(self._stats[1]), eps, clip
        if M:
            g.shadow = Args(E=M, episode_len=2 ** 31 - 1, fixed_len=1, action_start=self.base["action_start"], seed0=self.seed, state=p(self.sh_state), step_count=p(self.sh_sc),
                            episode=p(self.sh_ep), gstep=p(self.sh_gs))
            g.rec_obs0, g.rec_act, g.rec_obs = p(obs0), p(ract), p(robs)
        getattr(self.lib, "dril_env_plugin_host_evaluate" + ("_scaled" if self.scaled else ""))(C.byref(g))
        return rew, flags, obs0[:M], ract[:, :M], robs[:, :M]

    def run(self, steps, K, deterministic):
        """`steps` env steps in launches of K (the last one shortened), concatenated: rew, flags (steps, E); obs0 (M, D) of the first launch; act, obs (steps, M, .)"""
        parts, first = [], None
        for s0 in range(0, steps, K):
            out = self.launch(min(K, steps - s0), deterministic)
            first = out[2] if first is None else first
            parts.append(out)
        return (np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts]), first, np.concatenate([q[3] for q in parts]), np.concatenate([q[4] for q in parts]))


def actor_forward(params, D, hidden, A, activation, obs):
    """the actor of a parameter vector {W_1 b_1 ...}, W column-major (out x in), in float64; activation 0 = tanh"""
    assert activation == 0
    x, off, k = np.asarray(obs, np.float64), 0, D
    for i, o in enumerate(list(hidden) + [A]):
        W = params[off:off + k * o].astype(np.float64).reshape(k, o); b = params[off + k * o:off + k * o + o].astype(np.float64)
        x = x @ W + b
        if i < len(hidden):
            x = np.tanh(x)
        off += k * o + o; k = o
    return x


_ROWS_DRIVER = r'''
#include "dril_traj_record.h"
#include "device/dril_normalize.h"
extern "C" {
// the library's launch over the K rows a plug-in's evaluation kernel left (traj_record_rows_kernel): the lanes of the launch in the sequence `order` [M * lanes]
long long rows(int E, int M, int D, int W, int Tcap, int K, int t0, const float* rew, const unsigned char* flags, const float* obs0, const unsigned int* act, const float* obs,
               const int* order, const float* maps, int scaled, int discrete, int final_original, float* rec_obs, unsigned int* rec_act, float* rec_rew, int* length,
               unsigned char* end_flags, unsigned int* finished) {
    const dril::TrajRec r{M, D, W, Tcap, rec_obs, rec_act, rec_rew, length, end_flags, finished};
    const float *ol = maps, *oh = ol + D, *cl = oh + D, *ch = cl + W, *al = ch + W, *ah = al + W;
    const dril::TrajMaps x{scaled ? ol : nullptr, scaled ? oh : nullptr, discrete ? nullptr : cl, discrete ? nullptr : ch, (scaled && !discrete) ? al : nullptr,
                           (scaled && !discrete) ? ah : nullptr, discrete, final_original};
    const dril::TrajRows s{K, E, rew, flags, obs0, act, obs};
    const int lanes = D > W ? D : W;
    for (int i = 0; i < M * lanes; ++i) dril::traj_record_lane_rows(r, x, s, t0, order[i] / lanes, order[i] % lanes);
    return *finished;
}
void normalize(int n, const float* v, const float* mean, const float* var, float eps, float clip, float* out) { for (int i = 0; i < n; ++i) out[i] = dril::normalize_obs(v[i], mean[i], var[i], eps, clip); }
}
'''


def rows_driver(tmp):
    d = Path(tmp)
    src = d / "rows.cpp"; src.write_text(_ROWS_DRIVER)
    so = d / "rows.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / "dril.jl_amd" / "csrc"), "-I", str(ROOT / "include"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.rows.restype = C.c_longlong
    lib.rows.argtypes = [C.c_int] * 7 + [C.c_void_p] * 7 + [C.c_int] * 3 + [C.c_void_p] * 6
    lib.normalize.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_void_p]
    return lib


def normalize(lib, v, mean, var, eps, clip):
    """dril::normalize_obs (include/device/dril_normalize.h: the line nz_obs of dril_norm_wrap.h expands), element by element over rows of width len(mean)"""
    v = np.ascontiguousarray(v, f32)
    m = np.ascontiguousarray(np.broadcast_to(np.asarray(mean, f32), v.shape)); s = np.ascontiguousarray(np.broadcast_to(np.asarray(var, f32), v.shape))
    out = np.empty_like(v)
    lib.normalize(v.size, v.ctypes.data, m.ctypes.data, s.ctypes.data, eps, clip, out.ctypes.data)
    return out


def record_rows(lib, launches, E, M, D, W, Tcap, maps, rng):
    """the step-major recording from a sequence of launches (rew, flags, obs0, act, obs): one call of the library's rule per launch, lanes in random order"""
    ol, oh, cl, ch, al, ah, scaled, discrete, final_original = maps
    table = np.concatenate([ol, oh, cl, ch, al, ah]).astype(f32)
    lanes = max(D, W)
    rec_obs = np.zeros((Tcap + 1) * M * D, f32); rec_act = np.zeros(Tcap * M * W, np.uint32); rec_rew = np.zeros(Tcap * M, f32)
    length = np.full(M, -7, np.int32); end = np.full(M, 0xEE, np.uint8); finished = np.zeros(1, np.uint32)
    p = lambda a: np.ascontiguousarray(a).ctypes.data
    t0 = 0
    for rew, flags, obs0, act, obs in launches:
        K = rew.shape[0]
        keep = [np.ascontiguousarray(a) for a in (rew, flags, obs0, act, obs, rng.permutation(M * lanes).astype(np.int32))]
        lib.rows(E, M, D, W, Tcap, K, t0, *[a.ctypes.data for a in keep[:5]], keep[5].ctypes.data, p(table), int(scaled), int(discrete), int(final_original),
                 rec_obs.ctypes.data, rec_act.ctypes.data, rec_rew.ctypes.data, length.ctypes.data, end.ctypes.data, finished.ctypes.data)
        t0 += K
    return int(finished[0]), rec_obs.reshape(Tcap + 1, M, D), rec_act.reshape(Tcap, M, W), rec_rew.reshape(Tcap, M), length, end
