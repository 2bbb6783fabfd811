"""Shared by tests/test_env_plugin_fused.py (CPU) and tests/test_gpu_env_plugin_fused.py (GPU): the argument block of the fused rollout
(include/device/dril_env_rollout.h) for ctypes, a host build driven like a Handle, and the comparison of a collection with the CPU oracle — the loop and the
tolerances of test_collect_rollout_matches_oracle (tests/test_gpu_parity.py), restated."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from test_env_plugin import Args, Desc

ROOT = Path(__file__).resolve().parents[1]
ENVS = ROOT / "examples" / "envs"
_PV = C.c_void_p
(BUF_OBSERVATIONS, BUF_ACTIONS, BUF_REWARDS, BUF_ADVANTAGES, BUF_RETURNS, BUF_LOGPROBS, BUF_VALUES, BUF_FLAGS, BUF_BOOTSTRAP, BUF_LAST_VALUES) = range(10)


class RolloutDesc(C.Structure):
    """struct DrilEnvRolloutDesc"""
    _fields_ = [("abi_version", C.c_uint32), ("args_size", C.c_uint32), ("tile", C.c_int32), ("threads", C.c_int32), ("max_width", C.c_int32), ("has_scaled", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class RolloutArgs(C.Structure):
    """struct DrilEnvRolloutArgs"""
    _fields_ = [("env", Args), ("T", C.c_int32), ("n_hidden", C.c_int32), ("activation", C.c_int32), ("n_params", C.c_int32), ("hidden", C.c_int32 * 4),
                ("actor_off", C.c_int32), ("critic_off", C.c_int32), ("log_std_off", C.c_int32), ("reserved2", C.c_int32), ("params", _PV), ("noise", _PV),
                ("obs", _PV), ("act", _PV), ("rew", _PV), ("logp", _PV), ("val", _PV), ("boot", _PV), ("flags", _PV), ("last_values", _PV), ("ep_ret", _PV), ("ep_len", _PV)]


def host_build(name, tmp, flags=("-march=x86-64-v3",), defines=()):
    """g++ build of examples/envs/<name>_plugin.hip with DRIL_ENV_PLUGIN_HOST; the default target is the CPU oracle's own (oracle/Makefile): products contract into FMAs"""
    so = Path(tmp) / f"{name}_host.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-x", "c++", "-DDRIL_ENV_PLUGIN_HOST", *[f"-D{d}" for d in defines], *flags, "-I", str(ROOT / "include"),
                    str(ENVS / f"{name}_plugin.hip"), "-o", str(so)], check=True)
    return C.CDLL(str(so))


def net_size(D, hidden, out):
    n, k = 0, D
    for h in list(hidden) + [out]:
        n += k * h + h; k = h
    return n


class HostRollout:
    """E envs of a fused plug-in's host build, collected by dril_env_plugin_host_rollout; the surface of Handle the comparison needs"""

    def __init__(self, lib, E, T, episode_len=0, hidden=(64, 64), activation=0, action_start=1, fixed_len=False, monitor=False, scaled=False, gamma=0.99, gae_lambda=0.95):
        self.lib, self.E, self.T, self.hidden, self.activation, self.scaled = lib, E, T, tuple(hidden), activation, scaled
        d = self.desc = Desc.in_dll(lib, "dril_env_plugin_desc")
        self.rdesc = RolloutDesc.in_dll(lib, "dril_env_plugin_rollout_desc")
        assert self.rdesc.abi_version == 1 and self.rdesc.args_size == C.sizeof(RolloutArgs)
        self.S, self.D, self.A, self.discrete = d.S, d.D, d.A, bool(d.discrete)
        self.Pa, self.Pc = net_size(self.D, hidden, self.A), net_size(self.D, hidden, 1)
        self.P = self.Pa + self.Pc + (0 if self.discrete else self.A)
        self.gamma, self.gae_lambda = gamma, gae_lambda
        self.base = dict(E=E, episode_len=episode_len or d.episode_len, fixed_len=int(fixed_len), action_start=action_start)
        f32 = np.float32
        self.state = np.zeros((E, d.S), f32); self.sc = np.zeros(E, np.int32); self.ep = np.zeros(E, np.uint32); self.gs = np.zeros(E, np.uint32)
        self.mon_ret = np.zeros(E, f32); self.mon_len = np.zeros(E, np.int32); self.monitor = monitor
        self.e_term = np.zeros(E, np.uint8); self.e_trunc = np.zeros(E, np.uint8); self.e_tobs = np.zeros((E, self.D), f32); self.e_obs = np.zeros((E, self.D), f32)
        N = E * T
        self.bufs = {BUF_OBSERVATIONS: np.zeros((N, self.D), f32), BUF_ACTIONS: np.zeros(N, np.int32) if self.discrete else np.zeros((N, self.A), f32),
                     BUF_REWARDS: np.zeros(N, f32), BUF_ADVANTAGES: np.zeros(N, f32), BUF_RETURNS: np.zeros(N, f32), BUF_LOGPROBS: np.zeros(N, f32), BUF_VALUES: np.zeros(N, f32),
                     BUF_FLAGS: np.zeros(N, np.uint8), BUF_BOOTSTRAP: np.zeros(N, f32), BUF_LAST_VALUES: np.zeros(E, f32)}
        self.ep_ret = np.full(N, np.nan, f32); self.ep_len = np.full(N, -1, np.int32)
        self.params = None; self.noise = None; self.seed = 0

    def set_params(self, flat):
        self.params = np.ascontiguousarray(flat, np.float32); assert self.params.size == self.P

    def set_noise(self, noise):
        self.noise = None if noise is None else np.ascontiguousarray(noise, np.float64 if self.discrete else np.float32)

    def _env_args(self):
        p = lambda a: a.ctypes.data_as(_PV)
        a = Args(**self.base, seed0=self.seed, state=p(self.state), step_count=p(self.sc), episode=p(self.ep), gstep=p(self.gs),
                 terminated=p(self.e_term), truncated=p(self.e_trunc), terminal_obs=p(self.e_tobs), obs=p(self.e_obs))
        if self.monitor:
            a.mon_cur_ret, a.mon_cur_len = p(self.mon_ret), p(self.mon_len)
        return a

    def env_reset(self, seed):
        self.seed = seed
        self.lib.dril_env_plugin_host_reset(C.byref(self._env_args()))

    def env_get_state(self):
        return self.state.copy(), self.sc.copy()

    def collect_rollout(self, gae):
        """gae(E, T, gamma, lambda, rewards, values, flags, bootstrap, last_values, advantages, returns): GAE on the rows the rollout wrote (the oracle's orc_gae)"""
        p = lambda a: a.ctypes.data_as(_PV)
        b = self.bufs
        g = RolloutArgs(env=self._env_args(), T=self.T, n_hidden=len(self.hidden), activation=self.activation, n_params=self.P, actor_off=0, critic_off=self.Pa, log_std_off=self.Pa + self.Pc,
                        params=p(self.params), noise=None if self.noise is None else p(self.noise), obs=p(b[BUF_OBSERVATIONS]), act=p(b[BUF_ACTIONS]), rew=p(b[BUF_REWARDS]),
                        logp=p(b[BUF_LOGPROBS]), val=p(b[BUF_VALUES]), boot=p(b[BUF_BOOTSTRAP]), flags=p(b[BUF_FLAGS]), last_values=p(b[BUF_LAST_VALUES]))
        for i, h in enumerate(self.hidden):
            g.hidden[i] = h
        if self.monitor:
            g.ep_ret, g.ep_len = p(self.ep_ret), p(self.ep_len)
        getattr(self.lib, "dril_env_plugin_host_rollout" + ("_scaled" if self.scaled else ""))(C.byref(g))
        self.noise = None                                                   # injected noise covers one collection, as dril_debug_set_noise
        assert gae(self.E, self.T, self.gamma, self.gae_lambda, p(b[BUF_REWARDS]), p(b[BUF_VALUES]), p(b[BUF_FLAGS]), p(b[BUF_BOOTSTRAP]), p(b[BUF_LAST_VALUES]),
                   p(b[BUF_ADVANTAGES]), p(b[BUF_RETURNS])) == 0
        return 1.0

    def buffer(self, which):
        return self.bufs[which].copy()


def flip_report(o, cfg, obs, u, a_dev, a_orc, where=""):
    """_flip_report of tests/test_gpu_parity.py: a discrete action may differ from the oracle's only where u sits within 1e-6 of a CDF edge (the oracle's
    probabilities give the edges); returns the number of flips"""
    flip = np.flatnonzero(np.asarray(a_dev).reshape(-1) != np.asarray(a_orc).reshape(-1))
    if flip.size == 0:
        return 0
    ob = np.ascontiguousarray(np.asarray(obs, np.float32).reshape(-1, o.D)[flip])
    probs = np.stack([np.exp(o.evaluate_actions(ob, np.full(flip.size, cfg.action_start + a, np.int32))[1].astype(np.float64)) for a in range(o.A)], axis=1)
    edges = np.cumsum(probs, axis=1)[:, :-1]
    margin = np.abs(edges - np.asarray(u, np.float64).reshape(-1)[flip][:, None]).min(axis=1)
    print(f"[flips]{where} {flip.size} of {np.asarray(a_orc).size} actions differ; max |u - CDF edge| = {margin.max():.2e}")
    assert margin.max() <= 1e-6, f"{where}: an action differs with u {margin.max():.3e} away from the nearest CDF edge"
    return int(flip.size)


ORACLE_CASES = [("cartpole", 0, 64, 48, 500, False), ("cartpole", 0, 100, 40, 9, True), ("pendulum", 1, 33, 50, 12, False)]   # of test_collect_rollout_matches_oracle


def oracle_params(P, seed):
    return (np.random.default_rng(seed).standard_normal(P) * 0.4).astype(np.float32)           # _params(P, seed, 0.4)


def compare_with_oracle(make, oracle_mod, cfg, collect, label):
    """the body of test_collect_rollout_matches_oracle: `make()` gives a fresh collector (a Handle on the fused path, or a HostRollout) with P, discrete, A, set_params,
    env_reset, set_noise, buffer, env_get_state; collect(h) runs one collection including GAE.  Injected noise (two collections without a reset), then the shared Philox
    stream.  Returns the collector of the last pass."""
    E, T, L = cfg.n_envs, cfg.n_steps, cfg.episode_len
    seed = 17 + E
    for inject in (True, False):
        h, o = make(), oracle_mod.Oracle(cfg)
        assert h.P == o.P
        flat = oracle_params(h.P, seed); h.set_params(flat); o.set_params(flat)
        h.env_reset(seed); o.env_reset(seed)
        if inject:
            rng = np.random.default_rng(E)
            noise = rng.random(E * T) if h.discrete else rng.standard_normal((E * T, h.A)).astype(np.float32)
            h.set_noise(noise); o.set_noise(noise)
        for rollout in range(2):                       # the env is NOT reset between rollouts (trajectory.jl:26)
            collect(h); o.collect_rollout()
            ah, ao = h.buffer(BUF_ACTIONS).reshape(T, E, -1), o.buffer(BUF_ACTIONS).reshape(T, E, -1)
            if h.discrete:
                ok = np.cumprod((ah == ao).all(axis=2), axis=0).astype(bool)     # env matches up to its first action flip
                share = ok.all(axis=0).mean()
                print(f"[{label}] inject={inject} rollout={rollout}: share of envs that never flip {share:.4f}")
                assert share >= 0.98
                if inject and rollout == 0:                                       # the FIRST difference of an env must be a CDF-edge flip
                    first = ok.copy(); first[1:] = ok[:-1]; first[0] = True
                    fo_obs = o.buffer(BUF_OBSERVATIONS).reshape(T, E, -1)
                    sel = first & ~ok
                    if sel.any():
                        flip_report(o, cfg, fo_obs[sel], noise.reshape(T, E)[sel], ah[sel], ao[sel], f" {label}:")
            else:
                ok = np.ones((T, E), bool)
            full = ok.all(axis=0)                       # GAE looks ahead, so compare whole envs that never diverged
            for which, tol in ((BUF_OBSERVATIONS, 2e-5), (BUF_VALUES, 5e-5), (BUF_LOGPROBS, 1e-4), (BUF_REWARDS, 1e-4), (BUF_ADVANTAGES, 1e-3), (BUF_RETURNS, 1e-3)):
                a, b = h.buffer(which).reshape(T, E, -1), o.buffer(which).reshape(T, E, -1)
                print(f"[{label}] inject={inject} rollout={rollout} buffer {which}: max |diff| {np.abs(a[:, full] - b[:, full]).max():.3e}")
                np.testing.assert_allclose(a[:, full], b[:, full], atol=tol, rtol=tol, err_msg=f"{label} buffer {which}")
            fh, fo = h.buffer(BUF_FLAGS).reshape(T, E), o.buffer(BUF_FLAGS).reshape(T, E)
            np.testing.assert_array_equal(fh[:, full], fo[:, full])
            tr = (fo & 2).astype(bool) & full[None, :]
            np.testing.assert_allclose(h.buffer(BUF_BOOTSTRAP).reshape(T, E)[tr], o.buffer(BUF_BOOTSTRAP).reshape(T, E)[tr], atol=5e-5, rtol=5e-5)
            live = full & (fo[T - 1] == 0)                # V(new_obs) is only consumed for rollout-limited tails (trajectory.jl:65-70)
            np.testing.assert_allclose(h.buffer(BUF_LAST_VALUES)[live], o.buffer(BUF_LAST_VALUES)[live], atol=5e-5, rtol=5e-5)
            np.testing.assert_allclose(h.buffer(BUF_RETURNS), h.buffer(BUF_ADVANTAGES) + h.buffer(BUF_VALUES), atol=1e-5)
            if not inject:
                break
            st, sc = h.env_get_state(); o.env_set_state(st, sc)           # keep the two simulators in lock-step for the second rollout
        if L < T:
            assert (fh & 2).any()
    return h
