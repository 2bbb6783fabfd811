"""Deployment policies: mirror of src/deployment/deployment_policy.jl over include/dril_policy.h.

    extract_policy(agent)            -> NeuralPolicy        actor parameters + action adapter, nothing else
    extract_policy(agent, norm_env)  -> NormWrapperPolicy   ... + the wrapper's frozen observation statistics, epsilon, clip_obs
    RandomPolicy(env | action_space), ConstantPolicy(action)

A NeuralPolicy / NormWrapperPolicy owns one `dril_policy*`: a light device object that turns raw observations into env actions in one kernel launch
(policy_act_kernel; docs/deployment.md).  There is no host fallback: without libdril_hip.so and an MI355X, constructing one raises.  Calls follow the
reference's shape rule: one observation in -> one action out; a list or (B, D) array in -> B actions out.
"""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Optional

import numpy as np

from . import _capi as capi
from .host import ACTIVATIONS, Box, Discrete, DrilError, Handle, _env_handle, _norm_view, _normalize_kw

KINDS = ("Categorical", "DiagGaussian", "SquashedDiagGaussian")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def actor_tree_to_flat(actor_head: dict) -> np.ndarray:
    """{layer_k: {weight (out x in), bias}} -> the actor's slice of dril_get_params (weights column-major)"""
    parts = []
    for l in sorted(actor_head, key=lambda s: int(s.rsplit("_", 1)[1])):
        parts.append(np.asarray(actor_head[l]["weight"], np.float32).ravel(order="F"))
        parts.append(np.asarray(actor_head[l]["bias"], np.float32).ravel())
    return np.concatenate(parts)


def actor_flat_to_tree(flat: np.ndarray, dims) -> dict:
    tree, off = {}, 0
    for l, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        w = flat[off:off + i * o].reshape((o, i), order="F").copy(); off += i * o
        tree[f"layer_{l + 1}"] = {"weight": w, "bias": flat[off:off + o].copy()}; off += o
    return tree


def make_policy_desc(kind: int, obs_dim: int, action_dim: int, hidden_dims, activation, *, action_start: int = 0, action_low=None, action_high=None,
                     clip_obs: Optional[float] = None, epsilon: float = 1e-8, device: int = 0) -> capi.DrilPolicyDesc:
    d = capi.DrilPolicyDesc()
    d.abi_version, d.kind, d.obs_dim, d.action_dim, d.action_start = capi.POLICY_ABI_VERSION, kind, obs_dim, action_dim, action_start
    hidden_dims = tuple(int(h) for h in hidden_dims)
    d.n_hidden = len(hidden_dims)
    for l, h in enumerate(hidden_dims[:4]):
        d.hidden[l] = h
    d.activation = ACTIVATIONS.index(activation) if isinstance(activation, str) else int(activation)
    d.has_norm = 0 if clip_obs is None else 1
    d.clip_obs, d.epsilon, d.device = (0.0 if clip_obs is None else clip_obs), epsilon, device
    if action_low is not None:
        lo, hi = np.broadcast_to(np.asarray(action_low, np.float32).ravel(), (action_dim,)), np.broadcast_to(np.asarray(action_high, np.float32).ravel(), (action_dim,))
        for a in range(action_dim):
            d.action_low[a], d.action_high[a] = float(lo[a]), float(hi[a])
    return d


class NeuralPolicy:
    """NeuralPolicy (deployment_policy.jl:3-41) on the device.  Build with `extract_policy`, `NeuralPolicy.create(...)` (host arrays),
    `NeuralPolicy.from_handle(handle)` (device-to-device snapshot of a training handle) or `load_policy(path)`."""

    def __init__(self, ptr: C.c_void_p, lib: Optional[C.CDLL] = None):
        self.lib = lib or capi.load_library()
        self._p = ptr
        self.desc = capi.DrilPolicyDesc()
        self._chk(self.lib.dril_policy_describe(self._p, C.byref(self.desc)))
        self.kind, self.D, self.A = self.desc.kind, self.desc.obs_dim, self.desc.action_dim
        self.discrete = self.kind == capi.POLICY_CATEGORICAL
        self.hidden_dims = tuple(self.desc.hidden[l] for l in range(self.desc.n_hidden))
        self.activation = ACTIVATIONS[self.desc.activation]

    # construction
    @classmethod
    def create(cls, desc: capi.DrilPolicyDesc, actor_params, log_std=None, obs_mean=None, obs_var=None, lib: Optional[C.CDLL] = None):
        lib = lib or capi.load_library()
        flat = np.ascontiguousarray(actor_params, np.float32).ravel()
        ls, mu, var = (None if a is None else np.ascontiguousarray(a, np.float32).ravel() for a in (log_std, obs_mean, obs_var))
        if ls is not None and ls.size != desc.action_dim:
            raise ValueError(f"log_std holds {ls.size} entries, the action space has {desc.action_dim}")
        if desc.has_norm and (mu is None or var is None or mu.size != desc.obs_dim or var.size != desc.obs_dim):
            raise ValueError(f"obs_mean / obs_var must hold obs_dim = {desc.obs_dim} entries each")
        ptr = C.c_void_p()
        rc = lib.dril_policy_create(C.byref(desc), _p(flat), flat.size, _p(ls), _p(mu), _p(var), C.byref(ptr))
        if rc != capi.OK:
            raise DrilError(rc, (lib.dril_policy_last_error(None) or b"").decode())
        return (NormWrapperPolicy if desc.has_norm else NeuralPolicy)(ptr, lib)

    @classmethod
    def from_handle(cls, handle, with_norm: bool = False):
        """extract_policy on a training handle (host.Handle or sac.SacHandle): copies device-to-device, reads the handle only"""
        lib, ptr = handle.lib, C.c_void_p()
        fn = lib.dril_policy_from_handle if isinstance(handle, Handle) else lib.dril_policy_from_sac_handle
        rc = fn(handle._h, int(with_norm), C.byref(ptr))
        if rc != capi.OK:
            raise DrilError(rc, (lib.dril_policy_last_error(None) or b"").decode())
        return (NormWrapperPolicy if with_norm else NeuralPolicy)(ptr, lib)

    def close(self):
        if self._p:
            self.lib.dril_policy_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != capi.OK:
            raise DrilError(rc, (self.lib.dril_policy_last_error(self._p) or b"").decode())

    # inspection
    @property
    def action_space(self):
        if self.discrete:
            return Discrete(self.A, self.desc.action_start)
        return Box(tuple(self.desc.action_low[a] for a in range(self.A)), tuple(self.desc.action_high[a] for a in range(self.A)))

    def get_params(self):
        """-> (actor parameters, flat, in the layout of the actor's slice of dril_get_params; log_std or None)"""
        flat = np.empty(int(self.lib.dril_policy_param_count(self._p)), np.float32)
        ls = None if self.discrete else np.empty(self.A, np.float32)
        self._chk(self.lib.dril_policy_get_params(self._p, _p(flat), flat.size, _p(ls)))
        return flat, ls

    def get_norm(self):
        mean, var = np.empty(self.D, np.float32), np.empty(self.D, np.float32)
        self._chk(self.lib.dril_policy_get_norm(self._p, _p(mean), _p(var)))
        return mean, var

    def set_seed(self, seed: int):
        self._chk(self.lib.dril_policy_set_seed(self._p, int(seed) & (2 ** 64 - 1)))

    def set_threshold(self, threshold: int):
        self._chk(self.lib.dril_policy_set_threshold(self._p, int(threshold)))

    def kernel_time(self, enable: bool = True) -> float:
        """switch the HIP-event bracket of act calls on / off; -> device milliseconds of the last bracketed call (-1.0: none yet)"""
        ms = C.c_double()
        self._chk(self.lib.dril_policy_kernel_time(self._p, int(enable), C.byref(ms)))
        return ms.value

    # acting
    def act(self, obs, deterministic: bool = True, noise=None, want_raw: bool = False):
        """obs (B, D) raw observations -> env actions (B,) int32 | (B, A) float32; want_raw: -> (raw, env)"""
        obs = np.ascontiguousarray(obs, np.float32)
        if obs.ndim != 2 or obs.shape[1] != self.D:
            raise ValueError(f"observations must be (batch, {self.D}), got {obs.shape}")
        B = obs.shape[0]
        shape, dt = ((B,), np.int32) if self.discrete else ((B, self.A), np.float32)
        env, raw = np.empty(shape, dt), (np.empty(shape, dt) if want_raw else None)
        if noise is not None:
            noise = np.ascontiguousarray(noise, np.float64 if self.discrete else np.float32)
            if noise.size != B * (1 if self.discrete else self.A):
                raise ValueError("noise: one f64 uniform per observation (Categorical) or action_dim f32 normals per observation")
        self._chk(self.lib.dril_policy_act(self._p, _p(obs), B, int(deterministic), _p(noise), _p(raw), _p(env)))
        return (raw, env) if want_raw else env

    def __call__(self, obs, deterministic: bool = True, rng: Optional[np.random.Generator] = None):
        return _call_with_shape_rule(self, obs, deterministic, rng)

    def _draw(self, rng: np.random.Generator, B: int):
        return rng.random(B) if self.discrete else rng.standard_normal((B, self.A)).astype(np.float32)

    def _format(self, env_row):
        return int(env_row) if self.discrete else env_row


class NormWrapperPolicy(NeuralPolicy):
    """NormWrapperPolicy (deployment_policy.jl:44-74): the same object with frozen observation statistics; observations go in RAW"""

    @property
    def obs_rms(self):
        mean, var = self.get_norm()
        return {"mean": mean, "var": var}

    @property
    def eps(self) -> float:
        return self.desc.epsilon

    @property
    def clip_obs(self) -> float:
        return self.desc.clip_obs


def _call_with_shape_rule(policy, obs, deterministic, rng):
    """deployment_policy.jl:25-41: size(obs) == size(observation_space) is ONE observation -> one action; anything else is a batch -> a list of actions"""
    single = not isinstance(obs, (list, tuple)) and np.ndim(obs) == 1
    batch = np.asarray(obs, np.float32).reshape(1, -1) if single else np.stack([np.asarray(o, np.float32).ravel() for o in obs])
    noise = None if deterministic or rng is None else policy._draw(rng, batch.shape[0])
    env = policy.act(batch, deterministic, noise)
    acts = [policy._format(a) for a in env]
    return acts[0] if single else acts


def _layer_policy_desc(layer, *, clip_obs=None, epsilon=1e-8, device=0) -> capi.DrilPolicyDesc:
    asp = layer.action_space
    if isinstance(asp, Discrete):
        return make_policy_desc(capi.POLICY_CATEGORICAL, layer.obs_dim, asp.n, layer.hidden_dims, layer.activation, action_start=asp.start, clip_obs=clip_obs, epsilon=epsilon, device=device)
    squashed = type(layer).__name__ == "SACLayer"                       # SquashedDiagGaussian + TanhScaleAdapter (sac.jl:72-85); PPO's Box layer: DiagGaussian + ClampAdapter
    kind = capi.POLICY_SQUASHED_DIAG_GAUSSIAN if squashed else capi.POLICY_DIAG_GAUSSIAN
    return make_policy_desc(kind, layer.obs_dim, len(asp.low), layer.hidden_dims, layer.activation, action_low=asp.low, action_high=asp.high, clip_obs=clip_obs, epsilon=epsilon, device=device)


def _norm_of(norm_env):
    """(obs_mean, obs_var, epsilon, clip_obs) of a NormalizeWrapperEnv: a DeviceParallelEnv / DeviceModuleEnv with normalize= and a bound handle, a Handle wrapped by
    normalize_enable, or a SacHandle with its wrapper on"""
    h = norm_env if hasattr(norm_env, "norm_get_stats") else _env_handle(norm_env) if hasattr(norm_env, "handle") else None
    if h is None:
        raise ValueError("extract_policy(agent, norm_env): the env has no bound handle yet (its statistics live on the device: train or bind first)")
    h = _norm_view(h)                                                           # an external handle's wrapper answers through dril_ext_normalize_*
    kw = _normalize_kw(norm_env) if hasattr(norm_env, "_kw") else None           # DeviceParallelEnv(normalize=...) / DeviceModuleEnv(..., normalize=...) / a wrapped DeviceArrayParallelEnv
    if kw is None and hasattr(h, "normalize_config"):
        try:
            kw = h.normalize_config()                                           # the keywords as the handle holds them (normalize_enable verbs)
        except DrilError:
            kw = None
    if not kw:
        raise DrilError(capi.ERR_NOT_INITIALISED, "extract_policy(agent, norm_env): the env is not wrapped by NormalizeWrapperEnv")
    st = h.norm_get_stats()
    return np.asarray(st["obs_mean"], np.float32), np.asarray(st["obs_var"], np.float32), float(kw.get("epsilon", 1e-8)), float(kw.get("clip_obs", 10.0))


def extract_policy(agent, norm_env=None, *, device: int = 0):
    """extract_policy(agent) / extract_policy(agent, norm_env) (deployment_policy.jl:15-22, :52-58) for Agent and SACAgent"""
    params = agent.train_state.parameters if hasattr(agent, "train_state") else agent.parameters
    mean = var = None
    kw = {}
    if norm_env is not None:
        mean, var, eps, clip = _norm_of(norm_env)
        kw = dict(clip_obs=clip, epsilon=eps)
    desc = _layer_policy_desc(agent.layer, device=device, **kw)
    return NeuralPolicy.create(desc, actor_tree_to_flat(params["actor_head"]), params.get("log_std"), mean, var)


class RandomPolicy:
    """RandomPolicy(env | action_space) (deployment_policy.jl:76-101): rand(rng, action_space) whatever the observation"""

    def __init__(self, env_or_space):
        self.action_space = env_or_space if isinstance(env_or_space, (Box, Discrete)) else env_or_space.action_space()
        self._default_rng = np.random.default_rng()

    def __call__(self, obs=None, deterministic: bool = True, rng: Optional[np.random.Generator] = None):
        rng = rng or self._default_rng
        sp = self.action_space
        if isinstance(sp, Discrete):
            return int(sp.start + rng.integers(sp.n))
        lo, hi = np.asarray(sp.low, np.float32), np.asarray(sp.high, np.float32)
        return (lo + rng.random(lo.shape, np.float32) * (hi - lo)).astype(np.float32)


class ConstantPolicy:
    """ConstantPolicy(action) (deployment_policy.jl:104-127): raises when deterministic is False, warns when handed an rng"""

    def __init__(self, action):
        self.action = action

    def __call__(self, obs=None, deterministic: bool = True, rng=None):
        if not deterministic:
            raise ValueError("ConstantPolicy is deterministic")
        if rng is not None:
            warnings.warn("rng is not used by ConstantPolicy")
        return self.action
