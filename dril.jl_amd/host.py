"""Host-side mirror of DRiL.jl's interface for the rollout + PPO-update hot path.

The reference is Julia (no Julia toolchain exists in the build image), so this module mirrors the
reference's types and verbs in Python on top of the C ABI (include/dril_hip.h); the Julia `ccall`
shim a maintainer would use lives in dril.jl_amd/julia/DRiLHIP.jl and binds the same symbols.

Names follow the reference (Julia's `f!` is spelled `f_`):
    Box, Discrete                      src/spaces.jl
    ActorCriticLayer(...)              src/layers/layer_constructors.jl:3-96
    PPO(...)                           src/algorithms/ppo.jl:25-40
    Agent(layer, alg)                  src/algorithms/ppo.jl:42-62
    DeviceParallelEnv <: AbstractParallelEnv   stands in for MultiThreadedParallelEnv
                                       (src/environment_wrappers/multithreadedParallelEnv.jl)
    RolloutBuffer, collect_rollout_    src/buffers/rollout_buffer.jl:6-18,46-90
    train_(agent, env, alg, max_steps) src/algorithms/ppo.jl:100-325

All arithmetic happens in libdril_hip.so; nothing here computes the hot path and there is no CPU
fallback (loading fails loudly when the library is missing).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
import sys
import time
import warnings
from dataclasses import dataclass, field, asdict
from typing import Optional, Sequence

import numpy as np

from . import _capi as capi, _normalize
from ._capi import DrilConfig, DrilPPOStats


class DrilError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[dril status {code}] {msg}")
        self.code = code


# --------------------------------------------------------------------------------------------
# spaces (src/spaces.jl)
# --------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Box:
    low: tuple
    high: tuple

    @property
    def shape(self):
        return (len(self.low),)


@dataclass(frozen=True)
class Discrete:
    n: int
    start: int = 1  # src/spaces.jl:160


# env descriptors: CartPoleEnv / PendulumEnv come from ClassicControlEnvironments.jl in the reference
# (test/Project.toml:22-23); here they only carry the constructor kwargs the device simulator needs.
@dataclass
class CartPoleEnv:
    max_steps: int = 500
    action_start: int = 1
    kind: int = capi.ENV_CARTPOLE

    def observation_space(self):
        return Box((-4.8, -math.inf, -0.41887903, -math.inf), (4.8, math.inf, 0.41887903, math.inf))

    def action_space(self):
        return Discrete(2, self.action_start)


@dataclass
class PendulumEnv:
    max_steps: int = 200
    kind: int = capi.ENV_PENDULUM

    def observation_space(self):
        return Box((-1.0, -1.0, -8.0), (1.0, 1.0, 8.0))

    def action_space(self):
        return Box((-2.0,), (2.0,))


@dataclass
class MountainCarEnv:
    """MountainCar-v0 (Gymnasium equations; the reference takes its classic-control envs from ClassicControlEnvironments.jl)"""
    max_steps: int = 200
    action_start: int = 1
    kind: int = capi.ENV_MOUNTAINCAR

    def observation_space(self):
        return Box((-1.2, -0.07), (0.6, 0.07))

    def action_space(self):
        return Discrete(3, self.action_start)


@dataclass
class AcrobotEnv:
    """Acrobot-v1 (Gymnasium "book" dynamics; ClassicControlEnvironments.jl in the reference): six observation dims: the fused kernels at hidden [64,64] / [128,128] / [256,256] (four first-layer k-steps), generic kernels otherwise"""
    max_steps: int = 500
    action_start: int = 1
    kind: int = capi.ENV_ACROBOT

    def observation_space(self):
        return Box((-1.0, -1.0, -1.0, -1.0, -12.566371, -28.274334), (1.0, 1.0, 1.0, 1.0, 12.566371, 28.274334))

    def action_space(self):
        return Discrete(3, self.action_start)


@dataclass
class MountainCarContinuousEnv:
    """MountainCarContinuous-v0"""
    max_steps: int = 999
    kind: int = capi.ENV_MOUNTAINCAR_CONTINUOUS

    def observation_space(self):
        return Box((-1.2, -0.07), (0.6, 0.07))

    def action_space(self):
        return Box((-1.0,), (1.0,))


@dataclass
class ScalingWrapperEnv:
    """ScalingWrapperEnv(env) (src/environment_wrappers/scalingWrapperEnv.jl:15-49) around a Box/Box env: the agent-facing spaces become
    [-1, 1]; on device the two affine maps are fused into the env kernels (env kinds DRIL_ENV_PENDULUM_SCALED, DRIL_ENV_MOUNTAINCAR_CONTINUOUS_SCALED)."""
    env: object

    def __new__(cls, env=None):
        """ScalingWrapperEnv(DeviceModuleEnv(path, n)): the wrapper around every env of a device env plug-in is a mode of the plug-in's own kernels
        (dril_scaling_enable), so — like NormalizeWrapperEnv — this returns the parallel env with the wrapper switched on"""
        if isinstance(env, DeviceParallelEnv):
            if not isinstance(env, DeviceModuleEnv):
                raise NotImplementedError("ScalingWrapperEnv wraps single envs (ScalingWrapperEnv(PendulumEnv()), then DeviceParallelEnv) or a DeviceModuleEnv")
            return env._set_scaling(True)
        return super().__new__(cls)

    def __post_init__(self):
        if not isinstance(self.env, (PendulumEnv, MountainCarContinuousEnv)):
            raise NotImplementedError("ScalingWrapperEnv needs Box observation and action spaces (scalingWrapperEnv.jl:22); the device envs with both are Pendulum-v1 and MountainCarContinuous-v0")

    @property
    def max_steps(self) -> int:
        return self.env.max_steps

    @property
    def kind(self) -> int:
        return capi.ENV_PENDULUM_SCALED if isinstance(self.env, PendulumEnv) else capi.ENV_MOUNTAINCAR_CONTINUOUS_SCALED

    def unwrap(self):
        return self.env

    def observation_space(self):
        n = len(self.env.observation_space().low)
        return Box((-1.0,) * n, (1.0,) * n)

    def action_space(self):
        n = len(self.env.action_space().low)
        return Box((-1.0,) * n, (1.0,) * n)

    # scale! / unscale! (:71-79) on host arrays, for callers that want the original units back
    def scale_observation(self, obs):
        lo, hi = (np.asarray(v, np.float32) for v in (self.env.observation_space().low, self.env.observation_space().high))
        return (np.asarray(obs, np.float32) - lo) * (np.float32(2) / (hi - lo)) - np.float32(1)

    def unscale_observation(self, obs):
        lo, hi = (np.asarray(v, np.float32) for v in (self.env.observation_space().low, self.env.observation_space().high))
        return (np.asarray(obs, np.float32) + np.float32(1)) / (np.float32(2) / (hi - lo)) + lo

    def unscale_action(self, act):
        lo, hi = (np.asarray(v, np.float32) for v in (self.env.action_space().low, self.env.action_space().high))
        return (np.asarray(act, np.float32) + np.float32(1)) / (np.float32(2) / (hi - lo)) + lo


# --------------------------------------------------------------------------------------------
# PPO (src/algorithms/ppo.jl:25-40)
# --------------------------------------------------------------------------------------------
@dataclass
class PPO:
    gamma: float = 0.99
    gae_lambda: float = 0.95
    clip_range: float = 0.2
    clip_range_vf: Optional[float] = None
    ent_coef: float = 0.0
    vf_coef: float = 0.5
    max_grad_norm: Optional[float] = 0.5
    target_kl: Optional[float] = None
    normalize_advantage: bool = True
    n_steps: int = 2048
    batch_size: int = 64
    epochs: int = 10
    learning_rate: float = 3e-4


# --------------------------------------------------------------------------------------------
# layers (src/layers/): parameter tree + orthogonal init
# --------------------------------------------------------------------------------------------
def _orthogonal(rng: np.random.Generator, out_dims: int, in_dims: int, gain: float) -> np.ndarray:
    """WeightInitializers.orthogonal equivalent (QR of a normal matrix, sign-fixed); the exact Julia
    RNG stream is not reproducible outside Julia."""
    rows, cols = (out_dims, in_dims) if out_dims >= in_dims else (in_dims, out_dims)
    a = rng.standard_normal((rows, cols))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.diag(r))
    w = q if out_dims >= in_dims else q.T
    return (gain * w).astype(np.float32)


ACTIVATIONS = ("tanh", "relu", "sigmoid", "elu", "leakyrelu", "softplus", "gelu", "swish")   # dril_config.activation codes 0 .. 7 (include/dril_hip.h)


@dataclass
class ActorCriticLayer:
    """ActorCriticLayer(observation_space, action_space; hidden_dims=[64,64], activation=tanh, log_std_init=0)
    (src/layers/layer_constructors.jl:3-96).  Actor and critic are always separate MLPs
    (layer_helpers.jl:13-25)."""
    observation_space: Box
    action_space: object
    hidden_dims: Sequence[int] = (64, 64)      # any length 1..4 (get_mlp, layer_helpers.jl:27-57); two equal layers of 64 / 128 / 256 with tanh run the fused kernels
    log_std_init: float = 0.0
    activation: str = "tanh"                   # "tanh" (the reference's default, layer_constructors.jl:8,56), "relu", "sigmoid", "elu", "leakyrelu", "softplus", "gelu", "swish" (NNlib's definitions; anything but tanh runs the generic kernels)

    def __post_init__(self):
        self.hidden_dims = tuple(int(h) for h in self.hidden_dims)
        if not 1 <= len(self.hidden_dims) <= 4:
            raise ValueError("hidden_dims: 1..4 hidden layers are supported on the device path")
        if self.activation not in ACTIVATIONS:
            raise ValueError("activation: one of " + ", ".join(ACTIVATIONS))

    @property
    def discrete(self) -> bool:
        return isinstance(self.action_space, Discrete)

    @property
    def obs_dim(self) -> int:
        return len(self.observation_space.low)

    @property
    def actor_out(self) -> int:
        return self.action_space.n if self.discrete else len(self.action_space.low)

    def parameterlength(self) -> int:
        """Lux.parameterlength (test/test_policies.jl:55-57)."""
        a = self.actor_out

        def net(o):
            dims = (self.obs_dim, *self.hidden_dims, o)
            return sum(i * j + j for i, j in zip(dims[:-1], dims[1:]))
        return net(a) + net(1) + (0 if self.discrete else a)

    def initialparameters(self, rng: np.random.Generator) -> dict:
        """Lux.initialparameters: orthogonal gains sqrt(2) / 0.01 / 1.0, zero bias (layer_constructors.jl:16-20,61-65)."""
        def mlp(out, out_gain):
            dims = (self.obs_dim, *self.hidden_dims, out)
            n = len(dims) - 1
            return {f"layer_{l + 1}": {"weight": _orthogonal(rng, dims[l + 1], dims[l], out_gain if l == n - 1 else math.sqrt(2.0)),
                                       "bias": np.zeros(dims[l + 1], np.float32)} for l in range(n)}

        ps = {"feature_extractor": {}, "actor_head": mlp(self.actor_out, 0.01), "critic_head": mlp(1, 1.0)}
        if not self.discrete:
            ps["log_std"] = np.full(self.actor_out, self.log_std_init, np.float32)
        return ps


DiscreteActorCriticLayer = ActorCriticLayer
ContinuousActorCriticLayer = ActorCriticLayer


def _layer_keys(head: dict) -> list:
    """layer_1 .. layer_n in order (Lux.Chain names its layers layer_k, layer_lux.jl:31-39)"""
    return sorted((k for k in head if k.startswith("layer_")), key=lambda k: int(k.split("_")[1]))


def flatten_params(ps: dict) -> np.ndarray:
    """Lux NamedTuple -> the flat layout of dril_set_params (weights column-major out x in)."""
    parts = []
    for head in ("actor_head", "critic_head"):
        for l in _layer_keys(ps[head]):
            parts.append(np.asarray(ps[head][l]["weight"], np.float32).ravel(order="F"))
            parts.append(np.asarray(ps[head][l]["bias"], np.float32).ravel())
    if "log_std" in ps:
        parts.append(np.asarray(ps["log_std"], np.float32).ravel())
    return np.concatenate(parts)


def unflatten_params(flat: np.ndarray, like: dict) -> dict:
    out = {"feature_extractor": {}, "actor_head": {}, "critic_head": {}}
    off = 0
    for head in ("actor_head", "critic_head"):
        for l in _layer_keys(like[head]):
            w = like[head][l]["weight"]
            n = w.size
            out[head][l] = {"weight": flat[off:off + n].reshape(w.shape, order="F").copy()}
            off += n
            b = like[head][l]["bias"]
            out[head][l]["bias"] = flat[off:off + b.size].copy()
            off += b.size
    if "log_std" in like:
        out["log_std"] = flat[off:off + like["log_std"].size].copy()
    return out


@dataclass
class TrainState:
    """Lux.Training.TrainState (ppo.jl:52-53): parameters + optimizer_state.  optimizer_state is the Adam leaf state of Optimisers.jl flattened in the parameter
    layout — {"m", "v": float32 (P), "beta_powers": (beta1^t, beta2^t), "steps": t} — or None for a fresh optimiser (what `Agent(...)` and
    load_policy_params_and_state! build, ppo.jl:77-94).  train_ moves it into the device handle on entry and back on every exit, so the moments follow the
    TrainState from env to env and through a re-created handle, as they follow the Julia object."""
    parameters: dict
    step: int = 0
    optimizer_state: Optional[dict] = None


@dataclass
class Agent:
    """Agent(layer, alg; rng) — src/algorithms/ppo.jl:42-62 (optimiser Adam(eta=lr, eps=1e-5), :64-66)."""
    layer: ActorCriticLayer
    alg: PPO
    seed: int = 0
    verbose: int = 0
    train_state: TrainState = field(init=False)
    rng: np.random.Generator = field(init=False)
    steps_taken: int = 0
    gradient_updates: int = 0

    def __post_init__(self):
        self.rng = np.random.default_rng(self.seed)
        self.train_state = TrainState(self.layer.initialparameters(self.rng))


# --------------------------------------------------------------------------------------------
# the device handle
# --------------------------------------------------------------------------------------------
def make_config(env, n_envs: int, alg: PPO, layer: Optional[ActorCriticLayer] = None, *, seed: int = 42,
                fixed_length_episodes: bool = False, device: int = 0, rank: int = 0, world_size: int = 1,
                profile_events: bool = False, normalize: Optional[dict] = None, monitor_window: int = 0) -> DrilConfig:
    c = capi.default_config(env.kind)
    c.n_envs, c.n_steps = n_envs, alg.n_steps
    if layer is not None:
        hd = tuple(layer.hidden_dims)
        c.hidden1, c.hidden2 = hd[0], hd[1] if len(hd) > 1 else hd[0]
        if len(hd) != 2 or getattr(layer, "activation", "tanh") != "tanh":            # dril_config v2: any depth / relu (n_hidden == 0 is the two-layer tanh form)
            c.n_hidden = len(hd)
            for i, w in enumerate(hd):
                c.hidden[i] = w
            c.activation = ACTIVATIONS.index(layer.activation)
        c.log_std_init = layer.log_std_init
    c.episode_len = getattr(env, "max_steps", 0)
    c.fixed_length_episodes = int(fixed_length_episodes)
    c.action_start = getattr(env, "action_start", 1)
    if env.kind == capi.ENV_EXTERNAL:   # host envs: the spaces travel in the config (include/dril_hip.h, DRIL_ENV_EXTERNAL)
        osp, asp = env.observation_space(), env.action_space()
        c.ext_obs_dim = int(np.prod(osp.shape))
        c.ext_discrete = int(isinstance(asp, Discrete))
        if c.ext_discrete:
            c.ext_action_dim, c.action_start = asp.n, asp.start
        else:
            c.ext_action_dim = int(np.prod(asp.shape))
            lo, hi = np.unique(np.asarray(asp.low, np.float32)), np.unique(np.asarray(asp.high, np.float32))
            # ClampAdapter on the device needs one (low, high) pair; per-dimension bounds are clamped by HostParallelEnv.act_ instead
            c.ext_action_low, c.ext_action_high = (float(lo[0]), float(hi[0])) if lo.size == 1 and hi.size == 1 else (0.0, 0.0)
    c.gamma, c.gae_lambda, c.clip_range = alg.gamma, alg.gae_lambda, alg.clip_range
    c.has_clip_range_vf = int(alg.clip_range_vf is not None)
    c.clip_range_vf = alg.clip_range_vf or 0.0
    c.ent_coef, c.vf_coef = alg.ent_coef, alg.vf_coef
    c.has_max_grad_norm = int(alg.max_grad_norm is not None)
    c.max_grad_norm = alg.max_grad_norm or 0.0
    c.has_target_kl = int(alg.target_kl is not None)
    c.target_kl = alg.target_kl or 0.0
    c.normalize_advantage = int(alg.normalize_advantage)
    c.batch_size, c.epochs, c.learning_rate = alg.batch_size, alg.epochs, alg.learning_rate
    c.seed, c.device, c.rank, c.world_size = seed, device, rank, world_size
    c.profile_events = int(profile_events)      # True / 1: every launch bracketed; k > 1: the per-optimiser-step kernels at every k-th launch
    c.monitor_window = int(monitor_window)
    if normalize is not None:   # NormalizeWrapperEnv kwargs, normalizeWrapperEnv.jl:71-80
        c.norm_training = int(normalize.get("training", True))
        c.norm_obs = int(normalize.get("norm_obs", True))
        c.norm_reward = int(normalize.get("norm_reward", True))
        c.clip_obs = normalize.get("clip_obs", 10.0)
        c.clip_reward = normalize.get("clip_reward", 10.0)
        c.norm_gamma = normalize.get("gamma", 0.99)
        c.norm_epsilon = normalize.get("epsilon", 1e-8)
    return c


def _module_info_dict(info) -> dict:
    A = info.action_dim
    return dict(plugin_abi=info.plugin_abi, state_dim=info.state_dim, obs_dim=info.obs_dim, action_dim=A, discrete=bool(info.discrete), episode_len=info.episode_len,
                action_low=np.asarray(info.action_low[:A], np.float32), action_high=np.asarray(info.action_high[:A], np.float32), name=info.name.decode())


def describe_env_module(code_object_path, device: int = 0) -> dict:
    """dril_env_module_describe + dril_env_module_obs_space + dril_env_module_agents: what a device env plug-in's code object says about itself (spaces, bounds, time
    limit, name; `obs_low` / `obs_high` and `obs_declared`: the observation space the env declares, -inf / +inf and False when it declares none; `agents`: agents per
    world, 1 for a classic plug-in)."""
    lib = capi.load_library()
    info = capi.DrilEnvModuleInfo()
    rc = lib.dril_env_module_describe(os.fsencode(code_object_path), device, C.byref(info))
    if rc != capi.OK:
        raise DrilError(rc, (lib.dril_last_error(None) or b"").decode())
    d = _module_info_dict(info)
    lo, hi, decl = np.empty(info.obs_dim, np.float32), np.empty(info.obs_dim, np.float32), C.c_int32()
    rc = lib.dril_env_module_obs_space(os.fsencode(code_object_path), device, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), C.byref(decl))
    if rc != capi.OK:
        raise DrilError(rc, (lib.dril_last_error(None) or b"").decode())
    d.update(obs_low=lo, obs_high=hi, obs_declared=bool(decl.value))
    agents = C.c_int32()
    rc = lib.dril_env_module_agents(os.fsencode(code_object_path), device, C.byref(agents))
    if rc != capi.OK:
        raise DrilError(rc, (lib.dril_last_error(None) or b"").decode())
    d.update(agents=agents.value)               # N for a world (include/device/dril_env_world.h: N agents share a state, one row each), 1 for a classic plug-in
    return d


def _agent_spaces(fn, h, D: int, A: int) -> dict:
    """dril_agent_spaces / dril_sac_agent_spaces as a dict"""
    ol, oh, al, ah, on = (np.empty(D, np.float32), np.empty(D, np.float32), np.full(A, np.nan, np.float32), np.full(A, np.nan, np.float32), C.c_int32())
    rc = fn(h, *(a.ctypes.data_as(C.c_void_p) for a in (ol, oh, al, ah)), C.byref(on))
    return rc, dict(obs_low=ol, obs_high=oh, action_low=al, action_high=ah, scaling=bool(on.value))


_DEV_DTYPES = {"float32": (np.dtype(np.float32),), "int32": (np.dtype(np.int32),), "uint8": (np.dtype(np.uint8), np.dtype(np.bool_))}


def _dev_ptr(name: str, a, shape: tuple, dtype: str, optional: bool = False):
    """the device pointer behind `a`: an integer (a raw device pointer, taken as it is) or any object with `__cuda_array_interface__` (torch-ROCm tensors,
    CuPy arrays), whose shape, dtype and C-contiguity are checked here — a ValueError names the argument before the library is called"""
    if a is None:
        if optional:
            return None
        raise ValueError(f"{name}: None, expected a device array of shape {shape} ({dtype})")
    if isinstance(a, (int, np.integer)) and not isinstance(a, bool):
        return C.c_void_p(int(a))
    try:
        cai = getattr(a, "__cuda_array_interface__", None)
    except Exception:
        cai = None
    if cai is None:
        raise ValueError(f"{name}: expected a device array (an object with __cuda_array_interface__) or an integer device pointer, got {type(a).__name__}; host arrays go to the verbs without `_device`")
    got_shape, dt = tuple(int(x) for x in cai["shape"]), np.dtype(cai["typestr"])
    if dt not in _DEV_DTYPES[dtype]:
        raise ValueError(f"{name}: dtype {dt} where {dtype}{' / bool' if dtype == 'uint8' else ''} is expected")
    if got_shape != tuple(shape):
        hint = f": the layout is (n_envs, dim) = {tuple(shape)}, one row per env" if len(shape) == 2 and got_shape == tuple(shape)[::-1] and got_shape != tuple(shape) else ""
        raise ValueError(f"{name}: shape {got_shape} where {tuple(shape)} is expected{hint}")
    strides = cai.get("strides")
    if strides is not None:
        want, acc = [], dt.itemsize
        for n in reversed(got_shape):
            want.append(acc); acc *= n
        if any(n > 1 and int(st) != w for n, st, w in zip(got_shape, strides, reversed(want))):
            raise ValueError(f"{name}: not C-contiguous (strides {tuple(strides)}); pass a contiguous copy")
    ptr = int(cai["data"][0])
    if ptr == 0 and int(np.prod(got_shape)) > 0:
        raise ValueError(f"{name}: null device pointer")
    return C.c_void_p(ptr)


def _stream_ptr(stream):
    """a hipStream_t as an int, a callable returning one (`lambda: torch.cuda.current_stream().cuda_stream`), or None = the null stream"""
    if callable(stream):
        stream = stream()
    return C.c_void_p(int(stream)) if stream else None


def _opt_in_persistent(impl):
    """The positional signatures of evaluate_agent_device / collect_trajectory_device / collect_trajectory are a fixed interface (callers and tests rely on them
    as inspect.signature reports them).  The opt-in `persistent` is therefore a keyword-only option added in front of the verb: the decorated function states the
    fixed interface (and is what inspect.signature reports), `impl` — the same parameters plus `persistent` — does the work."""
    def decorate(public):
        @functools.wraps(public)
        def verb(*args, persistent: bool = False, **kwargs):
            return impl(*args, persistent=persistent, **kwargs)
        verb.__doc__ = (impl.__doc__ or "") + "\n\n" + (public.__doc__ or "")
        return verb
    return decorate


@_normalize.normalize_verbs(lambda self, verb: getattr(self.lib, ("dril_normalize_" if verb == "config_default" else "dril_ext_normalize_") + verb), "normalize_", "ext_")
@_normalize.normalize_verbs(lambda self, verb: getattr(self.lib, "dril_normalize_" + verb), "normalize_")
class Handle:
    """Owns one dril_handle*; every method is a thin typed wrapper of one C entry point."""

    def __init__(self, cfg: DrilConfig, lib: Optional[C.CDLL] = None, env_module: Optional[os.PathLike] = None):
        self.lib = lib or capi.load_library()
        self.cfg = cfg
        self._h = C.c_void_p()
        if env_module is not None:      # cfg.env_kind == ENV_MODULE: the env is a code object built from include/device/dril_env_plugin.h
            rc = self.lib.dril_create_with_env_module(C.byref(cfg), os.fsencode(env_module), C.byref(self._h))
        else:
            rc = self.lib.dril_create(C.byref(cfg), C.byref(self._h))
        if rc != capi.OK:
            raise DrilError(rc, (self.lib.dril_last_error(None) or b"").decode())
        self.D = self.lib.dril_obs_dim(self._h)
        self.A = self.lib.dril_action_dim(self._h)
        self.discrete = bool(self.lib.dril_is_discrete(self._h))
        self.P = int(self.lib.dril_param_count(self._h))
        self.E, self.T = cfg.n_envs, cfg.n_steps
        self.N = self.E * self.T

    def close(self):
        if self._h:
            self._chk(self.lib.dril_destroy(self._h))      # refused while the handle is a member of a Population: close the population first
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != capi.OK:
            raise DrilError(rc, (self.lib.dril_last_error(self._h) or b"").decode())

    @staticmethod
    def _p(a: Optional[np.ndarray]):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    # parameters
    def set_params(self, flat: np.ndarray):
        flat = np.ascontiguousarray(flat, np.float32)
        self._chk(self.lib.dril_set_params(self._h, self._p(flat), flat.size))

    def get_params(self) -> np.ndarray:
        out = np.empty(self.P, np.float32)
        self._chk(self.lib.dril_get_params(self._h, self._p(out), out.size))
        return out

    def reset_optimizer(self):
        self._chk(self.lib.dril_reset_optimizer(self._h))

    def get_optimizer_state(self) -> dict:
        m, v, bp, steps = np.empty(self.P, np.float32), np.empty(self.P, np.float32), np.empty(2, np.float32), C.c_int64()
        self._chk(self.lib.dril_get_optimizer_state(self._h, self._p(m), self._p(v), m.size, self._p(bp), C.byref(steps)))
        return {"m": m, "v": v, "beta_powers": (float(bp[0]), float(bp[1])), "steps": int(steps.value)}

    def set_optimizer_state(self, st: Optional[dict]):
        if st is None:
            return self.reset_optimizer()
        m, v = np.ascontiguousarray(st["m"], np.float32), np.ascontiguousarray(st["v"], np.float32)
        if m.size != self.P or v.size != self.P:
            raise ValueError(f"optimizer_state holds {m.size} parameters, the layer has {self.P}: it belongs to another layer")
        bp = np.asarray(st["beta_powers"], np.float32)
        self._chk(self.lib.dril_set_optimizer_state(self._h, self._p(m), self._p(v), m.size, self._p(bp), int(st["steps"])))

    def set_learning_rate(self, lr: float):
        self._chk(self.lib.dril_set_learning_rate(self._h, lr))

    # env verbs
    def env_module_info(self) -> dict:
        info = capi.DrilEnvModuleInfo()
        self._chk(self.lib.dril_env_module_info_of(self._h, C.byref(info)))
        return _module_info_dict(info)

    def env_module_obs_space(self) -> dict:
        """dril_env_module_obs_space_of: the observation space the plug-in declares (the env's own, whether ScalingWrapperEnv is on or not)"""
        lo, hi, decl = np.empty(self.D, np.float32), np.empty(self.D, np.float32), C.c_int32()
        self._chk(self.lib.dril_env_module_obs_space_of(self._h, self._p(lo), self._p(hi), C.byref(decl)))
        return dict(low=lo, high=hi, declared=bool(decl.value))

    def env_module_agents(self) -> int:
        """dril_env_module_agents_of: agents per world of a plug-in handle (rows w N .. w N + N - 1 are world w); 1 for a classic plug-in"""
        n = C.c_int32()
        self._chk(self.lib.dril_env_module_agents_of(self._h, C.byref(n)))
        return n.value

    def rollout_fused_enable(self, on: bool = True):
        """dril_rollout_fused_enable: collections of a plug-in handle in ONE launch of the plug-in's own rollout kernel (a code object built with
        DRIL_ENV_PLUGIN_ROLLOUT, include/device/dril_env_rollout.h); legal at any time between collections"""
        self._chk(self.lib.dril_rollout_fused_enable(self._h, int(bool(on))))

    def rollout_fused_info(self) -> dict:
        """dril_rollout_fused_info: available / enabled / tile / threads / max_width / last_collection_launches / reason"""
        info = capi.DrilFusedRolloutInfo()
        self._chk(self.lib.dril_rollout_fused_info(self._h, C.byref(info)))
        return dict(available=bool(info.available), enabled=bool(info.enabled), tile=info.tile, threads=info.threads, max_width=info.max_width,
                    last_collection_launches=info.last_collection_launches, reason=info.reason.decode())

    def norm_rollout_enable(self, on: bool = True):
        """dril_norm_rollout_enable: collections of a normalising built-in handle (n_envs <= 128, hidden_dims [64,64]) as the opening observe and ONE launch of
        rollout_norm_kernel instead of three launches per env step (docs/normalized_rollout.md); legal at any time between collections"""
        self._chk(self.lib.dril_norm_rollout_enable(self._h, int(bool(on))))

    def norm_rollout_info(self) -> dict:
        """dril_norm_rollout_info: available / enabled / max_envs / last_collection_launches / last_collection_path (1 = the kernel, 0 = step-granular) /
        total_stepwise_fallbacks / reason"""
        info = capi.DrilNormRolloutInfo()
        self._chk(self.lib.dril_norm_rollout_info(self._h, C.byref(info)))
        return dict(available=bool(info.available), enabled=bool(info.enabled), max_envs=info.max_envs, last_collection_launches=info.last_collection_launches,
                    last_collection_path=info.last_collection_path, total_stepwise_fallbacks=info.total_stepwise_fallbacks, reason=info.reason.decode())

    def update_fused_enable(self, on: bool = True):
        """dril_update_fused_enable: every optimiser step of dril_ppo_update on a generic handle (a plug-in, external envs, a built-in with other hidden_dims or
        activation) at batch_size <= 64 inside ONE launch of ppo_update_generic_small_kernel instead of 3 nh + 6 launches per step (docs/generic_update.md); legal at
        any time between updates.  A handle that cannot take it raises the library's message and stays as it was"""
        self._chk(self.lib.dril_update_fused_enable(self._h, int(bool(on))))

    def update_fused_info(self) -> dict:
        """dril_update_fused_info: available / enabled / the kernel's caps / last_update_path (1 = the kernel, 0 = per step) / last_update_launches /
        steps_per_launch / reason; faster_up_to_batch = the largest batch_size at which the route measured faster than the per-step
        route (it is accepted up to max_batch)"""
        info = capi.DrilUpdateFusedInfo()
        self._chk(self.lib.dril_update_fused_info(self._h, C.byref(info)))
        return dict(available=bool(info.available), enabled=bool(info.enabled), max_width=info.max_width, max_obs_dim=info.max_obs_dim,
                    max_action_dim=info.max_action_dim, max_params=info.max_params, max_hidden_layers=info.max_hidden_layers, min_batch=info.min_batch,
                    max_batch=info.max_batch, faster_up_to_batch=info.faster_up_to_batch, last_update_path=info.last_update_path, last_update_launches=info.last_update_launches,
                    steps_per_launch=info.steps_per_launch, reason=info.reason.decode())

    def evaluate_fused_info(self) -> dict:
        """dril_evaluate_fused_info: available / tile / threads / max_width / reason — whether persistent=True of the evaluation and trajectory verbs would run the
        plug-in's own evaluation kernel (path 2; a code object built with DRIL_ENV_PLUGIN_EVALUATE, include/device/dril_env_evaluate.h) on this handle"""
        info = capi.DrilFusedEvaluateInfo()
        self._chk(self.lib.dril_evaluate_fused_info(self._h, C.byref(info)))
        return dict(available=bool(info.available), tile=info.tile, threads=info.threads, max_width=info.max_width, reason=info.reason.decode())

    def scaling_enable(self, on: bool = True):
        """dril_scaling_enable: ScalingWrapperEnv around every env of a plug-in handle; between create and the first env_reset"""
        self._chk(self.lib.dril_scaling_enable(self._h, int(bool(on))))

    def agent_spaces(self) -> dict:
        """dril_agent_spaces: the spaces the agent sees (Box(-1, 1) throughout under ScalingWrapperEnv)"""
        rc, d = _agent_spaces(self.lib.dril_agent_spaces, self._h, self.D, self.A)
        self._chk(rc)
        return d

    def env_reset(self, seed: int):
        self._chk(self.lib.dril_env_reset(self._h, seed))

    def env_observe(self, update_stats: bool = True) -> np.ndarray:
        obs = np.empty((self.E, self.D), np.float32)  # row e = observation of env e ((D x E) column-major)
        self._chk(self.lib.dril_env_observe(self._h, self._p(obs), int(update_stats)))
        return obs

    def env_step(self, actions: np.ndarray):
        actions = np.ascontiguousarray(actions, np.int32 if self.discrete else np.float32)
        rew = np.empty(self.E, np.float32)
        term = np.empty(self.E, np.uint8)
        trunc = np.empty(self.E, np.uint8)
        tobs = np.zeros((self.E, self.D), np.float32)
        self._chk(self.lib.dril_env_step(self._h, self._p(actions), self._p(rew), self._p(term), self._p(trunc), self._p(tobs)))
        return rew, term.astype(bool), trunc.astype(bool), tobs

    def env_get_state(self):
        S = self.env_module_info()["state_dim"] if self.cfg.env_kind == capi.ENV_MODULE else 4 if self.cfg.env_kind in (capi.ENV_CARTPOLE, capi.ENV_ACROBOT) else 2      # CartPole / Acrobot (theta1, theta2, dtheta1, dtheta2); (x, x_dot, theta, theta_dot); Pendulum (theta, theta_dot); MountainCar (position, velocity)
        W = self.E // self.env_module_agents() if self.cfg.env_kind == capi.ENV_MODULE else self.E     # a world handle: one state per world, (W, S); counters per row
        st = np.empty((W, S), np.float32)
        sc = np.empty(self.E, np.int32)
        self._chk(self.lib.dril_env_get_state(self._h, self._p(st), self._p(sc)))
        return st, sc

    def env_set_state(self, st: np.ndarray, sc: Optional[np.ndarray] = None):
        st = np.ascontiguousarray(st, np.float32)
        sc = None if sc is None else np.ascontiguousarray(sc, np.int32)
        if self.cfg.env_kind == capi.ENV_MODULE:                       # (W, S) for a world handle, (E, S) otherwise; step counts per row
            W = self.E // self.env_module_agents()
            if st.size != W * self.env_module_info()["state_dim"] or (sc is not None and sc.size != self.E):
                raise ValueError(f"env_set_state: state of {st.size} floats / {0 if sc is None else sc.size} step counts for {W} states and {self.E} rows")
        self._chk(self.lib.dril_env_set_state(self._h, self._p(st), self._p(sc)))

    def monitor_stats(self):
        """(ep_rew_mean, ep_len_mean, n_episodes) of MonitorWrapperEnv's window (log_stats, monitorWrapperEnv.jl:64-70)."""
        r, l, n = C.c_float(), C.c_float(), C.c_int32()
        self._chk(self.lib.dril_monitor_get_stats(self._h, C.byref(r), C.byref(l), C.byref(n)))
        return r.value, l.value, n.value

    def norm_get_stats(self) -> dict:
        """RunningMeanStd fields of the wrapper (normalizeWrapperEnv.jl:8-19)."""
        om = np.empty(self.D, np.float32); ov = np.empty(self.D, np.float32)
        oc, rc = C.c_int64(), C.c_int64(); rm, rv = C.c_float(), C.c_float()
        self._chk(self.lib.dril_norm_get_stats(self._h, self._p(om), self._p(ov), C.byref(oc), C.byref(rm), C.byref(rv), C.byref(rc)))
        return dict(obs_mean=om, obs_var=ov, obs_count=oc.value, ret_mean=rm.value, ret_var=rv.value, ret_count=rc.value)

    def norm_get_original(self):
        """-> (get_original_obs, get_original_rewards), normalizeWrapperEnv.jl:220-222"""
        obs = np.empty((self.E, self.D), np.float32); rew = np.empty(self.E, np.float32)
        self._chk(self.lib.dril_norm_get_original(self._h, self._p(obs), self._p(rew)))
        return obs, rew

    def norm_set_stats(self, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count):
        om = np.ascontiguousarray(obs_mean, np.float32); ov = np.ascontiguousarray(obs_var, np.float32)
        self._chk(self.lib.dril_norm_set_stats(self._h, self._p(om), self._p(ov), int(obs_count), float(ret_mean), float(ret_var), int(ret_count)))

    # NormalizeWrapperEnv around a device env plug-in (dril_normalize_*; built-in envs are wrapped at create through cfg.norm_*): normalize_enable, normalize_config,
    # normalize_set_training, normalize_get_stats / set_stats / get_original / get_returns come from _normalize.normalize_verbs
    _NORMALIZE_KEYS = _normalize.KEYS

    # policy on host batches
    def policy_forward(self, obs: np.ndarray, noise: Optional[np.ndarray] = None):
        obs = np.ascontiguousarray(obs, np.float32)
        B = obs.shape[0]
        act = np.empty(B, np.int32) if self.discrete else np.empty((B, self.A), np.float32)
        val = np.empty(B, np.float32)
        lp = np.empty(B, np.float32)
        if noise is not None:
            noise = np.ascontiguousarray(noise, np.float64 if self.discrete else np.float32)
        self._chk(self.lib.dril_policy_forward(self._h, self._p(obs), B, self._p(noise), self._p(act), self._p(val), self._p(lp)))
        return act, val, lp

    def evaluate_actions(self, obs: np.ndarray, actions: np.ndarray):
        obs = np.ascontiguousarray(obs, np.float32)
        actions = np.ascontiguousarray(actions, np.int32 if self.discrete else np.float32)
        B = obs.shape[0]
        val, lp, ent = (np.empty(B, np.float32) for _ in range(3))
        self._chk(self.lib.dril_evaluate_actions(self._h, self._p(obs), self._p(actions), B, self._p(val), self._p(lp), self._p(ent)))
        return val, lp, ent

    def predict_actions(self, obs: np.ndarray, deterministic: bool = False, noise: Optional[np.ndarray] = None) -> np.ndarray:
        obs = np.ascontiguousarray(obs, np.float32)
        B = obs.shape[0]
        act = np.empty(B, np.int32) if self.discrete else np.empty((B, self.A), np.float32)
        if noise is not None:
            noise = np.ascontiguousarray(noise, np.float64 if self.discrete else np.float32)
        self._chk(self.lib.dril_predict_actions(self._h, self._p(obs), B, int(deterministic), self._p(noise), self._p(act)))
        return act

    def predict_values(self, obs: np.ndarray) -> np.ndarray:
        obs = np.ascontiguousarray(obs, np.float32)
        val = np.empty(obs.shape[0], np.float32)
        self._chk(self.lib.dril_predict_values(self._h, self._p(obs), obs.shape[0], self._p(val)))
        return val

    # rollout
    def collect_rollout(self) -> float:
        fps = C.c_double()
        self._chk(self.lib.dril_collect_rollout(self._h, C.byref(fps)))
        return fps.value

    # rollout over host envs (DRIL_ENV_EXTERNAL), trajectory.jl:22-78
    def ext_act(self, obs: np.ndarray):
        """-> (raw policy actions, env-space actions) for one env step; obs is (E, D)"""
        obs = np.ascontiguousarray(obs, np.float32).reshape(self.E, self.D)
        raw = np.empty(self.E, np.int32) if self.discrete else np.empty((self.E, self.A), np.float32)
        env_a = np.empty_like(raw)
        self._chk(self.lib.dril_ext_act(self._h, self._p(obs), self._p(raw), self._p(env_a)))
        return raw, env_a

    def ext_record(self, rewards, terminated, truncated, terminal_obs=None):
        r = np.ascontiguousarray(rewards, np.float32); te = np.ascontiguousarray(terminated, np.uint8); tr = np.ascontiguousarray(truncated, np.uint8)
        to = None if terminal_obs is None else np.ascontiguousarray(terminal_obs, np.float32).reshape(self.E, self.D)
        self._chk(self.lib.dril_ext_record(self._h, self._p(r), self._p(te), self._p(tr), self._p(to)))

    def ext_finish(self, last_obs: np.ndarray):
        o = np.ascontiguousarray(last_obs, np.float32).reshape(self.E, self.D)
        self._chk(self.lib.dril_ext_finish(self._h, self._p(o)))

    def ext_steps(self) -> int:
        return int(self.lib.dril_ext_steps(self._h))

    # the same rollout over DEVICE arrays (dril_ext_*_device): integers (raw device pointers) or objects with __cuda_array_interface__; nothing is copied or allocated here
    def _act_shape(self, n: int) -> tuple:
        return (n,) if self.discrete else (n, self.A)

    def ext_act_device(self, obs, raw_actions=None, env_actions=None, stream=None):
        """obs (E, D) f32 on the device; raw_actions / env_actions: device OUTPUT arrays i32 (E,) | f32 (E, A), either may be None.  Enqueues and returns:
        the outputs are ready for work enqueued on `stream` afterwards"""
        at = "int32" if self.discrete else "float32"
        args = (_dev_ptr("obs", obs, (self.E, self.D), "float32"), _dev_ptr("raw_actions", raw_actions, self._act_shape(self.E), at, True),
                _dev_ptr("env_actions", env_actions, self._act_shape(self.E), at, True))
        self._chk(self.lib.dril_ext_act_device(self._h, *args, _stream_ptr(stream)))

    def ext_record_device(self, rewards, terminated, truncated, terminal_obs=None, stream=None):
        """rewards f32 (E,), terminated / truncated u8 or bool (E,), terminal_obs f32 (E, D) or None = no env was truncated in this step"""
        args = (_dev_ptr("rewards", rewards, (self.E,), "float32"), _dev_ptr("terminated", terminated, (self.E,), "uint8"), _dev_ptr("truncated", truncated, (self.E,), "uint8"),
                _dev_ptr("terminal_obs", terminal_obs, (self.E, self.D), "float32", True))
        self._chk(self.lib.dril_ext_record_device(self._h, *args, _stream_ptr(stream)))

    def ext_finish_device(self, last_obs, stream=None):
        o = _dev_ptr("last_obs", last_obs, (self.E, self.D), "float32")
        self._chk(self.lib.dril_ext_finish_device(self._h, o, _stream_ptr(stream)))

    def predict_actions_device(self, obs, deterministic: bool = False, raw_actions=None, env_actions=None, stream=None, batch: Optional[int] = None):
        """dril_predict_actions on device arrays, the adapter applied in env_actions; `batch` is read from obs's shape (B, D) unless obs is a raw pointer"""
        if batch is None:
            cai = getattr(obs, "__cuda_array_interface__", None)
            if cai is None or len(cai["shape"]) != 2:
                raise ValueError("obs: expected a device array of shape (batch, obs_dim), or a raw pointer together with batch=")
            batch = int(cai["shape"][0])
        if raw_actions is None and env_actions is None:
            raise ValueError("raw_actions / env_actions: at least one device output array is needed")
        at = "int32" if self.discrete else "float32"
        args = (_dev_ptr("obs", obs, (batch, self.D), "float32"), batch, int(deterministic), _dev_ptr("raw_actions", raw_actions, self._act_shape(batch), at, True),
                _dev_ptr("env_actions", env_actions, self._act_shape(batch), at, True))
        self._chk(self.lib.dril_predict_actions_device(self._h, *args, _stream_ptr(stream)))

    def ext_set_action_bounds(self, low, high):
        """the ClampAdapter's Box per action dimension (host arrays of A floats; both None: back to the config's scalar pair)"""
        if low is None and high is None:
            self._chk(self.lib.dril_ext_set_action_bounds(self._h, None, None)); return
        lo, hi = np.ascontiguousarray(low, np.float32).ravel(), np.ascontiguousarray(high, np.float32).ravel()
        if lo.size != self.A or hi.size != self.A:
            raise ValueError(f"low / high: {lo.size} / {hi.size} values where action_dim = {self.A} are expected")
        self._chk(self.lib.dril_ext_set_action_bounds(self._h, self._p(lo), self._p(hi)))

    # NormalizeWrapperEnv / MonitorWrapperEnv around device-resident external envs (dril_ext_normalize_* / dril_ext_monitor_*, docs/external_envs.md section 10, "Wrappers on device-resident arrays"):
    # ext_normalize_enable, ext_normalize_config, ext_normalize_set_training, ext_normalize_get_stats / _set_stats / _get_original / _get_returns come from
    # _normalize.normalize_verbs
    def ext_normalize_reset(self, stream=None):
        """the wrapper's half of reset! (normalizeWrapperEnv.jl:111-121): returns <- 0, statistics kept; enqueued, no host wait"""
        self._chk(self.lib.dril_ext_normalize_reset(self._h, _stream_ptr(stream)))

    def ext_monitor_enable(self, stats_window: int):
        """MonitorWrapperEnv(env, stats_window) around the external envs; 0 switches it off"""
        self._chk(self.lib.dril_ext_monitor_enable(self._h, int(stats_window)))

    def ext_monitor_stats(self):
        """(ep_rew_mean, ep_len_mean, n_episodes) of the window: raw rewards, episodes in (step, env) order"""
        r, l, n = C.c_float(), C.c_float(), C.c_int32()
        self._chk(self.lib.dril_ext_monitor_get_stats(self._h, C.byref(r), C.byref(l), C.byref(n)))
        return r.value, l.value, n.value

    def ext_wrap_info(self) -> dict:
        """which wrappers are on, the launches they added to the act / record / finish calls of the current (or last) rollout, allocations since enable"""
        info = capi.DrilExtWrapInfo()
        self._chk(self.lib.dril_ext_wrap_info(self._h, C.byref(info)))
        return {k: int(getattr(info, k)) for k in ("normalize_on", "monitor_on", "monitor_window", "launches_act", "launches_record", "launches_finish", "allocations")}

    def ext_device_info(self) -> dict:
        info = capi.DrilExtDeviceInfo()
        self._chk(self.lib.dril_ext_device_info(self._h, C.byref(info)))
        return dict(steps_device=info.steps_device, steps_host=info.steps_host, host_syncs=info.host_syncs, per_dim_bounds=bool(info.per_dim_bounds), launches=int(info.launches))

    def set_noise(self, noise: Optional[np.ndarray]):
        if noise is None:
            self._chk(self.lib.dril_debug_set_noise(self._h, None, 0))
            return
        noise = np.ascontiguousarray(noise, np.float64 if self.discrete else np.float32)
        self._chk(self.lib.dril_debug_set_noise(self._h, self._p(noise), noise.size))

    _BUF = {
        capi.BUF_OBSERVATIONS: ("f4", "ND"), capi.BUF_ACTIONS: (None, "NA"), capi.BUF_REWARDS: ("f4", "N"),
        capi.BUF_ADVANTAGES: ("f4", "N"), capi.BUF_RETURNS: ("f4", "N"), capi.BUF_LOGPROBS: ("f4", "N"),
        capi.BUF_VALUES: ("f4", "N"), capi.BUF_FLAGS: ("u1", "N"), capi.BUF_BOOTSTRAP: ("f4", "N"),
        capi.BUF_LAST_VALUES: ("f4", "E"),
    }

    def _buf_like(self, which: int) -> np.ndarray:
        dt, shp = self._BUF[which]
        if which == capi.BUF_ACTIONS:
            return np.empty(self.N, np.int32) if self.discrete else np.empty((self.N, self.A), np.float32)
        shape = {"ND": (self.N, self.D), "N": (self.N,), "E": (self.E,)}[shp]
        return np.empty(shape, np.dtype(dt))

    def buffer(self, which: int) -> np.ndarray:
        """time-major copy of one RolloutBuffer field (index n = t*E + e)."""
        out = self._buf_like(which)
        self._chk(self.lib.dril_buffer_copy_out(self._h, which, self._p(out), out.nbytes))
        return out

    def set_buffer(self, which: int, arr: np.ndarray):
        like = self._buf_like(which)
        arr = np.ascontiguousarray(arr, like.dtype).reshape(like.shape)
        self._chk(self.lib.dril_buffer_copy_in(self._h, which, self._p(arr), arr.nbytes))

    def compute_gae(self):
        self._chk(self.lib.dril_compute_gae(self._h))

    # update
    def ppo_update(self) -> DrilPPOStats:
        st = DrilPPOStats()
        self._chk(self.lib.dril_ppo_update(self._h, C.byref(st)))
        return st

    def f32_retries(self) -> int:
        """updates redone on the exact-f32 kernels because an f16-piece kernel left f16's range (dril_f32_retries)"""
        return int(self.lib.dril_f32_retries(self._h))

    def f32_fallback_info(self) -> dict:
        """struct dril_f32_fallback as a dict: retries, direct_updates, persistent_fallbacks, latch_updates_left, forward_exact_f32, max_abs_w2"""
        fb = capi.DrilF32Fallback()
        self._chk(self.lib.dril_f32_fallback_info(self._h, C.byref(fb)))
        return {k: getattr(fb, k) for k, _ in fb._fields_ if k != "reserved"}

    def step_stats(self, rows: int) -> np.ndarray:
        """dril_debug_get_step_stats: the (rows, 16) per-optimiser-step rows of the last ppo_update as the device wrote them"""
        out = np.zeros((int(rows), 16), np.float32)
        if rows:
            self._chk(self.lib.dril_debug_get_step_stats(self._h, self._p(out), int(rows)))
        return out

    def set_permutation(self, perm: Optional[np.ndarray]):
        if perm is None:
            self._chk(self.lib.dril_debug_set_permutation(self._h, None, 0))
            return
        perm = np.ascontiguousarray(perm, np.int64)
        self._chk(self.lib.dril_debug_set_permutation(self._h, self._p(perm), perm.size))

    def ppo_loss_grad(self, obs, actions, adv, ret, old_logp, old_val):
        obs = np.ascontiguousarray(obs, np.float32)
        actions = np.ascontiguousarray(actions, np.int32 if self.discrete else np.float32)
        adv, ret, old_logp, old_val = (np.ascontiguousarray(x, np.float32) for x in (adv, ret, old_logp, old_val))
        loss = C.c_float()
        stats = np.empty(7, np.float32)
        grads = np.empty(self.P, np.float32)
        self._chk(self.lib.dril_ppo_loss_grad(self._h, self._p(obs), self._p(actions), self._p(adv), self._p(ret), self._p(old_logp),
                                              self._p(old_val), obs.shape[0], C.byref(loss), self._p(stats), self._p(grads)))
        return loss.value, stats, grads

    def apply_gradients(self, grads: np.ndarray) -> float:
        grads = np.ascontiguousarray(grads, np.float32)
        norm = C.c_float()
        self._chk(self.lib.dril_apply_gradients(self._h, self._p(grads), grads.size, C.byref(norm)))
        return norm.value

    def evaluate_agent(self, n_eval_episodes: int = 10, deterministic: bool = True):
        """evaluate_agent(agent, env; n_eval_episodes, deterministic) -> (stats dict, episode_rewards, episode_lengths), evaluation.jl:54-143"""
        st = capi.DrilEvalStats()
        er = np.empty(n_eval_episodes, np.float32); el = np.empty(n_eval_episodes, np.int32)
        self._chk(self.lib.dril_evaluate_agent(self._h, n_eval_episodes, int(deterministic), C.byref(st), self._p(er), self._p(el)))
        return dict(mean_reward=st.mean_reward, std_reward=st.std_reward, mean_length=st.mean_length, std_length=st.std_length,
                    n_steps=st.n_steps), er, el

    def _evaluate_agent_device(self, n_eval_episodes: int = 10, deterministic: bool = True, seed: Optional[int] = None, poll_steps: int = 0,
                               force_step_granular: bool = False, persistent: bool = False):
        """The same evaluation with the episode accounting on the device, leaving nothing behind on the handle (dril_evaluate_agent_device, docs/evaluation.md)
        -> (stats dict, episode_rewards, episode_lengths, info dict).  seed None: the env seed in force; env e is reset with seed + its global index.
        persistent=True asks for the persistent evaluate kernel wherever it can run, cfg.norm_* handles included (the frozen statistics are an argument of the
        kernel); the default keeps such handles on the step-granular launches.  force_step_granular wins.
        info: path (what ran: 0 step-granular launches, 1 the persistent evaluate kernel, 2 a plug-in's fused evaluation kernel — persistent=True on a plug-in handle
        whose code object carries one, evaluate_fused_info), launches, steps_enqueued, events."""
        o = capi.DrilEvalOptions()
        self._chk(self.lib.dril_eval_options_default(C.byref(o)))
        o.n_eval_episodes, o.deterministic, o.poll_steps, o.force_step_granular = int(n_eval_episodes), int(deterministic), int(poll_steps), int(force_step_granular)
        o.reserved[capi.EVAL_OPT_PERSISTENT] = int(bool(persistent))
        if seed is not None:
            o.seed, o.has_seed = int(seed), 1
        st, info = capi.DrilEvalStats(), capi.DrilEvalInfo()
        n = max(int(n_eval_episodes), 0)
        er = np.empty(n, np.float32); el = np.empty(n, np.int32)
        self._chk(self.lib.dril_evaluate_agent_device(self._h, C.byref(o), C.byref(st), self._p(er), self._p(el), C.byref(info)))
        return (dict(mean_reward=st.mean_reward, std_reward=st.std_reward, mean_length=st.mean_length, std_length=st.std_length, n_steps=st.n_steps), er, el,
                dict(path=info.path, launches=info.launches, steps_enqueued=info.steps_enqueued, events=info.events))

    @_opt_in_persistent(_evaluate_agent_device)
    def evaluate_agent_device(self, n_eval_episodes: int = 10, deterministic: bool = True, seed: Optional[int] = None, poll_steps: int = 0,
                              force_step_granular: bool = False):
        """Handle._evaluate_agent_device with the keyword-only option `persistent` (default False): evaluate_agent_device(..., persistent=True)."""

    def _collect_trajectory_device(self, n_trajectories: int = 1, max_steps: Optional[int] = None, deterministic: bool = True, seed: Optional[int] = None,
                                   poll_steps: int = 0, final_original: bool = False, persistent: bool = False):
        """collect_trajectory on the device, leaving nothing behind on the handle (dril_collect_trajectory_device, docs/evaluation.md): envs 0..n_trajectories-1 record
        their first episode after the call's own reset -> (trajectories, lengths, end_flags, info dict).  trajectories[m] = (observations (L+1, D), actions (L,) | (L, A),
        rewards (L,)): original observations (rows 0..L-1 unscaled under ScalingWrapperEnv, never normalised), the actions the env's physics received, raw rewards;
        the last observation is the terminal state as the wrapper delivers it (final_original: unscaled too).  end_flags: capi.TRAJ_TERMINATED | TRAJ_TRUNCATED |
        TRAJ_MAX_STEPS.  persistent=True asks for the one-launch form (the recording inside the persistent evaluate kernel, K steps per launch, no shadow envs)
        where that kernel can run; elsewhere the request falls back silently.  The recording is the same, bit for bit.
        info: capacity, steps_enqueued, launches, longest, cut_by_max_steps, path (what ran: 0 step-granular launches, 1 the persistent kernel, 2 the recording mode
        of a plug-in's fused evaluation kernel)."""
        o = capi.DrilTrajOptions()
        self._chk(self.lib.dril_traj_options_default(C.byref(o)))
        o.n_trajectories, o.max_steps, o.deterministic = int(n_trajectories), 0 if max_steps is None else int(max_steps), int(deterministic)
        o.poll_steps, o.final_original = int(poll_steps), int(bool(final_original))
        o.reserved[capi.TRAJ_OPT_PERSISTENT] = int(bool(persistent))
        if max_steps is not None and int(max_steps) < 1:
            raise ValueError("max_steps is None or >= 1")
        if seed is not None:
            o.seed, o.has_seed = int(seed), 1
        cap, info = C.c_int32(), capi.DrilTrajInfo()
        self._chk(self.lib.dril_trajectory_capacity(self._h, C.byref(o), C.byref(cap)))
        M, T = max(int(n_trajectories), 1), cap.value
        obs = np.empty((M, T + 1, self.D), np.float32)
        act = np.empty((M, T), np.int32) if self.discrete else np.empty((M, T, self.A), np.float32)
        rew = np.empty((M, T), np.float32); lengths = np.empty(M, np.int32); flags = np.empty(M, np.uint8)
        self._chk(self.lib.dril_collect_trajectory_device(self._h, C.byref(o), self._p(obs), self._p(act), self._p(rew), self._p(lengths), self._p(flags), C.byref(info)))
        trajs = [(obs[m, :L + 1].copy(), act[m, :L].copy(), rew[m, :L].copy()) for m, L in enumerate(lengths)]
        return trajs, lengths, flags, dict(capacity=info.capacity, steps_enqueued=info.steps_enqueued, launches=info.launches, longest=info.longest,
                                           cut_by_max_steps=info.cut_by_max_steps, path=info.reserved[capi.TRAJ_INFO_PATH])

    @_opt_in_persistent(_collect_trajectory_device)
    def collect_trajectory_device(self, n_trajectories: int = 1, max_steps: Optional[int] = None, deterministic: bool = True, seed: Optional[int] = None,
                                  poll_steps: int = 0, final_original: bool = False):
        """Handle._collect_trajectory_device with the keyword-only option `persistent` (default False): collect_trajectory_device(..., persistent=True)."""

    def train(self, max_steps: int):
        per_iter = self.N * self.cfg.world_size
        iters = max_steps // per_iter
        stats = (DrilPPOStats * max(iters, 1))()
        fps = (C.c_double * max(iters, 1))()
        done = C.c_int32()
        self._chk(self.lib.dril_train(self._h, max_steps, stats, fps, C.byref(done)))
        return [stats[i] for i in range(done.value)], [fps[i] for i in range(done.value)]

    # multi-GPU
    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * 128)()
        rc = self.lib.dril_comm_unique_id(buf)
        if rc != capi.OK:
            raise DrilError(rc, (self.lib.dril_last_error(None) or b"").decode())
        return bytes(buf)

    def comm_init(self, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._chk(self.lib.dril_comm_init(self._h, buf))

    def comm_ranks(self) -> int:
        """ranks the communicator itself reports (ncclCommCount), 1 without a communicator"""
        return int(self.lib.dril_comm_ranks(self._h))

    def grad_kernel_info(self) -> str:
        """"<kernel>: <arithmetic>" of the last optimiser step's gradient kernel"""
        return self.lib.dril_grad_kernel_info(self._h).decode()

    def comm_allreduce_calls(self) -> int:
        return int(self.lib.dril_comm_allreduce_calls(self._h))

    def device_info(self) -> str:
        """"device <ordinal> of <n> visible: <name> <arch>, <CUs> CUs, PCI <bus id>, HIP_VISIBLE_DEVICES=.. ROCR_VISIBLE_DEVICES=.." (dril_device_info)"""
        return (self.lib.dril_device_info(self._h) or b"").decode()

    @staticmethod
    def comm_loopback(handles: Sequence["Handle"]):
        """DEBUG / TEST: join handles (ranks 0..n-1 of one process, one device) into a loopback communicator; afterwards every handle
        must be driven from its own thread (dril_debug_comm_loopback, include/dril_hip.h)"""
        arr = (C.c_void_p * len(handles))(*[h._h for h in handles])
        rc = handles[0].lib.dril_debug_comm_loopback(arr, len(handles))
        if rc != capi.OK:
            msg = b""
            for h in handles:
                msg = msg or (h.lib.dril_last_error(h._h) or b"")
            raise DrilError(rc, (msg or handles[0].lib.dril_last_error(None) or b"").decode())

    # measurement
    def synchronize(self):
        self._chk(self.lib.dril_synchronize(self._h))

    def profile(self) -> dict:
        """per kernel class since the last reset: `launches` (all of them), `timed_launches` / `timed_ms` (the launches bracketed by HIP events: all of them at
        profile_events = 1, every k-th of the per-optimiser-step classes at profile_events = k) and `total_ms` = timed average x launches"""
        out = {}
        for k in range(capi.K_COUNT):
            ms, n, na = C.c_double(), C.c_int64(), C.c_int64()
            self._chk(self.lib.dril_profile_get(self._h, k, C.byref(ms), C.byref(n)))
            self._chk(self.lib.dril_profile_launches(self._h, k, C.byref(na)))
            out[self.lib.dril_kernel_name(k).decode()] = {"total_ms": ms.value * (na.value / n.value if n.value else 0.0), "launches": na.value if n.value else 0,
                                                          "timed_ms": ms.value, "timed_launches": n.value}
        return out

    def profile_reset(self):
        self._chk(self.lib.dril_profile_reset(self._h))


# --------------------------------------------------------------------------------------------
# DeviceParallelEnv <: AbstractParallelEnv (interfaces/environments.jl:21-39)
# --------------------------------------------------------------------------------------------
class Population:
    """Owns one dril_population*: ordinary PPO handles joined for batched launches (include/dril_hip.h, docs/population.md).  Every member is bit-identical to the
    same handle driven alone; the handles stay the caller's and every Handle method works on a member between population calls.  close() (or leaving the `with`
    block) releases the population, never the members; a member cannot be closed while it is joined."""

    def __init__(self, handles: Sequence[Handle]):
        handles = list(handles)
        if not handles:
            raise ValueError("Population: at least one handle")
        self.handles = handles
        self.lib = handles[0].lib
        self._p = C.c_void_p()
        arr = (C.c_void_p * len(handles))(*[h._h for h in handles])
        rc = self.lib.dril_population_join(arr, len(handles), C.byref(self._p))
        if rc != capi.OK:
            raise DrilError(rc, (self.lib.dril_population_last_error(None) or b"").decode())

    def __len__(self):
        return len(self.handles)

    def close(self):
        if self._p:
            self.lib.dril_population_destroy(self._p)
            self._p = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != capi.OK:
            raise DrilError(rc, (self.lib.dril_population_last_error(self._p) or b"").decode())

    def collect_rollout(self) -> list:
        """dril_collect_rollout of every member in one launch; returns the members' fps"""
        fps = (C.c_double * len(self))()
        self._chk(self.lib.dril_population_collect_rollout(self._p, fps))
        return list(fps)

    def ppo_update(self) -> list:
        """dril_ppo_update of every member in one launch per `cap` members; returns the members' DrilPPOStats"""
        st = (DrilPPOStats * len(self))()
        self._chk(self.lib.dril_population_ppo_update(self._p, st))
        return list(st)

    def train(self, max_steps: int):
        """dril_train of every member: (stats[iteration][member], fps[iteration][member]) of the iterations that completed"""
        n = len(self)
        iters = max_steps // self.handles[0].N
        stats = (DrilPPOStats * (max(iters, 1) * n))()
        fps = (C.c_double * (max(iters, 1) * n))()
        done = C.c_int32()
        self._chk(self.lib.dril_population_train(self._p, max_steps, stats, fps, C.byref(done)))
        return ([[stats[i * n + m] for m in range(n)] for i in range(done.value)], [[fps[i * n + m] for m in range(n)] for i in range(done.value)])

    def info(self) -> dict:
        i = capi.DrilPopulationInfo()
        self._chk(self.lib.dril_population_info(self._p, C.byref(i)))
        return {k: getattr(i, k) for k, _ in i._fields_ if k != "reserved"}

    def evaluate(self, n_eval_episodes: int = 10, deterministic: bool = True, seed: Optional[int] = None, poll_steps: int = 0, force_step_granular: bool = False) -> list:
        """Handle.evaluate_agent_device of every member, with one evaluate_pop_kernel launch and one look at the members' counters per K env steps
        (dril_population_evaluate_device, docs/population.md "Evaluation") -> [(stats dict, episode_rewards, episode_lengths, info dict), ...] per member, each byte
        for byte what the member's own evaluate_agent_device returns; nothing is left behind on any member.  seed=None: every member's own env seed in force;
        a seed: the same for all members (common random numbers).  self.last_eval_info: launches, looks, batched_members, solo_members, kernel_ms."""
        n = len(self)
        o = capi.DrilEvalOptions()
        rc = self.lib.dril_eval_options_default(C.byref(o))
        if rc != capi.OK:
            raise DrilError(rc, "dril_eval_options_default")
        o.n_eval_episodes, o.deterministic, o.poll_steps, o.force_step_granular = int(n_eval_episodes), int(deterministic), int(poll_steps), int(bool(force_step_granular))
        if seed is not None:
            o.seed, o.has_seed = int(seed), 1
        ne = max(int(n_eval_episodes), 1)
        st = (capi.DrilEvalStats * n)(); mi = (capi.DrilEvalInfo * n)(); pi = capi.DrilPopulationEvalInfo()
        er = np.empty((n, ne), np.float32); el = np.empty((n, ne), np.int32)
        self.last_eval_info = None
        self._chk(self.lib.dril_population_evaluate_device(self._p, C.byref(o), st, er.ctypes.data_as(C.c_void_p), el.ctypes.data_as(C.c_void_p), mi, C.byref(pi)))
        self.last_eval_info = {k: getattr(pi, k) for k, _ in pi._fields_ if k != "reserved"}
        return [(dict(mean_reward=s.mean_reward, std_reward=s.std_reward, mean_length=s.mean_length, std_length=s.std_length, n_steps=s.n_steps), er[m].copy(), el[m].copy(),
                 dict(path=i.path, launches=i.launches, steps_enqueued=i.steps_enqueued, events=i.events)) for m, (s, i) in enumerate(zip(st, mi))]


class DeviceParallelEnv:
    """Device-resident batched simulator standing in for
    `MultiThreadedParallelEnv([CartPoleEnv() for _ in 1:n_envs])`.  The env verbs keep the reference's
    contract (auto-reset, `terminal_observation` only on truncation,
    multithreadedParallelEnv.jl:47-74) with host copy-out, so generic callers keep working; `train_`
    dispatches to the fused device path."""

    def __init__(self, env, n_envs: int, *, seed: int = 42, fixed_length_episodes: bool = False, device: int = 0,
                 rank: int = 0, world_size: int = 1, profile_events: bool = False):
        self.env, self.n_envs, self.seed = env, n_envs, seed
        self._kw = dict(fixed_length_episodes=fixed_length_episodes, device=device, rank=rank, world_size=world_size,
                        profile_events=profile_events, normalize=None, monitor_window=0)
        self.handle: Optional[Handle] = None
        self._bound_key = None
        self._last_term = np.zeros(n_envs, bool)
        self._last_trunc = np.zeros(n_envs, bool)
        self.last_f32_paths: list = []      # dril_ppo_stats.f32_path of every iteration of the last train_ (0 = the default kernels throughout)
        self.norm_fused_rollout = False     # NormalizeWrapperEnv(env, fused_rollout=True): dril_norm_rollout_enable on every handle bound to this env

    def f32_fallback_info(self) -> dict:
        """how often this env's handle left the f16-piece arithmetic (dril_f32_fallback_info); all zeros for a healthy run on normalised data"""
        return self.handle.f32_fallback_info() if self.handle else {}

    # binding: one handle carries env + agent + alg state; (re)created when the alg/layer shape changes
    def bind(self, alg: PPO, layer: Optional[ActorCriticLayer] = None) -> Handle:
        key = (tuple(sorted(asdict(alg).items())), None if layer is None else (tuple(layer.hidden_dims), layer.log_std_init, getattr(layer, "activation", "tanh")),
               None if self._kw["normalize"] is None else tuple(sorted(self._kw["normalize"].items())), self._kw["monitor_window"], self._bind_extra())
        if self.handle is None or key != self._bound_key:
            if self.handle is not None:
                self.handle.close()
            cfg = make_config(self.env, self.n_envs, alg, layer, seed=self.seed, **self._kw)
            self.handle = Handle(cfg, env_module=getattr(self.env, "code_object_path", None))
            self._after_create(self.handle)
            self.handle.env_reset(self.seed)  # Random.seed!(env, seed) + reset!(env)
            self._bound_key = key
        return self.handle

    def _bind_extra(self):
        """what bind's key holds beyond the config: here the one-launch normalised collection; a subclass states its own"""
        return self.norm_fused_rollout

    def _after_create(self, h: Handle):
        """verbs applied to a freshly created handle, before its first reset: here the one-launch normalised collection; a subclass states its own"""
        if self.norm_fused_rollout:
            h.norm_rollout_enable(True)

    def _h(self) -> Handle:
        return self.handle or self.bind(PPO(n_steps=1, batch_size=self.n_envs * max(1, self._kw["world_size"])))

    def number_of_envs(self) -> int:
        return self.n_envs

    def observation_space(self):
        return self.env.observation_space()

    def action_space(self):
        return self.env.action_space()

    def reset_(self):
        self._h().env_reset(self.seed)

    def observe(self):
        """-> list of n_envs observation vectors (multithreadedParallelEnv.jl:19-25)."""
        return list(self._h().env_observe())

    def act_(self, actions):
        """-> (rewards, terminateds, truncateds, infos) (multithreadedParallelEnv.jl:47-74)."""
        rew, term, trunc, tobs = self._h().env_step(np.asarray(actions))
        infos = [dict() for _ in range(self.n_envs)]
        for i in np.nonzero(trunc)[0]:
            infos[i]["terminal_observation"] = tobs[i].copy()
        self._last_term, self._last_trunc = term, trunc
        return rew, term, trunc, infos

    def terminated(self):
        return self._last_term

    def truncated(self):
        return self._last_trunc


@dataclass
class ModuleEnv:
    """One env of a device env plug-in: the spaces and the time limit its code object declares."""
    code_object_path: str
    info: dict
    max_steps: int
    action_start: int = 1
    kind: int = capi.ENV_MODULE
    scaling: bool = False            # ScalingWrapperEnv around the env (DeviceModuleEnv(..., scaling=True) / ScalingWrapperEnv(DeviceModuleEnv(...)))

    def declared_observation_space(self):
        """the env's own observation space: the declared box, or Box(-inf, inf) when the plug-in declares none"""
        D = self.info["obs_dim"]
        if not self.info.get("obs_declared"):
            return Box((-math.inf,) * D, (math.inf,) * D)
        return Box(tuple(float(v) for v in self.info["obs_low"]), tuple(float(v) for v in self.info["obs_high"]))

    def declared_action_space(self):
        if self.info["discrete"]:
            return Discrete(self.info["action_dim"], self.action_start)
        return Box(tuple(float(v) for v in self.info["action_low"]), tuple(float(v) for v in self.info["action_high"]))

    def observation_space(self):
        D = self.info["obs_dim"]
        return Box((-1.0,) * D, (1.0,) * D) if self.scaling else self.declared_observation_space()

    def action_space(self):
        A = self.info["action_dim"]
        return Box((-1.0,) * A, (1.0,) * A) if self.scaling else self.declared_action_space()

    # scale! / unscale! (scalingWrapperEnv.jl:71-79) on host arrays, from the declared bounds
    def _bounds(self, space):
        return (np.asarray(v, np.float32) for v in (space.low, space.high))

    def scale_observation(self, obs):
        lo, hi = self._bounds(self.declared_observation_space())
        return (np.asarray(obs, np.float32) - lo) * (np.float32(2) / (hi - lo)) - np.float32(1)

    def unscale_observation(self, obs):
        lo, hi = self._bounds(self.declared_observation_space())
        return (np.asarray(obs, np.float32) + np.float32(1)) / (np.float32(2) / (hi - lo)) + lo

    def unscale_action(self, act):
        lo, hi = self._bounds(self.declared_action_space())
        return (np.asarray(act, np.float32) + np.float32(1)) / (np.float32(2) / (hi - lo)) + lo


class DeviceModuleEnv(DeviceParallelEnv):
    """`n_envs` copies of the CALLER'S OWN env, living on the device: the env is a gfx950 code object built from include/device/dril_env_plugin.h
    (`hipcc --genco`), loaded by the library and stepped by its own kernels where a built-in env's kernels would run — no host env anywhere in the loop.
    Everything a DeviceParallelEnv does works unchanged (Agent, train_, collect_rollout_, MonitorWrapperEnv, callbacks, evaluate_agent, checkpoints).

    `normalize=dict(training=..., norm_obs=..., norm_reward=..., clip_obs=..., clip_reward=..., gamma=..., epsilon=...)` (any subset; `{}` = the defaults of
    normalizeWrapperEnv.jl:71-80) puts NormalizeWrapperEnv around the envs for any observation width: the handle is created plain and the wrapper is switched on with
    dril_normalize_enable, so train_, collect_rollout_, evaluate_agent (frozen statistics, raw episode returns), unnormalize_obs_ / unnormalize_rewards_ and
    get_original_obs / get_original_rewards honour it.  The keyword takes part in bind's key.  The statistics live in the handle: a bind that has to re-create the
    handle (another alg or layer shape) starts a FRESH wrapper — a caller who wants to carry the statistics over saves them before
    (`env.handle.normalize_get_stats()`) and loads them after (`env.handle.normalize_set_stats(**st)`).
    The function NormalizeWrapperEnv(DeviceModuleEnv(...)) stays refused: it works through cfg.norm_*, which size the built-in envs' tables (docs/external_envs.md).

    `scaling=True` (or ScalingWrapperEnv(DeviceModuleEnv(...))) puts ScalingWrapperEnv around every env: the plug-in's own _scaled kernels run where observe / step ran
    (dril_scaling_enable, applied to a fresh handle before its first reset), `observation_space()` / `action_space()` become Box(-1, 1), and NormalizeWrapperEnv —
    when both are asked for — sits outside it.  It needs a plug-in that declares finite obs_low / obs_high; the library's refusal says what is missing.  Part of
    bind's key.  `scale_observation / unscale_observation / unscale_action` convert host arrays with the declared bounds.

    `fused_rollout=True` makes every PPO collection ONE launch of the plug-in's own rollout kernel (dril_rollout_fused_enable) — the code object must be built with
    DRIL_ENV_PLUGIN_ROLLOUT (include/device/dril_env_rollout.h); not together with `normalize`.  The library's refusal says what is missing.  Part of bind's key.

    A code object built with DRIL_ENV_PLUGIN_WORLD (include/device/dril_env_world.h) holds a multi-agent WORLD, the device form of MultiAgentParallelEnv: `n_envs` counts
    rows, `agents_per_world` of them share one state and one joint step (row w N + i is agent i of world w), `n_worlds = n_envs / agents_per_world`; for a classic
    plug-in the two numbers are 1 and n_envs.  One shared policy acts for every row; `scaling` and `fused_rollout` are refused by the library for a world, and
    collect_trajectory records whole worlds (n_trajectories a multiple of agents_per_world)."""

    def __init__(self, code_object_path, n_envs: int, *, seed: int = 42, device: int = 0, max_steps: Optional[int] = None, action_start: int = 1,
                 fixed_length_episodes: bool = False, rank: int = 0, world_size: int = 1, profile_events: bool = False, normalize: Optional[dict] = None,
                 scaling: bool = False, fused_rollout: bool = False):
        info = describe_env_module(code_object_path, device)
        # a world (include/device/dril_env_world.h): agents_per_world rows share one state and one joint step; row w N + i is agent i of world w
        self.agents_per_world = int(info["agents"])
        if int(n_envs) % self.agents_per_world != 0:
            raise ValueError(f"{info['name']} is a world of {self.agents_per_world} agents (one row each): n_envs {n_envs} is not a multiple of {self.agents_per_world}")
        self.n_worlds = int(n_envs) // self.agents_per_world
        env = ModuleEnv(os.fspath(code_object_path), info, int(max_steps) if max_steps else info["episode_len"], action_start, scaling=bool(scaling))
        super().__init__(env, n_envs, seed=seed, fixed_length_episodes=fixed_length_episodes, device=device, rank=rank, world_size=world_size,
                         profile_events=profile_events)
        if normalize is not None:
            bad = [k for k in normalize if k not in Handle._NORMALIZE_KEYS]
            if bad:
                raise TypeError(f"NormalizeWrapperEnv has no keyword {bad[0]!r}")
            normalize = {**_normalize.DEFAULTS, **normalize}
        self.module_normalize = normalize
        self.fused_rollout = bool(fused_rollout)

    def _bind_extra(self):
        return (None if self.module_normalize is None else tuple(sorted(self.module_normalize.items())), self.env.scaling, self.fused_rollout)

    def _after_create(self, h: Handle):
        if self.env.scaling:                      # inside NormalizeWrapperEnv: its statistics are those of scaled observations
            h.scaling_enable(True)
        if self.fused_rollout:
            h.rollout_fused_enable(True)
        if self.module_normalize is not None:
            h.normalize_enable(**self.module_normalize)

    def _set_scaling(self, on: bool):
        self.env.scaling = bool(on)
        if self.handle is not None:
            self.handle.close(); self.handle = None
        if on:                                    # fail here, with the library's message, rather than at the first bind
            self._h()
        return self

    def scale_observation(self, obs):
        return self.env.scale_observation(obs)

    def unscale_observation(self, obs):
        return self.env.unscale_observation(obs)

    def unscale_action(self, act):
        return self.env.unscale_action(act)


class HostParallelEnv:
    """`BroadcastedParallelEnv(envs)` (broadcastedParallelEnv.jl:41-66) over the CALLER'S OWN envs: any objects with the reference's
    AbstractEnv verbs (interfaces/environments.jl:21-39) — `reset_()`, `act_(action) -> reward`, `observe()`, `terminated()`,
    `truncated()`, `observation_space()`, `action_space()`, optional `get_info()`.  The envs step on the host; `train_` sends their
    observations to the device once per step and runs everything else there (DRIL_ENV_EXTERNAL: dril_ext_act / _record / _finish,
    generic kernels for any obs / action / hidden width)."""
    kind = capi.ENV_EXTERNAL

    def __init__(self, envs, *, seed: int = 42, device: int = 0, profile_events: bool = False):
        self.envs, self.n_envs, self.seed = list(envs), len(envs), seed
        self._kw = dict(device=device, profile_events=profile_events)
        self.handle: Optional[Handle] = None
        self._bound_key = None
        self._last_term = np.zeros(self.n_envs, bool)
        self._last_trunc = np.zeros(self.n_envs, bool)

    def bind(self, alg: PPO, layer: Optional[ActorCriticLayer] = None) -> Handle:
        key = (tuple(sorted(asdict(alg).items())), None if layer is None else (tuple(layer.hidden_dims), layer.log_std_init, getattr(layer, "activation", "tanh")))
        if self.handle is None or key != self._bound_key:
            if self.handle is not None:
                self.handle.close()
            self.handle = Handle(make_config(self, self.n_envs, alg, layer, seed=self.seed, **self._kw))
            self._bound_key = key
        return self.handle

    def number_of_envs(self) -> int:
        return self.n_envs

    def observation_space(self):
        return self.envs[0].observation_space()

    def action_space(self):
        return self.envs[0].action_space()

    def reset_(self):
        for e in self.envs:
            e.reset_()

    def observe(self):
        return [np.asarray(e.observe(), np.float32).ravel() for e in self.envs]

    def act_(self, actions):
        """-> (rewards, terminateds, truncateds, infos); auto-reset, `terminal_observation` only on truncation (:58-66)"""
        assert len(actions) == self.n_envs
        rewards = np.array([e.act_(a) for e, a in zip(self.envs, actions)], np.float32)
        term = np.array([bool(e.terminated()) for e in self.envs]); trunc = np.array([bool(e.truncated()) for e in self.envs])   # before the reset
        infos = [dict(e.get_info()) if hasattr(e, "get_info") else dict() for e in self.envs]
        for i, e in enumerate(self.envs):
            if trunc[i]:
                infos[i]["terminal_observation"] = np.asarray(e.observe(), np.float32).ravel().copy()
            if term[i] or trunc[i]:
                e.reset_()
        self._last_term, self._last_trunc = term, trunc
        return rewards, term, trunc, infos

    def terminated(self):
        return self._last_term

    def truncated(self):
        return self._last_trunc


def _host_rollout(h: Handle, env: HostParallelEnv, on_step=None):
    """collect_trajectories (trajectory.jl:22-78) with the envs on the host and the agent on the device; -> fps (rollout_buffer.jl:60-64), or None
    when an on_step callback stopped the collection (:34-39)"""
    t0 = time.perf_counter()
    asp = env.action_space()
    new_obs = np.stack(env.observe())                                                # :32
    for _ in range(h.T):
        if on_step is not None and not on_step():
            return None
        raw, ea = h.ext_act(new_obs)                                                 # get_action_and_values + to_env, :41-42
        if isinstance(asp, Box) and h.cfg.ext_action_low >= h.cfg.ext_action_high:   # per-dimension bounds: ClampAdapter here (default_adapters.jl:4-11)
            ea = np.clip(ea, np.asarray(asp.low, np.float32).reshape(1, -1), np.asarray(asp.high, np.float32).reshape(1, -1))
        acts = list(ea) if h.discrete else [a.reshape(asp.shape) for a in ea]
        rew, term, trunc, infos = env.act_(acts)                                     # :44
        new_obs = np.stack(env.observe())                                            # :45
        tobs = None
        if trunc.any():
            tobs = np.zeros((h.E, h.D), np.float32)
            for i in np.nonzero(trunc)[0]:
                tobs[i] = infos[i]["terminal_observation"]
        h.ext_record(rew, term, trunc, tobs)                                         # :46-61
    h.ext_finish(new_obs)                                                            # :65-70 + compute_advantages! + returns
    return h.N / max(time.perf_counter() - t0, 1e-12)


def _default_empty(like):
    """the `empty(shape, dtype)` factory of the array library `like` comes from: torch tensors and CuPy arrays are recognised"""
    mod = type(like).__module__.split(".")[0]
    if mod == "torch":
        import torch
        return lambda shape, dtype: torch.empty(tuple(shape), dtype=getattr(torch, np.dtype(dtype).name), device=like.device)
    if mod == "cupy":
        import cupy
        return lambda shape, dtype: cupy.empty(tuple(shape), dtype=np.dtype(dtype))
    raise ValueError(f"DeviceArrayParallelEnv: cannot allocate action arrays like {type(like).__name__}; pass empty=lambda shape, dtype: <a device array of your library>")


def _to_host(a, stream) -> np.ndarray:
    """a small device array (rewards, flags) as NumPy, for the episode accounting of evaluate_agent: the caller's stream is drained, then one blocking copy"""
    cai = a.__cuda_array_interface__
    out = np.empty(tuple(cai["shape"]), np.dtype(cai["typestr"]))
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]; hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for rc in (hip.hipStreamSynchronize(_stream_ptr(stream)), hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(int(cai["data"][0])), out.nbytes, 2)):   # 2 = hipMemcpyDeviceToHost
        if rc != 0:
            raise DrilError(capi.ERR_HIP, f"copying a device array to the host failed with HIP status {rc}")
    return out


class DeviceArrayParallelEnv:
    """The twin of HostParallelEnv for ONE batched env object whose arrays live on the DEVICE (a simulator in torch-ROCm / CuPy tensor ops, another HIP library):
        n_envs, observation_space(), action_space(), reset_()
        observe() -> (E, D) f32 device array
        act_(actions) -> (rewards (E,) f32, terminated (E,), truncated (E,) u8 / bool, terminal_obs (E, D) f32 or None), all device arrays; finished envs reset inside
                         act_ (as HostParallelEnv.act_ does), terminal_obs holds the pre-reset observation of the truncated envs (any other row may hold anything)
    `actions` is the wrapper's own env-action array — i32 (E,) | f32 (E, A), the ClampAdapter applied on the device — allocated once through `empty(shape, dtype)`
    (default: the library of the first observation).  `stream`: the hipStream_t the env's work runs on, an int or a callable returning one
    (`lambda: torch.cuda.current_stream().cuda_stream`); None = the null stream.  collect_rollout_, train_ and evaluate_agent accept it; a rollout makes no host
    wait before its last call (dril_ext_act_device / dril_ext_record_device / dril_ext_finish_device, docs/external_envs.md section 10)."""
    kind = capi.ENV_EXTERNAL

    def __init__(self, env, *, seed: int = 42, device: int = 0, stream=None, empty=None, profile_events: bool = False):
        for name in ("n_envs", "observation_space", "action_space", "reset_", "observe", "act_"):
            if not hasattr(env, name):
                raise TypeError(f"DeviceArrayParallelEnv: the env has no `{name}`")
        self.env, self.n_envs, self.seed, self.stream, self._empty = env, int(env.n_envs), seed, stream, empty
        self._kw = dict(device=device, profile_events=profile_events)
        self.handle: Optional[Handle] = None
        self.sac_handle = None                                                       # the SAC handle sac_train_ drives this env with (bind_sac); owned by its ReplayBuffer
        self._bound_key = None
        self._raw = self._env_actions = None
        self._last_term = self._last_trunc = None
        self.ext_normalize: Optional[dict] = None                                    # NormalizeWrapperEnv(env, ...) / MonitorWrapperEnv(env, window): the wrappers of the
        self.ext_monitor_window = 0                                                  # handle (dril_ext_normalize_enable / dril_ext_monitor_enable), switched on by bind

    def bind(self, alg: PPO, layer: Optional[ActorCriticLayer] = None) -> Handle:
        key = (tuple(sorted(asdict(alg).items())), None if layer is None else (tuple(layer.hidden_dims), layer.log_std_init, getattr(layer, "activation", "tanh")))
        self.sac_handle = None                                                       # PPO drives the env from here on
        if self.handle is None or key != self._bound_key:
            if self.handle is not None:
                self.handle.close()
            self.handle = h = Handle(make_config(self, self.n_envs, alg, layer, seed=self.seed, **self._kw))
            asp = self.action_space()
            if isinstance(asp, Box) and h.cfg.ext_action_low >= h.cfg.ext_action_high:   # per-dimension bounds: the ClampAdapter's table on the device
                h.ext_set_action_bounds(np.asarray(asp.low, np.float32), np.asarray(asp.high, np.float32))
            self._bound_key = key
            self._apply_wrappers()
        return self.handle

    def bind_sac(self, h):
        """the DRIL_ENV_EXTERNAL SacHandle that sac_train_ drives this env with: it takes the recorded wrappers (dril_sac_ext_normalize_enable /
        dril_sac_ext_monitor_enable), and monitor_stats, reset_ and the normalisation helpers answer from it until a PPO bind"""
        self.sac_handle = h
        self._apply_wrappers()
        return h

    def wrapper_handle(self):
        """the handle that holds the env's wrappers: the SAC handle of the latest sac_train_, else the bound PPO handle (None: neither yet)"""
        if self.sac_handle is not None and not getattr(self.sac_handle, "_h", True):                   # closed by its owner (replay_buffer.handle.close()): the env lets go of it
            self.sac_handle = None
        return self.sac_handle if self.sac_handle is not None else self.handle

    def _apply_wrappers(self):
        """the recorded wrappers on the bound handle (between rollouts / env steps): the same normaliser again keeps its statistics.  Handle and SacHandle carry the
        same ext_* method names"""
        h = self.wrapper_handle()
        if h is None:
            return
        h.ext_monitor_enable(self.ext_monitor_window)
        if self.ext_normalize is None:
            h.ext_normalize_enable(False)
        else:
            h.ext_normalize_enable(**self.ext_normalize)

    def monitor_stats(self):
        """what log_stats logs (env/ep_rew_mean, env/ep_len_mean, episodes in the window), monitorWrapperEnv.jl:64-70"""
        return self.wrapper_handle().ext_monitor_stats()

    def number_of_envs(self) -> int:
        return self.n_envs

    def observation_space(self):
        return self.env.observation_space()

    def action_space(self):
        return self.env.action_space()

    def reset_(self):
        self.env.reset_()
        if self.ext_normalize is not None and self.wrapper_handle() is not None:
            self.wrapper_handle().ext_normalize_reset(self.stream)                             # reset! of the wrapper: returns <- 0 (normalizeWrapperEnv.jl:111-121)

    def observe(self):
        return self.env.observe()

    def action_arrays(self, h: Handle, like):
        """(raw, env) action arrays of the handle's action shape, allocated once"""
        shape = (h.E,) if h.discrete else (h.E, h.A)
        if self._raw is None or tuple(self._raw.__cuda_array_interface__["shape"]) != shape:
            make = self._empty or _default_empty(like)
            dt = np.int32 if h.discrete else np.float32
            self._raw, self._env_actions = make(shape, dt), make(shape, dt)
        return self._raw, self._env_actions

    def act_(self, actions):
        """-> (rewards, terminated, truncated, terminal_obs or None), device arrays, as the env's own act_ returns them"""
        out = self.env.act_(actions)
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            n = len(out) if isinstance(out, (tuple, list)) else 1
            raise ValueError(f"DeviceArrayParallelEnv: act_ must return (rewards, terminated, truncated, terminal_obs or None), got {n} value{'s' if n != 1 else ''}")
        self._last_term, self._last_trunc = out[1], out[2]
        return tuple(out)

    def terminated(self):
        return self._last_term

    def truncated(self):
        return self._last_trunc


def _device_array_rollout(h: Handle, env: DeviceArrayParallelEnv, on_step=None):
    """collect_trajectories (trajectory.jl:22-78) with env arrays and agent both on the device: every call enqueues and returns, the one host wait is
    dril_ext_finish_device's.  -> fps, or None when an on_step callback stopped the collection"""
    t0 = time.perf_counter()
    new_obs = env.observe()                                                          # :32
    raw, ea = env.action_arrays(h, new_obs)
    for _ in range(h.T):
        if on_step is not None and not on_step():
            return None
        h.ext_act_device(new_obs, raw, ea, env.stream)                               # get_action_and_values + to_env, :41-42
        rew, term, trunc, tobs = env.act_(ea)                                        # :44
        new_obs = env.observe()                                                      # :45
        h.ext_record_device(rew, term, trunc, tobs, env.stream)                      # :46-61
    h.ext_finish_device(new_obs, env.stream)                                         # :65-70 + compute_advantages! + returns
    return h.N / max(time.perf_counter() - t0, 1e-12)



def _stepwise_rollout(h: Handle, env, on_step=None):
    """collect_trajectories (trajectory.jl:22-78) over a DeviceParallelEnv through the step-granular env verbs — the path callbacks with an `on_step`
    hook need; the buffer is assembled on the host and handed back for compute_advantages! (dril_compute_gae).  -> fps or None"""
    t0 = time.perf_counter()
    E, T, asp = h.E, h.T, env.action_space()
    obs_b = np.empty((T * E, h.D), np.float32); act_b = np.empty(T * E, np.int32) if h.discrete else np.empty((T * E, h.A), np.float32)
    rew_b, val_b, lp_b, boot_b = (np.zeros(T * E, np.float32) for _ in range(4)); fl_b = np.zeros(T * E, np.uint8)
    new_obs = h.env_observe()                                                        # :32
    for t in range(T):
        if on_step is not None and not on_step():
            return None
        a, v, lp = h.policy_forward(new_obs)                                         # :41
        ea = a if h.discrete else np.clip(a, np.asarray(asp.low, np.float32), np.asarray(asp.high, np.float32))   # to_env :42
        rew, term, trunc, tobs = h.env_step(ea)                                      # :44
        k = slice(t * E, (t + 1) * E)
        obs_b[k], act_b[k], rew_b[k], val_b[k], lp_b[k] = new_obs, a, rew, v, lp     # :46-51
        fl_b[k] = term.astype(np.uint8) | (trunc.astype(np.uint8) << 1)
        if trunc.any():
            boot_b[k][trunc] = h.predict_values(tobs[trunc])                         # :57-61
        new_obs = h.env_observe()                                                    # :45
    for which, arr in ((capi.BUF_OBSERVATIONS, obs_b), (capi.BUF_ACTIONS, act_b), (capi.BUF_REWARDS, rew_b), (capi.BUF_VALUES, val_b), (capi.BUF_LOGPROBS, lp_b),
                       (capi.BUF_FLAGS, fl_b), (capi.BUF_BOOTSTRAP, boot_b), (capi.BUF_LAST_VALUES, h.predict_values(new_obs))):   # :65-70
        h.set_buffer(which, arr)
    h.compute_gae()                                                                  # rollout_buffer.jl:83-87
    return h.N / max(time.perf_counter() - t0, 1e-12)


def MonitorWrapperEnv(env: DeviceParallelEnv, stats_window: int = 100) -> DeviceParallelEnv:
    """MonitorWrapperEnv(env, stats_window) (monitorWrapperEnv.jl:15-24): episode return/length statistics from the device
    done flags; `env.handle.monitor_stats()` gives what `log_stats` logs (env/ep_rew_mean, env/ep_len_mean)."""
    if isinstance(env, HostParallelEnv):
        raise TypeError("MonitorWrapperEnv: the envs of a HostParallelEnv live on the host and are wrapped there, env by env; the device wrappers take a DeviceParallelEnv or a DeviceArrayParallelEnv")
    if isinstance(env, DeviceArrayParallelEnv):                                      # the handle's own wrapper (dril_ext_monitor_enable): the same object, the wrapper recorded
        env.ext_monitor_window = int(stats_window)
        env._apply_wrappers()
        return env
    env._kw["monitor_window"] = int(stats_window)
    if env.handle is not None:
        env.handle.close(); env.handle = None
    return env


def NormalizeWrapperEnv(env: DeviceParallelEnv, *, training: bool = True, norm_obs: bool = True, norm_reward: bool = True,
                        clip_obs: float = 10.0, clip_reward: float = 10.0, gamma: float = 0.99, epsilon: float = 1e-8,
                        fused_rollout: bool = False) -> DeviceParallelEnv:
    """NormalizeWrapperEnv(env; kwargs...) (normalizeWrapperEnv.jl:71-107).  On device the wrapper is a mode of the same
    handle (running mean/std kernels fused around the env step), so this returns the env with the wrapper switched on.
    `fused_rollout=True` (built-in envs, n_envs <= 128, hidden_dims [64,64]) asks every handle bound to the env to collect in ONE launch of rollout_norm_kernel
    (dril_norm_rollout_enable, docs/normalized_rollout.md) — through `train_` and `train_population_` alike; the library refuses, with what to do, where it cannot."""
    if fused_rollout and (isinstance(env, (HostParallelEnv, DeviceArrayParallelEnv, DeviceModuleEnv)) or not (norm_obs or norm_reward)):
        raise TypeError("NormalizeWrapperEnv(fused_rollout=True) is the one-launch collection of a normalising built-in env (norm_obs and / or norm_reward): a device env "
                        "plug-in has DeviceModuleEnv(path, n, fused_rollout=True), host and device-array envs step outside the library")
    if isinstance(env, HostParallelEnv):
        raise TypeError("NormalizeWrapperEnv: the envs of a HostParallelEnv live on the host and are wrapped there (the statistics couple all envs at every step); the device wrappers take a DeviceParallelEnv or a DeviceArrayParallelEnv")
    if isinstance(env, DeviceArrayParallelEnv):                                      # the handle's own wrapper (dril_ext_normalize_enable): the same object, the wrapper recorded
        env.ext_normalize = dict(training=training, norm_obs=norm_obs, norm_reward=norm_reward, clip_obs=clip_obs, clip_reward=clip_reward, gamma=gamma, epsilon=epsilon)
        env._apply_wrappers()
        return env
    env._kw["normalize"] = dict(training=training, norm_obs=norm_obs, norm_reward=norm_reward, clip_obs=clip_obs,
                                clip_reward=clip_reward, gamma=gamma, epsilon=epsilon)
    env.norm_fused_rollout = bool(fused_rollout)
    if env.handle is not None:
        env.handle.close(); env.handle = None
    if isinstance(env, DeviceModuleEnv) and (norm_obs or norm_reward):   # cfg.norm_* are the built-in envs': fail here, with the library's message and the way that works
        try:
            env._h()
        except DrilError as e:
            raise DrilError(e.code, str(e).split("] ", 1)[-1] + " — in Python: DeviceModuleEnv(path, n_envs, normalize=dict(...))") from None
    return env


def _normalize_kw(env: DeviceParallelEnv) -> Optional[dict]:
    """the wrapper's keywords: cfg.norm_* of a built-in env, the `normalize` keyword of a DeviceModuleEnv, the recorded wrapper of a DeviceArrayParallelEnv"""
    if isinstance(env, DeviceArrayParallelEnv):
        return env.ext_normalize
    return env._kw["normalize"] if env._kw["normalize"] is not None else getattr(env, "module_normalize", None)


class _ExtNormView:
    """the normaliser of an external handle (dril_ext_normalize_*) under the names the wrapper helpers use for every other handle"""

    def __init__(self, h: Handle):
        self.h = h

    def norm_get_stats(self) -> dict:
        return self.h.ext_normalize_get_stats()

    def norm_set_stats(self, *a, **kw):
        return self.h.ext_normalize_set_stats(*a, **kw)

    def norm_get_original(self):
        return self.h.ext_normalize_get_original()

    def normalize_config(self) -> dict:
        return self.h.ext_normalize_config()


def _norm_view(h):
    """h, or the view of its dril_ext_normalize_* / dril_sac_ext_normalize_* verbs when h is a PPO or SAC handle on external envs (norm_get_stats itself is
    unchanged there)"""
    ext = getattr(getattr(h, "cfg", None), "env_kind", None) == capi.ENV_EXTERNAL and hasattr(h, "ext_normalize_get_stats")
    return _ExtNormView(h) if ext else h


def _env_handle(env):
    """the handle behind an env's wrappers: a DeviceArrayParallelEnv may be driven by a SAC handle (bind_sac)"""
    return env.wrapper_handle() if isinstance(env, DeviceArrayParallelEnv) else env.handle


def unnormalize_obs_(obs: np.ndarray, env: DeviceParallelEnv) -> np.ndarray:
    """unnormalize_obs!(obs, env) (normalizeWrapperEnv.jl:200-210): obs * sqrt(var + eps) + mean with the wrapper's running statistics, in place"""
    kw = _normalize_kw(env)
    if kw is None or not kw["norm_obs"]:
        return obs
    st = _norm_view(_env_handle(env)).norm_get_stats()
    obs *= np.sqrt(st["obs_var"] + np.float32(kw["epsilon"])); obs += st["obs_mean"]
    return obs


def unnormalize_rewards_(rewards: np.ndarray, env: DeviceParallelEnv) -> np.ndarray:
    """unnormalize_rewards!(rewards, env) (normalizeWrapperEnv.jl:212-218): rewards * sqrt(var(returns) + eps), in place"""
    kw = _normalize_kw(env)
    if kw is None or not kw["norm_reward"]:
        return rewards
    rewards *= np.sqrt(np.float32(_norm_view(_env_handle(env)).norm_get_stats()["ret_var"]) + np.float32(kw["epsilon"]))
    return rewards


def get_original_obs(env: DeviceParallelEnv) -> np.ndarray:
    return _norm_view(_env_handle(env)).norm_get_original()[0]


def get_original_rewards(env: DeviceParallelEnv) -> np.ndarray:
    return _norm_view(_env_handle(env)).norm_get_original()[1]


# --------------------------------------------------------------------------------------------
# RolloutBuffer + collect_rollout! (src/buffers/rollout_buffer.jl)
# --------------------------------------------------------------------------------------------
@dataclass
class RolloutBuffer:
    """Host mirror of RolloutBuffer (buffer_types.jl:3-15).  Arrays are TIME-MAJOR copies of the device
    buffer (n = t*n_envs + env); `to_reference_order` gives the permutation into the reference's
    trajectory-major completion order (rollout_buffer.jl:70-80)."""
    n_steps: int
    n_envs: int
    gae_lambda: float
    gamma: float
    observations: np.ndarray = None
    actions: np.ndarray = None
    rewards: np.ndarray = None
    advantages: np.ndarray = None
    returns: np.ndarray = None
    logprobs: np.ndarray = None
    values: np.ndarray = None
    flags: np.ndarray = None

    def __len__(self):
        return self.n_steps * self.n_envs

    def to_reference_order(self) -> np.ndarray:
        """order[p] = time-major index of element p of the reference's flat buffer: trajectories are
        appended when they end, scanning steps then envs (trajectory.jl:46-75)."""
        E, T = self.n_envs, self.n_steps
        done = (self.flags.reshape(T, E) != 0)
        done[T - 1, :] = True
        order = []
        start = np.zeros(E, np.int64)
        for t in range(T):
            for e in np.nonzero(done[t])[0]:
                order.extend(range(start[e] * E + e, t * E + e + 1, E))
                start[e] = t + 1
        return np.asarray(order, np.int64)


def collect_rollout_(buffer: RolloutBuffer, agent: Agent, alg: PPO, env: DeviceParallelEnv):
    """collect_rollout!(rollout_buffer, agent, alg, env) -> (fps, success), rollout_buffer.jl:46-90."""
    h = env.bind(alg, agent.layer)
    h.set_params(flatten_params(agent.train_state.parameters))
    fps = _host_rollout(h, env) if isinstance(env, HostParallelEnv) else _device_array_rollout(h, env) if isinstance(env, DeviceArrayParallelEnv) else h.collect_rollout()
    buffer.observations = h.buffer(capi.BUF_OBSERVATIONS)
    acts = h.buffer(capi.BUF_ACTIONS)
    buffer.actions = acts.astype(np.int64) if h.discrete else acts  # eltype(Discrete{Int}) = Int64, spaces.jl:169
    buffer.rewards = h.buffer(capi.BUF_REWARDS)
    buffer.advantages = h.buffer(capi.BUF_ADVANTAGES)
    buffer.returns = h.buffer(capi.BUF_RETURNS)
    buffer.logprobs = h.buffer(capi.BUF_LOGPROBS)
    buffer.values = h.buffer(capi.BUF_VALUES)
    buffer.flags = h.buffer(capi.BUF_FLAGS)
    return fps, True


# --------------------------------------------------------------------------------------------
# train! (src/algorithms/ppo.jl:100-325)
# --------------------------------------------------------------------------------------------
_STAT_KEYS = ("entropy_losses", "policy_losses", "value_losses", "approx_kl_divs", "clip_fractions", "losses",
              "explained_variances", "fps", "grad_norms", "learning_rates")


def train_(agent: Agent, env: DeviceParallelEnv, alg: PPO, max_steps: int, callbacks=None, fused_update: bool = False):
    """train!(agent, env, alg, max_steps) -> (learn_stats, timer).  learn_stats has the reference's keys
    (ppo.jl:301-312); `timer` holds the TimerOutputs section names (ppo.jl:109,154,167,205-207,239) with
    wall seconds.  `callbacks`: objects with any of on_training_start / on_rollout_start / on_step / on_rollout_end / on_training_end(locals) -> bool;
    a false return stops the training and train_ returns None (ppo.jl:145-152).  An `on_step` hook routes the rollout through the step-granular
    env verbs instead of the fused kernel.  `fused_update=True` switches the bound handle to the one-launch update of the generic path
    (dril_update_fused_enable, docs/generic_update.md); where the handle cannot take it the library's message is raised."""
    cbs = list(callbacks or [])
    hook = lambda name, loc: all(getattr(c, name)(loc) for c in cbs if hasattr(c, name))   # a callback returning false stops the training (ppo.jl:145-152)
    step_hooks = [c for c in cbs if hasattr(c, "on_step")]
    timer = {}
    t0 = time.perf_counter()
    h = env.bind(alg, agent.layer)
    if fused_update:
        h.update_fused_enable(True)
    h.set_params(flatten_params(agent.train_state.parameters))
    h.set_optimizer_state(agent.train_state.optimizer_state)                                   # the TrainState owns the Adam moments (ppo.jl:52-53), not the env's handle
    per_iter = alg.n_steps * env.n_envs * h.cfg.world_size
    iterations = max_steps // per_iter  # ppo.jl:117
    timer["setup"] = time.perf_counter() - t0
    learn_stats = {k: [] for k in _STAT_KEYS}
    env.last_f32_paths = []
    env.last_monitor_stats = []
    loc = dict.fromkeys(TRAINING_START_LOCALS)                                                # the keys test/test_callbacks.jl:25-27 looks for in Base.@locals
    loc.update(agent=agent, env=env, alg=alg, iterations=iterations, total_steps=iterations * per_iter, max_steps=max_steps, n_steps=alg.n_steps,
               n_envs=env.n_envs, roll_buffer=None, total_fps=learn_stats["fps"], callbacks=cbs, learn_stats=learn_stats)
    prof0 = h.profile() if h.cfg.profile_events else None
    primary = None
    try:
        if not hook("on_training_start", loc):
            return None
        t1 = time.perf_counter()
        t_roll = t_upd = 0.0
        for i in range(iterations):
            h.set_learning_rate(alg.learning_rate)  # Optimisers.adjust!, ppo.jl:155-156
            learn_stats["learning_rates"].append(alg.learning_rate)
            loc.update(i=i + 1, learning_rate=alg.learning_rate)                              # ROLLOUT_START_LOCALS, test_callbacks.jl:36-39
            if not hook("on_rollout_start", loc):
                return None
            a = time.perf_counter()
            on_step = (lambda: all(c.on_step(loc) for c in step_hooks)) if step_hooks else None
            if isinstance(env, HostParallelEnv):
                fps = _host_rollout(h, env, on_step)
            elif isinstance(env, DeviceArrayParallelEnv):
                fps = _device_array_rollout(h, env, on_step)
            else:
                fps = _stepwise_rollout(h, env, on_step) if on_step else h.collect_rollout()  # ppo.jl:167; on_step hooks need the step-granular path
            if fps is None:
                return None                                                                   # "Collecting trajectories stopped due to callback failure", trajectory.jl:34-39
            loc.update(fps=fps)
            if not hook("on_rollout_end", loc):
                return None
            b = time.perf_counter()
            st = h.ppo_update()  # ppo.jl:188-264
            c = time.perf_counter()
            t_roll += b - a
            t_upd += c - b
            agent.steps_taken += per_iter
            agent.gradient_updates += st.n_updates
            learn_stats["fps"].append(fps)
            learn_stats["entropy_losses"].append(st.entropy_loss)
            learn_stats["policy_losses"].append(st.policy_loss)
            learn_stats["value_losses"].append(st.value_loss)
            learn_stats["approx_kl_divs"].append(st.approx_kl_div)
            learn_stats["clip_fractions"].append(st.clip_fraction)
            learn_stats["losses"].append(st.loss)
            learn_stats["explained_variances"].append(st.explained_variance)
            learn_stats["grad_norms"].append(st.grad_norm)
            if isinstance(env, DeviceArrayParallelEnv) and env.ext_monitor_window:
                env.last_monitor_stats.append(env.monitor_stats())                            # log_stats: env/ep_rew_mean, env/ep_len_mean per iteration (monitorWrapperEnv.jl:64-70)
            env.last_f32_paths.append(int(st.f32_path))                                       # per iteration: 0 default kernels, 1 redone on exact f32, 2 run directly on exact f32 (learn_stats keeps the reference's keys)
        timer["training_loop"] = time.perf_counter() - t1
        timer["collect_rollout"] = t_roll
        timer["epoch loop"] = t_upd
        timer.update(_timer_sections(h, prof0, t_upd))
        if not hook("on_training_end", loc):
            return None
        return learn_stats, timer
    except BaseException as e:
        primary = e
        raise
    finally:
        # the reference mutates agent.train_state in place at every optimiser step (ppo.jl:239), so after an early stop by a callback
        # (ppo.jl:145-152,170-176) the agent holds the partially trained weights: every exit path copies the device parameters back
        # (guarded: a device error on the way out must not mask the exception that brought us here)
        try:
            agent.train_state.parameters = unflatten_params(h.get_params(), agent.train_state.parameters)
            agent.train_state.optimizer_state = h.get_optimizer_state()
        except DrilError:
            if primary is None:
                raise


def _population_envs(what: str, envs) -> bool:
    """the env types a population's members train and evaluate on: DeviceParallelEnv of a built-in kind, or DeviceModuleEnv(path, n, fused_rollout=True) of one
    code object (the library compares the files); True for the second"""
    plugin = all(type(e) is DeviceModuleEnv for e in envs)
    for e in envs:
        if not plugin and type(e) is not DeviceParallelEnv:
            raise TypeError(f"{what}: members are DeviceParallelEnv of a built-in kind, or all of them DeviceModuleEnv(path, n, fused_rollout=True) of one code object "
                            "(host and device-array envs: one call per member)")
    return plugin


def train_population_(agents: Sequence[Agent], envs: Sequence[DeviceParallelEnv], algs: Sequence[PPO], max_steps: int, fused_update: bool = False):
    """The list form of train_: train_population_(agents, envs, algs, max_steps) -> [(learn_stats, timer), ...], one pair per agent, each equal to what
    train_(agents[i], envs[i], algs[i], max_steps) returns and leaves behind (parameters and optimiser state are copied back on every exit path) — but every
    iteration of all agents is one batched rollout launch and one batched update launch (Population, docs/population.md).  The envs are DeviceParallelEnv of one
    built-in kind and shape; the algs may differ in everything the kernels take at run time (learning rate, gamma, clip ranges, coefficients, target_kl, ...).
    Device env plug-ins: a list of DeviceModuleEnv(path, n, fused_rollout=True) of ONE code object built with DRIL_ENV_PLUGIN_ROLLOUT_POP and one shape;
    `fused_update=True` switches each bound handle to the one-launch update as train_ does (dril_update_fused_enable) — a plug-in member needs both opt-ins, and
    without them the library's refusal is raised (docs/population.md, "Plug-in members").
    Callbacks are out of scope here: hooks observe and steer one agent's loop step by step, so per-member train_ remains the way to use them.  `timer` holds the
    wall seconds of the whole population (the members share every launch)."""
    agents, envs, algs = list(agents), list(envs), list(algs)
    if not agents:
        raise ValueError("train_population_: empty population")
    if not (len(agents) == len(envs) == len(algs)):
        raise ValueError(f"train_population_: {len(agents)} agents, {len(envs)} envs and {len(algs)} algs: one of each per member")
    _population_envs("train_population_", envs)
    t0 = time.perf_counter()
    handles = []
    for agent, env, alg in zip(agents, envs, algs):
        h = env.bind(alg, agent.layer)
        if fused_update:
            h.update_fused_enable(True)
        h.set_params(flatten_params(agent.train_state.parameters))
        h.set_optimizer_state(agent.train_state.optimizer_state)
        handles.append(h)
    per_iter = algs[0].n_steps * envs[0].n_envs
    results = [({k: [] for k in _STAT_KEYS}, {}) for _ in agents]
    for env in envs:
        env.last_f32_paths = []
        env.last_monitor_stats = []
    primary = None
    try:
        with Population(handles) as pop:
            t_setup = time.perf_counter() - t0
            t1 = time.perf_counter()
            t_roll = t_upd = 0.0
            for _ in range(max_steps // per_iter):  # ppo.jl:117
                for h, alg, (ls, _t) in zip(handles, algs, results):
                    h.set_learning_rate(alg.learning_rate)  # Optimisers.adjust!, ppo.jl:155-156
                    ls["learning_rates"].append(alg.learning_rate)
                a = time.perf_counter()
                fps = pop.collect_rollout()  # ppo.jl:167
                b = time.perf_counter()
                sts = pop.ppo_update()  # ppo.jl:188-264
                c = time.perf_counter()
                t_roll += b - a
                t_upd += c - b
                for agent, env, f, st, (ls, _t) in zip(agents, envs, fps, sts, results):
                    agent.steps_taken += per_iter
                    agent.gradient_updates += st.n_updates
                    ls["fps"].append(f)
                    ls["entropy_losses"].append(st.entropy_loss)
                    ls["policy_losses"].append(st.policy_loss)
                    ls["value_losses"].append(st.value_loss)
                    ls["approx_kl_divs"].append(st.approx_kl_div)
                    ls["clip_fractions"].append(st.clip_fraction)
                    ls["losses"].append(st.loss)
                    ls["explained_variances"].append(st.explained_variance)
                    ls["grad_norms"].append(st.grad_norm)
                    env.last_f32_paths.append(int(st.f32_path))
            for _ls, timer in results:
                timer.update({"setup": t_setup, "training_loop": time.perf_counter() - t1, "collect_rollout": t_roll, "epoch loop": t_upd,
                              "batch loop": t_upd, "compute_gradients": float("nan"), "apply_gradients": float("nan")})
        return results
    except BaseException as e:
        primary = e
        raise
    finally:
        for agent, h in zip(agents, handles):   # as train_: every exit path copies the device parameters back
            try:
                agent.train_state.parameters = unflatten_params(h.get_params(), agent.train_state.parameters)
                agent.train_state.optimizer_state = h.get_optimizer_state()
            except DrilError:
                if primary is None:
                    raise


# keys of Base.@locals the reference's callback test reads (test/test_callbacks.jl:25-27 at training start, :36-39 at rollout start);
# the Julia shim builds its Dict from the same two lists (tools/check_shim.py asserts that they cannot drift)
TRAINING_START_LOCALS = ("agent", "env", "alg", "iterations", "total_steps", "max_steps", "n_steps", "n_envs", "roll_buffer", "total_fps", "callbacks", "learn_stats")
ROLLOUT_START_LOCALS = ("i", "learning_rate")
# TimerOutputs sections of the reference's train! (ppo.jl:109,154,167,205-207,239) and the device timings that fill them
TIMER_SECTIONS = ("setup", "training_loop", "collect_rollout", "epoch loop", "batch loop", "compute_gradients", "apply_gradients")


def _timer_sections(h: Handle, prof0, t_upd: float) -> dict:
    """"batch loop" / "compute_gradients" / "apply_gradients" (ppo.jl:206-207,239): with cfg.profile_events the HIP-event totals of the kernels that
    stand in for them (dril_profile_get); without, only the enclosing wall time is known and the three sections report it as an upper bound"""
    if prof0 is None:
        return {"batch loop": t_upd, "compute_gradients": float("nan"), "apply_gradients": float("nan")}
    p1 = h.profile()
    ms = lambda *names: sum(p1[n]["total_ms"] - prof0[n]["total_ms"] for n in names) * 1e-3
    grad = ms("adv_moments_kernel", "ppo_grad_kernel", "grad_reduce_kernel", "ncclAllReduce")
    apply = ms("adam_kernel")
    return {"batch loop": grad + apply, "compute_gradients": grad, "apply_gradients": apply}


def evaluate_agent(agent: Agent, env: DeviceParallelEnv, n_eval_episodes: int = 10, deterministic: bool = True,
                   reward_threshold: Optional[float] = None, return_stats: bool = True, isolated: bool = False, persistent: bool = False):
    """evaluate_agent(agent, env; ...) (src/evaluation.jl:54-143).  isolated=True (device envs): the evaluation runs on the device and leaves the env as it was —
    state, counters, the monitor's window, a normaliser's statistics (frozen for the call) — so it may sit between two training iterations
    (Handle.evaluate_agent_device, docs/evaluation.md); the default resets the env and lets its episodes enter the monitor's window, as before.
    persistent=True (with isolated=True) asks for the persistent evaluate kernel wherever it can run, normalised envs included; the numbers are the same."""
    h = env.bind(agent.alg, agent.layer)
    h.set_params(flatten_params(agent.train_state.parameters))
    if isolated and isinstance(env, (HostParallelEnv, DeviceArrayParallelEnv)):
        raise NotImplementedError("evaluate_agent(isolated=True): host envs (HostParallelEnv) live with the caller, who keeps a second set of envs for evaluation; the device verb steps device envs")
    if isinstance(env, HostParallelEnv):       # the reference loop on the caller's envs, predict_actions on the device (evaluation.jl:86-125)
        asp = env.action_space()
        er, el = [], []
        cur_r, cur_l = np.zeros(env.n_envs, np.float32), np.zeros(env.n_envs, np.int64)
        env.reset_()
        obs = np.stack(env.observe())
        while len(er) < n_eval_episodes:
            raw = h.predict_actions(obs, deterministic)
            acts = list(raw) if h.discrete else [np.clip(a, np.asarray(asp.low, np.float32), np.asarray(asp.high, np.float32)).reshape(asp.shape) for a in raw]
            rew, term, trunc, _ = env.act_(acts)
            cur_r += rew; cur_l += 1
            obs = np.stack(env.observe())
            for i in np.nonzero(term | trunc)[0]:
                if len(er) < n_eval_episodes:
                    er.append(float(cur_r[i])); el.append(int(cur_l[i]))
                    cur_r[i] = 0; cur_l[i] = 0
        er, el = np.asarray(er, np.float32), np.asarray(el, np.int64)
        sd = lambda x: float(np.std(x, ddof=1)) if len(x) > 1 else float("nan")
        stats = {"mean_reward": float(er.mean()), "std_reward": sd(er), "mean_length": float(el.mean()), "std_length": sd(el)}
    elif isinstance(env, DeviceArrayParallelEnv):   # the same loop; observations and actions stay on the device, only rewards and flags (E values each) come to the host for the accounting
        er, el = [], []
        cur_r, cur_l = np.zeros(env.n_envs, np.float32), np.zeros(env.n_envs, np.int64)
        env.reset_()
        obs = env.observe()
        _, ea = env.action_arrays(h, obs)
        while len(er) < n_eval_episodes:
            h.predict_actions_device(obs, deterministic, None, ea, env.stream)
            rew, term, trunc, _ = env.act_(ea)
            obs = env.observe()
            rew, done = _to_host(rew, env.stream), _to_host(term, env.stream).astype(bool) | _to_host(trunc, env.stream).astype(bool)
            cur_r += rew; cur_l += 1
            for i in np.nonzero(done)[0]:
                if len(er) < n_eval_episodes:
                    er.append(float(cur_r[i])); el.append(int(cur_l[i]))
                    cur_r[i] = 0; cur_l[i] = 0
        er, el = np.asarray(er, np.float32), np.asarray(el, np.int64)
        sd = lambda x: float(np.std(x, ddof=1)) if len(x) > 1 else float("nan")
        stats = {"mean_reward": float(er.mean()), "std_reward": sd(er), "mean_length": float(el.mean()), "std_length": sd(el)}
    elif isolated:
        stats, er, el, _ = h.evaluate_agent_device(n_eval_episodes, deterministic, persistent=persistent)
    else:
        stats, er, el = h.evaluate_agent(n_eval_episodes, deterministic)
    if reward_threshold is not None and stats["mean_reward"] < reward_threshold:
        raise RuntimeError(f"Mean reward below threshold: {stats['mean_reward']:.2f} < {reward_threshold}")   # evaluation.jl:131-135
    return {k: stats[k] for k in ("mean_reward", "std_reward", "mean_length", "std_length")} if return_stats else (er, el)


def evaluate_population(agents: Sequence[Agent], envs: Sequence[DeviceParallelEnv], n_eval_episodes: int = 10, deterministic: bool = True, seed: Optional[int] = None,
                        population: Optional[Population] = None) -> list:
    """The list form of evaluate_agent(agent, env, isolated=True): one stats dict per agent (the keys of evaluate_agent(..., return_stats=True)), each equal to what
    the per-agent call returns, with one batched launch and one look per K env steps for all of them (Population.evaluate, docs/population.md "Evaluation"); the
    envs are left as they were (plug-in members — DeviceModuleEnv, as train_population_ takes them — are evaluated one by one inside the call).  Each env is bound as train_population_ binds it.  The handles are joined into a population for the call; handles that already are
    joined are evaluated through the population the caller passes as `population=` (its members, in the order of `agents`).  seed=None: every env's own seed."""
    agents, envs = list(agents), list(envs)
    if not agents:
        raise ValueError("evaluate_population: empty population")
    if len(agents) != len(envs):
        raise ValueError(f"evaluate_population: {len(agents)} agents and {len(envs)} envs: one of each per member")
    _population_envs("evaluate_population", envs)
    handles = []
    for agent, env in zip(agents, envs):
        h = env.bind(agent.alg, agent.layer)
        h.set_params(flatten_params(agent.train_state.parameters))
        handles.append(h)
    if population is not None:
        if len(population.handles) != len(handles) or any(a is not b for a, b in zip(population.handles, handles)):
            raise ValueError("evaluate_population: population= must hold exactly the handles of `envs`, in the same order")
        res = population.evaluate(n_eval_episodes, deterministic, seed)
    else:
        with Population(handles) as pop:
            res = pop.evaluate(n_eval_episodes, deterministic, seed)
    return [{k: stats[k] for k in ("mean_reward", "std_reward", "mean_length", "std_length")} for stats, _er, _el, _info in res]


def _collect_trajectory(agent: Agent, env: DeviceParallelEnv, max_steps: Optional[int] = None, norm_env=None, deterministic: bool = True,
                        n_trajectories: int = 1, seed: Optional[int] = None, persistent: bool = False):
    """collect_trajectory(agent, env; max_steps, norm_env, deterministic) (src/utils/trajectory_utils.jl:3-49) -> (observations, actions, rewards): the original
    observations (L + 1 of them, the last one the terminal state), the env actions and the raw rewards of one episode; n_trajectories > 1: a list of such triples,
    envs 0..n-1 of the parallel env, each its first episode after the reset.  Runs on the device and leaves the env as it was (Handle.collect_trajectory_device,
    docs/evaluation.md); persistent=True asks for its one-launch form where the persistent evaluate kernel can run.  norm_env: None, or `env` itself — a NormalizeWrapperEnv around the device env is a mode of its handle, found there and applied frozen."""
    if isinstance(env, (HostParallelEnv, DeviceArrayParallelEnv)):
        raise NotImplementedError("collect_trajectory: host envs (HostParallelEnv, DeviceArrayParallelEnv) live with the caller; the device verb steps device envs")
    if norm_env is not None and norm_env is not env:
        raise NotImplementedError("collect_trajectory: norm_env is None or the env itself (NormalizeWrapperEnv around a device env is a mode of the env's handle and is applied frozen)")
    h = env.bind(agent.alg, agent.layer)
    h.set_params(flatten_params(agent.train_state.parameters))
    trajs, _, flags, _ = h.collect_trajectory_device(n_trajectories, max_steps, deterministic, seed, persistent=persistent)
    if (flags & capi.TRAJ_MAX_STEPS).any():
        warnings.warn("Max steps reached")                                           # trajectory_utils.jl:39
    return trajs[0] if n_trajectories == 1 else trajs


@_opt_in_persistent(_collect_trajectory)
def collect_trajectory(agent: Agent, env: DeviceParallelEnv, max_steps: Optional[int] = None, norm_env=None, deterministic: bool = True,
                       n_trajectories: int = 1, seed: Optional[int] = None):
    """_collect_trajectory with the keyword-only option `persistent` (default False): collect_trajectory(agent, env, ..., persistent=True)."""


def get_action_and_values(agent: Agent, env: DeviceParallelEnv, observations):
    """get_action_and_values(agent, observations) -> (actions, values, logprobs), agent_methods.jl:19-35."""
    h = env.bind(agent.alg, agent.layer)
    h.set_params(flatten_params(agent.train_state.parameters))
    return h.policy_forward(np.stack(observations))


def predict_values(agent: Agent, env: DeviceParallelEnv, observations):
    """predict_values(agent, observations), agent_methods.jl:49-64."""
    h = env.bind(agent.alg, agent.layer)
    h.set_params(flatten_params(agent.train_state.parameters))
    return h.predict_values(np.stack(observations))
