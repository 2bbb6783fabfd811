"""Host-side mirror of the reference's SAC interface (src/algorithms/sac.jl) over the C ABI of include/dril_sac.h.

    SAC, AutoEntropyCoefficient, FixedEntropyCoefficient        sac.jl:25-36, src/interfaces/entropy.jl
    SACLayer(obs_space, act_space; hidden_dims=[512,512], ...)  sac.jl:72-85  (ContinuousActorCriticLayer{QCritic})
    SACAgent(layer, alg)                                        sac.jl:160-188
    ReplayBuffer(obs_space, act_space, capacity)                src/buffers/replay_buffer.jl
    sac_train_(agent, env, alg, max_steps)                      sac.jl:406-549  ->  (agent, replay_buffer, training_stats, timer)

`SacHandle` types one dril_sac_handle* of libdril_hip.so — there is no fallback and no way to point it elsewhere; the parity tests drive the
CPU oracle ("orc_sac_" symbols, same signatures) through a subclass that lives in tests/oracle_lib.py.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import time
import warnings
from dataclasses import dataclass, field, replace
from typing import Optional, Sequence

import numpy as np

from . import _capi as capi, _normalize
from ._capi import DrilSacConfig, DrilSacStats
from .host import Box, DeviceArrayParallelEnv, DrilError, HostParallelEnv, PendulumEnv, ScalingWrapperEnv, _dev_ptr, _orthogonal, _stream_ptr, _to_host


# --------------------------------------------------------------------------------------------
# algorithm + layer (host-side data only)
# --------------------------------------------------------------------------------------------
@dataclass
class AutoEntropyCoefficient:
    """entropy.jl:21-24; target None = AutoEntropyTarget (-dim(action_space), sac.jl:47-57)"""
    target: Optional[float] = None
    initial_value: float = 1.0


@dataclass
class FixedEntropyCoefficient:
    coef: float = 0.2


@dataclass
class SAC:
    """SAC(; ...) sac.jl:25-36"""
    learning_rate: float = 3e-4
    buffer_capacity: int = 1_000_000
    start_steps: int = 100
    batch_size: int = 256
    tau: float = 0.005
    gamma: float = 0.99
    train_freq: int = 1
    gradient_steps: int = 1
    ent_coef: object = field(default_factory=AutoEntropyCoefficient)
    target_update_interval: int = 1


def get_gradient_steps(alg: SAC, train_freq: Optional[int] = None, n_envs: int = 1) -> int:
    """sac.jl:59-65"""
    tf = alg.train_freq if train_freq is None else train_freq
    return tf * n_envs if alg.gradient_steps == -1 else alg.gradient_steps


@dataclass
class SACLayer:
    """SACLayer(observation_space, action_space; log_std_init=-3, hidden_dims=[512,512], activation=relu) sac.jl:72-85:
    ContinuousActorCriticLayer with critic_type = QCritic() (n_critics = 2) and separate features."""
    observation_space: Box
    action_space: Box
    hidden_dims: Sequence[int] = (512, 512)
    log_std_init: float = -3.0
    activation: str = "relu"

    @property
    def obs_dim(self) -> int:
        return len(self.observation_space.low)

    @property
    def act_dim(self) -> int:
        return len(self.action_space.low)

    def q_parameterlength(self) -> int:
        d, a, (h1, h2) = self.obs_dim, self.act_dim, self.hidden_dims
        return (d + a) * h1 + h1 + h1 * h2 + h2 + h2 + 1

    def parameterlength(self) -> int:
        d, a, (h1, h2) = self.obs_dim, self.act_dim, self.hidden_dims
        return d * h1 + h1 + h1 * h2 + h2 + h2 * a + a + 2 * self.q_parameterlength() + a

    def initialparameters(self, rng: np.random.Generator) -> dict:
        """orthogonal gains sqrt(2) hidden / 0.01 actor output / 1.0 Q output, zero bias (layer_constructors.jl:16-20);
        critic_head = Lux.Parallel(vcat, mlp, mlp) -> layer_1 / layer_2 (layer_helpers.jl:100-112)"""
        d, a, (h1, h2) = self.obs_dim, self.act_dim, self.hidden_dims

        def mlp(inp, out, gain):
            return {"layer_1": {"weight": _orthogonal(rng, h1, inp, math.sqrt(2.0)), "bias": np.zeros(h1, np.float32)},
                    "layer_2": {"weight": _orthogonal(rng, h2, h1, math.sqrt(2.0)), "bias": np.zeros(h2, np.float32)},
                    "layer_3": {"weight": _orthogonal(rng, out, h2, gain), "bias": np.zeros(out, np.float32)}}

        return {"actor_head": mlp(d, a, 0.01), "critic_head": {"layer_1": mlp(d + a, 1, 1.0), "layer_2": mlp(d + a, 1, 1.0)},
                "log_std": np.full(a, self.log_std_init, np.float32)}


def _mlp_flat(m: dict):
    for l in ("layer_1", "layer_2", "layer_3"):
        yield np.asarray(m[l]["weight"], np.float32).ravel(order="F")
        yield np.asarray(m[l]["bias"], np.float32).ravel()


def sac_flatten_params(ps: dict) -> np.ndarray:
    """Lux NamedTuple -> the flat layout of dril_sac_set_params"""
    parts = list(_mlp_flat(ps["actor_head"])) + list(_mlp_flat(ps["critic_head"]["layer_1"])) + list(_mlp_flat(ps["critic_head"]["layer_2"]))
    parts.append(np.asarray(ps["log_std"], np.float32).ravel())
    return np.concatenate(parts)


def sac_unflatten_params(flat: np.ndarray, like: dict) -> dict:
    off = 0

    def mlp(m):
        nonlocal off
        out = {}
        for l in ("layer_1", "layer_2", "layer_3"):
            w, b = m[l]["weight"], m[l]["bias"]
            out[l] = {"weight": flat[off:off + w.size].reshape(w.shape, order="F").copy()}
            off += w.size
            out[l]["bias"] = flat[off:off + b.size].copy()
            off += b.size
        return out

    ps = {"actor_head": mlp(like["actor_head"])}
    ps["critic_head"] = {"layer_1": mlp(like["critic_head"]["layer_1"]), "layer_2": mlp(like["critic_head"]["layer_2"])}
    ps["log_std"] = flat[off:off + like["log_std"].size].copy()
    return ps


def make_sac_config(env, n_envs: int, alg: SAC, layer: SACLayer, *, seed: int = 42, device: int = 0,
                    profile_events: bool = False, per_dim_bounds: bool = False) -> DrilSacConfig:
    """`env`: one env of a DeviceParallelEnv (`.env`), a HostParallelEnv, or a device env plug-in (a DeviceModuleEnv or its ModuleEnv: the spaces and the Box
    bounds per dimension are the code object's, the handle is made with SacHandle(cfg, env_module=path))"""
    if getattr(env, "kind", None) is None and getattr(getattr(env, "env", None), "kind", None) == capi.ENV_MODULE:
        env = env.env                                     # a DeviceModuleEnv: its ModuleEnv
    external, module = getattr(env, "kind", None) == capi.ENV_EXTERNAL, getattr(env, "kind", None) == capi.ENV_MODULE
    if module:
        if env.info["discrete"]:
            raise NotImplementedError(f"SAC needs a Box action space (sac.jl:74): the device env plug-in {env.info['name']!r} is Discrete")
        asp = env.action_space()
        if len(asp.low) != layer.act_dim or env.info["obs_dim"] != layer.obs_dim:
            raise ValueError(f"SACLayer is ({layer.obs_dim} obs, {layer.act_dim} action dims), the plug-in {env.info['name']!r} ({env.info['obs_dim']}, {len(asp.low)})")
    if not external and not module and getattr(env, "kind", None) not in (capi.ENV_PENDULUM, capi.ENV_PENDULUM_SCALED, capi.ENV_MOUNTAINCAR_CONTINUOUS, capi.ENV_MOUNTAINCAR_CONTINUOUS_SCALED):
        raise NotImplementedError("SAC needs a Box action space (sac.jl:74); the device envs with one are Pendulum-v1 (optionally under ScalingWrapperEnv), MountainCarContinuous-v0 and Box device env plug-ins (DeviceModuleEnv)")
    c = DrilSacConfig()
    c.abi_version = capi.SAC_ABI_VERSION
    c.env_kind, c.n_envs, c.episode_len = env.kind, n_envs, getattr(env, "max_steps", 0)
    if external:     # host envs: the spaces travel in the config (include/dril_sac.h)
        osp, asp = env.observation_space(), env.action_space()
        lo, hi = np.unique(np.asarray(asp.low, np.float32)), np.unique(np.asarray(asp.high, np.float32))
        if (lo.size != 1 or hi.size != 1) and not per_dim_bounds:
            raise NotImplementedError("DRIL_ENV_EXTERNAL SAC: one (low, high) pair for all action dimensions (wrap the env in a ScalingWrapperEnv-style Box(-1, 1))")
        # per_dim_bounds: the caller hands the Box per dimension to SacHandle.ext_set_action_bounds right after create; the config carries the enclosing pair
        c.ext_obs_dim, c.ext_action_dim, c.ext_action_low, c.ext_action_high = len(osp.low), len(asp.low), float(lo[0]), float(hi[-1])
    c.hidden1, c.hidden2 = layer.hidden_dims
    c.activation = {"tanh": 0, "relu": 1}[layer.activation]
    c.buffer_capacity, c.start_steps, c.batch_size = alg.buffer_capacity, alg.start_steps, alg.batch_size
    c.tau, c.gamma = alg.tau, alg.gamma
    c.train_freq, c.gradient_steps, c.target_update_interval = alg.train_freq, alg.gradient_steps, alg.target_update_interval
    if isinstance(alg.ent_coef, AutoEntropyCoefficient):
        c.auto_ent_coef, c.ent_coef_init = 1, alg.ent_coef.initial_value
        c.auto_target_entropy = int(alg.ent_coef.target is None)
        c.target_entropy = 0.0 if alg.ent_coef.target is None else alg.ent_coef.target
    else:
        c.auto_ent_coef, c.ent_coef_init, c.auto_target_entropy, c.target_entropy = 0, alg.ent_coef.coef, 1, 0.0
    c.learning_rate, c.adam_beta1, c.adam_beta2, c.adam_eps = alg.learning_rate, 0.9, 0.999, 1e-8
    c.seed, c.device, c.profile_events = seed, device, int(profile_events)
    return c


# --------------------------------------------------------------------------------------------
# typed wrapper of one dril_sac_handle*
# --------------------------------------------------------------------------------------------
@_normalize.normalize_verbs(lambda self, verb: self._f(("normalize_" if verb == "config_default" else "ext_normalize_") + verb), "normalize_", "ext_")
@_normalize.normalize_verbs(lambda self, verb: self._f("normalize_" + verb), "norm_")
class SacHandle:
    """typed wrapper of one dril_sac_handle* of libdril_hip.so (there is no other backend: the CPU oracle is driven by a subclass that lives under tests/)"""
    _PREFIX = "dril_sac_"

    @classmethod
    def _load(cls) -> C.CDLL:
        return capi.load_library()

    def __init__(self, cfg: DrilSacConfig, env_module: Optional[os.PathLike] = None):
        self.lib = self._load()
        self.prefix = self._PREFIX
        prefix = self.prefix
        self.cfg = cfg
        self._h = C.c_void_p()
        if env_module is not None:      # cfg.env_kind == ENV_MODULE: the env is a code object built from include/device/dril_env_plugin.h
            rc = self._f("create_with_env_module")(C.byref(cfg), os.fsencode(env_module), C.byref(self._h))
        else:
            rc = self._f("create")(C.byref(cfg), C.byref(self._h))
        if rc != capi.OK:
            le = getattr(self.lib, prefix + "last_error", None)
            raise DrilError(rc, (le(None) or b"").decode() if le else "create failed")
        self.D, self.A = self._f("obs_dim")(self._h), self._f("action_dim")(self._h)
        self.P, self.Pq = int(self._f("param_count")(self._h)), int(self._f("q_param_count")(self._h))
        self.E, self.B = cfg.n_envs, cfg.batch_size

    def _f(self, name):
        return getattr(self.lib, self.prefix + name)

    def env_module_obs_space(self) -> dict:
        """dril_sac_env_module_obs_space_of: the observation space the plug-in declares"""
        lo, hi, decl = np.empty(self.D, np.float32), np.empty(self.D, np.float32), C.c_int32()
        self._chk(self._f("env_module_obs_space_of")(self._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), C.byref(decl)))
        return dict(low=lo, high=hi, declared=bool(decl.value))

    def scaling_enable(self, on: bool = True):
        """dril_sac_scaling_enable: ScalingWrapperEnv around every env of a plug-in handle; between create and the first env_reset"""
        self._chk(self._f("scaling_enable")(self._h, int(bool(on))))

    def agent_spaces(self) -> dict:
        """dril_sac_agent_spaces: the spaces the agent and its adapters see (Box(-1, 1) throughout under ScalingWrapperEnv)"""
        from .host import _agent_spaces
        rc, d = _agent_spaces(self._f("agent_spaces"), self._h, self.D, self.A)
        self._chk(rc)
        return d

    def env_module_info(self) -> dict:
        """dril_sac_env_module_info_of: spaces and bounds of the plug-in behind this handle"""
        from .host import _module_info_dict
        info = capi.DrilEnvModuleInfo()
        self._chk(self._f("env_module_info_of")(self._h, C.byref(info)))
        return _module_info_dict(info)

    def close(self):
        if self._h:
            self._f("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != capi.OK:
            le = getattr(self.lib, self.prefix + "last_error", None)
            raise DrilError(rc, (le(self._h) or b"").decode() if le else f"status {rc}")

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    @staticmethod
    def _f32(a):
        return None if a is None else np.ascontiguousarray(a, np.float32)

    # parameters
    def set_params(self, flat):
        flat = self._f32(flat)
        self._chk(self._f("set_params")(self._h, self._p(flat), flat.size))

    def get_params(self) -> np.ndarray:
        out = np.empty(self.P, np.float32)
        self._chk(self._f("get_params")(self._h, self._p(out), out.size))
        return out

    def get_target_params(self) -> np.ndarray:
        out = np.empty(2 * self.Pq, np.float32)
        self._chk(self._f("get_target_params")(self._h, self._p(out), out.size))
        return out

    def set_target_params(self, flat):
        flat = self._f32(flat)
        self._chk(self._f("set_target_params")(self._h, self._p(flat), flat.size))

    def get_log_ent_coef(self) -> float:
        v = C.c_float()
        self._chk(self._f("get_log_ent_coef")(self._h, C.byref(v)))
        return v.value

    def set_log_ent_coef(self, v: float):
        self._chk(self._f("set_log_ent_coef")(self._h, v))

    def reset_optimizer(self):
        self._chk(self._f("reset_optimizer")(self._h))

    # env
    def env_reset(self, seed: int):
        self._chk(self._f("env_reset")(self._h, seed))

    def env_observe(self) -> np.ndarray:
        out = np.empty((self.E, self.D), np.float32)
        self._chk(self._f("env_observe")(self._h, self._p(out)))
        return out

    # layer calls; arrays are (batch, features) row-major == (features x batch) column-major
    def action_log_prob(self, obs, noise=None):
        obs, noise = self._f32(obs), self._f32(noise)
        B = obs.shape[0]
        a, lp = np.empty((B, self.A), np.float32), np.empty(B, np.float32)
        self._chk(self._f("action_log_prob")(self._h, self._p(obs), B, self._p(noise), self._p(a), self._p(lp)))
        return a, lp

    def predict_actions(self, obs, deterministic=False, noise=None):
        obs, noise = self._f32(obs), self._f32(noise)
        B = obs.shape[0]
        raw, env = np.empty((B, self.A), np.float32), np.empty((B, self.A), np.float32)
        self._chk(self._f("predict_actions")(self._h, self._p(obs), B, int(deterministic), self._p(noise), self._p(raw), self._p(env)))
        return raw, env

    def predict_q(self, obs, actions, use_target=False):
        obs, actions = self._f32(obs), self._f32(actions)
        B = obs.shape[0]
        q = np.empty((B, 2), np.float32)
        self._chk(self._f("predict_q")(self._h, self._p(obs), self._p(actions), B, int(use_target), self._p(q)))
        return q

    # collection + replay
    def collect_rollout(self, n_steps: int, use_random_actions: bool = False) -> float:
        fps = C.c_double()
        self._chk(self._f("collect_rollout")(self._h, n_steps, int(use_random_actions), C.byref(fps)))
        return fps.value

    def collect_continue(self, n_steps: int = 1, use_random_actions: bool = False) -> float:
        """dril_sac_collect_continue: further steps of the collection the previous collect call left off (host code between the env steps of ONE
        collect_trajectories: on_step callbacks) — under NormalizeWrapperEnv without the observe a collection begins with"""
        fps = C.c_double()
        self._chk(self._f("collect_continue")(self._h, n_steps, int(use_random_actions), C.byref(fps)))
        return fps.value

    def ext_push(self, obs, stored_actions, rewards, terminated, truncated, next_obs, terminal_obs=None):
        """one env step of the caller's host envs into the replay ring (DRIL_ENV_EXTERNAL)"""
        o, a, r, n = self._f32(obs), self._f32(stored_actions), self._f32(rewards), self._f32(next_obs)
        te, tr = np.ascontiguousarray(terminated, np.uint8), np.ascontiguousarray(truncated, np.uint8)
        to = None if terminal_obs is None else self._f32(terminal_obs)
        self._chk(self._f("ext_push")(self._h, self._p(o), self._p(a), self._p(r), self._p(te), self._p(tr), self._p(n), self._p(to)))

    # the same loop over DEVICE arrays (dril_sac_ext_*_device, docs/sac.md last section): integers (raw device pointers) or objects with __cuda_array_interface__
    # (torch-ROCm tensors, CuPy arrays); nothing is copied or allocated here, and none of act / push / predict / update_enqueue waits on the host
    discrete = False                                                                  # SAC needs a Box: what DeviceArrayParallelEnv.action_arrays asks of a handle

    def ext_act_device(self, obs, use_random_actions: bool = False, noise=None, stored_actions=None, env_actions=None, stream=None):
        """obs (E, D) f32 on the device; noise (E, A) f32 standard normals (uniforms in [0, 1) for random actions) or None = the handle's stream;
        stored_actions / env_actions: device OUTPUT arrays (E, A) f32, either may be None.  The outputs are ready for work enqueued on `stream` afterwards"""
        args = (_dev_ptr("obs", obs, (self.E, self.D), "float32"), int(bool(use_random_actions)), _dev_ptr("noise", noise, (self.E, self.A), "float32", True),
                _dev_ptr("stored_actions", stored_actions, (self.E, self.A), "float32", True), _dev_ptr("env_actions", env_actions, (self.E, self.A), "float32", True))
        self._chk(self._f("ext_act_device")(self._h, *args, _stream_ptr(stream)))

    def ext_push_device(self, rewards, terminated, truncated, next_obs, terminal_obs=None, stream=None):
        """rewards f32 (E,), terminated / truncated u8 or bool (E,), next_obs f32 (E, D), terminal_obs f32 (E, D) or None = no env was truncated in this step"""
        args = (_dev_ptr("rewards", rewards, (self.E,), "float32"), _dev_ptr("terminated", terminated, (self.E,), "uint8"), _dev_ptr("truncated", truncated, (self.E,), "uint8"),
                _dev_ptr("next_obs", next_obs, (self.E, self.D), "float32"), _dev_ptr("terminal_obs", terminal_obs, (self.E, self.D), "float32", True))
        self._chk(self._f("ext_push_device")(self._h, *args, _stream_ptr(stream)))

    def predict_actions_device(self, obs, deterministic: bool = False, noise=None, raw_actions=None, env_actions=None, stream=None, batch: Optional[int] = None):
        """dril_sac_predict_actions on device arrays; `batch` is read from obs's shape (B, D) unless obs is a raw pointer"""
        if batch is None:
            cai = getattr(obs, "__cuda_array_interface__", None)
            if cai is None or len(cai["shape"]) != 2:
                raise ValueError("obs: expected a device array of shape (batch, obs_dim), or a raw pointer together with batch=")
            batch = int(cai["shape"][0])
        if raw_actions is None and env_actions is None:
            raise ValueError("raw_actions / env_actions: at least one device output array is needed")
        args = (_dev_ptr("obs", obs, (batch, self.D), "float32"), batch, int(bool(deterministic)), _dev_ptr("noise", noise, (batch, self.A), "float32", True),
                _dev_ptr("raw_actions", raw_actions, (batch, self.A), "float32", True), _dev_ptr("env_actions", env_actions, (batch, self.A), "float32", True))
        self._chk(self._f("predict_actions_device")(self._h, *args, _stream_ptr(stream)))

    def update_enqueue(self, n_updates: int = 1):
        """the launches of update(n_updates), no wait; the statistics rows wait in the pending table for flush()"""
        self._chk(self._f("update_enqueue")(self._h, n_updates))

    def flush(self) -> list:
        """the one drain: -> the pending statistics rows in order.  The sticky error of ext_push_device (truncated envs without terminal_obs) is raised as a
        DrilError whose `stats` attribute carries the rows this flush took out of the table: the library has emptied it, they would be lost otherwise"""
        cap = capi.SAC_PENDING_CAPACITY
        out, n = (DrilSacStats * cap)(), C.c_int64(0)
        rc = self._f("flush")(self._h, C.cast(out, C.c_void_p), cap, C.byref(n))
        rows = list(out[:n.value])
        try:
            self._chk(rc)
        except DrilError as e:
            e.stats = rows
            raise
        return rows

    def ext_set_action_bounds(self, low, high):
        """the Box per action dimension for TanhScaleAdapter and rand(action_space) on an external handle (host arrays of A floats)"""
        if low is None or high is None:
            raise ValueError("low / high: None, expected action_dim floats each")
        lo, hi = np.ascontiguousarray(low, np.float32).ravel(), np.ascontiguousarray(high, np.float32).ravel()
        if lo.size != self.A or hi.size != self.A:
            raise ValueError(f"low / high: {lo.size} / {hi.size} values where action_dim = {self.A} are expected")
        self._chk(self._f("ext_set_action_bounds")(self._h, self._p(lo), self._p(hi)))

    def ext_device_info(self) -> dict:
        info = capi.DrilSacExtDeviceInfo()
        self._chk(self._f("ext_device_info")(self._h, C.byref(info)))
        return dict(steps_device=int(info.steps_device), steps_host=int(info.steps_host), host_syncs=int(info.host_syncs), flushes=int(info.flushes), launches=int(info.launches),
                    pending_updates=int(info.pending_updates), pending_capacity=int(info.pending_capacity), per_dim_bounds=bool(info.per_dim_bounds))

    # NormalizeWrapperEnv / MonitorWrapperEnv around device-resident external envs (dril_sac_ext_normalize_* / dril_sac_ext_monitor_*, docs/sac.md last section), under
    # the names of the PPO handle: ext_normalize_enable, ext_normalize_config, ext_normalize_set_training, ext_normalize_get_stats / _set_stats / _get_original /
    # _get_returns come from _normalize.normalize_verbs
    def ext_normalize_reset(self, stream=None):
        """the wrapper's half of reset!: returns <- 0, statistics kept; enqueued, no host wait"""
        self._chk(self._f("ext_normalize_reset")(self._h, _stream_ptr(stream)))

    def ext_collection_begin(self):
        """the next ext_act_device is the opening observe(env) of a collect_trajectories call (a host flag; a no-op while the normaliser is off)"""
        self._chk(self._f("ext_collection_begin")(self._h))

    def ext_monitor_enable(self, stats_window: int):
        """MonitorWrapperEnv(env, stats_window) around the handle's device-resident envs; 0 switches it off"""
        self._chk(self._f("ext_monitor_enable")(self._h, int(stats_window)))

    def ext_monitor_stats(self):
        """(ep_rew_mean, ep_len_mean, n_episodes) of the window (log_stats, monitorWrapperEnv.jl:64-70); the means are nan while it is empty.  Drains the stream"""
        r, l, n = C.c_float(float("nan")), C.c_float(float("nan")), C.c_int32()
        self._chk(self._f("ext_monitor_get_stats")(self._h, C.byref(r), C.byref(l), C.byref(n)))
        return r.value, l.value, n.value

    def ext_wrap_info(self) -> dict:
        info = capi.DrilSacExtWrapInfo()
        self._chk(self._f("ext_wrap_info")(self._h, C.byref(info)))
        return dict(normalize_on=int(info.normalize_on), monitor_on=int(info.monitor_on), monitor_window=int(info.monitor_window), launches_act=int(info.launches_act),
                    launches_push=int(info.launches_push), allocations=int(info.allocations))

    def set_collect_noise(self, noise):
        self._noise = self._f32(noise)       # the oracle keeps the pointer until the next collect call
        self._chk(self._f("debug_set_collect_noise")(self._h, self._p(self._noise), 0 if noise is None else self._noise.size))

    def replay_size(self) -> int:
        return int(self._f("replay_size")(self._h))

    def replay_capacity(self) -> int:
        return int(self._f("replay_capacity")(self._h))

    def replay(self, which: int) -> np.ndarray:
        n = self.replay_size()
        shape, dt = {capi.RB_OBSERVATIONS: ((n, self.D), np.float32), capi.RB_NEXT_OBSERVATIONS: ((n, self.D), np.float32),
                     capi.RB_ACTIONS: ((n, self.A), np.float32), capi.RB_REWARDS: ((n,), np.float32),
                     capi.RB_TERMINATED: ((n,), np.uint8), capi.RB_TRUNCATED: ((n,), np.uint8)}[which]
        out = np.empty(shape, dt)
        self._chk(self._f("replay_copy_out")(self._h, which, self._p(out), out.nbytes))
        return out

    def replay_fill(self, obs, actions, rewards, terminated, truncated, next_obs):
        obs, actions, rewards, next_obs = self._f32(obs), self._f32(actions), self._f32(rewards), self._f32(next_obs)
        term = np.ascontiguousarray(terminated, np.uint8)
        trunc = np.ascontiguousarray(truncated, np.uint8)
        self._chk(self._f("replay_fill")(self._h, rewards.size, self._p(obs), self._p(actions), self._p(rewards), self._p(term), self._p(trunc), self._p(next_obs)))

    # gradient steps
    def set_batches(self, n_updates: int, idx=None, noise_ent=None, noise_next=None, noise_pi=None):
        self._inj = (None if idx is None else np.ascontiguousarray(idx, np.int64), self._f32(noise_ent), self._f32(noise_next), self._f32(noise_pi))
        self._chk(self._f("debug_set_batches")(self._h, n_updates, *[self._p(a) for a in self._inj]))

    def update(self, n_updates: int = 1):
        out = (DrilSacStats * n_updates)()
        self._chk(self._f("update")(self._h, n_updates, C.cast(out, C.c_void_p)))
        return list(out)

    def last_grads(self):
        gc, ga = np.empty(self.P, np.float32), np.empty(self.P, np.float32)
        self._chk(self._f("get_last_grads")(self._h, self._p(gc), self._p(ga), self.P))
        return gc, ga

    def update_info(self) -> str:
        """dril_sac_update_info: the launches the last gradient step enqueued ("gather=l1 head=fused,pre dw1=fused ...")"""
        return self._f("update_info")(self._h).decode()

    def train(self, max_steps: int, stats_capacity: int = 1 << 16, fps_capacity: int = 1 << 16):
        stats = (DrilSacStats * stats_capacity)()
        fps = np.zeros(fps_capacity, np.float64)
        n_upd, iters, total = C.c_int64(), C.c_int32(), C.c_int64()
        self._chk(self._f("train")(self._h, max_steps, C.cast(stats, C.c_void_p), stats_capacity, C.byref(n_upd),
                                   fps.ctypes.data_as(C.POINTER(C.c_double)), fps_capacity, C.byref(iters), C.byref(total)))
        return list(stats[:min(n_upd.value, stats_capacity)]), fps[:min(iters.value, fps_capacity)], n_upd.value, iters.value, total.value

    def iterate(self, iterations: int, want_stats: bool = True):
        """`iterations` rounds of train!'s loop body (sac.jl:464-535: collect train_freq env steps, then the gradient steps) without a host sync between them
        (dril_sac_iterate) -> (stats of every gradient step, fps of every iteration)"""
        n_upd = self.cfg.train_freq * self.E if self.cfg.gradient_steps == -1 else self.cfg.gradient_steps
        cap = iterations * max(n_upd, 0) if want_stats else 0
        stats = (DrilSacStats * max(cap, 1))()
        fps = np.zeros(iterations if want_stats else 1, np.float64)
        self._chk(self._f("iterate")(self._h, C.c_int32(iterations), C.cast(stats, C.c_void_p) if want_stats else None, C.c_int64(cap),
                                     fps.ctypes.data_as(C.POINTER(C.c_double)) if want_stats else None, C.c_int64(iterations if want_stats else 0)))
        return list(stats[:cap]), fps[:iterations] if want_stats else fps[:0]

    # MonitorWrapperEnv + evaluate_agent on the handle's device envs
    def monitor_enable(self, window: int = 100):
        """MonitorWrapperEnv(env, stats_window) around the handle's envs (monitorWrapperEnv.jl:15-24); 0 switches it off"""
        self._chk(self._f("monitor_enable")(self._h, int(window)))

    def monitor_stats(self):
        """(ep_rew_mean, ep_len_mean, n_episodes) of MonitorWrapperEnv's window (log_stats, monitorWrapperEnv.jl:64-70); the means are nan while the window is empty"""
        r, l, n = C.c_float(float("nan")), C.c_float(float("nan")), C.c_int32()
        self._chk(self._f("monitor_get_stats")(self._h, C.byref(r), C.byref(l), C.byref(n)))
        return r.value, l.value, n.value

    # NormalizeWrapperEnv around the handle's device envs (dril_sac_normalize_*): normalize_enable, normalize_config, normalize_set_training, norm_get_stats /
    # norm_set_stats / norm_get_original / norm_get_returns come from _normalize.normalize_verbs

    def evaluate_agent(self, n_eval_episodes: int = 10, deterministic: bool = True, seed: Optional[int] = None):
        """evaluate_agent(agent, env; n_eval_episodes, deterministic) -> (stats dict, episode_rewards, episode_lengths), evaluation.jl:54-143; env e is reset
        with seed + e (default: the config's seed).  Leaves the ring, the parameters and the training envs as they were."""
        st = capi.DrilEvalStats()
        er = np.empty(max(n_eval_episodes, 0), np.float32); el = np.empty(max(n_eval_episodes, 0), np.int32)
        self._chk(self._f("evaluate_agent")(self._h, n_eval_episodes, int(deterministic), self.cfg.seed if seed is None else seed, C.byref(st), self._p(er), self._p(el)))
        return dict(mean_reward=st.mean_reward, std_reward=st.std_reward, mean_length=st.mean_length, std_length=st.std_length,
                    n_steps=st.n_steps), er, el

    def collect_trajectory(self, n_trajectories: int = 1, max_steps: Optional[int] = None, deterministic: bool = True, seed: Optional[int] = None,
                           poll_steps: int = 0, final_original: bool = False):
        """collect_trajectory on the device, leaving nothing behind on the handle (dril_sac_collect_trajectory, docs/sac.md "Trajectories"): envs 0..n_trajectories-1
        record their first episode after the call's own reset -> (trajectories, lengths, end_flags, info dict), in the shapes of Handle.collect_trajectory_device.
        trajectories[m] = (observations (L+1, D), actions (L, A), rewards (L,)): original observations (rows 0..L-1 unscaled under ScalingWrapperEnv, never normalised),
        the actions the env's physics received, raw rewards; the last observation is the terminal state as the wrapper delivers it (final_original: unscaled too).
        end_flags: capi.TRAJ_TERMINATED | TRAJ_TRUNCATED | TRAJ_MAX_STEPS.  info: capacity, steps_enqueued, launches, longest, cut_by_max_steps, path (0)."""
        if max_steps is not None and int(max_steps) < 1:
            raise ValueError("max_steps is None or >= 1")
        o = capi.DrilTrajOptions()
        o.n_trajectories, o.max_steps, o.deterministic = int(n_trajectories), 0 if max_steps is None else int(max_steps), int(deterministic)
        o.poll_steps, o.final_original = int(poll_steps), int(bool(final_original))
        if seed is not None:
            o.seed, o.has_seed = int(seed), 1
        cap, info = C.c_int32(), capi.DrilTrajInfo()
        self._chk(self._f("trajectory_capacity")(self._h, C.byref(o), C.byref(cap)))
        M, T = max(int(n_trajectories), 1), cap.value
        obs = np.empty((M, T + 1, self.D), np.float32); act = np.empty((M, T, self.A), np.float32)
        rew = np.empty((M, T), np.float32); lengths = np.empty(M, np.int32); flags = np.empty(M, np.uint8)
        self._chk(self._f("collect_trajectory")(self._h, C.byref(o), self._p(obs), self._p(act), self._p(rew), self._p(lengths), self._p(flags), C.byref(info)))
        trajs = [(obs[m, :L + 1].copy(), act[m, :L].copy(), rew[m, :L].copy()) for m, L in enumerate(lengths)]
        return trajs, lengths, flags, dict(capacity=info.capacity, steps_enqueued=info.steps_enqueued, launches=info.launches, longest=info.longest,
                                           cut_by_max_steps=info.cut_by_max_steps, path=info.reserved[capi.TRAJ_INFO_PATH])

    def profile(self) -> dict:
        cm, um, cs, us = C.c_double(), C.c_double(), C.c_int64(), C.c_int64()
        self._chk(self._f("profile_get")(self._h, C.byref(cm), C.byref(cs), C.byref(um), C.byref(us)))
        return {"collect_ms": cm.value, "collect_steps": cs.value, "update_ms": um.value, "updates": us.value}

    def profile_reset(self):
        self._chk(self._f("profile_reset")(self._h))


# --------------------------------------------------------------------------------------------
# Agent / ReplayBuffer / train!
# --------------------------------------------------------------------------------------------
@dataclass
class SACAgent:
    """Agent(layer, alg::SAC; rng) sac.jl:160-188: train_state, Q_target_parameters (copy of the critics), ent_train_state"""
    layer: SACLayer
    alg: SAC
    seed: int = 0
    parameters: dict = field(init=False)
    q_target_parameters: np.ndarray = field(init=False)
    log_ent_coef: float = field(init=False)
    steps_taken: int = 0
    gradient_updates: int = 0

    def __post_init__(self):
        rng = np.random.default_rng(self.seed)
        self.parameters = self.layer.initialparameters(rng)
        flat = sac_flatten_params(self.parameters)
        a = self.layer
        n_actor = a.obs_dim * a.hidden_dims[0] + a.hidden_dims[0] + a.hidden_dims[0] * a.hidden_dims[1] + a.hidden_dims[1] + a.hidden_dims[1] * a.act_dim + a.act_dim
        self.q_target_parameters = flat[n_actor:n_actor + 2 * a.q_parameterlength()].copy()           # copy_critic_parameters sac.jl:191-197
        ec = self.alg.ent_coef
        self.log_ent_coef = math.log(ec.initial_value if isinstance(ec, AutoEntropyCoefficient) else ec.coef)   # sac.jl:207-213


class ReplayBuffer:
    """ReplayBuffer(observation_space, action_space, capacity) replay_buffer.jl:14-31 — a view of the device ring of one SacHandle"""

    def __init__(self, observation_space: Box, action_space: Box, capacity: int):
        self.observation_space, self.action_space, self.capacity = observation_space, action_space, capacity
        self.handle: Optional[SacHandle] = None

    def __len__(self):
        return 0 if self.handle is None else self.handle.replay_size()

    def isfull(self) -> bool:
        return len(self) == self.capacity

    def _get(self, which):
        return self.handle.replay(which)

    observations = property(lambda s: s._get(capi.RB_OBSERVATIONS))
    actions = property(lambda s: s._get(capi.RB_ACTIONS))
    rewards = property(lambda s: s._get(capi.RB_REWARDS))
    terminated = property(lambda s: s._get(capi.RB_TERMINATED).astype(bool))
    truncated = property(lambda s: s._get(capi.RB_TRUNCATED).astype(bool))
    next_observations = property(lambda s: s._get(capi.RB_NEXT_OBSERVATIONS))


_SAC_STAT_KEYS = ("actor_losses", "critic_losses", "entropy_losses", "entropy_coefficients", "q_values", "learning_rates", "grad_norms",
                  "fps", "steps_taken")


def _monitor_from_env(h: SacHandle, env):
    """MonitorWrapperEnv(env, stats_window) over a device env (host.py: it records the window in the env's keywords): the same wrapper around the SAC handle's envs,
    so that `replay_buffer.handle.monitor_stats()` gives what the reference logs as env/ep_rew_mean after every iteration (sac.jl:307)"""
    window = int(getattr(env, "_kw", {}).get("monitor_window", 0) or 0)
    if window > 0:
        h.monitor_enable(window)


def _scaling_from_env(h: SacHandle, env):
    """ScalingWrapperEnv around a DeviceModuleEnv (DeviceModuleEnv(..., scaling=True) / ScalingWrapperEnv(DeviceModuleEnv(...))): the same wrapper around the SAC
    handle's envs, before their first reset and inside NormalizeWrapperEnv.  A handle that comes back with a replay buffer already has it."""
    want = bool(getattr(getattr(env, "env", None), "scaling", False))
    if getattr(getattr(env, "env", None), "kind", None) == capi.ENV_MODULE and h.agent_spaces()["scaling"] != want:
        h.scaling_enable(want)


def _normalize_kw(env, normalize: Optional[dict]) -> Optional[dict]:
    """the NormalizeWrapperEnv keywords of a run: the `normalize=` argument (the one way a DeviceModuleEnv gets the wrapper: host.NormalizeWrapperEnv probes the PPO
    handle, which refuses plug-ins) wins over what NormalizeWrapperEnv(DeviceParallelEnv(...)) recorded in the env's keywords; None: no wrapper"""
    if normalize is not None:
        return dict(normalize)
    kw = getattr(env, "_kw", {}).get("normalize")
    return dict(kw) if kw is not None else None


def _normalize_from_env(h: SacHandle, env, normalize: Optional[dict]):
    """the wrapper of this run around the SAC handle's envs (a handle that already carries this configuration keeps its statistics); no keywords: off"""
    kw = _normalize_kw(env, normalize)
    if kw is None:
        h.normalize_enable(False)
    else:
        h.normalize_enable(**kw)


def _sac_throwaway_handle(agent: "SACAgent", env, normalize: Optional[dict], normalize_stats, who: str, what: str) -> "SacHandle":
    """the throw-away handle of sac_evaluate_agent / sac_collect_trajectory over a DeviceParallelEnv or a DeviceModuleEnv: the agent's parameters, ScalingWrapperEnv as
    the env carries it, NormalizeWrapperEnv (the env's own keywords, or `normalize`) with training off and the statistics of `normalize_stats` — the training handle, a
    norm_get_stats() dict, or "fresh"; without them a RuntimeWarning says that the run is under mean 0 / var 1.  The caller closes it."""
    small = replace(agent.alg, buffer_capacity=max(env.n_envs, 1))        # neither verb touches the ring: the smallest one the library accepts
    cfg = make_sac_config(env.env, env.n_envs, small, agent.layer, seed=env.seed, device=env._kw.get("device", 0))
    h = SacHandle(cfg, env_module=getattr(env.env, "code_object_path", None))
    try:
        h.set_params(sac_flatten_params(agent.parameters))
        _scaling_from_env(h, env)
        kw = _normalize_kw(env, normalize)
        if kw is not None:           # sync_normalization_stats! + set_training(eval_env, false) (normalizeWrapperEnv.jl:245-249,299-309): the training statistics, frozen
            h.normalize_enable(**{**kw, "training": False})
            if normalize_stats is None:
                warnings.warn(f"{who}: the env is normalised but no normalize_stats were given: the {what} runs with fresh statistics (mean 0, var 1), "
                              "not those the agent was trained under; pass the training handle (replay_buffer.handle), a norm_get_stats() dict, or \"fresh\" to say so",
                              RuntimeWarning, stacklevel=3)
            st = None if isinstance(normalize_stats, str) else normalize_stats.norm_get_stats() if hasattr(normalize_stats, "norm_get_stats") else normalize_stats
            if isinstance(normalize_stats, str) and normalize_stats != "fresh":
                raise ValueError("normalize_stats: a handle, a norm_get_stats() dict, or \"fresh\"")
            if st is not None:
                h.norm_set_stats(*(st[k] for k in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count")))
    except BaseException:
        h.close()
        raise
    return h


def sac_evaluate_agent(agent: SACAgent, env, n_eval_episodes: int = 10, deterministic: bool = True, reward_threshold: Optional[float] = None,
                       return_stats: bool = True, *, normalize: Optional[dict] = None, normalize_stats=None):
    """evaluate_agent(agent, env; ...) (src/evaluation.jl:54-143) of a SAC agent on a DeviceParallelEnv over a Box env or a DeviceModuleEnv over a Box plug-in:
    the agent's actor on `env.n_envs` device envs seeded env.seed + i, episode accounting on the device (dril_sac_evaluate_agent).  Return shapes of
    host.py::evaluate_agent: the statistics dict, or (episode_rewards, episode_lengths) with return_stats=False.
    NormalizeWrapperEnv (the env's own keywords, or `normalize=dict(...)`): the evaluation handle is a throw-away one, so the training statistics are loaded into it
    from `normalize_stats` — the training handle (`replay_buffer.handle`) or a norm_get_stats() dict — with training off; reported returns are raw.  Without
    them the evaluation would silently run under mean 0 / var 1: that is a RuntimeWarning unless `normalize_stats="fresh"` asks for it (an untrained agent)."""
    if isinstance(env, DeviceArrayParallelEnv):
        return _sac_evaluate_device_arrays(agent, env, n_eval_episodes, deterministic, reward_threshold, return_stats, normalize_stats)
    if getattr(env, "kind", None) == capi.ENV_EXTERNAL:
        raise NotImplementedError("sac_evaluate_agent: host envs (HostParallelEnv) are evaluated on the host; the device verb steps device envs")
    h = _sac_throwaway_handle(agent, env, normalize, normalize_stats, "sac_evaluate_agent", "evaluation")
    try:
        stats, er, el = h.evaluate_agent(n_eval_episodes, deterministic, seed=env.seed)
    finally:
        h.close()
    if reward_threshold is not None and stats["mean_reward"] < reward_threshold:
        raise RuntimeError(f"Mean reward below threshold: {stats['mean_reward']:.2f} < {reward_threshold}")   # evaluation.jl:131-135
    return {k: stats[k] for k in ("mean_reward", "std_reward", "mean_length", "std_length")} if return_stats else (er, el.astype(np.int64))


def sac_collect_trajectory(agent: SACAgent, env, max_steps: Optional[int] = None, norm_env=None, deterministic: bool = True, n_trajectories: int = 1,
                           seed: Optional[int] = None, *, normalize: Optional[dict] = None, normalize_stats=None):
    """collect_trajectory(agent, env; max_steps, norm_env, deterministic) (src/utils/trajectory_utils.jl:3-49) of a SAC agent on a DeviceParallelEnv over a Box env or a
    DeviceModuleEnv over a Box plug-in -> (observations, actions, rewards): the original observations (L + 1 of them, the last one the terminal state), the env actions
    and the raw rewards of one episode; n_trajectories > 1: a list of such triples, envs 0..n-1 of the parallel env, each its first episode after the reset (seed:
    env.seed by default).  Runs on a throw-away handle built as sac_evaluate_agent builds its own (dril_sac_collect_trajectory, docs/sac.md "Trajectories"):
    NormalizeWrapperEnv frozen, under `normalize_stats`; the recording is raw.  norm_env: None, or `env` itself — the normaliser around a device env is a mode of the
    handle, found in the env's keywords (or `normalize=`)."""
    if isinstance(env, (HostParallelEnv, DeviceArrayParallelEnv)) or getattr(env, "kind", None) == capi.ENV_EXTERNAL:
        raise NotImplementedError("sac_collect_trajectory: host envs (HostParallelEnv, DeviceArrayParallelEnv) live with the caller; the device verb steps device envs "
                                  "(record there, in a loop over predict_actions)")
    if norm_env is not None and norm_env is not env:
        raise NotImplementedError("sac_collect_trajectory: norm_env is None or the env itself (NormalizeWrapperEnv around a device env is a mode of the handle: it is "
                                  "taken from the env's keywords or `normalize=` and applied frozen, with the statistics of `normalize_stats`)")
    h = _sac_throwaway_handle(agent, env, normalize, normalize_stats, "sac_collect_trajectory", "recording")
    try:
        trajs, _, flags, _ = h.collect_trajectory(n_trajectories, max_steps, deterministic, env.seed if seed is None else seed)
    finally:
        h.close()
    if (flags & capi.TRAJ_MAX_STEPS).any():
        warnings.warn("Max steps reached")                                           # trajectory_utils.jl:39
    return trajs[0] if n_trajectories == 1 else trajs


def _sac_ext_handle(agent: SACAgent, env, alg: SAC, rb_handle=None) -> "SacHandle":
    """the DRIL_ENV_EXTERNAL handle of a DeviceArrayParallelEnv: a Box with per-dimension bounds goes through dril_sac_ext_set_action_bounds"""
    if rb_handle is not None:
        return rb_handle
    asp = env.action_space()
    cfg = make_sac_config(env, env.n_envs, alg, agent.layer, seed=env.seed, device=env._kw.get("device", 0), profile_events=env._kw.get("profile_events", False), per_dim_bounds=True)
    h = SacHandle(cfg)
    lo, hi = np.asarray(asp.low, np.float32).ravel(), np.asarray(asp.high, np.float32).ravel()
    if np.unique(lo).size != 1 or np.unique(hi).size != 1:
        h.ext_set_action_bounds(lo, hi)
    return h


def _eval_normalize_stats(normalize_stats):
    """normalize_stats of sac_evaluate_agent -> a statistics dict, or None for "fresh": the training handle, a norm_get_stats() dict, or the word"""
    from .host import _norm_view
    if isinstance(normalize_stats, str):
        if normalize_stats != "fresh":
            raise ValueError("normalize_stats: a handle, a norm_get_stats() dict, or \"fresh\"")
        return None
    if normalize_stats is None:
        warnings.warn("sac_evaluate_agent: the env is normalised but no normalize_stats were given: the evaluation runs with fresh statistics (mean 0, var 1), "
                      "not those the agent was trained under; pass the training handle (replay_buffer.handle), a norm_get_stats() dict, or \"fresh\" to say so",
                      RuntimeWarning, stacklevel=4)
        return None
    return _norm_view(normalize_stats).norm_get_stats() if hasattr(normalize_stats, "norm_get_stats") else normalize_stats


def _sac_evaluate_device_arrays(agent: SACAgent, env: DeviceArrayParallelEnv, n_eval_episodes: int, deterministic: bool, reward_threshold: Optional[float], return_stats: bool,
                                normalize_stats=None):
    """the reference loop (evaluation.jl:86-125) with observations and actions on the device: dril_sac_predict_actions_device per step.  Rewards and flags (E values
    each) come to the host once per step for the episode accounting — that wait is the accounting's, not the library's.  A wrapped env (NormalizeWrapperEnv(env)):
    the throw-away handle takes the wrapper with training off and the statistics of `normalize_stats`; dril_sac_predict_actions_device normalises under them and
    updates nothing; the rewards come from the env itself, so the reported returns are raw"""
    h = _sac_ext_handle(agent, env, replace(agent.alg, buffer_capacity=max(env.n_envs, 1)))   # an evaluation never touches the ring
    try:
        h.set_params(sac_flatten_params(agent.parameters))
        if env.ext_normalize is not None:       # sync_normalization_stats! + set_training(eval_env, false) (normalizeWrapperEnv.jl:245-249,299-309)
            h.ext_normalize_enable(**{**env.ext_normalize, "training": False})
            st = _eval_normalize_stats(normalize_stats)
            if st is not None:
                h.ext_normalize_set_stats(*(st[k] for k in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count")))
        er, el = [], []
        cur_r, cur_l = np.zeros(env.n_envs, np.float32), np.zeros(env.n_envs, np.int64)
        env.reset_()
        obs = env.observe()
        _, ea = env.action_arrays(h, obs)
        while len(er) < n_eval_episodes:
            h.predict_actions_device(obs, deterministic, None, None, ea, env.stream)
            rew, term, trunc, _ = env.act_(ea)
            obs = env.observe()
            rew, done = _to_host(rew, env.stream), _to_host(term, env.stream).astype(bool) | _to_host(trunc, env.stream).astype(bool)
            cur_r += rew; cur_l += 1
            for i in np.nonzero(done)[0]:
                if len(er) < n_eval_episodes:
                    er.append(float(cur_r[i])); el.append(int(cur_l[i]))
                    cur_r[i] = 0; cur_l[i] = 0
    finally:
        h.close()
    er, el = np.asarray(er, np.float32), np.asarray(el, np.int64)
    sd = lambda x: float(np.std(x, ddof=1)) if len(x) > 1 else float("nan")
    stats = {"mean_reward": float(er.mean()), "std_reward": sd(er), "mean_length": float(el.mean()), "std_length": sd(el)}
    if reward_threshold is not None and stats["mean_reward"] < reward_threshold:
        raise RuntimeError(f"Mean reward below threshold: {stats['mean_reward']:.2f} < {reward_threshold}")   # evaluation.jl:131-135
    return stats if return_stats else (er, el)


def sac_train_(agent: SACAgent, env, alg: SAC, max_steps: int, *, replay_buffer: Optional[ReplayBuffer] = None, callbacks=None, normalize: Optional[dict] = None):
    """train!(agent, env, alg::SAC, max_steps) sac.jl:406-549 -> (agent, replay_buffer, training_stats, timer); `env` is a
    DeviceParallelEnv over PendulumEnv / MountainCarContinuousEnv, a DeviceModuleEnv over a Box plug-in, or a HostParallelEnv.  training_stats carries the fields of SACTrainingStats (sac.jl:243-257).
    NormalizeWrapperEnv(DeviceParallelEnv(...)) trains on normalised observations and rewards (dril_sac_normalize_enable); `normalize=dict(...)` gives the same wrapper
    to any device env — a DeviceModuleEnv has no other way to it — and wins over the env's own keywords.  The statistics stay on `replay_buffer.handle` (norm_get_stats)."""
    if getattr(env, "kind", None) == capi.ENV_EXTERNAL:
        if normalize is not None:
            raise NotImplementedError("sac_train_: host envs (HostParallelEnv) are normalised on the host; normalize= wraps device envs")
        if isinstance(env, DeviceArrayParallelEnv):
            return _sac_train_device_arrays(agent, env, alg, max_steps, replay_buffer, list(callbacks or []))
        return _sac_train_host(agent, env, alg, max_steps, replay_buffer, list(callbacks or []))
    if callbacks:
        return _sac_train_callbacks(agent, env, alg, max_steps, replay_buffer, list(callbacks), normalize)
    t0 = time.perf_counter()
    rb = replay_buffer or ReplayBuffer(env.observation_space(), env.action_space(), alg.buffer_capacity)     # sac.jl:411
    cfg = make_sac_config(env.env, env.n_envs, alg, agent.layer, seed=env.seed, device=env._kw.get("device", 0), profile_events=env._kw.get("profile_events", False))
    h = rb.handle if rb.handle is not None else SacHandle(cfg, env_module=getattr(env.env, "code_object_path", None))
    rb.handle = h
    _monitor_from_env(h, env)
    _scaling_from_env(h, env)
    _normalize_from_env(h, env, normalize)
    h.set_params(sac_flatten_params(agent.parameters))
    h.set_target_params(agent.q_target_parameters)
    h.set_log_ent_coef(agent.log_ent_coef)
    h.env_reset(env.seed)
    stats, fps, n_upd, iters, total = h.train(max_steps)
    ts = {k: [] for k in _SAC_STAT_KEYS}
    for s in stats:
        ts["actor_losses"].append(s.actor_loss); ts["critic_losses"].append(s.critic_loss)
        if s.has_entropy_loss:
            ts["entropy_losses"].append(s.entropy_loss)
        ts["entropy_coefficients"].append(s.entropy_coefficient); ts["q_values"].append(s.mean_q_values)
        ts["learning_rates"].append(alg.learning_rate); ts["grad_norms"].append(s.grad_norm)
    ts["fps"] = list(fps)
    agent.steps_taken += total
    agent.gradient_updates += n_upd
    agent.parameters = sac_unflatten_params(h.get_params(), agent.parameters)
    agent.q_target_parameters = h.get_target_params()
    agent.log_ent_coef = h.get_log_ent_coef()
    return agent, rb, ts, {"training_loop": time.perf_counter() - t0, "iterations": iters}


def _jl_div(a: int, b: int) -> int:
    """Julia's div: truncation toward zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def _sac_train_callbacks(agent: SACAgent, env, alg: SAC, max_steps: int, replay_buffer: Optional[ReplayBuffer], cbs: list, normalize: Optional[dict] = None):
    """train!(agent, replay_buffer, env, alg::SAC, max_steps; callbacks) (sac.jl:428-559) step by step, so that the hooks run where the reference runs them:
    on_training_start (:476-483), on_rollout_start (:488-495), on_step before every env step of the collection (off_policy_collection.jl:44-49), on_rollout_end
    (:508-515), on_training_end (:545-552).  Each gets a dict of the reference's locals; a false return stops the training and — as in the reference — the early
    returns are (agent, replay_buffer, training_stats) without the timer.  Differences: the transitions of a collection that on_step interrupted are already in
    the device ring (the reference drops that partial rollout), and one env step is one device call (a drain per step: callbacks want the state) —
    `dril_sac_collect_rollout(1)` for the first step of a collection and `dril_sac_collect_continue(1)` for the others, so that NormalizeWrapperEnv observes once at
    the collection's start as inside the reference's collect_trajectories: statistics, ring and weights are those of the callback-less loop, bit for bit."""
    hook = lambda name, loc: all(getattr(c, name)(loc) for c in cbs if hasattr(c, name))
    step_hooks = [c for c in cbs if hasattr(c, "on_step")]
    t0 = time.perf_counter()
    rb = replay_buffer or ReplayBuffer(env.observation_space(), env.action_space(), alg.buffer_capacity)
    cfg = make_sac_config(env.env, env.n_envs, alg, agent.layer, seed=env.seed, device=env._kw.get("device", 0), profile_events=env._kw.get("profile_events", False))
    h = rb.handle if rb.handle is not None else SacHandle(cfg, env_module=getattr(env.env, "code_object_path", None))
    rb.handle = h
    _monitor_from_env(h, env)
    _scaling_from_env(h, env)
    _normalize_from_env(h, env, normalize)
    h.set_params(sac_flatten_params(agent.parameters)); h.set_target_params(agent.q_target_parameters); h.set_log_ent_coef(agent.log_ent_coef)
    h.env_reset(env.seed)
    E = env.n_envs
    total_start = alg.start_steps if alg.start_steps > 0 else alg.train_freq * E              # sac.jl:456-458
    adjusted = max(1, _jl_div(total_start, E)) * E
    n_steps = _jl_div(adjusted, E)
    iterations = _jl_div(max_steps - adjusted, alg.train_freq * E) + 1                          # :463
    total_steps = n_steps * E + alg.train_freq * E * (iterations - 1)
    ts = {k: [] for k in _SAC_STAT_KEYS}
    loc = dict(agent=agent, replay_buffer=rb, env=env, alg=alg, max_steps=max_steps, callbacks=cbs, n_envs=E, layer=agent.layer, training_stats=ts,
               gradient_updates_performed=0, total_start_steps=total_start, adjusted_total_start_steps=adjusted, n_steps=n_steps, training_iteration=0,
               iterations=iterations, total_steps=total_steps, update_entropy_coef=isinstance(alg.ent_coef, AutoEntropyCoefficient))
    done_updates = 0

    def sync_agent():
        agent.parameters = sac_unflatten_params(h.get_params(), agent.parameters)
        agent.q_target_parameters = h.get_target_params()
        agent.log_ent_coef = h.get_log_ent_coef()

    try:
        if not hook("on_training_start", loc):
            return agent, rb, ts
        for it in range(1, max(iterations, 0) + 1):
            loc.update(training_iteration=it, n_steps=n_steps)
            if not hook("on_rollout_start", loc):
                return agent, rb, ts
            use_random = it == 1 and alg.start_steps > 0
            a = time.perf_counter()
            for i in range(1, n_steps + 1):
                loc.update(i=i, use_random_actions=use_random)
                if step_hooks and not all(c.on_step(loc) for c in step_hooks):
                    return agent, rb, ts                                                          # "Collecting rollout stopped due to callback failure", :502-505
                if i == 1:
                    h.collect_rollout(1, use_random)
                else:                                                                             # the same collect_trajectories call: NormalizeWrapperEnv observes once, at its start
                    h.collect_continue(1, use_random)
            fps = n_steps * E / max(time.perf_counter() - a, 1e-9)
            loc.update(fps=fps, success=True)
            if not hook("on_rollout_end", loc):
                return agent, rb, ts
            ts["fps"].append(fps)
            agent.steps_taken += n_steps * E
            n_steps = alg.train_freq                                                              # :521
            n_upd = get_gradient_steps(alg, alg.train_freq, E)
            for s_ in (h.update(n_upd) if n_upd > 0 else []):
                ts["actor_losses"].append(s_.actor_loss); ts["critic_losses"].append(s_.critic_loss)
                if s_.has_entropy_loss:
                    ts["entropy_losses"].append(s_.entropy_loss)
                ts["entropy_coefficients"].append(s_.entropy_coefficient); ts["q_values"].append(s_.mean_q_values)
                ts["learning_rates"].append(alg.learning_rate); ts["grad_norms"].append(s_.grad_norm)
                done_updates += 1
            agent.gradient_updates += n_upd
            loc.update(gradient_updates_performed=done_updates, n_updates=n_upd)
        timer = {"training_loop": time.perf_counter() - t0, "iterations": max(iterations, 0)}
        if not hook("on_training_end", loc):
            return agent, rb, ts, timer                                                           # :548-550 (this one returns the timer too)
        return agent, rb, ts, timer
    finally:
        sync_agent()                                                                              # the reference mutates the agent's train_state in place: every exit leaves the trained weights in it


def _sac_train_host(agent: SACAgent, env, alg: SAC, max_steps: int, replay_buffer: Optional[ReplayBuffer] = None, cbs: Optional[list] = None):
    """train!(agent, replay_buffer, env, alg::SAC, max_steps) (sac.jl:428-559) over the caller's own envs (HostParallelEnv): the envs step on the
    host, the policy, the replay ring and every gradient step live on the device (DRIL_ENV_EXTERNAL: dril_sac_predict_actions + dril_sac_ext_push).
    `cbs`: callbacks with the reference's five hooks in the reference's places (see _sac_train_callbacks); a false return ends the training with the
    reference's early-return shape (agent, replay_buffer, training_stats), the trained weights in the agent"""
    cbs = cbs or []
    hook = lambda name, loc: all(getattr(c, name)(loc) for c in cbs if hasattr(c, name))
    step_hooks = [c for c in cbs if hasattr(c, "on_step")]
    t0 = time.perf_counter()
    E, asp = env.n_envs, env.action_space()
    rb = replay_buffer or ReplayBuffer(env.observation_space(), asp, alg.buffer_capacity)
    cfg = make_sac_config(env, E, alg, agent.layer, seed=env.seed, device=env._kw.get("device", 0), profile_events=env._kw.get("profile_events", False))
    h = rb.handle if rb.handle is not None else SacHandle(cfg)
    rb.handle = h
    h.set_params(sac_flatten_params(agent.parameters)); h.set_target_params(agent.q_target_parameters); h.set_log_ent_coef(agent.log_ent_coef)
    rng = np.random.default_rng(env.seed)
    low, high = np.float32(asp.low[0]), np.float32(asp.high[0])
    total_start = alg.start_steps if alg.start_steps > 0 else alg.train_freq * E                    # sac.jl:456-458
    adjusted = max(1, total_start // E) * E
    n_steps = adjusted // E
    iterations = int((max_steps - adjusted) / (alg.train_freq * E)) + 1                             # div truncates toward zero, :462
    n_updates = get_gradient_steps(alg, alg.train_freq, E)
    ts = {k: [] for k in _SAC_STAT_KEYS}
    total = n_upd = 0
    t_env = t_dev = 0.0
    obs = np.stack(env.observe())
    loc = dict(agent=agent, replay_buffer=rb, env=env, alg=alg, max_steps=max_steps, callbacks=cbs, n_envs=E, layer=agent.layer, training_stats=ts,
               gradient_updates_performed=0, total_start_steps=total_start, adjusted_total_start_steps=adjusted, n_steps=n_steps, training_iteration=0,
               iterations=iterations, total_steps=n_steps * E + alg.train_freq * E * (iterations - 1))

    def leave(early):
        agent.steps_taken += total
        agent.gradient_updates += n_upd
        agent.parameters = sac_unflatten_params(h.get_params(), agent.parameters)
        agent.q_target_parameters = h.get_target_params()
        agent.log_ent_coef = h.get_log_ent_coef()
        timer = {"training_loop": time.perf_counter() - t0, "iterations": max(iterations, 0), "collect_rollout": t_env, "device": t_dev}
        return (agent, rb, ts) if early else (agent, rb, ts, timer)

    if not hook("on_training_start", loc):
        return leave(True)
    for it in range(max(iterations, 0)):
        use_random = it == 0 and alg.start_steps > 0                                                # :487
        loc.update(training_iteration=it + 1, n_steps=n_steps)
        if not hook("on_rollout_start", loc):
            return leave(True)
        a = time.perf_counter()
        for i_step in range(n_steps):                                                               # collect_trajectories, off_policy_collection.jl:28-96
            if step_hooks:
                loc.update(i=i_step + 1, use_random_actions=use_random)
                if not all(c.on_step(loc) for c in step_hooks):
                    return leave(True)
            if use_random:
                stored = env_act = rng.uniform(low, high, (E, h.A)).astype(np.float32)              # rand(rng, act_space): env space, stored as is (:50-53,72)
            else:
                b = time.perf_counter()
                stored, env_act = h.predict_actions(obs)                                            # raw squashed action + to_env(TanhScaleAdapter), :55-58
                t_dev += time.perf_counter() - b
            rew, term, trunc, infos = env.act_([x.reshape(asp.shape) for x in env_act])             # :60
            nobs = np.stack(env.observe())                                                          # :61
            tobs = None
            if trunc.any():
                tobs = nobs.copy()
                for i in np.nonzero(trunc)[0]:
                    tobs[i] = infos[i]["terminal_observation"]
            b = time.perf_counter()
            h.ext_push(obs, stored, rew, term, trunc, nobs, tobs)                                   # push!(buffer, traj), replay_buffer.jl:98-114
            t_dev += time.perf_counter() - b
            obs = nobs
        t_env += time.perf_counter() - a
        fps = n_steps * E / max(time.perf_counter() - a, 1e-12)
        total += n_steps * E
        loc.update(fps=fps, success=True)
        if not hook("on_rollout_end", loc):
            return leave(True)
        ts["fps"].append(fps)
        n_steps = alg.train_freq                                                                    # :520
        if n_updates > 0:
            b = time.perf_counter()
            for s in h.update(n_updates):                                                           # :523-538
                ts["actor_losses"].append(s.actor_loss); ts["critic_losses"].append(s.critic_loss)
                if s.has_entropy_loss:
                    ts["entropy_losses"].append(s.entropy_loss)
                ts["entropy_coefficients"].append(s.entropy_coefficient); ts["q_values"].append(s.mean_q_values)
                ts["learning_rates"].append(alg.learning_rate); ts["grad_norms"].append(s.grad_norm)
            t_dev += time.perf_counter() - b
            n_upd += n_updates
            loc.update(gradient_updates_performed=n_upd)
    hook("on_training_end", loc)                                                                    # (a failure here still returns the timer, sac.jl:548-550)
    return leave(False)


def _sac_train_device_arrays(agent: SACAgent, env: DeviceArrayParallelEnv, alg: SAC, max_steps: int, replay_buffer: Optional[ReplayBuffer] = None, cbs: Optional[list] = None):
    """the loop of _sac_train_host for ONE batched env whose arrays live on the device (DeviceArrayParallelEnv): dril_sac_ext_act_device -> the env's own act_ ->
    dril_sac_ext_push_device -> dril_sac_update_enqueue, none of which waits on the host or copies across PCIe; the random actions of the start phase are drawn on the
    device.  dril_sac_flush — the one drain, which also brings the statistics rows — runs when the pending table would overflow, before a callback hook (it may read
    the agent or the statistics) and at the end.  The timer dict gains "flushes" and "host_syncs" (waits inside the sync-free verbs: 0).
    NormalizeWrapperEnv(env) / MonitorWrapperEnv(env, window) around the DeviceArrayParallelEnv are the handle's own wrappers (dril_sac_ext_normalize_enable /
    dril_sac_ext_monitor_enable): the loop stays as it is, plus dril_sac_ext_collection_begin before every collection; `replay_buffer.handle.ext_monitor_stats()`
    and `.ext_normalize_get_stats()` read them, and env.reset_() resets the wrapper with the env."""
    cbs = cbs or []
    has_hook = lambda name: any(hasattr(c, name) for c in cbs)
    step_hooks = [c for c in cbs if hasattr(c, "on_step")]
    t0 = time.perf_counter()
    E, asp = env.n_envs, env.action_space()
    rb = replay_buffer or ReplayBuffer(env.observation_space(), asp, alg.buffer_capacity)
    h = _sac_ext_handle(agent, env, alg, rb.handle)
    rb.handle = h
    env.bind_sac(h)                                                                                 # NormalizeWrapperEnv(env) / MonitorWrapperEnv(env, window) as recorded on the env: the handle's own wrappers (a handle that comes back keeps its statistics)
    h.set_params(sac_flatten_params(agent.parameters)); h.set_target_params(agent.q_target_parameters); h.set_log_ent_coef(agent.log_ent_coef)
    total_start = alg.start_steps if alg.start_steps > 0 else alg.train_freq * E                    # sac.jl:456-458
    adjusted = max(1, total_start // E) * E
    n_steps = adjusted // E
    iterations = int((max_steps - adjusted) / (alg.train_freq * E)) + 1                             # div truncates toward zero, :462
    n_updates = get_gradient_steps(alg, alg.train_freq, E)
    ts = {k: [] for k in _SAC_STAT_KEYS}
    total = n_upd = 0
    t_env = t_dev = 0.0
    info0 = h.ext_device_info()
    cap = info0["pending_capacity"]
    pending = info0["pending_updates"]
    obs = env.observe()
    _, env_act = env.action_arrays(h, obs)
    loc = dict(agent=agent, replay_buffer=rb, env=env, alg=alg, max_steps=max_steps, callbacks=cbs, n_envs=E, layer=agent.layer, training_stats=ts,
               gradient_updates_performed=0, total_start_steps=total_start, adjusted_total_start_steps=adjusted, n_steps=n_steps, training_iteration=0,
               iterations=iterations, total_steps=n_steps * E + alg.train_freq * E * (iterations - 1))

    def flush():
        nonlocal pending, t_dev
        b = time.perf_counter()
        try:
            rows, err = h.flush(), None
        except DrilError as e:                                                                      # the sticky error: the rows it took out of the table still count
            rows, err = getattr(e, "stats", []), e
        for s_ in rows:
            ts["actor_losses"].append(s_.actor_loss); ts["critic_losses"].append(s_.critic_loss)
            if s_.has_entropy_loss:
                ts["entropy_losses"].append(s_.entropy_loss)
            ts["entropy_coefficients"].append(s_.entropy_coefficient); ts["q_values"].append(s_.mean_q_values)
            ts["learning_rates"].append(alg.learning_rate); ts["grad_norms"].append(s_.grad_norm)
        pending = 0
        t_dev += time.perf_counter() - b
        if err is not None:
            raise err

    def hook(name):
        if not has_hook(name):
            return True
        flush()                                                                                     # the hook may read the agent, the ring or the statistics
        return all(getattr(c, name)(loc) for c in cbs if hasattr(c, name))

    def leave(early):
        try:
            flush()
        finally:
            agent.steps_taken += total
            agent.gradient_updates += n_upd
            agent.parameters = sac_unflatten_params(h.get_params(), agent.parameters)
            agent.q_target_parameters = h.get_target_params()
            agent.log_ent_coef = h.get_log_ent_coef()
        info = h.ext_device_info()
        timer = {"training_loop": time.perf_counter() - t0, "iterations": max(iterations, 0), "collect_rollout": t_env, "device": t_dev,
                 "flushes": info["flushes"] - info0["flushes"], "host_syncs": info["host_syncs"] - info0["host_syncs"]}
        return (agent, rb, ts) if early else (agent, rb, ts, timer)

    if not hook("on_training_start"):
        return leave(True)
    for it in range(max(iterations, 0)):
        use_random = it == 0 and alg.start_steps > 0                                                # :487
        loc.update(training_iteration=it + 1, n_steps=n_steps)
        if not hook("on_rollout_start"):
            return leave(True)
        a = time.perf_counter()
        h.ext_collection_begin()                                                                    # the next act is the opening observe(env), :43 (a host flag)
        for i_step in range(n_steps):                                                               # collect_trajectories, off_policy_collection.jl:28-96
            if step_hooks:
                loc.update(i=i_step + 1, use_random_actions=use_random)
                if not hook("on_step"):
                    return leave(True)
            b = time.perf_counter()
            h.ext_act_device(obs, use_random, None, None, env_act, env.stream)                      # rand(act_space) | predict_actions + to_env(TanhScaleAdapter), :50-58
            t_dev += time.perf_counter() - b
            rew, term, trunc, tobs = env.act_(env_act)                                              # :60
            nobs = env.observe()                                                                    # :61
            b = time.perf_counter()
            h.ext_push_device(rew, term, trunc, nobs, tobs, env.stream)                             # push!(buffer, traj), replay_buffer.jl:98-114
            t_dev += time.perf_counter() - b
            obs = nobs
        t_env += time.perf_counter() - a
        fps = n_steps * E / max(time.perf_counter() - a, 1e-12)                                     # (enqueue rate: nothing waited for the device)
        total += n_steps * E
        loc.update(fps=fps, success=True)
        if not hook("on_rollout_end"):
            return leave(True)
        ts["fps"].append(fps)
        n_steps = alg.train_freq                                                                    # :520
        left = n_updates
        while left > 0:                                                                             # :523-538, in pieces the pending table holds
            k = min(left, cap)
            if pending + k > cap:
                flush()
            b = time.perf_counter()
            h.update_enqueue(k)
            t_dev += time.perf_counter() - b
            pending += k; left -= k
        n_upd += max(n_updates, 0)
        loc.update(gradient_updates_performed=n_upd)
    hook("on_training_end")                                                                         # (a failure here still returns the timer, sac.jl:548-550)
    return leave(False)
