"""NormalizeWrapperEnv (normalizeWrapperEnv.jl) on a handle, through either verb family of the library: dril_normalize_* (Handle: a PPO handle on a device env
plug-in), dril_ext_normalize_* (Handle: a PPO handle on device-resident external envs; the methods carry the prefix ext_) and dril_sac_normalize_* (SacHandle).
The families have one shape, so the Python methods are defined once and installed per family."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import DrilNormalizeConfig

# the wrapper's keywords and their defaults, normalizeWrapperEnv.jl:71-80
DEFAULTS = dict(training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8)
KEYS = tuple(DEFAULTS)
_FLAGS = ("training", "norm_obs", "norm_reward")


def normalize_verbs(fn, data_prefix: str, name_prefix: str = ""):
    """class decorator: normalize_enable / normalize_config / normalize_set_training and <data_prefix>get_stats / set_stats / get_original / get_returns on a handle
    class with _h, _chk, _p, E and D, every name behind name_prefix; fn(self, verb) is the library function of the verb ("enable", "get_stats", ...)"""

    def normalize_enable(self, enabled: bool = True, **kw):
        """NormalizeWrapperEnv(env; training, norm_obs, norm_reward, clip_obs, clip_reward, gamma, epsilon) (normalizeWrapperEnv.jl:71-80) around the handle's envs:
        a fresh wrapper, or nothing when the handle already has this configuration (`training` apart, which is set); normalize_enable(False) switches it off"""
        for k in kw:                                                     # before the library is called
            if k not in KEYS:
                raise TypeError(f"NormalizeWrapperEnv has no keyword {k!r}")
        if not enabled:
            self._chk(fn(self, "enable")(self._h, None)); return
        c = DrilNormalizeConfig()
        self._chk(fn(self, "config_default")(C.byref(c)))
        for k, v in kw.items():
            setattr(c, k, int(v) if k in _FLAGS else float(v))
        self._chk(fn(self, "enable")(self._h, C.byref(c)))

    def normalize_config(self) -> dict:
        """the wrapper's keywords as the handle holds them (get_config)"""
        c = DrilNormalizeConfig()
        self._chk(fn(self, "get_config")(self._h, C.byref(c)))
        return {k: bool(getattr(c, k)) if k in _FLAGS else getattr(c, k) for k in KEYS}

    def normalize_set_training(self, training: bool):
        """set_training(env, training) (normalizeWrapperEnv.jl:245-249)"""
        self._chk(fn(self, "set_training")(self._h, int(bool(training))))

    def get_stats(self) -> dict:
        """RunningMeanStd fields of the wrapper (normalizeWrapperEnv.jl:8-19); the keys of Handle.norm_get_stats"""
        om = np.empty(self.D, np.float32); ov = np.empty(self.D, np.float32)
        oc, rc = C.c_int64(), C.c_int64(); rm, rv = C.c_float(), C.c_float()
        self._chk(fn(self, "get_stats")(self._h, self._p(om), self._p(ov), C.byref(oc), C.byref(rm), C.byref(rv), C.byref(rc)))
        return dict(obs_mean=om, obs_var=ov, obs_count=oc.value, ret_mean=rm.value, ret_var=rv.value, ret_count=rc.value)

    def set_stats(self, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count):
        om = np.ascontiguousarray(obs_mean, np.float32).reshape(-1); ov = np.ascontiguousarray(obs_var, np.float32).reshape(-1)
        if om.size != self.D or ov.size != self.D:
            raise ValueError(f"obs_mean / obs_var must hold {self.D} values")
        self._chk(fn(self, "set_stats")(self._h, self._p(om), self._p(ov), int(obs_count), float(ret_mean), float(ret_var), int(ret_count)))

    def get_original(self):
        """-> (get_original_obs (E, D), get_original_rewards (E)), normalizeWrapperEnv.jl:220-222"""
        obs = np.empty((self.E, self.D), np.float32); rew = np.empty(self.E, np.float32)
        self._chk(fn(self, "get_original")(self._h, self._p(obs), self._p(rew)))
        return obs, rew

    def get_returns(self) -> np.ndarray:
        """env.returns: the discounted running return per env behind ret_rms"""
        r = np.empty(self.E, np.float32)
        self._chk(fn(self, "get_returns")(self._h, self._p(r)))
        return r

    def install(cls):
        for f in (normalize_enable, normalize_config, normalize_set_training):
            setattr(cls, name_prefix + f.__name__, f)
        for f in (get_stats, set_stats, get_original, get_returns):
            setattr(cls, name_prefix + data_prefix + f.__name__, f)
        return cls
    return install
