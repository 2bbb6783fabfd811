"""CPU: SAC on device env plug-ins (dril_sac_create_with_env_module) without a GPU.

  * the library exports the two new entry points; include/dril_sac.h, dril.jl_amd/_capi.py and the Julia shim agree on them;
  * the path refusals of the new function come before any HIP call, with the shared loader's messages; dril_sac_config_default takes DRIL_ENV_MODULE;
  * the per-dimension TanhScaleAdapter of the SAC sampling kernels (dril.jl_amd/csrc/dril_sac_adapter.h, the lines the kernels compile) built for the host with g++
    against a NumPy statement of scale_to_space / from_env / rand(Box)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW = ("dril_sac_create_with_env_module", "dril_sac_env_module_info_of")


def test_the_two_entry_points_are_exported_and_header_capi_and_shim_agree(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    header = (ROOT / "include" / "dril_sac.h").read_text()
    shim = (ROOT / "dril.jl_amd" / "julia" / "DRiLHIP_sac.jl").read_text()
    for name in NEW:
        assert hasattr(lib, name), f"libdril_hip.so does not export {name}"
        assert re.search(rf"\bint32_t\s+{name}\s*\(", header), f"include/dril_sac.h does not declare {name}"
        assert name in capi.EXPORTED_SYMBOLS, f"_capi.py does not type {name}"
        assert f"(:{name}, LIB[])" in shim, f"the Julia shim has no ccall of {name}"
    assert getattr(lib, NEW[0]).argtypes == [C.POINTER(capi.DrilSacConfig), C.c_char_p, C.POINTER(C.c_void_p)]
    assert getattr(lib, NEW[1]).argtypes == [C.c_void_p, C.POINTER(capi.DrilEnvModuleInfo)]
    # the ABI numbers this change must not move
    assert capi.SAC_ABI_VERSION == 1 and "#define DRIL_SAC_ABI_VERSION 1u" in header
    r = subprocess.run(["python", str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]


def test_path_and_kind_refusals_come_before_any_gpu_work(pkg, tmp_path):
    capi = pkg._capi
    lib = capi.load_library()
    h = C.c_void_p()
    cfg = capi.DrilSacConfig()
    assert lib.dril_sac_config_default(C.byref(cfg), capi.ENV_MODULE) == capi.OK
    assert cfg.env_kind == capi.ENV_MODULE == 8 and cfg.episode_len == 0 and cfg.abi_version == capi.SAC_ABI_VERSION
    not_co = tmp_path / "notes.hsaco"; not_co.write_text("this is not a code object, however it is named\n")
    for path, message in ((None, b"null code_object_path"), (str(tmp_path / "missing.hsaco").encode(), b"cannot read code object"), (str(not_co).encode(), b"is not a code object")):
        assert lib.dril_sac_create_with_env_module(C.byref(cfg), path, C.byref(h)) == capi.ERR_INVALID_ARG
        err = lib.dril_sac_last_error(None)
        assert message in err and b"dril_sac_create_with_env_module" in err, err
    other = capi.DrilSacConfig()
    assert lib.dril_sac_config_default(C.byref(other), capi.ENV_PENDULUM) == capi.OK
    assert lib.dril_sac_create_with_env_module(C.byref(other), str(not_co).encode(), C.byref(h)) == capi.ERR_INVALID_ARG and b"DRIL_ENV_MODULE" in lib.dril_sac_last_error(None)
    bad = capi.DrilSacConfig(); bad.abi_version = 7; bad.env_kind = capi.ENV_MODULE
    assert lib.dril_sac_create_with_env_module(C.byref(bad), str(not_co).encode(), C.byref(h)) == capi.ERR_INVALID_ARG and b"abi_version" in lib.dril_sac_last_error(None)
    # dril_sac_create has no code object to load: it keeps refusing the kind and names the function that takes one
    assert lib.dril_sac_create(C.byref(cfg), C.byref(h)) == capi.ERR_UNSUPPORTED
    assert b"plug-in" in lib.dril_sac_last_error(None) and b"dril_sac_create_with_env_module" in lib.dril_sac_last_error(None)
    assert not h.value
    # the Python wrapper hands the library's status on
    with pytest.raises(pkg.DrilError) as e:
        pkg.SacHandle(cfg, env_module=not_co)
    assert e.value.code == capi.ERR_INVALID_ARG
    assert lib.dril_sac_env_module_info_of(None, None) == capi.ERR_NOT_INITIALISED


def test_make_sac_config_takes_the_spaces_of_a_plugin_and_refuses_a_discrete_one(pkg):
    """make_sac_config over a ModuleEnv description (no library call: the description is what dril_env_module_describe returns)"""
    capi = pkg._capi
    info = dict(plugin_abi=1, state_dim=9, obs_dim=12, action_dim=3, discrete=False, episode_len=100, name="Reacher3",
                action_low=np.array([-1, -0.5, 0], np.float32), action_high=np.array([1, 2, 3], np.float32))
    env = pkg.host.ModuleEnv("some.hsaco", info, 100)
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(64, 64))
    assert (layer.obs_dim, layer.act_dim) == (12, 3) and tuple(env.action_space().high) == (1.0, 2.0, 3.0)
    cfg = pkg.sac.make_sac_config(env, 8, pkg.SAC(), layer, seed=3)
    assert (cfg.env_kind, cfg.n_envs, cfg.episode_len, cfg.hidden1, cfg.seed) == (capi.ENV_MODULE, 8, 100, 64, 3)
    with pytest.raises(NotImplementedError, match="Discrete"):
        pkg.sac.make_sac_config(pkg.host.ModuleEnv("some.hsaco", dict(info, discrete=True), 100), 8, pkg.SAC(), layer)
    wrong = pkg.SACLayer(env.observation_space(), pkg.Box((-1.0,), (1.0,)), hidden_dims=(64, 64))
    with pytest.raises(ValueError, match="SACLayer"):
        pkg.sac.make_sac_config(env, 8, pkg.SAC(), wrong)


# ---- the adapter the kernels compile, on the host -----------------------------------------------------------------------------------------------------
_ADAPTER_SHIM = r'''
#include "dril_sac_adapter.h"
extern "C" {
void to_env(int n, int A, const float* raw, const float* low, const float* high, float* out) { for (int i = 0; i < n * A; ++i) out[i] = dril::sac_to_env(raw[i], low[i % A], high[i % A]); }
void scale(int n, int A, const float* t, const float* low, const float* high, float* out) { for (int i = 0; i < n * A; ++i) out[i] = dril::sac_scale_to_space(t[i], low[i % A], high[i % A]); }
void from_env(int n, int A, const float* act, const float* low, const float* high, float* out) { for (int i = 0; i < n * A; ++i) out[i] = dril::sac_from_env(act[i], low[i % A], high[i % A]); }
void rand_box(int n, int A, const float* u, const float* low, const float* high, float* out) { for (int i = 0; i < n * A; ++i) out[i] = dril::sac_rand_box(u[i], low[i % A], high[i % A]); }
}
'''


def test_per_dimension_tanh_scale_adapter_follows_numpy(tmp_path):
    src = tmp_path / "adapter.cpp"; src.write_text(_ADAPTER_SHIM)
    so = tmp_path / "adapter.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", str(ROOT / "dril.jl_amd" / "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    f = np.float32
    low, high = np.array([-1, -0.5, 0, -2], f), np.array([1, 2, 3, 2], f)
    A, n = len(low), 4096
    rng = np.random.default_rng(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(name, x):
        out = np.empty_like(x)
        getattr(lib, name)(n, A, p(x), p(low), p(high), p(out))
        return out

    # scale_to_space(t, space) = low + (t + 1) (high - low) / 2, default_adapters.jl:13-21; the kernels' operation order stated in float32
    t = rng.uniform(-1, 1, (n, A)).astype(f); t[0] = -1; t[1] = 1
    got = call("scale", t)
    assert np.array_equal(got, t * (high - low) / f(2) + (low + high) / f(2))
    assert np.allclose(got, low + (t.astype(np.float64) + 1) * (high.astype(np.float64) - low) / 2, atol=1e-6)
    assert np.array_equal(got[0], low) and np.array_equal(got[1], high)
    # to_env squashes first (the adapter applies tanh to the already squashed sample, as the reference has it): strictly inside the Box
    raw = np.tanh(rng.normal(0, 2, (n, A))).astype(f)
    env = call("to_env", raw)
    assert np.allclose(env, low + (np.tanh(raw.astype(np.float64)) + 1) * (high.astype(np.float64) - low) / 2, atol=1e-6)
    assert (env > low).all() and (env < high).all()
    # from_env is the inverse of scale_to_space (default_adapters.jl:24-30)
    back = call("from_env", got)
    assert np.array_equal(back, f(2) * (got - (low + high) / f(2)) / (high - low))
    assert np.allclose(back, t, atol=1e-6) and np.allclose(call("from_env", env), np.tanh(raw), atol=1e-6)
    # rand(action_space): low + u (high - low) per dimension, inside the Box for u in [0, 1)
    u = rng.random((n, A)).astype(f); u[0] = 0; u[1] = np.nextafter(f(1), f(0))
    r = call("rand_box", u)
    assert np.array_equal(r, low + u * (high - low)) and (r >= low).all() and (r <= high).all()
    # one pair in every entry (the built-in and external envs) is the scalar form the kernels had before the table: same float32 operations
    lo1, hi1 = np.full(A, -2, f), np.full(A, 2, f)
    out = np.empty_like(raw); lib.to_env(n, A, p(raw), p(lo1), p(hi1), p(out))
    assert np.allclose(out, np.tanh(raw) * (f(2) - f(-2)) / f(2) + (f(-2) + f(2)) / f(2), atol=5e-7)
