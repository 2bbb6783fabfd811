"""CPU: NormalizeWrapperEnv / MonitorWrapperEnv on a DRIL_ENV_EXTERNAL handle (dril_ext_normalize_* / dril_ext_monitor_* / dril_ext_wrap_info,
docs/external_envs.md section 10, "Wrappers on device-resident arrays"), without a GPU.

  * the prototypes and struct dril_ext_wrap_info: a C compile against include/dril_hip.h, compared with the ctypes mirror; dril_config, the ABI number and
    struct dril_ext_device_info have not moved;
  * null-handle calls, and the Python keyword check that runs before the library is called;
  * the per-env scalar rules the record kernel runs (dril.jl_amd/csrc/dril_ext_record.h), built with g++ and driven step by step, against
    tests/sac_normalize_ref.py's Wrapper (the `returns` recursion and reset) and a NumPy restatement of monitorWrapperEnv.jl (running sums, the window);
  * the Julia shim's new ccalls pass the static check, and the check catches a wrong arity of one of them."""
import ctypes as C
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import sac_normalize_ref as ref
from ext_wrap_ref import Monitor

ROOT = Path(__file__).resolve().parents[1]
F = np.float32
VERBS = ("dril_ext_normalize_enable", "dril_ext_normalize_get_config", "dril_ext_normalize_set_training", "dril_ext_normalize_get_stats", "dril_ext_normalize_set_stats",
         "dril_ext_normalize_get_original", "dril_ext_normalize_get_returns", "dril_ext_normalize_reset", "dril_ext_monitor_enable", "dril_ext_monitor_get_stats",
         "dril_ext_wrap_info")
FIELDS = ("normalize_on", "monitor_on", "monitor_window", "reserved0", "launches_act", "launches_record", "launches_finish", "allocations", "reserved")


def _layout(tmp_path, name, structs):
    body = "".join(f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {f}));' for f in fs) + 'printf("\\n");' for s, fs in structs)
    src = tmp_path / f"{name}.c"; exe = tmp_path / name
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_hip.h"\nint main(){' + body + "return 0;}")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    return [[int(x) for x in line.split()] for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]


def test_prototypes_and_struct_match_a_c_compile_of_the_header(pkg, tmp_path):
    capi = pkg._capi
    # the prototypes as the header's own comment states them: assigning to typed function pointers fails to compile on any mismatch (-Werror)
    uses = """
    int32_t (*f1)(dril_handle*, const dril_normalize_config*) = dril_ext_normalize_enable;
    int32_t (*f2)(dril_handle*, dril_normalize_config*) = dril_ext_normalize_get_config;
    int32_t (*f3)(dril_handle*, int32_t) = dril_ext_normalize_set_training;
    int32_t (*f4)(dril_handle*, float*, float*, int64_t*, float*, float*, int64_t*) = dril_ext_normalize_get_stats;
    int32_t (*f5)(dril_handle*, const float*, const float*, int64_t, float, float, int64_t) = dril_ext_normalize_set_stats;
    int32_t (*f6)(dril_handle*, float*, float*) = dril_ext_normalize_get_original;
    int32_t (*f7)(dril_handle*, float*) = dril_ext_normalize_get_returns;
    int32_t (*f8)(dril_handle*, void*) = dril_ext_normalize_reset;
    int32_t (*f9)(dril_handle*, int32_t) = dril_ext_monitor_enable;
    int32_t (*f10)(dril_handle*, float*, float*, int32_t*) = dril_ext_monitor_get_stats;
    int32_t (*f11)(const dril_handle*, struct dril_ext_wrap_info*) = dril_ext_wrap_info;
    /* the families the new verbs borrow their signatures from */
    f1 = dril_normalize_enable; f2 = dril_normalize_get_config; f3 = dril_normalize_set_training; f4 = dril_normalize_get_stats; f5 = dril_normalize_set_stats;
    f6 = dril_normalize_get_original; f7 = dril_normalize_get_returns; f10 = dril_monitor_get_stats;
    if (!f1 || !f2 || !f3 || !f4 || !f5 || !f6 || !f7 || !f8 || !f9 || !f10 || !f11) return 1;
    """
    protos = tmp_path / "protos.c"
    protos.write_text('#include "dril_hip.h"\nint use(void){' + uses + "return 0;}")
    subprocess.run(["gcc", "-Wall", "-Werror", "-Wno-unused-variable", "-I", str(ROOT / "include"), "-c", str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    dev_fields = ("steps_device", "steps_host", "host_syncs", "per_dim_bounds", "launches", "reserved")
    wrap, dev, cfg = _layout(tmp_path, "layout", [("struct dril_ext_wrap_info", FIELDS), ("struct dril_ext_device_info", dev_fields), ("dril_config", ("abi_version", "monitor_window", "ext_obs_dim"))])
    K = capi.DrilExtWrapInfo
    assert [C.sizeof(K)] + [getattr(K, f).offset for f in FIELDS] == wrap and tuple(n for n, _ in K._fields_) == FIELDS
    KD = capi.DrilExtDeviceInfo
    assert [C.sizeof(KD)] + [getattr(KD, f).offset for f in dev_fields] == dev and dev == [40, 0, 4, 8, 12, 16, 24]       # as the parent commit's header lays it out
    KC = capi.DrilConfig
    assert [C.sizeof(KC)] + [getattr(KC, f).offset for f in ("abi_version", "monitor_window", "ext_obs_dim")] == cfg
    header = (ROOT / "include" / "dril_hip.h").read_text()
    assert "#define DRIL_ABI_VERSION 2u" in header and capi.ABI_VERSION == 2
    lib = capi.load_library()
    P = C.c_void_p
    for name in VERBS:
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS, name
    for new, old in (("enable", "enable"), ("get_config", "get_config"), ("set_training", "set_training"), ("get_stats", "get_stats"), ("set_stats", "set_stats"),
                     ("get_original", "get_original"), ("get_returns", "get_returns")):
        assert getattr(lib, "dril_ext_normalize_" + new).argtypes == getattr(lib, "dril_normalize_" + old).argtypes, new
    assert lib.dril_ext_normalize_reset.argtypes == [P, P] and lib.dril_ext_monitor_enable.argtypes == [P, C.c_int32]
    assert lib.dril_ext_monitor_get_stats.argtypes == lib.dril_monitor_get_stats.argtypes and lib.dril_ext_wrap_info.argtypes == [P, C.POINTER(K)]


def test_dril_config_has_the_parent_size(pkg, tmp_path):
    (size,), = _layout(tmp_path, "cfgsize", [("dril_config", ())])
    assert size == C.sizeof(pkg._capi.DrilConfig) == 232                             # sizeof(dril_config) at the parent commit


def test_null_handle_returns_before_any_gpu_work(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    NI = capi.ERR_NOT_INITIALISED
    cfg = capi.DrilNormalizeConfig()
    assert lib.dril_normalize_config_default(C.byref(cfg)) == capi.OK and cfg.training == 1 and cfg.clip_obs == 10.0
    info = capi.DrilExtWrapInfo(); info.allocations = 77
    assert lib.dril_ext_normalize_enable(None, C.byref(cfg)) == NI and lib.dril_ext_normalize_enable(None, None) == NI
    assert lib.dril_ext_normalize_get_config(None, C.byref(cfg)) == NI and lib.dril_ext_normalize_set_training(None, 1) == NI
    assert lib.dril_ext_normalize_get_stats(None, None, None, None, None, None, None) == NI
    assert lib.dril_ext_normalize_set_stats(None, None, None, 0, 0.0, 1.0, 0) == NI
    assert lib.dril_ext_normalize_get_original(None, None, None) == NI and lib.dril_ext_normalize_get_returns(None, None) == NI
    assert lib.dril_ext_normalize_reset(None, None) == NI
    assert lib.dril_ext_monitor_enable(None, 3) == NI and lib.dril_ext_monitor_get_stats(None, None, None, None) == NI
    assert lib.dril_ext_wrap_info(None, C.byref(info)) == NI and info.allocations == 77


class _NoLib:
    """stands where the library would be: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_python_keyword_checks_run_before_the_library(pkg):
    h = object.__new__(pkg.Handle)                                                    # no dril_create: no GPU here
    h.lib, h._h, h.E, h.D, h.A, h.discrete, h.T = _NoLib(), C.c_void_p(), 6, 3, 2, False, 2
    with pytest.raises(TypeError, match="clip"):
        h.ext_normalize_enable(clip=3)
    with pytest.raises(TypeError, match="clip"):
        h.normalize_enable(clip=3)                                                   # the plug-in family's method: the same rule
    with pytest.raises(ValueError, match="3 values"):
        h.ext_normalize_set_stats(np.zeros(2), np.ones(2), 0, 0.0, 1.0, 0)
    for name in ("ext_normalize_enable", "ext_normalize_config", "ext_normalize_set_training", "ext_normalize_get_stats", "ext_normalize_set_stats",
                 "ext_normalize_get_original", "ext_normalize_get_returns", "ext_normalize_reset", "ext_monitor_enable", "ext_monitor_stats", "ext_wrap_info"):
        assert callable(getattr(pkg.Handle, name)), name
    # the wrapper functions: a HostParallelEnv stays refused, with a message that says where its wrapper belongs
    host = object.__new__(pkg.HostParallelEnv)
    for wrap in (lambda: pkg.NormalizeWrapperEnv(host), lambda: pkg.MonitorWrapperEnv(host, 5)):
        with pytest.raises(TypeError, match="on the host"):
            wrap()


class _Env:
    n_envs = 4

    def __init__(self, pkg):
        self.pkg = pkg

    def observation_space(self):
        return self.pkg.Box(low=[-1.0] * 3, high=[1.0] * 3)

    def action_space(self):
        return self.pkg.Discrete(2)

    def reset_(self):
        pass

    def observe(self):
        return None

    def act_(self, actions):
        return None


def test_wrapper_functions_record_the_wrapper_on_a_device_array_env(pkg):
    env = pkg.DeviceArrayParallelEnv(_Env(pkg))
    assert env.ext_normalize is None and env.ext_monitor_window == 0
    out = pkg.NormalizeWrapperEnv(pkg.MonitorWrapperEnv(env, 7), training=False, clip_obs=1.25, gamma=0.9)
    assert out is env and env.ext_monitor_window == 7                                 # the same object, the wrappers recorded; bind switches them on
    assert env.ext_normalize == dict(training=False, norm_obs=True, norm_reward=True, clip_obs=1.25, clip_reward=10.0, gamma=0.9, epsilon=1e-8)
    assert pkg.host._normalize_kw(env) is env.ext_normalize
    env.reset_()                                                                     # no handle yet: the env's own reset alone


# ---- the record kernel's per-env rules against the reference wrapper and a restatement of the monitor ---------------------------------------------------
_DRIVER = r'''
#include <stdint.h>
#include "dril_ext_record.h"
using namespace dril;
extern "C" {
// one env step of E envs as the kernels run it: the recursion (norm_moments_kernel's line), then env e's thread of ext_norm_record_kernel.  training: the recursion
// runs.  ep_ret / ep_len: the step's row (written where the episode ended).  Returns the sticky error word
int step(int E, float gamma, int training, int has_tobs, const float* rew, const uint8_t* term, const uint8_t* trunc,
         float* returns, float* cur_ret, int32_t* cur_len, uint8_t* flags, float* ep_ret, int32_t* ep_len) {
    int err = 0;
    if (training) for (int e = 0; e < E; ++e) returns[e] = xr_returns_step(returns[e], gamma, rew[e]);
    for (int e = 0; e < E; ++e) {
        const bool te = term[e] != 0, tr = trunc[e] != 0, done = te || tr;
        flags[e] = xr_flags(te, tr);
        if (xr_sticky(tr, has_tobs != 0)) err = 1;
        returns[e] = xr_returns_reset(returns[e], done);
        xr_monitor(rew[e], done, cur_ret[e], cur_len[e], ep_ret + e, ep_len + e);
    }
    return err;
}
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("ext_record")
    src = d / "drive.cpp"; src.write_text(_DRIVER)
    so = d / "drive.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / "dril.jl_amd" / "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.step.restype = C.c_int
    lib.step.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 9
    return lib


def _script(E, steps, seed):
    rng = np.random.default_rng(seed)
    rew = rng.standard_normal((steps, E)).astype(F)
    term = (rng.random((steps, E)) < 0.2).astype(np.uint8); trunc = (rng.random((steps, E)) < 0.2).astype(np.uint8)
    term[1, 0] = trunc[1, 0] = 1                                                     # terminated and truncated in the same step
    return rew, term, trunc


@pytest.mark.parametrize("training", [True, False])
def test_record_rules_match_the_reference_wrapper_and_the_monitor(driver, training):
    steps, W, gamma = 12, 3, 0.9
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for E in range(1, 41):
        rew, term, trunc = _script(E, steps, 100 + E)
        w = ref.Wrapper(E, 1, training=training, gamma=gamma); mon = Monitor(E, W)
        returns, cur_ret, cur_len = np.zeros(E, F), np.zeros(E, F), np.zeros(E, np.int32)
        window, finished = [], 0
        for t in range(steps):
            flags, ep_ret, ep_len = np.zeros(E, np.uint8), np.full(E, np.nan, F), np.full(E, -1, np.int32)
            has_tobs = int(t % 2 == 0)
            err = driver.step(E, gamma, int(training), has_tobs, p(rew[t]), p(term[t]), p(trunc[t]), p(returns), p(cur_ret), p(cur_len), p(flags), p(ep_ret), p(ep_len))
            w.act(rew[t], term[t], trunc[t], np.zeros((E, 1), F)); mon.act(rew[t], term[t], trunc[t])
            assert np.array_equal(flags, term[t] | (trunc[t] << 1)) and err == int(bool(trunc[t].any()) and not has_tobs)
            assert np.array_equal(returns.view(np.uint32), w.returns.view(np.uint32)), (E, t)          # the recursion and the reset, bit for bit (no contraction on either side)
            assert np.array_equal(cur_ret.view(np.uint32), mon.cur_ret.view(np.uint32)) and np.array_equal(cur_len, mon.cur_len)
            done = (flags != 0)
            assert np.isnan(ep_ret[~done]).all() and (ep_len[~done] == -1).all()     # rows of running episodes are not written
            for e in np.nonzero(done)[0]:                                            # what launch_monitor_collect does with the rows: (step, env) order
                window.append((ep_ret[e], int(ep_len[e]))); finished += 1
            window = window[-W:]
        if E >= 2:
            assert finished > W                                                      # the window is smaller than the number of finished episodes
        assert [(r.tobytes(), l) for r, l in window] == [(r.tobytes(), l) for r, l in mon.window], E   # lengths and float32 return sums exactly
        if not training:
            assert not returns.any()


def test_shim_check_passes_and_catches_a_wrong_arity_of_a_new_ccall(tmp_path):
    tool = ROOT / "tools" / "check_shim.py"
    shim_dir = ROOT / "dril.jl_amd" / "julia"
    r = subprocess.run([sys.executable, str(tool)], capture_output=True, text=True)
    assert r.returncode == 0 and "check_shim: ok" in r.stdout, r.stdout[-2000:]
    text = (shim_dir / "DRiLHIP_host_envs.jl").read_text()
    for verb in VERBS:
        assert f"ccall((:{verb}, LIB[])" in text, verb                               # a thin ccall for every new verb
    for f in shim_dir.glob("DRiLHIP*.jl"): shutil.copy(f, tmp_path / f.name)
    good = "ccall((:dril_ext_monitor_enable, LIB[]), Int32, (Ptr{Cvoid}, Int32)"
    assert good in text
    (tmp_path / "DRiLHIP_host_envs.jl").write_text(text.replace(good, good.replace("(Ptr{Cvoid}, Int32)", "(Ptr{Cvoid}, Int32, Int32)")))
    r = subprocess.run([sys.executable, str(tool), "--shim", str(tmp_path / "DRiLHIP.jl")], capture_output=True, text=True)
    assert r.returncode == 1 and "ccall dril_ext_monitor_enable" in r.stdout and "3 argument types" in r.stdout, r.stdout[-1500:]
    (tmp_path / "DRiLHIP_host_envs.jl").write_text(text.replace(good, good.replace("(Ptr{Cvoid}, Int32)", "(Ptr{Cvoid}, Int64)")))
    r = subprocess.run([sys.executable, str(tool), "--shim", str(tmp_path / "DRiLHIP.jl")], capture_output=True, text=True)
    assert r.returncode == 1 and "ccall dril_ext_monitor_enable" in r.stdout and "argument 2 Int64" in r.stdout, r.stdout[-1500:]
