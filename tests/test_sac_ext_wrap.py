"""CPU: NormalizeWrapperEnv / MonitorWrapperEnv on a DRIL_ENV_EXTERNAL SAC handle over device-resident arrays (dril_sac_ext_normalize_* / dril_sac_ext_monitor_* /
dril_sac_ext_collection_begin / dril_sac_ext_wrap_info, docs/sac.md last section), without a GPU.

  * every new symbol is exported by the built library, declared in include/dril_sac.h and typed in _capi.py; the library exports as many dril_sac_ext_* symbols as the
    header declares; struct dril_sac_ext_wrap_info has the layout of its ctypes mirror (a C compile of the header);
  * null-handle calls return before any GPU work;
  * tools/check_shim.py accepts the Julia shim's new ccalls;
  * tests/sac_ext_wrap_ref.py's ExtVerbs — the verb-level call order begin / act / push, which the GPU tests use as the expected ring — reproduces
    tests/sac_normalize_ref.py's replay_through over the same script, bit for bit, for 8 collections x 1 step and 2 x 4 steps, and refuses an act without a begin;
  * the wrappers recorded on a DeviceArrayParallelEnv reach the handle _sac_train_device_arrays drives (a stub handle: no GPU)."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import sac_normalize_ref as ref
from ext_wrap_ref import Monitor
from sac_ext_wrap_ref import ExtVerbs, NotBegun, run_script
from test_gpu_ext_wrap import _script

ROOT = Path(__file__).resolve().parents[1]
F = np.float32
NEW = ("ext_normalize_enable", "ext_normalize_get_config", "ext_normalize_set_training", "ext_normalize_get_stats", "ext_normalize_set_stats", "ext_normalize_get_original",
       "ext_normalize_get_returns", "ext_normalize_reset", "ext_collection_begin", "ext_monitor_enable", "ext_monitor_get_stats", "ext_wrap_info")
FIELDS = ("normalize_on", "monitor_on", "monitor_window", "reserved0", "launches_act", "launches_push", "allocations", "reserved")
KW = dict(clip_obs=1.25, clip_reward=0.75, gamma=0.9, epsilon=1e-6)


def test_symbols_are_exported_declared_and_typed(pkg, tmp_path):
    capi = pkg._capi
    lib = capi.load_library()
    header = (ROOT / "include" / "dril_sac.h").read_text()
    declared = set(re.findall(r"^int32_t (dril_sac_ext_\w+)\(", header, re.M))
    nm = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dril_sac_ext_\w+)$", nm, re.M))
    assert exported == declared and len(exported) == len(declared) >= len(NEW) + 5, (sorted(exported - declared), sorted(declared - exported))
    for v in NEW:
        name = "dril_sac_" + v
        assert name in declared and name in capi.EXPORTED_SYMBOLS and v in capi._SAC_SIG and hasattr(lib, name), name
    P = C.c_void_p
    for v in ("enable", "get_config", "set_training", "get_stats", "set_stats", "get_original", "get_returns"):   # the contracts of the verbs of the same names
        assert getattr(lib, "dril_sac_ext_normalize_" + v).argtypes == getattr(lib, "dril_sac_normalize_" + v).argtypes, v
    assert lib.dril_sac_ext_normalize_reset.argtypes == [P, P] and lib.dril_sac_ext_collection_begin.argtypes == [P]
    assert lib.dril_sac_ext_monitor_enable.argtypes == lib.dril_sac_monitor_enable.argtypes and lib.dril_sac_ext_monitor_get_stats.argtypes == lib.dril_sac_monitor_get_stats.argtypes
    # prototypes and the struct, as a C compiler reads the header
    uses = """
    int32_t (*f1)(dril_sac_handle*, const dril_sac_normalize_config*) = dril_sac_ext_normalize_enable;
    int32_t (*f2)(dril_sac_handle*, void*) = dril_sac_ext_normalize_reset;
    int32_t (*f3)(dril_sac_handle*) = dril_sac_ext_collection_begin;
    int32_t (*f4)(dril_sac_handle*, int32_t) = dril_sac_ext_monitor_enable;
    int32_t (*f5)(dril_sac_handle*, float*, float*, int32_t*) = dril_sac_ext_monitor_get_stats;
    int32_t (*f6)(const dril_sac_handle*, struct dril_sac_ext_wrap_info*) = dril_sac_ext_wrap_info;
    f1 = dril_sac_normalize_enable; f4 = dril_sac_monitor_enable; f5 = dril_sac_monitor_get_stats;
    if (!f1 || !f2 || !f3 || !f4 || !f5 || !f6) return 1;
    """
    body = 'printf("%zu", sizeof(struct dril_sac_ext_wrap_info));' + "".join(f'printf(" %zu", offsetof(struct dril_sac_ext_wrap_info, {f}));' for f in FIELDS)
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_sac.h"\nint main(){' + uses + body + "return 0;}")
    subprocess.run(["gcc", "-Wall", "-Werror", "-Wno-unused-variable", "-I", str(ROOT / "include"), str(src), "-o", str(exe), "-Wl,--unresolved-symbols=ignore-all"], check=True)
    layout = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    K = capi.DrilSacExtWrapInfo
    assert [C.sizeof(K)] + [getattr(K, f).offset for f in FIELDS] == layout and tuple(n for n, _ in K._fields_) == FIELDS


def test_null_handle_returns_before_any_gpu_work(pkg):
    capi = pkg._capi
    lib, NI = capi.load_library(), capi.ERR_NOT_INITIALISED
    cfg = capi.DrilSacNormalizeConfig()
    assert lib.dril_sac_normalize_config_default(C.byref(cfg)) == capi.OK
    info = capi.DrilSacExtWrapInfo(); info.allocations = 77
    assert lib.dril_sac_ext_normalize_enable(None, C.byref(cfg)) == NI and lib.dril_sac_ext_normalize_enable(None, None) == NI
    assert lib.dril_sac_ext_normalize_get_config(None, C.byref(cfg)) == NI and lib.dril_sac_ext_normalize_set_training(None, 1) == NI
    assert lib.dril_sac_ext_normalize_get_stats(None, None, None, None, None, None, None) == NI and lib.dril_sac_ext_normalize_set_stats(None, None, None, 0, 0.0, 1.0, 0) == NI
    assert lib.dril_sac_ext_normalize_get_original(None, None, None) == NI and lib.dril_sac_ext_normalize_get_returns(None, None) == NI
    assert lib.dril_sac_ext_normalize_reset(None, None) == NI and lib.dril_sac_ext_collection_begin(None) == NI
    assert lib.dril_sac_ext_monitor_enable(None, 3) == NI and lib.dril_sac_ext_monitor_get_stats(None, None, None, None) == NI
    assert lib.dril_sac_ext_wrap_info(None, C.byref(info)) == NI and info.allocations == 77
    assert {"ext_normalize_enable", "ext_normalize_config", "ext_normalize_set_training", "ext_normalize_get_stats", "ext_normalize_set_stats", "ext_normalize_get_original",
            "ext_normalize_get_returns", "ext_normalize_reset", "ext_collection_begin", "ext_monitor_enable", "ext_monitor_stats", "ext_wrap_info"} <= set(dir(pkg.SacHandle))
    assert set(dir(pkg.SacHandle)) >= {m for m in dir(pkg.Handle) if m.startswith(("ext_normalize_", "ext_monitor_"))}   # named after the PPO handle's


def test_check_shim_accepts_the_new_ccalls():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0 and "check_shim: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    shim = (ROOT / "dril.jl_amd" / "julia" / "DRiLHIP_sac.jl").read_text()
    for v in NEW:
        assert ":dril_sac_" + v + "," in shim, v


@pytest.mark.parametrize("norm_obs,norm_reward", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("T,k", [(1, 8), (4, 2)])
@pytest.mark.parametrize("E,D", [(5, 1), (5, 24), (257, 133), (257, 300)])
def test_verb_order_reproduces_replay_through(E, D, T, k, norm_obs, norm_reward):
    sc = _script(E, D)
    kw = dict(KW, norm_obs=norm_obs, norm_reward=norm_reward)
    raw = run_script(ExtVerbs(), sc, T, k)                                           # no wrapper: the raw ring (terminal observation where truncated)
    assert np.array_equal(raw["obs"], sc["obs"][:T * k]) and np.isfinite(raw["next"]).all()
    tr = sc["trunc"][:T * k].astype(bool)
    assert np.array_equal(raw["next"][tr], sc["tobs"][:T * k][tr]) and np.array_equal(raw["next"][~tr], sc["obs"][1:T * k + 1][~tr])
    with np.errstate(invalid="ignore"):
        want = ref.replay_through(ref.Wrapper(E, D, **kw), raw, sc["obs"][T * k], T, k)
    v = ExtVerbs(ref.Wrapper(E, D, **kw), Monitor(E, 3))
    got = run_script(v, sc, T, k)
    for f in ("obs", "rew", "next"):
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f
    assert np.isfinite(got["next"]).all()
    assert v.w.obs_count == k * E * (T + 1) * norm_obs and v.w.ret_count == k * E * T * norm_reward
    if norm_obs:
        assert (np.abs(got["obs"]) == F(KW["clip_obs"])).any() and (np.abs(got["next"]) == F(KW["clip_obs"])).any()
    if norm_reward:
        assert (np.abs(got["rew"]) == F(KW["clip_reward"])).any()
    m = Monitor(E, 3)
    for t in range(T * k):
        m.act(sc["rew"][t], sc["term"][t], sc["trunc"][t])
    assert v.mon.stats() == m.stats() and m.stats()[2] == 3                          # raw rewards, whatever the normaliser does


def test_act_without_begin_and_the_null_terminal_obs_row():
    E, D = 5, 24
    sc = _script(E, D)
    v = ExtVerbs(ref.Wrapper(E, D, **KW))
    with pytest.raises(NotBegun):
        v.act(sc["obs"][0])
    v.collection_begin(); v.act(sc["obs"][0]); v.push(sc["rew"][0], sc["term"][0], sc["trunc"][0], sc["obs"][1], None)
    v.act(sc["obs"][1])                                                              # the same collection goes on
    row = v.push(sc["rew"][1], sc["term"][1], sc["trunc"][1], sc["obs"][2], None)   # truncated envs, terminal_obs = None: the sticky error, the normalised next obs
    assert row["sticky"] and np.array_equal(row["next"], v.w.normalize_obs(sc["obs"][2]))
    v.reset()
    assert not v.w.returns.any()
    with pytest.raises(NotBegun):
        v.act(sc["obs"][2])


class _StubHandle:
    """records what _sac_train_device_arrays asks of its handle; no library behind it"""
    discrete = False

    def __init__(self, E, A):
        self.E, self.A, self.calls = E, A, []

    def ext_device_info(self):
        return dict(pending_capacity=64, pending_updates=0, flushes=0, host_syncs=0)

    def flush(self):
        self.calls.append(("flush",)); return []

    def get_params(self):
        return self.params

    def set_params(self, p):
        self.params = np.asarray(p, F)

    def get_target_params(self):
        return self.target

    def set_target_params(self, p):
        self.target = p

    def get_log_ent_coef(self):
        return 0.0

    def replay_size(self):
        return 8

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **kw: self.calls.append((name, a, kw))


class _Arr:
    def __init__(self, shape):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr="<f4", data=(0x1000, False), version=2)


class _StubEnv:
    n_envs = 4

    def __init__(self, pkg):
        self.pkg = pkg

    def observation_space(self):
        return self.pkg.Box(low=(-1.0,) * 3, high=(1.0,) * 3)

    def action_space(self):
        return self.pkg.Box(low=(-1.0, -1.0), high=(1.0, 1.0))

    def reset_(self):
        pass

    def observe(self):
        return _Arr((4, 3))

    def act_(self, actions):
        return _Arr((4,)), _Arr((4,)), _Arr((4,)), None


def test_recorded_wrappers_reach_the_sac_handle(pkg, monkeypatch):
    sac_mod = sys.modules[pkg.SacHandle.__module__]
    env = pkg.NormalizeWrapperEnv(pkg.MonitorWrapperEnv(pkg.DeviceArrayParallelEnv(_StubEnv(pkg), empty=lambda shape, dt: _Arr(shape)), 7), **KW)
    assert env.ext_monitor_window == 7 and env.ext_normalize["clip_obs"] == 1.25 and env.wrapper_handle() is None
    stub = _StubHandle(4, 2)
    monkeypatch.setattr(sac_mod, "_sac_ext_handle", lambda agent, env_, alg, rb_handle=None: rb_handle or stub)
    alg = pkg.SAC(start_steps=0, train_freq=2, gradient_steps=1, batch_size=4, buffer_capacity=64)
    agent = pkg.SACAgent(pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(32, 32)), alg, seed=0)
    _, rb, _, timer = pkg.sac_train_(agent, env, alg, 3 * 2 * 4)
    names = [c[0] for c in stub.calls]
    assert rb.handle is stub and env.wrapper_handle() is stub
    i_mon, i_nz = names.index("ext_monitor_enable"), names.index("ext_normalize_enable")
    assert stub.calls[i_mon][1] == (7,) and stub.calls[i_nz][2] == env.ext_normalize and max(i_mon, i_nz) < names.index("ext_act_device")
    # a begin before every collection of train_freq steps, an act and a push per step
    assert timer["iterations"] == 3 and names.count("ext_collection_begin") == 3 and names.count("ext_act_device") == names.count("ext_push_device") == 6
    seq = [n for n in names if n in ("ext_collection_begin", "ext_act_device", "ext_push_device")]
    assert seq == ["ext_collection_begin", "ext_act_device", "ext_push_device", "ext_act_device", "ext_push_device"] * 3
    env.reset_()                                                                     # reset! of the wrapper goes to the handle that holds it
    assert stub.calls[-1][0] == "ext_normalize_reset"
    pkg.sac_train_(agent, env, alg, 2 * 4, replay_buffer=rb)                         # the handle comes back through the replay buffer: the same configuration again
    assert [c for c in stub.calls if c[0] == "ext_normalize_enable"][-1][2] == env.ext_normalize
    with pytest.raises(NotImplementedError, match="normalize"):                      # the keyword stays refused for external envs
        pkg.sac_train_(agent, env, alg, 8, normalize=dict())
