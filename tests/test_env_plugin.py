"""CPU: device env plug-ins (include/device/dril_env_plugin.h, DRIL_ENV_MODULE) without a GPU.

  * the examples cross-compile for gfx950 and their code objects define the three kernels and the descriptor; what the library cannot take fails at the PLUG-IN's compile;
  * the header's host build (-DDRIL_ENV_PLUGIN_HOST, g++: the same wrapper over a serial loop) of the CartPole / Pendulum twins against the CPU oracle's env verbs, and of
    reacher3 against a NumPy float32 twin; the wrapper's step order asserted directly;
  * the host-side checks of the library: struct layout, path / magic refusals before any HIP call, dril_create naming the right entry point."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
ENVS = ROOT / "examples" / "envs"
HIPCC = "/opt/rocm/bin/hipcc"
GENCO = [HIPCC, "--genco", "--offload-arch=gfx950", "--no-gpu-bundle-output", "-O3", "-fno-slp-vectorize", "-std=c++17", "-I", str(ROOT / "include")]
_PV = C.c_void_p


class Args(C.Structure):
    """struct DrilEnvPluginArgs, include/device/dril_env_plugin.h"""
    _fields_ = [("E", C.c_int32), ("episode_len", C.c_int32), ("fixed_len", C.c_int32), ("action_start", C.c_int32), ("seed0", C.c_uint64),
                ("actions", _PV), ("state", _PV), ("step_count", _PV), ("episode", _PV), ("gstep", _PV), ("rewards", _PV), ("terminated", _PV), ("truncated", _PV),
                ("flags", _PV), ("terminal_obs", _PV), ("obs", _PV), ("mon_cur_ret", _PV), ("mon_cur_len", _PV), ("ep_ret", _PV), ("ep_len", _PV)]


class Desc(C.Structure):
    """struct DrilEnvPluginDesc"""
    _fields_ = [("abi_version", C.c_uint32), ("args_size", C.c_uint32), ("S", C.c_int32), ("D", C.c_int32), ("A", C.c_int32), ("discrete", C.c_int32),
                ("episode_len", C.c_int32), ("reserved", C.c_int32), ("action_low", C.c_float * 64), ("action_high", C.c_float * 64), ("name", C.c_char * 64)]


class HostEnv:
    """E envs of a plug-in's host build, driven like Handle's env verbs"""

    def __init__(self, name, tmp, E, seed, episode_len=0, action_start=1, monitor=False, fixed_len=False, flags=("-ffp-contract=off",)):
        so = Path(tmp) / f"{name}_host.so"
        subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-x", "c++", "-DDRIL_ENV_PLUGIN_HOST", *flags, "-I", str(ROOT / "include"),
                        str(ENVS / f"{name}_plugin.hip"), "-o", str(so)], check=True)
        self.lib = C.CDLL(str(so))
        self.desc = Desc.in_dll(self.lib, "dril_env_plugin_desc")
        assert self.desc.abi_version == 1 and self.desc.args_size == C.sizeof(Args)
        d = self.desc
        self.E, self.S, self.D, self.A, self.discrete = E, d.S, d.D, d.A, bool(d.discrete)
        self.state = np.zeros((E, d.S), np.float32); self.sc = np.zeros(E, np.int32); self.ep = np.zeros(E, np.uint32); self.gs = np.zeros(E, np.uint32)
        self.mon_ret = np.zeros(E, np.float32); self.mon_len = np.zeros(E, np.int32); self.ep_ret = np.full(E, np.nan, np.float32); self.ep_len = np.full(E, -1, np.int32)
        self.base = dict(E=E, episode_len=episode_len or d.episode_len, fixed_len=int(fixed_len), action_start=action_start, seed0=seed)
        self.monitor = monitor

    def _args(self, **kw):
        p = lambda a: a.ctypes.data_as(_PV)
        a = Args(**self.base, state=p(self.state), step_count=p(self.sc), episode=p(self.ep), gstep=p(self.gs))
        if self.monitor:
            a.mon_cur_ret, a.mon_cur_len, a.ep_ret, a.ep_len = p(self.mon_ret), p(self.mon_len), p(self.ep_ret), p(self.ep_len)
        for k, v in kw.items():
            setattr(a, k, p(v))
        return a

    def reset(self):
        self.lib.dril_env_plugin_host_reset(C.byref(self._args()))

    def observe(self):
        obs = np.empty((self.E, self.D), np.float32)
        self.lib.dril_env_plugin_host_observe(C.byref(self._args(obs=obs)))
        return obs

    def step(self, actions):
        actions = np.ascontiguousarray(actions, np.int32 if self.discrete else np.float32)
        E = self.E
        rew = np.empty(E, np.float32); term = np.empty(E, np.uint8); trunc = np.empty(E, np.uint8); fl = np.empty(E, np.uint8)
        tobs = np.zeros((E, self.D), np.float32); nxt = np.empty((E, self.D), np.float32)
        self.lib.dril_env_plugin_host_step(C.byref(self._args(actions=actions, rewards=rew, terminated=term, truncated=trunc, flags=fl, terminal_obs=tobs, obs=nxt)))
        assert np.array_equal(fl, term | (trunc << 1))                      # the BUF_FLAGS byte
        return rew, term.astype(bool), trunc.astype(bool), tobs, nxt


# ---- the examples as gfx950 code objects ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole", "pendulum", "reacher3"])
def test_examples_compile_for_gfx950_and_define_the_contract(name, tmp_path):
    co = tmp_path / f"{name}.hsaco"
    subprocess.run(GENCO + [str(ENVS / f"{name}_plugin.hip"), "-o", str(co)], check=True)
    assert co.read_bytes()[:4] == b"\x7fELF"
    syms = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "-s", str(co)], capture_output=True, text=True, check=True).stdout
    for s in ("dril_env_plugin_reset", "dril_env_plugin_observe", "dril_env_plugin_step"):
        assert f" {s}\n" in syms and f" {s}.kd\n" in syms, s
    line = next(l for l in syms.splitlines() if l.endswith(" dril_env_plugin_desc"))
    assert int(line.split()[2]) == C.sizeof(Desc) and "OBJECT" in line and "GLOBAL" in line


BAD = """#include "device/dril_env_plugin.h"
struct Bad {
    static constexpr int S = 2, D = 2, A = %d;
    static constexpr bool discrete = %s;
    static constexpr int episode_len = 10;
    %s
    static constexpr const char* name = "Bad";
    DRIL_ENV_FN static void reset(const DrilEnvRng&, float* st) { st[0] = st[1] = 0.f; }
    DRIL_ENV_FN static void observe(const float* st, float* obs) { obs[0] = st[0]; obs[1] = st[1]; }
    DRIL_ENV_FN static float step(float* st, const float*, int, bool* t) { *t = false; return 0.f; }
};
DRIL_ENV_PLUGIN(Bad)
"""


@pytest.mark.parametrize("A,discrete,bounds,message", [
    (65, "true", "", "A (action dims, or number of discrete actions) must be 1..64"),
    (2, "false", "", "a continuous env (discrete = false) must define static constexpr float action_low[A] and action_high[A]"),
])
def test_a_plugin_the_library_cannot_take_fails_at_its_own_compile(A, discrete, bounds, message, tmp_path):
    src = tmp_path / "bad.hip"
    src.write_text(BAD % (A, discrete, bounds))
    r = subprocess.run(GENCO + [str(src), "-o", str(tmp_path / "bad.hsaco")], capture_output=True, text=True)
    assert r.returncode != 0 and message in r.stderr, r.stderr[-2000:]
    ok = tmp_path / "ok.hip"
    ok.write_text(BAD % (2, "false", "static constexpr float action_low[A] = {-1, -1}, action_high[A] = {1, 1};"))       # the control: the same plug-in, acceptable
    subprocess.run(GENCO + [str(ok), "-o", str(tmp_path / "ok.hsaco")], check=True)


# ---- host builds of the twins against the CPU oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("cartpole", 0), ("pendulum", 1)])
def test_host_build_of_a_twin_follows_the_oracle_env(pkg, oracle_mod, name, kind, tmp_path):
    E, L, seed = 8, 60, 5
    cfg = pkg._capi.default_config(kind); cfg.n_envs, cfg.n_steps, cfg.batch_size, cfg.episode_len = E, 2, E, L
    o = oracle_mod.Oracle(cfg); o.env_reset(seed)
    m = HostEnv(name, tmp_path, E, seed, episode_len=L, flags=("-march=x86-64-v3",)); m.reset()   # the oracle's own target (oracle/Makefile): products contract into FMAs, as on the device
    assert np.array_equal(o.env_get_state()[0], m.state)                      # reset states: the same Philox words, the same conversion
    tol = 1e-5 if kind == 0 else 3e-4     # two compilers, two libm: f32 rounding differences grow along a Pendulum episode (|theta_dot| up to 8) until the next reset re-synchronises
    rng = np.random.default_rng(0)
    n_term = n_trunc = 0
    for t in range(540):
        np.testing.assert_allclose(m.observe(), o.env_observe(), atol=tol, rtol=tol)
        if kind == 0:
            act = np.empty(E, np.int32); act[: E // 2] = 1 + (t // 7) % 2; act[E // 2:] = 1 + t % 2     # half the poles fall, half balance to the time limit
        else:
            act = rng.uniform(-3, 3, (E, 1)).astype(np.float32)
        ro, to, uo, oo = o.env_step(np.clip(act, -2, 2) if kind == 1 else act)   # the oracle's verb takes env-space actions; the plug-in wrapper clamps itself
        rm, tm, um, om, _ = m.step(act)
        assert np.array_equal(to, tm) and np.array_equal(uo, um), t
        np.testing.assert_allclose(rm, ro, atol=tol, rtol=tol)
        np.testing.assert_allclose(om[um], oo[uo], atol=tol, rtol=tol)      # terminal observations
        so, co = o.env_get_state()
        assert np.array_equal(co, m.sc)
        done = to | uo
        assert np.array_equal(so[done], m.state[done])                         # auto-reset episodes: bit-identical fresh states
        n_term += int(to.sum()); n_trunc += int(uo.sum())
    assert n_trunc > 0 and (kind != 0 or n_term > 0)
    assert (m.gs == 540).all() and (m.ep > 0).all()


# ---- reacher3 against NumPy, and the wrapper's step order ---------------------------------------------------------------------------------------------
def _reacher_step(st, act):
    f = np.float32
    st = st.astype(f).copy(); a = np.clip(act.astype(f), f(-1), f(1))
    dist2 = np.zeros(len(st), f); act2 = np.zeros(len(st), f); out = np.zeros(len(st), bool)
    for i in range(3):
        v = (st[:, 3 + i] + f(0.1) * a[:, i]) * f(0.95)
        p = st[:, i] + f(0.1) * v
        st[:, i] = p; st[:, 3 + i] = v
        d = p - st[:, 6 + i]
        dist2 = dist2 + d * d
        act2 = act2 + a[:, i] * a[:, i]
        out |= (p < f(-2)) | (p > f(2))
    return st, -dist2 - f(0.01) * act2, out


def _reacher_obs(st):
    return np.concatenate([st, st[:, 0:3] - st[:, 6:9]], axis=1).astype(np.float32)


def _philox_u01(oracle_mod, seed, episode, block):
    w = np.zeros(4, np.uint32)
    oracle_mod.lib().orc_philox(seed, episode, 0, 0, block, w.ctypes.data_as(_PV))
    return (w >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0)


def test_host_build_of_reacher3_follows_the_numpy_twin_and_the_wrapper_keeps_its_order(oracle_mod, tmp_path):
    E, L, seed = 6, 7, 100
    m = HostEnv("reacher3", tmp_path, E, seed, episode_len=L, monitor=True); m.reset()
    assert (m.S, m.D, m.A, m.discrete, m.desc.episode_len, m.desc.name) == (9, 12, 3, False, 100, b"Reacher3")
    assert list(m.desc.action_low[:3]) == [-1.0] * 3 and list(m.desc.action_high[:3]) == [1.0] * 3

    def fresh(e, episode):                                                     # Reacher3::reset from stream 0: key seed + e, counter (episode, 0, 0, block)
        u0, u1 = _philox_u01(oracle_mod, seed + e, episode, 0), _philox_u01(oracle_mod, seed + e, episode, 1)
        return np.concatenate([u0[:3] - np.float32(0.5), np.zeros(3, np.float32), u1[:3] * np.float32(2) - np.float32(1)])
    for e in range(E):
        assert np.array_equal(m.state[e], fresh(e, 0))
    rng = np.random.default_rng(3)
    st = m.state.copy(); cur_ret = np.zeros(E, np.float32); cur_len = np.zeros(E, np.int64); episode = np.zeros(E, np.int64)
    m.state[0, 0] = st[0, 0] = np.float32(1.99); m.state[0, 3] = st[0, 3] = np.float32(1.0)      # env 0 leaves the box at once: a termination
    saw_term = saw_trunc = False
    for t in range(3 * L + 2):
        assert np.array_equal(m.observe(), _reacher_obs(st))
        act = rng.uniform(-1.5, 1.5, (E, 3)).astype(np.float32)
        raw = act.copy()
        want_st, want_r, want_term = _reacher_step(st, act)
        sc_before = m.sc.copy()
        rew, term, trunc, tobs, nxt = m.step(act)
        assert np.array_equal(act, raw)                                        # the raw action stays as it was: the clamp happens on a copy
        assert np.array_equal(rew, want_r) and np.array_equal(term, want_term)
        assert np.array_equal(trunc, sc_before + 1 >= L)
        cur_ret += rew; cur_len += 1
        done = term | trunc
        assert np.array_equal(tobs[trunc], _reacher_obs(want_st)[trunc])       # terminal observation: of the state after the step, BEFORE the reset
        assert not tobs[~trunc].any()                                          # ... and only where truncated
        for e in np.nonzero(done)[0]:
            assert m.ep_ret[e] == cur_ret[e] and m.ep_len[e] == cur_len[e]     # the finished episode goes to the monitor's arrays
            cur_ret[e] = 0; cur_len[e] = 0; episode[e] += 1
            want_st[e] = fresh(e, episode[e])                                  # the next episode starts from the stream's next counter
        assert np.array_equal(m.state, want_st) and np.array_equal(nxt, _reacher_obs(want_st))     # next observation: of the fresh state where one started
        assert np.array_equal(m.mon_ret, cur_ret) and np.array_equal(m.mon_len, cur_len)             # the monitor's sums restart with the episode
        assert np.array_equal(m.ep, episode) and (m.sc[done] == 0).all() and np.array_equal(m.sc[~done], sc_before[~done] + 1)
        assert (m.gs == t + 1).all()                                           # gstep counts steps since reset!: never reset by an episode's end
        st = want_st; saw_term |= term.any(); saw_trunc |= trunc.any()
    assert saw_term and saw_trunc
    f = HostEnv("reacher3", tmp_path, 2, seed, episode_len=3, fixed_len=True); f.reset()
    f.state[:, 0] = 5.0                                                        # outside the box, but fixed_length_episodes suppresses termination
    _, term, trunc, _, _ = f.step(np.zeros((2, 3), np.float32))
    assert not term.any() and not trunc.any()


# ---- the library's host side ---------------------------------------------------------------------------------------------------------------------------
def test_module_info_layout_matches_c(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %d\\n", sizeof(dril_env_module_info),'
                   ' offsetof(dril_env_module_info, episode_len), offsetof(dril_env_module_info, action_low), offsetof(dril_env_module_info, action_high),'
                   ' offsetof(dril_env_module_info, name), (int)DRIL_ENV_MODULE);return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    sz, o_len, o_lo, o_hi, o_name, kind = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    K = pkg._capi.DrilEnvModuleInfo
    assert (C.sizeof(K), K.episode_len.offset, K.action_low.offset, K.action_high.offset, K.name.offset) == (sz, o_len, o_lo, o_hi, o_name)
    assert kind == pkg._capi.ENV_MODULE == 8


def test_path_checks_come_before_any_gpu_work(pkg, tmp_path):
    capi = pkg._capi
    lib = capi.load_library()
    h = C.c_void_p()
    cfg = capi.default_config(capi.ENV_MODULE)
    c2 = capi.DrilConfig()
    assert lib.dril_config_default(C.byref(c2), capi.ENV_MODULE) == capi.OK and c2.episode_len == cfg.episode_len == 0 and c2.env_kind == 8
    assert lib.dril_create(C.byref(cfg), C.byref(h)) == capi.ERR_INVALID_ARG and b"dril_create_with_env_module" in lib.dril_last_error(None)
    not_co = tmp_path / "notes.hsaco"; not_co.write_text("this is not a code object, however it is named\n")
    info = capi.DrilEnvModuleInfo()
    for path, message in ((None, b"null code_object_path"), (str(tmp_path / "missing.hsaco").encode(), b"cannot read code object"), (str(not_co).encode(), b"is not a code object")):
        assert lib.dril_create_with_env_module(C.byref(cfg), path, C.byref(h)) == capi.ERR_INVALID_ARG
        assert message in lib.dril_last_error(None), lib.dril_last_error(None)
        assert lib.dril_env_module_describe(path, 0, C.byref(info)) == capi.ERR_INVALID_ARG and message in lib.dril_last_error(None)
    other = capi.default_config(capi.ENV_CARTPOLE)
    assert lib.dril_create_with_env_module(C.byref(other), str(not_co).encode(), C.byref(h)) == capi.ERR_INVALID_ARG and b"DRIL_ENV_MODULE" in lib.dril_last_error(None)
    # NormalizeWrapperEnv on a plug-in env: refused with the library's message, through the C ABI and through the Python wrapper's Handle
    elf = tmp_path / "some.hsaco"; elf.write_bytes(b"\x7fELF" + bytes(60))
    cfg.norm_obs = 1
    assert lib.dril_create_with_env_module(C.byref(cfg), str(elf).encode(), C.byref(h)) == capi.ERR_UNSUPPORTED and b"NormalizeWrapperEnv" in lib.dril_last_error(None)
    with pytest.raises(pkg.DrilError) as e:
        pkg.Handle(cfg, env_module=elf)
    assert e.value.code == capi.ERR_UNSUPPORTED
    sc = capi.DrilSacConfig(); sc.abi_version = capi.SAC_ABI_VERSION; sc.env_kind = capi.ENV_MODULE
    assert lib.dril_sac_create(C.byref(sc), C.byref(h)) == capi.ERR_UNSUPPORTED and b"plug-in" in lib.dril_sac_last_error(None)
