"""CPU: the observation space and the ScalingWrapperEnv kernels of a device env plug-in (include/device/dril_env_plugin.h) without a GPU.

  * which symbols a code object and a host build get: an env without obs_low / obs_high exports exactly what the header gave it before the observation space existed;
    a declared space adds dril_env_plugin_obs_space; finite bounds on a continuous env add the two _scaled kernels; an infinite bound does not;
  * the host build's _observe_scaled / _step_scaled of the pendulum and reacher3 examples against NumPy float32 formulas written from scalingWrapperEnv.jl, over a
    few hundred steps with episode ends;
  * dril::scale_to_unit / unscale_from_unit (include/device/dril_scaling.h) against tests/golden/scaling_kats.json;
  * header, ctypes table and Julia shim agree on the new entry points; Python's ScalingWrapperEnv keeps refusing what it refused."""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_env_plugin import Args, Desc, GENCO

ROOT = Path(__file__).resolve().parents[1]
ENVS = ROOT / "examples" / "envs"
READELF = "/opt/rocm/llvm/bin/llvm-readelf"
_PV = C.c_void_p
f32 = np.float32

# a continuous env, D = 2, A = 1; %s: nothing, or the declaration of its observation space
SRC = """#include "device/dril_env_plugin.h"
struct Walk {
    static constexpr int S = 2, D = 2, A = 1;
    static constexpr bool discrete = false;
    static constexpr int episode_len = 7;
    static constexpr float action_low[A] = {-0.5f}, action_high[A] = {1.5f};
    %s
    static constexpr const char* name = "Walk";
    DRIL_ENV_FN static void reset(const DrilEnvRng& rng, float* st) { st[0] = DrilEnvRng::u01(rng.words(0).w[0]); st[1] = 0.f; }
    DRIL_ENV_FN static void observe(const float* st, float* obs) { obs[0] = st[0]; obs[1] = st[1]; }
    DRIL_ENV_FN static float step(float* st, const float* a, int, bool* t) { st[0] += a[0]; st[1] += 1.f; *t = st[0] > 3.f; return -st[0]; }
};
DRIL_ENV_PLUGIN(Walk)
"""
NO_SPACE = ""
FINITE = "static constexpr float obs_low[D] = {-4.f, 0.f}, obs_high[D] = {5.f, 7.f};"
INFINITE = "static constexpr float obs_low[D] = {-INFINITY, 0.f}, obs_high[D] = {5.f, 7.f};"
# what `llvm-readelf -s` listed for a plug-in before the observation space existed (the .kd objects are the kernel descriptors)
BEFORE = {"dril_env_plugin_desc", "dril_env_plugin_reset", "dril_env_plugin_reset.kd", "dril_env_plugin_observe", "dril_env_plugin_observe.kd",
          "dril_env_plugin_step", "dril_env_plugin_step.kd"}
SPACE = {"dril_env_plugin_obs_space", "dril_env_plugin_obs_space.kd"}
SCALED = {"dril_env_plugin_observe_scaled", "dril_env_plugin_observe_scaled.kd", "dril_env_plugin_step_scaled", "dril_env_plugin_step_scaled.kd"}


def _code_object_symbols(src: Path, out: Path) -> set:
    subprocess.run(GENCO + [str(src), "-o", str(out)], check=True)
    listing = subprocess.run([READELF, "-s", str(out)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in listing.splitlines() if "GLOBAL" in l and l.split()[-1].startswith("dril_")}


def _host_build(src: Path, so: Path) -> C.CDLL:
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-x", "c++", "-DDRIL_ENV_PLUGIN_HOST", "-ffp-contract=off", "-I", str(ROOT / "include"), str(src), "-o", str(so)], check=True)
    return C.CDLL(str(so))


@pytest.mark.parametrize("decl,extra", [(NO_SPACE, set()), (FINITE, SPACE | SCALED), (INFINITE, SPACE)])
def test_symbols_of_a_code_object_follow_the_declared_space(decl, extra, tmp_path):
    src = tmp_path / "walk.hip"
    src.write_text(SRC % decl)
    assert _code_object_symbols(src, tmp_path / "walk.hsaco") == BEFORE | extra
    lib = _host_build(src, tmp_path / "walk_host.so")
    for name in ("reset", "observe", "step"):
        assert hasattr(lib, f"dril_env_plugin_host_{name}")
    assert hasattr(lib, "dril_env_plugin_host_obs_space") == bool(extra)
    assert hasattr(lib, "dril_env_plugin_host_observe_scaled") == hasattr(lib, "dril_env_plugin_host_step_scaled") == (extra == SPACE | SCALED)
    d = Desc.in_dll(lib, "dril_env_plugin_desc")
    assert d.abi_version == 1 and d.args_size == C.sizeof(Args)          # DRIL_ENV_PLUGIN_ABI and the argument block did not move


@pytest.mark.parametrize("name,space,scaled", [("cartpole", True, False), ("pendulum", True, True), ("reacher3", True, True)])
def test_symbols_of_the_examples(name, space, scaled, tmp_path):
    got = _code_object_symbols(ENVS / f"{name}_plugin.hip", tmp_path / f"{name}.hsaco")
    assert got == BEFORE | (SPACE if space else set()) | (SCALED if scaled else set())


def test_a_misdeclared_space_fails_at_the_plugins_compile(tmp_path):
    src = tmp_path / "bad.hip"
    src.write_text(SRC % "static constexpr float obs_low[3] = {0.f, 0.f, 0.f}, obs_high[D] = {1.f, 1.f};")
    r = subprocess.run(GENCO + [str(src), "-o", str(tmp_path / "bad.hsaco")], capture_output=True, text=True)
    assert r.returncode != 0 and "obs_low and obs_high must be float[D]" in r.stderr, r.stderr[-1500:]


# ---- the host build of the scaled entry points ----------------------------------------------------------------------------------------------------------
class HostEnvs:
    """E envs of a plug-in's host build; `scaled` picks the _scaled entry points"""

    def __init__(self, lib, E, seed, episode_len=0):
        self.lib = lib
        d = self.d = Desc.in_dll(lib, "dril_env_plugin_desc")
        self.E = E
        self.state = np.zeros((E, d.S), f32); self.sc = np.zeros(E, np.int32); self.ep = np.zeros(E, np.uint32); self.gs = np.zeros(E, np.uint32)
        self.base = dict(E=E, episode_len=episode_len or d.episode_len, fixed_len=0, action_start=0, seed0=seed)

    def _args(self, **kw):
        p = lambda a: a.ctypes.data_as(_PV)
        a = Args(**self.base, state=p(self.state), step_count=p(self.sc), episode=p(self.ep), gstep=p(self.gs))
        for k, v in kw.items():
            setattr(a, k, p(v))
        return a

    def obs_space(self):
        buf = np.empty(2 * self.d.D, f32)
        self.lib.dril_env_plugin_host_obs_space(C.byref(self._args(obs=buf)))
        return buf[: self.d.D].copy(), buf[self.d.D:].copy()

    def reset(self):
        self.lib.dril_env_plugin_host_reset(C.byref(self._args()))

    def observe(self, scaled):
        obs = np.empty((self.E, self.d.D), f32)
        getattr(self.lib, "dril_env_plugin_host_observe" + ("_scaled" if scaled else ""))(C.byref(self._args(obs=obs)))
        return obs

    def step(self, actions, scaled):
        E, D = self.E, self.d.D
        rew = np.empty(E, f32); term = np.empty(E, np.uint8); trunc = np.empty(E, np.uint8)
        tobs = np.full((E, D), np.nan, f32); nxt = np.empty((E, D), f32)
        getattr(self.lib, "dril_env_plugin_host_step" + ("_scaled" if scaled else ""))(
            C.byref(self._args(actions=actions, rewards=rew, terminated=term, truncated=trunc, terminal_obs=tobs, obs=nxt)))
        return rew, term.astype(bool), trunc.astype(bool), tobs, nxt

    def clone_state_from(self, other):
        for a, b in ((self.state, other.state), (self.sc, other.sc), (self.ep, other.ep), (self.gs, other.gs)):
            a[...] = b


def scale(x, lo, hi):       # scale! scalingWrapperEnv.jl:71-74, every operation in float32
    sf = f32(2) / (hi - lo)
    return ((x.astype(f32) - lo) * sf - f32(1)).astype(f32)


def unscale(x, lo, hi):     # unscale! :76-79
    sf = f32(2) / (hi - lo)
    return ((x.astype(f32) + f32(1)) / sf + lo).astype(f32)


@pytest.mark.parametrize("name,episode_len", [("pendulum", 23), ("reacher3", 45)])
def test_host_scaled_entry_points_against_the_reference_formulas(name, episode_len, tmp_path):
    """two sets of envs of one host build in lock step: the scaled entry points on one, the plain ones on the other fed with the action the wrapper hands the env
    (clamp to [-1, 1], unscale!); every observation of the first is scale! of the second's, everything else is equal to the bit"""
    lib = _host_build(ENVS / f"{name}_plugin.hip", tmp_path / f"{name}_host.so")
    E = 24
    w, p = HostEnvs(lib, E, 5, episode_len), HostEnvs(lib, E, 5, episode_len)
    lo, hi = w.obs_space()
    A = w.d.A
    alo, ahi = np.array(w.d.action_low[:A], f32), np.array(w.d.action_high[:A], f32)
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()
    if name == "pendulum":
        assert lo.tolist() == [-1.0, -1.0, -8.0] and hi.tolist() == [1.0, 1.0, 8.0]           # Gymnasium's Box
    w.reset(); p.reset()
    rng = np.random.default_rng(0)
    n_trunc = n_term = 0
    for t in range(300):
        assert np.array_equal(w.observe(True), scale(p.observe(False), lo, hi)), t
        assert np.array_equal(w.observe(False), p.observe(False)), t                           # the plain entry point of the same build is untouched by the wrapper
        act = rng.uniform(-1.6, 1.6, (E, A)).astype(f32)                                       # beyond Box(-1, 1): the ClampAdapter of the wrapper's action space
        if name == "reacher3":
            act[: E // 3] = f32(1.5)                                                           # a third of the envs is pushed out of |p| <= 2: terminations
        keep = act.copy()
        rw, tw, uw, ow, nw = w.step(act, True)
        assert np.array_equal(act, keep)                                                       # the caller's array keeps the raw action
        rp, tp, up, op, npl = p.step(unscale(np.clip(act, f32(-1), f32(1)), alo, ahi), False)
        assert np.array_equal(rw, rp) and np.array_equal(tw, tp) and np.array_equal(uw, up), t
        assert np.array_equal(nw, scale(npl, lo, hi)), t
        assert uw.any() == up.any() and np.array_equal(ow[uw], scale(op[up], lo, hi)), t       # the terminal observation of a truncated env is scaled
        assert np.isnan(ow[~uw]).all()                                                         # and written for truncated envs only
        assert np.array_equal(w.state, p.state) and np.array_equal(w.sc, p.sc) and np.array_equal(w.ep, p.ep) and np.array_equal(w.gs, p.gs), t
        n_trunc += int(uw.sum()); n_term += int(tw.sum())
    assert n_trunc > 0 and (name != "reacher3" or n_term > 0)
    inside = np.abs(w.observe(True)) <= 1.0 + 1e-6
    assert inside.all(), "the declared box of the example holds its observations"


def test_scale_and_unscale_known_answers(tmp_path):
    kats = json.loads((ROOT / "tests" / "golden" / "scaling_kats.json").read_text())     # the reference's own ScalingWrapperEnv test vectors
    src = tmp_path / "kat.cpp"
    src.write_text('#include "device/dril_scaling.h"\nextern "C" float kat_scale(float x, float lo, float hi) { return dril::scale_to_unit(x, lo, hi); }\n'
                   'extern "C" float kat_unscale(float x, float lo, float hi) { return dril::unscale_from_unit(x, lo, hi); }\n')
    so = tmp_path / "kat.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", str(ROOT / "include"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for fn in (lib.kat_scale, lib.kat_unscale):
        fn.restype, fn.argtypes = C.c_float, [C.c_float] * 3
    for key, fn, ref, inv in (("observation", lib.kat_scale, scale, lib.kat_unscale), ("action", lib.kat_unscale, unscale, lib.kat_scale)):
        assert len(kats[key]) >= 4
        for c in kats[key]:
            lo, hi, x = (np.array(c[k], f32) for k in ("low", "high", "x"))
            got = np.array([fn(float(a), float(l), float(h)) for a, l, h in zip(x, lo, hi)], f32)
            np.testing.assert_allclose(got, c["expected"], rtol=0, atol=c["atol"])
            assert np.array_equal(got, ref(x, lo, hi))                                         # the NumPy statement the other tests check against, to the bit
            back = np.array([inv(float(a), float(l), float(h)) for a, l, h in zip(got, lo, hi)], f32)
            np.testing.assert_allclose(back, x, rtol=1e-5, atol=1e-5 * float((hi - lo).max()))   # the round trip


# ---- the library's side, as far as it goes without a GPU ----------------------------------------------------------------------------------------------------
NEW = ("dril_env_module_obs_space", "dril_env_module_obs_space_of", "dril_scaling_enable", "dril_agent_spaces",
       "dril_sac_env_module_obs_space_of", "dril_sac_scaling_enable", "dril_sac_agent_spaces")


def test_entry_points_are_exported_and_header_capi_and_shim_agree(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    headers = (ROOT / "include" / "dril_hip.h").read_text() + (ROOT / "include" / "dril_sac.h").read_text()
    shim = "".join(p.read_text() for p in (ROOT / "dril.jl_amd" / "julia").glob("DRiLHIP*.jl"))
    for name in NEW:
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
        assert re.search(rf"\bint32_t\s+{name}\s*\(", headers), name
    for name in ("dril_env_module_obs_space", "dril_scaling_enable", "dril_sac_scaling_enable"):
        assert f"(:{name}, LIB[])" in shim, f"the Julia shim has no ccall of {name}"
    assert "scaling::Bool = false" in shim
    plug = (ROOT / "include" / "device" / "dril_env_plugin.h").read_text()
    assert "#define DRIL_ENV_PLUGIN_ABI 1u" in plug                     # no ABI bump
    dev = (ROOT / "dril.jl_amd" / "csrc" / "dril_device.h").read_text()
    assert "device/dril_scaling.h" in dev and "float scale_to_unit(" not in dev       # one definition, included from both places
    r = subprocess.run(["python", str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]


def test_path_refusals_come_before_any_gpu_work_and_null_handles_fail_loudly(pkg, tmp_path):
    capi = pkg._capi
    lib = capi.load_library()
    decl = C.c_int32(-1)
    assert lib.dril_env_module_obs_space(None, 0, None, None, C.byref(decl)) == capi.ERR_INVALID_ARG
    junk = tmp_path / "junk.hsaco"
    junk.write_bytes(b"not a code object at all")
    assert lib.dril_env_module_obs_space(str(junk).encode(), 0, None, None, C.byref(decl)) == capi.ERR_INVALID_ARG
    assert b"not a code object" in lib.dril_last_error(None)
    assert lib.dril_scaling_enable(None, 1) == capi.ERR_NOT_INITIALISED and lib.dril_sac_scaling_enable(None, 1) == capi.ERR_NOT_INITIALISED
    assert lib.dril_agent_spaces(None, None, None, None, None, None) == capi.ERR_NOT_INITIALISED


def test_python_scaling_wrapper_keeps_its_refusals_and_module_env_spaces(pkg):
    with pytest.raises(NotImplementedError):
        pkg.ScalingWrapperEnv(pkg.CartPoleEnv())
    with pytest.raises(NotImplementedError):
        pkg.ScalingWrapperEnv(pkg.DeviceParallelEnv(pkg.PendulumEnv(), 4))                     # the parallel env of a built-in: wrap the single env
    assert pkg.ScalingWrapperEnv(pkg.PendulumEnv()).kind == pkg._capi.ENV_PENDULUM_SCALED
    from dril_jl_amd.host import ModuleEnv
    info = dict(obs_dim=2, action_dim=1, discrete=False, action_low=np.array([-0.5], f32), action_high=np.array([1.5], f32),
                obs_low=np.array([-4, 0], f32), obs_high=np.array([5, 7], f32), obs_declared=True, name="Walk", episode_len=7)
    m = ModuleEnv("walk.hsaco", info, 7)
    assert m.observation_space() == pkg.Box((-4.0, 0.0), (5.0, 7.0)) and m.action_space() == pkg.Box((-0.5,), (1.5,))
    m.scaling = True
    assert m.observation_space() == pkg.Box((-1.0, -1.0), (1.0, 1.0)) and m.action_space() == pkg.Box((-1.0,), (1.0,))
    lo, hi = np.array([-4, 0], f32), np.array([5, 7], f32)
    x = np.array([[0.5, 3.0], [-4.0, 7.0]], f32)
    assert np.array_equal(m.scale_observation(x), scale(x, lo, hi)) and np.array_equal(m.unscale_observation(x), unscale(x, lo, hi))
    assert np.array_equal(m.unscale_action(np.array([[-1.0], [1.0]], f32)), np.array([[-0.5], [1.5]], f32))
    undeclared = ModuleEnv("old.hsaco", {**info, "obs_declared": False}, 7)
    assert undeclared.observation_space() == pkg.Box((-np.inf,) * 2, (np.inf,) * 2)            # an undeclared space keeps the answer it had
