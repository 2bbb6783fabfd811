"""CPU: the population entry of a device env plug-in's fused rollout (include/device/dril_env_rollout_pop.h, DRIL_ENV_PLUGIN_ROLLOUT_POP) without a GPU.

  * which symbols the fourth macro adds to a code object and to a host build, and that the descriptor repeats the rollout's;
  * the host build (-DDRIL_ENV_PLUGIN_HOST): dril_env_plugin_host_rollout_pop over a table of member blocks leaves every array byte-equal to one
    dril_env_plugin_host_rollout call per member, whatever the order of the table;
  * train_population_ takes DeviceModuleEnv members to the native join (a stubbed library), and still refuses other env types."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import fused_rollout_helpers as F
from test_env_plugin_fused import ENVS, FUSED_SRC, ROLLOUT, ROLLOUT_SCALED, ROOT
from test_env_plugin_scaling import BEFORE, FINITE, INFINITE, NO_SPACE, SCALED, SPACE, _code_object_symbols

f32 = np.float32
POP = {"dril_env_plugin_rollout_pop", "dril_env_plugin_rollout_pop.kd", "dril_env_plugin_rollout_pop_desc"}
POP_SCALED = {"dril_env_plugin_rollout_pop_scaled", "dril_env_plugin_rollout_pop_scaled.kd"}
POP_SRC = FUSED_SRC + '#include "device/dril_env_rollout_pop.h"\nDRIL_ENV_PLUGIN_ROLLOUT_POP(Walk)\n'


def _desc(lib, name):
    d = F.RolloutDesc.in_dll(lib, name)
    return (d.abi_version, d.args_size, d.tile, d.threads, d.max_width, d.has_scaled)


@pytest.mark.parametrize("decl,scaled", [(NO_SPACE, False), (FINITE, True), (INFINITE, False)], ids=["no-space", "finite", "infinite"])
def test_the_fourth_macro_adds_exactly_the_new_names(decl, scaled, tmp_path):
    fused, pop = tmp_path / "fused.hip", tmp_path / "pop.hip"
    fused.write_text(FUSED_SRC % decl); pop.write_text(POP_SRC % decl)
    have = _code_object_symbols(fused, tmp_path / "fused.hsaco")
    assert (ROLLOUT_SCALED <= have) == scaled
    assert _code_object_symbols(pop, tmp_path / "pop.hsaco") == have | POP | (POP_SCALED if scaled else set())
    so = tmp_path / "pop_host.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-x", "c++", "-DDRIL_ENV_PLUGIN_HOST", "-I", str(ROOT / "include"), str(pop), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    assert hasattr(lib, "dril_env_plugin_host_rollout_pop") and hasattr(lib, "dril_env_plugin_host_rollout_pop_scaled") == scaled
    assert _desc(lib, "dril_env_plugin_rollout_pop_desc") == _desc(lib, "dril_env_plugin_rollout_desc") == (1, C.sizeof(F.RolloutArgs), 16, 256, 256, int(scaled))


@pytest.mark.parametrize("name,scaled", [("cartpole", False), ("reacher3", True)])
def test_symbols_of_the_pop_examples(name, scaled, tmp_path):
    fused = _code_object_symbols(ENVS / f"{name}_fused_plugin.hip", tmp_path / f"{name}_fused.hsaco")
    assert _code_object_symbols(ENVS / f"{name}_pop_plugin.hip", tmp_path / f"{name}_pop.hsaco") == fused | POP | (POP_SCALED if scaled else set())
    lib = F.host_build(f"{name}_pop", tmp_path)
    assert hasattr(lib, "dril_env_plugin_host_rollout_pop") and hasattr(lib, "dril_env_plugin_host_rollout_pop_scaled") == scaled
    assert _desc(lib, "dril_env_plugin_rollout_pop_desc") == _desc(lib, "dril_env_plugin_rollout_desc")
    text = (ENVS / f"{name}_pop_plugin.hip").read_text()
    code = [ln for ln in text.splitlines() if ln.strip() and not ln.startswith("//")]
    assert len(code) == 3 and code[0] == f'#include "{name}_fused_plugin.hip"' and code[1] == '#include "device/dril_env_rollout_pop.h"'   # two lines on top of the fused twin


# ---- the host build: the table against one call per member ---------------------------------------------------------------------------------------------------
class Member(F.HostRollout):
    """a HostRollout whose argument block can be built without running it (the statements of HostRollout.collect_rollout)"""

    def args(self):
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        b = self.bufs
        g = F.RolloutArgs(env=self._env_args(), T=self.T, n_hidden=len(self.hidden), activation=self.activation, n_params=self.P, actor_off=0, critic_off=self.Pa,
                          log_std_off=self.Pa + self.Pc, params=p(self.params), noise=None if self.noise is None else p(self.noise), obs=p(b[F.BUF_OBSERVATIONS]),
                          act=p(b[F.BUF_ACTIONS]), rew=p(b[F.BUF_REWARDS]), logp=p(b[F.BUF_LOGPROBS]), val=p(b[F.BUF_VALUES]), boot=p(b[F.BUF_BOOTSTRAP]),
                          flags=p(b[F.BUF_FLAGS]), last_values=p(b[F.BUF_LAST_VALUES]))
        for i, h in enumerate(self.hidden):
            g.hidden[i] = h
        if self.monitor:
            g.ep_ret, g.ep_len = p(self.ep_ret), p(self.ep_len)
        return g

    def everything(self):
        arrays = [self.state, self.sc, self.ep, self.gs, self.mon_ret, self.mon_len, self.e_term, self.e_trunc, self.e_tobs, self.e_obs, self.ep_ret, self.ep_len]
        arrays += [self.bufs[k] for k in (F.BUF_OBSERVATIONS, F.BUF_ACTIONS, F.BUF_REWARDS, F.BUF_LOGPROBS, F.BUF_VALUES, F.BUF_FLAGS, F.BUF_BOOTSTRAP, F.BUF_LAST_VALUES)]
        return [np.ascontiguousarray(a).view(np.uint8).tobytes() for a in arrays]


E, T, LIMIT = 20, 13, 11


def _members(lib, name):
    """three members with their own seeds and parameters; member 1 has monitor arrays, member 2 an injected noise table"""
    out = []
    for m in range(3):
        h = Member(lib, E, T, episode_len=LIMIT, action_start=1 if name == "cartpole" else 0, monitor=(m == 1))
        h.set_params((np.random.default_rng(10 + m).standard_normal(h.P) * 0.3).astype(f32))
        h.env_reset(100 + 7 * m)
        if m == 2:
            rng = np.random.default_rng(3)
            h.set_noise(rng.random(E * T) if h.discrete else rng.standard_normal((E * T, h.A)).astype(f32))
        out.append(h)
    return out


@pytest.mark.parametrize("name", ["cartpole", "reacher3"])
def test_host_rollout_pop_equals_one_host_rollout_per_member(name, tmp_path):
    lib = F.host_build(f"{name}_pop", tmp_path)
    alone = _members(lib, name)                                                         # (deterministic: every call builds the same inputs)
    for h in alone:
        lib.dril_env_plugin_host_rollout(C.byref(h.args()))
    want = [h.everything() for h in alone]
    assert all((h.bufs[F.BUF_FLAGS] & 2).any() for h in alone)                          # truncations, and with them bootstrap values inside the rollout
    assert all((h.bufs[F.BUF_BOOTSTRAP][(h.bufs[F.BUF_FLAGS] & 2) != 0] != 0).any() for h in alone)
    assert want[0] != want[1] != want[2] and np.isfinite(alone[1].ep_ret).any()      # the members differ; the monitor rows were written
    for order in itertools.permutations(range(3)):
        hs = _members(lib, name)
        table = (F.RolloutArgs * 3)(*[hs[m].args() for m in order])
        lib.dril_env_plugin_host_rollout_pop(table, 3)
        for m in range(3):
            assert hs[m].everything() == want[m], f"member {m} in table order {order}"


def test_scaled_host_rollout_pop(tmp_path):
    """the _scaled entry runs the scaled host rollout per member"""
    lib = F.host_build("reacher3_pop", tmp_path)
    alone = _members(lib, "reacher3")
    for h in alone:
        lib.dril_env_plugin_host_rollout_scaled(C.byref(h.args()))
    hs = _members(lib, "reacher3")
    lib.dril_env_plugin_host_rollout_pop_scaled((F.RolloutArgs * 3)(*[h.args() for h in hs]), 3)
    assert [h.everything() for h in hs] == [h.everything() for h in alone]
    plain = _members(lib, "reacher3")
    lib.dril_env_plugin_host_rollout_pop((F.RolloutArgs * 3)(*[h.args() for h in plain]), 3)
    assert plain[0].everything() != hs[0].everything()                                  # scaling changed what the agent saw


# ---- Python ------------------------------------------------------------------------------------------------------------------------------------------------
def test_train_population_takes_plugin_envs_to_the_native_join(pkg, monkeypatch):
    """a list of DeviceModuleEnv reaches dril_population_join with every bound handle switched to the one-launch update; any other env type is a TypeError"""
    host = pkg.host
    calls = []

    class StubHandle:
        def __init__(self, i):
            self.i = i
        def update_fused_enable(self, on):
            calls.append(("update_fused_enable", self.i, on))
        def set_params(self, flat):
            calls.append(("set_params", self.i))
        def set_optimizer_state(self, st):
            pass
        def get_params(self):
            return np.zeros(0, f32)
        def get_optimizer_state(self):
            return {}

    class Joined(Exception):
        pass

    def join(self, handles):
        calls.append(("join", [h.i for h in handles]))
        raise Joined()

    envs = [host.DeviceModuleEnv.__new__(host.DeviceModuleEnv) for _ in range(3)]
    for i, e in enumerate(envs):
        e.n_envs = 4
    monkeypatch.setattr(host.DeviceModuleEnv, "bind", lambda self, alg, layer=None: StubHandle(envs.index(self)))
    monkeypatch.setattr(host.Population, "__init__", join)
    monkeypatch.setattr(host, "flatten_params", lambda p: np.zeros(0, f32))
    monkeypatch.setattr(host, "unflatten_params", lambda flat, like: like)
    alg = pkg.PPO()
    agent = lambda: pkg.Agent(pkg.ActorCriticLayer(pkg.CartPoleEnv().observation_space(), pkg.CartPoleEnv().action_space()), alg)
    with pytest.raises(Joined):
        pkg.train_population_([agent() for _ in range(3)], envs, [alg] * 3, 8192, fused_update=True)
    assert calls[-1] == ("join", [0, 1, 2]) and [c for c in calls if c[0] == "update_fused_enable"] == [("update_fused_enable", i, True) for i in range(3)]
    calls.clear()
    with pytest.raises(Joined):
        pkg.train_population_([agent() for _ in range(3)], envs, [alg] * 3, 8192)          # without the opt-in: the library decides at the join
    assert not [c for c in calls if c[0] == "update_fused_enable"] and calls[-1][0] == "join"
    with pytest.raises(TypeError):
        pkg.train_population_([agent()], [object()], [alg], 8192)
    with pytest.raises(TypeError):
        pkg.train_population_([agent(), agent()], [envs[0], pkg.DeviceParallelEnv(pkg.CartPoleEnv(), 4)], [alg, alg], 8192)   # plug-in and built-in members do not mix
    with pytest.raises(TypeError):
        pkg.evaluate_population([agent()], [object()])


def test_header_docs_and_shim_name_the_new_entry():
    header = (ROOT / "include" / "device" / "dril_env_rollout_pop.h").read_text()
    assert "#define DRIL_ENV_ROLLOUT_POP_ABI 1u" in header and "DRIL_ENV_PLUGIN_ROLLOUT_POP(Env)" in header
    assert "#define DRIL_ENV_ROLLOUT_ABI 1u" in (ROOT / "include" / "device" / "dril_env_rollout.h").read_text()      # no ABI bump of the rollout
    assert "#define DRIL_ENV_PLUGIN_ABI 1u" in (ROOT / "include" / "device" / "dril_env_plugin.h").read_text()
    shim = (ROOT / "dril.jl_amd" / "julia" / "DRiLHIP.jl").read_text()
    # (OnDeviceModule is a constructor of DeviceParallelEnv, not a type: the list method of train! is the plug-ins' too, and forwards here)
    assert "function train_population!(agents::Vector, envs::Vector{<:DeviceParallelEnv}, algs::Vector{<:PPO}, max_steps::Int; fused_update::Bool = true)" in shim
    assert "fused_update && check(ccall((:dril_update_fused_enable, LIB[])" in shim
    r = subprocess.run(["python", str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
