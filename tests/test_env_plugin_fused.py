"""CPU: the fused rollout of a device env plug-in (include/device/dril_env_rollout.h, DRIL_ENV_PLUGIN_ROLLOUT) without a GPU.

  * which symbols the second macro adds to a code object and to a host build, and that a source without it keeps exactly the symbols it had;
  * the host build (-DDRIL_ENV_PLUGIN_HOST: the kernel's per-env functions — transition, head, the k-ascending fmaf chain of a dense row — in a serial loop) of the
    CartPole and Pendulum fused twins against the CPU oracle's built-in kinds 0 and 1, with the inputs, the comparison and the tolerances of
    test_collect_rollout_matches_oracle (tests/test_gpu_parity.py);
  * reacher3's host rollout against the NumPy twin of tests/test_gpu_env_plugin.py driven with the recorded actions;
  * header, ctypes table and Julia shim agree on the new entry points."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fused_rollout_helpers as F
from test_env_plugin import GENCO
from test_env_plugin_scaling import BEFORE, FINITE, INFINITE, NO_SPACE, SCALED, SPACE, SRC, _code_object_symbols

ROOT = Path(__file__).resolve().parents[1]
ENVS = ROOT / "examples" / "envs"
f32 = np.float32

ROLLOUT = {"dril_env_plugin_rollout", "dril_env_plugin_rollout.kd", "dril_env_plugin_rollout_desc"}
ROLLOUT_SCALED = {"dril_env_plugin_rollout_scaled", "dril_env_plugin_rollout_scaled.kd"}
FUSED_SRC = SRC + '#include "device/dril_env_rollout.h"\nDRIL_ENV_PLUGIN_ROLLOUT(Walk)\n'


@pytest.mark.parametrize("decl,extra", [(NO_SPACE, set()), (FINITE, SPACE | SCALED | ROLLOUT_SCALED), (INFINITE, SPACE)])
def test_the_second_macro_adds_exactly_the_new_names(decl, extra, tmp_path):
    src = tmp_path / "walk.hip"
    src.write_text(FUSED_SRC % decl)
    assert _code_object_symbols(src, tmp_path / "walk.hsaco") == BEFORE | ROLLOUT | extra
    so = tmp_path / "walk_host.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-x", "c++", "-DDRIL_ENV_PLUGIN_HOST", "-I", str(ROOT / "include"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    assert hasattr(lib, "dril_env_plugin_host_rollout")
    assert hasattr(lib, "dril_env_plugin_host_rollout_scaled") == (ROLLOUT_SCALED <= extra)
    d = F.RolloutDesc.in_dll(lib, "dril_env_plugin_rollout_desc")
    assert (d.abi_version, d.args_size, d.tile, d.threads, d.max_width, d.has_scaled) == (1, C.sizeof(F.RolloutArgs), 16, 256, 256, int(ROLLOUT_SCALED <= extra))
    plain = tmp_path / "plain.hip"
    plain.write_text(SRC % decl)                                             # without the second macro: what it always was
    assert _code_object_symbols(plain, tmp_path / "plain.hsaco") == BEFORE | (extra - ROLLOUT_SCALED)


@pytest.mark.parametrize("name,space,scaled", [("cartpole", True, False), ("pendulum", True, True), ("reacher3", True, True)])
def test_symbols_of_the_examples_and_their_fused_twins(name, space, scaled, tmp_path):
    before = BEFORE | (SPACE if space else set()) | (SCALED if scaled else set())
    assert _code_object_symbols(ENVS / f"{name}_plugin.hip", tmp_path / f"{name}.hsaco") == before
    assert _code_object_symbols(ENVS / f"{name}_fused_plugin.hip", tmp_path / f"{name}_fused.hsaco") == before | ROLLOUT | (ROLLOUT_SCALED if scaled else set())
    lib = F.host_build(f"{name}_fused", tmp_path)
    assert hasattr(lib, "dril_env_plugin_host_rollout") and hasattr(lib, "dril_env_plugin_host_rollout_scaled") == scaled


def test_a_compile_time_width_the_env_does_not_fit_fails_at_the_plugins_compile(tmp_path):
    r = subprocess.run(GENCO + ["-DDRIL_ENV_ROLLOUT_MAX_WIDTH=8", str(ENVS / "reacher3_fused_plugin.hip"), "-o", str(tmp_path / "bad.hsaco")], capture_output=True, text=True)
    assert r.returncode != 0 and "D and A must fit DRIL_ENV_ROLLOUT_MAX_WIDTH" in r.stderr, r.stderr[-1500:]


# ---- the host build against the CPU oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,E,T,L,fixed", F.ORACLE_CASES)
def test_host_rollout_of_a_twin_matches_the_oracle(pkg, oracle_mod, name, kind, E, T, L, fixed, tmp_path):
    """collect_rollout! (rollout_buffer.jl:46-90) by dril_env_plugin_host_rollout: every buffer field against the trajectory-based oracle, injected noise and the shared
    Philox stream, two collections without a reset; truncations with V(terminal_observation) bootstraps and rollout-limited tails.  Advantages and returns: the oracle's
    GAE on the rows the host rollout wrote."""
    cfg = pkg._capi.default_config(kind)
    cfg.n_envs, cfg.n_steps, cfg.episode_len, cfg.batch_size, cfg.epochs, cfg.fixed_length_episodes = E, T, L, max(2, (E * T) // 4), 2, int(fixed)
    lib = F.host_build(f"{name}_fused", tmp_path)
    make = lambda: F.HostRollout(lib, E, T, episode_len=L, action_start=cfg.action_start, fixed_len=fixed, gamma=cfg.gamma, gae_lambda=cfg.gae_lambda)
    F.compare_with_oracle(make, oracle_mod, cfg, lambda h: h.collect_rollout(oracle_mod.lib().orc_gae), f"host {name} E={E}")


# ---- reacher3 against the NumPy twin ------------------------------------------------------------------------------------------------------------------------
from test_gpu_env_plugin import _reacher_obs, _reacher_step  # noqa: E402  (plain functions of a GPU-marked module: importing them runs nothing on a GPU)


@pytest.mark.parametrize("hidden,activation", [((64, 64), 0), ((40, 24, 72), 6)])
def test_host_rollout_of_reacher3_follows_the_numpy_twin(hidden, activation, tmp_path):
    E, T, L, seed = 24, 40, 13, 5
    lib = F.host_build("reacher3_fused", tmp_path, flags=("-ffp-contract=off",))
    h = F.HostRollout(lib, E, T, episode_len=L, hidden=hidden, activation=activation, action_start=0, monitor=True)
    rng = np.random.default_rng(1)
    h.set_params((rng.standard_normal(h.P) * 0.3).astype(f32))
    h.env_reset(seed)
    h.state[: E // 4, 0] = f32(1.9); h.state[: E // 4, 3] = f32(1.0)          # a quarter of the envs starts on its way out of |p| <= 2: terminations
    st = h.state.copy(); sc = np.zeros(E, np.int64)
    h.collect_rollout(lambda *a: 0)
    obs, act = h.buffer(F.BUF_OBSERVATIONS).reshape(T, E, 12), h.buffer(F.BUF_ACTIONS).reshape(T, E, 3)
    rew, fl = h.buffer(F.BUF_REWARDS).reshape(T, E), h.buffer(F.BUF_FLAGS).reshape(T, E)
    assert (fl & 2).any() and (fl & 1).any() and np.isfinite(h.buffer(F.BUF_LOGPROBS)).all() and np.isfinite(h.buffer(F.BUF_VALUES)).all()
    for t in range(T):
        np.testing.assert_allclose(obs[t], _reacher_obs(st), rtol=2e-6, atol=2e-6)
        want_st, want_r, want_term = _reacher_step(st, act[t])
        sc += 1
        np.testing.assert_allclose(rew[t], want_r, rtol=2e-6, atol=2e-6)
        assert np.array_equal((fl[t] & 1) != 0, want_term) and np.array_equal((fl[t] & 2) != 0, sc >= L), t
        done = fl[t] != 0
        sc[done] = 0
        st = want_st
        if t + 1 < T:
            st[done] = obs[t + 1][done][:, :9]                                 # a fresh episode: its state is the next observation's first nine entries
    # MonitorWrapperEnv's finished-episode rows equal their recomputation from rewards and flags
    cur_r, cur_l = np.zeros(E, f32), np.zeros(E, np.int64)
    er, el = h.ep_ret.reshape(T, E), h.ep_len.reshape(T, E)
    for t in range(T):
        cur_r += rew[t]; cur_l += 1
        for e in np.nonzero(fl[t])[0]:
            assert er[t, e] == cur_r[e] and el[t, e] == cur_l[e]
            cur_r[e] = 0; cur_l[e] = 0
    assert np.array_equal(h.mon_ret, cur_r) and np.array_equal(h.mon_len, cur_l) and (h.gs == T).all()
    # a second handle over envs [8, 16) of the same seeds reproduces those envs to the bit: an env's rows do not depend on its neighbours
    part = F.HostRollout(lib, 8, T, episode_len=L, hidden=hidden, activation=activation, action_start=0)
    part.set_params(h.params); part.env_reset(seed + 8)
    part.collect_rollout(lambda *a: 0)
    for which, width in ((F.BUF_OBSERVATIONS, 12), (F.BUF_ACTIONS, 3), (F.BUF_LOGPROBS, 1), (F.BUF_VALUES, 1), (F.BUF_REWARDS, 1), (F.BUF_BOOTSTRAP, 1)):
        assert np.array_equal(part.buffer(which).reshape(T, 8, width), h.buffer(which).reshape(T, E, width)[:, 8:16]), which


# ---- the library's side, as far as it goes without a GPU ----------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_header_capi_and_shim_agree(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    header = (ROOT / "include" / "dril_hip.h").read_text()
    shim = "".join(p.read_text() for p in (ROOT / "dril.jl_amd" / "julia").glob("DRiLHIP*.jl"))
    for name in ("dril_rollout_fused_enable", "dril_rollout_fused_info"):
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
        assert re.search(rf"\bint32_t\s+{name}\s*\(", header), name
        assert f"(:{name}, LIB[])" in shim, f"the Julia shim has no ccall of {name}"
    assert "fused_rollout::Bool = false" in shim
    assert lib.dril_rollout_fused_enable(None, 1) == capi.ERR_NOT_INITIALISED and lib.dril_rollout_fused_info(None, None) == capi.ERR_NOT_INITIALISED
    # the info struct: C and ctypes agree on its layout
    plug = (ROOT / "include" / "device" / "dril_env_plugin.h").read_text()
    assert "#define DRIL_ENV_PLUGIN_ABI 1u" in plug                     # no ABI bump of the plug-in contract
    for src in ("dril_generic.hip", "dril_policy.hip", "dril_gemm.hip"):                          # one definition of head and activations, under include/device
        text = (ROOT / "dril.jl_amd" / "csrc" / src).read_text()
        assert "float act_gelu(" not in text and "void softmax_stats(" not in text
    r = subprocess.run(["python", str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]


def test_fused_info_layout_matches_c(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_hip.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(dril_fused_rollout_info),'
                   ' offsetof(dril_fused_rollout_info, last_collection_launches), offsetof(dril_fused_rollout_info, reason));return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    sz, o_n, o_reason = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    K = pkg._capi.DrilFusedRolloutInfo
    assert (C.sizeof(K), K.last_collection_launches.offset, K.reason.offset) == (sz, o_n, o_reason)
