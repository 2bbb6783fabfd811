"""CPU: the fused evaluation of a device env plug-in (include/device/dril_env_evaluate.h, DRIL_ENV_PLUGIN_EVALUATE) without a GPU.

  * which symbols the macro adds to a code object and to a host build, with and without DRIL_ENV_PLUGIN_ROLLOUT in the same source, and that a source without it keeps
    exactly the symbols it had; the descriptor against the ctypes mirror;
  * the host build (-DDRIL_ENV_PLUGIN_HOST: the kernel's per-env functions in a serial loop), stochastic: raw rewards and flags equal those of
    dril_env_plugin_host_rollout from the same reset, bit for bit, whatever the launch length;
  * the host build, deterministic: against NumPy — the reacher3 twin of tests/test_env_plugin.py, a float64 actor, evaluation.jl:87-124 (reference_loop of
    tests/test_eval_device.py) and trajectory_utils.jl:16-45 (reference_trajectory of tests/test_traj_device.py) over the rows the launches leave, consumed by the
    library's own rules (eval_account, traj_record_lane_rows) compiled with g++;
  * the normaliser: the host build's expression is dril::normalize_obs — the line nz_obs of dril_norm_wrap.h expands — bit for bit, with a clip that bites;
  * struct, default and refusal tests of dril_evaluate_fused_info that need no GPU; the shim check."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fused_evaluate_helpers as V
import fused_rollout_helpers as F
from test_env_plugin import _reacher_obs, _reacher_step
from test_env_plugin_fused import ROLLOUT, ROLLOUT_SCALED
from test_env_plugin_scaling import BEFORE, FINITE, INFINITE, NO_SPACE, SCALED, SPACE, SRC, _code_object_symbols
from test_eval_device import _DRIVER as ACCT_DRIVER, reference_loop, run_device_form
from test_traj_device import reference_trajectory

ROOT = Path(__file__).resolve().parents[1]
ENVS = ROOT / "examples" / "envs"
f32 = np.float32

EVALUATE = {"dril_env_plugin_evaluate", "dril_env_plugin_evaluate.kd", "dril_env_plugin_evaluate_desc"}
EVALUATE_SCALED = {"dril_env_plugin_evaluate_scaled", "dril_env_plugin_evaluate_scaled.kd"}
EVAL_SRC = SRC + '#include "device/dril_env_evaluate.h"\nDRIL_ENV_PLUGIN_EVALUATE(Walk)\n'
BOTH_SRC = SRC + '#include "device/dril_env_rollout.h"\nDRIL_ENV_PLUGIN_ROLLOUT(Walk)\n#include "device/dril_env_evaluate.h"\nDRIL_ENV_PLUGIN_EVALUATE(Walk)\n'


def _params(P, seed, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(P) * scale).astype(f32)


# ---- symbols ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decl,extra", [(NO_SPACE, set()), (FINITE, SPACE | SCALED), (INFINITE, SPACE)])
def test_the_macro_adds_exactly_the_new_names(decl, extra, tmp_path):
    scalable = SCALED <= extra
    src = tmp_path / "walk.hip"
    src.write_text(EVAL_SRC % decl)
    assert _code_object_symbols(src, tmp_path / "walk.hsaco") == BEFORE | extra | EVALUATE | (EVALUATE_SCALED if scalable else set())
    both = tmp_path / "both.hip"
    both.write_text(BOTH_SRC % decl)                                          # with the rollout macro in the same source: the union, nothing else
    assert _code_object_symbols(both, tmp_path / "both.hsaco") == BEFORE | extra | ROLLOUT | EVALUATE | ((ROLLOUT_SCALED | EVALUATE_SCALED) if scalable else set())
    so = tmp_path / "walk_host.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-x", "c++", "-DDRIL_ENV_PLUGIN_HOST", "-I", str(ROOT / "include"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    assert hasattr(lib, "dril_env_plugin_host_evaluate") and not hasattr(lib, "dril_env_plugin_host_rollout")
    assert hasattr(lib, "dril_env_plugin_host_evaluate_scaled") == scalable
    d = V.EvaluateDesc.in_dll(lib, "dril_env_plugin_evaluate_desc")
    assert (d.abi_version, d.args_size, d.tile, d.threads, d.max_width, d.has_scaled) == (1, C.sizeof(V.EvaluateArgs), 16, 256, 256, int(scalable))
    plain = tmp_path / "plain.hip"
    plain.write_text(SRC % decl)                                              # without the macro: what it always was
    assert _code_object_symbols(plain, tmp_path / "plain.hsaco") == BEFORE | extra


def test_the_other_descriptors_and_abi_numbers_stand():
    plug = (ROOT / "include" / "device" / "dril_env_plugin.h").read_text(); roll = (ROOT / "include" / "device" / "dril_env_rollout.h").read_text()
    assert "#define DRIL_ENV_PLUGIN_ABI 1u" in plug and "#define DRIL_ENV_ROLLOUT_ABI 1u" in roll
    assert "#define DRIL_ENV_EVALUATE_ABI 1u" in (ROOT / "include" / "device" / "dril_env_evaluate.h").read_text()
    assert C.sizeof(F.RolloutArgs) == 288 and C.sizeof(V.EvaluateArgs) == 288 + 144 + 16 + 40


# ---- the host build, stochastic: the fused rollout's rewards and flags, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,scaled,start", [("cartpole", False, 1), ("pendulum", False, 1), ("pendulum", True, 1), ("reacher3", False, 0)])
def test_stochastic_host_evaluation_equals_the_host_rollout(name, scaled, start, tmp_path):
    E, L, T, seed = 37, 13, 70, 11
    lib = F.host_build(f"{name}_eval", tmp_path)
    roll = F.HostRollout(lib, E, T, episode_len=L, action_start=start, scaled=scaled)
    flat = _params(roll.P, 5, 0.3)
    roll.set_params(flat); roll.env_reset(seed)
    if name == "reacher3":
        roll.state[: E // 4, 0] = f32(1.9); roll.state[: E // 4, 3] = f32(1.0)
    if name == "cartpole":
        roll.state[: E // 4, 2] = f32(0.2); roll.state[: E // 4, 3] = f32(1.0)   # a quarter of the poles starts next to the 12 degree limit, falling
    st0 = roll.state.copy()
    roll.collect_rollout(lambda *a: 0)
    rew, fl = roll.buffer(F.BUF_REWARDS).reshape(T, E), roll.buffer(F.BUF_FLAGS).reshape(T, E)
    assert (fl & 2).any() and (name == "pendulum" or (fl & 1).any())
    for K in (1, 7, 64):
        h = V.HostEvaluate(lib, E, episode_len=L, action_start=start, scaled=scaled)
        h.set_params(flat); h.env_reset(seed); h.state[:] = st0
        steps = T if K != 64 else 64
        r, f, *_ = h.run(steps, K, deterministic=False)
        assert np.array_equal(r.view(np.uint32), rew[:steps].view(np.uint32)) and np.array_equal(f, fl[:steps]), (name, K)
        assert (h.gs == steps).all()


# ---- the host build, deterministic: against NumPy ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("evaluate_drivers")
    src = d / "acct.cpp"; src.write_text(ACCT_DRIVER)
    so = d / "acct.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / "dril.jl_amd" / "csrc"), str(src), "-o", str(so)], check=True)
    acct = C.CDLL(str(so))
    acct.drive.restype = C.c_longlong
    acct.drive.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int]
    acct.reduce.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    acct.capacity.restype = C.c_longlong; acct.capacity.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong]
    return acct, V.rows_driver(d)


def _maps(h, final_original):
    """TrajMaps of an unscaled plug-in: ClampAdapter on the env's own Box"""
    D, W = h.D, h.W
    lo = np.asarray(h.desc.action_low[:W], f32); hi = np.asarray(h.desc.action_high[:W], f32)
    return np.zeros(D, f32), np.zeros(D, f32), lo, hi, lo, hi, False, h.discrete, final_original


def _episodes_and_trajectories(drivers, make, E, L, K, rng):
    """the rows of launches of K steps through the library's rules, against the reference loops on the same rows"""
    acct, rows = drivers
    h = make(E)
    rew, fl, obs0, act, obs = h.run(3 * L, K, deterministic=True)
    done = np.ascontiguousarray(fl != 0, np.uint8)
    for n_eval in (E, 3 * E // 2):
        want_r, want_l, want_steps = reference_loop(rew, done, n_eval)
        order = np.stack([rng.permutation(E) for _ in range(3 * L)]).astype(np.int32)
        steps = -(-want_steps // K) * K                                        # the launch that completes the list runs to its end
        n, out, er, el, _ = run_device_form(acct, rew, done, order, n_eval, min(steps, 3 * L), K)
        assert n == n_eval and np.array_equal(er, want_r) and np.array_equal(el, want_l) and int(out[5]) == want_steps
    for max_steps, final_original in ((0, False), (5, True), (1, False)):
        Tcap = min(max_steps, L) if max_steps else L
        for M in (1, E):
            g = make(E, M)
            launches = [g.launch(min(K, Tcap - s0), True) for s0 in range(0, Tcap, K)]
            maps = _maps(g, final_original)
            finished, r_obs, r_act, r_rew, length, end = V.record_rows(rows, launches, E, M, g.D, g.W, Tcap, maps, rng)
            assert finished == M
            data = (np.concatenate([q[3] for q in launches]), np.concatenate([q[0] for q in launches]), np.concatenate([q[1] for q in launches]) & 1,
                    (np.concatenate([q[1] for q in launches]) >> 1) & 1, np.concatenate([q[4] for q in launches]), launches[0][2])
            for m in range(M):
                o, a, r, f = reference_trajectory(m, data, max_steps, maps)
                n = len(r)
                assert length[m] == n and end[m] == f, (m, max_steps)
                assert np.array_equal(r_obs[:n + 1, m].view(np.uint32), o.view(np.uint32)) and np.array_equal(r_act[:n, m], a.reshape(n, g.W))
                assert np.array_equal(r_rew[:n, m].view(np.uint32), r.view(np.uint32))
            if M == E and max_steps == 0:
                assert (end & 1).any() and (end & 2).any()                     # terminated and truncated trajectories both present
    return rew, fl


def test_deterministic_host_evaluation_of_reacher3_follows_numpy(drivers, tmp_path):
    E, L, seed, hidden = 37, 13, 5, (64, 64)
    lib = F.host_build("reacher3_eval", tmp_path, flags=("-ffp-contract=off",))
    flat = _params(V.HostEvaluate(lib, 1).P, 5, 0.3)

    def make(E_, M=0, seed_=seed, first=0):
        h = V.HostEvaluate(lib, E_, episode_len=L, hidden=hidden, action_start=0, M=M)
        h.set_params(flat); h.env_reset(seed_ + first)
        q = np.arange(first, first + E_) < E // 4
        h.state[q, 0] = f32(1.9); h.state[q, 3] = f32(1.0)                    # a quarter of the envs starts on its way out of |p| <= 2: terminations
        return h

    # launches of ONE step: obs0 is then every step's pre-step observation, and the NumPy twin can follow step by step
    h = make(E, E)
    sc = np.zeros(E, np.int64)
    ref = []
    for t in range(3 * L):
        rew, fl, pre, act, post = h.launch(1, True)
        ref.append((rew, fl, act, post))
        a = act[0].view(f32)
        np.testing.assert_allclose(pre, _reacher_obs(pre[:, :9]), rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(a, V.actor_forward(flat, h.D, hidden, h.A, 0, pre), rtol=2e-6, atol=2e-6)     # the mode of a DiagGaussian: the mean
        want_st, want_r, want_term = _reacher_step(pre[:, :9], a)
        sc += 1
        np.testing.assert_allclose(post[0], _reacher_obs(want_st), rtol=2e-6, atol=2e-6)                          # after the step, BEFORE the reset
        np.testing.assert_allclose(rew[0], want_r, rtol=2e-6, atol=2e-6)
        assert np.array_equal((fl[0] & 1) != 0, want_term) and np.array_equal((fl[0] & 2) != 0, sc >= L), t
        sc[fl[0] != 0] = 0
    all_fl = np.concatenate([q[1] for q in ref])
    assert (all_fl & 1).any() and (all_fl & 2).any()
    # the launch length changes nothing, and neither do the neighbours
    rng = np.random.default_rng(3)
    for K in (1, 7, 64):
        rew, fl = _episodes_and_trajectories(drivers, make, E, L, K, rng)
        assert np.array_equal(rew.view(np.uint32), np.concatenate([q[0] for q in ref]).view(np.uint32)) and np.array_equal(fl, all_fl), K
    part = make(8, 8, first=16)
    rew, fl, _, act, post = part.run(3 * L, 7, True)
    assert np.array_equal(rew.view(np.uint32), np.concatenate([q[0] for q in ref])[:, 16:24].view(np.uint32)) and np.array_equal(fl, all_fl[:, 16:24])
    assert np.array_equal(act, np.concatenate([q[2] for q in ref])[:, 16:24]) and np.array_equal(post.view(np.uint32), np.concatenate([q[3] for q in ref])[:, 16:24].view(np.uint32))


def test_deterministic_host_evaluation_of_cartpole_takes_the_mode(drivers, tmp_path):
    E, L, seed, hidden = 37, 13, 300, (64, 64)                               # (env seeds 7 .. 12 all hold the env of global seed 28, which meets one near-tie of the float64 logits)
    lib = F.host_build("cartpole_eval", tmp_path)
    flat = _params(V.HostEvaluate(lib, 1).P, 5, 0.3)

    def make(E_, M=0):
        h = V.HostEvaluate(lib, E_, episode_len=L, hidden=hidden, action_start=1, M=M)
        h.set_params(flat); h.env_reset(seed)
        h.state[: E // 4, 2] = f32(0.2); h.state[: E // 4, 3] = f32(1.0)       # a quarter of the poles starts next to the 12 degree limit, falling
        return h

    h = make(E, E)
    excluded = 0
    for t in range(3 * L):
        rew, fl, pre, act, post = h.launch(1, True)
        z = V.actor_forward(flat, h.D, hidden, h.A, 0, pre)
        top = np.sort(z, axis=1)
        close = top[:, -1] - top[:, -2] < 1e-4
        excluded += int(close.sum())
        assert np.array_equal(act[0, ~close, 0].astype(np.int64), z[~close].argmax(axis=1) + 1)                   # mode(d) + action_start
    assert excluded == 0                                                       # the host build alone: no near-tie on this seed
    rng = np.random.default_rng(4)
    ref = None
    for K in (1, 7, 64):
        rew, fl = _episodes_and_trajectories(drivers, make, E, L, K, rng)
        ref = (rew, fl) if ref is None else ref
        assert np.array_equal(rew.view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(fl, ref[1])
    assert (ref[1] & 1).any() and (ref[1] & 2).any()


# ---- the normaliser -----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_expression_is_the_wrappers_line(drivers, tmp_path):
    """what the actor sees under frozen statistics: dril::normalize_obs — one definition, which nz_obs (dril_norm_wrap.h) and the plug-in's kernel both expand"""
    wrap = (ROOT / "dril.jl_amd" / "csrc" / "dril_norm_wrap.h").read_text()
    assert re.search(r"float nz_obs\(float v, float mean, float var, float eps, float clip\) \{ return dril::normalize_obs\(v, mean, var, eps, clip\); \}", wrap)
    assert "sqrtf(var + eps)" not in wrap.split("nz_reward")[0]                # no second copy of the expression next to it
    assert "dril::normalize_obs(" in (ROOT / "include" / "device" / "dril_env_evaluate.h").read_text()
    _, rows = drivers
    rng = np.random.default_rng(9)
    v = rng.normal(0, 4, (1000, 12)).astype(f32); mean = rng.normal(0, 1, 12).astype(f32); var = rng.uniform(0.05, 3, 12).astype(f32)
    got = V.normalize(rows, v, mean, var, 1e-8, 2.5)
    want = np.clip((v - mean) / np.sqrt(var + f32(1e-8), dtype=f32), f32(-2.5), f32(2.5)).astype(f32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (np.abs(got) == f32(2.5)).any()
    # the host build: a Box env's deterministic action is the actor's mean of the NORMALISED observation
    E, L, hidden = 37, 13, (64, 64)
    lib = F.host_build("reacher3_eval", tmp_path, flags=("-ffp-contract=off",))
    flat = _params(V.HostEvaluate(lib, 1).P, 5, 0.3)
    mean = rng.normal(0.2, 0.5, 12).astype(f32); var = rng.uniform(0.05, 0.6, 12).astype(f32)

    def run(norm):
        h = V.HostEvaluate(lib, E, episode_len=L, hidden=hidden, action_start=0, M=E, norm=norm)
        h.set_params(flat); h.env_reset(5)
        return h, h.launch(1, True)

    h, (rew, fl, pre, act, post) = run((mean, var, 1e-8, 1.5))
    seen = V.normalize(rows, pre, mean, var, 1e-8, 1.5)
    assert (np.abs(seen) == f32(1.5)).any() and (np.abs(seen) < f32(1.5)).any()                                  # the clip bites, and not everywhere
    np.testing.assert_allclose(act[0].view(f32), V.actor_forward(flat, h.D, hidden, h.A, 0, seen), rtol=2e-6, atol=2e-6)
    unclipped = V.actor_forward(flat, h.D, hidden, h.A, 0, V.normalize(rows, pre, mean, var, 1e-8, 1e9))
    assert np.abs(act[0].view(f32) - unclipped).max() > 1e-3
    # statistics (0, 1) and a clip that never bites: the un-normalised launch, bit for bit
    _, plain = run(None)
    _, ident = run((np.zeros(12, f32), np.ones(12, f32), 1e-8, 1e9))
    for a, b in zip(plain, ident):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- the library's side, as far as it goes without a GPU ----------------------------------------------------------------------------------------------------
def test_info_verb_is_exported_and_header_capi_and_shim_agree(pkg, tmp_path):
    capi = pkg._capi
    lib = capi.load_library()
    header = (ROOT / "include" / "dril_hip.h").read_text()
    shim = "".join(p.read_text() for p in (ROOT / "dril.jl_amd" / "julia").glob("DRiLHIP*.jl"))
    name = "dril_evaluate_fused_info"
    assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS and re.search(rf"\bint32_t\s+{name}\s*\(", header)
    assert f"(:{name}, LIB[])" in shim and hasattr(pkg.host.Handle, "evaluate_fused_info")
    assert lib.dril_evaluate_fused_info(None, None) == capi.ERR_NOT_INITIALISED                                   # a null handle fails loudly, before any GPU work
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(dril_fused_evaluate_info),'
                   ' offsetof(dril_fused_evaluate_info, tile), offsetof(dril_fused_evaluate_info, max_width), offsetof(dril_fused_evaluate_info, reason));return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    K = capi.DrilFusedEvaluateInfo
    assert [C.sizeof(K), K.tile.offset, K.max_width.offset, K.reason.offset] == list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    o = capi.DrilEvalOptions(); assert lib.dril_eval_options_default(C.byref(o)) == 0 and not any(o.reserved)     # the request stays opt-in
    t = capi.DrilTrajOptions(); assert lib.dril_traj_options_default(C.byref(t)) == 0 and not any(t.reserved)
    r = subprocess.run(["python", str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]


@pytest.mark.parametrize("name,scaled", [("cartpole", False), ("pendulum", True), ("reacher3", True)])
def test_symbols_of_the_eval_examples(name, scaled, tmp_path):
    fused = _code_object_symbols(ENVS / f"{name}_fused_plugin.hip", tmp_path / f"{name}_fused.hsaco")
    assert _code_object_symbols(ENVS / f"{name}_eval_plugin.hip", tmp_path / f"{name}_eval.hsaco") == fused | EVALUATE | (EVALUATE_SCALED if scaled else set())
