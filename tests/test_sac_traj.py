"""CPU: collect_trajectory of a SAC handle on the device (dril_sac_collect_trajectory, docs/sac.md "Trajectories"), without a GPU.

  * the two prototypes: declared in include/dril_sac.h, bound in _capi with the header's arity, exported, null arguments answered before any HIP call;
  * the per-env rule as the two launch sequences apply it (dril.jl_amd/csrc/dril_traj_record.h), built with g++ against test_traj_device's NumPy restatement of the
    reference's loop (trajectory_utils.jl:16-45), once per env: the built-in kinds' form — row 0 by traj_record_lane, then traj_record_env<D, 1> fed ONE step per
    "launch" with `length` reloaded from r.length[m] each time, as sac_traj_env_kernel does — and the plug-ins' form, traj_record_lane with W = A = 3.  No
    ClampAdapter in either (the clamp pointers are null, as the SAC verb passes them);
  * the Julia shim's new ccall passes the static check, and the check catches a wrong arity of it;
  * the Python mirror's argument handling, with the throw-away handle replaced by a stub."""
import ctypes as C
import inspect
import re
import shutil
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

from test_traj_device import GUARD, OPEN, make_data, reference_trajectory

ROOT = Path(__file__).resolve().parents[1]


# ---- bindings ------------------------------------------------------------------------------------------------------------------------------------------
def test_prototypes_are_declared_bound_and_exported(pkg):
    capi = pkg._capi
    header = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "dril_sac.h").read_text(), flags=re.S)
    P = C.c_void_p
    want = {"trajectory_capacity": [P, C.POINTER(capi.DrilTrajOptions), C.POINTER(C.c_int32)],
            "collect_trajectory": [P, C.POINTER(capi.DrilTrajOptions), P, P, P, P, P, C.POINTER(capi.DrilTrajInfo)]}
    lib = capi.load_library()
    for name, args in want.items():
        m = re.search(r"int32_t\s+dril_sac_" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(args) == len(capi._SAC_SIG[name][1]), name      # the header's arity is the binding's
        assert capi._SAC_SIG[name] == (C.c_int32, args)
        assert "dril_sac_" + name in capi.EXPORTED_SYMBOLS and getattr(lib, "dril_sac_" + name).argtypes == args
    assert "float* actions" in header[header.index("dril_sac_collect_trajectory"):]              # Box actions only: f32, not the PPO verb's void*
    assert "dril_sac_env_step" not in header                                                      # out of scope, and stays out
    sig = inspect.signature(pkg.SacHandle.collect_trajectory).parameters
    assert [(k, sig[k].default) for k in list(sig)[1:]] == [("n_trajectories", 1), ("max_steps", None), ("deterministic", True), ("seed", None), ("poll_steps", 0), ("final_original", False)]
    sig = inspect.signature(pkg.sac_collect_trajectory).parameters
    assert [(k, sig[k].default) for k in list(sig)[2:]] == [("max_steps", None), ("norm_env", None), ("deterministic", True), ("n_trajectories", 1), ("seed", None),
                                                             ("normalize", None), ("normalize_stats", None)]
    assert sig["normalize"].kind is inspect.Parameter.KEYWORD_ONLY and sig["seed"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


def test_null_handle_returns_before_any_gpu_work(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    o, info, cap = capi.DrilTrajOptions(), capi.DrilTrajInfo(), C.c_int32(77)
    lib.dril_traj_options_default(C.byref(o))
    info.capacity = 5
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.dril_sac_collect_trajectory(None, C.byref(o), p, p, p, p, p, C.byref(info)) == capi.ERR_NOT_INITIALISED
    assert lib.dril_sac_collect_trajectory(None, None, None, None, None, None, None, None) == capi.ERR_NOT_INITIALISED
    assert lib.dril_sac_trajectory_capacity(None, C.byref(o), C.byref(cap)) == capi.ERR_NOT_INITIALISED
    assert (info.capacity, cap.value) == (5, 77) and not buf.any()
    assert b"null handle" in lib.dril_sac_last_error(None)


# ---- the recording against the reference loop ----------------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include "dril_traj_record.h"
using namespace dril;
// the built-in kinds' launch: the thread of env m loads length from r.length[m], holds the row in registers, calls traj_record_env<D, 1>
template <int D> static void env_launch(const TrajRec& r, const TrajMaps& x, int t, int M, const int* order, const unsigned int* act, const float* rew,
                                        const unsigned char* term, const unsigned char* trunc, const float* obs) {
    for (int i = 0; i < M; ++i) {
        const int m = order[i];
        int length = r.length[m];
        unsigned int a[1] = {act[m]};
        float o[D];
        for (int d = 0; d < D; ++d) o[d] = obs[(size_t)m * D + d];
        traj_record_env<D, 1>(r, x, t, m, a, rew[m], term[m] != 0, trunc[m] != 0, o, length);
    }
}
extern "C" {
// One call = the row-0 launch (traj_record_lane, t = 0) and the launches of `steps` env steps.  Per-step arrays are [T][E][.], obs0 [E][D]; order [steps + 1][M * lanes]
// the sequence in which a launch's lanes run (env form: the first M entries of a row modulo M are not used — order_env [steps + 1][M]).  maps: obs_low | obs_high (D),
// act_low | act_high (W); the clamp pointers are null.  env_form: 1 = traj_record_env<D, 1> per step (W must be 1), 0 = traj_record_lane per step.
long long drive(int env_form, int E, int M, int D, int W, int Tcap, int steps, const unsigned int* act, const float* rew, const unsigned char* term, const unsigned char* trunc,
                const float* obs, const float* obs0, const int* order, const int* order_env, const float* maps, int scaled, int final_original,
                float* rec_obs, unsigned int* rec_act, float* rec_rew, int* length, unsigned char* end_flags) {
    unsigned int finished = 0;
    const TrajRec r{M, D, W, Tcap, rec_obs, rec_act, rec_rew, length, end_flags, &finished};
    const float *ol = maps, *oh = ol + D, *al = oh + D, *ah = al + W;
    const TrajMaps x{scaled ? ol : nullptr, scaled ? oh : nullptr, nullptr, nullptr, scaled ? al : nullptr, scaled ? ah : nullptr, 0, final_original};
    const int lanes = D > W ? D : W;
    for (int t = 0; t <= steps; ++t) {
        const size_t k = t ? (size_t)(t - 1) * E : 0;
        if (t == 0 || !env_form) {
            const TrajStep s = t ? TrajStep{act + k * W, rew + k, term + k, trunc + k, obs + k * D} : TrajStep{nullptr, nullptr, nullptr, nullptr, obs0};
            for (int i = 0; i < M * lanes; ++i) { const int l = order[(size_t)t * M * lanes + i]; traj_record_lane(r, x, s, t, l / lanes, l % lanes); }
            continue;
        }
        const int* oe = order_env + (size_t)t * M;
        switch (D) {
            case 1: env_launch<1>(r, x, t, M, oe, act + k, rew + k, term + k, trunc + k, obs + k * D); break;
            case 2: env_launch<2>(r, x, t, M, oe, act + k, rew + k, term + k, trunc + k, obs + k * D); break;
            case 3: env_launch<3>(r, x, t, M, oe, act + k, rew + k, term + k, trunc + k, obs + k * D); break;
            case 4: env_launch<4>(r, x, t, M, oe, act + k, rew + k, term + k, trunc + k, obs + k * D); break;
            case 5: env_launch<5>(r, x, t, M, oe, act + k, rew + k, term + k, trunc + k, obs + k * D); break;
            default: return -1;
        }
    }
    return finished;
}
void reorder(long long M, long long D, long long W, long long Tcap, const int* length, const float* obs_tm, const unsigned int* act_tm, const float* rew_tm,
             float* obs, unsigned int* act, float* rew) { traj_reorder(M, D, W, Tcap, length, obs_tm, act_tm, rew_tm, obs, act, rew); }
}
'''


@pytest.fixture(scope="module")
def rec(tmp_path_factory):
    d = tmp_path_factory.mktemp("sac_traj_record")
    src = d / "drive.cpp"; src.write_text(_DRIVER)
    so = d / "drive.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / "dril.jl_amd" / "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.drive.restype = C.c_longlong
    lib.drive.argtypes = [C.c_int] * 7 + [C.c_void_p] * 9 + [C.c_int] * 2 + [C.c_void_p] * 5
    lib.reorder.argtypes = [C.c_longlong] * 4 + [C.c_void_p] * 7
    return lib


def make_maps(rng, D, W, scaled, final_original):
    """test_traj_device's nine-tuple with the clamp switched off (clamp_low == clamp_high: reference_trajectory clamps where low < high)"""
    ol = -rng.uniform(0.5, 9, D).astype(np.float32); oh = rng.uniform(0.5, 9, D).astype(np.float32)
    al = -rng.uniform(0.5, 3, W).astype(np.float32); ah = rng.uniform(0.5, 3, W).astype(np.float32)
    z = np.zeros(W, np.float32)
    return ol, oh, z, z.copy(), al, ah, scaled, False, final_original


def run_recording(rec, env_form, data, E, M, D, W, Tcap, steps, maps, rng):
    act, rew, term, trunc, obs, obs0 = data
    ol, oh, _, _, al, ah, scaled, _, final_original = maps
    table = np.concatenate([ol, oh, al, ah]).astype(np.float32)
    lanes = max(D, W)
    order = np.stack([rng.permutation(M * lanes) for _ in range(steps + 1)]).astype(np.int32)
    order_env = np.stack([rng.permutation(M) for _ in range(steps + 1)]).astype(np.int32)
    rec_obs = np.full(((Tcap + 1) * M * D + GUARD,), -7, np.float32); rec_act = np.full((Tcap * M * W + GUARD,), 0xABCD, np.uint32)
    rec_rew = np.full((Tcap * M + GUARD,), -7, np.float32); length = np.full(M + GUARD, -7, np.int32); flags = np.full(M + GUARD, 0xEE, np.uint8)
    p = lambda a: a.ctypes.data
    finished = rec.drive(int(env_form), E, M, D, W, Tcap, steps, p(act), p(rew), p(term), p(trunc), p(obs), p(obs0), p(order), p(order_env), p(table), int(scaled),
                         int(final_original), p(rec_obs), p(rec_act), p(rec_rew), p(length), p(flags))
    assert (rec_obs[-GUARD:] == -7).all() and (rec_act[-GUARD:] == 0xABCD).all() and (rec_rew[-GUARD:] == -7).all() and (length[M:] == -7).all() and (flags[M:] == 0xEE).all()
    return finished, rec_obs[:-GUARD], rec_act[:-GUARD], rec_rew[:-GUARD], length[:M], flags[:M]


def check_rule(rec, E, env_form):
    rng = np.random.default_rng((900 if env_form else 1700) + E)
    limit = 9
    scaled, final_original = bool(E % 2), E % 4 == 1
    D = 1 + E % 5
    W = 1 if env_form else 3
    T = limit + 31
    data = make_data(rng, T, E, D, W, limit, False)
    maps = make_maps(rng, D, W, scaled, final_original)
    for max_steps in (1, 5, 0):
        Tcap = max_steps if 0 < max_steps < limit else limit
        want = [reference_trajectory(m, data, max_steps, maps) for m in range(E)]
        for o, a, r, f in want:
            assert len(o) == len(a) + 1 == len(r) + 1 and 1 <= len(r) <= Tcap
        if max_steps == 5 and E > 3:        # an episode of length 1; done and cut in one step (the end wins); cut one step before the end
            assert want[0][3] == 1 and len(want[0][2]) == 1 and want[2][3] == 1 and len(want[2][2]) == 5 and want[3][3] == 4 and len(want[3][2]) == 5
        if max_steps == 0 and E > 1:        # an episode of exactly Tcap
            assert want[1][3] == 2 and len(want[1][2]) == limit == Tcap
        if max_steps == 1:
            assert all(len(w[2]) == 1 for w in want) and (E < 2 or want[1][3] == 4)
        for M in range(1, E + 1):
            longest = max(len(w[2]) for w in want[:M])
            for extra in (0, 1, 31):        # steps past the last finish, and with them a second episode of a fast env (env 0 ends at step 1), change nothing
                if extra and M not in (1, E, (E + 1) // 2):
                    continue
                finished, o_tm, a_tm, r_tm, length, flags = run_recording(rec, env_form, data, E, M, D, W, Tcap, longest + extra, maps, rng)
                assert finished == M, (E, M, max_steps, extra)
                assert length.tolist() == [len(w[2]) for w in want[:M]] and flags.tolist() == [w[3] for w in want[:M]]
                obs = np.full((M, Tcap + 1, D), np.nan, np.float32); act = np.full((M, Tcap, W), 7, np.uint32); rw = np.full((M, Tcap), np.nan, np.float32)
                p = lambda x: x.ctypes.data
                rec.reorder(M, D, W, Tcap, p(length), p(o_tm), p(a_tm), p(r_tm), p(obs), p(act), p(rw))
                for m in range(M):
                    o, a, r, _ = want[m]
                    L = len(r)
                    assert np.array_equal(obs[m, :L + 1].view(np.uint32), o.view(np.uint32)), (E, M, m, max_steps)
                    assert np.array_equal(act[m, :L], a.reshape(L, W)) and np.array_equal(rw[m, :L].view(np.uint32), r.view(np.uint32))
                    assert not obs[m, L + 1:].any() and not act[m, L:].any() and not rw[m, L:].any()
            if M > 1:                       # an open trajectory stops the count
                finished, *_rest, length, flags = run_recording(rec, env_form, data, E, M, D, W, Tcap, longest - 1, maps, rng)
                n_open = sum(len(w[2]) == longest for w in want[:M])
                assert finished == M - n_open and (length == OPEN).sum() == n_open


@pytest.mark.parametrize("E", list(range(1, 41)))
def test_builtin_rule_follows_the_reference_loop_per_env(rec, E):
    check_rule(rec, E, env_form=True)


@pytest.mark.parametrize("E", list(range(1, 41)))
def test_plugin_rule_follows_the_reference_loop_per_env(rec, E):
    check_rule(rec, E, env_form=False)


# ---- the shim ------------------------------------------------------------------------------------------------------------------------------------------
def test_shim_check_passes_and_catches_a_wrong_arity_of_the_new_ccall(tmp_path):
    tool = ROOT / "tools" / "check_shim.py"
    shim_dir = ROOT / "dril.jl_amd" / "julia"
    r = subprocess.run([sys.executable, str(tool)], capture_output=True, text=True)
    assert r.returncode == 0 and "check_shim: ok" in r.stdout, r.stdout[-2000:]
    for f in shim_dir.glob("DRiLHIP*.jl"): shutil.copy(f, tmp_path / f.name)
    sac = tmp_path / "DRiLHIP_sac.jl"
    text = sac.read_text()
    assert "function DRiL.collect_trajectory(agent::SACAgent, env::DeviceParallelEnv; max_steps" in text and "ccall((:dril_sac_collect_trajectory, LIB[])" in text
    good = "(Ptr{Cvoid}, Ref{DrilTrajOptions}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Ptr{UInt8}, Ptr{DrilTrajInfo})"
    assert text.count(good) == 1
    sac.write_text(text.replace(good, good.replace(", Ptr{DrilTrajInfo})", ")")))
    r = subprocess.run([sys.executable, str(tool), "--shim", str(tmp_path / "DRiLHIP.jl")], capture_output=True, text=True)
    assert r.returncode == 1 and "ccall dril_sac_collect_trajectory" in r.stdout and "7 argument types" in r.stdout, r.stdout[-1500:]
    sac.write_text(text.replace("(:dril_sac_trajectory_capacity, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilTrajOptions}, Ref{Int32})", "(:dril_sac_trajectory_capacity, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilTrajOptions}, Int32)"))
    r = subprocess.run([sys.executable, str(tool), "--shim", str(tmp_path / "DRiLHIP.jl")], capture_output=True, text=True)
    assert r.returncode == 1 and "ccall dril_sac_trajectory_capacity" in r.stdout and "argument 3" in r.stdout, r.stdout[-1500:]


# ---- the Python mirror's argument handling ---------------------------------------------------------------------------------------------------------------
class _StubHandle:
    def __init__(self, flags):
        self.flags, self.calls, self.closed = np.asarray(flags, np.uint8), [], False

    def collect_trajectory(self, n_trajectories, max_steps, deterministic, seed):
        self.calls.append((n_trajectories, max_steps, deterministic, seed))
        trajs = [(np.full((m + 3, 2), m, np.float32), np.zeros((m + 2, 1), np.float32), np.ones(m + 2, np.float32)) for m in range(n_trajectories)]
        return trajs, np.arange(n_trajectories, dtype=np.int32) + 2, self.flags[:n_trajectories], {}

    def close(self):
        self.closed = True


def test_python_mirror_argument_handling(pkg, monkeypatch):
    sac = sys.modules[pkg.sac_collect_trajectory.__module__]
    env = pkg.DeviceParallelEnv(pkg.PendulumEnv(), 4, seed=11)
    agent = object()
    built = []

    def stub(agent_, env_, normalize, normalize_stats, who, what):
        built.append((_StubHandle([2, 4, 2, 1]), normalize, normalize_stats, who))
        return built[-1][0]
    monkeypatch.setattr(sac, "_sac_throwaway_handle", stub)
    # the refusals come before any handle is built
    with pytest.raises(NotImplementedError, match="norm_env is None or the env itself"):
        pkg.sac_collect_trajectory(agent, env, norm_env=object())
    with pytest.raises(NotImplementedError, match="norm_env is None or the env itself"):
        pkg.sac_collect_trajectory(agent, env, norm_env=pkg.DeviceParallelEnv(pkg.PendulumEnv(), 4, seed=11))
    with pytest.raises(NotImplementedError, match="live with the caller"):
        pkg.sac_collect_trajectory(agent, pkg.HostParallelEnv([], seed=0))
    with pytest.raises(NotImplementedError, match="live with the caller"):
        pkg.sac_collect_trajectory(agent, object.__new__(pkg.DeviceArrayParallelEnv))
    assert not built
    # one trajectory: the reference's triple; the env's seed; no warning where bit 2 is clear
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = pkg.sac_collect_trajectory(agent, env, norm_env=env, normalize_stats="fresh")
    assert isinstance(out, tuple) and len(out) == 3 and out[0].shape == (3, 2) and out[1].shape == (2, 1) and out[2].shape == (2,)
    assert not any("Max steps reached" in str(w.message) for w in caught)
    h, normalize, stats, who = built[-1]
    assert h.calls == [(1, None, True, 11)] and h.closed and normalize is None and stats == "fresh" and who == "sac_collect_trajectory"
    # several: a list of triples, and the warning where a trajectory was cut
    with pytest.warns(UserWarning, match="Max steps reached"):
        many = pkg.sac_collect_trajectory(agent, env, 5, None, False, 3, 99, normalize=dict(norm_obs=True))
    assert isinstance(many, list) and len(many) == 3 and all(len(t) == 3 for t in many) and many[2][0].shape == (5, 2)
    h, normalize, stats, _ = built[-1]
    assert h.calls == [(3, 5, False, 99)] and h.closed and normalize == dict(norm_obs=True) and stats is None
    with pytest.raises(ValueError, match="max_steps is None or >= 1"):
        pkg.SacHandle.collect_trajectory(object.__new__(pkg.SacHandle), max_steps=0)
