"""CPU: collect_trajectory of a PPO handle on the device (dril_collect_trajectory_device, docs/evaluation.md, "Trajectories"), without a GPU.

  * the two structs and prototypes: ctypes layout == a C compile of include/dril_hip.h, the defaults, null arguments before any HIP call, the capacity rule;
  * the per-env recording the kernel runs (dril.jl_amd/csrc/dril_traj_record.h) and the host's reorder, built with g++ and driven lane by lane with recorded step
    arrays, against a NumPy restatement of the reference's loop (trajectory_utils.jl:16-45), once per env;
  * the Julia shim's new ccall passes the static check, and the check catches a wrong arity of it."""
import ctypes as C
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
OPEN = 0x7F7F7F7F


# ---- structs and prototypes --------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_a_c_compile_of_the_header(pkg, tmp_path):
    capi = pkg._capi
    fields = {"dril_traj_options": ("n_trajectories", "max_steps", "deterministic", "has_seed", "seed", "poll_steps", "final_original", "reserved"),
              "dril_traj_info": ("capacity", "steps_enqueued", "launches", "longest", "cut_by_max_steps", "reserved")}
    body = "".join(f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {f}));' for f in fs) + 'printf("\\n");' for s, fs in fields.items())
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_hip.h"\nint main(){' + body + "return 0;}")
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for (s, fs), line, K in zip(fields.items(), lines, (capi.DrilTrajOptions, capi.DrilTrajInfo)):
        want = [int(x) for x in line.split()]
        assert [C.sizeof(K)] + [getattr(K, f).offset for f in fs] == want, s
        assert tuple(n for n, _ in K._fields_) == fs
    assert C.sizeof(capi.DrilTrajOptions) == 56 and capi.DrilTrajOptions.seed.offset == 16 and C.sizeof(capi.DrilTrajInfo) == 32
    # the ABI numbers this change must not move
    header = (ROOT / "include" / "dril_hip.h").read_text()
    assert "#define DRIL_ABI_VERSION 2u" in header and capi.ABI_VERSION == 2
    assert C.sizeof(capi.DrilEvalOptions) == 40 and C.sizeof(capi.DrilEvalInfo) == 32


def test_defaults_exports_and_python_surface(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    for name in ("dril_traj_options_default", "dril_trajectory_capacity", "dril_collect_trajectory_device"):
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    P = C.c_void_p
    assert lib.dril_collect_trajectory_device.argtypes == [P, C.POINTER(capi.DrilTrajOptions), P, P, P, P, P, C.POINTER(capi.DrilTrajInfo)]
    o = capi.DrilTrajOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    assert lib.dril_traj_options_default(C.byref(o)) == capi.OK
    assert (o.n_trajectories, o.max_steps, o.deterministic, o.has_seed, o.seed, o.poll_steps, o.final_original, tuple(o.reserved)) == (1, 0, 1, 0, 0, 0, 0, (0,) * 5)
    assert lib.dril_traj_options_default(None) == capi.ERR_INVALID_ARG
    assert (capi.TRAJ_TERMINATED, capi.TRAJ_TRUNCATED, capi.TRAJ_MAX_STEPS) == (1, 2, 4)
    import inspect
    sig = inspect.signature(pkg.Handle.collect_trajectory_device).parameters
    assert [(k, sig[k].default) for k in list(sig)[1:]] == [("n_trajectories", 1), ("max_steps", None), ("deterministic", True), ("seed", None), ("poll_steps", 0), ("final_original", False)]
    sig = inspect.signature(pkg.collect_trajectory).parameters
    assert [(k, sig[k].default) for k in list(sig)[2:]] == [("max_steps", None), ("norm_env", None), ("deterministic", True), ("n_trajectories", 1), ("seed", None)]


def test_null_handle_returns_before_any_gpu_work(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    o, info, cap = capi.DrilTrajOptions(), capi.DrilTrajInfo(), C.c_int32(77)
    lib.dril_traj_options_default(C.byref(o))
    info.capacity = 5
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.dril_collect_trajectory_device(None, C.byref(o), p, p, p, p, p, C.byref(info)) == capi.ERR_NOT_INITIALISED
    assert lib.dril_collect_trajectory_device(None, None, None, None, None, None, None, None) == capi.ERR_NOT_INITIALISED
    assert lib.dril_trajectory_capacity(None, C.byref(o), C.byref(cap)) == capi.ERR_NOT_INITIALISED
    assert (info.capacity, cap.value) == (5, 77) and not buf.any()
    assert b"null handle" in lib.dril_last_error(None)


# ---- the recording against the reference loop ----------------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <vector>
#include "dril_traj_record.h"
extern "C" {
int capacity(int max_steps, int episode_len) { return dril::traj_capacity(max_steps, episode_len); }
long long bytes(long long M, long long Tcap, long long D, long long W) { return dril::traj_bytes(M, Tcap, D, W); }
// One call = the launches of `steps` env steps after the step-0 launch.  Per-step arrays are [T][E][.] (obs: the shadow envs' post-step, pre-reset observation), obs0
// [E][D]; order [steps + 1][M * lanes]: the sequence in which the lanes of a launch run (a kernel's threads have none).  maps: obs_low | obs_high (D), clamp_low |
// clamp_high | act_low | act_high (W); scaled / discrete / final_original as TrajMaps.  rec_*: the step-major recording; returns the finished-counter.
long long drive(int E, int M, int D, int W, int Tcap, int steps, const unsigned int* act, const float* rew, const unsigned char* term, const unsigned char* trunc,
                const float* obs, const float* obs0, const int* order, const float* maps, int scaled, int discrete, int final_original,
                float* rec_obs, unsigned int* rec_act, float* rec_rew, int* length, unsigned char* end_flags) {
    unsigned int finished = 0;
    const dril::TrajRec r{M, D, W, Tcap, rec_obs, rec_act, rec_rew, length, end_flags, &finished};
    const float *ol = maps, *oh = ol + D, *cl = oh + D, *ch = cl + W, *al = ch + W, *ah = al + W;
    const dril::TrajMaps x{scaled ? ol : nullptr, scaled ? oh : nullptr, discrete ? nullptr : cl, discrete ? nullptr : ch, (scaled && !discrete) ? al : nullptr,
                           (scaled && !discrete) ? ah : nullptr, discrete, final_original};
    const int lanes = D > W ? D : W;
    for (int t = 0; t <= steps; ++t) {
        const size_t k = t ? (size_t)(t - 1) * E : 0;
        const dril::TrajStep s = t ? dril::TrajStep{act + k * W, rew + k, term + k, trunc + k, obs + k * D} : dril::TrajStep{nullptr, nullptr, nullptr, nullptr, obs0};
        for (int i = 0; i < M * lanes; ++i) { const int l = order[(size_t)t * M * lanes + i]; dril::traj_record_lane(r, x, s, t, l / lanes, l % lanes); }
    }
    return finished;
}
void reorder(long long M, long long D, long long W, long long Tcap, const int* length, const float* obs_tm, const unsigned int* act_tm, const float* rew_tm,
             float* obs, unsigned int* act, float* rew) { dril::traj_reorder(M, D, W, Tcap, length, obs_tm, act_tm, rew_tm, obs, act, rew); }
}
'''


@pytest.fixture(scope="module")
def rec(tmp_path_factory):
    d = tmp_path_factory.mktemp("traj_record")
    src = d / "drive.cpp"; src.write_text(_DRIVER)
    so = d / "drive.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / "dril.jl_amd" / "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.capacity.argtypes = [C.c_int, C.c_int]
    lib.bytes.restype = C.c_longlong; lib.bytes.argtypes = [C.c_longlong] * 4
    lib.drive.restype = C.c_longlong
    lib.drive.argtypes = [C.c_int] * 6 + [C.c_void_p] * 8 + [C.c_int] * 3 + [C.c_void_p] * 5
    lib.reorder.argtypes = [C.c_longlong] * 4 + [C.c_void_p] * 7
    return lib


def test_capacity_rule_and_recording_size(rec):
    """Tcap = max_steps > 0 ? min(max_steps, episode_len) : episode_len; the 1 GiB bound is on 4 M ((Tcap + 1) D + Tcap W + Tcap) + 5 M bytes, in 64 bits"""
    for max_steps, limit, want in ((0, 200, 200), (1, 200, 1), (5, 200, 5), (200, 200, 200), (201, 200, 200), (10 ** 9, 7, 7), (3, 1, 1)):
        assert rec.capacity(max_steps, limit) == want
    assert rec.bytes(3, 5, 4, 1) == 4 * 3 * (6 * 4 + 5 + 5) + 15
    assert rec.bytes(2 ** 20, 999, 1024, 64) == 4 * 2 ** 20 * (1000 * 1024 + 999 * 64 + 999) + 5 * 2 ** 20 > 2 ** 40


def unscale(x, lo, hi):
    """unscale_from_unit (include/device/dril_scaling.h), float32 operation by operation"""
    sf = np.float32(2) / (hi - lo)
    return (x + np.float32(1)) / sf + lo


def reference_trajectory(m, data, max_steps, maps):
    """trajectory_utils.jl:16-45 for env m alone, on the recorded arrays: observe / unscale / push, predict (to_env, unscale!) / push, act! / push, the cut, the final
    observe — and the episode's end taking precedence over the cut where both fall on one step (the verb's contract)"""
    act, rew, term, trunc, obs, obs0 = data
    ol, oh, cl, ch, al, ah, scaled, discrete, final_original = maps
    observations, actions, rewards = [], [], []
    cur, t, flags = obs0[m], 0, 0
    while True:
        observations.append(unscale(cur, ol, oh) if scaled else cur)                   # :17-23
        a = act[t, m]
        if not discrete:
            a = a.view(np.float32)
            clamp = cl < ch
            a = np.where(clamp, np.minimum(np.maximum(a, cl), ch), a)                  # to_env: ClampAdapter on the agent-facing Box
            if scaled:
                a = unscale(a, al, ah)                                                 # :30-32
            a = a.astype(np.float32).view(np.uint32)
        actions.append(a); rewards.append(rew[t, m])                                   # :34-37
        cur = obs[t, m]
        done = bool(term[t, m] or trunc[t, m])
        t += 1
        if done:
            flags = int(term[t - 1, m]) | int(trunc[t - 1, m]) << 1
            break
        if max_steps and len(observations) >= max_steps:                               # :38-41
            flags = 4
            break
    observations.append(unscale(cur, ol, oh) if scaled and final_original else cur)    # :44
    return np.stack(observations), np.stack(actions), np.asarray(rewards, np.float32), flags


GUARD = 3


def run_recording(rec, data, E, M, D, W, Tcap, steps, maps, rng):
    act, rew, term, trunc, obs, obs0 = data
    ol, oh, cl, ch, al, ah, scaled, discrete, final_original = maps
    table = np.concatenate([ol, oh, cl, ch, al, ah]).astype(np.float32)
    lanes = max(D, W)
    order = np.stack([rng.permutation(M * lanes) for _ in range(steps + 1)]).astype(np.int32)
    rec_obs = np.full(((Tcap + 1) * M * D + GUARD,), -7, np.float32); rec_act = np.full((Tcap * M * W + GUARD,), 0xABCD, np.uint32)
    rec_rew = np.full((Tcap * M + GUARD,), -7, np.float32); length = np.full(M + GUARD, -7, np.int32); flags = np.full(M + GUARD, 0xEE, np.uint8)
    p = lambda a: a.ctypes.data
    finished = rec.drive(E, M, D, W, Tcap, steps, p(act), p(rew), p(term), p(trunc), p(obs), p(obs0), p(order), p(table), int(scaled), int(discrete), int(final_original),
                         p(rec_obs), p(rec_act), p(rec_rew), p(length), p(flags))
    assert (rec_obs[-GUARD:] == -7).all() and (rec_act[-GUARD:] == 0xABCD).all() and (rec_rew[-GUARD:] == -7).all() and (length[M:] == -7).all() and (flags[M:] == 0xEE).all()
    return finished, rec_obs[:-GUARD], rec_act[:-GUARD], rec_rew[:-GUARD], length[:M], flags[:M]


def make_data(rng, T, E, D, W, limit, discrete):
    act = rng.integers(0, 3, (T, E, W)).astype(np.uint32) if discrete else rng.normal(0, 1.5, (T, E, W)).astype(np.float32).view(np.uint32)
    rew = rng.normal(0, 3, (T, E)).astype(np.float32)
    term = rng.random((T, E)) < 0.15
    trunc = np.zeros((T, E), bool)
    for e in range(E):                                                                 # the time limit: `limit` steps after the episode's start, as the envs truncate
        start = 0
        for t in range(T):
            if t - start + 1 >= limit:
                trunc[t, e] = True
            if term[t, e] or trunc[t, e]:
                start = t + 1
    if E > 0:
        term[0, 0] = True                                                              # an episode of length 1 (and a second, third, ... episode of a fast env after it)
    if E > 1:
        term[:limit, 1] = False; trunc[:limit - 1, 1] = False; trunc[limit - 1, 1] = True   # an episode of exactly the time limit
    if E > 2 and limit > 5:
        term[:5, 2] = False; term[4, 2] = True                                         # done at step 5: with max_steps = 5, done and cut in the same step
    if E > 3 and limit > 5:
        term[:6, 3] = False; term[5, 3] = True                                         # done at step 6: with max_steps = 5, cut one step before its end
    obs = rng.normal(0, 1, (T, E, D)).astype(np.float32)
    obs0 = rng.normal(0, 1, (E, D)).astype(np.float32)
    return tuple(np.ascontiguousarray(a) for a in (act, rew, term.astype(np.uint8), trunc.astype(np.uint8), obs, obs0))


def make_maps(rng, D, W, scaled, discrete, final_original):
    ol = -rng.uniform(0.5, 9, D).astype(np.float32); oh = rng.uniform(0.5, 9, D).astype(np.float32)
    al = -rng.uniform(0.5, 3, W).astype(np.float32); ah = rng.uniform(0.5, 3, W).astype(np.float32)
    cl, ch = (np.full(W, -1, np.float32), np.full(W, 1, np.float32)) if scaled else (al.copy(), ah.copy())
    if not scaled and W > 1:
        cl[-1] = ch[-1] = 0                                                            # a dimension without bounds: no clamp
    return ol, oh, cl, ch, al, ah, scaled, discrete, final_original


@pytest.mark.parametrize("E", list(range(1, 41)))
def test_recording_follows_the_reference_loop_per_env(rec, E):
    rng = np.random.default_rng(500 + E)
    limit = 9
    scaled, discrete, final_original = bool(E % 2), E % 3 == 0, E % 4 == 1
    D = 1 + E % 5
    W = 1 if discrete else 1 + E % 3
    T = limit + 31
    data = make_data(rng, T, E, D, W, limit, discrete)
    maps = make_maps(rng, D, W, scaled, discrete, final_original)
    for max_steps in (1, 5, 0):
        Tcap = rec.capacity(max_steps, limit)
        want = [reference_trajectory(m, data, max_steps, maps) for m in range(E)]
        for m, (o, a, r, f) in enumerate(want):
            assert len(o) == len(a) + 1 == len(r) + 1 and 1 <= len(r) <= Tcap
        if max_steps == 5 and E > 3:
            assert want[0][3] == 1 and len(want[0][2]) == 1 and want[2][3] == 1 and len(want[2][2]) == 5 and want[3][3] == 4 and len(want[3][2]) == 5
        if max_steps == 0 and E > 1:
            assert want[1][3] == 2 and len(want[1][2]) == limit == Tcap
        if max_steps == 1:
            assert all(len(w[2]) == 1 for w in want) and (E < 2 or want[1][3] == 4)
        for M in range(1, E + 1):
            longest = max(len(w[2]) for w in want[:M])
            for extra in (0, 1, 31):                                                   # steps enqueued past the last finish change nothing
                if extra and M not in (1, E, (E + 1) // 2):
                    continue
                finished, o_tm, a_tm, r_tm, length, flags = run_recording(rec, data, E, M, D, W, Tcap, longest + extra, maps, rng)
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
                    assert not obs[m, L + 1:].any() and not act[m, L:].any() and not rw[m, L:].any()   # rows past the trajectory's own length are zero
            if M > 1:                                                                  # an open trajectory stops the count: one step short of the longest, one is missing
                finished, *_rest, length, flags = run_recording(rec, data, E, M, D, W, Tcap, longest - 1, maps, rng)
                n_open = sum(len(w[2]) == longest for w in want[:M])
                assert finished == M - n_open and (length == OPEN).sum() == n_open


# ---- the shim -----------------------------------------------------------------------------------------------------------------------------------------
def test_shim_check_passes_and_catches_a_wrong_arity_of_the_new_ccall(tmp_path):
    tool = ROOT / "tools" / "check_shim.py"
    shim_dir = ROOT / "dril.jl_amd" / "julia"
    r = subprocess.run([sys.executable, str(tool)], capture_output=True, text=True)
    assert r.returncode == 0 and "check_shim: ok" in r.stdout, r.stdout[-2000:]
    for f in shim_dir.glob("DRiLHIP*.jl"): shutil.copy(f, tmp_path / f.name)
    extras = tmp_path / "DRiLHIP_extras.jl"
    good = "ccall((:dril_collect_trajectory_device, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilTrajOptions}, Ptr{Float32}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Int32}, Ptr{UInt8}, Ptr{DrilTrajInfo})"
    text = extras.read_text()
    assert good in text and "function DRiL.collect_trajectory(agent, env::DeviceParallelEnv; max_steps" in text
    extras.write_text(text.replace(good, good.replace(", Ptr{DrilTrajInfo})", ")")))
    r = subprocess.run([sys.executable, str(tool), "--shim", str(tmp_path / "DRiLHIP.jl")], capture_output=True, text=True)
    assert r.returncode == 1 and "ccall dril_collect_trajectory_device" in r.stdout and "7 argument types" in r.stdout, r.stdout[-1500:]
    extras.write_text(text.replace("    poll_steps::Int32; final_original::Int32\n", ""))   # a mirror struct that lost two fields
    r = subprocess.run([sys.executable, str(tool), "--shim", str(tmp_path / "DRiLHIP.jl")], capture_output=True, text=True)
    assert r.returncode == 1 and "DrilTrajOptions fields" in r.stdout, r.stdout[-1500:]
