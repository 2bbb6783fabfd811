"""CPU: the opt-in modes of the persistent evaluate kernel (docs/evaluation.md: a frozen NormalizeWrapperEnv and the trajectory recording inside the kernel), without a GPU.

  * the per-env record function the kernel compiles (traj_record_env, dril.jl_amd/csrc/dril_traj_record.h), built with g++ and driven as the kernel drives it — one
    lane per env, the open / closed state in a local across the steps of a launch and in length[m] across launches of 1 / 7 / 64 steps, the envs of a launch in
    random order — against the NumPy restatement of trajectory_utils.jl:16-45 of tests/test_traj_device.py, and against traj_record_lane on the same step stream,
    every array slot for slot;
  * the request words: the defaults leave them 0, the header's slot numbers are the Python mirror's, the Python keywords reach the struct and info["path"] comes back;
  * the Julia shim takes the keyword, passes the static check, and the check catches a wrong arity."""
import ctypes as C
import inspect
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_traj_device import _DRIVER, GUARD, OPEN, make_data, make_maps, reference_trajectory, run_recording

ROOT = Path(__file__).resolve().parents[1]

# the kernel's form: launches of K steps; per launch every recorded env once, in the given order (the waves of a launch have none), with its length word in a local
_ENV_DRIVER = _DRIVER + r'''
template <int D, int W>
static long long drive_env_t(int E, int M, int Tcap, int steps, int K, const unsigned int* act, const float* rew, const unsigned char* term, const unsigned char* trunc,
                             const float* obs, const float* obs0, const int* order, const float* maps, int scaled, int discrete, int final_original,
                             float* rec_obs, unsigned int* rec_act, float* rec_rew, int* length, unsigned char* end_flags) {
    unsigned int finished = 0;
    const dril::TrajRec r{M, D, W, Tcap, rec_obs, rec_act, rec_rew, length, end_flags, &finished};
    const float *ol = maps, *oh = ol + D, *cl = oh + D, *ch = cl + W, *al = ch + W, *ah = al + W;
    const dril::TrajMaps x{scaled ? ol : nullptr, scaled ? oh : nullptr, discrete ? nullptr : cl, discrete ? nullptr : ch, (scaled && !discrete) ? al : nullptr,
                           (scaled && !discrete) ? ah : nullptr, discrete, final_original};
    int launch = 0;
    for (int t0 = 0; t0 < steps || t0 == 0; t0 += K, ++launch) {
        const int n = steps - t0 < K ? steps - t0 : K;
        for (int i = 0; i < M; ++i) {
            const int m = order[(size_t)launch * M + i];
            int32_t len = -12345;                                                  // the lane's register: set by row 0, or loaded where a launch continues
            float o[D]; uint32_t a[W];
            if (t0 == 0) {
                for (int j = 0; j < D; ++j) o[j] = obs0[(size_t)m * D + j];
                for (int j = 0; j < W; ++j) a[j] = 0u;
                dril::traj_record_env<D, W>(r, x, 0, m, a, 0.f, false, false, o, len);
            } else len = length[m];
            for (int k = 0; k < n; ++k) {
                const int t = t0 + k + 1; const size_t idx = (size_t)(t - 1) * E + m;
                for (int j = 0; j < D; ++j) o[j] = obs[idx * D + j];
                for (int j = 0; j < W; ++j) a[j] = act[idx * W + j];
                dril::traj_record_env<D, W>(r, x, t, m, a, rew[idx], term[idx] != 0, trunc[idx] != 0, o, len);
            }
        }
    }
    return finished;
}
extern "C" long long drive_env(int E, int M, int D, int W, int Tcap, int steps, int K, const unsigned int* act, const float* rew, const unsigned char* term,
                               const unsigned char* trunc, const float* obs, const float* obs0, const int* order, const float* maps, int scaled, int discrete,
                               int final_original, float* rec_obs, unsigned int* rec_act, float* rec_rew, int* length, unsigned char* end_flags) {
#define CASE(DD, WW) if (D == DD && W == WW) return drive_env_t<DD, WW>(E, M, Tcap, steps, K, act, rew, term, trunc, obs, obs0, order, maps, scaled, discrete, \
                                                                        final_original, rec_obs, rec_act, rec_rew, length, end_flags);
#define ROW(DD) CASE(DD, 1) CASE(DD, 2) CASE(DD, 3)
    ROW(1) ROW(2) ROW(3) ROW(4) ROW(5)
    return -1;
}
'''


@pytest.fixture(scope="module")
def rec(tmp_path_factory):
    d = tmp_path_factory.mktemp("traj_record_env")
    src = d / "drive.cpp"; src.write_text(_ENV_DRIVER)
    so = d / "drive.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / "dril.jl_amd" / "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.capacity.argtypes = [C.c_int, C.c_int]
    lib.drive.restype = C.c_longlong
    lib.drive.argtypes = [C.c_int] * 6 + [C.c_void_p] * 8 + [C.c_int] * 3 + [C.c_void_p] * 5
    lib.drive_env.restype = C.c_longlong
    lib.drive_env.argtypes = [C.c_int] * 7 + [C.c_void_p] * 8 + [C.c_int] * 3 + [C.c_void_p] * 5
    lib.reorder.argtypes = [C.c_longlong] * 4 + [C.c_void_p] * 7
    return lib


def fresh_arrays(M, D, W, Tcap):
    """the fill patterns of test_traj_device.run_recording: whatever neither form writes is equal in both"""
    return (np.full(((Tcap + 1) * M * D + GUARD,), -7, np.float32), np.full((Tcap * M * W + GUARD,), 0xABCD, np.uint32), np.full((Tcap * M + GUARD,), -7, np.float32),
            np.full(M + GUARD, -7, np.int32), np.full(M + GUARD, 0xEE, np.uint8))


def run_env_form(rec, data, E, M, D, W, Tcap, steps, K, maps, rng):
    act, rew, term, trunc, obs, obs0 = data
    ol, oh, cl, ch, al, ah, scaled, discrete, final_original = maps
    table = np.concatenate([ol, oh, cl, ch, al, ah]).astype(np.float32)
    launches = max(1, -(-steps // K))
    order = np.stack([rng.permutation(M) for _ in range(launches)]).astype(np.int32)
    arrays = fresh_arrays(M, D, W, Tcap)
    p = lambda a: a.ctypes.data
    finished = rec.drive_env(E, M, D, W, Tcap, steps, K, p(act), p(rew), p(term), p(trunc), p(obs), p(obs0), p(order), p(table), int(scaled), int(discrete),
                             int(final_original), *[p(a) for a in arrays])
    assert finished >= 0, "no instantiation for this (D, W)"
    return finished, arrays


@pytest.mark.parametrize("E", list(range(1, 41)))
def test_the_per_env_record_function_follows_the_reference_loop_and_the_lane_form(rec, E):
    """test_traj_device's cases (its data and maps: an episode of length 1 and later episodes of that fast env, an episode of exactly Tcap, done and cut on one step,
    a cut one step before the end; scaling maps on / off, Discrete / Box with 1-3 words, final_original 0 / 1), max_steps 1 / 5 / none, M = 1 .. E, launches of
    1 / 7 / 64 steps, the last one shortened at Tcap as the host loop shortens it, and 0 / 1 / 31 steps past the last finish where the capacity leaves room"""
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
        if max_steps == 5 and E > 3:                                                   # length 1; done and cut on one step; cut one step before the end
            assert want[0][3] == 1 and len(want[0][2]) == 1 and want[2][3] == 1 and len(want[2][2]) == 5 and want[3][3] == 4 and len(want[3][2]) == 5
        if max_steps == 0 and E > 1:
            assert want[1][3] == 2 and len(want[1][2]) == limit == Tcap                # exactly Tcap
        if max_steps == 0 and E > 0:
            assert data[2][1:limit, 0].any() or data[3][1:limit, 0].any()              # the fast env finishes a later episode inside the recording's horizon
        for M in range(1, E + 1):
            longest = max(len(w[2]) for w in want[:M])
            for K in (1, 7, 64):
                for extra in (0, 1, 31):
                    if extra and M not in (1, E, (E + 1) // 2):
                        continue
                    steps = longest + extra                                            # (past Tcap the function writes nothing; the host loop never gets there)
                    finished, (o_tm, a_tm, r_tm, length, flags) = run_env_form(rec, data, E, M, D, W, Tcap, steps, K, maps, rng)
                    where = (E, M, max_steps, K, extra)
                    assert finished == M, where
                    assert length[:M].tolist() == [len(w[2]) for w in want[:M]] and flags[:M].tolist() == [w[3] for w in want[:M]], where
                    # the lane form on the same step stream: every slot of every array, the untouched ones and the guards included
                    lf, lo, la, lr, ll, lfl = run_recording(rec, data, E, M, D, W, Tcap, steps, maps, rng)
                    assert lf == finished
                    assert np.array_equal(o_tm[:-GUARD].view(np.uint32), lo.view(np.uint32)) and np.array_equal(a_tm[:-GUARD], la), where
                    assert np.array_equal(r_tm[:-GUARD].view(np.uint32), lr.view(np.uint32)) and np.array_equal(length[:M], ll) and np.array_equal(flags[:M], lfl), where
                    assert (o_tm[-GUARD:] == -7).all() and (a_tm[-GUARD:] == 0xABCD).all() and (r_tm[-GUARD:] == -7).all() and (length[M:] == -7).all() and (flags[M:] == 0xEE).all()
                    if extra or K != 7:
                        continue
                    # and the reference loop, through the host's reorder
                    obs = np.full((M, Tcap + 1, D), np.nan, np.float32); act = np.full((M, Tcap, W), 7, np.uint32); rw = np.full((M, Tcap), np.nan, np.float32)
                    p = lambda x: x.ctypes.data
                    rec.reorder(M, D, W, Tcap, p(length), p(o_tm), p(a_tm), p(r_tm), p(obs), p(act), p(rw))
                    for m in range(M):
                        o, a, r, _ = want[m]
                        L = len(r)
                        assert np.array_equal(obs[m, :L + 1].view(np.uint32), o.view(np.uint32)), (where, m)
                        assert np.array_equal(act[m, :L], a.reshape(L, W)) and np.array_equal(rw[m, :L].view(np.uint32), r.view(np.uint32)), (where, m)
                        assert not obs[m, L + 1:].any() and not act[m, L:].any() and not rw[m, L:].any()
            if M > 1:                                                                  # one step short of the longest: the open ones stay open, across a launch boundary too
                for K in (1, 7):
                    finished, (*_rest, length, flags) = run_env_form(rec, data, E, M, D, W, Tcap, longest - 1, K, maps, rng)
                    n_open = sum(len(w[2]) == longest for w in want[:M])
                    assert finished == M - n_open and (length[:M] == OPEN).sum() == n_open


# ---- options, info, the Python surface ---------------------------------------------------------------------------------------------------------------------------------
def test_request_words_default_to_zero_and_the_slots_are_the_headers(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    header = (ROOT / "include" / "dril_hip.h").read_text()
    slot = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))
    assert (slot("DRIL_EVAL_OPT_PERSISTENT"), slot("DRIL_TRAJ_OPT_PERSISTENT"), slot("DRIL_TRAJ_INFO_PATH")) == (capi.EVAL_OPT_PERSISTENT, capi.TRAJ_OPT_PERSISTENT, capi.TRAJ_INFO_PATH)
    assert capi.EVAL_OPT_PERSISTENT < 3 and capi.TRAJ_OPT_PERSISTENT < 5 and capi.TRAJ_INFO_PATH < 3
    assert "#define DRIL_ABI_VERSION 2u" in header and capi.ABI_VERSION == 2
    assert (C.sizeof(capi.DrilEvalOptions), C.sizeof(capi.DrilEvalInfo), C.sizeof(capi.DrilTrajOptions), C.sizeof(capi.DrilTrajInfo)) == (40, 32, 56, 32)
    eo, to = capi.DrilEvalOptions(), capi.DrilTrajOptions()
    for o, default in ((eo, lib.dril_eval_options_default), (to, lib.dril_traj_options_default)):
        C.memset(C.byref(o), 0xFF, C.sizeof(o))
        assert default(C.byref(o)) == capi.OK and not any(o.reserved)
    assert inspect.signature(pkg.evaluate_agent).parameters["persistent"].default is False
    assert inspect.signature(pkg.evaluate_agent).parameters["isolated"].default is False


class _Recorder:
    """a library whose two device verbs record the options they are given and report a path; everything else is the real library"""
    def __init__(self, capi):
        self.real, self.capi, self.eval_opts, self.traj_opts = capi.load_library(), capi, [], []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def dril_evaluate_agent_device(self, h, o, st, er, el, info):
        o, info = o._obj, info._obj
        self.eval_opts.append((o.n_eval_episodes, o.deterministic, o.poll_steps, o.force_step_granular, tuple(o.reserved)))
        info.path = 1 if o.reserved[self.capi.EVAL_OPT_PERSISTENT] else 0
        return self.capi.OK

    def dril_trajectory_capacity(self, h, o, cap):
        cap._obj.value = 3
        return self.capi.OK

    def dril_collect_trajectory_device(self, h, o, obs, act, rew, lengths, flags, info):
        o, info = o._obj, info._obj
        self.traj_opts.append((o.n_trajectories, o.max_steps, o.deterministic, o.poll_steps, o.final_original, tuple(o.reserved)))
        C.memset(lengths, 0, 4 * o.n_trajectories); C.memset(flags, 0, o.n_trajectories)
        info.reserved[self.capi.TRAJ_INFO_PATH] = 1 if o.reserved[self.capi.TRAJ_OPT_PERSISTENT] else 0
        return self.capi.OK


def test_python_keywords_reach_the_structs_and_the_path_comes_back(pkg):
    capi = pkg._capi
    h = object.__new__(pkg.Handle)                                                     # no device: the verbs below only fill structs and call the library
    h.lib, h._h, h.D, h.A, h.discrete = _Recorder(capi), None, 4, 2, True
    slot = lambda n, i: tuple(1 if j == i else 0 for j in range(n))
    assert h.evaluate_agent_device(7, False)[3]["path"] == 0
    assert h.evaluate_agent_device(7, False, persistent=True)[3]["path"] == 1
    assert h.evaluate_agent_device(7, False, None, 5, True, persistent=True)[3]["path"] == 1
    assert h.lib.eval_opts == [(7, 0, 0, 0, (0, 0, 0)), (7, 0, 0, 0, slot(3, capi.EVAL_OPT_PERSISTENT)), (7, 0, 5, 1, slot(3, capi.EVAL_OPT_PERSISTENT))]
    assert h.collect_trajectory_device(2)[3]["path"] == 0
    assert h.collect_trajectory_device(2, 3, False, None, 4, True, persistent=True)[3]["path"] == 1
    assert h.lib.traj_opts == [(2, 0, 1, 0, 0, (0,) * 5), (2, 3, 0, 4, 1, slot(5, capi.TRAJ_OPT_PERSISTENT))]
    with pytest.raises(TypeError):
        h.evaluate_agent_device(7, False, None, 0, False, True)                        # keyword-only: the positional interface is the one callers have
    for verb in (pkg.Handle.evaluate_agent_device, pkg.Handle.collect_trajectory_device, pkg.collect_trajectory):
        assert "persistent" in verb.__doc__


# ---- the shim -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_shim_takes_the_keyword_passes_the_check_and_a_wrong_arity_is_caught(tmp_path):
    tool = ROOT / "tools" / "check_shim.py"
    shim_dir = ROOT / "dril.jl_amd" / "julia"
    r = subprocess.run([sys.executable, str(tool)], capture_output=True, text=True)
    assert r.returncode == 0 and "check_shim: ok" in r.stdout, r.stdout[-2000:]
    text = (shim_dir / "DRiLHIP_extras.jl").read_text()
    ev = text[text.index("function DRiL.evaluate_agent(agent, env::DeviceParallelEnv"):text.index("# ---- collect_trajectory")]
    tr = text[text.index("function DRiL.collect_trajectory(agent, env::DeviceParallelEnv"):text.index("# ---- deployment policies")]
    assert "persistent::Bool = false" in ev and "(Int32(persistent), Int32(0), Int32(0))" in ev
    assert "persistent::Bool = false" in tr and "(Int32(persistent), Int32(0), Int32(0), Int32(0), Int32(0))" in tr
    for f in shim_dir.glob("DRiLHIP*.jl"): shutil.copy(f, tmp_path / f.name)
    extras = tmp_path / "DRiLHIP_extras.jl"
    good = "ccall((:dril_evaluate_agent_device, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilEvalOptions}, Ref{DrilEvalStats}, Ptr{Float32}, Ptr{Int32}, Ptr{DrilEvalInfo})"
    assert good in text
    extras.write_text(text.replace(good, good.replace("Ref{DrilEvalStats}, ", "")))
    r = subprocess.run([sys.executable, str(tool), "--shim", str(tmp_path / "DRiLHIP.jl")], capture_output=True, text=True)
    assert r.returncode == 1 and "ccall dril_evaluate_agent_device" in r.stdout and "5 argument types" in r.stdout, r.stdout[-1500:]
    extras.write_text(text.replace("    reserved::NTuple{5, Int32}\n", ""))           # a mirror struct that lost the words the request travels in
    r = subprocess.run([sys.executable, str(tool), "--shim", str(tmp_path / "DRiLHIP.jl")], capture_output=True, text=True)
    assert r.returncode == 1 and "DrilTrajOptions" in r.stdout, r.stdout[-1500:]
