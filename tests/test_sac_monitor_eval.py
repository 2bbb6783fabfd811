"""CPU: MonitorWrapperEnv statistics and evaluate_agent of a SAC handle, without a GPU.

  * the library exports the three new entry points; include/dril_sac.h, dril.jl_amd/_capi.py and the Julia shim agree on them (arity and widths);
  * a null handle and bad arguments return their status before any HIP call;
  * the host arithmetic of the device-resident evaluation (dril.jl_amd/csrc/dril_sac_eval.h, the lines dril_sac_eval.hip compiles) built with g++ against a
    restatement of the reference's loop (evaluation.jl:100-124)."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW = {
    "dril_sac_monitor_enable": ("dril_sac_handle* h, int32_t window", "(Ptr{Cvoid}, Int32)"),
    "dril_sac_monitor_get_stats": ("dril_sac_handle* h, float* ep_rew_mean, float* ep_len_mean, int32_t* n_episodes", "(Ptr{Cvoid}, Ref{Float32}, Ref{Float32}, Ref{Int32})"),
    "dril_sac_evaluate_agent": ("dril_sac_handle* h, int32_t n_eval_episodes, int32_t deterministic, uint64_t seed, dril_eval_stats* out, float* episode_rewards, int32_t* episode_lengths",
                                "(Ptr{Cvoid}, Int32, Int32, UInt64, Ref{DrilEvalStats}, Ptr{Float32}, Ptr{Int32})"),
}


def test_the_three_entry_points_are_exported_and_header_capi_and_shim_agree(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    header = re.sub(r"\s+", " ", (ROOT / "include" / "dril_sac.h").read_text())
    shim = (ROOT / "dril.jl_amd" / "julia" / "DRiLHIP_sac.jl").read_text()
    for name, (c_args, jl_args) in NEW.items():
        assert hasattr(lib, name), f"libdril_hip.so does not export {name}"
        assert f"int32_t {name}({c_args});" in header, f"include/dril_sac.h does not declare {name} with these arguments"
        assert name in capi.EXPORTED_SYMBOLS, f"_capi.py does not type {name}"
        assert f"ccall((:{name}, LIB[]), Int32, {jl_args}," in shim, f"the Julia shim has no ccall of {name} with these types"
    P = C.c_void_p
    assert lib.dril_sac_monitor_enable.argtypes == [P, C.c_int32]
    assert lib.dril_sac_monitor_get_stats.argtypes == [P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    assert lib.dril_sac_evaluate_agent.argtypes == [P, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(capi.DrilEvalStats), P, P]
    # exported = declared, and the ABI numbers this change must not move
    nm = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "dril.jl_amd" / "csrc" / "libdril_hip.so")], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("dril_sac_")}
    declared = set(re.findall(r"\b(dril_sac_\w+)\s*\(", (ROOT / "include" / "dril_sac.h").read_text()))
    assert exported == declared and set(NEW) <= exported, (declared - exported, exported - declared)
    assert capi.SAC_ABI_VERSION == 1 and "#define DRIL_SAC_ABI_VERSION 1u" in (ROOT / "include" / "dril_sac.h").read_text()
    for w in ("monitor_enable", "monitor_stats", "evaluate_agent"):
        assert callable(getattr(pkg.SacHandle, w))
    assert callable(pkg.sac_evaluate_agent)
    r = subprocess.run(["python", str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]


def test_null_handle_and_bad_arguments_return_before_any_gpu_work(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    r, l, n = C.c_float(5.0), C.c_float(6.0), C.c_int32(7)
    st = capi.DrilEvalStats()
    assert lib.dril_sac_monitor_enable(None, 100) == capi.ERR_NOT_INITIALISED
    assert lib.dril_sac_monitor_get_stats(None, C.byref(r), C.byref(l), C.byref(n)) == capi.ERR_NOT_INITIALISED
    assert (r.value, l.value, n.value) == (5.0, 6.0, 7)
    assert lib.dril_sac_evaluate_agent(None, 10, 1, 0, C.byref(st), None, None) == capi.ERR_NOT_INITIALISED
    assert b"null handle" in lib.dril_sac_last_error(None)


# ---- the event-list arithmetic, on the host ---------------------------------------------------------------------------------------------------------------------
_SHIM = r'''
#include "dril_sac_eval.h"
extern "C" {
int reduce(dril::SacEvalEvent* ev, long long n_events, int n_eval, double* out6, float* er, int* el) {
    dril::SacEvalSummary s{};
    const int n = dril::sac_eval_reduce(ev, n_events, n_eval, &s, er, el);
    out6[0] = s.mean_reward; out6[1] = s.std_reward; out6[2] = s.mean_length; out6[3] = s.std_length; out6[4] = s.n_episodes; out6[5] = s.n_steps;
    return n;
}
long long capacity(long long n_eval, long long n_envs) { return dril::sac_eval_event_capacity(n_eval, n_envs); }
int event_bytes() { return (int)sizeof(dril::SacEvalEvent); }
}
'''
EVENT = np.dtype([("step", np.int32), ("env", np.int32), ("ret", np.float32), ("len", np.int32)])


@pytest.fixture(scope="module")
def evlib(tmp_path_factory):
    d = tmp_path_factory.mktemp("sac_eval")
    src = d / "eval.cpp"; src.write_text(_SHIM)
    so = d / "eval.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / "dril.jl_amd" / "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.reduce.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.capacity.restype = C.c_longlong; lib.capacity.argtypes = [C.c_longlong, C.c_longlong]
    return lib


def reference_loop(done, ret, ln, n_eval):
    """evaluation.jl:92-124 over per-step arrays [T][E]: after each step the envs in index order, until n_eval episodes are in"""
    er, el, steps = [], [], 0
    for t in range(done.shape[0]):
        if len(er) >= n_eval:
            break
        steps = t + 1
        for e in range(done.shape[1]):
            if len(er) < n_eval and done[t, e]:
                er.append(ret[t, e]); el.append(ln[t, e])
    er, el = np.asarray(er, np.float64), np.asarray(el, np.float64)
    sd = lambda x: float(np.std(x, ddof=1)) if len(x) > 1 else float("nan")
    return er, el, steps, (float(er.mean()), sd(er), float(el.mean()), sd(el))


def device_list(rng, done, ret, ln, n_eval, steps_enqueued):
    """what the kernels leave behind: events of a step in arbitrary order, steps in order, slots past n_eval + E dropped; the host may have enqueued more steps"""
    E = done.shape[1]
    ev = []
    for t in range(steps_enqueued):
        es = np.nonzero(done[t])[0]
        rng.shuffle(es)
        ev += [(t + 1, e, ret[t, e], ln[t, e]) for e in es]
    return np.array(ev[:n_eval + E], EVENT), len(ev)


def run_reduce(evlib, events, n_eval):
    out, er, el = np.zeros(6), np.full(n_eval, np.nan, np.float32), np.full(n_eval, -1, np.int32)
    n = evlib.reduce(events.ctypes.data, len(events), n_eval, out.ctypes.data, er.ctypes.data, el.ctypes.data)
    return n, out, er, el


def test_event_reduction_follows_the_reference_loop(evlib):
    assert evlib.event_bytes() == EVENT.itemsize == 16 and evlib.capacity(10, 64) == 74
    rng = np.random.default_rng(0)
    E, T = 9, 40
    done = rng.random((T, E)) < 0.15
    done[3] = True                                                    # a step in which every env finishes
    done[4] = False
    ret = rng.normal(-100, 30, (T, E)).astype(np.float32)
    ret[7, 2] = ret[7, 5]                                             # ties in the return change nothing about the order
    ln = rng.integers(1, 200, (T, E)).astype(np.int32)
    total = int(done.sum())
    for n_eval in (1, 2, E - 1, E, E + 1, 3 * E + 2, total):          # one episode; fewer, as many and more than one step's worth; every event there is
        want_r, want_l, want_steps, want = reference_loop(done, ret, ln, n_eval)
        assert len(want_r) == n_eval
        for extra in (0, 1, 7, T - want_steps):                       # steps enqueued past the one that completed the list: poll intervals
            events, counted = device_list(rng, done, ret, ln, n_eval, min(T, want_steps + extra))
            assert counted >= n_eval
            n, out, er, el = run_reduce(evlib, events, n_eval)
            assert n == n_eval and np.array_equal(er, want_r.astype(np.float32)) and np.array_equal(el, want_l.astype(np.int32))
            assert int(out[4]) == n_eval and int(out[5]) == want_steps
            assert out[0] == pytest.approx(want[0], rel=1e-12) and out[2] == pytest.approx(want[2], rel=1e-12)
            if n_eval == 1:
                assert math.isnan(out[1]) and math.isnan(out[3])      # Julia's std of one element
            else:
                assert out[1] == pytest.approx(want[1], rel=1e-12) and out[3] == pytest.approx(want[3], rel=1e-12)
    # fewer events than asked for (the caller reports that): what there is, in order; no events at all
    events, _ = device_list(rng, done, ret, ln, total, 5)
    n, out, er, el = run_reduce(evlib, events, total)
    assert n == len(events) < total and int(out[5]) == int(events["step"].max()) and np.isnan(er[n:]).all()
    n, out, _, _ = run_reduce(evlib, np.zeros(0, EVENT), 3)
    assert n == 0 and int(out[4]) == 0 and int(out[5]) == 0
