"""CPU: evaluate_agent of a PPO handle on the device (dril_evaluate_agent_device, docs/evaluation.md), without a GPU.

  * the two structs and prototypes: ctypes layout == a C compile of include/dril_hip.h, the defaults, null / bad arguments before any HIP call;
  * the per-env accounting the kernels run (dril.jl_amd/csrc/dril_eval_account.h) and the host's reduction (dril_sac_eval.h), built with g++ and driven with
    recorded step arrays, against a NumPy restatement of the reference's loop (evaluation.jl:92-124);
  * the Julia shim's new ccall passes the static check, and the check catches a wrong arity of it."""
import ctypes as C
import math
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
EVENT = np.dtype([("step", np.int32), ("env", np.int32), ("ret", np.float32), ("len", np.int32)])


# ---- structs and prototypes --------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_a_c_compile_of_the_header(pkg, tmp_path):
    capi = pkg._capi
    fields = {"dril_eval_options": ("n_eval_episodes", "deterministic", "seed", "has_seed", "poll_steps", "force_step_granular", "reserved"),
              "dril_eval_info": ("path", "launches", "steps_enqueued", "events", "reserved")}
    body = "".join(f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {f}));' for f in fs) + 'printf("\\n");' for s, fs in fields.items())
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_hip.h"\nint main(){' + body + "return 0;}")
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for (s, fs), line, K in zip(fields.items(), lines, (capi.DrilEvalOptions, capi.DrilEvalInfo)):
        want = [int(x) for x in line.split()]
        assert [C.sizeof(K)] + [getattr(K, f).offset for f in fs] == want, s
        assert tuple(n for n, _ in K._fields_) == fs
    # the ABI numbers this change must not move
    header = (ROOT / "include" / "dril_hip.h").read_text()
    assert "#define DRIL_ABI_VERSION 2u" in header and capi.ABI_VERSION == 2
    assert C.sizeof(capi.DrilEvalStats) == 40


def test_defaults_exports_and_python_surface(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    for name in ("dril_eval_options_default", "dril_evaluate_agent_device"):
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    P = C.c_void_p
    assert lib.dril_evaluate_agent_device.argtypes == [P, C.POINTER(capi.DrilEvalOptions), C.POINTER(capi.DrilEvalStats), P, P, C.POINTER(capi.DrilEvalInfo)]
    o = capi.DrilEvalOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    assert lib.dril_eval_options_default(C.byref(o)) == capi.OK
    assert (o.n_eval_episodes, o.deterministic, o.has_seed, o.seed, o.poll_steps, o.force_step_granular, tuple(o.reserved)) == (10, 1, 0, 0, 0, 0, (0, 0, 0))   # evaluation.jl:57-58
    assert lib.dril_eval_options_default(None) == capi.ERR_INVALID_ARG
    assert callable(pkg.Handle.evaluate_agent_device)
    import inspect
    assert inspect.signature(pkg.evaluate_agent).parameters["isolated"].default is False
    sig = inspect.signature(pkg.Handle.evaluate_agent_device).parameters
    assert [(k, sig[k].default) for k in list(sig)[1:]] == [("n_eval_episodes", 10), ("deterministic", True), ("seed", None), ("poll_steps", 0), ("force_step_granular", False)]


def test_null_handle_returns_before_any_gpu_work(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    o, st, info = capi.DrilEvalOptions(), capi.DrilEvalStats(), capi.DrilEvalInfo()
    lib.dril_eval_options_default(C.byref(o))
    st.n_steps = 77; info.path = 5
    assert lib.dril_evaluate_agent_device(None, C.byref(o), C.byref(st), None, None, C.byref(info)) == capi.ERR_NOT_INITIALISED
    assert lib.dril_evaluate_agent_device(None, None, None, None, None, None) == capi.ERR_NOT_INITIALISED
    assert (st.n_steps, info.path) == (77, 5)
    assert b"null handle" in lib.dril_last_error(None)


# ---- the accounting against the reference loop --------------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <vector>
#include "dril_eval_account.h"
#include "dril_sac_eval.h"
extern "C" {
// rew / done / order: [T][E] (order: the sequence in which the envs of a step take their turn at the counter).  Runs `steps` env steps; returns the counter.
// in_registers = K > 0: the sums live in locals for K steps at a time and travel through cur_ret / cur_len in between (the persistent kernel); 0: in the arrays
long long drive(int E, int steps, const float* rew, const unsigned char* done, const int* order, long long cap, dril::SacEvalEvent* events, int in_registers) {
    std::vector<float> cur_ret(E, 0.f); std::vector<int32_t> cur_len(E, 0);
    unsigned int counter = 0;
    const dril::EvalAcct a{E, cur_ret.data(), cur_len.data(), &counter, events, (unsigned int)cap};
    if (!in_registers) {
        for (int t = 0; t < steps; ++t) for (int i = 0; i < E; ++i) { const int e = order[(size_t)t * E + i]; dril::eval_account_env(a, t + 1, e, rew[(size_t)t * E + e], done[(size_t)t * E + e] != 0); }
        return counter;
    }
    for (int t0 = 0; t0 < steps; t0 += in_registers)
        for (int i = 0; i < E; ++i) {                      // a launch: every env walks its K steps with the sums in registers (envs interleave only at the counter)
            const int e = order[(size_t)t0 * E + i];
            float r = cur_ret[e]; int32_t l = cur_len[e];
            for (int t = t0; t < steps && t < t0 + in_registers; ++t) dril::eval_account(a, t + 1, e, rew[(size_t)t * E + e], done[(size_t)t * E + e] != 0, r, l);
            cur_ret[e] = r; cur_len[e] = l;
        }
    return counter;
}
int reduce(dril::SacEvalEvent* ev, long long n_events, int n_eval, double* out6, float* er, int* el) {
    dril::SacEvalSummary s{};
    const int n = dril::sac_eval_reduce(ev, n_events, n_eval, &s, er, el);
    out6[0] = s.mean_reward; out6[1] = s.std_reward; out6[2] = s.mean_length; out6[3] = s.std_length; out6[4] = s.n_episodes; out6[5] = s.n_steps;
    return n;
}
long long capacity(long long n_eval, long long n_envs, long long launch_steps) { return dril::eval_event_capacity(n_eval, n_envs, launch_steps); }
}
'''


@pytest.fixture(scope="module")
def acct(tmp_path_factory):
    d = tmp_path_factory.mktemp("eval_account")
    src = d / "drive.cpp"; src.write_text(_DRIVER)
    so = d / "drive.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / "dril.jl_amd" / "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.drive.restype = C.c_longlong
    lib.drive.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int]
    lib.reduce.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.capacity.restype = C.c_longlong; lib.capacity.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong]
    return lib


def reference_loop(rew, done, n_eval):
    """evaluation.jl:92-124: current_rewards .+= rewards (Float32), current_lengths .+= 1, then the envs in index order until n_eval episodes are in"""
    T, E = rew.shape
    cur_r, cur_l = np.zeros(E, np.float32), np.zeros(E, np.int64)
    er, el = [], []
    for t in range(T):
        cur_r += rew[t]; cur_l += 1
        for e in range(E):
            if done[t, e] and len(er) < n_eval:
                er.append(cur_r[e]); el.append(cur_l[e]); cur_r[e] = 0; cur_l[e] = 0
        if len(er) >= n_eval:
            return np.asarray(er, np.float32), np.asarray(el, np.int32), t + 1
    raise AssertionError("the recorded arrays hold fewer episodes than asked for")


GUARD = 5


def run_device_form(acct, rew, done, order, n_eval, steps, in_registers):
    E = rew.shape[1]
    cap = acct.capacity(n_eval, E, max(in_registers, 1))                            # one launch per env step: n + E; a launch of K steps: n + E K
    assert cap == n_eval + E * max(in_registers, 1) and acct.capacity(n_eval, E, 0) == n_eval + E
    events = np.zeros(cap + GUARD, EVENT); events["step"] = -7                      # slots past the capacity must stay as they are
    counter = acct.drive(E, steps, rew.ctypes.data, done.ctypes.data, order.ctypes.data, cap, events.ctypes.data, in_registers)
    assert (events["step"][cap:] == -7).all(), "an event was written past the list's capacity"
    assert counter == int(done[:steps].sum()), "every finished episode bumps the counter, stored or not"
    used = events[:min(counter, cap)].copy()
    out, er, el = np.zeros(6), np.full(n_eval, np.nan, np.float32), np.full(n_eval, -1, np.int32)
    n = acct.reduce(used.ctypes.data, len(used), n_eval, out.ctypes.data, er.ctypes.data, el.ctypes.data)
    return n, out, er, el, counter


@pytest.mark.parametrize("E", [1, 2, 7, 31, 32, 33, 40])
def test_accounting_and_reduction_follow_the_reference_loop(acct, E):
    rng = np.random.default_rng(100 + E)
    limit = 12                                                                        # a time limit: every env finishes at least once per `limit` steps
    for n_eval in sorted({1, 2, max(1, E - 1), E, E + 1, (5 * E + 1) // 2, 3 * E}):
        T = ((n_eval + E - 1) // E + 1) * limit + 31
        rew = rng.normal(0, 3, (T, E)).astype(np.float32)
        done = rng.random((T, E)) < 0.12
        done[limit - 1::limit] = True
        if E > 2:
            done[3] = True; done[4] = False                                           # a step in which every env finishes, one in which none does
        done = np.ascontiguousarray(done, np.uint8)
        order = np.stack([rng.permutation(E) for _ in range(T)]).astype(np.int32)     # the atomics' order inside a step: arbitrary
        want_r, want_l, want_steps = reference_loop(rew, done, n_eval)
        assert len(want_r) == n_eval and want_steps + 31 <= T
        for extra in (0, 1, 31):                                                      # steps enqueued past the completing one: poll intervals
            for regs in (0, 1, 7, 64):                                                # the step-granular form; the persistent form at three launch lengths
                n, out, er, el, counter = run_device_form(acct, rew, done, order, n_eval, want_steps + extra, regs)
                assert n == n_eval and counter >= n_eval
                assert np.array_equal(er, want_r), (E, n_eval, extra, regs)
                assert np.array_equal(el, want_l), (E, n_eval, extra, regs)
                assert int(out[4]) == n_eval and int(out[5]) == want_steps
                assert out[0] == float(np.mean(want_r.astype(np.float64))) or out[0] == pytest.approx(float(np.mean(want_r.astype(np.float64))), rel=1e-14)
                if n_eval == 1:
                    assert math.isnan(out[1]) and math.isnan(out[3])                  # Julia's std of one element
                else:
                    assert out[1] == pytest.approx(float(np.std(want_r.astype(np.float64), ddof=1)), rel=1e-12)
                    assert out[3] == pytest.approx(float(np.std(want_l.astype(np.float64), ddof=1)), rel=1e-12)
                assert out[2] == pytest.approx(float(np.mean(want_l)), rel=1e-14)


def test_a_list_longer_than_its_capacity_only_moves_the_counter(acct):
    rng = np.random.default_rng(7)
    E, T, n_eval = 5, 60, 3
    rew = rng.normal(0, 1, (T, E)).astype(np.float32)
    done = np.ones((T, E), np.uint8)                                                  # 300 episodes into a list of 8 slots
    order = np.stack([rng.permutation(E) for _ in range(T)]).astype(np.int32)
    for regs in (0, 16):
        n, out, er, el, counter = run_device_form(acct, rew, done, order, n_eval, T, regs)
        assert counter == E * T > n_eval + E and n == n_eval
        assert np.array_equal(er, rew[0, :n_eval]) and (el == 1).all() and int(out[5]) == 1


# ---- the shim -----------------------------------------------------------------------------------------------------------------------------------------
def test_shim_check_passes_and_catches_a_wrong_arity_of_the_new_ccall(tmp_path):
    tool = ROOT / "tools" / "check_shim.py"
    shim_dir = ROOT / "dril.jl_amd" / "julia"
    r = subprocess.run([sys.executable, str(tool)], capture_output=True, text=True)
    assert r.returncode == 0 and "check_shim: ok" in r.stdout, r.stdout[-2000:]
    for f in shim_dir.glob("DRiLHIP*.jl"): shutil.copy(f, tmp_path / f.name)
    extras = tmp_path / "DRiLHIP_extras.jl"
    good = "ccall((:dril_evaluate_agent_device, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilEvalOptions}, Ref{DrilEvalStats}, Ptr{Float32}, Ptr{Int32}, Ptr{DrilEvalInfo})"
    text = extras.read_text()
    assert good in text and "isolated::Bool = false" in text
    extras.write_text(text.replace(good, good.replace(", Ptr{DrilEvalInfo})", ")")))
    r = subprocess.run([sys.executable, str(tool), "--shim", str(tmp_path / "DRiLHIP.jl")], capture_output=True, text=True)
    assert r.returncode == 1 and "ccall dril_evaluate_agent_device" in r.stdout and "5 argument types" in r.stdout, r.stdout[-1500:]
    extras.write_text(text.replace("    poll_steps::Int32\n", ""))                   # a mirror struct that lost a field
    r = subprocess.run([sys.executable, str(tool), "--shim", str(tmp_path / "DRiLHIP.jl")], capture_output=True, text=True)
    assert r.returncode == 1 and "DrilEvalOptions fields" in r.stdout, r.stdout[-1500:]
