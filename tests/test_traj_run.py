"""CPU: the recording setup both handles' collect_trajectory verbs share (dril.jl_amd/csrc/dril_traj_run.h), without a GPU.  Its two pure functions, built with g++:

  * traj_layout: the regions of the private blob are disjoint, 256-aligned and inside the total, and the five regions of the recording hold the terms of traj_bytes;
  * traj_bounds_table: the values of the table and which of the six TrajMaps pointers are null, for a Box handle with ClampAdapter (unscaled, scaled), a Discrete
    handle and a handle without ClampAdapter (the SAC handle)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
REGIONS = ("obs", "act", "rew", "len", "flg", "st", "sc", "ep", "gs", "srew", "sterm", "strunc", "stobs", "sobs", "tab")

_DRIVER = r'''
#include "dril_traj_run.h"
using namespace dril;
extern "C" {
// out: (at, bytes) of the 15 regions in declaration order, then the total
void layout(long long M, long long D, long long W, long long S, long long Tcap, long long* out) {
    const TrajLayout L = traj_layout(M, D, W, S, Tcap);
    const TrajRegion r[15] = {L.obs, L.act, L.rew, L.len, L.flg, L.st, L.sc, L.ep, L.gs, L.srew, L.sterm, L.strunc, L.stobs, L.sobs, L.tab};
    for (int i = 0; i < 15; ++i) { out[2 * i] = (long long)r[i].at; out[2 * i + 1] = (long long)r[i].bytes; }
    out[30] = (long long)L.total;
}
long long table_floats(long long D, long long W) { return (long long)traj_table_floats(D, W); }
long long bytes(long long M, long long Tcap, long long D, long long W) { return traj_bytes(M, Tcap, D, W); }   // what the 1 GiB refusal (traj_size_error) is stated in
// boxes: six host arrays or null; ptr_at: where each of the six TrajMaps pointers points, in floats from the table's device address (-1: null); flags: discrete, final_original
void table(int D, int W, const float* obs_low, const float* obs_high, const float* act_low, const float* act_high, const float* clamp_low, const float* clamp_high,
           int discrete, int final_original, float* tab, long long* ptr_at, int* flags) {
    static float dev[1];                                       // stands for the device address: never read
    const TrajMaps x = traj_bounds_table(D, W, TrajBoxes{obs_low, obs_high, act_low, act_high, clamp_low, clamp_high, discrete != 0}, final_original != 0, tab, dev);
    const float* p[6] = {x.obs_low, x.obs_high, x.clamp_low, x.clamp_high, x.act_low, x.act_high};
    for (int i = 0; i < 6; ++i) ptr_at[i] = p[i] ? (long long)(p[i] - dev) : -1;
    flags[0] = x.discrete; flags[1] = x.final_original;
}
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("traj_run")
    src = d / "drive.cpp"; src.write_text(_DRIVER)
    so = d / "drive.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / "dril.jl_amd" / "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.layout.argtypes = [C.c_longlong] * 5 + [C.c_void_p]
    lib.table_floats.restype = C.c_longlong; lib.table_floats.argtypes = [C.c_longlong] * 2
    lib.bytes.restype = C.c_longlong; lib.bytes.argtypes = [C.c_longlong] * 4
    lib.table.argtypes = [C.c_int] * 2 + [C.c_void_p] * 6 + [C.c_int] * 2 + [C.c_void_p] * 3
    return lib


@pytest.mark.parametrize("M,D,W,S,Tcap", [(1, 1, 1, 1, 1), (3, 5, 2, 4, 7)])
def test_layout_regions_are_disjoint_aligned_and_hold_the_recording(run, M, D, W, S, Tcap):
    out = np.zeros(31, np.int64)
    run.layout(M, D, W, S, Tcap, out.ctypes.data_as(C.c_void_p))
    at, nbytes, total = out[0:30:2], out[1:30:2], int(out[30])
    assert (at % 256 == 0).all() and (nbytes > 0).all() and (at + nbytes <= total).all() and at.min() == 0
    order = np.argsort(at)
    assert (at[order][1:] >= (at + nbytes)[order][:-1]).all()                      # disjoint: every region ends before the next one starts
    # observations | actions | rewards | lengths | end flags: the terms of traj_bytes (dril_traj_record.h), which the caller's 1 GiB bound is stated in.  The
    # library's own traj_bytes is the sum of the terms, so the five regions hold at least what the bound counts
    terms = (4 * M * (Tcap + 1) * D, 4 * M * Tcap * W, 4 * M * Tcap, 4 * M, M)
    assert all(int(nbytes[i]) >= t for i, t in enumerate(terms))
    assert run.bytes(M, Tcap, D, W) == sum(terms) <= int(nbytes[:5].sum())
    # the rest: the shadow envs' arrays, what their step and observe write, and the table
    want = dict(st=4 * M * S, sc=4 * M, ep=4 * M, gs=4 * M, srew=4 * M, sterm=M, strunc=M, stobs=4 * M * D, sobs=4 * M * D, tab=4 * run.table_floats(D, W))
    assert {k: int(nbytes[REGIONS.index(k)]) for k in want} == want


D, W = 3, 2
OBS = (np.array([-1.0, -2.0, -8.0], np.float32), np.array([1.0, 2.0, 8.0], np.float32))
ACT = (np.array([-2.0, -0.5], np.float32), np.array([2.0, 0.25], np.float32))
UNIT = (np.full(W, -1.0, np.float32), np.full(W, 1.0, np.float32))
ZERO = (np.zeros(W, np.float32), np.zeros(W, np.float32))
# boxes (obs, act, clamp; None: absent), discrete -> which pointers are set (obs, clamp, act) and the table's columns obs_low | obs_high | clamp_low | clamp_high | act_low | act_high
CASES = {
    "box_unscaled": ((None, None, ACT), 0, (False, True, False), (0, 0, ACT[0], ACT[1], 0, 0)),         # ClampAdapter on the env's own Box
    "box_scaled": ((OBS, ACT, UNIT), 0, (True, True, True), (OBS[0], OBS[1], UNIT[0], UNIT[1], ACT[0], ACT[1])),   # ClampAdapter on Box(-1, 1), then unscale!
    "discrete_scaled": ((OBS, None, ZERO), 1, (True, False, False), (OBS[0], OBS[1], 0, 0, 0, 0)),     # a Discrete space has neither clamp nor action map
    "no_clamp_scaled": ((OBS, ACT, None), 0, (True, False, True), (OBS[0], OBS[1], 0, 0, ACT[0], ACT[1])),   # the SAC handle: TanhScaleAdapter, no ClampAdapter
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("final_original", [0, 1])
def test_bounds_table_values_and_null_pointers(run, case, final_original):
    boxes, discrete, (has_obs, has_clamp, has_act), columns = CASES[case]
    arrays = [a for pair in boxes for a in (pair if pair is not None else (None, None))]
    n = run.table_floats(D, W)
    assert n == 2 * D + 4 * W
    tab, ptr_at, flags = np.full(n, np.nan, np.float32), np.zeros(6, np.int64), np.zeros(2, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    run.table(D, W, *[p(a) for a in arrays], discrete, final_original, p(tab), p(ptr_at), p(flags))
    starts = (0, D, 2 * D, 2 * D + W, 2 * D + 2 * W, 2 * D + 3 * W)                  # ONE layout for both handles
    set_ = (has_obs, has_obs, has_clamp, has_clamp, has_act, has_act)
    assert ptr_at.tolist() == [s if on else -1 for s, on in zip(starts, set_)]
    widths = (D, D, W, W, W, W)
    want = np.concatenate([np.broadcast_to(np.float32(c), (w,)) for c, w in zip(columns, widths)])
    assert np.array_equal(tab, want)                                                # absent columns are zero, not left over
    assert flags.tolist() == [discrete, final_original]
