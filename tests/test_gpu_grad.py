"""GPU: the five PPO gradient paths (ppo_grad_kernel, ppo_grad_pair_kernel, ppo_grad_wide_kernel, ppo_grad_wide_split_kernel, generic_ppo_grad) through
dril_ppo_loss_grad, EVERY ELEMENT of the gradient, the loss and the statistics against the float64 reference of tests/grad_cases.py: one test per row of its table
(kernel, env kind, hidden, grid switch), each running the row's batch sizes and input families — random, one-sample indicators, decisions at the edges of both clips,
edges — twice on the same handle (bit-identical) and through the assertion functions that tests/test_grad_cases.py holds against the CPU oracle and thirteen defects.
The kernel that ran and its grid (G, Gc) are asserted through grad_kernel_info() on every call.  A negative control runs two rows on libdril_hip_droplo.so (the `lo` products of the
operand split dropped): the per-element bound of dW2 must be broken there."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import grad_cases as gc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CONTROL_ROWS = ("pair.k0", "wsplit.k1.h128")


def _check_grid(row, case, grid):
    """the grid grad_kernel_info() reports for the step that just ran: the row's switch took effect"""
    G, Gc = grid
    tiles = (case.B + gc.K_TILE - 1) // gc.K_TILE
    assert G >= 1 and Gc >= 1
    if row.gmax:
        assert G == Gc == row.gmax, f"{case.name}: DRIL_GRAD_GMAX={row.gmax}, grid {grid}"
    if row.kernel == "ppo_grad_pair_kernel":
        assert G % 2 == 0 and Gc % 2 == 0, f"{case.name}: pairs come two to a workgroup, grid {grid}"
    if row.chip:                                                                     # the chip-filling division: unequal, and all of the chip's pair slots
        assert G != Gc and G + Gc > (tiles & ~1), f"{case.name}: {tiles} tiles did not reach the unequal division, grid {grid}"
        assert (G < Gc) if (row.permille or not row.dims[2]) else True, f"{case.name}: grid {grid}"
    elif row.kernel == "ppo_grad_pair_kernel" and not row.gmax:
        assert G == Gc == max(2, tiles & ~1), f"{case.name}: {tiles} tiles, grid {grid}"
    elif row.kernel == "ppo_grad_kernel" and not row.gmax:
        assert G == Gc == (tiles + 3) // 4, f"{case.name}: {tiles} tiles over workgroups of four waves, grid {grid}"


@pytest.mark.parametrize("row", gc.ROWS, ids=lambda r: r.name)
def test_gradient_kernel_row_vs_float64(pkg, row):
    run = gc.RowRunner(pkg, row)
    plain = gc.RowRunner(pkg, row, switches=False) if row.no_small else None
    worst = {}
    try:
        for case in gc.cases_of(row):
            ref = gc.ref_of(case)
            out0, out1 = run.run(case), run.run(case)
            gc.check_same(case, out0, out1)
            _check_grid(row, case, run.grid)
            res = gc.check(case, out0, ref)
            if plain is not None:                                                    # the in-kernel advantage moments against the two moments launches
                outp = plain.run(case)
                gc.check(case, outp, ref)
                if case.family != "equal_adv":                                       # (there T is that of a division by eps)
                    gc.check_moments_paths(case, outp[2], out0[2], ref)
            if case.family == "equal_adv":
                res = {k: v for k, v in res.items() if k.startswith("critic") or k in ("value_loss",)}
            for k, q in res.items():
                if q > worst.get(k, (0.0, ""))[0]:
                    worst[k] = (q, case.name)
    finally:
        run.close()
        if plain is not None:
            plain.close()
    print("[grad row]", json.dumps({"row": row.name, "kernel": row.kernel, "worst_error_over_bound": {k: round(v[0], 4) for k, v in worst.items()},
                                    "at": max(worst.values())[1]}))


def test_negative_control_dropped_lo_products_break_the_dW2_bound(pkg):
    """one pair-kernel row and one wide-split row on the build without the `lo` products (hi.hi alone, an 11-bit product), in a child process: some element of dW2 must
    leave its bound; the same random cases pass on the real library"""
    so = ROOT / "dril.jl_amd" / "csrc" / "libdril_hip_droplo.so"
    assert so.exists(), f"{so} missing: __graft_entry__.build() compiles it"
    env = dict(os.environ, DRIL_HIP_LIBRARY=str(so))
    for k in ("DRIL_GRAD_VARIANT", "DRIL_DEBUG", "DRIL_FORCE_GENERIC"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "grad_cases.py"), json.dumps(CONTROL_ROWS)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for name in CONTROL_ROWS:
        over = {k: res[name][k] / gc.CONSTANTS[k] for k in ("actor.W2", "critic.W2")}
        print("[negative control]", name, json.dumps(over))
        assert max(over.values()) > 1.0, (name, over)
        row = gc.ROW_BY_NAME[name]
        run = gc.RowRunner(pkg, row)
        try:
            for case in gc.cases_of(row):
                if case.family == "random":
                    gc.check(case, run.run(case), gc.ref_of(case))
        finally:
            run.close()
