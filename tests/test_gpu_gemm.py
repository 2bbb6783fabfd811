"""GPU (-m gpu): every kernel launch_gemm can pick, launch_gemm_pair and launch_gemm_multi, directly against a float64 reference (tests/gemm_cases.py: the table, the
reference, the tolerances; tests/test_gemm_plan.py: which kernel each row runs on).

One process (tests/gemm_check.hip) runs the whole table, each case twice, and writes the C / zout images; a second one, compiled with -DDRIL_DEBUG_DROP_LO (the
split kernel without its two `lo` products — the NEGATIVE CONTROL, never the library), runs the split cases.  Neither is retried; a non-zero exit fails every test
of the module.  The tests below only read files and compute the numpy reference.

exact mode  : bit-for-bit equality with float64 — operands are multiples of 1/8, every partial sum is exact in f32 and in the bf16 split.
normal mode : |C - C64| <= tolerance (gemm_cases.tolerance), zout within the pre-activation bound.
every run   : the two runs are bit-identical, no sentinel outside the logical C / zout is overwritten, no NaN inside it.
split cases : RMS distance from float64 at most twice that of the exact-f32 big kernel on the same operands (the criterion of tests/split_budget.py); the
              drop-lo build must break that on every split case.
"""
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gemm_cases as gc

pytestmark = pytest.mark.gpu
BY_NAME = {c.name: c for c in gc.CASES}
BY_NAME.update({gc.big_twin(c).name: gc.big_twin(c) for c in gc.SPLIT_CASES})


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    exe, exe_droplo = gc.build_driver(), gc.build_driver(droplo=True)
    root = tmp_path_factory.mktemp("gemm")
    data, out, out_droplo = root / "data", root / "out", root / "out_droplo"
    for d in (data, out, out_droplo):
        d.mkdir()
    runs = [(c, m) for c in gc.CASES for m in gc.MODES] + [(gc.big_twin(c), "normal") for c in gc.SPLIT_CASES]
    for c, m in runs:
        gc.write_images(c, m, data)
    gc.write_case_file(root / "cases.txt", runs)
    gc.write_case_file(root / "cases_droplo.txt", [(c, "normal") for c in gc.SPLIT_CASES])
    for e, cases, o in ((exe, "cases.txt", out), (exe_droplo, "cases_droplo.txt", out_droplo)):          # the second starts only after a clean first
        r = subprocess.run([str(e), str(root / cases), str(data), str(o)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    return {"out": out, "droplo": out_droplo}


@functools.lru_cache(maxsize=None)
def _evaluate(name, mode, out_dir):
    """every check of one run; -> {contraction index: (worst error / tolerance, worst zout error / bound, activation spread)}, RMS error of contraction 0"""
    case, res = BY_NAME[name], {}
    rms0 = None
    for i, con in enumerate(case.cons):
        ref, pre, bound = gc.reference(case, i, mode)
        aux = gc.operands(case, i, mode)[3]
        r_c = r_z = spread = 0.0
        for kind in ("C", "Z") if con.zout else ("C",):
            img0, img1 = (np.fromfile(Path(out_dir) / f"{gc.run_name(case, mode)}.{i}.{kind}{run}.bin", np.float32) for run in (0, 1))
            assert img0.size == con.layout()["totalC"]
            assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32)), f"{name}.{mode}[{i}] {kind}: the two runs differ"
            got, outside = gc.logical(con, img0)
            assert np.all(img0[outside] == gc.SENTINEL), f"{name}.{mode}[{i}] {kind}: wrote outside the logical output"
            assert not np.isnan(got).any(), f"{name}.{mode}[{i}] {kind}: NaN"
            want = ref if kind == "C" else pre
            err = np.abs(got.astype(np.float64) - want)
            if mode == "exact":
                assert np.array_equal(got.astype(np.float64), want), f"{name}.exact[{i}] {kind}: {np.count_nonzero(err)} elements differ, worst {err.max():.3e}"
            elif kind == "Z":
                r_z = float(np.max(err / bound))
            else:
                tol, spread = gc.tolerance(con, mode, pre, aux, bound)
                r_c = float(np.max(err / tol))
                if i == 0:
                    rms0 = gc.rms(err)
        res[i] = (r_c, r_z, spread)
    return res, rms0


@pytest.mark.parametrize("name", [c.name for c in gc.CASES])
def test_exact_operands_equal_float64_bit_for_bit(outputs, name):
    _evaluate(name, "exact", str(outputs["out"]))


@pytest.mark.parametrize("name", [c.name for c in gc.CASES] + [gc.big_twin(c).name for c in gc.SPLIT_CASES])
def test_normal_operands_within_the_error_bound(outputs, name):
    res, _ = _evaluate(name, "normal", str(outputs["out"]))
    for i, (r_c, r_z, spread) in res.items():
        print(f"[gemm] {name}[{i}] {BY_NAME[name].target}: error / tolerance {r_c:.3f}, zout error / bound {r_z:.3f}, activation spread {spread:.2e}")
    assert all(r_c <= 1.0 and r_z <= 1.0 for r_c, r_z, _ in res.values()), res


@pytest.mark.parametrize("name", [c.name for c in gc.SPLIT_CASES])
def test_split_is_within_twice_the_f32_kernels_distance_from_float64(outputs, name):
    _, split = _evaluate(name, "normal", str(outputs["out"]))
    _, f32 = _evaluate(name + "_f32", "normal", str(outputs["out"]))
    print(f"[gemm split] {name} {BY_NAME[name].target}: rms split {split:.3e}, f32 {f32:.3e}, ratio {split / f32:.2f}")
    assert split <= 2.0 * f32


@pytest.mark.parametrize("name", [c.name for c in gc.SPLIT_CASES])
def test_negative_control_four_products_break_the_criterion(outputs, name):
    """the same operands through the drop-lo build: a criterion that a 16-bit product passed would say nothing about 2^-24"""
    case = BY_NAME[name]
    con = case.cons[0]
    _, f32 = _evaluate(name + "_f32", "normal", str(outputs["out"]))
    ref, _, _ = gc.reference(case, 0, "normal")
    got, _ = gc.logical(con, np.fromfile(outputs["droplo"] / f"{gc.run_name(case, 'normal')}.0.C0.bin", np.float32))
    four = gc.rms(got.astype(np.float64) - ref)
    print(f"[gemm droplo] {name} {case.target}: rms four-product {four:.3e}, f32 {f32:.3e}, ratio {four / f32:.1f}")
    assert four > 2.0 * f32
