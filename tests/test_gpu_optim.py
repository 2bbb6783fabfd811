"""GPU (-m gpu): the four routes of the PPO optimiser tail (grad_reduce_kernel -> adam_kernel, ppo_finish_small_kernel, grad_norm_kernel -> adam_kernel, adam_kernel with
norm_from_flat) directly against a float64 reference of one step (tests/optim_cases.py: the table, the images, the reference, the bounds and the assertion
functions; tests/test_optim_cases.py holds those to their own terms without a GPU).

One process (tests/optim_check.hip: the library's own dril_kernels.hip and its four launchers) runs the whole table, every case twice from the same initial images,
and dumps every buffer a kernel may write after every step.  It is not retried; a non-zero exit fails every test of the module.  The tests only read files.

every case   : the two runs are bit-identical; the guard zones around flat, params, m, v, bt, norm_partials, norm_out and step_stats hold their sentinels; a buffer the
               route does not write (norm_partials on B and D) still holds them; bt's output slot is f32(bt_in) * f32(beta) bit for bit, its input slot unchanged
exact mode   : flat[0..P+8) equals the float64 sums bit for bit (the addressing: log_std behind the actor net, Gc != G, the statistics in the last 8 floats of a slab)
normal mode  : flat, norm, m, v, parameters and step_stats within the bounds of optim_cases (error / bound printed per case, the worst per route by the last test)
skipped step : kl stop or a non-finite norm: params, m, v unchanged bit for bit, bt carried over, stop_flag 1, nan_flag 1 only for the non-finite norm, step_stats[9..11]
launched with stop_flag set: nothing written anywhere, flat included
A and B      : bit-identical flat[0..P+8) for G, Gc <= 32 (the same order of additions);  C and D: norm_out within 4 u of each other, both within the same reference's bounds
"""
import functools
import subprocess

import numpy as np
import pytest

import optim_cases as oc

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in oc.CASES]
AB_KEYS = sorted({c.key for c in oc.CASES if c.route == "B"})
CD_KEYS = sorted({c.key for c in oc.CASES if c.route == "D"})


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    exe = oc.build_driver()
    root = tmp_path_factory.mktemp("optim")
    data, out = root / "data", root / "out"
    data.mkdir(), out.mkdir()
    for c in oc.CASES:
        oc.write_images(c, data)
    oc.write_case_file(root / "cases.txt", oc.CASES)
    r = subprocess.run([str(exe), str(root / "cases.txt"), str(data), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    return out


@functools.lru_cache(maxsize=None)
def _evaluate(name, out_dir):
    """every check of one case (optim_cases.check_case) -> worst error / bound per quantity, the decisions of its steps"""
    case = oc.BY_NAME[name]
    run0, run1 = (oc.read_run(case, f"{out_dir}/{name}.run{r}.bin") for r in (0, 1))
    return oc.check_case(case, run0, run1)


def _first_step(name, out_dir):
    return oc.read_run(oc.BY_NAME[name], f"{out_dir}/{name}.run0.bin")[0]


def test_driver_used_the_layouts_of_the_table(outputs):
    got = oc.read_layouts(outputs / "layouts.txt")
    assert set(got) == set(NAMES)
    for c in oc.CASES:
        lay = c.layout
        assert got[c.name] == (lay.P, lay.Pa, lay.Pc, lay.slab_a, lay.slab_c), (c.name, got[c.name])


@pytest.mark.parametrize("name", [c.name for c in oc.CASES if c.mode == "exact" and c.slabs])
def test_exact_operands_equal_float64_bit_for_bit(outputs, name):
    worst, _ = _evaluate(name, str(outputs))
    assert worst["flat"] == 0.0


@pytest.mark.parametrize("name", [c.name for c in oc.CASES if len(c.steps) == 1 and not c.steps[0].variant and not (c.mode == "exact" and c.slabs)])
def test_one_step_is_within_the_bounds(outputs, name):
    worst, _ = _evaluate(name, str(outputs))
    print(f"[optim] {name}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("name", [c.name for c in oc.CASES if len(c.steps) == 1 and c.steps[0].variant and c.steps[0].variant.startswith(("norm", "kl")) or ".clip_off" in c.name])
def test_decision_at_its_threshold(outputs, name):
    _, dec = _evaluate(name, str(outputs))
    what = name.split(".")[-1]
    assert dec[0]["clip"] == (what == "clip_above") and dec[0]["kl_stop"] == (what == "kl_above") and not dec[0]["bad"]
    st = _first_step(name, str(outputs))
    assert st["stop_flag"] == int(what == "kl_above") and st["nan_flag"] == 0


@pytest.mark.parametrize("name", [c.name for c in oc.CASES if len(c.steps) == 1 and c.steps[0].variant.startswith(("nan_", "inf_", "overflow", "single"))])
def test_poisoned_gradients_are_data(outputs, name):
    _, dec = _evaluate(name, str(outputs))
    st = _first_step(name, str(outputs))
    if name.endswith("single_1e19"):                                       # finite: clipped and applied
        assert dec[0]["clip"] and not dec[0]["bad"] and (st["nan_flag"], st["stop_flag"]) == (0, 0)
    else:
        assert dec[0]["bad"] and (st["nan_flag"], st["stop_flag"]) == (1, 1)


@pytest.mark.parametrize("name", [c.name for c in oc.CASES if len(c.steps) > 1])
def test_twelve_steps_across_clip_kl_stop_and_poison(outputs, name):
    worst, dec = _evaluate(name, str(outputs))
    print(f"[optim] {name}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert [i for i, d in enumerate(dec) if d.get("clip")] == [3] and [i for i, d in enumerate(dec) if d.get("kl_stop")] == [5]
    assert [i for i, d in enumerate(dec) if d.get("launched_stopped")] == [6] and [i for i, d in enumerate(dec) if d.get("bad")] == [9]


@pytest.mark.parametrize("key", AB_KEYS)
def test_routes_a_and_b_sum_in_the_same_order(outputs, key):
    a, b = oc.BY_NAME[f"A.{key}"], oc.BY_NAME[f"B.{key}"]
    assert a.G <= 32 and a.Gc <= 32 and (a.G, a.Gc) == (b.G, b.Gc)
    ra, rb = (oc.read_run(c, outputs / f"{c.name}.run0.bin") for c in (a, b))
    for i, (sa, sb) in enumerate(zip(ra, rb)):
        fa, fb = oc.logical(a, sa, "flat"), oc.logical(b, sb, "flat")
        assert fa.tobytes() == fb.tobytes(), f"{key} step {i}: {np.count_nonzero(fa.view(np.uint32) != fb.view(np.uint32))} elements of flat differ between A and B"


@pytest.mark.parametrize("key", CD_KEYS)
def test_routes_c_and_d_agree(outputs, key):
    c, d = oc.BY_NAME[f"C.{key}"], oc.BY_NAME[f"D.{key}"]
    _evaluate(c.name, str(outputs)), _evaluate(d.name, str(outputs))                # parameters, m, v: each within the bounds of the same float64 reference
    rc, rd = (oc.read_run(x, outputs / f"{x.name}.run0.bin") for x in (c, d))
    for i, (sc, sd) in enumerate(zip(rc, rd)):
        nc, nd = (float(oc.logical(c, s, "norm_out")[0]) for s in (sc, sd))
        if np.isfinite(nc) and nc != float(oc.SENTINEL):
            assert abs(nc - nd) <= 4 * oc.U * abs(nc), f"{key} step {i}: norm_out {nc!r} (C) and {nd!r} (D)"
        else:
            assert np.array([nc], np.float32).tobytes() == np.array([nd], np.float32).tobytes() or (np.isnan(nc) and np.isnan(nd)), f"{key} step {i}: norm_out {nc!r} (C) and {nd!r} (D)"
        assert (sc["nan_flag"], sc["stop_flag"]) == (sd["nan_flag"], sd["stop_flag"])


def test_worst_error_over_bound_per_route(outputs):
    """the figures of docs/kernels/ppo_kernels.md, "optimiser tail: direct tests" """
    for route in "ABCD":
        worst = dict.fromkeys(oc.RATIOS, 0.0)
        for c in (c for c in oc.CASES if c.route == route):
            w, _ = _evaluate(c.name, str(outputs))
            worst = {k: max(worst[k], w[k]) for k in worst}
        print(f"[optim worst] route {route}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert all(v <= 1.0 for v in worst.values())
