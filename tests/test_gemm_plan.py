"""CPU: where every row of the contraction case table (tests/gemm_cases.py) lands, by the library's own selection — tests/gemm_check.hip --plan calls gemm_prepare /
gemm_select / gemm_splitk_body of dril_gemm.hip and makes no HIP call, so it runs without a GPU.  tests/test_gpu_gemm.py then runs the same table on the device; this
module is what says WHICH kernel each of those results came from.  It also shows that the split criterion used there (RMS error against float64 at most twice the
exact-f32 kernel's) can tell the six-product split from a four-product one, on the numpy emulation of both."""
import subprocess

import numpy as np
import pytest

import gemm_cases as gc


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = gc.build_driver()
    runs = [(c, m) for c in gc.CASES for m in gc.MODES] + [(gc.big_twin(c), "normal") for c in gc.SPLIT_CASES]
    path = tmp_path_factory.mktemp("gemm_plan") / "cases.txt"
    gc.write_case_file(path, runs)
    r = subprocess.run([str(exe), "--plan", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = dict(line.split() for line in r.stdout.splitlines())
    assert len(got) == len(runs)
    return runs, got


def test_every_case_lands_on_the_target_its_row_names(plan):
    runs, got = plan
    wrong = [(gc.run_name(c, m), c.target, got[gc.run_name(c, m)]) for c, m in runs if got[gc.run_name(c, m)] != c.target]
    assert not wrong, wrong


def test_the_table_reaches_all_18_targets(plan):
    runs, got = plan
    assert len(gc.TARGETS) == 18 and len(set(gc.TARGETS)) == 18
    reached = {got[gc.run_name(c, m)] for c, m in runs if c.kind == 0}
    assert reached == set(gc.TARGETS), sorted(set(gc.TARGETS) ^ reached)
    for t in gc.TARGETS:                                                                # and each of them in both modes
        assert {m for c, m in runs if c.kind == 0 and c.target == t} == set(gc.MODES), t


def test_pair_launches_mix_lds_and_direct_bodies(plan):
    _, got = plan
    pairs = {v for k, v in got.items() if v.startswith("pair:")}
    assert len(pairs) >= 2
    for p in pairs:
        bodies = p[5:].split("+")
        assert len(bodies) == 2 and "direct_splitk" in bodies and any(b.startswith("lds_") for b in bodies), p


def test_multi_launches_of_1_3_and_4_contractions(plan):
    _, got = plan
    counts = {len(v[6:].split("+")) for v in got.values() if v.startswith("multi:")}
    assert counts == {1, 3, 4}


def test_split_cases_have_an_f32_twin_on_the_big_kernel_of_the_same_layout(plan):
    _, got = plan
    for c in gc.SPLIT_CASES:
        assert got[gc.run_name(gc.big_twin(c), "normal")] == "big_" + c.target[6:11], c.name


SPLIT_KS = sorted({c.cons[0].K for c in gc.SPLIT_CASES})


@pytest.mark.parametrize("K", SPLIT_KS)
@pytest.mark.parametrize("rounding", ["nearest", "truncate"])
def test_the_2x_criterion_tells_six_products_from_four(K, rounding):
    """standard-normal operands at the split cases' own K: the six-product emulation stays within twice the f32 chain's RMS distance from float64, the four-product
    one (the DRIL_DEBUG_DROP_LO build: 2^-16 relative) breaks it by more than an order of magnitude.  `nearest` is what split3_pair does; `truncate` (the pieces
    cut by masking, the earlier form of the split) has to separate the two as well"""
    rng = np.random.default_rng(K)
    A, B = rng.standard_normal((48, K), dtype=np.float32), rng.standard_normal((K, 40), dtype=np.float32)
    ref = A.astype(np.float64) @ B.astype(np.float64)
    f32 = gc.rms(gc.emulate_f32(A, B) - ref)
    six = gc.rms(gc.emulate_split(A, B, 6, rounding) - ref)
    four = gc.rms(gc.emulate_split(A, B, 4, rounding) - ref)
    print(f"[split emulation] K {K} {rounding}: six / f32 {six / f32:.2f}, four / f32 {four / f32:.1f}")
    assert six <= 2.0 * f32
    assert four > 2.0 * f32 and four > 10.0 * f32


def test_split3_is_exact_and_the_exact_mode_operands_sit_in_the_first_piece():
    x = np.random.default_rng(0).standard_normal(4096, dtype=np.float32)
    for rounding in ("nearest", "truncate"):
        hi, mid, lo = gc.split3(x, rounding)
        assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64), x.astype(np.float64))
        for p in (hi, mid, lo):
            assert not np.any(p.view(np.uint32) & np.uint32(0xFFFF))
        e = (np.arange(-8, 9) / 8.0).astype(np.float32)
        hi, mid, lo = gc.split3(e, rounding)
        assert np.array_equal(hi, e) and not mid.any() and not lo.any()


def test_exact_mode_maps_every_epilogue_onto_none_relu_mask_relu():
    assert {gc.exact_epi(e) for e in gc.EPI} == {"NONE", "RELU", "MASK_RELU"}
    for c in gc.CASES:
        for con in c.cons:
            assert con.alpha in (1.0, 0.5)
