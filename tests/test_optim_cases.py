"""CPU: the case table of the optimiser-tail tests (tests/optim_cases.py) is held to its own terms before any GPU sees it.

  * the numpy float32 emulation of the kernels' expressions stays at or below HALF of every bound on every case — the condition that keeps the bounds honest (a
    case that breaks it gets other inputs, never another constant);
  * the assertion functions tests/test_gpu_optim.py uses reject emulated outputs with one defect each (the mutants);
  * the decisions of the table are the ones it names (which steps clip, stop on kl, are poisoned), and no undecided step sits near a threshold;
  * the Python layout arithmetic agrees with tests/golden/param_counts.json.
"""
import json
from pathlib import Path

import numpy as np
import pytest

import optim_cases as oc

SINGLE = [c for c in oc.CASES if len(c.steps) == 1]


def _plain(c, route, shift=None):
    return c.route == route and len(c.steps) == 1 and c.mode == "normal" and not c.steps[0].variant and c.steps[0].use_stats and c.steps[0].has_max and \
        (shift is None or c.steps[0].shift == shift) and c.layout.L > 0


def _pick(route, pred):
    return next(c for c in oc.CASES if c.route == route and pred(c))


@pytest.mark.parametrize("route", "ABCD")
def test_emulation_stays_within_half_of_every_bound(route):
    worst = dict.fromkeys(oc.RATIOS, 0.0)
    for c in (c for c in oc.CASES if c.route == route):
        e = oc.emulate(c)
        w, _ = oc.check_case(c, e, e, limit=0.5)
        worst = {k: max(worst[k], w[k]) for k in worst}
    print(f"[optim emulation] route {route}: worst error / bound {worst}")


def test_table_covers_what_it_names():
    names = {c.name for c in oc.CASES}
    for route, counts in (("A", oc.COMMON + oc.A_ONLY), ("B", oc.COMMON)):
        assert {(c.G, c.Gc) for c in oc.CASES if c.route == route} >= set(counts)
    assert {c.layout for c in oc.CASES if c.route == "A"} == set(oc.LAYOUTS) and len(oc.LAYOUTS) == 12
    assert {c.layout for c in oc.CASES if c.route == "B"} == {l for l in oc.LAYOUTS if l.P <= 16384}
    assert oc.S16384.P == 16384 and oc.PENDULUM128.P in range(16385, 65537) and oc.PENDULUM256.P > 65536
    for route in "ABCD":
        single = [c for c in SINGLE if c.route == route and not c.steps[0].variant]
        assert {c.steps[0].n for c in single} == set(oc.SAMPLE_COUNTS)
        assert {(c.mode, c.zero_params) for c in single} >= {("normal", True), ("normal", False), ("exact", False)}
        assert f"{route}.pendulum64.seq" in names and f"{route}.s33_31_3.seq" in names
    assert {c.steps[0].use_stats for c in oc.CASES if c.route == "C"} == {0, 1}


@pytest.mark.parametrize("route", "ABCD")
def test_decisions_are_the_ones_the_table_names(route):
    """and every step that is not a decision case is far from both thresholds: the float64 reference and an f32 kernel cannot decide differently"""
    seen = set()
    for c in (c for c in oc.CASES if c.route == route):
        e = oc.emulate(c)
        _, dec = oc.check_case(c, e, e)
        for st, d in zip(c.steps, dec):
            if d.get("launched_stopped"):
                continue
            seen.add((c.mode, d["clip"]))
            poisoned = st.variant.startswith(("nan_", "inf_", "overflow"))
            assert d["bad"] == poisoned, (c.name, st, d)
            assert d["kl_stop"] == (st.variant in ("kl=64000", "kl=24.000001907348633") and bool(st.has_kl)), (c.name, st, d)
            if st.variant != "norm0625" and st.has_max and not d["bad"]:
                assert d["norm"] == float(st.max_norm) or abs(d["norm"] / float(st.max_norm) - 1) > 1e-3, (c.name, d)      # (exact operands may tie: then both sides hold the same number)
            if not st.variant.startswith("kl=") and st.use_stats and st.has_kl:
                assert abs(d["kl"]) < 0.9 * 0.375, (c.name, d)
        if len(c.steps) == 12:
            assert [bool(d.get("clip")) for d in dec] == [i == 3 for i in range(12)], c.name
            assert [bool(d.get("kl_stop")) for d in dec] == [i == 5 for i in range(12)] and [bool(d.get("bad")) for d in dec] == [i == 9 for i in range(12)], c.name
            assert [bool(d.get("launched_stopped")) for d in dec] == [i == 6 for i in range(12)], c.name
    assert seen >= {("normal", True), ("normal", False), ("exact", True), ("exact", False)}
    by = {c.name.split(".")[-1]: oc.check_case(c, oc.emulate(c), oc.emulate(c))[1][0] for c in oc.CASES if c.route == route and c.key.startswith("s33_31_3.") and len(c.steps) == 1
          and "." not in c.key[len("s33_31_3."):]}
    assert [by[k]["clip"] for k in ("clip_eq", "clip_above", "clip_below", "clip_off")] == [False, True, False, False]
    assert all(by[k]["norm"] == 0.625 for k in ("clip_eq", "clip_above", "clip_below")) and by["clip_off"]["norm"] > 1000
    assert [by[k]["kl_stop"] for k in ("kl_eq", "kl_above", "kl_off")] == [False, True, False]
    assert by["kl_eq"]["kl"] == 0.375 and by["kl_above"]["kl"] == float(np.nextafter(np.float32(0.375), np.float32(1))) and by["kl_off"]["kl"] == 1000.0
    single = oc.BY_NAME.get(f"{route}.pendulum64.g31x32.single_1e19")
    d = oc.check_case(single, oc.emulate(single), oc.emulate(single))[1][0]
    assert d["clip"] and not d["bad"] and d["norm"] > 9e18


# ---- mutants: (defect, the cases it is run on).  Every one must make the assertion functions of the GPU test fail.
def _mutant_cases(defect):
    out = []
    for route in "ABCD":
        if defect in ("drop_slab", "logstd_from_critic", "stat_slot_off"):
            if route in "AB":
                out += [oc.BY_NAME[f"{route}.s33_31_3.g2x1.exact"], oc.BY_NAME[f"{route}.s33_31_3.g2x1.normal"], oc.BY_NAME[f"{route}.pendulum64.g31x32.normal"]]
                if route == "A":
                    out += [oc.BY_NAME["A.s40_50_6.g255x129.exact"], oc.BY_NAME["A.pendulum64.g33x32.normal"]]
        elif defect in ("bt_stale", "eps_in_sqrt"):
            out += [_pick(route, lambda c: _plain(c, route, 0)), _pick(route, lambda c: _plain(c, route, 12)), oc.BY_NAME[f"{route}.s33_31_3.seq"]]
        elif defect == "clip_m_only":
            out += [_pick(route, lambda c: _plain(c, route, 0)), oc.BY_NAME[f"{route}.s33_31_3.clip_above"], oc.BY_NAME[f"{route}.pendulum64.seq"]]
        elif defect == "kl_ge":
            out.append(oc.BY_NAME[f"{route}.s33_31_3.kl_eq"])
        elif defect == "bt_not_copied":
            out += [oc.BY_NAME[f"{route}.s33_31_3.kl_above"], oc.BY_NAME[f"{route}.pendulum64.g31x32.nan_actor0"], oc.BY_NAME[f"{route}.s33_31_3.seq"]]
        elif defect == "poison_writes_m":
            out += [oc.BY_NAME[f"{route}.pendulum64.g31x32.{p}"] for p in ("nan_actor0", "nan_critic_last", "nan_log_std", "overflow_3e19")] + [oc.BY_NAME[f"{route}.pendulum64.seq"]]
    return out


@pytest.mark.parametrize("defect", [d for d in oc.DEFECTS if d != "clip_ge"])
def test_mutant_is_rejected(defect):
    cases = _mutant_cases(defect)
    assert cases
    for c in cases:
        good, bad = oc.emulate(c), oc.emulate(c, defect)
        oc.check_case(c, good, good)
        with pytest.raises(AssertionError):
            oc.check_case(c, bad, bad)
        with pytest.raises(AssertionError, match="the two runs differ"):
            oc.check_case(c, good, bad)


def test_mutant_clip_ge_at_the_exact_threshold_is_the_same_function():
    """`norm >= max_grad_norm` where the kernels say `>`: at norm == max_grad_norm the scale is max_grad_norm / norm = 1.0f exactly (IEEE x / x), and the kernels multiply by
    the scale only when it differs from 1 — so at the exact threshold this mutant computes the same bits as the kernel, and one ulp to either side the two comparisons agree.
    No check of outputs can tell them apart, here or on a GPU: this test holds that the mutant's outputs ARE bit-identical (were a clip ever to do more than scale by
    max / norm — an epsilon in the denominator, a clamp — the identity would break and this test with it), and that the threshold cases decide as the kernel's `>` does.
    The comparison that does show, kl's, is among the rejected mutants (kl_ge)."""
    for route in "ABCD":
        for name in ("clip_eq", "clip_above", "clip_below"):
            c = oc.BY_NAME[f"{route}.s33_31_3.{name}"]
            good, bad = oc.emulate(c), oc.emulate(c, "clip_ge")
            _, dec = oc.check_case(c, good, bad)
            assert dec[0]["clip"] == (name == "clip_above")
        c = oc.BY_NAME[f"{route}.s33_31_3.clip_eq"]                       # the scale the mutant applies at the threshold
        assert np.float32(c.steps[0].max_norm) / np.float32(0.625) == np.float32(1)


def test_layout_arithmetic_matches_the_golden_parameter_counts():
    golden = json.loads((Path(__file__).parent / "golden" / "param_counts.json").read_text())
    kinds = {"CartPole": 0, "Pendulum": 1}
    for g in golden:
        kind = kinds[g["env"]]
        D, A, discrete = oc.ENV[kind]
        assert (D, A, discrete) == (g["obs_dim"], g["actor_out"], g["discrete"]) and g["hidden"][0] == g["hidden"][1]
        lay = oc.real_layout("golden", kind, g["hidden"][0])
        assert lay.P == g["total"], (g, lay)
    assert (oc.CARTPOLE64.P, oc.PENDULUM64.P, oc.PENDULUM256.P) == (9155, 8963, 134147)
    for lay in oc.LAYOUTS:                                                  # the slab rule: rounded up to 4 floats, room for the 8 statistics behind the gradients
        assert lay.slab_a % 4 == 0 and lay.slab_c % 4 == 0 and 0 <= lay.slab_a - (lay.Pa + lay.L + 8) < 4 and 0 <= lay.slab_c - (lay.Pc + 8) < 4
