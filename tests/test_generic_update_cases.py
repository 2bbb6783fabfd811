"""CPU: the case table of the one-launch generic update (tests/generic_update_cases.py) held to its own terms — the float64 restatement of one update agrees with the
oracle on every case at the tolerances the device is later held to, the table covers what it says it covers, and the armed target_kl case stops where it was aimed."""
import numpy as np
import pytest

import generic_update_cases as G


@pytest.mark.parametrize("c", G.ALL + [G.KL_MID], ids=lambda c: c["name"])
def test_float64_restatement_agrees_with_the_oracle(pkg, oracle_mod, c):
    capi = pkg._capi
    r = G.reference(oracle_mod, capi, c)
    so, f = r["stats"], r["f64"]
    assert r["cfg"].n_hidden == len(c["hidden"]) and oracle_mod.Oracle(r["cfg"]).P == G.param_count(c) == r["flat"].size
    assert (so.n_updates, so.early_stopped, so.nan_or_inf) == (f["n_updates"], f["early_stopped"], f["nan_or_inf"])
    if so.n_updates and c["epochs"] <= 2:
        assert so.loss == pytest.approx(f["loss"], rel=G.LOSS_REL, abs=G.LOSS_ABS) and so.grad_norm == pytest.approx(f["grad_norm"], rel=G.GNORM_REL)
    elif so.n_updates:   # means over a long update: the learn_stats tolerance of the configs[0] test
        assert so.loss == pytest.approx(f["loss"], rel=2e-3, abs=5e-6) and so.grad_norm == pytest.approx(f["grad_norm"], rel=2e-3)
    if c["epochs"] <= 2:
        np.testing.assert_allclose(r["params"], f["params"], rtol=G.PARAM_RTOL, atol=G.PARAM_ATOL)
    else:   # a long update on a non-smooth loss: the float64 yardstick rule of the configs[0] test, here for the oracle against the Float32 loop
        r = G.reference(oracle_mod, capi, c, with_f32=True)
        _, r_orc, r_f32 = G.distances(r, r["params"])
        print(f"[{c['name']}] distance from the float64 loop: oracle {r_orc:.2e}, Float32 loop {r_f32:.2e}")
        assert r_orc <= max(3.0 * r_f32, 1e-5)
    if c["epochs"] == 0:
        assert np.array_equal(r["params"], r["flat"]) and so.n_updates == 0


def test_the_table_covers_what_the_kernel_can_get_wrong():
    one = G.ONE_STEP
    assert {len(c["hidden"]) for c in one} >= {1, 2, 4}
    assert any(w % 4 for c in one for w in c["hidden"]) and any(c["hidden"] == (64, 64) for c in one)
    assert {c["act"] for c in one} == set(G.ACT) and {c["discrete"] for c in one} == {True, False}
    assert {c["kw"].get("action_start", 1) for c in one if c["discrete"]} == {0, 1}
    assert {c["kw"].get("has_clip_range_vf", 0) for c in one} == {0, 1} and all(c["kw"]["ent_coef"] != 0 for c in one)
    assert all(c["epochs"] == 1 and c["B"] >= G.n_of(c) for c in one)                        # one optimiser step each
    assert {2, 7, 33, 64} <= {c["B"] for c in one}                                           # below a tile, a ragged tile, two tiles with a ragged second, two full tiles
    assert max(c["D"] for c in one) == 16 and max(c["A"] for c in one) == 8
    nb = lambda c: -(-G.n_of(c) // c["B"])
    assert nb(G.CHUNKS) * G.CHUNKS["epochs"] == 14 and G.n_of(G.CHUNKS) % G.CHUNKS["B"]
    assert nb(G.README) * G.README["epochs"] == 1280 and nb(G.README_SHORT) * G.README_SHORT["epochs"] == 256
    assert G.COUNT[1]["epochs"] == 4 * G.COUNT[0]["epochs"]


def test_the_armed_target_kl_stops_in_the_middle_of_the_second_epoch(pkg, oracle_mod):
    capi = pkg._capi
    c, s_star = G.kl_mid_case(oracle_mod, capi)
    nb = -(-G.n_of(c) // c["B"])
    assert nb < s_star < 2 * nb - 1
    r = G.reference(oracle_mod, capi, c)
    assert (r["stats"].n_updates, r["stats"].early_stopped, r["stats"].nan_or_inf) == (s_star, 1, 0)
    assert (r["f64"]["n_updates"], r["f64"]["early_stopped"]) == (s_star, 1)
    kl = np.asarray(G.reference(oracle_mod, capi, G.KL_MID)["f64"]["kl"]); lim = 1.5 * c["kw"]["target_kl"]
    assert kl[s_star] > 1.14 * lim and kl[:s_star].max() < lim / 1.14                        # more than rounding away on both sides
