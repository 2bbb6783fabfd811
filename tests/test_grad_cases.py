"""CPU: the infrastructure of the direct tests of the PPO gradient kernels (tests/grad_cases.py) held against three independent things, without a GPU:
  * its float64 reference against torch's float64 autograd (torch_ppo_loss of tests/test_oracle_crosschecks.py) on every configuration of the table: every element within
    1e-12 of the LARGEST gradient element plus 2^-50 T[e], the float64 rounding of the two sums themselves (about 1e-10 relative on a typical element);
  * its bounds against the project's f32 CPU oracle: orc_ppo_loss_grad meets ONE QUARTER of every bound on every case — true by construction of the constants
    (4 x the oracle's worst ratio), pinned here so that an edit of the table re-measures them;
  * its assertion functions against defects: the oracle's output with one defect each must be rejected on every row the defect applies to.
tests/test_gpu_grad.py feeds the same functions the device's outputs."""
import numpy as np
import pytest

import grad_cases as gc
from test_oracle_crosschecks import torch_ppo_loss

CONFIGS = sorted({(r.kind, r.H) for r in gc.ROWS})
FAMILY_OF = {"ind_actor": ("ind_actor", "j33"), "ind_critic": ("ind_critic", "j64"), "decisions": ("decisions", ""), "norm_noent": ("equal_adv", "")}


def _row_of(kind, H):
    return next(r for r in gc.ROWS if (r.kind, r.H) == (kind, H))


def test_the_table_is_the_one_the_issue_lists():
    names = {r.kernel for r in gc.ROWS}
    assert names == {"ppo_grad_kernel", "ppo_grad_pair_kernel", "ppo_grad_wide_kernel", "ppo_grad_wide_split_kernel", "generic path"}
    by = lambda kernel: [r for r in gc.ROWS if r.kernel == kernel]
    assert {(r.kind, r.H) for r in by("ppo_grad_kernel")} == {(k, 64) for k in (0, 1, 3, 4, 6)} | {(0, 32), (1, 32)}
    assert {r.kind for r in by("ppo_grad_pair_kernel")} == {0, 1, 3, 4, 6} and sum(r.chip for r in gc.ROWS) == 2
    for kernel in ("ppo_grad_wide_kernel", "ppo_grad_wide_split_kernel"):
        assert {(r.kind, r.H) for r in by(kernel)} == {(k, H) for k in (0, 1, 6) for H in (128, 256)}
    assert set(gc.CONSTANTS) == set(gc.BLOCKS + gc.STATS) and all(gc.CONSTANTS[k] == 4.0 * gc.ORACLE_WORST[k] for k in gc.CONSTANTS)
    for r in gc.ROWS:                                                                # every setting x parameter scale of the random family within every row
        rnd = {(c.setting, c.scale) for c in gc.cases_of(r) if c.family == "random"}
        assert rnd == {(s, sc) for s in ("default", "ent_vfclip", "no_norm") for sc in gc.scales(r.H)}, r.name
    assert gc.indicator_slots(gc.ROW_BY_NAME["f32.k0.h64.gmax1"], 300) == [0, 31, 32, 128, 288, 299]
    assert gc.indicator_slots(gc.ROW_BY_NAME["pair.k0.gmax2"], 333) == [0, 31, 32, 64, 320, 332]


@pytest.mark.parametrize("kind,H", CONFIGS)
def test_reference_vs_torch_float64_autograd(pkg, kind, H):
    """loss, the seven statistics and every gradient element against autograd, for every loss setting and both parameter scales: within 1e-12 of the value (gradient:
    of the largest element) plus 2^-50 of the absolute addends T, which is what two float64 summation orders may differ by"""
    row = _row_of(kind, H)
    for setting in gc.SETTINGS:
        for scale in gc.scales(H):
            fam, tag = FAMILY_OF.get(setting, ("random", ""))
            case = gc.Case(row, 97, fam, setting, scale, tag)
            flat, batch = gc.inputs(case)
            ref = gc.ref_of(case)
            cfg = gc.make_cfg(pkg._capi, row, setting)
            tl, ts, tg = torch_ppo_loss(flat, cfg, *batch, row.dims[2], row.dims[1])
            assert abs(ref.loss - tl) <= 1e-12 * abs(tl) + 2.0 ** -50 * ref.stat_T["loss"], case.name
            for k, slot in gc.STAT_SLOT.items():
                assert abs(ref.stats[slot] - ts[slot]) <= 1e-12 * abs(ts[slot]) + 2.0 ** -50 * ref.stat_T[k], (case.name, k)
            assert ref.stats[3] == ts[3] and ref.clip_count == round(ts[3] * 97)
            # (2^-50 T: both sides are float64 sums with their own rounding, 2^-53 per operation against the absolute addends — log_std at scale 1 cancels 1e4 : 1)
            assert np.all(np.abs(ref.g - tg) <= 1e-12 * np.max(np.abs(tg)) + 2.0 ** -50 * ref.T), case.name
            assert np.all(ref.T >= np.abs(ref.g) * (1 - 1e-12)), f"{case.name}: the absolute-value pass must dominate the signed one"
            if fam == "random":
                assert 0 < ref.clip_count < 97                                       # some ratios are clipped, not all


@pytest.mark.parametrize("row", gc.ROWS, ids=lambda r: r.name)
def test_oracle_meets_a_quarter_of_every_bound(oracle_mod, row):
    """and the exact expectations of the families (zero blocks, zero dW1 column, the clip count) hold for it"""
    run = gc.OracleRunner(oracle_mod, row)
    for case in gc.cases_of(row):
        gc.check(case, run.run(case), gc.ref_of(case), limit=0.25)


@pytest.mark.parametrize("kind,H", CONFIGS)
def test_f32_takes_the_decisions_of_float64(oracle_mod, kind, H):
    """the precondition of the decision family: the margins (1e-3 of the ratio, 1e-2 of clip_range_vf) are far above the f32 error of logp and V, so that the oracle's
    own f32 forward pass puts every sample on the side float64 puts it — zero disagreements — and the clip count is the one the construction gives"""
    row = _row_of(kind, H)
    for B in (33, 257):
        case = gc.Case(row, B, "decisions", "decisions", gc.scales(H)[0])
        flat, (obs, act, adv, ret, olp, ov) = gc.inputs(case)
        ref, cfg = gc.ref_of(case), gc.make_cfg(oracle_mod.capi, row, "decisions")
        o = oracle_mod.Oracle(cfg)
        o.set_params(flat)
        v32, lp32, _ = o.evaluate_actions(obs, act)
        r32 = np.exp((lp32 - olp).astype(np.float32))
        c, cv = np.float32(cfg.clip_range), np.float32(cfg.clip_range_vf)
        out32 = (r32 < np.float32(1) - c) | (r32 > np.float32(1) + c)
        d32 = v32 - ov
        assert np.array_equal(out32, ref.ratio_clipped) and np.array_equal((d32 < -cv) | (d32 > cv), ref.v_clipped), case.name
        assert ref.clip_count == gc.expected_clip_count(case) and 0 < ref.v_clipped.sum() < B and ref.blocked.any() and (ref.ratio_clipped & ~ref.blocked).any()


# a defect applies to a row when it changes the float64 result of at least one of the row's cases
# std_uncorrected scales the normalised advantages by sqrt((n - 1) / n), 1 / (2 n) relative: 3e-5 at n = 16 417, which is inside the f32 bound of every output of a
# minibatch that large (error / bound 0.02 - 0.1).  It cannot be rejected by a check of outputs on the two chip-filling rows; every other row rejects it (1.5e-3 at
# n = 333 leaves the dW1 bound by 3 - 20 x), and the chip-filling rows run the same advantage-moment launches as those (ppo_step)
NOT_APPLICABLE = {"swap_dW3_rows": lambda r: not r.dims[2], "log_std_no_entropy": lambda r: r.dims[2], "log_std_missing": lambda r: r.dims[2],
                  "std_uncorrected": lambda r: r.chip}


def _may_change(case, defect):
    """cheap necessary conditions, so that the float64 pass with the defect runs only where it can differ"""
    st = gc.SETTINGS[case.setting]
    return {"vclip_passes": st.get("has_clip_range_vf", 0) == 1, "std_uncorrected": st.get("normalize_advantage", 1) == 1, "log_std_no_entropy": st.get("ent_coef", 0.0) > 0,
            "drop_last_ragged": case.B % gc.K_TILE != 0, "invB_tile_rounded": case.B % gc.K_TILE != 0}.get(defect, True)


@pytest.mark.parametrize("row", gc.ROWS, ids=lambda r: r.name)
def test_every_defect_is_rejected(oracle_mod, row):
    """the oracle's output with one defect each: the first case of the row that the defect changes — the random family comes first — must already be rejected, and the
    same case without the defect passes.  (dW3 has one row on the one-dimensional Gaussian heads, log_std exists on them alone: those combinations do not exist.)"""
    run = gc.OracleRunner(oracle_mod, row)
    cases = gc.cases_of(row)
    for defect in gc.DEFECTS:
        if NOT_APPLICABLE.get(defect, lambda r: False)(row):
            continue
        for case in cases:
            if not _may_change(case, defect):
                continue
            out = run.run(case)
            bad, changed = gc.with_defect(case, out, defect)
            if not changed:
                continue
            gc.check(case, out, gc.ref_of(case))
            with pytest.raises(AssertionError):
                gc.check(case, bad, gc.ref_of(case))
            break
        else:
            pytest.fail(f"{row.name}: no case of the row is changed by {defect}")
