"""CPU: the infrastructure of the direct tests of the SAC update! step (tests/sac_update_cases.py) held against three independent things, without a GPU:
  * its float64 reference against TorchSAC, the torch float64 autograd restatement of tests/test_sac_oracle.py, over three consecutive steps on every shape of the
    table: every gradient element, parameter and target within 1e-12 of the LARGEST element of its block plus 2^-50 T[e], every loss and log_ent_coef likewise;
  * its bounds against the project's f32 CPU oracle: orc_sac_update meets ONE QUARTER of every bound on every case — true by construction of the constants
    (4 x the oracle's worst ratio), pinned here so that an edit of the table re-measures them — together with the conditions on the inputs that check() asserts
    (no twin minimum and no clamp within 64 forward-error units of its edge, no differentiated relu pre-activation within 2 of its kink, no decision's jump in T outside
    saturated/edge; both sides of every decision present);
  * its assertion functions against defects: the oracle's trace with one defect each must be rejected on every row the defect applies to.
tests/test_gpu_sac_update.py feeds the same functions the device's traces."""
import numpy as np
import pytest

import sac_update_cases as sc
from test_sac_oracle import TorchSAC

SHAPES = sorted({(r.D, r.A, r.hidden, r.act, r.ent) for r in sc.ROWS})


def _row_of(shape):
    return next(r for r in sc.ROWS if (r.D, r.A, r.hidden, r.act, r.ent) == shape)


def test_the_table_is_the_one_the_issue_lists():
    by = lambda **kw: [r for r in sc.ROWS if all(getattr(r, k) == v for k, v in kw.items())]
    fused = by(gather="l1", head="fused,pre", dw1="fused")
    assert {r.W for r in fused} == {3, 4} and {r.hidden for r in fused} == {(32, 32), (16, 260), (20, 24), (512, 512)}
    assert 1024 in {B for r in fused for B in r.sizes} and any(r.hidden == (512, 512) and 256 in r.sizes for r in fused)
    nodw1 = by(gather="l1", head="fused,pre", dw1="launch")
    assert {r.hidden for r in nodw1 if r.switches == ("DRIL_SAC_NO_FUSED_DW1",)} == {(32, 32), (20, 24)}
    assert {B for r in nodw1 if not r.switches for B in r.sizes} == {1028}
    assert {r.hidden for r in by(gather="l1", head="fused,nopre", dw1="fused")} == {(516, 32)}
    assert {(r.D, r.A) for r in by(gather="l1", head="fused,nopre", dw1="launch")} == {(4, 1), (11, 5), (8, 8)}
    assert {(r.D, r.A) for r in by(gather="plain", head="fused,nopre")} == {(16, 1), (1, 16), (40, 6)}
    unf = by(head="unfused")
    assert {(r.D, r.A) for r in unf} == {(3, 1), (11, 5)} and all(r.switches == ("DRIL_SAC_NO_FUSED_HEADS",) and {7, 257} <= set(r.sizes) for r in unf if r.ent == "auto")
    for route in {r.route for r in sc.ROWS}:                                         # both entropy coefficients and both activations on every route
        rs = [r for r in sc.ROWS if r.route == route]
        assert {r.ent for r in rs} == {"auto", "fixed"} and {r.act for r in rs} == {"relu", "tanh"}, route
    for r in sc.ROWS:
        assert (1 in r.sizes or min(r.sizes) >= 1024) and any(B % 64 for B in r.sizes), r.name
    assert set(sc.CONSTANTS) == set(sc.KEYS) and all(sc.CONSTANTS[k] == 4.0 * sc.ORACLE_WORST[k] for k in sc.KEYS)
    assert sc.indicator_slots(257) == [0, 128, 255, 256] and sc.indicator_slots(1) == [0]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"d{s[0]}a{s[1]}.h{s[2][0]}x{s[2][1]}.{s[3]}.{s[4]}")
def test_reference_vs_torch_float64_autograd(pkg, shape):
    """three consecutive steps (the reference's own gradients feed its Adam) against autograd + textbook Adam, target_update_interval 2, with
    TorchSAC's constants (double hyper-parameters, the clamp at 1 - 1e-6 in float64)"""
    row = _row_of(shape)
    B = 7 if max(row.hidden) < 512 else 3
    c0, c1 = sc.critic_range(row)
    for fam, tag in (("random", ""), ("saturated", "edge"), ("saturated", "far"), ("decision", ""), ("tie", ""), ("edges", "alpha_large"), ("edges", "gamma0tau1"), ("indicator", "j1")):
        case = sc.Case(row, B, fam, tag)
        inp = sc.inputs(case)
        gamma, tau = case.setting
        cfg, _ = sc.make_cfg(pkg, row, B, 2, sc.LR, gamma, tau)
        hp = dict(sc.hyper(cfg, row.A, hi=1 - 1e-6), lr=sc.LR, b1=0.9, b2=0.999, eps=1e-8, tau=tau, gamma=gamma, f32_bt=False)
        alg = pkg.SAC(learning_rate=sc.LR, gamma=gamma, tau=tau, target_update_interval=2)
        T = TorchSAC(inp["flat"], row.D, row.A, row.hidden, row.act, alg, inp["le0"], -float(row.A))
        T.target = [t.detach().clone() for t in TorchSAC(np.concatenate([inp["flat"][:c0], inp["target"], inp["flat"][c1:]]), row.D, row.A, row.hidden, row.act, alg, 0.0, 0.0).p[6:18]]
        tr = sc.Tracker(inp["flat"].size)
        for s in range(sc.N_STEPS):
            batch, noises = sc.batch_of(inp, s)
            # every step starts from TorchSAC's own state, moments included (the staging rule of the module: a saturated sample amplifies the last bit of tanh 5e5 times,
            # and two float64 trajectories part by that much)
            state = (T.flat(T.p), T.flat(T.target), T.log_ent.item())
            tr.m, tr.v, tr.ent[0], tr.ent[1] = T.flat(T.m), T.flat(T.v), T.ent_m, T.ent_v
            ref = sc.ref_step(row, hp, state, batch, noises, tr, own_scale=True)
            tgt, Ttgt, _ = sc.expected_target(ref, ref.params)
            st, gc, ga = T.update(batch[0], batch[1], batch[2], batch[3], batch[4], *noises, row.ent == "auto")
            full_c, full_a = np.zeros(ref.gc.size), np.zeros(ref.ga.size)
            full_c[c0:c1] = T.flat(gc)
            tga = T.flat(ga)
            full_a[:c0], full_a[c1:] = tga[:c0], tga[c0:]
            sl, _ = sc.row_layout(row)
            where = f"{case.name} step {s}"
            for b in sc.BLOCKS:
                lo, hi, _ = sl[b]
                for got, want, Tb in ((ref.gc, full_c, ref.Tgc), (ref.ga, full_a, ref.Tga), (ref.params, T.flat(T.p), ref.Tparams)):
                    assert np.all(np.abs(got[lo:hi] - want[lo:hi]) <= 1e-12 * np.abs(want[lo:hi]).max() + 2.0 ** -50 * Tb[lo:hi]), (where, b)
                if b in sc.CRITIC_BLOCKS:
                    want = T.flat(T.target)[lo - c0:hi - c0]
                    assert np.all(np.abs(tgt[lo - c0:hi - c0] - want) <= 1e-12 * np.abs(want).max() + 2.0 ** -50 * Ttgt[lo - c0:hi - c0]), (where, b)
            for k in ("critic_loss", "actor_loss", "mean_q_values", "entropy_coefficient", "grad_norm") + (("entropy_loss",) if row.ent == "auto" else ()):
                assert abs(ref.stats[k] - st[k]) <= 1e-12 * abs(st[k]) + 2.0 ** -50 * ref.statT[k], (where, k)
            assert abs(ref.stats["log_ent_coef"] - T.log_ent.item()) <= 1e-12 * abs(T.log_ent.item()) + 2.0 ** -50 * ref.statT["log_ent_coef"], where
            assert np.all(ref.Tgc >= np.abs(ref.gc) * (1 - 1e-12)) and np.all(ref.Tga >= np.abs(ref.ga) * (1 - 1e-12)), f"{where}: the absolute-value pass must dominate the signed one"
            assert ref.polyak == (s % 2 == 0)


def _oracle_runner(pkg, oracle_mod, row):
    return sc.RowRunner(pkg, row, oracle_mod.sac_oracle)


@pytest.mark.parametrize("row", sc.ROWS, ids=lambda r: r.name)
def test_oracle_meets_a_quarter_of_every_bound(pkg, oracle_mod, row):
    """... and the conditions on the inputs and the exact expectations of the families (zero sub-trees, closed polyak gate, learning_rate = 0, dead units, ties, both
    sides of every decision) hold for it"""
    run = _oracle_runner(pkg, oracle_mod, row)
    for case in sc.cases_of(row):
        for seq in case.sequences:
            trace, cfg = run.run(case, seq)
            sc.check(case, trace, sc.replay_refs(case, trace, cfg), limit=0.25)


def test_terminated_rows_hide_their_next_observation(pkg, oracle_mod):
    """the decision family's terminated rows carry next observations of 1e5: the oracle's update does not change when they are replaced by zeros (sac.jl:127,141;
    oracle/dril_sac_oracle.c:390), and would by orders of magnitude if they were read (the terminated_ignored defect)"""
    row = sc.ROW_BY_NAME["mid.d4a1"]                                                # (relu: a tanh net bounds what an observation of 1e5 can do to Q)
    case = sc.Case(row, 64, "decision")
    run = _oracle_runner(pkg, oracle_mod, row)
    trace, cfg = run.run(case, sc.SEQUENCES[0])
    inp = sc.inputs(case)
    obs, actn, rew, term, trunc, nobs = inp["replay"]
    assert term.sum() == 16 and np.abs(nobs[term.astype(bool)]).min() == 1e5
    h, _ = run.handle(64, 1, sc.LR, *case.setting)
    h.set_params(inp["flat"]); h.set_target_params(inp["target"]); h.set_log_ent_coef(inp["le0"]); h.reset_optimizer()
    h.replay_fill(obs, actn, rew, term, trunc, np.where(term.astype(bool)[:, None], 0.0, nobs).astype(np.float32))
    h.set_batches(1, inp["idx"][:1], *[z[:1] for z in inp["noises"]])
    h.update(1)
    assert h.last_grads()[0].tobytes() == trace[0]["gc"].tobytes()
    bad, changed = sc.with_defect(case, trace, cfg, "terminated_ignored")
    assert changed and np.abs(bad[0]["gc"]).max() > 1e3 * np.abs(trace[0]["gc"]).max()


# a defect applies to a row when it changes the float64 result of at least one of the row's cases.  Not rejectable, with the reason:
#   tie_to_critic1              on every row: a bit-for-bit tie needs identical twins, whose dQ/da are identical too, and no parameter gradient of a critic leaves the
#                               actor pass (zero_critic_grads!), so where the tie's gradient is sent is not observable in any output of update!
#   alpha_before_entropy_step   on the FixedEntropyCoefficient rows: alpha does not move
#   mean_over_first_256         on rows whose batches have at most 256 samples
#   min_is_critic0              on the 512 / 516-wide rows without the decision family: their twins are 3 apart (sac_update_cases._draw), critic 0 IS the minimum
#   inside_always_1             on fused.w4.h512: its saturated cases have one sample, and that one is at u = 6, inside the clamp;
#                               on fused.w4.h512.tanh, which runs the random family alone (no sample outside the clamp)
_WIDE_ONE_SIDED = lambda r: max(r.hidden) >= 512 and "decision" not in r.families
NOT_APPLICABLE = {"tie_to_critic1": lambda r: True, "alpha_before_entropy_step": lambda r: r.ent == "fixed", "mean_over_first_256": lambda r: max(r.sizes) <= 256,
                  "min_is_critic0": _WIDE_ONE_SIDED, "inside_always_1": lambda r: r.name == "fused.w4.h512" or "saturated" not in r.families}


@pytest.mark.parametrize("row", sc.ROWS, ids=lambda r: r.name)
def test_every_defect_is_rejected(pkg, oracle_mod, row):
    """the oracle's trace with one defect each: the first sequence of the row that the defect changes must already be rejected, and the same sequence without the defect
    passes"""
    run = _oracle_runner(pkg, oracle_mod, row)
    cases = sorted(sc.cases_of(row), key=lambda c: (c.B == 1, c.B))                  # one sample shows few defects: those cases come last
    for defect in sc.DEFECTS:
        if NOT_APPLICABLE.get(defect, lambda r: False)(row):
            continue
        for case in cases:
            if defect == "mean_over_first_256" and case.B <= 256 or defect == "inside_always_1" and (case.family, case.tag) != ("saturated", "far"):    # (at |u| = 7.2 / 7.3 the flag may legitimately differ: the jump is in T)
                continue
            seq = sc.SEQUENCES[1] if defect.startswith("polyak") else sc.SEQUENCES[0]
            if seq not in case.sequences:
                continue
            trace, cfg = run.run(case, seq)
            bad, changed = sc.with_defect(case, trace, cfg, defect)
            if not changed:
                continue
            refs = sc.replay_refs(case, trace, cfg)
            sc.check(case, trace, refs)
            with pytest.raises(AssertionError, match="error / bound"):
                sc.check(case, bad, refs)
            break
        else:
            pytest.fail(f"{row.name}: no case of the row is changed by {defect}")


def test_the_tie_is_not_observable(pkg, oracle_mod):
    """the reason tie_to_critic1 is listed above, as a check: on the tie family the defect changes no output bit"""
    row = sc.ROW_BY_NAME["fused.w4.h32"]
    run = _oracle_runner(pkg, oracle_mod, row)
    case = sc.Case(row, 7, "tie")
    trace, cfg = run.run(case, sc.SEQUENCES[0])
    assert not sc.with_defect(case, trace, cfg, "tie_to_critic1")[1]
