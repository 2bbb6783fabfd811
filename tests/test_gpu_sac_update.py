"""GPU: the SAC update! step (sac_one_update: sac_gather[_l1]_kernel, sac_actor_out_ent_kernel<PRE>, sac_q_out_head_kernel, sac_dx_squash_kernel, sac_adam_kernel /
sac_step_end_kernel with first_layer_opt_block, the four unfused head kernels) through dril_sac_update, EVERY ELEMENT of both gradients, of the parameters and of the
targets, log_ent_coef and the statistics against the float64 reference of tests/sac_update_cases.py: one test per row of its table (a route of sac_one_update and the
shapes that reach it), each running the row's batch sizes and input families — random, one-sample indicators, saturated actions, decisions on both sides of both twin
minima, exact ties, edges — as three consecutive steps at target_update_interval 1 and 2 and one step at learning_rate = 0, every sequence twice from the same state
(bit-identical), through the assertion functions that tests/test_sac_update_cases.py holds against the CPU oracle and seventeen defects.  The route that ran is asserted
through dril_sac_update_info() on every step.  The row's switches are latched by dril_sac_create: they are set before a handle is made and removed afterwards."""
import json

import pytest

import sac_update_cases as sc

pytestmark = pytest.mark.gpu


class _Switched(sc.RowRunner):
    def __init__(self, pkg, row, monkeypatch):
        super().__init__(pkg, row)
        self.mp = monkeypatch

    def handle(self, *key):
        if key not in self.handles:
            for k in self.row.switches:
                self.mp.setenv(k, "1")
            try:
                return super().handle(*key)
            finally:
                for k in self.row.switches:
                    self.mp.delenv(k, raising=False)
        return self.handles[key]


@pytest.mark.parametrize("row", sc.ROWS, ids=lambda r: r.name)
def test_update_row_vs_float64(pkg, monkeypatch, row):
    run = _Switched(pkg, row, monkeypatch)
    worst, n_seq, n_jump = {}, 0, 0
    try:
        for case in sc.cases_of(row):
            for seq in case.sequences:
                (t0, cfg), (t1, _) = run.run(case, seq), run.run(case, seq)
                sc.check_same(case, t0, t1)
                sc.check_route(case, t0)
                refs = sc.replay_refs(case, t0, cfg)
                n_seq += 1
                n_jump += any(r.margins["jumps"] for r in refs)                      # (check() asserts: saturated/edge alone)
                for k, (q, s, i) in sc.check(case, t0, refs).items():
                    if q > worst.get(k, (0.0, ""))[0]:
                        worst[k] = (q, f"{case.name}/{seq[0]}/step{s}[{i}]")
    finally:
        run.close()
    print("[sac update row]", json.dumps({"row": row.name, "route": row.route, "sequences": n_seq, "sequences_with_a_jump_in_T": n_jump, "worst_error_over_bound": {k: round(v[0], 4) for k, v in worst.items()},
                                           "at": {k: v[1] for k, v in worst.items()}}))
