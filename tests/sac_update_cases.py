"""The case table of the SAC update! step (sac_one_update of dril.jl_amd/csrc/dril_sac_update.hip: sac_gather[_l1]_kernel, sac_actor_out_ent_kernel<PRE>, sac_q_out_head_kernel,
sac_dx_squash_kernel, sac_adam_kernel / sac_step_end_kernel with first_layer_opt_block, and the unfused sac_ent_next / sac_critic_head / sac_actor_head / sac_squash_bwd
kernels), its inputs, the float64 reference, the per-element error bounds and the assertion functions (test infrastructure of tests/test_sac_update_cases.py and
tests/test_gpu_sac_update.py; conventions and helpers of tests/grad_cases.py).

Reference: ref_step, a numpy float64 restatement of ONE update! (sac.jl:299-404) with a hand-written reverse pass, in the order of docs/sac.md "What update! does":
entropy-coefficient step; critic loss with the target networks and the updated alpha; critic Adam; actor loss through tanh -> clamp(+-(1 - 1e-6)) -> atanh -> logpdf with
the updated critics; actor + log_std Adam; the zero-gradient critic Adam (moments decay, second bias-correction tick); polyak, gated by grad_updates %
target_update_interval counted before the increment.  tests/test_sac_update_cases.py pins it to TorchSAC (float64 autograd, tests/test_sac_oracle.py).

Staging — every element is compared free of the divergence of an f32 and an f64 trajectory:
  * every step starts from the state read back from the implementation under test (parameters, targets, log_ent_coef: f32 values are exact in f64);
  * the Adam moments are not readable: a Tracker carries them in float64 from the gradients the implementation REPORTED (last_grads); the expected parameters are
    "its parameters before" minus "the float64 Adam step(s) from the tracked moments".  The entropy coefficient's gradient is not reported: its moments follow the
    reference's own -c, whose forward error enters T[log_ent_coef];
  * alpha of the critic and actor stages is exp of the log_ent_coef read back AFTER the step (it changes in the entropy stage only), so its only error is exp's;
  * the expected targets are the float64 polyak of the implementation's own parameters after the step (bit-identical to before when the gate is closed);
  * the actor stage uses the critics that the float64 Adam step gives from the reported critic gradient; they differ from the mid-step f32 critics by the rounding of
    that step, so there every critic parameter enters T with the input error |p| + E(step) (in u) — nothing at learning_rate = 0, where the critics do not move;
  * hyper-parameters are the f32 values of the config (beta2 = f32(0.999) makes 1 - beta2 differ from 0.001 by 1.3e-5), the clamp is at f32(1) - f32(1e-6).

Bound, with u = 2^-24:  |x - x64| <= c_block u T[e].  T is the absolute-value pass carried as a running error analysis, with the rules of grad_cases.py (above its
_forward_scale) plus:
  * an input with an error (the squashed action in a critic's input, a mid-step critic parameter) carries it: E(sum_k a_k b_k) has both E(a_k)|b_k| and |a_k|E(b_k);
  * relu: E(h) = [z > 0] E(z), and the derivative [z > 0] is exact unless f32 can put z on the other side of 0.  E(z) sums the absolute addends, so |z32 - z64| <= u E(z)
    to first order in ANY summation order: only |z| < 2 u E(z) can change side.  That is a condition on the INPUTS, like the two below: no differentiated relu
    pre-activation (the actor on obs, the critics in the critic and in the actor stage) of any sample comes within 2 units of its kink; inputs() draws such replay rows again
    on the CPU, check() asserts it on every step that runs.  (grad_cases.py carries E(1 - h^2) for tanh, which has no kink.)
  * the two twin-critic minima and the clamp's `inside` flag are decisions too.  In the random, indicator, decision and edge families NO sample comes within 64
    forward-error units of either (inputs() again; asserted by check()), so that NO case of the table but one carries a decision's jump in T — check() asserts the count
    is zero, and every element of those cases is held to the f32 bound proper.  The one: saturated/edge puts u = mu + sigma noise at +-7.2 and +-7.3, on both sides of
    atanh(1 - 1e-6) = 7.25 and within 4 units of the clamp's edge (which is only 17 u from 1; tanhf is good to 2 ulp).  There an f32 evaluation may take either branch, the
    jump |dlogp dlp_dg| enters T as 64 / u, and since every sample reaches every actor element, THE ACTOR-GRADIENT AND log_std BOUNDS OF saturated/edge ARE VOID: what
    that case checks is the critic side, the parameters and targets given the reported gradients, the statistics, the zero sub-trees, bit-identity and finiteness.
    saturated/far (+-6, +-9, +-20: saturated, `inside` = 0, 1 - x^2 = 0, and 8 units clear of the edge) holds every actor element, and is what rejects `inside` always 1;
  * Adam carries the conditioning of m^ / (sqrt(v^) + eps): E(m), E(v) by their recurrences (E(m) has the absolute addends |beta1 m| + |(1 - beta1) g|: a sign change
    of g cancels), beta^t is the host's f32 running product, reproduced bit for bit (a bound on it would cost 500 u of the step through 1 - beta2^t ~ 0.002), E(1 - beta^t) = 1 - beta^t, E(sqrt v^) = E(v^) / (2 sqrt v^) + sqrt v^ and
    E(step) = lr (E(m^) / den + |m^| E(den) / den^2) + 2 |step|, den = sqrt(v^) + eps.  With an exact g (the reported one) this is a few u of the step; with g's own
    error E(g) (the entropy coefficient) the first step is sign-like for |g| >> eps and E(step) ~ lr E(g) / (|g| + eps) grows as |g| -> eps.  No element is exempt.
Blocks: W1 b1 W2 b2 W3 b3 of the actor and of each critic plus log_std, with separate constants for the gradients (g.*), the parameters after the step (p.*) and the
targets (t.*); critic_loss, actor_loss, entropy_loss, mean_q_values, entropy_coefficient, grad_norm and log_ent_coef have one each.  The constants are not fitted to the
device: c = MARGIN x the largest error / (u T) that the f32 CPU oracle (orc_sac_* through oracle_lib.sac_oracle) reaches on this same table (ORACLE_WORST;
`python tests/sac_update_cases.py oracle` measures it again), MARGIN = 4 = 2 (another summation order) x 2 (headroom), the reasoning of grad_cases.py.

A row of the table is a route of sac_one_update (dril_sac_update_info names it) and the smallest shapes that reach it; a case is (row, B, family); it runs three
consecutive steps at target_update_interval 1 and 2, each sequence twice from the same state (bit-identical), and one step at learning_rate = 0 (parameters
bit-identical, both gradients against the reference without the mid-step term).  Families: random, indicator, saturated (edge / far), decision (mirrored twin critics and targets:
both sides of both minima; terminated rows whose next observation is 1e5 — sac.jl:127,141 drop them, oracle/dril_sac_oracle.c:390 does), tie (identical twins: q0 == q1
bit for bit, the choice is critic 0, oracle/dril_sac_oracle.c:438), edges (log_ent_coef -12 / +4, gamma = 0 with tau = 1, rewards 1e4, dead relu units).
The b1028 row has no B = 1: its route IS the batch size.
"""
from __future__ import annotations

import functools
import json
import math
import sys
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from grad_cases import F, TINY, U, _rng, environ  # noqa: E402  (the shared conventions: u, the seeded generator, the env switch context)

NET_BLOCKS = ("W1", "b1", "W2", "b2", "W3", "b3")
NETS = ("actor", "q0", "q1")
BLOCKS = tuple(f"{n}.{b}" for n in NETS for b in NET_BLOCKS) + ("log_std",)
ACTOR_BLOCKS = tuple(f"actor.{b}" for b in NET_BLOCKS) + ("log_std",)
CRITIC_BLOCKS = tuple(f"{n}.{b}" for n in ("q0", "q1") for b in NET_BLOCKS)
STATS = ("critic_loss", "actor_loss", "entropy_loss", "mean_q_values", "entropy_coefficient", "grad_norm", "log_ent_coef")
KEYS = tuple(f"g.{b}" for b in BLOCKS) + tuple(f"p.{b}" for b in BLOCKS) + tuple(f"t.{b}" for b in CRITIC_BLOCKS) + STATS
KINK = 64.0                      # forward-error units below which a decision may fall on the other side in f32
KINK_RELU = 2.0                  # a relu pre-activation: |z32 - z64| <= u E(z) to first order whatever the summation order (E(z) sums the absolute addends), so only |z| < 2 u E(z) can change side
KINK_IN = 4.0                    # the clamp's own threshold for that rule: its edge is 17 u from 1, so a sample at |u| >= 9 sits 8 units of E(tanh) outside it, and is outside in f32 too
JUMP = KINK / 2.0 ** -24         # ... and what the jump between its two branches then weighs in T: 64 / u, so that taking the other branch is inside every bound with c >= 1 / 64
HI32 = float(np.float32(1.0) - np.float32(1.0e-6))
N_STEPS = 3
LR = 3e-3
SEQUENCES = (("i1", 1, LR, N_STEPS), ("i2", 2, LR, N_STEPS), ("lr0", 1, 0.0, 1))          # (name, target_update_interval, learning rate, steps)

# the largest error / (u T) of the CPU oracle over the whole table, per block and per statistic (`python tests/sac_update_cases.py oracle`)
ORACLE_WORST = {                        # (rounded up to three digits)      reached at
    "g.actor.W1": 0.179,                # l1nopre.h516/B7/saturated.far/i1/step0
    "g.actor.b1": 0.187,                # l1nopre.h516/B7/saturated.far/i1/step0
    "g.actor.W2": 0.867,                # plain.d16a1/B7/saturated.far/lr0/step0
    "g.actor.b2": 0.571,                # fused.w4.h16x260/B255/saturated.far/i2/step2
    "g.actor.W3": 0.532,                # fused.w3.h20x24/B1/random/i1/step2
    "g.actor.b3": 0.368,                # plain.d40a6/B1/saturated.far/i1/step1
    "g.q0.W1": 0.309,                   # plain.d16a1/B1/edges.rew1e4/lr0/step0
    "g.q0.b1": 0.244,                   # mid.d4a1/B7/edges.rew1e4/i2/step2
    "g.q0.W2": 0.886,                   # plain.d16a1/B7/edges.dead_relu/i1/step0
    "g.q0.b2": 0.401,                   # fused.w4.h32/B7/saturated.far/i2/step2
    "g.q0.W3": 0.546,                   # fused.w4.h16x260/B255/random/i1/step2
    "g.q0.b3": 0.38,                    # fused.w4.h512/B1/indicator.j0/i1/step2
    "g.q1.W1": 0.349,                   # fused.w4.h20x24/B1/edges.rew1e4/i1/step0
    "g.q1.b1": 0.342,                   # fused.w4.h16x260/B1/edges.rew1e4/i2/step2
    "g.q1.W2": 0.836,                   # plain.d16a1/B7/edges.rew1e4/lr0/step0
    "g.q1.b2": 0.468,                   # fused.w4.h16x260/B255/random/i1/step2
    "g.q1.W3": 1.07,                    # fused.w4.h512/B1/indicator.j0/i1/step0
    "g.q1.b3": 0.463,                   # fused.w4.h512/B1/indicator.j0/i1/step0
    "g.log_std": 0.572,                 # plain.d40a6/B1/saturated.far/i1/step1
    "p.actor.W1": 0.947,                # mid.d11a5/B1/indicator.j0/i2/step2
    "p.actor.b1": 0.926,                # l1nopre.h516.fixed/B7/random/i1/step1
    "p.actor.W2": 0.977,                # plain.d16a1/B7/tie/i2/step2
    "p.actor.b2": 0.902,                # mid.d11a5/B255/indicator.j254/i1/step1
    "p.actor.W3": 0.867,                # fused.w4.h20x24/B7/indicator.j0/i2/step2
    "p.actor.b3": 0.88,                 # unfused.d11a5/B1/decision/i1/step1
    "p.q0.W1": 0.902,                   # fused.w4.h32/B257/indicator.j128/i1/step1
    "p.q0.b1": 0.846,                   # fused.w4.h512/B1/saturated.far/i2/step2
    "p.q0.W2": 0.935,                   # fused.w3.h32/B256/edges.rew1e4/i2/step2
    "p.q0.b2": 0.846,                   # fused.w4.h16x260/B255/indicator.j254/i1/step2
    "p.q0.W3": 0.874,                   # fused.w4.h20x24/B1/edges.alpha_small/i2/step2
    "p.q0.b3": 0.762,                   # fused.w4.h32/B255/random/i2/step2
    "p.q1.W1": 0.913,                   # mid.d4a1/B257/edges.alpha_large/i1/step2
    "p.q1.b1": 0.877,                   # plain.d1a16/B1/edges.rew1e4/i2/step2
    "p.q1.W2": 0.925,                   # fused.w4.h32/B1/edges.gamma0tau1/i1/step1
    "p.q1.b2": 0.824,                   # mid.d4a1/B7/indicator.j6/i2/step2
    "p.q1.W3": 0.874,                   # fused.w4.h32/B7/indicator.j3/i1/step2
    "p.q1.b3": 0.685,                   # fused.w4.h32/B7/indicator.j0/i1/step2
    "p.log_std": 0.961,                 # unfused.d11a5/B257/indicator.j128/i1/step2
    "t.q0.W1": 0.711,                   # fused.w4.h32/B64/random/i1/step1
    "t.q0.b1": 0.678,                   # fused.w3.h20x24/B64/saturated.edge/i1/step1
    "t.q0.W2": 0.716,                   # fused.w4.h512/B1/saturated.edge/i1/step1
    "t.q0.b2": 0.683,                   # fused.w4.h16x260/B255/edges.dead_relu/i1/step2
    "t.q0.W3": 0.671,                   # unfused.w4.fixed/B1/decision/i2/step2
    "t.q0.b3": 0.659,                   # plain.d1a16/B7/edges.rew1e4/i1/step1
    "t.q1.W1": 0.689,                   # mid.d11a5/B1/edges.alpha_small/i1/step2
    "t.q1.b1": 0.683,                   # fused.w4.h32/B64/random/i2/step2
    "t.q1.W2": 0.72,                    # fused.w4.h16x260/B255/indicator.j0/i2/step2
    "t.q1.b2": 0.695,                   # unfused.w4.fixed/B7/edges.rew1e4/i1/step0
    "t.q1.W3": 0.672,                   # fused.w3.h32/B7/random/i1/step2
    "t.q1.b3": 0.659,                   # fused.w3.h32/B1/indicator.j0/lr0/step0
    "critic_loss": 0.404,               # fused.w4.h512/B1/indicator.j0/i1/step1
    "actor_loss": 0.207,                # nodw1.w4.h20x24/B1/saturated.edge/i2/step2
    "entropy_loss": 0.207,              # fused.w4.h20x24/B1/saturated.edge/i1/step2
    "mean_q_values": 0.566,             # fused.w4.h16x260/B1/decision/i1/step2
    "entropy_coefficient": 0.797,       # fused.w4.h32.fixed/B1/random/i1/step0
    "grad_norm": 0.991,                 # fused.w4.h32/B1/edges.rew1e4/lr0/step0
    "log_ent_coef": 0.859,              # mid.d4a1/B1/edges.alpha_large/i1/step0
}
MARGIN = 4.0
CONSTANTS = {k: MARGIN * v for k, v in ORACLE_WORST.items()}


# =====================================================================================================================
# rows
# =====================================================================================================================
@dataclass(frozen=True)
class Row:
    name: str
    D: int
    A: int
    hidden: tuple
    act: str                      # relu | tanh
    ent: str                      # auto | fixed
    sizes: tuple
    gather: str                   # what dril_sac_update_info must report: l1 | plain
    head: str                     # fused,pre | fused,nopre | unfused
    dw1: str                      # fused | launch
    switches: tuple = ()          # DRIL_SAC_NO_* set around the creation of the handle (latched there)
    families: tuple = ("random", "indicator", "saturated", "decision", "tie", "edges")

    @property
    def W(self):
        return self.D + self.A

    @property
    def route(self):
        return f"gather={self.gather} head={self.head} dw1={self.dw1}"

    @property
    def env(self):
        return {k: "1" for k in self.switches}


def _rows():
    R = []
    fused = dict(gather="l1", head="fused,pre", dw1="fused")
    R.append(Row("fused.w4.h32", 3, 1, (32, 32), "relu", "auto", (1, 7, 64, 255, 256, 257), **fused))                  # the benchmark's route
    R.append(Row("fused.w4.h32.fixed", 3, 1, (32, 32), "tanh", "fixed", (1, 257), **fused))
    R.append(Row("fused.w3.h32", 2, 1, (32, 32), "tanh", "auto", (1, 7, 256), **fused))
    R.append(Row("fused.w4.h16x260", 3, 1, (16, 260), "relu", "auto", (1, 255), **fused))                             # one first_layer_opt_block exactly full; wave_dot loops twice
    R.append(Row("fused.w4.h20x24", 3, 1, (20, 24), "tanh", "auto", (1, 7, 257), **fused))                           # a ragged second unit block (H1 = 16 + 4)
    R.append(Row("fused.w3.h20x24", 2, 1, (20, 24), "relu", "fixed", (1, 64), **fused))
    R.append(Row("fused.w4.h512", 3, 1, (512, 512), "relu", "auto", (1, 256), families=("random", "indicator", "saturated"), **fused))     # B = 256: the benchmark's shape, once
    R.append(Row("fused.w4.h512.tanh", 3, 1, (512, 512), "tanh", "fixed", (1, 256), families=("random",), **fused))                                       # ... and once with tanh, which has no kink
    R.append(Row("fused.w4.h32.b1024", 3, 1, (32, 32), "relu", "auto", (1, 1024), families=("random", "indicator", "saturated"), **fused))   # the last batch size of the fused dW1
    nodw1 = dict(gather="l1", head="fused,pre", dw1="launch")
    R.append(Row("nodw1.w4.h32", 3, 1, (32, 32), "relu", "auto", (1, 7, 257), switches=("DRIL_SAC_NO_FUSED_DW1",), **nodw1))
    R.append(Row("nodw1.w4.h20x24", 3, 1, (20, 24), "tanh", "fixed", (1, 255), switches=("DRIL_SAC_NO_FUSED_DW1",), **nodw1))
    R.append(Row("b1028.w4.h32", 3, 1, (32, 32), "relu", "auto", (1028,), **nodw1))                                               # fused dW1 off by batch size
    R.append(Row("b1028.w4.h32.fixed", 3, 1, (32, 32), "tanh", "fixed", (1028,), families=("random", "saturated"), **nodw1))
    nopre = dict(gather="l1", head="fused,nopre", dw1="fused")
    R.append(Row("l1nopre.h516", 3, 1, (516, 32), "relu", "auto", (1, 7, 64), families=("random", "indicator", "saturated", "decision"), **nopre))   # H1 above 512: first_l1 in the <false> head
    R.append(Row("l1nopre.h516.fixed", 3, 1, (516, 32), "tanh", "fixed", (1, 7), families=("random", "saturated"), **nopre))
    mid = dict(gather="l1", head="fused,nopre", dw1="launch")                                                        # 5 <= W <= 16
    R.append(Row("mid.d4a1", 4, 1, (32, 32), "relu", "auto", (1, 7, 257), **mid))
    R.append(Row("mid.d11a5", 11, 5, (24, 40), "tanh", "auto", (1, 64, 255), **mid))
    R.append(Row("mid.d8a8", 8, 8, (32, 32), "relu", "fixed", (1, 7, 256), **mid))                                   # 2 A = 16 pairs on four waves
    plain = dict(gather="plain", head="fused,nopre", dw1="launch")                                                   # W >= 17: contraction first layers
    R.append(Row("plain.d16a1", 16, 1, (32, 32), "relu", "auto", (1, 7, 257), **plain))
    R.append(Row("plain.d1a16", 1, 16, (32, 32), "tanh", "fixed", (1, 7, 64), **plain))                              # A = kMaxA
    R.append(Row("plain.d40a6", 40, 6, (24, 40), "relu", "auto", (1, 255), **plain))
    unf = dict(head="unfused", dw1="launch", switches=("DRIL_SAC_NO_FUSED_HEADS",))                                   # the four unfused kernels (and the plain gather: l1 needs fused heads)
    R.append(Row("unfused.w4", 3, 1, (32, 32), "relu", "auto", (1, 7, 257), gather="plain", **unf))
    R.append(Row("unfused.w4.fixed", 3, 1, (32, 32), "tanh", "fixed", (1, 7), gather="plain", **unf))
    R.append(Row("unfused.d11a5", 11, 5, (24, 40), "tanh", "auto", (1, 7, 257), gather="plain", **unf))
    return R


ROWS = _rows()
ROW_BY_NAME = {r.name: r for r in ROWS}
assert len(ROW_BY_NAME) == len(ROWS)


@dataclass(frozen=True)
class Case:
    row: Row
    B: int
    family: str
    tag: str = ""

    @property
    def name(self):
        return f"{self.row.name}/B{self.B}/{self.family}{'.' + self.tag if self.tag else ''}"

    @property
    def sequences(self):
        """all three — the step at learning_rate = 0 alone at 512 x 512 relu units x 256 samples: some ten of those rows come within 3 units of a relu kink of the actor stage's
        critics, WHICH ten follows the critic step of the whole batch, and no redraw of rows settles that (the shape's stepping sequences run at B = 1, and at B = 256 with tanh)"""
        return SEQUENCES[2:] if max(self.row.hidden) >= 512 and self.B >= 64 and self.row.act == "relu" else SEQUENCES

    @property
    def checked(self):
        """the decisions whose margin is a condition on this case's inputs.  saturated/edge has none: its `inside` flags may differ between implementations, the actor
        gradients and so the trajectories with them, and no condition on a later step can be set from the inputs"""
        return () if (self.family, self.tag) == ("saturated", "edge") else CHECKED_MARGINS[self.family]

    @property
    def setting(self):
        """(gamma, tau) of the handle: the config is latched at creation"""
        return (0.0, 1.0) if self.tag == "gamma0tau1" else (0.99, 0.05)


def indicator_slots(B):
    """first, last, middle, and 255 / 256 where the batch has them"""
    return sorted({0, B - 1, B // 2} | {j for j in (255, 256) if j < B})


def cases_of(row):
    out = []
    for B in row.sizes:
        wide_big = max(row.hidden) >= 512 and B >= 64                                # (a float64 pass at 512 x 512 x 256 takes a third of a second)
        full = B in (1, 7, max(row.sizes))                                           # every family at the smallest two and the largest batch, the sample positions at all
        for fam in (("random",) if wide_big else row.families if full else tuple(f for f in row.families if f in ("random", "indicator"))):
            if fam == "indicator":
                slots = indicator_slots(B)
                out += [Case(row, B, fam, f"j{j}") for j in (slots if B <= 257 and max(row.hidden) < 512 else slots[:2])]
            elif fam == "edges":
                out += [Case(row, B, fam, t) for t in ("alpha_small", "alpha_large", "gamma0tau1", "rew1e4") + (("dead_relu",) if row.act == "relu" else ())]
            else:
                out += [Case(row, B, fam, t) for t in ("edge", "far")] if fam == "saturated" else [Case(row, B, fam)]
    return out


# =====================================================================================================================
# the parameter vector (include/dril_sac.h): {W1 b1 W2 b2 W3 b3} of the actor, of critic 0, of critic 1, log_std; W (out x in) column-major
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def layout(D, A, H1, H2):
    sl, off = {}, 0
    for net, inp, O in (("actor", D, A), ("q0", D + A, 1), ("q1", D + A, 1)):
        for (i, o), (w, b) in zip(((inp, H1), (H1, H2), (H2, O)), (("W1", "b1"), ("W2", "b2"), ("W3", "b3"))):
            sl[f"{net}.{w}"] = (off, off + o * i, (i, o)); off += o * i
            sl[f"{net}.{b}"] = (off, off + o, None); off += o
    sl["log_std"] = (off, off + A, None)
    return sl, off + A


def _get(flat, sl, k):
    lo, hi, sh = sl[k]
    return flat[lo:hi].reshape(sh).T if sh else flat[lo:hi]


def _net(flat, sl, net):
    return tuple(_get(flat, sl, f"{net}.{b}") for b in NET_BLOCKS)


def _put(vec, sl, k, a):
    lo, hi, sh = sl[k]
    vec[lo:hi] = a.T.ravel() if sh else np.ravel(a)


def row_layout(row):
    return layout(row.D, row.A, *row.hidden)


def critic_range(row):
    sl, _ = row_layout(row)
    return sl["q0.W1"][0], sl["q1.b3"][1]


# =====================================================================================================================
# float64 forward / reverse passes with their scales
# =====================================================================================================================
def _tanh_own(h):
    """the SAC kernels and the contractions' epilogue call tanhf (dril_sac_update.hip, dril_sac_net.hip, include/device/dril_activations.h), 2 ulp of the result — not the exp2 / rcp form of the PPO
    kernels, whose scale grad_cases._tanh_own is 3 (1 - h) + |h|"""
    return 2 * np.abs(h)


def _f(z, act):
    return np.tanh(z) if act == "tanh" else np.maximum(z, 0.0)


def _fwd(net, x, act):
    W1, b1, W2, b2, W3, b3 = net
    z1 = x @ W1.T + b1; h1 = _f(z1, act)
    z2 = h1 @ W2.T + b2; h2 = _f(z2, act)
    return dict(z1=z1, h1=h1, z2=z2, h2=h2, out=h2 @ W3.T + b3)


def _d(h, z, act):
    return 1 - h * h if act == "tanh" else (z > 0).astype(np.float64)


def _fscale(net, enet, x, ex, fw, act):
    """E of h1, h2, out and of the two derivatives (|f'| + its error), given E(x) = ex and E(parameters) = enet (None: exact)"""
    aW1, ab1, aW2, ab2, aW3, ab3 = (np.abs(t) for t in net)
    eW1, eb1, eW2, eb2, eW3, eb3 = enet if enet is not None else (0.0 * aW1, 0.0, 0.0 * aW2, 0.0, 0.0 * aW3, 0.0)
    ax, a1, a2 = np.abs(x), np.abs(fw["h1"]), np.abs(fw["h2"])
    res = {}
    ez = (ex + ax) @ aW1.T + ax @ eW1.T + ab1 + eb1
    for l, (h, z, nxt) in enumerate(((fw["h1"], fw["z1"], (aW2, eW2, ab2, eb2)), (fw["h2"], fw["z2"], (aW3, eW3, ab3, eb3))), 1):
        d = np.abs(_d(h, z, act))
        if act == "tanh":
            e = d * ez + _tanh_own(h)
            t = d + 2 * np.abs(h) * e
        else:
            e = d * ez
            with np.errstate(divide="ignore", invalid="ignore"):
                km = np.where(ez > 0, np.abs(z) / (U * ez), np.inf)
            kink = km < KINK_RELU
            t = d + kink * JUMP
            res[f"kink{l}"] = int(kink.sum())
            res["kmin"] = np.minimum(res.get("kmin", np.inf), km.min(axis=1))
        res[f"h{l}"], res[f"t{l}"] = e, t
        aW, eW, ab, eb = nxt
        ez = (e + np.abs(h)) @ aW.T + np.abs(h) @ eW.T + ab + eb
    res["out"] = ez
    return res


def _bwd(net, x, fw, dout, act, params=True):
    W1, b1, W2, b2, W3, b3 = net
    dz2 = (dout @ W3) * _d(fw["h2"], fw["z2"], act)
    dz1 = (dz2 @ W2) * _d(fw["h1"], fw["z1"], act)
    g = {"W1": dz1.T @ x, "b1": dz1.sum(axis=0), "W2": dz2.T @ fw["h1"], "b2": dz2.sum(axis=0), "W3": dout.T @ fw["h2"], "b3": dout.sum(axis=0)} if params else {}
    g["dx"] = dz1 @ W1
    return g


def _bscale(net, enet, x, ex, fw, fs, dout, e_dout, act):
    """E of every gradient block and of dx, from the head signal (dout, E(dout)) and the forward scales fs"""
    W1, b1, W2, b2, W3, b3 = net
    aW1, aW2, aW3 = np.abs(W1), np.abs(W2), np.abs(W3)
    eW1, _, eW2, _, eW3, _ = enet if enet is not None else (0.0 * aW1, 0.0, 0.0 * aW2, 0.0, 0.0 * aW3, 0.0)
    d2, d1 = _d(fw["h2"], fw["z2"], act), _d(fw["h1"], fw["z1"], act)
    a_dout = np.abs(dout)
    dh2 = dout @ W3
    e_dh2 = (e_dout + a_dout) @ aW3 + a_dout @ eW3
    dz2 = dh2 * d2; a_dz2 = np.abs(dz2)
    e_dz2 = np.abs(dh2) * fs["t2"] + np.abs(d2) * e_dh2 + a_dz2
    dh1 = dz2 @ W2
    e_dh1 = (e_dz2 + a_dz2) @ aW2 + a_dz2 @ eW2
    dz1 = dh1 * d1; a_dz1 = np.abs(dz1)
    e_dz1 = np.abs(dh1) * fs["t1"] + np.abs(d1) * e_dh1 + a_dz1
    ax, a1, a2 = np.abs(x), np.abs(fw["h1"]), np.abs(fw["h2"])
    return {"W1": (e_dz1 + a_dz1).T @ ax + a_dz1.T @ (ex + 0 * ax), "b1": (e_dz1 + a_dz1).sum(axis=0), "W2": e_dz2.T @ a1 + a_dz2.T @ (fs["h1"] + a1),
            "b2": (e_dz2 + a_dz2).sum(axis=0), "W3": e_dout.T @ a2 + a_dout.T @ (fs["h2"] + a2), "b3": (e_dout + a_dout).sum(axis=0),
            "dx": (e_dz1 + a_dz1) @ aW1 + a_dz1 @ eW1}


LOG2, LOG2PI = math.log(2.0), math.log(2 * math.pi)


def _softplus(x):
    return np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0.0)


def _alp(mu, e_mu, ls, noise, hi, defect=None):
    """rand + logpdf of the squashed Gaussian (squashedDiagGaussian.jl:24-46) with the scale of every quantity the reverse pass reads"""
    A = mu.shape[1]
    sig, e2 = np.exp(ls), np.exp(-2 * ls)
    e_sig, e_e2 = sig * (np.abs(ls) + 1), e2 * (2 * np.abs(ls) + 1)
    u = mu + sig * noise
    e_u = e_mu + e_sig * np.abs(noise) + np.abs(sig * noise) + np.abs(u)
    a = np.tanh(u)
    e_a = (1 - a * a) * e_u + _tanh_own(a)
    inside = (a >= -hi) & (a <= hi)
    in_margin = np.abs(np.abs(a) - hi) / (U * e_a)
    xc = np.clip(a, -hi, hi)
    e_xc = np.where(inside | (in_margin < KINK_IN), e_a, 0.0)                           # (the clamp's value is continuous: a sample at the edge carries E(a) on either side)
    g = np.arctanh(xc)
    e_g = e_xc / (1 - xc * xc) + np.abs(g)
    d = g - mu
    e_d = e_g + e_mu + np.abs(d)
    q = d * d * e2
    e_q = 2 * np.abs(d) * e2 * e_d + d * d * e_e2 + q
    glp = -0.5 * (2 * ls.sum() + q.sum(axis=1) + A * LOG2PI)
    e_glp = 0.5 * e_q.sum(axis=1) + np.abs(ls).sum() + 0.5 * q.sum(axis=1) + 0.5 * A * LOG2PI
    sp = _softplus(-2 * g)
    e_sp = 2 * e_g / (1 + np.exp(2 * g)) + sp
    corr = 2 * (LOG2 - g - sp)
    e_corr = 2 * (e_g + e_sp + LOG2 + np.abs(g) + sp)
    lp = glp - corr.sum(axis=1)
    e_lp = e_glp + e_corr.sum(axis=1) + np.abs(lp)
    return dict(a=a, e_a=e_a, g=g, e_g=e_g, d=d, e_d=e_d, q=q, e_q=e_q, lp=lp, e_lp=e_lp, inside=inside, in_margin=in_margin, sig=sig, e_sig=e_sig, e2=e2, e_e2=e_e2, xc=xc)


@functools.lru_cache(maxsize=None)
def _bt(b, t, f32):
    """beta^t as the implementations hold it: a running f32 product on the host, one multiplication per tick (f32 = False: the exact power, for the autograd pin)"""
    if not f32:
        return b ** t
    r = x = np.float32(b)
    for _ in range(t - 1):
        r = np.float32(r * x)
    return float(r)


def _adam(m, v, em, ev, g, eg, t, hp, eps=None):
    """one Adam step in float64 with the scales of the module docstring -> (m, v, E(m), E(v), step, E(step))"""
    b1, b2, lr = hp["b1"], hp["b2"], hp["lr"]
    eps = hp["eps"] if eps is None else eps
    m2 = b1 * m + (1 - b1) * g
    em2 = b1 * (em + np.abs(m)) + (1 - b1) * (eg + np.abs(g)) + np.abs(m2)
    v2 = b2 * v + (1 - b2) * g * g
    ev2 = b2 * (ev + v) + (1 - b2) * (2 * np.abs(g) * eg + 2 * g * g) + v2
    c1, c2 = 1 - _bt(b1, t, hp["f32_bt"]), 1 - _bt(b2, t, hp["f32_bt"])
    ec1, ec2 = c1, c2                                                                # (the subtraction; the running product itself is reproduced, not bounded)
    mh, vh = m2 / c1, v2 / c2
    emh, evh = em2 / c1 + np.abs(m2) * ec1 / c1 ** 2 + np.abs(mh), ev2 / c2 + v2 * ec2 / c2 ** 2 + vh
    s = np.sqrt(vh)
    with np.errstate(divide="ignore", invalid="ignore"):
        es = np.where(vh > 0, evh / (2 * s), 0.0) + s
    den = s + eps
    S = lr * mh / den
    eS = lr * (emh / den + np.abs(mh) * (es + den) / den ** 2) + 2 * np.abs(S)
    return m2, v2, em2, ev2, S, eS


class Tracker:
    """the optimiser state nobody can read back: float64 moments (and their scales) built from the REPORTED gradients, the three step counters, grad_updates"""

    def __init__(self, P):
        self.m, self.v, self.em, self.ev = (np.zeros(P) for _ in range(4))
        self.t_actor = self.t_critic = self.t_ent = self.n = 0
        self.ent = [0.0, 0.0, 0.0, 0.0]


@dataclass
class StepRef:
    gc: np.ndarray
    ga: np.ndarray
    Tgc: np.ndarray
    Tga: np.ndarray
    params: np.ndarray
    Tparams: np.ndarray
    target: np.ndarray
    Ttarget: np.ndarray
    polyak: bool
    stats: dict
    statT: dict
    margins: dict                 # smallest margin, in forward-error units, of: tmin (target's twin min), amin (actor loss's), inside (the clamp), relu kinks counted
    decisions: dict = field(repr=False, default=None)


DEFECTS = ("alpha_before_entropy_step", "online_critics_in_target", "terminated_ignored", "min_is_mean", "min_is_critic0", "tie_to_critic1", "inside_always_1",
           "one_minus_x2_dropped", "two_tanh_dropped", "sigma_noise_missing", "actor_stage_old_critics", "zero_grad_adam_skipped", "critic_bias_once_per_update",
           "adam_eps_1e-5", "polyak_one_update_late", "polyak_before_second_critic_step", "mean_over_first_256")


def hyper(cfg, A, hi=HI32):
    """the f32 values of the config, as float64 (AutoEntropyTarget: -dim(action_space), sac.jl:47-57)"""
    return dict(lr=float(cfg.learning_rate), b1=float(cfg.adam_beta1), b2=float(cfg.adam_beta2), eps=float(cfg.adam_eps), tau=float(cfg.tau), gamma=float(cfg.gamma),
                interval=int(cfg.target_update_interval), auto=bool(cfg.auto_ent_coef), target_entropy=-float(A) if cfg.auto_target_entropy else float(cfg.target_entropy), hi=hi, f32_bt=True)


def ref_step(row, hp, before, batch, noises, tr, reported=None, log_ent_after=None, defect=None, own_scale=False):
    """one update! in float64 from `before` = (params, targets, log_ent_coef) -> StepRef; advances the Tracker `tr`.  reported: the (critic, actor) gradients the
    implementation under test reported for this step (None: the reference's own); log_ent_after: its log_ent_coef after the step (None: the reference's own);
    defect: one of DEFECTS, the float64 result an implementation with that defect would give; own_scale (with reported = None): the scale of the parameters carries the
    gradient's own, through Adam's conditioning — what the pin against autograd compares within"""
    D, A, act = row.D, row.A, row.act
    sl, P = row_layout(row)
    p0, tg0, le0 = np.asarray(before[0], np.float64), np.asarray(before[1], np.float64), float(before[2])
    obs, actn, rew, term, nobs = (np.asarray(t, np.float64) for t in batch)
    term = term.astype(bool)
    ne, nn, npi = (np.asarray(t, np.float64) for t in noises)
    n = len(rew)
    w = (np.arange(n) < 256).astype(np.float64) if defect == "mean_over_first_256" else np.ones(n)
    hi, gamma, tau = hp["hi"], hp["gamma"], hp["tau"]
    c0, c1_ = critic_range(row)
    Pq = (c1_ - c0) // 2
    actor, ls = _net(p0, sl, "actor"), _get(p0, sl, "log_std")
    stats, statT, margins = {}, {}, {}
    # ---- the actor's means of obs and next obs (the actor does not move until its own step)
    fa, fan = _fwd(actor, obs, act), _fwd(actor, nobs, act)
    sa, san = _fscale(actor, None, obs, 0.0, fa, act), _fscale(actor, None, nobs, 0.0, fan, act)
    kinks = sa.get("kink1", 0) + sa.get("kink2", 0)
    kmin = sa.get("kmin", np.full(n, np.inf))                                        # per sample: the nearest relu kink of the passes that are differentiated
    # ---- 1. entropy coefficient :313-343
    le1, e_le1 = le0, 0.0
    if hp["auto"]:
        pe = _alp(fa["out"], sa["out"], ls, ne, hi)
        c = ((pe["lp"] + hp["target_entropy"]) * w).sum() / n
        e_c = ((pe["e_lp"] + np.abs(pe["lp"] + hp["target_entropy"])) * w).sum() / n + abs(c)
        stats["entropy_loss"], statT["entropy_loss"] = -le0 * c, abs(le0) * e_c + abs(le0 * c)
        tr.t_ent += 1
        m, v, em, ev, S, eS = _adam(tr.ent[0], tr.ent[1], tr.ent[2], tr.ent[3], -c, e_c, tr.t_ent, hp, 1e-5 if defect == "adam_eps_1e-5" else None)
        tr.ent = [float(m), float(v), float(em), float(ev)]
        le1, e_le1 = le0 - float(S), float(eS) + abs(le0 - float(S))
    stats["log_ent_coef"], statT["log_ent_coef"] = le1, max(e_le1, abs(le1))
    le_used, e_le_used = (le1, e_le1) if log_ent_after is None else (float(log_ent_after), 0.0)
    alpha = math.exp(le_used)
    e_alpha = alpha * (e_le_used + 1)
    stats["entropy_coefficient"], statT["entropy_coefficient"] = alpha, e_alpha
    alpha_t, e_alpha_t = (math.exp(le0), math.exp(le0)) if defect == "alpha_before_entropy_step" else (alpha, e_alpha)
    # ---- 2. critic loss :107-150 with the target networks
    pn = _alp(fan["out"], san["out"], ls, nn, hi)
    xn, exn = np.concatenate([nobs, pn["a"]], 1), np.concatenate([0 * nobs, pn["e_a"]], 1)
    tflat = np.zeros(P); tflat[c0:c1_] = p0[c0:c1_] if defect == "online_critics_in_target" else tg0
    qn, e_qn = [], []
    for k in ("q0", "q1"):
        net = _net(tflat, sl, k)
        fw = _fwd(net, xn, act)
        fs = _fscale(net, None, xn, exn, fw, act)
        qn.append(fw["out"][:, 0]); e_qn.append(fs["out"][:, 0])
    kt = qn[1] < qn[0]
    mn, e_mn = np.where(kt, qn[1], qn[0]), np.where(kt, e_qn[1], e_qn[0])
    if defect == "min_is_mean":
        mn = 0.5 * (qn[0] + qn[1])
    elif defect == "min_is_critic0":
        mn = qn[0]
    live = np.ones(n, bool) if defect == "terminated_ignored" else ~term
    read = live & (gamma != 0.0)                                                     # (gamma = 0: the soft value is multiplied away)
    with np.errstate(divide="ignore", invalid="ignore"):
        tm = np.abs(qn[0] - qn[1]) / (U * (e_qn[0] + e_qn[1]))
    tie_t = qn[0] == qn[1]
    near_t = read & ~tie_t & (tm < KINK)
    e_mn = e_mn + near_t * np.abs(qn[0] - qn[1]) * JUMP
    per_sample = {"tmin": np.where(read & ~tie_t, tm, np.inf)}
    margins["tmin"] = float(per_sample["tmin"].min())
    soft = mn - alpha_t * pn["lp"]
    e_soft = e_mn + alpha_t * pn["e_lp"] + e_alpha_t * np.abs(pn["lp"]) + np.abs(alpha_t * pn["lp"]) + np.abs(soft)
    y = rew + np.where(live, gamma * soft, 0.0)
    e_y = np.where(live, gamma * e_soft + np.abs(gamma * soft), 0.0) + np.abs(y)
    xq = np.concatenate([obs, actn], 1)
    gc, Tgc = np.zeros(P), np.zeros(P)
    closs = closs_T = qsum = qsum_T = 0.0
    for k in ("q0", "q1"):
        net = _net(p0, sl, k)
        fw = _fwd(net, xq, act)
        fs = _fscale(net, None, xq, 0.0, fw, act)
        kinks += fs.get("kink1", 0) + fs.get("kink2", 0)
        kmin = np.minimum(kmin, fs.get("kmin", np.inf))
        q, e_q = fw["out"][:, 0], fs["out"][:, 0]
        d = q - y
        e_d = e_q + e_y + np.abs(d)
        closs += 0.5 * (d * d * w).sum() / n; closs_T += 0.5 * ((2 * np.abs(d) * e_d + 2 * d * d) * w).sum() / n
        qsum += (q * w).sum() / (2 * n); qsum_T += ((e_q + np.abs(q)) * w).sum() / (2 * n)
        dout, e_dout = (d * w / n)[:, None], ((e_d / n + np.abs(d) / n) * w)[:, None]
        gb, tb = _bwd(net, xq, fw, dout, act), _bscale(net, None, xq, 0.0, fw, fs, dout, e_dout, act)
        for b in NET_BLOCKS:
            _put(gc, sl, f"{k}.{b}", gb[b]); _put(Tgc, sl, f"{k}.{b}", tb[b])
    stats["critic_loss"], statT["critic_loss"] = closs, closs_T
    stats["mean_q_values"], statT["mean_q_values"] = qsum, qsum_T + abs(qsum)
    # ---- critic Adam :362 from the reported gradient
    g_c = gc if reported is None else np.asarray(reported[0], np.float64)
    eps_ = 1e-5 if defect == "adam_eps_1e-5" else None
    tc1 = tr.t_critic + 1 if defect != "critic_bias_once_per_update" else tr.n + 1
    cs = slice(c0, c1_)
    own = own_scale and reported is None
    eS1_own = _adam(tr.m[cs], tr.v[cs], tr.em[cs], tr.ev[cs], g_c[cs], Tgc[cs], tc1, hp, eps_)[5] if own else 0.0
    m, v, em, ev, S1, eS1 = _adam(tr.m[cs], tr.v[cs], tr.em[cs], tr.ev[cs], g_c[cs], 0.0, tc1, hp, eps_)
    tr.m[cs], tr.v[cs], tr.em[cs], tr.ev[cs] = m, v, em, ev
    tr.t_critic += 1
    p1 = p0.copy(); p1[cs] -= S1
    eP1 = np.zeros(P)
    if hp["lr"] != 0.0:
        eP1[cs] = np.abs(p1[cs]) + eS1
    # ---- 3. actor loss :93-105 with the updated critics
    pp = _alp(fa["out"], sa["out"], ls, npi, hi)
    xp, exp_ = np.concatenate([obs, pp["a"]], 1), np.concatenate([0 * obs, pp["e_a"]], 1)
    pq = p0 if defect == "actor_stage_old_critics" else p1
    qp, e_qp, dxs, e_dxs = [], [], [], []
    dq = np.full((n, 1), -1.0 / n) * w[:, None]
    for k in ("q0", "q1"):
        net, enet = _net(pq, sl, k), _net(eP1, sl, k)
        fw = _fwd(net, xp, act)
        fs = _fscale(net, enet, xp, exp_, fw, act)
        kinks += fs.get("kink1", 0) + fs.get("kink2", 0)
        kmin = np.minimum(kmin, fs.get("kmin", np.inf))
        qp.append(fw["out"][:, 0]); e_qp.append(fs["out"][:, 0])
        dxs.append(_bwd(net, xp, fw, dq, act, params=False)["dx"][:, D:])
        e_dxs.append(_bscale(net, enet, xp, exp_, fw, fs, dq, 0.0 * dq, act)["dx"][:, D:])
    km = qp[1] < qp[0]                                                               # a tie goes to critic 0 (oracle/dril_sac_oracle.c:438)
    if defect == "tie_to_critic1":
        km = qp[1] <= qp[0]
    if defect == "min_is_critic0":
        km = np.zeros(n, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        am = np.abs(qp[0] - qp[1]) / (U * (e_qp[0] + e_qp[1]))
    tie_a = qp[0] == qp[1]
    near_a = ~tie_a & (am < KINK)
    per_sample["amin"] = np.where(~tie_a, am, np.inf)
    margins["amin"] = float(per_sample["amin"].min())
    qmin, e_qmin = np.where(km, qp[1], qp[0]), np.where(km, e_qp[1], e_qp[0]) + near_a * np.abs(qp[0] - qp[1]) * JUMP
    da, e_da = np.where(km[:, None], dxs[1], dxs[0]), np.where(km[:, None], e_dxs[1], e_dxs[0]) + near_a[:, None] * np.abs(dxs[0] - dxs[1]) * JUMP
    if defect == "min_is_mean":
        qmin, da = 0.5 * (qp[0] + qp[1]), 0.5 * (dxs[0] + dxs[1])
    aloss = ((alpha * pp["lp"] - qmin) * w).sum() / n
    stats["actor_loss"] = aloss
    statT["actor_loss"] = ((alpha * pp["e_lp"] + e_alpha * np.abs(pp["lp"]) + np.abs(alpha * pp["lp"]) + e_qmin + np.abs(qmin)) * w).sum() / n + abs(aloss)
    # the reverse of the squashed sample (Zygote through tanh -> clamp -> atanh -> logpdf; oracle/dril_sac_oracle.c:102-113)
    a, g, dd, e2, sig = pp["a"], pp["g"], pp["d"], pp["e2"], pp["sig"]
    inside = np.ones_like(a) if defect == "inside_always_1" else pp["inside"].astype(np.float64)
    per_sample["inside"] = np.minimum(pp["in_margin"].min(axis=1), np.where(read, pn["in_margin"].min(axis=1), np.inf))
    if hp["auto"]:
        per_sample["inside"] = np.minimum(per_sample["inside"], pe["in_margin"].min(axis=1))
    margins["inside"] = float(per_sample["inside"].min())
    per_sample["relu"] = kmin
    margins["relu"] = float(kmin.min())
    jumps = int(kinks + near_t.sum() + near_a.sum() + (pp["in_margin"] < KINK_IN).sum())     # how many decisions put their jump into T
    dlogp, e_dlogp = alpha / n * w[:, None], (e_alpha / n + alpha / n) * w[:, None]
    th = np.tanh(g)
    dlp_dg = -dd * e2 + (0.0 if defect == "two_tanh_dropped" else 2 * th)
    e_dlp = pp["e_d"] * e2 + np.abs(dd) * pp["e_e2"] + np.abs(dd * e2) + 2 * ((1 - th * th) * pp["e_g"] + np.abs(th))
    t1 = dlogp * dlp_dg * inside
    e_t1 = inside * (e_dlogp * np.abs(dlp_dg) + dlogp * e_dlp + np.abs(t1)) + (pp["in_margin"] < KINK_IN) * np.abs(dlogp * dlp_dg) * JUMP
    om = 1.0 if defect == "one_minus_x2_dropped" else 1 - a * a
    t2 = da * om
    e_t2 = e_da * (1 - a * a) + np.abs(da) * (2 * np.abs(a) * pp["e_a"] + (1 - a * a)) + np.abs(t2)
    du, e_du = t1 + t2, e_t1 + e_t2 + np.abs(t1) + np.abs(t2)
    t3 = dlogp * dd * e2
    e_t3 = e_dlogp * np.abs(dd * e2) + dlogp * (pp["e_d"] * e2 + np.abs(dd) * pp["e_e2"]) + np.abs(t3)
    dmu, e_dmu = t3 + du, e_t3 + e_du + np.abs(t3) + np.abs(du)
    t4 = dlogp * (pp["q"] - 1)
    e_t4 = e_dlogp * np.abs(pp["q"] - 1) + dlogp * (pp["e_q"] + pp["q"] + 1) + np.abs(t4)
    sz = np.ones_like(a) if defect == "sigma_noise_missing" else sig * npi
    t5 = du * sz
    e_t5 = e_du * np.abs(sig * npi) + np.abs(du) * pp["e_sig"] * np.abs(npi) + 2 * np.abs(t5)
    ga, Tga = np.zeros(P), np.zeros(P)
    _put(ga, sl, "log_std", (t4 + t5).sum(axis=0)); _put(Tga, sl, "log_std", (e_t4 + e_t5 + np.abs(t4) + np.abs(t5)).sum(axis=0))
    gb, tb = _bwd(actor, obs, fa, dmu, act), _bscale(actor, None, obs, 0.0, fa, sa, dmu, e_dmu, act)
    for b in NET_BLOCKS:
        _put(ga, sl, f"actor.{b}", gb[b]); _put(Tga, sl, f"actor.{b}", tb[b])
    # ---- actor + log_std Adam :382, the zero-gradient critic Adam (zero_critic_grads! :381)
    g_a = ga if reported is None else np.asarray(reported[1], np.float64)
    tr.t_actor += 1
    asl = np.r_[0:sl["actor.b3"][1], sl["log_std"][0]:sl["log_std"][1]]
    eSa_own = _adam(tr.m[asl], tr.v[asl], tr.em[asl], tr.ev[asl], g_a[asl], Tga[asl], tr.t_actor, hp, eps_)[5] if own else 0.0
    m, v, em, ev, Sa, eSa = _adam(tr.m[asl], tr.v[asl], tr.em[asl], tr.ev[asl], g_a[asl], 0.0, tr.t_actor, hp, eps_)
    tr.m[asl], tr.v[asl], tr.em[asl], tr.ev[asl] = m, v, em, ev
    p2, Tp = p1.copy(), np.abs(p0)
    p2[asl] -= Sa
    Tp[asl] = eSa + eSa_own + np.abs(p2[asl])
    if defect == "zero_grad_adam_skipped":
        Tp[cs] = eS1 + np.abs(p1[cs])
    else:
        tc2 = tr.t_critic + 1 if defect != "critic_bias_once_per_update" else tr.n + 1
        m, v, em, ev, S2, eS2 = _adam(tr.m[cs], tr.v[cs], tr.em[cs], tr.ev[cs], 0.0 * g_c[cs], 0.0, tc2, hp, eps_)
        tr.m[cs], tr.v[cs], tr.em[cs], tr.ev[cs] = m, v, em, ev
        tr.t_critic += 1
        p2[cs] -= S2
        Tp[cs] = eS1 + eS1_own + eS2 + np.abs(p1[cs]) + np.abs(p2[cs])
    # ---- 4. polyak :385-389, gated by the count BEFORE the increment
    gate = tr.n % hp["interval"] == 0
    tr.n += 1
    stats["grad_norm"] = math.sqrt((g_c ** 2).sum() + (g_a ** 2).sum()) if reported is not None else math.sqrt((gc ** 2).sum() + (ga ** 2).sum())
    gn = stats["grad_norm"]
    statT["grad_norm"] = gn if reported is not None else ((np.abs(gc) * Tgc).sum() + (np.abs(ga) * Tga).sum()) / max(gn, TINY) + gn
    return StepRef(gc, ga, Tgc, Tga, p2, Tp, tg0, None, bool(gate), stats, statT, dict(margins, relu_kinks=kinks, jumps=jumps),
                   dict(kt=kt, km=km, inside=pp["inside"], p0=p0, p1=p1, tau=tau, c=(c0, c1_), tie_a=int(tie_a.sum()), tie_t=int((tie_t & live).sum()), per_sample=per_sample))


def expected_target(ref, params_after, defect=None):
    """the float64 polyak of the implementation's OWN parameters after the step, and its scale"""
    c0, c1_ = ref.decisions["c"]
    tau, tg0 = ref.decisions["tau"], ref.target
    if not ref.polyak:
        return tg0.copy(), np.abs(tg0), False
    src = {"polyak_one_update_late": ref.decisions["p0"], "polyak_before_second_critic_step": ref.decisions["p1"]}.get(defect)
    src = np.asarray(params_after, np.float64)[c0:c1_] if src is None else src[c0:c1_]
    t = tau * src + (1 - tau) * tg0
    return t, tau * np.abs(src) + 2 * (1 - tau) * np.abs(tg0) + np.abs(t), True


# =====================================================================================================================
# inputs
# =====================================================================================================================
def _spaces(pkg, row):
    from test_sac_oracle import _HostSpaces
    if (row.D, row.A) == (3, 1):
        return pkg.PendulumEnv(max_steps=200)
    if (row.D, row.A) == (2, 1):
        return pkg.MountainCarContinuousEnv(max_steps=200)
    return _HostSpaces(pkg, row.D, row.A)


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


def make_cfg(pkg, row, B, interval=1, lr=LR, gamma=0.99, tau=0.05):
    env = _spaces(pkg, row)
    ent = pkg.AutoEntropyCoefficient(initial_value=0.7) if row.ent == "auto" else pkg.FixedEntropyCoefficient(0.3)
    alg = pkg.SAC(batch_size=B, buffer_capacity=max(B, 8), ent_coef=ent, target_update_interval=interval, learning_rate=lr, tau=tau, gamma=gamma)
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=row.hidden, activation=row.act)
    return pkg.make_sac_config(env, 8, alg, layer, seed=7), layer


SAT = {"edge": (7.2, -7.2, 7.3, -7.3),                                             # both sides of atanh(1 - 1e-6) = 7.25, within 4 units of the clamp's edge: the jump of `inside` is in T (see the module docstring)
       "far": (6.0, -6.0, 9.0, -9.0, 20.0, -20.0)}                                 # saturated, and no jump in T: every actor element of these is held to its bound


def _draw(case, attempt):
    pkg = _pkg()
    row, B, fam, tag = case.row, case.B, case.family, case.tag
    D, A = row.D, row.A
    _, layer = make_cfg(pkg, row, B)
    sl, P = row_layout(row)
    rng = _rng("sac", D, A, row.hidden, row.act, B, fam, tag, attempt)
    ps = layer.initialparameters(rng)
    ps["actor_head"]["layer_3"]["weight"] *= 30.0 if A == 1 else 10.0               # output layers scaled so that every loss term matters
    for head in (ps["actor_head"], ps["critic_head"]["layer_1"], ps["critic_head"]["layer_2"]):
        for l in head.values():
            l["bias"] = rng.normal(0, 0.1, l["bias"].shape).astype(F)
    ps["log_std"] = rng.uniform(-3.0, 0.5, A).astype(F)                               # per dimension
    flat = pkg.sac_flatten_params(ps)
    assert flat.size == P
    c0, c1_ = critic_range(row)
    Pq = (c1_ - c0) // 2
    obs, nobs = rng.uniform(-1, 1, (B, D)).astype(F), rng.uniform(-1, 1, (B, D)).astype(F)
    actn = np.tanh(rng.normal(0, 1, (B, A))).astype(F)
    rew = rng.normal(-1, 1, B).astype(F)
    term = (rng.uniform(size=B) < 0.2).astype(np.uint8)
    noises = [rng.normal(0, 1, (N_STEPS, B, A)).astype(F) for _ in range(3)]
    idx = np.stack([rng.permutation(B) for _ in range(N_STEPS)]).astype(np.int64)
    le0 = math.log(0.7 if row.ent == "auto" else 0.3)
    if fam in ("decision", "tie"):                                                   # critic 1 = critic 0, mirrored in the output weights (decision) or identical (tie)
        flat[c0 + Pq:c1_] = flat[c0:c0 + Pq]
        if fam == "decision":
            lo, hi_, _ = sl["q1.W3"]
            flat[lo:hi_] = -flat[lo:hi_]
            term[:] = (np.arange(B) % 4 == 1)
            nobs[term.astype(bool)] = (1e5 * np.sign(nobs[term.astype(bool)])).astype(F)
    if max(row.hidden) >= 512 and fam not in ("decision", "tie"):                    # 516 / 512 units wide: E(Q) is some 5 000 u, and 64 of it is a tenth of the spread of
        flat[sl["q1.b3"][0]] += F(3.0)                                               # Q0 - Q1.  There the twins are 3 apart (one side of both minima); the decision family has both
    target = (flat[c0:c1_] * F(0.9)).astype(F)
    if fam == "decision":                                                            # q1 = 2 b - q0 with b the median of q0 over the batch: q1 < q0 on one half, q0 < q1 on the other
        p64 = flat.astype(np.float64)
        actor, sig = _net(p64, sl, "actor"), np.exp(_get(p64, sl, "log_std"))
        j = idx[0]
        o64, n64 = obs[j].astype(np.float64), nobs[j].astype(np.float64)
        a_pi = np.tanh(_fwd(actor, o64, row.act)["out"] + sig * noises[2][0])
        a_n = np.tanh(_fwd(actor, n64, row.act)["out"] + sig * noises[1][0])
        live = ~term[j].astype(bool)
        for vec, off, x in ((flat, 0, np.concatenate([o64, a_pi], 1)), (target, c0, np.concatenate([n64, a_n], 1)[live])):
            v64 = np.zeros(P); v64[c0:c1_] = vec[c0 - off:c1_ - off]
            q0 = _fwd(_net(v64, sl, "q0"), x, row.act)["out"][:, 0]
            vec[sl["q1.b3"][0] - off] = F(2 * np.median(q0) - float(vec[sl["q0.b3"][0] - off]))
    if fam == "indicator":
        j = int(tag[1:])
        others = np.arange(B) != j
        rew[others], term[others] = 0, 1
        idx[:] = np.arange(B)                                                        # the slot is a position of the BATCH
        for z in noises:
            z[:, others] = 0
    elif fam == "saturated":
        lo, hi_, _ = sl["actor.b3"]
        flat[lo:hi_] = np.where(np.arange(A) % 2, -3.0, 3.0).astype(F)
        lo, hi_, _ = sl["log_std"]
        flat[lo:hi_] = rng.uniform(-1.0, 0.5, A).astype(F)
    elif fam == "edges":
        if tag == "alpha_small":
            le0 = -12.0
        elif tag == "alpha_large":
            le0 = 4.0
        elif tag == "rew1e4":
            rew = (rew * F(1e4)).astype(F)
        elif tag == "dead_relu":                                                     # units 0 and H1 - 1 of both critics' first layer never fire: every gradient element of theirs is exactly 0
            for k in ("q0", "q1"):
                lo, hi_, _ = sl[f"{k}.b1"]
                flat[lo] = flat[hi_ - 1] = F(-100.0)
            target = (flat[c0:c1_] * F(0.9)).astype(F)
    inp = dict(flat=flat, target=target, le0=float(F(le0)), replay=(obs, actn, rew, term, np.zeros(B, np.uint8), nobs), idx=idx, noises=noises)
    if fam == "saturated":
        _sat_noise(case, inp)
    return inp


def _sat_noise(case, inp):
    """the saturated family's noise: u = mu + sigma noise lands on the family's points, whatever the observations are"""
    row, B, A = case.row, case.B, case.row.A
    sl, _ = row_layout(row)
    obs, _, _, _, _, nobs = inp["replay"]
    p64, idx, noises = inp["flat"].astype(np.float64), inp["idx"], inp["noises"]
    actor, sig = _net(p64, sl, "actor"), np.exp(_get(p64, sl, "log_std"))
    pts = SAT[case.tag]
    want = np.array(pts)[(np.arange(B)[:, None] + 3 * np.arange(A)[None, :]) % len(pts)]
    mu_o, mu_n = _fwd(actor, obs.astype(np.float64), row.act)["out"], _fwd(actor, nobs.astype(np.float64), row.act)["out"]
    for s in range(N_STEPS):                                                        # (idx permutes the rows: the noise of batch position i belongs to row idx[s, i])
        noises[0][s] = ((want - mu_o) / sig)[idx[s]].astype(F)
        noises[2][s] = ((np.roll(want, 1, axis=0) - mu_o) / sig)[idx[s]].astype(F)
        noises[1][s] = ((np.roll(want, 2, axis=0) - mu_n) / sig)[idx[s]].astype(F)


def batch_of(inp, s):
    obs, actn, rew, term, _, nobs = inp["replay"]
    j = inp["idx"][s]
    return (obs[j], actn[j], rew[j], term[j], nobs[j]), tuple(z[s] for z in inp["noises"])


_ALL = ("tmin", "amin", "inside", "relu")
CHECKED_MARGINS = {"random": _ALL, "indicator": _ALL, "decision": _ALL, "edges": _ALL, "tie": ("inside", "relu"), "saturated": ("tmin", "amin", "relu")}     # (saturated/far; Case.checked: saturated/edge has none)
THRESHOLD = {"tmin": KINK, "amin": KINK, "inside": KINK, "relu": KINK_RELU}           # (tanh rows have no kink: their relu margin is inf)
SEARCH = {"tmin": 1.5, "amin": 1.5, "inside": 1.5, "relu": 1.5}                       # what the redraw keeps, as a multiple: the implementation's trajectory differs from the reference's own by roundings


def _own_trajectory(case, inp, hp, steps):
    """the reference's own three steps from the inputs (no implementation involved) -> per step the per-sample decision margins, by replay row"""
    row, P = case.row, inp["flat"].size
    state, tr, out = (inp["flat"].astype(np.float64), inp["target"].astype(np.float64), inp["le0"]), Tracker(P), []
    for s in range(steps):
        ref = ref_step(row, hp, state, *batch_of(inp, s), tr)
        tgt, _, _ = expected_target(ref, ref.params)
        state = (ref.params, tgt, ref.stats["log_ent_coef"])
        out.append(ref.decisions["per_sample"])
    return out


@functools.lru_cache(maxsize=4)
def inputs(case):
    """a function of (shape, activation, B, family, tag).  The condition on the inputs — no twin minimum and no clamp within 64 forward-error units of its edge — is
    established here, on the CPU, with the reference alone: the rows of the replay (and their noise) that come within 1.5 x 64 units on the reference's own trajectory, of any of
    the three sequences, are drawn again.  check() then asserts the 64 units on every step an implementation runs"""
    pkg = _pkg()
    inp = _draw(case, 0)
    keys = case.checked
    if not keys:
        return inp
    rng = _rng("sac-redraw", case.name)
    obs, actn, rew, term, _, nobs = inp["replay"]
    B, D, A = case.B, case.row.D, case.row.A
    hps = []
    for _, interval, lr, steps in case.sequences:
        cfg, _ = make_cfg(pkg, case.row, B, interval, lr, *case.setting)
        hps.append((hyper(cfg, A), steps))
    for _ in range(200):
        bad = np.zeros(B, bool)
        for hp, steps in hps:
            for s, per in enumerate(_own_trajectory(case, inp, hp, steps)):
                low = np.zeros(B, bool)
                for k in keys:
                    low |= per[k] < SEARCH[k] * THRESHOLD[k]
                bad[inp["idx"][s][low]] = True
        if not bad.any():
            return inp
        for r in np.flatnonzero(bad):
            obs[r], actn[r] = rng.uniform(-1, 1, D).astype(F), np.tanh(rng.normal(0, 1, A)).astype(F)
            if not (case.family == "decision" and term[r]):
                nobs[r] = rng.uniform(-1, 1, D).astype(F)
            if case.family == "indicator" and r != int(case.tag[1:]):
                continue
            for s in range(N_STEPS):
                for z in inp["noises"]:
                    z[s, inp["idx"][s] == r] = rng.normal(0, 1, A).astype(F)
        if case.family == "saturated":
            _sat_noise(case, inp)
    raise AssertionError(f"{case.name}: no draw with clear decisions")


# =====================================================================================================================
# running a case: on the device or on the oracle, through the same typed wrapper
# =====================================================================================================================


class RowRunner:
    """the handles of one row, one per (B, interval, learning rate, gamma, tau), created under the row's switches"""

    def __init__(self, pkg, row, factory=None):
        self.pkg, self.row, self.handles, self.device = pkg, row, {}, factory is None
        self.factory = factory or (lambda cfg: pkg.SacHandle(cfg))

    def handle(self, B, interval, lr, gamma, tau):
        key = (B, interval, lr, gamma, tau)
        if key not in self.handles:
            cfg, _ = make_cfg(self.pkg, self.row, B, interval, lr, gamma, tau)
            with environ(**self.row.env):
                self.handles[key] = (self.factory(cfg), cfg)
        return self.handles[key]

    def run(self, case, seq):
        """-> the trace of one sequence: per step the state before, both gradients, the state after, the statistics, the route"""
        _, interval, lr, steps = seq
        h, cfg = self.handle(case.B, interval, lr, *case.setting)
        inp = inputs(case)
        h.set_params(inp["flat"]); h.set_target_params(inp["target"]); h.set_log_ent_coef(inp["le0"]); h.reset_optimizer()
        h.replay_fill(*inp["replay"])
        trace = []
        for s in range(steps):
            before = (h.get_params(), h.get_target_params(), h.get_log_ent_coef())
            h.set_batches(1, inp["idx"][s:s + 1], *[z[s:s + 1] for z in inp["noises"]])
            (st,) = h.update(1)
            gc, ga = h.last_grads()
            trace.append(dict(before=before, gc=gc, ga=ga, params=h.get_params(), target=h.get_target_params(), log_ent=h.get_log_ent_coef(),
                              stats={k: float(getattr(st, k)) for k in STATS if k != "log_ent_coef"}, has_ent=int(st.has_entropy_loss),
                              info=h.update_info() if self.device else None))
        return trace, cfg

    def close(self):
        for h, _ in self.handles.values():
            h.close()
        self.handles = {}


def replay_refs(case, trace, cfg, defect=None):
    """the float64 expectation of every step of a trace (the Tracker follows the REPORTED gradients)"""
    hp, tr, inp, refs = hyper(cfg, case.row.A), Tracker(trace[0]["gc"].size), inputs(case), []
    for s, st in enumerate(trace):
        batch, noises = batch_of(inp, s)
        refs.append(ref_step(case.row, hp, st["before"], batch, noises, tr, reported=(st["gc"], st["ga"]), log_ent_after=st["log_ent"], defect=defect))
    return refs


# =====================================================================================================================
# the assertion functions: (case, trace, references) and nothing else
# =====================================================================================================================
def _block_ratio(x, x64, T, lo, hi):
    e = np.abs(np.asarray(x[lo:hi], np.float64) - x64[lo:hi])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(e <= TINY, 0.0, e / (U * T[lo:hi]))
    i = int(np.argmax(q)) if q.size else 0
    return (float(q[i]) if q.size else 0.0), i


def ratios(case, trace, refs, defect=None):
    """error / (u T) per key: the largest over the steps and the elements -> {key: (ratio, step, index)}"""
    row = case.row
    sl, P = row_layout(row)
    c0, c1_ = critic_range(row)
    res = {}

    def put(k, q, s, i):
        if q > res.get(k, (-1.0, 0, 0))[0]:
            res[k] = (q, s, i)
    for s, (st, ref) in enumerate(zip(trace, refs)):
        for x in (st["gc"], st["ga"], st["params"], st["target"]):
            assert np.all(np.isfinite(x)), f"{case.name} step {s}: non-finite output"
        tgt, Ttgt, _ = expected_target(ref, st["params"], defect)
        for b in BLOCKS:
            lo, hi, _ = sl[b]
            g, g64, Tg = (st["ga"], ref.ga, ref.Tga) if b in ACTOR_BLOCKS else (st["gc"], ref.gc, ref.Tgc)
            q, i = _block_ratio(g, g64, Tg, lo, hi)
            put(f"g.{b}", q, s, i)
            q, i = _block_ratio(st["params"], ref.params, ref.Tparams, lo, hi)
            put(f"p.{b}", q, s, i)
            if b in CRITIC_BLOCKS:
                q, i = _block_ratio(st["target"], tgt, Ttgt, lo - c0, hi - c0)
                put(f"t.{b}", q, s, i)
        got = dict(st["stats"], log_ent_coef=st["log_ent"])
        for k in STATS:
            if k == "entropy_loss" and row.ent != "auto":
                continue
            e = abs(got[k] - ref.stats[k])
            put(k, 0.0 if e <= TINY else e / (U * ref.statT[k]) if ref.statT[k] > 0 else math.inf, s, 0)
    return res


def check(case, trace, refs, limit=1.0, constants=None, defect=None):
    """every check of one sequence of a case -> {key: error / bound}"""
    C = CONSTANTS if constants is None else constants
    row = case.row
    sl, P = row_layout(row)
    c0, c1_ = critic_range(row)
    a_end = sl["actor.b3"][1]
    for s, (st, ref) in enumerate(zip(trace, refs)):
        where = f"{case.name} step {s}"
        for k in case.checked:                                       # the condition on the INPUTS
            assert ref.margins[k] >= THRESHOLD[k], f"{where}: decision {k} is {ref.margins[k]:.1f} forward-error units from its edge (the inputs must keep {THRESHOLD[k]:g})"
        if (case.family, case.tag) != ("saturated", "edge"):                         # no jump in T: every element of the case is held to the f32 bound proper
            assert ref.margins["jumps"] == 0, f"{where}: {ref.margins['jumps']} decisions put their jump into T"
        gc, ga = st["gc"], st["ga"]                                                  # test/test_sac.jl:282-284,337-341
        assert not gc[:a_end].any() and not gc[sl["log_std"][0]:].any(), f"{where}: the critic gradient is not zero on the actor sub-tree / log_std"
        assert not ga[c0:c1_].any(), f"{where}: the actor gradient is not zero on the critics"
        assert st["has_ent"] == int(row.ent == "auto"), where
        if row.ent != "auto":
            assert st["log_ent"] == st["before"][2], f"{where}: a fixed entropy coefficient moved"
        _, _, moved = expected_target(ref, st["params"])
        if not moved:
            assert st["target"].tobytes() == st["before"][1].tobytes(), f"{where}: the targets moved with the polyak gate closed"
        if refs[0].decisions is not None and float(np.abs(ref.params - ref.decisions["p0"]).max()) == 0.0:
            assert st["params"].tobytes() == st["before"][0].tobytes(), f"{where}: learning_rate = 0 and the parameters moved"
        if case.family == "tie":
            assert ref.decisions["tie_a"] == case.B and ref.decisions["tie_t"] == int((~np.asarray(batch_of(inputs(case), s)[0][3], bool)).sum()), f"{where}: the twins are not tied"
            assert not ref.decisions["km"].any()
        if case.family == "decision":
            live = ~np.asarray(batch_of(inputs(case), s)[0][3], bool)
            if case.B >= 64 or case.B >= 7 and s == 0:                                 # (the split is the median of step 0; seven samples may all cross it later)
                assert ref.decisions["km"].any() and not ref.decisions["km"].all() and ref.decisions["kt"][live].any() and not ref.decisions["kt"][live].all(), f"{where}: one side of a minimum is missing"
        if case.family == "saturated" and case.B * row.A >= len(SAT[case.tag]) and (s == 0 or case.tag == "far"):   # (the edge points are 0.05 from the edge: later steps may carry them all across)
            assert (~ref.decisions["inside"]).any() and ref.decisions["inside"].any(), where
        if case.tag == "dead_relu":
            H1 = row.hidden[0]
            for k in ("q0", "q1"):
                w1, b1, w2 = _get(gc, sl, f"{k}.W1"), _get(gc, sl, f"{k}.b1"), _get(gc, sl, f"{k}.W2")
                for j in (0, H1 - 1):
                    assert not w1[j].any() and b1[j] == 0 and not w2[:, j].any(), f"{where}: {k} unit {j} is dead and has a gradient"
    res = {k: (q / C[k], s, i) for k, (q, s, i) in ratios(case, trace, refs, defect).items()}
    for k, (q, s, i) in res.items():
        assert q <= limit, f"{case.name} step {s}: {k}[{i}] error / bound {q:.3f} (limit {limit})"
    return res


def check_same(case, t0, t1):
    """the two runs of a sequence from the same state: bit-identical"""
    for s, (a, b) in enumerate(zip(t0, t1)):
        for k in ("gc", "ga", "params", "target"):
            assert a[k].tobytes() == b[k].tobytes(), f"{case.name} step {s}: the two runs differ in {k}"
        assert a["stats"] == b["stats"] and a["log_ent"] == b["log_ent"], f"{case.name} step {s}: the two runs differ in the statistics"


def check_route(case, trace):
    for s, st in enumerate(trace):
        assert st["info"].startswith(case.row.route + " "), f"{case.name} step {s}: {st['info']!r} ran, the row is about {case.row.route!r}"


# =====================================================================================================================
# a defect on top of a trace (the mutants of tests/test_sac_update_cases.py)
# =====================================================================================================================
def with_defect(case, trace, cfg, defect):
    """trace plus the float64 difference that `defect` makes, step by step -> (trace', does it change anything)"""
    good, bad = replay_refs(case, trace, cfg), replay_refs(case, trace, cfg, defect)
    out, changed = [], False
    for st, g, b in zip(trace, good, bad):
        tg, _, _ = expected_target(g, st["params"])
        tb, _, _ = expected_target(b, st["params"], defect)
        new = dict(st)
        for k, dg in (("gc", b.gc - g.gc), ("ga", b.ga - g.ga), ("params", b.params - g.params), ("target", tb - tg)):
            changed |= bool(np.any(dg != 0))
            new[k] = (st[k].astype(np.float64) + dg).astype(F)
        new["stats"] = {k: float(F(v + (b.stats[k] - g.stats[k]))) if k in g.stats else v for k, v in st["stats"].items()}
        new["log_ent"] = float(F(st["log_ent"] + (b.stats["log_ent_coef"] - g.stats["log_ent_coef"])))
        changed |= any(b.stats[k] != g.stats[k] for k in g.stats)
        out.append(new)
    return out, changed


def worst_of(runner_factory, rows, report=None):
    worst = {}
    for row in rows:
        r = runner_factory(row)
        for case in cases_of(row):
            for seq in case.sequences:
                trace, cfg = r.run(case, seq)
                for k, (q, s, i) in ratios(case, trace, replay_refs(case, trace, cfg)).items():
                    if q > worst.get(k, (0.0, ""))[0]:
                        worst[k] = (q, f"{case.name}/{seq[0]}/step{s}")
        r.close()
        if report:
            report(row)
    return worst


if __name__ == "__main__":
    import oracle_lib
    oracle_lib.ensure_built()
    pkg = _pkg()
    names = json.loads(sys.argv[2]) if len(sys.argv) > 2 else None
    w = worst_of(lambda row: RowRunner(pkg, row, oracle_lib.sac_oracle), [r for r in ROWS if not names or r.name in names], lambda row: print("#", row.name, file=sys.stderr, flush=True))
    for k in KEYS:                                                                   # rounded UP to three digits
        q = w.get(k, (0.0, ""))[0]
        if q <= 0:
            print(f'    "{k}": 0.0,'); continue
        d = 10.0 ** (math.floor(math.log10(q)) - 2)
        up = float(f"{math.ceil(q / d) * d:.3g}")
        up = up if up >= q else float(f"{up + d:.3g}")
        print(f'    "{k}": {up:g},'.ljust(40) + f"# {w[k][1]}")
