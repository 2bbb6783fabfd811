"""The case table of the five PPO gradient paths (ppo_grad_kernel, ppo_grad_pair_kernel, ppo_grad_wide_kernel, ppo_grad_wide_split_kernel, generic_ppo_grad), their
inputs, the float64 reference WITH ATTRIBUTION, the per-element error bounds and the assertion functions (test infrastructure of tests/test_grad_cases.py and
tests/test_gpu_grad.py).  Everything goes through dril_ppo_loss_grad: pack_records -> ppo_step -> the selected gradient kernel -> grad_reduce_kernel.

Reference: a numpy float64 restatement of ppo.jl:365-407 with a hand-written reverse pass (tanh, both heads, entropy term, value clip, advantage normalisation with the
corrected std and eps on the std).  Beside loss, the seven statistics and the gradient g64 it returns per sample the head signals dLoss/dout_i and dLoss/dV_i, the
decisions taken (ratio clipped, gradient blocked, value clipped) and T, the result of the ABSOLUTE-VALUE pass: the same recurrences with every factor replaced by its
absolute value and every sum of signed addends by the sum of their absolute values,
  |dz2| = (|dout| |W3|) o tanh'      |dh1| = |dz2| |W2|      T[dW] = sum_i |delta_i| |x_i|'  (products of absolute-value matrices, never a B x P array),
carried as a running error analysis: every quantity has a scale E >= |value|, the first-order bound in units of u of what a float32 evaluation leaves in it (the rules
stand above _forward_scale).  T[e] = E(g[e]) is what the error of element e is bounded against.  It covers the cancellation in the sample sum and inside the
back-propagated signals, and — what the pass over exact forward quantities cannot, and what the oracle shows to matter by factors of 1e5 - 1e7 on single samples,
saturated units and |logp| ~ 1e3 — the rounding of the forward pass itself: h1, h2, 1 - h^2, the softmax, exp(logp - old_logp).

Bound, with u = 2^-24:  |g[e] - g64[e]| <= c_block u T[e]  — one constant per parameter block (W1 b1 W2 b2 W3 b3 of each net, log_std); for the loss and the
statistics  c u sum_i E(term_i) / n;  clip_fraction n must be the float64 COUNT.  The constants are not derived and not fitted to the device: c = 4 x the largest
error / (u T) that the project's f32 CPU oracle (orc_ppo_loss_grad, one thread) reaches on this same case table (ORACLE_WORST below; `python tests/grad_cases.py oracle`
measures it again).  The 4 = 2 (the device sums the samples in another order: per-lane accumulators, slabs, a tree) x 2 (what split_budget.within_budget grants the
f16-piece kernels over exact f32).  tests/test_grad_cases.py holds the oracle to one quarter of every bound on every case, so an edit of the table re-measures.

A row of the table is (kernel, env kind, hidden, grid switch); it runs its batch sizes and input families, every case twice (bit-identical).  The loss settings are
latched by dril_create, so a row uses one handle per SETTING (default, ent_vfclip, no_norm, the indicator and decision settings), all created under the row's switches.
Rows of the same shape draw the same inputs, whatever kernel runs them.
"""
from __future__ import annotations

import contextlib
import functools
import hashlib
import json
import math
import os
import re
import sys
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

U = 2.0 ** -24
TINY = 2.0 ** -149
F = np.float32
K_TILE = 32
ENV = {0: (4, 2, True), 1: (3, 1, False), 3: (2, 3, True), 4: (2, 1, False), 6: (6, 3, True)}          # kind -> (obs dims, action dims, discrete): EnvSpec<KIND> of dril_device.h
NET_BLOCKS = ("W1", "b1", "W2", "b2", "W3", "b3")
BLOCKS = tuple(f"{n}.{b}" for n in ("actor", "critic") for b in NET_BLOCKS) + ("log_std",)
STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "entropy", "ratio")                # clip_fraction (statistic 3) is a count: exact
STAT_SLOT = {"policy_loss": 0, "value_loss": 1, "entropy_loss": 2, "approx_kl": 4, "entropy": 5, "ratio": 6}

# the largest error / (u T) of orc_ppo_loss_grad over the whole table, per block and per statistic (`python tests/grad_cases.py oracle`)
ORACLE_WORST = {                        # (rounded up to three digits)      reached at
    "actor.W1": 0.0279,                 # pair.k1/B20/random/ent_vfclip/s1
    "actor.b1": 0.0121,                 # f32.k4.h64/B33/random/default/s1
    "actor.W2": 0.456,                  # f32.k4.h64/B2/random/default/s1
    "actor.b2": 0.371,                  # f32.k1.h64/B2/random/default/s1
    "actor.W3": 0.076,                  # f32.k6.h64/B128/ind_actor.j31/ind_actor/s0.25
    "actor.b3": 0.0165,                 # pair.k1/B20/random/ent_vfclip/s1
    "critic.W1": 0.155,                 # f32.k0.h32/B2/random/default/s1
    "critic.b1": 0.0648,                # pair.k0/B129/random/ent_vfclip/s1
    "critic.W2": 0.499,                 # f32.k4.h64/B31/random/ent_vfclip/s1
    "critic.b2": 0.499,                 # f32.k4.h64/B31/random/ent_vfclip/s1
    "critic.W3": 0.0888,                # f32.k0.h64/B32/ind_critic.j31/ind_critic/s0.25
    "critic.b3": 0.0348,                # f32.k1.h32/B4096/ind_critic.j4064/ind_critic/s0.25
    "log_std": 0.0996,                  # f32.k1.h32/B33/ind_actor.j32/ind_actor/s0.25
    "loss": 0.405,                      # f32.k6.h64/B33/ind_actor.j31/ind_actor/s0.25
    "policy_loss": 0.405,               # f32.k6.h64/B33/ind_actor.j31/ind_actor/s0.25
    "value_loss": 0.536,                # f32.k4.h64/B2/log_std.p1/ent_vfclip/s0.25
    "entropy_loss": 0.546,              # wsplit.k1.h256/B2/random/default/s0.3
    "approx_kl": 0.0345,                # f32.k1.h32/B2/log_std.p1/ent_vfclip/s0.25
    "entropy": 0.546,                   # wsplit.k1.h256/B2/random/default/s0.3
    "ratio": 0.16,                      # f32.k4.h64/B257/random/ent_vfclip/s1
}
MARGIN = 4.0
CONSTANTS = {k: MARGIN * v for k, v in ORACLE_WORST.items()}


# =====================================================================================================================
# settings and rows
# =====================================================================================================================
SETTINGS = {
    "default": {},
    "ent_vfclip": dict(ent_coef=0.01, has_clip_range_vf=1, clip_range_vf=0.3, clip_range=0.1),
    "no_norm": dict(normalize_advantage=0),
    "ind_actor": dict(normalize_advantage=0, ent_coef=0.0, vf_coef=0.0),
    "ind_critic": dict(normalize_advantage=0, ent_coef=0.0, has_clip_range_vf=1, clip_range_vf=0.3),
    "decisions": dict(normalize_advantage=0, ent_coef=0.01, has_clip_range_vf=1, clip_range_vf=0.3),
    "norm_noent": dict(normalize_advantage=1, ent_coef=0.0),
}


@dataclass(frozen=True)
class Row:
    name: str
    kernel: str                   # what grad_kernel_info() must name
    kind: int
    H: int
    sizes: tuple
    variant: object = None        # DRIL_GRAD_VARIANT around dril_create (None: the library's own selection)
    gmax: int = 0                 # DRIL_GRAD_GMAX (with DRIL_DEBUG=1)
    no_small: bool = False        # DRIL_NO_SMALL_PATH (with DRIL_DEBUG=1): the two-launch advantage moments instead of the in-kernel ones
    permille: int = 0             # DRIL_GRAD_ACTOR_PERMILLE
    generic: bool = False         # DRIL_FORCE_GENERIC
    trip_tiles: int = 0           # tiles of one trip of the whole grid under gmax: slot 32 trip_tiles is the first sample of a second trip
    chip: bool = False            # the pair kernel's chip-filling division: G != Gc

    @property
    def dims(self):
        return ENV[self.kind]

    @property
    def env(self):
        e = {}
        if self.gmax or self.no_small:
            e["DRIL_DEBUG"] = "1"
        if self.gmax:
            e["DRIL_GRAD_GMAX"] = str(self.gmax)
        if self.no_small:
            e["DRIL_NO_SMALL_PATH"] = "1"
        if self.permille:
            e["DRIL_GRAD_ACTOR_PERMILLE"] = str(self.permille)
        if self.generic:
            e["DRIL_FORCE_GENERIC"] = "1"
        return e


CHIP_B = 16384 + 33


def _rows():
    R = []
    f32_sizes = (2, 31, 32, 33, 127, 128, 129, 257, 4096, 4097)           # 129: a second workgroup with one live lane; 4096 | 4097: in-kernel moments | the moments launches
    for H, kinds in ((64, (0, 1, 3, 4, 6)), (32, (0, 1))):
        for k in kinds:
            R.append(Row(f"f32.k{k}.h{H}", "ppo_grad_kernel", k, H, f32_sizes, variant=0))
    for k in (0, 1):                                                       # ten tiles over four waves: three trips, the last tile ragged
        R.append(Row(f"f32.k{k}.h64.gmax1", "ppo_grad_kernel", k, 64, (300,), variant=0, gmax=1, trip_tiles=4))
        R.append(Row(f"f32.k{k}.h64.nosmall", "ppo_grad_kernel", k, 64, (33, 300, 4096), variant=0, no_small=True))
    pair_sizes = (2, 20, 32, 33, 64, 65, 97, 129, 257)                     # 20: the second pair owns nothing; 97: three tiles on two pairs
    for k in (0, 1, 3, 4, 6):
        R.append(Row(f"pair.k{k}", "ppo_grad_pair_kernel", k, 64, pair_sizes, variant=2))
    for k in (0, 1):                                                       # eleven tiles on two pairs: one pair runs a trip more than the other
        R.append(Row(f"pair.k{k}.gmax2", "ppo_grad_pair_kernel", k, 64, (333,), variant=2, gmax=2, trip_tiles=2))
    R.append(Row("pair.k1.chip", "ppo_grad_pair_kernel", 1, 64, (CHIP_B,), variant=2, chip=True))              # 514 tiles: the default division (460 + 564 pairs on 256 CUs)
    R.append(Row("pair.k0.chip300", "ppo_grad_pair_kernel", 0, 64, (CHIP_B,), variant=2, permille=300, chip=True))
    wide_sizes = (2, 33, 64, 65, 129, 257)                                 # the split form takes kWideSplitNT = 2 tiles per pass
    for kernel, variant, tt in (("ppo_grad_wide_split_kernel", None, 2), ("ppo_grad_wide_kernel", 0, 1)):
        tag = "wsplit" if variant is None else "wide"
        for H in (128, 256):
            for k in (1, 0, 6):
                R.append(Row(f"{tag}.k{k}.h{H}", kernel, k, H, wide_sizes, variant=variant))
            R.append(Row(f"{tag}.k1.h{H}.gmax1", kernel, 1, H, (257,), variant=variant, gmax=1, trip_tiles=tt))  # five passes (nine tiles) in one workgroup, the last with one sample
    for k in (0, 1):                                                       # one, two and three slabs of >= 512 rows rounded to 32
        R.append(Row(f"generic.k{k}", "generic path", k, 64, (33, 513, 1025), generic=True))
    return R


ROWS = _rows()
ROW_BY_NAME = {r.name: r for r in ROWS}
assert len(ROW_BY_NAME) == len(ROWS)


@dataclass(frozen=True)
class Case:
    row: Row
    B: int
    family: str                   # random | ind_actor | ind_critic | decisions | equal_adv | zero_col | log_std | one_action | all_actions
    setting: str
    scale: float                  # of the parameters
    tag: str = ""                 # slot j of an indicator, the log_std value, ...

    @property
    def name(self):
        return f"{self.row.name}/B{self.B}/{self.family}{'.' + self.tag if self.tag else ''}/{self.setting}/s{self.scale:g}"


def scales(H):
    return (0.25, 1.0) if H <= 64 else (0.08, 0.3)


def indicator_slots(row, B):
    """0, 31, 32, B - 1, the first and the last slot of the last tile, the first slot of a second trip"""
    last = (B - 1) // K_TILE * K_TILE
    s = {0, 31, 32, B - 1, last}
    if row.trip_tiles:
        s.add(K_TILE * row.trip_tiles)
    return sorted(j for j in s if 0 <= j < B)


def cases_of(row):
    """the cases of a row in the order the tests run them: random first"""
    D, A, discrete = row.dims
    lo, hi = scales(row.H)
    combos = [(s, sc) for s in ("default", "ent_vfclip", "no_norm") for sc in (lo, hi)]
    out = []
    for i, B in enumerate(row.sizes):
        # every setting x scale within the row's sizes; all six at the single-size rows and around the 4096-sample edge of the in-kernel advantage moments
        pick = combos if len(row.sizes) < 3 or B >= 4096 else [combos[(2 * i) % 6], combos[(2 * i + 1) % 6]]
        out += [Case(row, B, "random", s, sc) for s, sc in pick]
        out.append(Case(row, B, "decisions", "decisions", lo))
        for j in indicator_slots(row, B):
            out.append(Case(row, B, "ind_actor", "ind_actor", lo, f"j{j}"))
            out.append(Case(row, B, "ind_critic", "ind_critic", lo, f"j{j}"))
        out.append(Case(row, B, "equal_adv", "norm_noent", lo))
        out.append(Case(row, B, "zero_col", "default", lo, f"c{i % D}"))
        if discrete:
            out.append(Case(row, B, "one_action", "ent_vfclip", lo, f"a{i % A}"))
            if B >= A:
                out.append(Case(row, B, "all_actions", "ent_vfclip", lo))
        else:
            out += [Case(row, B, "log_std", "ent_vfclip", lo, t) for t in ("m3", "p1")]
    return out


def make_cfg(capi, row, setting):
    cfg = capi.default_config(row.kind)
    cfg.n_envs, cfg.n_steps, cfg.batch_size, cfg.hidden1, cfg.hidden2 = 2, 2, 2, row.H, row.H
    for k, v in SETTINGS[setting].items():
        setattr(cfg, k, v)
    return cfg


@functools.lru_cache(maxsize=None)
def _host_cfg(row, setting):
    import __graft_entry__ as g
    return make_cfg(g.load_package()._capi, row, setting)


# =====================================================================================================================
# the parameter vector (include/dril_hip.h: {W1 b1 W2 b2 W3 b3} of the actor, of the critic, log_std; W as in x out, i.e. the transpose of out x in, row-major)
# =====================================================================================================================
def block_slices(D, H, A, discrete):
    out, off = {}, 0
    for net, O in (("actor", A), ("critic", 1)):
        for (i, o), (w, b) in zip(((D, H), (H, H), (H, O)), (("W1", "b1"), ("W2", "b2"), ("W3", "b3"))):
            out[f"{net}.{w}"] = slice(off, off + o * i); off += o * i
            out[f"{net}.{b}"] = slice(off, off + o); off += o
    out["log_std"] = slice(off, off + (0 if discrete else A))
    return out, off + (0 if discrete else A)


def _net(flat, sl, net, D, H, O):
    W = lambda k, i, o: flat[sl[f"{net}.{k}"]].reshape(i, o).T                               # out x in
    return (W("W1", D, H), flat[sl[f"{net}.b1"]], W("W2", H, H), flat[sl[f"{net}.b2"]], W("W3", H, O), flat[sl[f"{net}.b3"]])


def _mlp(net, x):
    W1, b1, W2, b2, W3, b3 = net
    h1 = np.tanh(x @ W1.T + b1)
    h2 = np.tanh(h1 @ W2.T + b2)
    return h1, h2, h2 @ W3.T + b3


LOG2PI = math.log(2 * math.pi)


def forward64(row, flat, obs, actions, action_start=1):
    """float64 log-probability, entropy and value of every sample (and what the reverse pass needs)"""
    D, A, discrete = row.dims
    flat, x = np.asarray(flat, np.float64), np.asarray(obs, np.float64)
    sl, P = block_slices(D, row.H, A, discrete)
    assert flat.size == P
    actor, critic = _net(flat, sl, "actor", D, row.H, A), _net(flat, sl, "critic", D, row.H, 1)
    fw = {"x": x, "actor": actor, "critic": critic, "sl": sl, "P": P}
    fw["h1a"], fw["h2a"], out = _mlp(actor, x)
    fw["h1c"], fw["h2c"], v = _mlp(critic, x)
    fw["out"], fw["v"] = out, v[:, 0]
    if discrete:
        z = out - out.max(axis=1, keepdims=True)
        logp_all = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
        p = np.exp(logp_all)
        a = np.asarray(actions).astype(np.int64) - action_start
        fw.update(p=p, logp_all=logp_all, a=a, logp=logp_all[np.arange(len(a)), a], ent=-(p * logp_all).sum(axis=1))
    else:
        ls = flat[sl["log_std"]]
        d = np.asarray(actions, np.float64).reshape(-1, A) - out
        iv = np.exp(-2 * ls)
        fw.update(ls=ls, d=d, iv=iv, act=np.asarray(actions, np.float64).reshape(-1, A), logp=-0.5 * (2 * ls.sum() + (d * d * iv).sum(axis=1) + A * LOG2PI),
                  ent=np.full(len(x), 0.5 * A * (1 + LOG2PI) + ls.sum()))
    return fw


@dataclass
class Ref:
    loss: float
    stats: np.ndarray             # the seven statistics (ppo.jl:388-396 order)
    g: np.ndarray
    T: np.ndarray                 # the absolute-value reverse pass
    stat_T: dict                  # sum_i |term_i| / n of the loss and of every statistic
    clip_count: int
    dout: np.ndarray              # (B, A) dLoss/dout_i
    dV: np.ndarray                # (B) dLoss/dV_i
    ratio_clipped: np.ndarray     # r != clamp(r)
    blocked: np.ndarray           # the clip takes the sample's policy gradient away
    v_clipped: np.ndarray
    logp: np.ndarray
    v: np.ndarray
    sl: dict = field(repr=False, default=None)


DEFECTS = ("drop_last_ragged", "double_sample", "drop_tile", "drop_critic_slab", "db2_from_actor", "swap_dW3_rows", "log_std_no_entropy", "log_std_missing",
           "ratio_clip_inverted_neg", "vclip_passes", "invB_tile_rounded", "std_uncorrected", "clip_fraction_off_by_one")


def _backward(net, x, h1, h2, dout):
    """the reverse pass of one net"""
    W1, b1, W2, b2, W3, b3 = net
    dz2 = (dout @ W3) * (1 - h2 * h2)
    dz1 = (dz2 @ W2) * (1 - h1 * h1)
    return {"W1": dz1.T @ x, "b1": dz1.sum(axis=0), "W2": dz2.T @ h1, "b2": dz2.sum(axis=0), "W3": dout.T @ h2, "b3": dout.sum(axis=0)}


# ---- the absolute-value pass.  Every quantity q of the computation gets a scale E(q) >= |q|: the first-order bound, in units of u, of the error a float32 evaluation
# leaves in it.  The rules are those of a running error analysis — each has ONE scale per term, all other factors are absolute VALUES:
#     E(sum_k a_k b_k) = sum_k |a_k| E(b_k) + E(a_k) |b_k| + |a_k b_k|            E(f(a)) = |f'(a)| E(a) + |f(a)|            E(input) = 0
# With exact forward quantities (E(h) = |h|, E(tanh') = tanh') this is the pass of the module docstring: |dz2| = (|dout| |W3|) o tanh', T[dW] = sum_i |delta_i| |x_i|'.
# The forward scales are what is added to it: without them a saturated unit (1 - h^2 ~ u: the scale of 1 - h^2 is 2 |h| E(h) + |1 - h^2|, which for an exact
# pre-activation is 1 + h^2, the sum of the absolute addends), a ratio exp(logp - old_logp) with |logp| ~ 1e3 (log_std = -3) or the single sample of an indicator whose
# h2 passes through zero have no bound in terms of the signed quantities at all (measured on the CPU oracle: 1e5 - 1e7 u T).
# Two properties of the fused kernels' arithmetic enter the scales, both read off dril_device.h, neither measured:
#   * tanh is 1 - 2 / (2^(x 2 log2 e) + 1) on the 1-ulp exp2 and rcp units (tanh_f32, tanh16): t = 1 / (e + 1) carries 3 u relative (exp2, the addition, rcp) and
#     1 - 2 t = h one more rounding, so the result is off by 3 (1 - h) + |h| in units of u — an ABSOLUTE 3 u at h = 0, where a libm tanh is off by |h| u; the share of
#     the rounded argument, |x| (1 - h^2), is part of tanh' E(z) already.  A libm tanh (the oracle's) meets the same scale.
#   * the f16-piece kernels (ppo_grad_pair_kernel, ppo_grad_wide_split_kernel) cut an operand x S into hi + lo, 2^-24 relative while lo is a normal f16 and an
#     ABSOLUTE 2^-25 below |x S| = 0.125 ("the same on f16 pieces", dril_device.h), with S = kActScale = 256 for activations, kWScale = 64 for W2 and
#     SG = 8 x 2^floor(log2 B) for the gradient tile dz2: 0.5 / S in units of u on every element of such an operand (FLOOR_*; `split` rows only).
SPLIT_KERNELS = ("ppo_grad_pair_kernel", "ppo_grad_wide_split_kernel")
FLOOR_ACT, FLOOR_W = 0.5 / 256.0, 0.5 / 64.0


def _tanh_own(h):
    return 3 * (1 - h) + np.abs(h)


def _forward_scale(net, x, h1, h2, split):
    W1, b1, W2, b2, W3, b3 = (np.abs(t) for t in net)
    x, a1, a2 = np.abs(x), np.abs(h1), np.abs(h2)
    fa, fw_ = (FLOOR_ACT, FLOOR_W) if split else (0.0, 0.0)
    e1 = (1 - a1 * a1) * (x @ W1.T + b1) + _tanh_own(h1)
    e2 = (1 - a2 * a2) * ((e1 + fa + a1) @ W2.T + fw_ * a1.sum(axis=1, keepdims=True) + b2) + _tanh_own(h2)
    return {"h1": e1 + fa, "h2": e2, "out": (e2 + a2) @ W3.T + b3, "t1": (1 - a1 * a1) + 2 * a1 * e1, "t2": (1 - a2 * a2) + 2 * a2 * e2}


def _backward_scale(net, x, h1, h2, dout, e_dout, fs, floor_g, floor_w):
    """E of every gradient block of one net from the head signal (dout, E(dout)) and the forward scales fs"""
    W1, b1, W2, b2, W3, b3 = (np.abs(t) for t in net)
    dh2 = dout @ net[4]
    tp2, tp1 = 1 - h2 * h2, 1 - h1 * h1
    dz2 = dh2 * tp2
    a_dout, a_dz2 = np.abs(dout), np.abs(dz2)
    e_dh2 = (e_dout + a_dout) @ W3
    e_dz2 = np.abs(dh2) * fs["t2"] + tp2 * e_dh2 + a_dz2 + floor_g * (a_dz2 > 0)                        # (the pieces of an exact zero are zero)
    dh1 = dz2 @ net[2]
    dz1 = dh1 * tp1
    e_dh1 = (e_dz2 + a_dz2) @ W2 + floor_w * a_dz2.sum(axis=1, keepdims=True)
    e_dz1 = np.abs(dh1) * fs["t1"] + tp1 * e_dh1 + np.abs(dz1)
    a_dz1, ax, a1, a2 = np.abs(dz1), np.abs(x), np.abs(h1), np.abs(h2)
    return {"W1": (e_dz1 + a_dz1).T @ ax, "b1": (e_dz1 + a_dz1).sum(axis=0), "W2": e_dz2.T @ a1 + a_dz2.T @ (fs["h1"] + a1), "b2": (e_dz2 + a_dz2).sum(axis=0),
            "W3": e_dout.T @ a2 + a_dout.T @ (fs["h2"] + a2), "b3": (e_dout + a_dout).sum(axis=0)}


def reference(row, cfg, flat, batch, defect=None):
    """float64 loss, statistics, gradient, attribution and T of one minibatch; `defect`: one of DEFECTS, the float64 result a kernel with that defect would give"""
    D, A, discrete = row.dims
    obs, actions, adv, ret, olp, ov = batch
    adv, ret, olp, ov = (np.asarray(t, np.float64) for t in (adv, ret, olp, ov))
    n = len(adv)
    fw = forward64(row, flat, obs, actions, cfg.action_start)
    sl, x = fw["sl"], fw["x"]
    c, cv, entc, vfc = float(cfg.clip_range), float(cfg.clip_range_vf), float(cfg.ent_coef), float(cfg.vf_coef)
    tiles = (n + K_TILE - 1) // K_TILE
    wa, wc = np.ones(n), np.ones(n)                                                  # how often the actor / the critic side counts a sample
    if defect == "drop_last_ragged":
        if n % K_TILE:
            wa[n - 1] = wc[n - 1] = 0
    elif defect == "double_sample":
        wa[n // 2] = wc[n // 2] = 2
    elif defect == "drop_tile":
        t = min(1, tiles - 1)
        wa[K_TILE * t:K_TILE * (t + 1)] = wc[K_TILE * t:K_TILE * (t + 1)] = 0
    elif defect == "drop_critic_slab":                                               # one slab share: every G-th tile of the critic
        G = max(2, min(tiles, 8))
        wc[(np.arange(n) // K_TILE) % G == G - 1] = 0
    invB = 1.0 / (K_TILE * tiles) if defect == "invB_tile_rounded" else 1.0 / n
    if cfg.normalize_advantage:                                                      # ppo.jl:350-356: corrected std, eps on the std
        mean, sd = adv.mean(), adv.std(ddof=0 if defect == "std_uncorrected" else 1)
        advn = (adv - mean) / (sd + 1e-8)
    else:
        advn = adv
    logp, ent, v = fw["logp"], fw["ent"], fw["v"]
    split = row.kernel in SPLIT_KERNELS
    floor_g, floor_w = (0.5 / (8.0 * 2.0 ** math.floor(math.log2(n))), FLOOR_W) if split else (0.0, 0.0)
    sa, sc = _forward_scale(fw["actor"], x, fw["h1a"], fw["h2a"], split), _forward_scale(fw["critic"], x, fw["h1c"], fw["h2c"], split)
    if cfg.normalize_advantage:
        e_adv = (np.abs(adv) + abs(mean)) / (sd + 1e-8) + 2 * np.abs(advn)
    else:
        e_adv = np.zeros(n)
    if discrete:                                                                     # softmax: dp_i / p_i = dz_i - sum_j p_j dz_j, at most twice the largest logit error
        p, la, H = fw["p"], fw["logp_all"], ent[:, None]
        eps_p = (2 * sa["out"].max(axis=1) + 1)[:, None]
        e_p, e_la = p * eps_p, eps_p + np.abs(la)
        e_H = (e_p * np.abs(la) + p * e_la + p * np.abs(la)).sum(axis=1, keepdims=True)
        e_logp, e_ent = e_la[np.arange(n), fw["a"]], e_H[:, 0] + ent
    else:
        dd, iv, ls = fw["d"], fw["iv"], fw["ls"]
        e_d, e_iv = sa["out"] + np.abs(dd), iv * (2 * np.abs(ls) + 1)
        q = dd * dd * iv
        e_q = 2 * np.abs(dd) * iv * e_d + dd * dd * e_iv + q
        e_logp = 0.5 * e_q.sum(axis=1) + np.abs(ls).sum() + 0.5 * q.sum(axis=1) + 0.5 * A * LOG2PI
        e_ent = np.full(n, np.abs(ls).sum() + 0.5 * A * (1 + LOG2PI))
    lr = logp - olp
    r = np.exp(lr)
    lo, hi = 1 - c, 1 + c
    rc = np.clip(r, lo, hi)
    t1, t2 = r * advn, rc * advn
    sel = t2 < t1                                                                    # min picks the clipped term only when it is smaller (ppo.jl:382)
    if defect == "ratio_clip_inverted_neg":
        sel = np.where(advn < 0, t2 > t1, sel)
    m = np.where(sel, t2, t1)
    outside = (r < lo) | (r > hi)
    blocked = sel & outside
    e_lr = e_logp + np.abs(lr)
    e_r = r * e_lr + r                                                               # an absolute error of the exponent is a relative error of the ratio
    e_m = np.abs(advn) * np.where(sel, 1.0, e_r) + np.where(sel, rc, r) * e_adv + np.abs(m)
    dm = np.where(blocked, 0.0, advn)
    dlogp = -invB * dm * r * wa
    e_dlogp = invB * (np.abs(dm) * e_r + r * np.where(blocked, 0.0, e_adv)) * wa + 2 * np.abs(dlogp)
    dent = -invB * entc * wa
    if cfg.has_clip_range_vf:                                                        # ppo.jl:344-346, 378: clamp passes the derivative on lo <= x <= hi
        d = v - ov
        vpass = (d >= -cv) & (d <= cv)
        vcl = ov + np.clip(d, -cv, cv)
        e_vcl = np.where(vpass, sc["out"][:, 0] + np.abs(d), 0.0) + np.abs(vcl)
    else:
        vpass, vcl, e_vcl = np.ones(n, bool), v, sc["out"][:, 0]
    ve = vcl - ret
    e_ve = e_vcl + np.abs(ve)
    pv = np.ones(n) if defect == "vclip_passes" else vpass.astype(np.float64)
    dV = pv * invB * vfc * 2 * ve * wc
    e_dV = pv * invB * vfc * 2 * e_ve * wc + 2 * np.abs(dV)
    g, T = np.zeros(fw["P"]), np.zeros(fw["P"])
    if discrete:
        onehot = np.zeros_like(p)
        onehot[np.arange(n), fw["a"]] = 1
        op, qh = onehot - p, p * (la + H)
        dout = dlogp[:, None] * op + dent[:, None] * (-qh)
        e_qh = e_p * np.abs(la + H) + p * (e_la + e_H) + 2 * np.abs(qh)
        e_dout = e_dlogp[:, None] * np.abs(op) + np.abs(dlogp)[:, None] * (e_p + 2 * np.abs(op)) + np.abs(dent)[:, None] * (e_qh + np.abs(qh)) + np.abs(dout)
    else:
        dout = dlogp[:, None] * dd * iv
        e_dout = e_dlogp[:, None] * np.abs(dd) * iv + np.abs(dlogp)[:, None] * (e_d * iv + np.abs(dd) * e_iv) + 2 * np.abs(dout)
        e_on = 0.0 if defect == "log_std_no_entropy" else 1.0
        sg = dlogp[:, None] * (q - 1)
        g[sl["log_std"]] = sg.sum(axis=0) + e_on * dent.sum()
        T[sl["log_std"]] = (e_dlogp[:, None] * np.abs(q - 1) + np.abs(dlogp)[:, None] * (e_q + np.abs(q - 1)) + 2 * np.abs(sg)).sum(axis=0) + 2 * np.abs(dent).sum()
        if defect == "log_std_missing":
            g[sl["log_std"]] = 0
    for net, sig, e_sig, h1, h2, fs in (("actor", dout, e_dout, fw["h1a"], fw["h2a"], sa), ("critic", dV[:, None], e_dV[:, None], fw["h1c"], fw["h2c"], sc)):
        gb = _backward(fw[net], x, h1, h2, sig)
        tb = _backward_scale(fw[net], x, h1, h2, sig, e_sig, fs, floor_g, floor_w)
        for k in NET_BLOCKS:
            g[sl[f"{net}.{k}"]] = gb[k].T.ravel() if gb[k].ndim == 2 else gb[k]
            T[sl[f"{net}.{k}"]] = tb[k].T.ravel() if tb[k].ndim == 2 else tb[k]
    if defect == "db2_from_actor":
        g[sl["critic.b2"]] = g[sl["actor.b2"]]
    elif defect == "swap_dW3_rows":                                                  # rows = outputs: W3 is stored in x out
        w = g[sl["actor.W3"]].reshape(row.H, A).copy()
        w[:, [0, 1]] = w[:, [1, 0]]
        g[sl["actor.W3"]] = w.ravel()
    kl = np.exp(lr) - 1 - lr
    clipped = r != rc
    pl, vl, em = -(m * wa).sum() / n, (ve * ve * wc).sum() / n, (ent * wa).sum() / n
    stats = np.array([pl, vl, -em, (clipped * wa).sum() / n, (kl * wa).sum() / n, em, (r * wa).sum() / n])
    pl_a, vl_a, em_a = ((e_m + np.abs(m)) * wa).sum() / n, ((2 * np.abs(ve) * e_ve + 2 * ve * ve) * wc).sum() / n, ((e_ent + np.abs(ent)) * wa).sum() / n
    stat_T = {"loss": pl_a + entc * em_a + vfc * vl_a, "policy_loss": pl_a, "value_loss": vl_a, "entropy_loss": em_a, "approx_kl": ((e_r + e_lr + r + 1 + np.abs(lr)) * wa).sum() / n,
              "entropy": em_a, "ratio": ((e_r + r) * wa).sum() / n}
    count = int(round((clipped * wa).sum())) + (1 if defect == "clip_fraction_off_by_one" else 0)
    if defect == "clip_fraction_off_by_one":
        stats[3] += 1.0 / n
    return Ref(pl + entc * (-em) + vfc * vl, stats, g, T, stat_T, count, dout, dV, clipped, blocked, ~vpass, logp, v, sl)


# =====================================================================================================================
# inputs
# =====================================================================================================================
def _rng(*key):
    h = hashlib.sha256("/".join(str(k) for k in key).encode()).digest()
    return np.random.default_rng(int.from_bytes(h[:8], "little"))


R_STAR = lambda c: ((1 + c) * (1 + 1e-3), (1 + c) * (1 - 1e-3), (1 - c) * (1 + 1e-3), (1 - c) * (1 - 1e-3))
D_STAR = lambda cv: (cv * 1.01, cv * 0.99, -cv * 0.99, -cv * 1.01)


@functools.lru_cache(maxsize=8)
def inputs(case):
    """-> flat (P) and the batch (obs, actions, adv, ret, old_logp, old_values), float32 / int32: a function of (row's shape, B, family, tag, setting, scale)"""
    row, B = case.row, case.B
    D, A, discrete = row.dims
    cfg = _host_cfg(row, case.setting)
    rng = _rng(row.kind, row.H, B, case.family, case.tag, case.setting, case.scale)
    sl, P = block_slices(D, row.H, A, discrete)
    flat = (rng.standard_normal(P) * case.scale).astype(F)
    obs = rng.uniform(-1, 1, (B, D)).astype(F)
    act = (rng.integers(0, A, B) + cfg.action_start).astype(np.int32) if discrete else rng.normal(0, 1, (B, A)).astype(F)
    adv, ret, ov = (rng.standard_normal(B).astype(F) for _ in range(3))
    noise = rng.normal(0, 0.1, B)
    fam = case.family
    if fam == "zero_col":
        obs[:, int(case.tag[1:])] = 0
    elif fam == "one_action":
        act[:] = cfg.action_start + int(case.tag[1:])
    elif fam == "all_actions":
        act = (np.arange(B) % A + cfg.action_start).astype(np.int32)
    elif fam == "log_std":
        flat[sl["log_std"]] = {"m3": -3.0, "p1": 1.0}[case.tag]
    fw = forward64(row, flat, obs, act, cfg.action_start)
    olp = (fw["logp"] + noise).astype(F)                                             # the _batch of the parity tests: old_logp = logp + N(0, 0.1)
    # ... with every decision definite: a ratio within 1e-3 (1 + |logp| / 64) of an edge of the clip, a value within 1e-2 clip_range_vf of one, is moved to 1.5 x that
    # distance.  An f32 evaluation (the oracle's, a kernel's) may put such a sample on the other side of the edge than float64 and be right; that is no finding
    guard = 1e-3 * (1 + np.abs(fw["logp"]) / 64)
    for edge in (1 - float(cfg.clip_range), 1 + float(cfg.clip_range)):
        dlt = fw["logp"] - olp.astype(np.float64) - math.log(edge)
        near = np.abs(dlt) < guard
        olp[near] = (fw["logp"] - math.log(edge) - np.where(dlt < 0, -1.5, 1.5) * guard)[near].astype(F)
    if cfg.has_clip_range_vf:
        cvf = float(cfg.clip_range_vf)
        for edge in (-cvf, cvf):
            dlt = fw["v"] - ov.astype(np.float64) - edge
            near = np.abs(dlt) < 1e-2 * cvf
            ov[near] = (fw["v"] - edge - np.where(dlt < 0, -1.5e-2, 1.5e-2) * cvf)[near].astype(F)
    idx = np.arange(B)
    if fam == "ind_actor":                                                           # one advantage, vf_coef = 0: the actor gradient is sample j's
        j = int(case.tag[1:])
        adv = np.zeros(B, F)
        adv[j] = F(1.5) if j % 2 else F(-1.5)
    elif fam == "ind_critic":                                                        # every value clipped away but sample j's
        j = int(case.tag[1:])
        adv = np.zeros(B, F)
        far = 10 * float(cfg.clip_range_vf) * np.where(idx % 2, 1.0, -1.0)
        ov = (fw["v"] + far).astype(F)
        ov[j] = F(fw["v"][j])
    elif fam == "decisions":                                                         # every side of both clips, both signs of the advantage, 1e-3 / 1e-2 away from the edge
        rs, ds = np.array(R_STAR(float(cfg.clip_range))), np.array(D_STAR(float(cfg.clip_range_vf)))
        olp = (fw["logp"] - np.log(rs[idx % 4])).astype(F)
        adv = np.where((idx // 4) % 2 == 0, 1.0, -1.0).astype(F)
        ov = (fw["v"] - ds[(idx // 8 + idx) % 4]).astype(F)
    elif fam == "equal_adv":
        adv = np.full(B, F(0.7))
    return flat, (obs, act, adv, ret, olp, ov)


@functools.lru_cache(maxsize=8)
def ref_of(case):
    flat, batch = inputs(case)
    return reference(case.row, _host_cfg(case.row, case.setting), flat, batch)


def expected_clip_count(case):
    """decisions family: r* is outside [1 - c, 1 + c] at slots 0 and 3 of every four"""
    idx = np.arange(case.B) % 4
    return int(np.count_nonzero((idx == 0) | (idx == 3)))


# =====================================================================================================================
# the assertion functions: (case, outputs, reference) and nothing else
# =====================================================================================================================
def ratios(case, out, ref):
    """error / (u T) per block and per statistic: the largest over the elements (inf where T = 0 and the element is not zero)"""
    loss, stats, g = out
    g = np.asarray(g, np.float64)
    assert g.shape == ref.g.shape, f"{case.name}: {g.shape} gradient elements, the layout gives {ref.g.shape}"
    assert np.all(np.isfinite(g)) and np.isfinite(loss) and np.all(np.isfinite(stats)), f"{case.name}: non-finite output"
    res = {}
    err = np.abs(g - ref.g)
    for k in BLOCKS:
        e, t = err[ref.sl[k]], ref.T[ref.sl[k]]
        if e.size:
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(e <= TINY, 0.0, e / (U * t))
            i = int(np.argmax(q))
            res[k] = (float(q[i]), i)
    got = dict(loss=float(loss), **{k: float(stats[s]) for k, s in STAT_SLOT.items()})
    want = dict(loss=ref.loss, **{k: float(ref.stats[s]) for k, s in STAT_SLOT.items()})
    for k in STATS:
        e = abs(got[k] - want[k])
        res[k] = (0.0 if e <= TINY else e / (U * ref.stat_T[k]) if ref.stat_T[k] > 0 else math.inf, 0)
    return res


def check(case, out, ref, limit=1.0, constants=None):
    """every check of one output of a case -> {block or statistic: error / bound}"""
    C = CONSTANTS if constants is None else constants
    loss, stats, g = out
    n = case.B
    res = {k: (q / C[k], i) for k, (q, i) in ratios(case, out, ref).items()}
    for k, (q, i) in res.items():
        assert q <= limit, f"{case.name}: {k}[{i}] error / bound {q:.3f} (limit {limit}); got {g[ref.sl[k]][i] if k in ref.sl else None!r}, float64 {ref.g[ref.sl[k]][i] if k in ref.sl else None!r}"
    cf = float(stats[3]) * n
    assert abs(cf - round(cf)) <= 4 * U * n and round(cf) == ref.clip_count, f"{case.name}: clip_fraction n = {cf!r}, the float64 count is {ref.clip_count}"
    sl, g = ref.sl, np.asarray(g)
    actor = np.r_[tuple(np.arange(sl[f"actor.{k}"].start, sl[f"actor.{k}"].stop) for k in NET_BLOCKS) + (np.arange(sl["log_std"].start, sl["log_std"].stop),)]
    critic = np.r_[tuple(np.arange(sl[f"critic.{k}"].start, sl[f"critic.{k}"].stop) for k in NET_BLOCKS)]
    fam = case.family
    if fam == "ind_actor":
        assert not g[critic].any(), f"{case.name}: vf_coef = 0, {np.count_nonzero(g[critic])} critic elements are not zero"
    if fam == "ind_critic":
        assert not g[actor].any(), f"{case.name}: no advantage, {np.count_nonzero(g[actor])} actor elements are not zero"
        assert ref.v_clipped.sum() == n - 1
    if fam == "equal_adv":
        assert not g[actor].any(), f"{case.name}: equal advantages normalise to zero, {np.count_nonzero(g[actor])} actor elements are not zero"
    if fam == "decisions":
        assert ref.clip_count == expected_clip_count(case)
    if fam == "zero_col":
        D, A, _ = case.row.dims
        col = int(case.tag[1:])
        for net in ("actor", "critic"):
            w1 = g[sl[f"{net}.W1"]].reshape(D, case.row.H)
            assert not w1[col].any() and g[sl[f"{net}.b1"]].any(), f"{case.name}: {net} dW1 of a zero observation column must be zero, db1 not"
    return {k: q for k, (q, i) in res.items()}


def check_same(case, out0, out1):
    """the two runs of a case on one handle: bit-identical"""
    for k, a, b in zip(("loss", "statistics", "gradient"), out0, out1):
        assert np.asarray(a, F).tobytes() == np.asarray(b, F).tobytes(), f"{case.name}: the two runs differ in the {k}"


def check_moments_paths(case, g_inline, g_launch, ref):
    """in-kernel advantage moments against the two moments launches: within 4 u T of each other, element by element"""
    d = np.abs(np.asarray(g_inline, np.float64) - np.asarray(g_launch, np.float64))
    bad = np.flatnonzero(d > 4 * U * ref.T + TINY)
    assert not bad.size, f"{case.name}: {bad.size} elements differ between the two moments paths by more than 4 u T, first {bad[:4]}"


# =====================================================================================================================
# a defect on top of an output (the mutants of tests/test_grad_cases.py)
# =====================================================================================================================
def with_defect(case, out, defect):
    """out plus the float64 difference that `defect` makes -> (out', does it change anything)"""
    flat, batch = inputs(case)
    bad, ref = reference(case.row, _host_cfg(case.row, case.setting), flat, batch, defect), ref_of(case)
    changed = bool(np.any(bad.g != ref.g) or np.any(bad.stats != ref.stats) or bad.loss != ref.loss)
    loss, stats, g = out
    if defect == "invB_tile_rounded":                                                # a scale of the gradient alone
        return (loss, stats, (g.astype(np.float64) + (bad.g - ref.g)).astype(F)), changed
    return (F(float(loss) + (bad.loss - ref.loss)), (stats.astype(np.float64) + (bad.stats - ref.stats)).astype(F), (g.astype(np.float64) + (bad.g - ref.g)).astype(F)), changed


# =====================================================================================================================
# running a row on the device / the oracle
# =====================================================================================================================
@contextlib.contextmanager
def environ(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


class RowRunner:
    """the handles of one row, one per setting, created under the row's switches"""

    def __init__(self, pkg, row, switches=True):
        self.pkg, self.row, self.switches, self.handles = pkg, row, switches, {}

    def handle(self, setting):
        if setting not in self.handles:
            from split_budget import grad_variant
            cfg = make_cfg(self.pkg._capi, self.row, setting)
            with grad_variant(self.row.variant), environ(**(self.row.env if self.switches else {k: v for k, v in self.row.env.items() if k == "DRIL_FORCE_GENERIC"})):
                self.handles[setting] = self.pkg.Handle(cfg)
        return self.handles[setting]

    def run(self, case):
        h = self.handle(case.setting)
        flat, batch = inputs(case)
        h.set_params(flat)
        out = h.ppo_loss_grad(*batch)
        info = h.grad_kernel_info()
        kernel = info.split(":")[0]
        assert kernel == self.row.kernel, f"{case.name}: {kernel} ran, the row is about {self.row.kernel}"
        m = re.search(r"; grid G=(\d+) Gc=(\d+)$", info)
        assert m, f"{case.name}: no grid in {info!r}"
        self.grid = (int(m.group(1)), int(m.group(2)))                              # what ppo_step launched: slabs (pair kernel: pairs) of the actor, of the critic
        return out

    def close(self):
        for h in self.handles.values():
            h.close()
        self.handles = {}


class OracleRunner:
    def __init__(self, oracle_mod, row):
        self.mod, self.row, self.oracles = oracle_mod, row, {}

    def oracle(self, setting):
        if setting not in self.oracles:
            self.oracles[setting] = self.mod.Oracle(_host_cfg(self.row, setting))
        return self.oracles[setting]

    def run(self, case):
        o = self.oracle(case.setting)
        flat, batch = inputs(case)
        o.set_params(flat)
        self.mod.lib().orc_set_num_threads(1)                                        # the 64-sample f32 chunks follow the thread count: one thread, one summation order
        try:
            return o.ppo_loss_grad(*batch)
        finally:
            self.mod.lib().orc_set_num_threads(self.mod.host_threads())


def worst_of(runner_factory, rows, families=None):
    """{block or statistic: the largest error / (u T)} over the cases of `rows`"""
    worst = {}
    for row in rows:
        r = runner_factory(row)
        for case in cases_of(row):
            if families and case.family not in families:
                continue
            for k, (q, i) in ratios(case, r.run(case), ref_of(case)).items():
                if case.family == "equal_adv" and (k.startswith("actor") or k == "log_std"):
                    continue                                                         # T is the one of a division by eps there: the check is "exactly zero"
                if q > worst.get(k, (0.0, ""))[0]:
                    worst[k] = (q, case.name)
        if hasattr(r, "close"):
            r.close()
    return worst


if __name__ == "__main__":
    import __graft_entry__ as g
    if sys.argv[1] == "oracle":                                                      # re-measure ORACLE_WORST
        import oracle_lib
        oracle_lib.ensure_built()
        w = worst_of(lambda row: OracleRunner(oracle_lib, row), ROWS)
        for k in BLOCKS + STATS:
            d = 10.0 ** (math.floor(math.log10(w[k][0])) - 2)                        # rounded UP to three digits
            up = float(f"{math.ceil(w[k][0] / d) * d:.3g}")
            up = up if up >= w[k][0] else float(f"{up + d:.3g}")
            print(f'    "{k}": {up:g},'.ljust(40) + f"# {w[k][1]}")
    else:                                                                            # device: the worst ratios of the random cases of the named rows, one JSON line
        pkg = g.load_package()
        res = {}
        for name in json.loads(sys.argv[1]):
            w = worst_of(lambda row: RowRunner(pkg, row), [ROW_BY_NAME[name]], ("random",))
            res[name] = {k: v[0] for k, v in w.items()}
        print(json.dumps(res))
