"""The case table of the PPO optimiser tail (dril_kernels.hip: grad_reduce_kernel, ppo_finish_small_kernel, grad_norm_kernel, adam_kernel), its buffer images, the
float64 reference of ONE step, the error bounds, a numpy float32 emulation of the kernels' own expressions and the assertion functions (test infrastructure of
tests/test_optim_cases.py and tests/test_gpu_optim.py; the driver is tests/optim_check.hip).

Routes (ppo_step / dril_apply_gradients in dril_update.hip pick one):
  A  grad_reduce_kernel -> adam_kernel (norm from norm_partials)        B  ppo_finish_small_kernel (one workgroup, P <= 16384)
  C  flat given -> grad_norm_kernel -> adam_kernel                      D  flat given -> adam_kernel with norm_from_flat = 1
A case is a layout, slab counts (G, Gc), a route and a sequence of steps.  Routes A and B of the same layout / slab counts read the SAME slab images, routes C and D
of the same layout the same flat image, so that their outputs can be held against each other.

Two operand modes:
  exact  : slab values are multiples of 1/8 (times a power of two): every summation order is exact in f32, so flat[0..P+8) must equal the float64 sums bit for bit —
           this pins the addressing;
  normal : standard-normal values times a per-parameter scale from 1e-4 .. 1, mixed signs across slabs, non-zero m and v.
Floats of a slab that no kernel may read (the padding behind log_std, the unused statistic slots) are NaN.

The reference is one float64 step from the device's OWN state before that step (the dumped f32 params, m, v, bt and flat, widened), so errors do not compound and
the bounds are those of single expressions.  With u = 2^-24:
  flat[p]   n_adds u sum_g |x_g|            n_adds = ceil(G / 32) + 31 (route A: 32 strided partial sums, then 32 in a row), G (route B: one row)
  norm      4 u relative                    (f64 sum of squares, one rounding to f32, sqrtf)
  m         8 u (|b1 m0| + |(1 - b1) g'|)   g' = the clipped gradient
  v         12 u v
  param     2 u |p'| + 16 u |step| + 8 u lr (|b1 m0| + |(1 - b1) g'|) / ((1 - bt1) den)          den = sqrt(v / (1 - bt2)) + eps
  step_stats[0..8]  8 u relative to the float64 value from the dumped flat; [9..11] exact
plus one subnormal quantum (2^-149) everywhere: no f32 result is finer than that.  tests/test_optim_cases.py holds the float32 emulation to HALF of every bound
on every case: the constants are margins of two over the arithmetic of the expressions themselves.
"""
from __future__ import annotations

import functools
import hashlib
import re
import subprocess
from dataclasses import dataclass, replace
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dril.jl_amd" / "csrc"
SENTINEL = np.float32(-7777.5)                      # tests/optim_check.hip kSentinel
GUARD = 64                                          # tests/optim_check.hip kGuard
U = 2.0 ** -24
TINY = 2.0 ** -149
F = np.float32
LR, BETA1, BETA2, EPS, ENT, VF = F(3e-4), F(0.9), F(0.999), F(1e-5), F(0.01), F(0.5)
MAX_NORM, TARGET_KL = F(0.5), F(0.25)
SAMPLE_COUNTS = (1, 64, 4096, 131077)
BUFFERS = ("norm_partials", "flat", "params", "m", "v", "bt", "norm_out", "step_stats")           # the order of a step's dump
RATIOS = ("flat", "norm", "m", "v", "param", "stats")


def r4(x):
    return (x + 3) // 4 * 4


# =====================================================================================================================
# layouts
# =====================================================================================================================
ENV = {0: (4, 2, True), 1: (3, 1, False), 6: (6, 3, True)}          # kind -> (obs dims, action dims, discrete): EnvSpec<KIND> of dril_device.h


def net_size(D, H, O):
    """{W1 b1 W2 b2 W3 b3} of one [H, H] net (net_off)"""
    return H * D + H + H * H + H + O * H + O


@dataclass(frozen=True)
class Layout:
    name: str
    Pa: int
    Pc: int
    L: int                        # log_std count: behind the actor net in the actor slab, last in flat
    kind: int = -1                # a built-in env kind, or -1: synthetic
    hidden: int = 0

    @property
    def P(self):
        return self.Pa + self.Pc + self.L

    @property
    def slab_a(self):
        return r4(self.Pa + self.L + 8)

    @property
    def slab_c(self):
        return r4(self.Pc + 8)

    @property
    def n_partials(self):
        return (self.P + 31) // 32


def real_layout(name, kind, hidden):
    D, A, discrete = ENV[kind]
    return Layout(name, net_size(D, hidden, A), net_size(D, hidden, 1), 0 if discrete else A, kind, hidden)


def synthetic(Pa, Pc, L):
    return Layout(f"s{Pa}_{Pc}_{L}", Pa, Pc, L)


CARTPOLE64, PENDULUM64, ACROBOT32 = real_layout("cartpole64", 0, 64), real_layout("pendulum64", 1, 64), real_layout("acrobot32", 6, 32)
PENDULUM128, PENDULUM256 = real_layout("pendulum128", 1, 128), real_layout("pendulum256", 1, 256)           # 16384 < P <= 65536, P > 65536
SMALL = [synthetic(1, 1, 0), synthetic(31, 1, 1), synthetic(33, 31, 3), synthetic(1000, 23, 1), synthetic(1001, 23, 1), synthetic(40, 50, 6)]
S16384 = synthetic(8000, 8383, 1)                                                                           # KMAX of route B
S33 = SMALL[2]
LAYOUTS = [CARTPOLE64, PENDULUM64, ACROBOT32, PENDULUM128, PENDULUM256] + SMALL + [S16384]
COMMON = [(1, 1), (2, 1), (31, 32), (32, 32)]
A_ONLY = [(33, 32), (64, 64), (255, 129), (384, 384)]
# (layout, slab counts of routes A and B, slab counts of route A alone): every count on the small layouts, the large ones where the images stay a few MB
SLAB_TABLE = [(l, COMMON, A_ONLY) for l in SMALL + [PENDULUM64, ACROBOT32]] + \
             [(CARTPOLE64, COMMON, [(33, 32), (384, 384)]), (S16384, COMMON, [(33, 32), (255, 129)]),
              (PENDULUM128, [(2, 1), (32, 32)], [(33, 32), (64, 64)]), (PENDULUM256, [(1, 1), (31, 32)], [(33, 32)])]


# =====================================================================================================================
# cases
# =====================================================================================================================
@dataclass(frozen=True)
class Step:
    data: str                     # "exact" | "normal"
    variant: str = ""             # a decision ("norm0625", "kl=S") or a poison (_grads, _stats, _poison)
    shift: int = 0                # every gradient times 2^-shift (12: the norm stays under max_grad_norm; -10: far above it)
    n: int = 64                   # samples of the minibatch: statistics slot 6
    parity: int = 0
    clear: int = 0
    use_stats: int = 1
    has_kl: int = 1
    target_kl: np.float32 = TARGET_KL
    has_max: int = 1
    max_norm: np.float32 = MAX_NORM


@dataclass(frozen=True)
class Case:
    name: str
    route: str
    layout: Layout
    G: int
    Gc: int
    steps: tuple
    key: str                      # names the input images: shared by the routes that read the same ones
    zero_params: bool = False

    @property
    def slabs(self):
        return self.route in "AB"

    @property
    def mode(self):
        return self.steps[0].data


def _table():
    T, k = [], 0
    for lay, common, a_only in SLAB_TABLE:
        for G, Gc in common + a_only:
            for mode in ("exact", "normal"):
                k += mode == "exact"                        # both modes of a row: the same shift, sample count and initial parameters
                st = Step(mode, shift=12 * (k % 2), n=SAMPLE_COUNTS[k // 2 % 4], has_kl=int(mode == "normal"))
                key = f"{lay.name}.g{G}x{Gc}.{mode}"
                for route in "AB":
                    if route == "B" and ((G, Gc) not in common or lay.P > 16384):
                        continue
                    T.append(Case(f"{route}.{key}", route, lay, G, Gc, (st,), key, zero_params=(k % 3 == 0)))
    for lay in LAYOUTS:                                     # flat given: the kernels take every size (in production C with statistics runs above, D up to 65536 parameters)
        for mode in ("exact", "normal"):
            k += mode == "exact"
            st = Step(mode, shift=12 * (k % 2), n=SAMPLE_COUNTS[k // 2 % 4], has_kl=int(mode == "normal"))
            key = f"{lay.name}.flat.{mode}"
            T.append(Case(f"C0.{key}", "C", lay, 1, 1, (replace(st, use_stats=0, has_kl=0),), key, zero_params=(k % 3 == 0)))        # dril_apply_gradients
            T.append(Case(f"C.{key}", "C", lay, 1, 1, (st,), key, zero_params=(k % 3 == 0)))
            T.append(Case(f"D.{key}", "D", lay, 1, 1, (st,), key, zero_params=(k % 3 == 0)))
    # ---- decisions: exactly representable inputs (gradients 0.375 and 0.5: norm 0.625; kl sum 24 over 64 samples: 0.375 = 1.5 target_kl)
    above = F(np.nextafter(F(24.0), F(np.inf)))
    dec = [("clip_eq", Step("exact", "norm0625", max_norm=F(0.625))), ("clip_above", Step("exact", "norm0625", max_norm=F(0.625 / 1.01))),
           ("clip_below", Step("exact", "norm0625", max_norm=F(0.625 * 1.01))), ("clip_off", Step("normal", "", shift=-10, has_max=0)),
           ("kl_eq", Step("normal", "kl=24", shift=12)), ("kl_above", Step("normal", f"kl={float(above)!r}", shift=12)),
           ("kl_off", Step("normal", "kl=64000", shift=12, has_kl=0))]
    poison = [("nan_actor0", True), ("nan_critic_last", True), ("nan_log_std", True), ("nan_last_slab", False), ("inf_two_slabs", False), ("overflow_3e19", True),
              ("single_1e19", True)]
    for name, st in dec:
        for route in "ABCD":
            key = f"{S33.name}.{name}"
            T.append(Case(f"{route}.{key}", route, S33, *((2, 1) if route in "AB" else (1, 1)), (replace(st, has_kl=st.has_kl if name.startswith("kl") else 0),), key))
    for lay, G, Gc in ((PENDULUM64, 31, 32), (S33, 33, 32)):
        for name, on_flat in poison:
            for route in "ABCD":
                if (route in "CD" and not on_flat) or (route == "B" and G > 32):
                    continue
                key = f"{lay.name}.g{G}x{Gc}.{name}"
                T.append(Case(f"{route}.{key}", route, lay, *((G, Gc) if route in "AB" else (1, 1)), (Step("normal", name, shift=12),), key))
    # ---- sequences: parity follows the step index; step 3 clips, 5 stops on kl, 6 is launched with the flag set, 9 is poisoned; the flag is cleared before 7 and 10
    for lay in (PENDULUM64, S33):
        steps = []
        for i in range(12):
            st = Step("normal", shift=0 if i == 3 else 12, n=SAMPLE_COUNTS[i % 4], parity=i & 1, clear=int(i in (7, 10)))
            if i == 5:
                st = replace(st, variant="kl=64000")
            if i == 9:
                st = replace(st, variant="nan_log_std")
            steps.append(st)
        for route in "ABCD":
            key = f"{lay.name}.seq"
            T.append(Case(f"{route}.{key}", route, lay, *((6, 2) if route in "AB" else (1, 1)), tuple(steps), key))
    return T


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# =====================================================================================================================
# inputs
# =====================================================================================================================
def _rng(*key):
    h = hashlib.sha256("/".join(str(k) for k in key).encode()).digest()
    return np.random.default_rng(int.from_bytes(h[:8], "little"))


@functools.lru_cache(maxsize=None)
def _scales(lay):
    """one scale per parameter, 1e-4 .. 1: gradients, m and v of a parameter share it"""
    return (10.0 ** (-4.0 * _rng(lay.name, "scales").random(lay.P))).astype(F)


def _draw(rng, shape, mode, scale):
    if mode == "exact":
        return (rng.integers(-8, 9, size=shape) / 8.0).astype(F)
    return rng.standard_normal(shape, dtype=F) * scale


STAT_SIGN = {0: 1.0, 1: -1.0, 5: 1.0}


def _stats(case, i, rng, rows, cols):
    """(rows, len(cols)) statistics columns `cols` of one net's slabs.  The loss of step_stats[7] is pl + ent_coef (-ent) + vf_coef vl: the totals of columns 0, 1, 5 are
    given the signs +, -, + so that its three terms do not cancel and a RELATIVE bound on it means something; single values keep mixed signs"""
    st = case.steps[i]
    if st.data == "exact":
        x = _draw(rng, (rows, len(cols)), "exact", None)
    else:
        x = rng.standard_normal((rows, len(cols)), dtype=F) * F(0.05 * st.n / np.sqrt(rows))      # kl = column 3 / n ~ 0.05: far below 1.5 target_kl
    for j, k in enumerate(cols):
        if k in STAT_SIGN and x[:, j].sum(dtype=np.float64) * STAT_SIGN[k] < 0:
            x[:, j] = -x[:, j]
        if k == 3 and st.variant.startswith("kl="):                # "kl=S": the kl sum is S at 64 samples, all of it in the LAST slab
            x[:, j] = 0
            x[rows - 1, j] = F(float(st.variant[3:])) * F(st.n) / F(64)
    return x


POISON_AT = {"nan_actor0": lambda l: 0, "nan_critic_last": lambda l: l.Pa + l.Pc - 1, "nan_log_std": lambda l: l.P - 1}


def _grads(case, i, rng, rows):
    """(rows, P) gradient rows in flat order, before the step's 2^-shift"""
    st, lay = case.steps[i], case.layout
    if st.variant == "norm0625":                                   # flat = 0.375 at parameter 0 (from two slabs), 0.5 at the last one: norm 0.625
        x = np.zeros((rows, lay.P), F)
        x[0, 0], x[case.G - 1, 0] = (0.25, 0.125) if case.G > 1 else (0.0, 0.375)
        x[case.G - 1, lay.P - 1] = 0.5
        return x
    return _draw(rng, (rows, lay.P), st.data, _scales(lay))


def _poison(case, i, x):
    """x: (rows, P) after the shift; rows of actor parameters (log_std included) below G, of critic parameters below Gc are used"""
    v, lay, G, Gc = case.steps[i].variant, case.layout, case.G, case.Gc
    if v in POISON_AT:
        x[(Gc if v == "nan_critic_last" else G) // 2, POISON_AT[v](lay)] = np.nan
    elif v == "nan_last_slab":
        x[G - 1, lay.Pa // 2] = np.nan
    elif v == "inf_two_slabs":
        x[0, lay.Pa // 2], x[G - 1, lay.Pa // 2] = np.inf, -np.inf
    elif v == "overflow_3e19":                                     # 16 finite gradients whose squares sum past f32
        x[0, :16] = 3e19
    elif v == "single_1e19":                                       # finite: must clip (to 0.5 on that parameter) and apply
        x[0, lay.Pa - 1] = 1e19
    return x


@functools.lru_cache(maxsize=6)
def inputs(case, i):
    """routes A, B: (actor slabs (G, slab_a), critic slabs (Gc, slab_c)); routes C, D: flat (P + 8); float32"""
    st, lay = case.steps[i], case.layout
    rng = _rng(case.key, i)
    sh = F(2.0 ** -st.shift)
    G, Gc = case.G, case.Gc
    g = _poison(case, i, _grads(case, i, rng, max(G, Gc)) * sh)
    if not case.slabs:
        flat = np.zeros(lay.P + 8, F)
        flat[:lay.P] = g[0]
        flat[lay.P:lay.P + 6] = _stats(case, i, rng, 1, range(6))[0]
        flat[lay.P + 6] = st.n
        return flat
    sa, sc = np.full((G, lay.slab_a), np.nan, F), np.full((Gc, lay.slab_c), np.nan, F)
    sa[:, :lay.Pa] = g[:G, :lay.Pa]
    sa[:, lay.Pa:lay.Pa + lay.L] = g[:G, lay.Pa + lay.Pc:]
    sc[:, :lay.Pc] = g[:Gc, lay.Pa:lay.Pa + lay.Pc]
    sa[:, lay.slab_a - 8:lay.slab_a - 3] = _stats(case, i, rng, G, range(5))
    sc[:, lay.slab_c - 8] = _stats(case, i, rng, Gc, [5])[:, 0]
    return sa, sc


def bt_powers(k):
    """(beta1^k, beta2^k) as k f32 multiplications leave them"""
    b1, b2 = F(1), F(1)
    for _ in range(k):
        b1, b2 = b1 * BETA1, b2 * BETA2
    return b1, b2


@functools.lru_cache(maxsize=4)
def initial(case):
    """params, m, v (P) and bt (4): the optimiser after five steps; the bt slot the first step WRITES holds values no step produces"""
    lay, rng = case.layout, _rng(case.layout.name, "init")
    sc = _scales(lay)
    params = np.zeros(lay.P, F) if case.zero_params else rng.standard_normal(lay.P, dtype=F) * F(0.3)
    rng = _rng(lay.name, "init-mv")
    m = rng.standard_normal(lay.P, dtype=F) * sc * F(0.5)
    v = np.maximum(np.square(rng.standard_normal(lay.P, dtype=F) * sc), F(1e-12))
    bt = np.array([0.123, 0.456, 0.123, 0.456], F)
    par = case.steps[0].parity & 1
    bt[2 * par:2 * par + 2] = bt_powers(5)
    return {"params": params, "m": m, "v": v, "bt": bt}


def _init_stem(case):
    return f"{case.layout.name}.init{'0' if case.zero_params else ''}.p{case.steps[0].parity & 1}"


def write_images(case, data_dir):
    data_dir = Path(data_dir)
    stem = _init_stem(case)
    if not (data_dir / f"{stem}.bt.bin").exists():
        for k, x in initial(case).items():
            x.tofile(data_dir / f"{stem}.{k}.bin")
    for i in range(len(case.steps)):
        if case.slabs and not (data_dir / f"{case.key}.s{i}.c.bin").exists():
            sa, sc = inputs(case, i)
            sa.tofile(data_dir / f"{case.key}.s{i}.a.bin")
            sc.tofile(data_dir / f"{case.key}.s{i}.c.bin")
        elif not case.slabs and not (data_dir / f"{case.key}.s{i}.flat.bin").exists():
            inputs(case, i).tofile(data_dir / f"{case.key}.s{i}.flat.bin")


def _bits(x):
    return int(np.asarray(x, F).view(np.uint32))


def case_lines(case):
    lay, stem = case.layout, _init_stem(case)
    out = [f"case {case.name} {case.route[0]} {lay.kind} {lay.hidden} {lay.Pa} {lay.Pc} {lay.L} {case.G} {case.Gc} {len(case.steps)} "
           f"{stem}.params.bin {stem}.m.bin {stem}.v.bin {stem}.bt.bin"]
    for i, st in enumerate(case.steps):
        files = f"{case.key}.s{i}.a.bin {case.key}.s{i}.c.bin" if case.slabs else f"{case.key}.s{i}.flat.bin -"
        out.append(f"step {st.parity} {st.clear} {st.use_stats} {st.has_kl} {st.has_max} {st.n} {_bits(st.target_kl)} {_bits(st.max_norm)} {_bits(LR)} {_bits(BETA1)} "
                   f"{_bits(BETA2)} {_bits(EPS)} {_bits(ENT)} {_bits(VF)} {files}")
    return out


def write_case_file(path, cases):
    Path(path).write_text("\n".join(line for c in cases for line in case_lines(c)) + "\n")


def read_run(case, path):
    """the dump of one run -> per step {buffer: image with its guard zones, "nan_flag", "stop_flag"}"""
    raw, lay, pos, steps = Path(path).read_bytes(), case.layout, 0, []
    sizes = {"norm_partials": lay.n_partials, "flat": lay.P + 8, "params": lay.P, "m": lay.P, "v": lay.P, "bt": 4, "norm_out": 1, "step_stats": 12}
    for _ in case.steps:
        d = {}
        for k in BUFFERS:
            dt = np.float64 if k == "norm_partials" else np.float32
            n = sizes[k] + 2 * GUARD
            d[k] = np.frombuffer(raw, dt, n, pos)
            pos += n * np.dtype(dt).itemsize
        d["nan_flag"], d["stop_flag"] = (int(x) for x in np.frombuffer(raw, np.int32, 2, pos))
        pos += 8
        steps.append(d)
    assert pos == len(raw), f"{case.name}: {len(raw)} bytes in the dump, the layout gives {pos}"
    return steps


def read_layouts(path):
    return {t[0]: tuple(int(x) for x in t[1:]) for t in (line.split() for line in Path(path).read_text().splitlines())}


# =====================================================================================================================
# the float64 reference of the reduction
# =====================================================================================================================
def columns(case, sa, sc, defect=None):
    """where flat comes from: [(first element of flat, (slabs, width) block summed over its rows)].  The log_std gradients sit behind the actor net in the actor slab
    but last in flat; the statistics are the last 8 floats of a slab, columns 0..4 from the actor's, column 5 from the first of the critic's"""
    lay = case.layout
    so = 7 if defect == "stat_slot_off" else 8
    if defect == "drop_slab":
        sa = sa[:-1]
    ls = sc[:, lay.Pc:lay.Pc + lay.L] if defect == "logstd_from_critic" else sa[:, lay.Pa:lay.Pa + lay.L]
    return [(0, sa[:, :lay.Pa]), (lay.Pa, sc[:, :lay.Pc]), (lay.Pa + lay.Pc, ls), (lay.P, sa[:, lay.slab_a - so:lay.slab_a - so + 5]),
            (lay.P + 5, sc[:, lay.slab_c - so:lay.slab_c - so + 1])]


def n_adds(route, G):
    return -(-G // 32) + 31 if route == "A" else G


def flat_reference(case, i):
    """float64 flat (P + 8) of step i from its slab images, and the bound of every element"""
    lay, st = case.layout, case.steps[i]
    ref, bound = np.zeros(lay.P + 8), np.full(lay.P + 8, TINY)
    with np.errstate(invalid="ignore"):
        for o, x in columns(case, *inputs(case, i)):
            x = x.astype(np.float64)
            ref[o:o + x.shape[1]] = x.sum(axis=0)
            bound[o:o + x.shape[1]] = n_adds(case.route, x.shape[0]) * U * np.abs(x).sum(axis=0) + TINY
    ref[lay.P + 6] = st.n
    return ref, bound


# =====================================================================================================================
# numpy float32 emulation of the kernels' expressions (and of one defect at a time: the mutants of tests/test_optim_cases.py)
# =====================================================================================================================
DEFECTS = ("drop_slab", "logstd_from_critic", "stat_slot_off", "bt_stale", "clip_m_only", "eps_in_sqrt", "clip_ge", "kl_ge", "bt_not_copied", "poison_writes_m")


def _guarded(x, dtype=np.float32):
    g = np.full(GUARD, SENTINEL, dtype)
    return np.concatenate([g, np.asarray(x, dtype).ravel(), g])


def _emulate_flat(case, i, defect):
    """flat as the route sums it: A = 32 strided partial sums per parameter, then the 32 in a row; B = one row; statistics: A f32 partials then f64, B f64"""
    lay, st = case.layout, case.steps[i]
    flat = np.zeros(lay.P + 8, F)
    with np.errstate(invalid="ignore", over="ignore"):
        for o, x in columns(case, *inputs(case, i), defect):
            Gn, w = x.shape
            if case.route == "A":
                part = np.zeros((32, w), F)
                for g in range(Gn):
                    part[g % 32] += x[g]
                if o >= lay.P:
                    tot = functools.reduce(lambda a, b: a + b, part.astype(np.float64)).astype(F)
                else:
                    tot = np.zeros(w, F)
                    for k in range(32):
                        tot = tot + part[k]
            elif o >= lay.P:
                tot = functools.reduce(lambda a, b: a + b, x.astype(np.float64), np.zeros(w)).astype(F)
            else:
                tot = np.zeros(w, F)
                for g in range(Gn):
                    tot = tot + x[g]
            flat[o:o + w] = tot
    flat[lay.P + 6] = st.n
    return flat


def emulate(case, defect=None):
    """one run of the case, in the form read_run gives"""
    lay, P = case.layout, case.layout.P
    state = {k: x.copy() for k, x in initial(case).items()}
    nan_flag = stop_flag = 0
    out = []
    one = F(1)
    for i, st in enumerate(case.steps):
        if st.clear:
            nan_flag = stop_flag = 0
        d = {"norm_partials": np.full(lay.n_partials, SENTINEL, np.float64), "flat": np.full(P + 8, SENTINEL, F) if case.slabs else inputs(case, i).copy(),
             "norm_out": np.full(1, SENTINEL, F), "step_stats": np.full(12, SENTINEL, F)}
        if not stop_flag:
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                if case.slabs:
                    d["flat"] = _emulate_flat(case, i, defect)
                flat = d["flat"]
                sq = np.square(flat[:P].astype(np.float64))
                if case.route in "AC":
                    d["norm_partials"] = np.add.reduceat(sq, np.arange(0, P, 32))
                norm = np.sqrt(F(sq.sum()))
                stf = flat[P:]
                n = stf[6] if st.use_stats else one
                kl = stf[3] / n if st.use_stats else F(0)
                bad = bool(not np.isfinite(norm))
                thr = F(1.5) * st.target_kl
                kl_stop = bool(st.use_stats and st.has_kl and (kl >= thr if defect == "kl_ge" else kl > thr))
                pl, ent, vl = stf[0] / n, stf[1] / n, stf[5] / n
                d["step_stats"] = np.array([pl, vl, -ent, stf[2] / n, kl, ent, stf[4] / n, pl + ENT * (-ent) + VF * vl, norm, 0.0 if bad or kl_stop else 1.0,
                                            1.0 if bad else 0.0, 1.0 if kl_stop else 0.0], F)
                d["norm_out"] = np.array([norm], F)
                bi, bo = 2 * (st.parity & 1), 2 * ((st.parity + 1) & 1)
                bt = state["bt"].copy()
                bt1, bt2 = bt[bi], bt[bi + 1]
                if bad:
                    nan_flag = 1
                if bad or kl_stop:
                    stop_flag = 1
                    if defect != "bt_not_copied":
                        bt[bo], bt[bo + 1] = bt1, bt2
                else:
                    bt[bo], bt[bo + 1] = bt1 * BETA1, bt2 * BETA2
                state["bt"] = bt
                if not (bad or kl_stop) or (bad and defect == "poison_writes_m"):
                    clip = st.has_max and (norm >= st.max_norm if defect == "clip_ge" else norm > st.max_norm)
                    scale = st.max_norm / norm if clip else one
                    g = flat[:P]
                    gs = g * scale if scale != one else g
                    m = BETA1 * state["m"] + (one - BETA1) * gs
                    gv = g if defect == "clip_m_only" else gs
                    v = BETA2 * state["v"] + (one - BETA2) * gv * gv
                    if defect == "bt_stale":
                        bt1, bt2 = bt1 / BETA1, bt2 / BETA2
                    den = np.sqrt(v / (one - bt2) + EPS) if defect == "eps_in_sqrt" else np.sqrt(v / (one - bt2)) + EPS
                    state["m"] = m
                    if not bad:
                        state["v"] = v
                        state["params"] = state["params"] - m / (one - bt1) / den * LR
        d.update({k: state[k].copy() for k in ("params", "m", "v", "bt")})
        d = {k: _guarded(x, np.float64 if k == "norm_partials" else np.float32) for k, x in d.items()}
        d["nan_flag"], d["stop_flag"] = nan_flag, stop_flag
        out.append(d)
    return out


# =====================================================================================================================
# the assertion functions
# =====================================================================================================================
def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def logical(case, step, k):
    """the logical part of a dumped buffer; its guard zones must hold the sentinel"""
    x = step[k]
    assert np.all(x[:GUARD] == SENTINEL) and np.all(x[-GUARD:] == SENTINEL), f"{case.name}: a guard zone of {k} was overwritten"
    return x[GUARD:-GUARD]


def _ratio(err, bound):
    err, bound = np.atleast_1d(err), np.atleast_1d(bound)
    return float(np.max(err / bound)) if err.size else 0.0


def check_step(case, i, before, flags_in, step, limit=1.0):
    """every check of step i.  before: the logical params / m / v / bt ahead of the step (the DEVICE's own, from the previous dump); flags_in: (nan_flag, stop_flag)
    ahead of it, after the step's clear.  -> {"what": worst error / bound}, the decisions taken"""
    lay, st, P, tag = case.layout, case.steps[i], case.layout.P, f"{case.name} step {i}"
    got = {k: logical(case, step, k) for k in BUFFERS}
    ratios = dict.fromkeys(RATIOS, 0.0)
    kept = {k: _same(got[k], before[k]) for k in ("params", "m", "v", "bt")}
    if flags_in[1]:                                                               # launched with stop_flag set: nothing is written anywhere
        for k in ("norm_partials", "norm_out", "step_stats") + (("flat",) if case.slabs else ()):
            assert np.all(got[k] == SENTINEL), f"{tag}: {k} written although stop_flag was set"
        assert case.slabs or _same(got["flat"], inputs(case, i)), f"{tag}: flat changed"
        assert all(kept.values()), f"{tag}: {[k for k, same in kept.items() if not same]} changed although stop_flag was set"
        assert (step["nan_flag"], step["stop_flag"]) == tuple(flags_in), f"{tag}: flags changed"
        return ratios, {"launched_stopped": True}

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        # ---- the reduction
        if case.slabs:
            ref, bound = flat_reference(case, i)
            fin = np.isfinite(ref)
            assert _same(np.isnan(got["flat"]), np.isnan(ref)) and np.array_equal(got["flat"][~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), f"{tag}: non-finite sums differ"
            err = np.abs(got["flat"][fin].astype(np.float64) - ref[fin])
            if st.data == "exact":
                assert not err.any(), f"{tag}: exact operands, {np.count_nonzero(err)} elements of flat differ from float64, first at {np.flatnonzero(got['flat'].astype(np.float64) != ref)[:4]}"
            ratios["flat"] = _ratio(err, bound[fin])
            assert ratios["flat"] <= limit, f"{tag}: flat error / bound {ratios['flat']:.3f}"
        else:
            assert _same(got["flat"], inputs(case, i)), f"{tag}: flat changed"
        f = got["flat"].astype(np.float64)
        # ---- the norm
        sq = np.square(f[:P])
        sumsq = sq.sum()
        bad = bool(not np.isfinite(F(sumsq)))
        norm = np.sqrt(sumsq)
        norm_out = float(got["norm_out"][0])
        if bad:
            assert (np.isnan(norm_out) if np.isnan(sumsq) else norm_out == np.inf), f"{tag}: norm_out {norm_out}, float64 {norm}"
        else:
            ratios["norm"] = _ratio(abs(norm_out - norm), 4 * U * norm + TINY)
            assert ratios["norm"] <= limit, f"{tag}: norm {norm_out!r}, float64 {norm!r}: error / bound {ratios['norm']:.3f}"
        if case.route in "AC":
            want = np.add.reduceat(sq, np.arange(0, P, 32))
            ok = np.abs(got["norm_partials"] - want) <= 64 * 2.0 ** -53 * want
            assert np.all(ok | (np.isnan(want) & np.isnan(got["norm_partials"])) | (np.isinf(want) & (want == got["norm_partials"]))), f"{tag}: norm_partials"
        else:
            assert np.all(got["norm_partials"] == SENTINEL), f"{tag}: norm_partials written by a route that has none"
        # ---- statistics and decisions
        stf = f[P:]
        n = stf[6] if st.use_stats else 1.0
        kl = stf[3] / n if st.use_stats else 0.0
        kl_stop = bool(st.use_stats and st.has_kl and kl > 1.5 * float(st.target_kl))
        pl, ent, vl = stf[0] / n, stf[1] / n, stf[5] / n
        want = np.array([pl, vl, -ent, stf[2] / n, kl, ent, stf[4] / n, pl + float(ENT) * (-ent) + float(VF) * vl])
        ratios["stats"] = _ratio(np.abs(got["step_stats"][:8] - want), 8 * U * np.abs(want) + TINY)
        assert ratios["stats"] <= limit, f"{tag}: step_stats {got['step_stats'][:8]}, float64 {want}: error / bound {ratios['stats']:.3f}"
        assert _same(got["step_stats"][8:9], got["norm_out"]), f"{tag}: step_stats[8] is not norm_out"
        flags = [0.0 if bad or kl_stop else 1.0, 1.0 if bad else 0.0, 1.0 if kl_stop else 0.0]
        assert list(got["step_stats"][9:]) == flags, f"{tag}: step_stats[9..11] {got['step_stats'][9:]}, expected {flags} (applied, not finite, kl stop)"
        assert step["nan_flag"] == (1 if bad else flags_in[0]), f"{tag}: nan_flag {step['nan_flag']}"
        assert step["stop_flag"] == (1 if bad or kl_stop else 0), f"{tag}: stop_flag {step['stop_flag']}"
        # ---- bt: read from slot (parity & 1), written to the other one
        bi, bo = 2 * (st.parity & 1), 2 * ((st.parity + 1) & 1)
        assert _same(got["bt"][bi:bi + 2], before["bt"][bi:bi + 2]), f"{tag}: the bt slot the step reads changed"
        bt1, bt2 = (float(x) for x in before["bt"][bi:bi + 2])
        decisions = {"bad": bad, "kl_stop": kl_stop, "clip": False, "norm": float(norm), "kl": float(kl)}
        if bad or kl_stop:
            assert _same(got["bt"][bo:bo + 2], before["bt"][bi:bi + 2]), f"{tag}: bt not carried over a skipped step: {got['bt']}"
            assert kept["params"] and kept["m"] and kept["v"], f"{tag}: {[k for k in ('params', 'm', 'v') if not kept[k]]} changed on a skipped step"
            return ratios, decisions
        assert _same(got["bt"][bo:bo + 2], before["bt"][bi:bi + 2] * np.array([BETA1, BETA2], F)), f"{tag}: bt {got['bt']} from {before['bt']}"
        # ---- clip + Adam, float64 from the device's own state
        b1, b2, eps, lr, mx = float(BETA1), float(BETA2), float(EPS), float(LR), float(st.max_norm)
        clip = bool(st.has_max and norm > mx)
        decisions["clip"] = clip
        g = f[:P] * (mx / norm) if clip else f[:P]
        m0, v0, p0 = (before[k].astype(np.float64) for k in ("m", "v", "params"))
        msum = np.abs(b1 * m0) + np.abs((1 - b1) * g)
        m, v = b1 * m0 + (1 - b1) * g, b2 * v0 + (1 - b2) * g * g
        den = np.sqrt(v / (1 - bt2)) + eps
        stepv = lr * m / (1 - bt1) / den
        p = p0 - stepv
        ratios["m"] = _ratio(np.abs(got["m"] - m), 8 * U * msum + TINY)
        ratios["v"] = _ratio(np.abs(got["v"] - v), 12 * U * v + TINY)
        ratios["param"] = _ratio(np.abs(got["params"] - p), 2 * U * np.abs(p) + 16 * U * np.abs(stepv) + 8 * U * lr * msum / ((1 - bt1) * den) + TINY)
        for k in ("m", "v", "param"):
            assert ratios[k] <= limit, f"{tag}: {k} error / bound {ratios[k]:.3f}"
    return ratios, decisions


def check_case(case, run0, run1, limit=1.0):
    """every check of a case on the two runs of it -> worst error / bound per quantity, the decisions of every step"""
    for i, (s0, s1) in enumerate(zip(run0, run1)):
        for k in BUFFERS:
            assert _same(s0[k], s1[k]), f"{case.name} step {i}: the two runs differ in {k}"
        assert (s0["nan_flag"], s0["stop_flag"]) == (s1["nan_flag"], s1["stop_flag"]), f"{case.name} step {i}: the two runs differ in the flags"
    before, flags = initial(case), (0, 0)
    worst, decisions = dict.fromkeys(RATIOS, 0.0), []
    for i, st in enumerate(case.steps):
        if st.clear:
            flags = (0, 0)
        r, d = check_step(case, i, before, flags, run0[i], limit)
        worst = {k: max(worst[k], r[k]) for k in RATIOS}
        decisions.append(d)
        before = {k: logical(case, run0[i], k) for k in ("params", "m", "v", "bt")}
        flags = (run0[i]["nan_flag"], run0[i]["stop_flag"])
    return worst, decisions


# =====================================================================================================================
# the driver
# =====================================================================================================================
def driver_flags():
    """the flags dril_kernels.hip is built with in the library: csrc/Makefile CXXFLAGS plus KERNELS_EXTRA"""
    import gemm_cases
    m = re.search(r"^KERNELS_EXTRA \?= (.*)$", (CSRC / "Makefile").read_text(), re.M)
    return gemm_cases.driver_flags() + m.group(1).split()


def build_driver():
    """compiles tests/optim_check.hip (about 80 s) into build/optim_check/, once per content of its sources and flags"""
    src = ROOT / "tests" / "optim_check.hip"
    deps = [src, CSRC / "dril_kernels.hip"] + sorted(CSRC.glob("*.h")) + sorted((ROOT / "include").rglob("*.h"))
    flags = driver_flags()
    h = hashlib.sha256(" ".join(flags).encode())
    for d in deps:
        h.update(d.read_bytes())
    out = ROOT / "build" / "optim_check" / f"optim_check-{h.hexdigest()[:16]}"
    if not out.exists():
        out.parent.mkdir(parents=True, exist_ok=True)
        tmp = out.with_suffix(".tmp")
        subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-I", str(CSRC), "-o", str(tmp), str(src)], check=True)
        tmp.replace(out)
    return out
