"""The cases of the one-launch update of a generic handle (dril_update_fused_enable, docs/generic_update.md): the table, the inputs, a float64 restatement of one
update (f64_ppo_update of test_oracle_crosschecks.py, extended here by the statistics, the target_kl stop and the non-finite stop of ppo.jl:213-239) and the bounds.
tests/test_generic_update_cases.py holds the table to its own terms on the CPU; tests/test_gpu_generic_update.py runs it on the device.

Every case is a DRIL_ENV_EXTERNAL handle whose rollout buffer is set by set_buffer: the update is the only thing that runs."""
import numpy as np

ACT = dict(tanh=0, relu=1, sigmoid=2, elu=3, leakyrelu=4, softplus=5, gelu=6, swish=7)

# the tolerances of tests/test_gpu_external.py::test_external_edge_sizes_and_control_flow (one short update against the oracle) ...
LOSS_REL, LOSS_ABS, GNORM_REL, PARAM_RTOL, PARAM_ATOL = 2e-4, 1e-6, 1e-3, 3e-4, 3e-6
# ... and of tests/test_gpu_parity.py::test_configs0_readme_quickstart_matches_oracle: the short-update tolerance (256 optimiser steps) and the float64 yardstick rule
SHORT_RTOL, SHORT_ATOL = 2e-4, 1e-5


def yardstick_bound(r_f32, r_orc):
    """how far from the float64 loop an update may sit: three times the reference's own precision (the same loop in Float32) or the oracle's distance"""
    return max(3.0 * r_f32, 3.0 * r_orc, 1e-5)


def case(name, D, A, discrete, hidden, act, B, E, T, epochs=1, seed=0, **kw):
    return dict(name=name, D=D, A=A, discrete=discrete, hidden=tuple(hidden), act=act, B=B, E=E, T=T, epochs=epochs, seed=seed, kw=kw)


def _both_vf(c):
    """the case with has_clip_range_vf off and on"""
    on = dict(c, name=c["name"] + "-vfclip", kw=dict(c["kw"], has_clip_range_vf=1, clip_range_vf=0.3))
    return [c, on]


# 1. one optimiser step (epochs = 1, one minibatch): the smallest shapes at which the kernel takes another path — one layer and four, widths that are no multiple of
#    the 4-unit blocks, one and two sample tiles, a ragged tile, both heads, action_start 0 and 1, activations differentiated by their output and by their pre-activation
ONE_STEP = sum((_both_vf(c) for c in [
    case("d1a2-5-tanh", 1, 2, True, [5], "tanh", 2, 1, 2, ent_coef=0.01),
    case("d5a3-16x24-relu-as0", 5, 3, True, [16, 24], "relu", 7, 1, 7, ent_coef=0.01, action_start=0),
    case("d5a3-16x24-relu-as1", 5, 3, True, [16, 24], "relu", 7, 1, 7, ent_coef=0.01, action_start=1),
    case("d12a3box-64x64-tanh", 12, 3, False, [64, 64], "tanh", 64, 4, 16, ent_coef=0.01),
    case("d16a8box-7x9x11x13-gelu", 16, 8, False, [7, 9, 11, 13], "gelu", 33, 3, 11, ent_coef=0.01),
    case("d3a1box-64-swish", 3, 1, False, [64], "swish", 64, 8, 8, ent_coef=0.01),
]), [])
# ... and the four remaining activations, whose derivatives the kernel takes from the same new function (a ragged two-tile minibatch, widths off the 4-unit blocks)
ONE_STEP += [
    case("d5a3-18x10-sigmoid", 5, 3, True, [18, 10], "sigmoid", 37, 1, 37, ent_coef=0.01),
    case("d7a2box-18x10-elu", 7, 2, False, [18, 10], "elu", 37, 1, 37, ent_coef=0.01),
    case("d5a3-18x10x6-leakyrelu", 5, 3, True, [18, 10, 6], "leakyrelu", 37, 1, 37, ent_coef=0.01),
    case("d7a2box-18x10-softplus", 7, 2, False, [18, 10], "softplus", 37, 1, 37, ent_coef=0.01, has_clip_range_vf=1, clip_range_vf=0.3),
]

# 2. control flow: the five edge configurations of test_external_edge_sizes_and_control_flow
CONTROL = [
    case("partial-larger-than-buffer", 5, 3, True, [16, 24], "tanh", 10, 1, 3, epochs=2, seed=13),
    case("ragged-last-minibatch", 5, 3, True, [16, 24], "tanh", 7, 5, 4, epochs=2, seed=54),
    case("kl-stop-before-first-apply", 5, 3, True, [16, 24], "tanh", 6, 3, 2, epochs=2, seed=32, has_target_kl=1, target_kl=1e-6),
    case("zero-epochs", 5, 3, True, [16, 24], "tanh", 4, 2, 2, epochs=0, seed=22),
    case("no-clip-no-norm", 5, 3, True, [16, 24], "tanh", 20, 4, 5, epochs=2, seed=45, has_max_grad_norm=0, normalize_advantage=0),
]
# ... and a target_kl that stops in the middle of the second epoch (kl_mid_case picks it from the oracle's per-step KL values)
KL_MID = case("kl-stop-mid-second-epoch", 5, 3, True, [16, 24], "tanh", 8, 8, 8, epochs=3, seed=7, learning_rate=3e-3, logp_noise=0.02)
# 3. launch boundaries: 14 optimiser steps (odd and even Adam parity), a ragged last minibatch
CHUNKS = case("fourteen-steps", 5, 3, False, [16, 24], "tanh", 8, 4, 13, epochs=2, seed=3, ent_coef=0.01)
# 4. the README shape: reacher3's spaces, PPO() defaults
README = case("readme", 12, 3, False, [64, 64], "tanh", 64, 4, 2048, epochs=10, seed=5)
README_SHORT = dict(README, name="readme-256", epochs=2)
# 5. launch count: the same case at one and at four epochs
COUNT = [case("count-1", 5, 3, True, [16, 24], "relu", 16, 4, 16, epochs=1, seed=9), case("count-4", 5, 3, True, [16, 24], "relu", 16, 4, 16, epochs=4, seed=9)]
# 6. / 7. / 9. three updates in a row, off means off, a NaN advantage
SEQUENCE = case("sequence", 12, 3, False, [32, 48], "relu", 32, 4, 32, epochs=2, seed=11, ent_coef=0.01)
NAN_CASE = case("nan-advantage", 5, 3, True, [16, 24], "tanh", 8, 4, 8, epochs=2, seed=17)

ALL = ONE_STEP + CONTROL + [CHUNKS, README_SHORT, README] + COUNT + [SEQUENCE]


def n_of(c):
    return c["E"] * c["T"]


def make_cfg(capi, c, **over):
    cfg = capi.default_config(capi.ENV_EXTERNAL)
    cfg.ext_obs_dim, cfg.ext_action_dim, cfg.ext_discrete = c["D"], c["A"], int(c["discrete"])
    cfg.ext_action_low, cfg.ext_action_high = -1.0, 1.0
    cfg.n_hidden = len(c["hidden"])
    for l, w in enumerate(c["hidden"]):
        cfg.hidden[l] = w
    cfg.hidden1, cfg.hidden2 = c["hidden"][0], c["hidden"][min(1, len(c["hidden"]) - 1)]
    cfg.activation = ACT[c["act"]]
    cfg.n_envs, cfg.n_steps, cfg.batch_size, cfg.epochs = c["E"], c["T"], c["B"], c["epochs"]
    for k, v in dict(c["kw"], **over).items():
        if k != "logp_noise":
            setattr(cfg, k, v)
    return cfg


def param_count(c):
    net = lambda out: sum((i + 1) * o for i, o in zip((c["D"],) + c["hidden"], c["hidden"] + (out,)))
    return net(c["A"]) + net(1) + (0 if c["discrete"] else c["A"])


def make_params(c, scale=0.3):
    return (np.random.default_rng(1000 + c["seed"]).standard_normal(param_count(c)) * scale).astype(np.float32)


def make_data(capi, c, oracle):
    """the rollout buffer of the case: observations, actions, advantages, returns, old values ~ N(0, 1); old log-probabilities = the policy's own + N(0, logp_noise).
    `oracle` holds the case's parameters"""
    rng = np.random.default_rng(c["seed"]); N = n_of(c); D, A = c["D"], c["A"]
    start = c["kw"].get("action_start", 1)
    bufs = {capi.BUF_OBSERVATIONS: rng.standard_normal((N, D)).astype(np.float32),
            capi.BUF_ACTIONS: (rng.integers(0, A, N) + start).astype(np.int32) if c["discrete"] else rng.normal(0, 1, (N, A)).astype(np.float32),
            capi.BUF_ADVANTAGES: rng.standard_normal(N).astype(np.float32), capi.BUF_RETURNS: rng.standard_normal(N).astype(np.float32),
            capi.BUF_VALUES: rng.standard_normal(N).astype(np.float32)}
    lp = oracle.evaluate_actions(bufs[capi.BUF_OBSERVATIONS], bufs[capi.BUF_ACTIONS])[1]
    bufs[capi.BUF_LOGPROBS] = (lp + rng.normal(0, c["kw"].get("logp_noise", 0.2), N)).astype(np.float32)
    return bufs


def make_perm(c, salt=0):
    N = n_of(c)
    return np.stack([np.random.default_rng(100 * salt + e).permutation(N) for e in range(c["epochs"])]).astype(np.int64) if c["epochs"] else None


def load(target, capi, bufs, perm):
    for which, arr in bufs.items():
        target.set_buffer(which, arr)
    if perm is not None:
        target.set_permutation(perm)


def buf_tuple(capi, c, bufs):
    N = n_of(c)
    return tuple(bufs[w].reshape(N, -1) if w == capi.BUF_OBSERVATIONS else (bufs[w].reshape(N, -1) if (w == capi.BUF_ACTIONS and not c["discrete"]) else bufs[w].reshape(N))
                 for w in (capi.BUF_OBSERVATIONS, capi.BUF_ACTIONS, capi.BUF_ADVANTAGES, capi.BUF_RETURNS, capi.BUF_LOGPROBS, capi.BUF_VALUES))


def f64_update(flat, cfg, bufs, perm, discrete, A, dtype=np.float64):
    """f64_ppo_update (tests/test_oracle_crosschecks.py) with what dril_ppo_update reports beside the parameters: the order of ppo.jl:207-239 per optimiser step —
    gradient, non-finite check (stop, nothing applied), global norm, clip, target_kl check (skip this apply and stop), Adam — and the means of ppo.jl:242-264.
    Returns dict(params, loss, grad_norm, n_updates, early_stopped, nan_or_inf, kl = the per-step approx KL values)"""
    import torch
    from test_oracle_crosschecks import torch_ppo_loss
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    obs, act, adv, ret, lp, val = bufs
    p = np.asarray(flat, dtype).copy(); m = np.zeros_like(p); v = np.zeros_like(p)
    b1, b2, t = dtype(cfg.adam_beta1), dtype(cfg.adam_beta2), 0
    one, lr, eps = dtype(1), dtype(cfg.learning_rate), dtype(cfg.adam_eps)
    N, B = adv.shape[0], int(cfg.batch_size)
    losses, norms, kls, stopped, nan = [], [], [], 0, 0
    for ep in range(0 if perm is None else perm.shape[0]):
        for k in range(0, N, B):
            idx = perm[ep, k:k + B]
            loss, stats, g = torch_ppo_loss(p, cfg, obs[idx], act[idx], adv[idx], ret[idx], lp[idx], val[idx], discrete, A, tdt)
            norm = np.sqrt((g * g).sum(dtype=dtype))
            if not np.isfinite(norm):
                nan = 1; break
            kls.append(float(stats[4])); norms.append(float(norm))
            if cfg.has_target_kl and stats[4] > 1.5 * cfg.target_kl:
                stopped = 1; break
            if cfg.has_max_grad_norm and norm > cfg.max_grad_norm:
                g = g * (dtype(cfg.max_grad_norm) / norm)
            t += 1; losses.append(loss)
            m = b1 * m + (one - b1) * g; v = b2 * v + (one - b2) * g * g
            p = p - lr * (m / (one - b1 ** dtype(t))) / (np.sqrt(v / (one - b2 ** dtype(t))) + eps)
        if stopped or nan:
            break
    return dict(params=p, loss=float(np.mean(losses)) if losses else 0.0, grad_norm=float(np.mean(norms)) if norms else 0.0, n_updates=t, early_stopped=stopped,
                nan_or_inf=nan, kl=kls)


_CACHE = {}


def reference(oracle_mod, capi, c, with_f32=False):
    """the case's inputs and what the oracle and the float64 loop make of them, computed once per process and shared by the tests (never modified by them):
    dict(cfg, flat, bufs, perm, stats = the oracle's dril_ppo_stats, params = the oracle's parameters, f64 = f64_update's dict, f32 = the same loop in Float32)"""
    key = (c["name"], tuple(sorted(c["kw"].items())))
    r = _CACHE.get(key)
    if r is None:
        cfg = make_cfg(capi, c)
        o = oracle_mod.Oracle(cfg)
        flat = make_params(c); o.set_params(flat)
        bufs = make_data(capi, c, o); perm = make_perm(c)
        load(o, capi, bufs, perm)
        stats = o.ppo_update()
        r = dict(cfg=cfg, flat=flat, bufs=bufs, perm=perm, stats=stats, rc=o.last_rc, params=o.get_params(),
                 f64=f64_update(flat, cfg, buf_tuple(capi, c, bufs), perm, c["discrete"], c["A"]))
        _CACHE[key] = r
    if with_f32 and "f32" not in r:
        r["f32"] = f64_update(r["flat"], r["cfg"], buf_tuple(capi, c, r["bufs"]), r["perm"], c["discrete"], c["A"], dtype=np.float32)
    return r


def distances(r, dev_params):
    """relative distance from the float64 update of: the device, the oracle, the Float32 loop"""
    p0 = r["flat"].astype(np.float64)
    d64 = r["f64"]["params"] - p0; n64 = np.linalg.norm(d64)
    return tuple(np.linalg.norm((np.asarray(x, np.float64) - p0) - d64) / n64 for x in (dev_params, r["params"], r["f32"]["params"]))


def kl_mid_case(oracle_mod, capi):
    """KL_MID with target_kl chosen from the float64 loop's per-step KL values of the run WITHOUT a stop: the first step s* inside the second epoch (not its first
    minibatch) whose KL is above 1.3 x every earlier step's; 1.5 target_kl = the geometric mean of that KL and the largest earlier one, so the stop is more than
    rounding (>= 14 %) away from both.  Returns (case, s*)"""
    if "klmid" not in _CACHE:
        free = reference(oracle_mod, capi, KL_MID)
        kl = np.asarray(free["f64"]["kl"]); nb = -(-n_of(KL_MID) // KL_MID["B"])
        pick = None
        for s in range(nb + 1, 2 * nb):
            if kl[s] > 1.3 * kl[:s].max():
                pick = s; break
        assert pick is not None, ("no step of the second epoch stands out", kl[:2 * nb])
        target = float(np.sqrt(kl[pick] * kl[:pick].max()) / 1.5)
        _CACHE["klmid"] = (dict(KL_MID, name="kl-stop-mid-second-epoch-armed", kw=dict(KL_MID["kw"], has_target_kl=1, target_kl=target)), pick)
    return _CACHE["klmid"]
