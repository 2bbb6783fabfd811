"""CPU: the one-launch normalised collection (dril_norm_rollout_enable, docs/normalized_rollout.md) — the Python keyword plumbing, the Julia shim's new ccalls, and why
rollout_norm_kernel reproduces the step-granular path's summation tree instead of picking its own."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


class _FakeHandle:
    def __init__(self):
        self.calls = []

    def norm_rollout_enable(self, on=True):
        self.calls.append(on)


def test_keyword_reaches_the_bound_handle(pkg):
    """NormalizeWrapperEnv(env, fused_rollout=True) is recorded on the env, is part of bind's key, and is applied to every freshly created handle — which is all
    train_ and train_population_ do with an env before they collect"""
    env = pkg.NormalizeWrapperEnv(pkg.DeviceParallelEnv(pkg.PendulumEnv(), 4), clip_obs=5.0, fused_rollout=True)
    assert env.norm_fused_rollout is True and env._bind_extra() is True
    assert env._kw["normalize"]["clip_obs"] == 5.0 and "fused_rollout" not in env._kw["normalize"]          # the wrapper's own keywords stay what make_config reads
    cfg = pkg.make_config(env.env, env.n_envs, pkg.PPO(), None, seed=env.seed, **env._kw)
    assert cfg.norm_obs == 1 and cfg.norm_reward == 1 and cfg.norm_training == 1 and cfg.clip_obs == 5.0
    h = _FakeHandle(); env._after_create(h)
    assert h.calls == [True]
    plain = pkg.NormalizeWrapperEnv(pkg.DeviceParallelEnv(pkg.PendulumEnv(), 4))
    assert plain.norm_fused_rollout is False and plain._bind_extra() is False
    h = _FakeHandle(); plain._after_create(h)
    assert h.calls == []
    again = pkg.NormalizeWrapperEnv(env)                                                                     # wrapping again without the keyword takes the request back
    assert again is env and env.norm_fused_rollout is False
    with pytest.raises(TypeError, match="fused_rollout"):
        pkg.NormalizeWrapperEnv(pkg.DeviceParallelEnv(pkg.PendulumEnv(), 4), norm_obs=False, norm_reward=False, fused_rollout=True)


def test_capi_declares_the_verbs(pkg):
    capi = pkg._capi
    assert {"dril_norm_rollout_enable", "dril_norm_rollout_info"} <= set(capi.EXPORTED_SYMBOLS)
    import ctypes as C
    assert C.sizeof(capi.DrilNormRolloutInfo) == 4 * 4 + 2 * 8 + 256                                          # struct dril_norm_rollout_report, include/dril_hip.h
    hdr = (ROOT / "include" / "dril_hip.h").read_text()
    assert "dril_norm_rollout_enable(dril_handle* h, int32_t on);" in hdr and "dril_norm_rollout_info(const dril_handle* h, dril_norm_rollout_report* out);" in hdr


def test_julia_shim_checks_with_the_new_symbols():
    src = (ROOT / "dril.jl_amd" / "julia" / "DRiLHIP.jl").read_text()
    assert ":dril_norm_rollout_enable" in src and ":dril_norm_rollout_info" in src and "fused_rollout::Bool = false" in src
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "check_shim: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _tree_sum(x, E):
    """norm_step_kernel's sum of E <= 256 values in one block of 256: thread e holds 0 + x[e] (0 beyond E); block_sum_f64 = the xor butterfly d = 32 .. 1 inside each
    wave of 64 lanes, then 0 + w0 + w1 + w2 + w3 in wave order.  rollout_norm_kernel runs exactly this on v[lane + 64 w]"""
    v = np.zeros(256, np.float64); v[:E] = x
    idx = np.arange(64)
    total = np.float64(0.0)
    for w in range(4):
        lane = v[64 * w:64 * w + 64].copy()
        for d in (32, 16, 8, 4, 2, 1):
            lane = lane + lane[idx ^ d]
        assert (lane == lane[0]).all()                       # the butterfly leaves the same bits in every lane
        total = total + lane[0]
    return total


def _batch_var_f32(s, q, n):
    bm = s / n
    return np.float32(max(q / n - bm * bm, 0.0))


def test_summation_order_can_change_the_float32_statistic():
    """the batch variance q / n - (s / n)^2 of observations with a large mean and a small spread cancels most of the float64 sums' digits: the tree above and the plain
    left-to-right float64 sum then differ in the float32 variance that enters the running statistics.  So 'any deterministic order' is not enough for bit-equality with
    the step-granular path: the kernel has to run that path's own tree"""
    rng = np.random.default_rng(0)
    E = 128
    differ = 0
    for _ in range(200):
        x = (100.0 + 1e-3 * rng.standard_normal(E)).astype(np.float32).astype(np.float64)
        sq = x * x                                          # exact: products of two float32 values fit a float64
        s_tree, q_tree = _tree_sum(x, E), _tree_sum(sq, E)
        s_seq = q_seq = np.float64(0.0)
        for e in range(E):
            s_seq = s_seq + x[e]; q_seq = q_seq + sq[e]
        assert abs(s_tree - s_seq) <= 1e-12 * abs(s_seq) and abs(q_tree - q_seq) <= 1e-12 * abs(q_seq)   # the same sums, up to float64 rounding
        differ += _batch_var_f32(s_tree, q_tree, E) != _batch_var_f32(s_seq, q_seq, E)
    assert differ > 0, "the two orders gave the same float32 variance on every draw"
    # ragged sizes: lanes beyond E add zeros, a wave of zeros adds zero
    x = rng.standard_normal(33)
    assert _tree_sum(x, 33) == _tree_sum(np.concatenate([x, np.zeros(31)]), 64)
