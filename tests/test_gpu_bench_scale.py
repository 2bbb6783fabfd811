"""GPU (-m gpu): the CPU oracle at the sizes bench.py measures — BASELINE configs[1] / configs[2]: 65 536 envs x 2048 steps = 2^27 samples, minibatches of 4 194 304.

(1) dril_ppo_loss_grad at the bench's minibatch size directly against orc_ppo_loss_grad, the exact-f32 kernel's distance beside the selected kernel's;
(2) a full-size rollout with real episodes against block oracles (tests/bench_scale.py: 64 envs with rank = r play envs [64 r, 64 r + 64)) for the blocks holding
    env 0, env 65 535 and every env with a row on a 2^31- / 2^32-byte offset of a device buffer (tests/diag/buffer_boundaries.py);
(3) the update the bench runs (32 minibatches in the device's own DataLoader order, pos0 up to 31 x 4 194 304, the perm32 index array and the in-kernel bijection)
    against orc_ppo_update on the device's own buffers (CartPole: the whole epoch), and for Acrobot — the only config whose packed records pass 2^32 bytes — against
    the oracle on host-gathered minibatches at learning rate 0.

Nearly all of the time is the oracle's (oracle_lib.host_threads() threads).  One full-size handle at a time; full-size host copies are freed as soon as they are sliced.
What stays uncompared at full size: configs[2] WITH NormalizeWrapperEnv (its running statistics couple all envs, so no block oracle reproduces them) and multi-rank runs.
"""
import time

import numpy as np
import pytest

import bench_scale
import split_budget
from test_gpu_parity import _cfg, _flip_report, _params

pytestmark = pytest.mark.gpu
E_FULL, T_FULL = 65536, 2048
EXPECTED = {64: "ppo_grad_pair_kernel", 128: "ppo_grad_wide_split_kernel", 256: "ppo_grad_wide_split_kernel"}
F32_KERNEL = {64: "ppo_grad_kernel", 128: "ppo_grad_wide_kernel", 256: "ppo_grad_wide_kernel"}
UPDATE_BUFS = ("BUF_OBSERVATIONS", "BUF_ACTIONS", "BUF_ADVANTAGES", "BUF_RETURNS", "BUF_LOGPROBS", "BUF_VALUES")
STATS = ("policy_loss", "value_loss", "entropy_loss", "approx_kl_div", "clip_fraction", "loss", "grad_norm", "explained_variance", "ratio_first")


def _batch(oracle, cfg, B, seed):
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-1, 1, (B, oracle.D)).astype(np.float32)
    act = (rng.integers(0, oracle.A, B) + cfg.action_start).astype(np.int32) if oracle.discrete else rng.normal(0, 1, (B, oracle.A)).astype(np.float32)
    adv, ret, ov = (rng.standard_normal(B).astype(np.float32) for _ in range(3))
    _, lp, _ = oracle.evaluate_actions(obs, act)
    return obs, act, adv, ret, (lp + rng.normal(0, 0.1, B)).astype(np.float32), ov


# ---- (1) loss and gradient at the bench's minibatch size -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,H,B,variant", [
    (0, 64, 4194304, "default"),            # configs[1]'s minibatch on ppo_grad_pair_kernel: 256 tiles per pair, the multi-trip loop
    (6, 64, 4194304 + 77, "ent_vfclip"),    # Acrobot: three-quad records, value clip (the old values by LDS-DMA), a ragged last tile
    (1, 256, 1048576, "default"),           # configs[2]'s shape on ppo_grad_wide_split_kernel (a quarter of its minibatch: the oracle needs ~13 s for it on 8 threads)
    (0, 128, 1048576 + 19, "ent_vfclip"),   # the other wide instance
])
def test_bench_minibatch_loss_and_gradient_vs_oracle(pkg, oracle_mod, kind, H, B, variant):
    """dril_ppo_loss_grad with the library's own kernel selection against orc_ppo_loss_grad (OpenMP, float64 accumulation), at the tolerances of the small tests; the
    exact-f32 kernel (DRIL_GRAD_VARIANT=0) on the same input is printed beside it, so that what the f32 slab accumulation over millions of samples costs is seen"""
    t0 = time.time()
    kw = dict(n_envs=2, n_steps=2, batch_size=2, hidden1=H, hidden2=H)
    if variant == "ent_vfclip":
        kw.update(ent_coef=0.01, has_clip_range_vf=1, clip_range_vf=0.3, clip_range=0.1)
    cfg = _cfg(pkg, kind, **kw)
    h, o = pkg.Handle(cfg), oracle_mod.Oracle(cfg)
    with split_budget.grad_variant(0):
        h0 = pkg.Handle(cfg)
    flat = (np.random.default_rng(50 + kind).standard_normal(h.P) * (0.25 if H == 64 else 0.08)).astype(np.float32)
    for x in (h, h0, o):
        x.set_params(flat)
    batch = _batch(o, cfg, B, 3)
    lh, sh, gh = h.ppo_loss_grad(*batch)
    assert h.grad_kernel_info().split(":")[0] == EXPECTED[H]
    lh2, _, gh2 = h.ppo_loss_grad(*batch)
    l0, s0, g0 = h0.ppo_loss_grad(*batch)
    assert h0.grad_kernel_info().split(":")[0] == F32_KERNEL[H]
    h.close(); h0.close()
    t1 = time.time()
    lo, so, go = o.ppo_loss_grad(*batch)
    t2 = time.time()
    gn = np.linalg.norm(go)
    rel, rel0 = np.linalg.norm(gh - go) / gn, np.linalg.norm(g0 - go) / gn
    print(f"[bench minibatch] kind {kind} H {H} B {B} {variant}: {EXPECTED[H]} loss rel {abs(lh - lo) / abs(lo):.2e} |dg|/|g| {rel:.2e}; "
          f"{F32_KERNEL[H]} loss rel {abs(l0 - lo) / abs(lo):.2e} |dg|/|g| {rel0:.2e}; max |dstat| {np.abs(sh - so).max():.2e}; "
          f"device + batch {t1 - t0:.1f} s, oracle {t2 - t1:.1f} s on {oracle_mod.host_threads()} threads")
    assert lh == pytest.approx(lo, rel=1e-4)
    np.testing.assert_allclose(sh, so, rtol=2e-4, atol=2e-6)
    assert rel <= 2e-4
    assert l0 == pytest.approx(lo, rel=1e-4) and rel0 <= 2e-4                # the exact-f32 kernels have not met the oracle at this size either
    assert lh2 == lh and np.array_equal(gh, gh2)                             # deterministic slabs


# ---- (2) rollouts against block oracles ------------------------------------------------------------------------------------------------------------------
def _uniform_draws(oracle_mod, seed, t, e):
    """the shared Philox stream's u of env e (global index) at its step t of the first rollout after a reset (oracle/dril_oracle.c orc_collect_rollout)"""
    import ctypes as C
    L, r, out = oracle_mod.lib(), (C.c_uint32 * 4)(), []
    for ti, ei in zip(np.asarray(t).reshape(-1), np.asarray(e).reshape(-1)):
        L.orc_philox(int(seed) + int(ei), int(ti), 0, 1, 0, r)
        out.append(float(((int(r[0]) << 32 | int(r[1])) >> 11) * (1.0 / 9007199254740992.0)))
    return np.asarray(out, np.float64)


def _rollout_vs_blocks(pkg, oracle_mod, cfg, flat, seed, blocks, must_hold=(), tag="", early_steps=None):
    """one device rollout of cfg after a reset, compared on the columns of `blocks` with block oracles, field by field as test_collect_rollout_matches_oracle does.
    Every device buffer is copied out once and sliced on the host.  must_hold: (t, e) that have to lie inside the compared region.
    early_steps (envs whose trajectories amplify fp32 differences; every episode must end by truncation, so that the step within the episode is t mod episode_len): the
    small test's tolerances hold for the first early_steps steps of every episode, 2e-2 for the rest.  -> (handle, flags of the compared columns)"""
    capi = pkg._capi
    E, T, BL = cfg.n_envs, cfg.n_steps, bench_scale.BLOCK
    cols = np.concatenate([np.arange(BL * r, BL * r + BL) for r in blocks])
    t0 = time.time()
    h = pkg.Handle(cfg); h.set_params(flat); h.env_reset(seed)
    assert h.collect_rollout() > 0
    dev = {}
    for name in bench_scale.ROLLOUT_BUFS:
        a = h.buffer(getattr(capi, name))
        dev[name] = a[cols].copy() if name == "BUF_LAST_VALUES" else np.ascontiguousarray(a.reshape(T, E, -1)[:, cols])
        del a
    t1 = time.time()
    orc = {name: [] for name in bench_scale.ROLLOUT_BUFS}
    for r in blocks:
        blk = bench_scale.oracle_block_rollout(oracle_mod, capi, cfg, flat, seed, r)
        for name in bench_scale.ROLLOUT_BUFS:
            orc[name].append(blk[name] if name == "BUF_LAST_VALUES" else blk[name].reshape(T, BL, -1))
    orc = {name: np.concatenate(v, axis=0 if name == "BUF_LAST_VALUES" else 1) for name, v in orc.items()}
    t2 = time.time()
    ah, ao = dev["BUF_ACTIONS"], orc["BUF_ACTIONS"]
    nflip = 0
    if h.discrete:
        ok = np.cumprod((ah == ao).all(axis=2), axis=0).astype(bool)             # an env is compared up to its first action difference
        first = ok.copy(); first[1:] = ok[:-1]; first[0] = True                  # steps whose inputs still agree
        sel = first & ~ok
        if sel.any():                                                            # the FIRST difference of an env must be a CDF-edge flip (later ones follow from diverged states)
            ts, cs = np.nonzero(sel)
            small = oracle_mod.Oracle(_cfg(pkg, cfg.env_kind, n_envs=2, n_steps=2, batch_size=2, hidden1=cfg.hidden1, hidden2=cfg.hidden2)); small.set_params(flat)
            u = _uniform_draws(oracle_mod, seed, ts, cols[cs])
            obs_d = dev["BUF_OBSERVATIONS"][sel]                                  # judged on the DEVICE's observation: where observations have drifted apart (early_steps), the
            a_d = small.policy_forward(obs_d, u)[0]                               # oracle's action for the device's own input is the one to agree with
            nflip = _flip_report(small, cfg, obs_d, u, ah[sel], a_d, f" {tag}:")
    else:
        ok = np.ones(ah.shape[:2], bool)
    full = ok.all(axis=0)                                                        # GAE looks ahead: whole envs that never diverged
    frac = float(full.mean())
    for t, e in must_hold:
        c = int(np.flatnonzero(cols == e)[0])
        assert ok[t, c], f"{tag}: env {e} diverged at a CDF-edge flip before its boundary sample t = {t}: that row was not compared (another seed moves the flip)"
    worst = {}
    fields = (("BUF_OBSERVATIONS", 2e-5), ("BUF_VALUES", 5e-5), ("BUF_LOGPROBS", 1e-4), ("BUF_REWARDS", 1e-4), ("BUF_ADVANTAGES", 1e-3), ("BUF_RETURNS", 1e-3))
    if early_steps is not None:
        # Pendulum and Acrobot amplify: two fp32 runs that differ by 1e-7 of the weights are up to 2e-4 apart in Pendulum's observations at the end of a 200-step
        # episode (measured on the oracle against itself), and device and oracle part completely within one 500-step episode of Acrobot's double pendulum (measured: the
        # first action differences of a rollout sat 1e-2 from any CDF edge of the oracle's own observation).  Every truncation resets both sides to the same seeded
        # state.  So the small test's tolerances hold for the first early_steps steps of every episode — the boundary rows must be among them — and the rest is
        # held to 2e-2: what a row read or written in the wrong place breaks by O(1)
        assert not (orc["BUF_FLAGS"] & 1).any()                                  # no terminations: the step within the episode is t mod episode_len
        early = (np.arange(T) % cfg.episode_len) < early_steps
        for t, e in must_hold:
            assert early[t], f"{tag}: the boundary row t = {t} is outside the tightly compared steps"
        if not h.discrete:
            np.testing.assert_allclose(ah[early], ao[early], atol=2e-5, rtol=2e-5, err_msg=f"{tag} BUF_ACTIONS")
            np.testing.assert_allclose(ah, ao, atol=2e-2, rtol=2e-2, err_msg=f"{tag} BUF_ACTIONS")
        oke = ok & early[:, None]
        for name, tol in fields:
            a, b = dev[name], orc[name]
            if name not in ("BUF_ADVANTAGES", "BUF_RETURNS"):                       # (GAE looks ahead over the whole episode)
                np.testing.assert_allclose(a[oke], b[oke], atol=tol, rtol=tol, err_msg=f"{tag} {name}")
                worst[name] = float(np.abs(a[oke] - b[oke]).max())
                np.testing.assert_allclose(a[ok], b[ok], atol=2e-2, rtol=2e-2, err_msg=f"{tag} {name}")
                worst[name + " (all steps)"] = float(np.abs(a[ok] - b[ok]).max())
            else:
                np.testing.assert_allclose(a[:, full], b[:, full], atol=2e-2, rtol=2e-2, err_msg=f"{tag} {name}")
                worst[name + " (all steps)"] = float(np.abs(a[:, full] - b[:, full]).max())
        fields = ()
    for name, tol in fields:
        a, b = dev[name], orc[name]
        if name in ("BUF_OBSERVATIONS", "BUF_VALUES", "BUF_LOGPROBS", "BUF_REWARDS"):   # per-step fields: every step up to the env's first difference (the boundary rows among them)
            np.testing.assert_allclose(a[ok], b[ok], atol=tol, rtol=tol, err_msg=f"{tag} {name}")
        np.testing.assert_allclose(a[:, full], b[:, full], atol=tol, rtol=tol, err_msg=f"{tag} {name}")
        worst[name] = float(np.abs(a[:, full] - b[:, full]).max())
    fh, fo = dev["BUF_FLAGS"][:, :, 0], orc["BUF_FLAGS"][:, :, 0]
    np.testing.assert_array_equal(fh[ok], fo[ok])
    tr = (fo & 2).astype(bool) & full[None, :]
    late = 5e-5 if early_steps is None else 2e-2                                 # (early_steps: these are values at the END of an episode, see above)
    np.testing.assert_allclose(dev["BUF_BOOTSTRAP"][:, :, 0][tr], orc["BUF_BOOTSTRAP"][:, :, 0][tr], atol=late, rtol=late)
    live = full & (fo[T - 1] == 0)                                               # V(new_obs) is only consumed for rollout-limited tails
    np.testing.assert_allclose(dev["BUF_LAST_VALUES"][live], orc["BUF_LAST_VALUES"][live], atol=late, rtol=late)
    print(f"[bench rollout] {tag}: blocks {list(blocks)} = {cols.size} envs x {T} steps; {nflip} CDF-edge flips, {frac:.4f} of the envs never diverged; "
          f"max |d| " + ", ".join(f"{k[4:].lower()} {v:.1e}" for k, v in worst.items()) +
          f"; terminations {int((fo & 1)[:, full].sum())}, truncations {int(tr.sum())}; device + copies {t1 - t0:.1f} s, oracle {t2 - t1:.1f} s")
    assert frac >= 0.98
    return h, fo[:, full]


ROLLOUT_CASES = {                       # kind, hidden, parameter scale, episode_len (0: the env's own), early_steps of _rollout_vs_blocks
    "cartpole": (0, 64, 0.3, 0, None),          # configs[1].  The pole falls within tens of steps: terminations throughout, nothing to amplify
    # the largest buffers: 24-byte observation rows, 48-byte records.  Truncation, bootstrap and reset every 48 steps (9.6 s): Acrobot's terminations need hundreds of
    # steps of a double pendulum, which no two fp32 implementations follow in lock step (see early_steps) — terminations are CartPole's part.  48 puts the boundary rows
    # t = 682 and t = 1365 at steps 10 and 21 of their episodes
    "acrobot": (6, 64, 0.3, 48, 32),
    "pendulum256": (1, 256, 0.05, 0, 32),       # configs[2]'s env and net WITHOUT NormalizeWrapperEnv: its running statistics couple all envs, which no block oracle can reproduce
}


def _rollout_cfg(pkg, case, E, T, **kw):
    kind, H, scale, L, _ = ROLLOUT_CASES[case]
    if L:
        kw["episode_len"] = L
    cfg = _cfg(pkg, kind, n_envs=E, n_steps=T, batch_size=E * T // 32, epochs=1, hidden1=H, hidden2=H, fixed_length_episodes=0, **kw)
    D, A, disc = bench_scale.SPACES[kind]
    P = 2 * (D * H + H + H * H + H) + (A * H + A) + (H + 1) + (0 if disc else A)      # actor, critic, log_std (include/dril_hip.h layout)
    return cfg, _params(P, 3, scale)


@pytest.mark.parametrize("case", ["cartpole", "acrobot", "pendulum256"])
def test_block_oracles_reproduce_a_small_device_rollout(pkg, oracle_mod, case):
    """runs first: 256 envs on the device against four 64-env oracles with rank = 0 .. 3 — the oracle's `rank` moves the env seeds and the keys of the sampling
    noise and nothing else (bit for bit on the CPU: tests/test_bench_scale_host.py), and the device seeds its envs by the same global index"""
    cfg, flat = _rollout_cfg(pkg, case, 256, 600)
    h, fl = _rollout_vs_blocks(pkg, oracle_mod, cfg, flat, 42, range(4), tag=f"{case} E=256", early_steps=ROLLOUT_CASES[case][4])
    h.close()
    assert ((fl & 1).any() if case == "cartpole" else (fl & 2).any())


@pytest.mark.parametrize("case", ["cartpole", "acrobot", "pendulum256"])
def test_full_size_rollout_vs_block_oracles(pkg, oracle_mod, case):
    """65 536 envs x 2048 steps with real episodes and the shared Philox stream: observations, actions, values, log-probabilities, rewards, flags, bootstrap values,
    last values, advantages and returns of the envs of the first and the last block and of every block with a row on a 2^31- / 2^32-byte offset of a per-sample device
    buffer, against block oracles.  The compared columns span all 2048 steps, so an address that goes wrong from some sample index on is met in every one of them."""
    E, T = E_FULL, T_FULL
    cfg, flat = _rollout_cfg(pkg, case, E, T)
    blocks, samples = bench_scale.blocks_to_check(cfg.env_kind, E, T)
    assert 0 in blocks and (E - 1) // bench_scale.BLOCK in blocks
    must = [(t, e) for name, _, _, t, e in samples if name in ("observations", "actions", "records")]
    h, fl = _rollout_vs_blocks(pkg, oracle_mod, cfg, flat, 42, blocks, must_hold=must, tag=f"{case} full size, boundary samples {[(s[0], s[3], s[4]) for s in samples]}",
                               early_steps=ROLLOUT_CASES[case][4])
    h.close()
    if case == "cartpole":
        assert (fl & 1).any()                                                    # real episodes: the pole falls
    else:
        assert (fl & 2).any() and not (fl & 1).any()                             # Pendulum never terminates, Acrobot not within 48 steps: truncations with V(terminal_observation) bootstraps


# ---- (3) the production update at full size --------------------------------------------------------------------------------------------------------------
def _full_size_update_handle(pkg, cfg, flat, seed):
    h = pkg.Handle(cfg); h.set_params(flat); h.env_reset(seed)
    assert h.collect_rollout() > 0
    return h


def test_full_size_update_vs_oracle_epoch(pkg, oracle_mod, monkeypatch):
    """BASELINE configs[1] as bench.py runs it — the rollout of 2^27 samples, then, without a reset, ONE dril_ppo_update of 32 minibatches of 4 194 304 in the device's
    own DataLoader order (default kernel selection: ppo_grad_pair_kernel on packed records of exactly 2^32 bytes, pos0 up to 31 x 4 194 304, the epoch's perm32 array) —
    against orc_ppo_update on the DEVICE's buffers with the same keyed bijection: the nine statistics and the parameters after the 32 Adam steps.  Then the same update
    with DRIL_NO_EPOCH_INDEX=1 (the bijection evaluated inside the kernel): bitwise the same parameters."""
    capi = pkg._capi
    E, T = E_FULL, T_FULL
    cfg, flat = _rollout_cfg(pkg, "cartpole", E, T, seed=4)
    t0 = time.time()
    h = _full_size_update_handle(pkg, cfg, flat, 42)
    o = oracle_mod.Oracle(cfg); o.set_params(flat)
    for name in UPDATE_BUFS:                                                     # one full-size host copy at a time
        o.set_buffer(getattr(capi, name), h.buffer(getattr(capi, name)))
    sh = h.ppo_update(); ph = h.get_params(); kernel = h.grad_kernel_info().split(":")[0]
    h.close()
    monkeypatch.setenv("DRIL_NO_EPOCH_INDEX", "1")                               # latched by dril_create
    h2 = _full_size_update_handle(pkg, cfg, flat, 42)
    monkeypatch.delenv("DRIL_NO_EPOCH_INDEX")
    sh2 = h2.ppo_update(); ph2 = h2.get_params()
    h2.close()
    t1 = time.time()
    so = o.ppo_update(); po = o.get_params()
    t2 = time.time()
    del o
    assert kernel == EXPECTED[64]
    assert sh.n_updates == so.n_updates == sh2.n_updates == 32 and not sh.early_stopped and sh.f32_path == 0 and sh2.f32_path == 0
    dstat = {f: abs(getattr(sh, f) - getattr(so, f)) / max(abs(getattr(so, f)), 1e-30) for f in STATS}
    dp = np.abs(ph - po)
    moved = np.abs(po - flat)
    print(f"[bench update] configs[1] full epoch: rel stat differences " + ", ".join(f"{k} {v:.1e}" for k, v in dstat.items()) +
          f"; parameters after 32 steps: max |d| {dp.max():.2e}, |d| / |update| {np.linalg.norm(ph - po) / np.linalg.norm(po - flat):.2e} (max |update| {moved.max():.2e}); "
          f"device (two rollouts + updates, copies) {t1 - t0:.1f} s, oracle epoch {t2 - t1:.1f} s on {oracle_mod.host_threads()} threads")
    # measured: statistics within 1.1e-6 of the oracle's, parameters within 1.2e-7 (2.4e-6 of the update).  The bounds are 10 - 50 x that, not the 5e-4 / 2e-5 of the
    # small tests: a minibatch that reads other valid samples than the oracle's differs from it only by sampling noise, ~ 1 / sqrt(4 194 304) = 5e-4 of a per-sample spread
    for f in STATS:
        assert getattr(sh, f) == pytest.approx(getattr(so, f), rel=5e-5, abs=2e-7), f
    assert moved.max() > 1e-3                                                    # 32 Adam steps moved the weights
    np.testing.assert_allclose(ph, po, rtol=2e-5, atol=2e-6)
    assert np.array_equal(ph, ph2), "the in-kernel bijection and the perm32 index array are two DataLoader orders"
    assert all(getattr(sh, f) == getattr(sh2, f) for f in STATS)


def _epoch_order(oracle_mod, N, key, p0, count):
    """buffer indices of positions [p0, p0 + count) of the epoch order (dril_device.h mix_bij32; N a power of two: no rejected positions), checked against orc_perm_index"""
    assert N & (N - 1) == 0
    bits = N.bit_length() - 1; mask = np.uint64(N - 1); sh = bits // 2
    x = np.arange(p0, p0 + count, dtype=np.uint64)
    for r in range(4):
        x ^= np.uint64((key >> (13 * r)) & (N - 1))
        x = (x * np.uint64(0x7F4A7C15) + np.uint64(0xD192ED03)) & mask; x ^= x >> np.uint64(sh)
        x = (x * np.uint64(0x1CE4E5B9)) & mask; x ^= x >> np.uint64(sh + 1 if sh + 1 < bits else sh)
    L = oracle_mod.lib()
    for i in (0, 1, count // 2, count - 1):
        assert int(x[i]) == L.orc_perm_index(p0 + i, N, key)
    return x.astype(np.int64)


def test_full_size_update_acrobot_minibatches_vs_oracle(pkg, oracle_mod):
    """Acrobot at full size — 48-byte records: the record buffer is 6.4 GB and passes 2^32 bytes at sample 89 478 485, the observation rows pass 2^31 bytes at the
    same sample — through the production update (32 minibatches, the device's own order).  The oracle's epoch would double this file's time, so its work is cut, not
    the size: the learning rate is 0 (the parameters must stay bit-identical, so all 32 minibatches are evaluated at the same weights, which differ from the
    rollout's by N(0, 0.03^2) per weight so that ratios, clipping and the KL estimate are not trivial), and
      * the value loss averaged over 32 equal minibatches is the mean of (V(obs) - return)^2 over ALL 2^27 samples, whatever the order: the oracle's critic gives it
        exactly (orc_predict_values) — a record read from the wrong place, a sample read twice or never, shifts it;
      * ratio_first is minibatch 0's own mean ratio: orc_ppo_loss_grad on that minibatch, gathered on the host in the oracle's order;
      * the means of the other statistics and of grad_norm are compared with the oracle's over minibatches 0, 31 (the highest pos0) and the one that holds sample
        89 478 485; every minibatch of a random order has samples on both sides of that offset (asserted).  A 32-minibatch mean against a 3-minibatch mean is a
        sampling comparison: the bound is the spread between minibatches (~ 1 / sqrt(4 194 304) of a per-sample deviation), not fp32."""
    capi = pkg._capi
    E, T = E_FULL, T_FULL
    N, B = E * T, E * T // 32
    cfg, flat = _rollout_cfg(pkg, "acrobot", E, T, seed=4, ent_coef=0.01)
    samples = bench_scale.blocks_to_check(6, E, T)[1]
    n_cross = [n for name, off, n, _, _ in samples if name == "records" and off == 1 << 32][0]
    t0 = time.time()
    h = _full_size_update_handle(pkg, cfg, flat, 42)
    flat2 = (flat + 0.03 * np.random.default_rng(8).standard_normal(flat.size)).astype(np.float32)
    h.set_params(flat2); h.set_learning_rate(0.0)
    bufs = {name: h.buffer(getattr(capi, name)) for name in UPDATE_BUFS}
    st = h.ppo_update()
    assert h.grad_kernel_info().split(":")[0] == EXPECTED[64]
    assert st.n_updates == 32 and st.f32_path == 0 and not st.early_stopped
    assert np.array_equal(h.get_params(), flat2)                                 # learning rate 0: 32 optimiser steps that move nothing
    h.close()
    t1 = time.time()
    o = oracle_mod.Oracle(_cfg(pkg, 6, n_envs=2, n_steps=2, batch_size=2, ent_coef=0.01)); o.set_params(flat2)
    # the exact one: value loss over the whole buffer
    sq, chunk = 0.0, 1 << 22
    for a in range(0, N, chunk):
        v = o.predict_values(bufs["BUF_OBSERVATIONS"][a:a + chunk]).astype(np.float64)
        sq += float(((v - bufs["BUF_RETURNS"][a:a + chunk]) ** 2).sum())
    vl_all = sq / N
    t2 = time.time()
    key = oracle_mod.lib().orc_perm_key(cfg.seed, 0, 0)
    holder = None
    for k in range(32):                                                          # the minibatch whose order holds the sample on the 2^32-byte offset
        idx = _epoch_order(oracle_mod, N, key, k * B, B)
        assert idx.min() < n_cross < idx.max()                                   # every minibatch reads on both sides of it
        if (idx == n_cross).any():
            holder = k
    assert holder is not None
    checked = sorted({0, 31, holder})
    rows = []
    for k in checked:
        idx = _epoch_order(oracle_mod, N, key, k * B, B)
        lo, so, go = o.ppo_loss_grad(*(bufs[name][idx] for name in UPDATE_BUFS))
        rows.append(dict(policy_loss=so[0], value_loss=so[1], entropy_loss=so[2], clip_fraction=so[3], approx_kl_div=so[4], loss=lo, grad_norm=float(np.linalg.norm(go)), ratio=so[6]))
    t3 = time.time()
    del bufs
    mean = {f: float(np.mean([r[f] for r in rows])) for f in rows[0]}
    spread = {f: float(np.ptp([r[f] for r in rows])) for f in rows[0]}
    print(f"[bench update] Acrobot full size, learning rate 0: value loss device {st.value_loss:.6f} vs all 2^27 samples {vl_all:.6f} (rel {abs(st.value_loss - vl_all) / vl_all:.1e}); "
          f"ratio_first device {st.ratio_first:.7f} oracle {rows[0]['ratio']:.7f}; minibatches checked {checked} (sample {n_cross} is in {holder}); "
          + ", ".join(f"{f} device {getattr(st, f):.5g} oracle {mean[f]:.5g} (spread {spread[f]:.1e})" for f in ("policy_loss", "entropy_loss", "clip_fraction", "approx_kl_div", "loss", "grad_norm"))
          + f"; device + copies {t1 - t0:.1f} s, critic over 2^27 samples {t2 - t1:.1f} s, order + {len(checked)} oracle minibatches {t3 - t2:.1f} s")
    assert st.value_loss == pytest.approx(vl_all, rel=2e-5)
    assert st.ratio_first == pytest.approx(rows[0]["ratio"], rel=2e-6)
    assert abs(rows[0]["ratio"] - 1.0) > 1e-4                                    # the perturbed weights make it a statement about minibatch 0's samples
    for f in ("policy_loss", "value_loss", "entropy_loss", "clip_fraction", "approx_kl_div", "loss", "grad_norm"):
        assert getattr(st, f) == pytest.approx(mean[f], rel=5e-3, abs=5e-3), f
