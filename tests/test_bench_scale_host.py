"""CPU: what tests/test_gpu_bench_scale.py stands on — the table of 2^31 / 2^32-byte offsets in the device buffers (tests/diag/buffer_boundaries.py) and the
claim that an oracle of 64 envs with `rank = r` plays envs [64 r, 64 r + 64) of a wider run (tests/bench_scale.py)."""
import numpy as np
import pytest

import bench_scale
from diag import buffer_boundaries as bb


def _cfg(pkg, kind, **kw):
    c = pkg._capi.default_config(kind)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_boundaries_of_one_buffer():
    G = 1 << 31
    assert bb.boundaries(32, 1 << 27) == [(G, (1 << 26) - 1, 1 << 26)]                # 2^32 bytes: the end of the buffer is not inside it
    assert bb.boundaries(16, 1 << 27) == [] and bb.boundaries(4, 1 << 27) == []        # 2^31 bytes exactly / 2^29 bytes
    got = bb.boundaries(48, 1 << 27)
    assert [o for o, _, _ in got] == [G, 2 * G]                                        # 3 x 2^31 is the buffer's end
    for off, lo, hi in got:
        assert lo == hi and lo * 48 < off < (lo + 1) * 48                              # 48 does not divide 2^31: a row straddles every offset
    assert bb.boundaries(24, 1 << 27) == [(G, 89478485, 89478485)]
    assert bb.boundaries(8, (1 << 28) + 1) == [(G, (1 << 28) - 1, 1 << 28)]            # one row past the offset is enough
    assert bb.boundaries(8, 1 << 28) == []
    for stride, rows in ((12, 400_000_000), (48, 134_217_728), (7, 1_000_000_000)):    # the definition, by brute force on the rows around every offset
        for off, lo, hi in bb.boundaries(stride, rows):
            assert off % G == 0 and 0 < off < stride * rows
            assert lo * stride <= off - 1 < (lo + 1) * stride and hi * stride <= off < (hi + 1) * stride and hi - lo in (0, 1)
        assert len(bb.boundaries(stride, rows)) == (stride * rows - 1) // G


def test_boundary_samples_of_the_bench_configs():
    E, T = 65536, 2048
    cart = bb.boundary_samples(*bb.SPACES[0], E, T)
    assert cart == [("records", 1 << 31, (1 << 26) - 1, 1023, 65535), ("records", 1 << 31, 1 << 26, 1024, 0)]
    pend = bb.boundary_samples(*bb.SPACES[1], E, T)
    assert [s[1:] for s in pend] == [s[1:] for s in cart]                              # D = 3: two-quad records as well, 12-byte observation rows stay below 2^31
    acro = bb.boundary_samples(*bb.SPACES[6], E, T)
    assert acro == [("observations", 1 << 31, 89478485, 1365, 21845), ("records", 1 << 31, 44739242, 682, 43690), ("records", 1 << 32, 89478485, 1365, 21845)]
    for name, off, n, t, e in cart + acro:
        assert n == t * E + e and 0 <= t < T and 0 <= e < E
        stride = bb.row_bytes(*bb.SPACES[0 if (name, off, n, t, e) in cart else 6])[name]
        assert n * stride <= off <= (n + 1) * stride
    assert bb.boundary_envs(*bb.SPACES[6], E, T) == [21845, 43690]
    assert bb.boundary_samples(*bb.SPACES[6], E, T, fields=("observations",)) == acro[:1]
    assert bench_scale.blocks_to_check(0, E, T)[0] == [0, 1023]
    assert bench_scale.blocks_to_check(6, E, T)[0] == [0, 341, 682, 1023]
    assert bb.boundary_samples(*bb.SPACES[0], 4096, 64) == []                          # small runs have none
    assert "straddles" in bb.table(6, E, T) and "2^32" in bb.table(6, E, T)


@pytest.mark.parametrize("kind,L,H", [(0, 40, 64), (6, 60, 64), (1, 50, 64), (1, 50, 128)])
def test_four_block_oracles_equal_one_wide_oracle(pkg, oracle_mod, kind, L, H):
    """envs [64 r, 64 r + 64) of a 256-env oracle == a 64-env oracle with rank = r, on every buffer field, bit for bit, over two rollouts without a reset in
    between (real episodes, the shared Philox stream): `rank` moves the env seeds and the keys of the sampling noise and nothing else"""
    capi = pkg._capi
    E, T = 256, 160
    cfg = _cfg(pkg, kind, n_envs=E, n_steps=T, episode_len=L, batch_size=E * T // 4, epochs=1, hidden1=H, hidden2=H, seed=11)
    wide = oracle_mod.Oracle(cfg)
    flat = (np.random.default_rng(3).standard_normal(wide.P) * (0.4 if H == 64 else 0.1)).astype(np.float32)
    wide.set_params(flat); wide.env_reset(42)
    wide.collect_rollout(); wide.collect_rollout()
    fl = wide.buffer(capi.BUF_FLAGS)
    assert ((fl & 1).any() if kind == 0 else (fl & 2).any())                           # episodes end inside the rollouts (the pole falls; the others reach their time limit): resets draw from the env's own seed
    for r in range(4):
        blk = bench_scale.oracle_block_rollout(oracle_mod, capi, cfg, flat, 42, r, rollouts=2)
        cols = slice(64 * r, 64 * r + 64)
        for name in bench_scale.ROLLOUT_BUFS:
            a = wide.buffer(getattr(capi, name))
            a = a[cols] if name == "BUF_LAST_VALUES" else a.reshape(T, E, -1)[:, cols].reshape(blk[name].shape)
            assert np.array_equal(a.view(np.uint8), blk[name].view(np.uint8)), (name, r)
    other = bench_scale.oracle_block_rollout(oracle_mod, capi, cfg, flat, 42, 1)["BUF_OBSERVATIONS"]
    assert not np.array_equal(other, bench_scale.oracle_block_rollout(oracle_mod, capi, cfg, flat, 42, 2)["BUF_OBSERVATIONS"])   # the blocks differ from each other


def test_block_oracle_refuses_coupled_envs(pkg):
    cfg = _cfg(pkg, 1, n_envs=256, n_steps=8, norm_obs=1, norm_training=1)
    with pytest.raises(AssertionError):
        bench_scale.block_config(cfg, 1)
