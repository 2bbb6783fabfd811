"""Helpers of the bench-scale tests (test infrastructure): an oracle for a block of a large run's envs, and the blocks that hold its buffer boundaries.

Envs are independent and seeded by GLOBAL index (env_seed0 = seed + rank * n_envs, oracle/dril_oracle.c orc_env_reset; the sampling noise is Philox keyed by
env_seed0 + e at the env's own step counter), so an oracle with n_envs = BLOCK and rank = r reproduces envs [BLOCK r, BLOCK r + BLOCK) of a run of any width —
as long as nothing couples the envs: no NormalizeWrapperEnv (its running statistics are taken over all envs), no injected noise (indexed by local env).
tests/test_bench_scale_host.py checks that claim bit for bit on the CPU, tests/test_gpu_bench_scale.py against the device before it relies on it.
"""
from __future__ import annotations

import copy

import numpy as np

from diag.buffer_boundaries import SPACES, boundary_samples

BLOCK = 64
ROLLOUT_BUFS = ("BUF_OBSERVATIONS", "BUF_ACTIONS", "BUF_REWARDS", "BUF_ADVANTAGES", "BUF_RETURNS", "BUF_LOGPROBS", "BUF_VALUES", "BUF_FLAGS", "BUF_BOOTSTRAP", "BUF_LAST_VALUES")


def block_config(cfg, r, block=BLOCK):
    """the config of the oracle that plays envs [block r, block r + block) of cfg's run"""
    assert cfg.n_envs % block == 0 and cfg.world_size == 1 and cfg.rank == 0
    assert not (cfg.norm_obs or cfg.norm_reward), "NormalizeWrapperEnv couples the envs: a block oracle cannot reproduce its statistics"
    c = copy.copy(cfg)
    c.n_envs, c.rank, c.world_size = block, r, cfg.n_envs // block
    c.batch_size = max(2, (block * cfg.n_steps) // 4) * c.world_size           # (per-rank minibatch = batch_size / world_size; the block oracles never update)
    return c


def oracle_block_rollout(oracle_mod, capi, cfg, flat, seed, r, block=BLOCK, rollouts=1):
    """{buffer name: array} of the last of `rollouts` rollouts of envs [block r, block r + block), arrays shaped (T, block[, width]) ((block,) for the last values)"""
    o = oracle_mod.Oracle(block_config(cfg, r, block))
    o.set_params(flat); o.env_reset(seed)
    for _ in range(rollouts):
        o.collect_rollout()
    out = {}
    for name in ROLLOUT_BUFS:
        a = o.buffer(getattr(capi, name))
        out[name] = a if name == "BUF_LAST_VALUES" else a.reshape(cfg.n_steps, block, -1) if a.ndim == 2 else a.reshape(cfg.n_steps, block)
    return out


def blocks_to_check(kind, E, T, block=BLOCK):
    """rank blocks holding env 0, env E - 1 and every env with a row on a 2^31 / 2^32-byte offset of a per-sample device buffer -> (sorted blocks, boundary samples)"""
    D, A, disc = SPACES[kind]
    samples = boundary_samples(D, A, disc, E, T)
    return sorted({0, (E - 1) // block} | {e // block for *_, e in samples}), samples
