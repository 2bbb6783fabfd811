"""diagnostic (CPU): byte sizes of the per-sample device buffers of a config and the samples whose rows sit on a 2^31- or 2^32-byte offset.

The device keeps one row per sample n = t * E + e in every rollout field (dril_api.hip dril_create: obs N x D f32, actions N x (4 | 4 A) bytes, seven 4-byte fields,
1-byte flags) and, for the update, packed records of 2 (D <= 4) or 3 (D <= 8) float4 per sample (pack_records_kernel, RecLayout in dril_grad_common.h) plus the
epoch order as N int32.  A byte offset that is held in 32 bits goes wrong at 2^31 (signed) or 2^32 (unsigned); `boundaries` lists, per buffer, the last sample that
starts below such an offset and the first that ends above it (one sample when a row straddles the offset), which tests/test_gpu_bench_scale.py turns into the envs
the oracle reproduces.  One definition: the tests import it, and run as a script it prints the table:

    python tests/diag/buffer_boundaries.py [env_kind] [n_envs] [n_steps]
"""
from __future__ import annotations

import sys

# (D, A, discrete) per env kind, include/dril_hip.h (ScalingWrapperEnv kinds share their inner env's spaces)
SPACES = {0: (4, 2, True), 1: (3, 1, False), 2: (3, 1, False), 3: (2, 3, True), 4: (2, 1, False), 6: (6, 3, True), 7: (2, 1, False)}
ROLLOUT_FIELDS = ("observations", "actions")                       # the rollout buffers whose rows are wider than four bytes
WORD_FIELDS = ("rewards", "advantages", "returns", "logprobs", "values", "bootstrap")


def row_bytes(D: int, A: int, discrete: bool) -> dict:
    """bytes per sample of every per-sample device buffer"""
    out = {"observations": 4 * D, "actions": 4 if discrete else 4 * A}
    out.update({f: 4 for f in WORD_FIELDS})
    out["flags"] = 1
    out["records"] = 16 * (2 if D <= 4 else 3)
    out["epoch_index"] = 4
    return out


def boundaries(stride: int, n_rows: int) -> list:
    """[(offset, first_row, last_row)] for every multiple of 2^31 strictly inside a buffer of n_rows rows of `stride` bytes: first_row holds the byte just below the
    offset, last_row the byte at it (equal when a row straddles the offset).  Offsets that are multiples of 2^32 are in the list as multiples of 2^31."""
    out, size = [], stride * n_rows
    off = 1 << 31
    while off < size:
        out.append((off, (off - 1) // stride, off // stride))
        off += 1 << 31
    return out


def boundary_samples(D: int, A: int, discrete: bool, E: int, T: int, fields=None) -> list:
    """[(buffer, offset, n, t, e)] over the buffers named in `fields` (default: all), both rows of every boundary"""
    out = []
    for name, stride in row_bytes(D, A, discrete).items():
        if fields is not None and name not in fields:
            continue
        for off, lo, hi in boundaries(stride, E * T):
            for n in sorted({lo, hi}):
                out.append((name, off, n, n // E, n % E))
    return out


def boundary_envs(D: int, A: int, discrete: bool, E: int, T: int, fields=None) -> list:
    return sorted({e for _, _, _, _, e in boundary_samples(D, A, discrete, E, T, fields)})


def table(kind: int, E: int, T: int) -> str:
    D, A, disc = SPACES[kind]
    lines = [f"env kind {kind}: D = {D}, A = {A}, {'discrete' if disc else 'continuous'}; {E} envs x {T} steps = {E * T} samples"]
    for name, stride in row_bytes(D, A, disc).items():
        size = stride * E * T
        lines.append(f"  {name:<13} {stride:>3} B/sample  {size:>13} B = {size / 2 ** 30:7.3f} GiB" + ("" if size > 1 << 31 else "   (no offset reaches 2^31)"))
        for off, lo, hi in boundaries(stride, E * T):
            what = f"{off // (1 << 31)} x 2^31" + (" (a multiple of 2^32)" if off % (1 << 32) == 0 else "")
            rows = f"sample {lo} (t = {lo // E}, env {lo % E}) straddles it" if lo == hi else \
                f"sample {lo} (t = {lo // E}, env {lo % E}) ends at it, sample {hi} (t = {hi // E}, env {hi % E}) starts at it"
            lines.append(f"      offset {what}: {rows}")
    return "\n".join(lines)


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    kinds = [a[0]] if a else [0, 6, 1]
    E, T = (a[1], a[2]) if len(a) >= 3 else (65536, 2048)
    for k in kinds:
        print(table(k, E, T))
