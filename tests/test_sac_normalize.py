"""No GPU: the C ABI surface of NormalizeWrapperEnv on the SAC handle (struct layout from a compiled C probe, defaults, statuses of null calls, exported = declared)
and the NumPy restatement of the wrapper (tests/sac_normalize_ref.py) against a float64 Welford over the same batches."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import sac_normalize_ref as ref

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("training", "norm_obs", "norm_reward", "clip_obs", "clip_reward", "gamma", "epsilon", "reserved")


def test_normalize_config_layout_matches_the_ctypes_mirror(pkg, tmp_path):
    capi = pkg._capi
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_sac.h"\nint main(void) {\n  printf("%zu\\n", sizeof(dril_sac_normalize_config));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(dril_sac_normalize_config, {f}));\n' for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = capi.DrilSacNormalizeConfig
    assert out[0] == C.sizeof(S)
    assert [f for f, _ in S._fields_] == list(FIELDS)
    assert out[1:] == [getattr(S, f).offset for f in FIELDS]


def test_defaults_are_the_references_keywords_and_null_calls_answer_with_a_message(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    c = capi.DrilSacNormalizeConfig()
    c.reserved = 7
    assert lib.dril_sac_normalize_config_default(C.byref(c)) == capi.OK
    assert (c.training, c.norm_obs, c.norm_reward, c.reserved) == (1, 1, 1, 0)
    assert (c.clip_obs, c.clip_reward) == (10.0, 10.0) and c.gamma == np.float32(0.99) and c.epsilon == np.float32(1e-8)   # normalizeWrapperEnv.jl:71-80
    assert lib.dril_sac_normalize_config_default(None) == capi.ERR_INVALID_ARG
    assert b"null" in lib.dril_sac_last_error(None)
    f, i = C.c_float(), C.c_int64()
    buf = (C.c_float * 4)()
    for rc in (lib.dril_sac_normalize_enable(None, C.byref(c)), lib.dril_sac_normalize_set_training(None, 1),
               lib.dril_sac_normalize_get_stats(None, buf, buf, C.byref(i), C.byref(f), C.byref(f), C.byref(i)),
               lib.dril_sac_normalize_set_stats(None, buf, buf, 0, 0.0, 1.0, 0), lib.dril_sac_normalize_get_original(None, buf, buf),
               lib.dril_sac_normalize_get_returns(None, buf)):
        assert rc == capi.ERR_NOT_INITIALISED
        assert b"null handle" in lib.dril_sac_last_error(None)


def test_every_normalize_verb_is_declared_exported_and_mirrored(pkg):
    header = (ROOT / "include" / "dril_sac.h").read_text()
    declared = set(re.findall(r"\b(dril_sac_normalize_\w+)\s*\(", header))
    mirrored = {s for s in pkg._capi.EXPORTED_SYMBOLS if s.startswith("dril_sac_normalize_")}
    assert declared == mirrored and len(declared) >= 6
    lib = C.CDLL(str(ROOT / "dril.jl_amd" / "csrc" / "libdril_hip.so"))
    assert all(hasattr(lib, s) for s in declared)
    for name in ("normalize_enable", "normalize_set_training", "norm_get_stats", "norm_set_stats", "norm_get_original"):
        assert callable(getattr(pkg.SacHandle, name))


def test_numpy_wrapper_statistics_agree_with_a_float64_welford():
    rng = np.random.default_rng(0)
    E, D = 37, 12
    scale = (10.0 ** rng.uniform(-2, 3, D)); shift = rng.normal(0, 50, D)
    w = ref.Wrapper(E, D)
    n, mean, m2 = 0, np.zeros(D), np.zeros(D)
    rn, rmean, rm2 = 0, 0.0, 0.0
    returns = np.zeros(E)
    for it in range(40):
        x = (rng.normal(0, 1, (E, D)) * scale + shift).astype(np.float32)
        if it == 0:
            assert w.obs_count == 0                                         # the count = 0 first merge takes the batch moments as they are
        w.observe(x)
        if it == 0:
            bm, bv = ref.batch_moments(x)
            assert np.array_equal(w.obs_mean, bm) and np.array_equal(w.obs_var, bv) and w.obs_count == E
        for row in x.astype(np.float64):
            n += 1; d = row - mean; mean += d / n; m2 += d * (row - mean)
        r = rng.normal(-3, 2, E).astype(np.float32)
        done = rng.random(E) < 0.1
        out, _ = w.act(r, done, np.zeros(E, bool), x)
        returns = returns * float(np.float32(0.99)) + r
        for v in returns:
            rn += 1; d = v - rmean; rmean += d / rn; rm2 += d * (v - rmean)
        assert np.allclose(out, np.clip(r / np.sqrt(rm2 / rn + 1e-8), -10, 10), rtol=1e-4, atol=1e-5)
        returns[done] = 0
        assert np.allclose(w.returns, returns, rtol=1e-5, atol=1e-5)
    assert w.obs_count == n == 40 * E and w.ret_count == rn
    assert np.allclose(w.obs_mean, mean, rtol=2e-5, atol=2e-5 * np.abs(scale))
    assert np.allclose(w.obs_var, m2 / n, rtol=2e-4)
    assert np.isclose(w.ret_mean, rmean, rtol=1e-4, atol=1e-4) and np.isclose(w.ret_var, rm2 / rn, rtol=2e-4)
    y = w.normalize_obs(x)
    assert np.allclose(y, np.clip((x - mean) / np.sqrt(m2 / n + 1e-8), -10, 10), rtol=1e-3, atol=1e-3)


def test_frozen_and_half_switched_wrappers():
    rng = np.random.default_rng(1)
    E, D = 5, 3
    x = rng.normal(0, 4, (E, D)).astype(np.float32); r = rng.normal(0, 4, E).astype(np.float32)
    w = ref.Wrapper(E, D, training=False, clip_obs=0.5, clip_reward=0.25)
    y = w.observe(x); out, _ = w.act(r, np.zeros(E, bool), np.zeros(E, bool), x)
    assert w.obs_count == 0 and w.ret_count == 0 and not w.returns.any()
    assert np.abs(y).max() <= 0.5 and np.abs(out).max() <= 0.25 and (np.abs(y) == 0.5).any()
    w = ref.Wrapper(E, D, norm_obs=False)
    assert np.array_equal(w.observe(x), x) and w.obs_count == 0
    w.act(r, np.zeros(E, bool), np.zeros(E, bool), x)
    assert w.ret_count == E
    w = ref.Wrapper(E, D, norm_reward=False)
    out, _ = w.act(r, np.zeros(E, bool), np.zeros(E, bool), x)
    assert np.array_equal(out, r) and w.ret_count == 0 and not w.returns.any()
