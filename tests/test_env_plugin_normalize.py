"""No GPU: the host side of NormalizeWrapperEnv around a device env plug-in of a PPO handle (dril_normalize_*, include/dril_hip.h) — struct layout against the
header, prototypes declared and exported, the Julia shim's ccalls, and the argument checks that come before any GPU work."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
VERBS = ("config_default", "enable", "get_config", "set_training", "get_stats", "set_stats", "get_original", "get_returns")
FIELDS = ("training", "norm_obs", "norm_reward", "clip_obs", "clip_reward", "gamma", "epsilon", "reserved")


def test_normalize_config_layout_matches_c(pkg, tmp_path):
    src = tmp_path / "sz.c"
    offs = ", ".join(f"offsetof(dril_normalize_config, {f})" for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_hip.h"\n#include "dril_sac.h"\nint main(){size_t v[] = {sizeof(dril_normalize_config), sizeof(dril_sac_normalize_config), '
                   + offs + '};\nfor (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]);\nprintf("%d %d\\n", (int)DRIL_ABI_VERSION, (int)sizeof(dril_config));return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    K = pkg._capi.DrilNormalizeConfig
    assert out[0] == out[1] == C.sizeof(K) == 32                                        # the two verb families read alike
    assert out[2:2 + len(FIELDS)] == [getattr(K, f).offset for f in FIELDS]
    assert tuple(n for n, _ in K._fields_) == FIELDS
    assert out[-2] == pkg._capi.ABI_VERSION == 2 and out[-1] == C.sizeof(pkg._capi.DrilConfig)   # dril_config and its ABI number did not move


def test_every_verb_is_declared_typed_and_exported(pkg):
    capi = pkg._capi
    header = (ROOT / "include" / "dril_hip.h").read_text()
    lib = capi.load_library()
    for v in VERBS:
        name = "dril_normalize_" + v
        assert re.search(r"int32_t\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTED_SYMBOLS and name in capi._SIG
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == capi._SIG[name][1]
    # the same shapes as the SAC family, handle type apart
    for v in VERBS:
        a, b = capi._SIG["dril_normalize_" + v][1], capi._SIG["dril_sac_normalize_" + v][1]
        assert len(a) == len(b), v
    h = pkg.Handle.__dict__
    for m in ("normalize_enable", "normalize_config", "normalize_set_training", "normalize_get_stats", "normalize_set_stats", "normalize_get_original", "normalize_get_returns"):
        assert m in h, m


def test_defaults_and_null_handles_without_a_gpu(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    c = capi.DrilNormalizeConfig()
    assert lib.dril_normalize_config_default(None) == capi.ERR_INVALID_ARG
    assert lib.dril_normalize_config_default(C.byref(c)) == capi.OK
    assert (c.training, c.norm_obs, c.norm_reward, c.clip_obs, c.clip_reward, c.reserved) == (1, 1, 1, 10.0, 10.0, 0)     # normalizeWrapperEnv.jl:71-80
    assert abs(c.gamma - 0.99) < 1e-7 and abs(c.epsilon - 1e-8) < 1e-15
    f, i64 = C.c_float(), C.c_int64()
    calls = (lambda: lib.dril_normalize_enable(None, C.byref(c)), lambda: lib.dril_normalize_enable(None, None), lambda: lib.dril_normalize_get_config(None, C.byref(c)),
             lambda: lib.dril_normalize_set_training(None, 1), lambda: lib.dril_normalize_get_stats(None, None, None, C.byref(i64), C.byref(f), C.byref(f), C.byref(i64)),
             lambda: lib.dril_normalize_set_stats(None, None, None, 0, 0.0, 1.0, 0), lambda: lib.dril_normalize_get_original(None, None, None),
             lambda: lib.dril_normalize_get_returns(None, None))
    for call in calls:
        assert call() in (capi.ERR_INVALID_ARG, capi.ERR_NOT_INITIALISED)
        assert b"null handle" in lib.dril_last_error(None)


def test_the_create_time_refusal_stays_and_points_to_the_verb(pkg, tmp_path):
    capi = pkg._capi
    lib = capi.load_library()
    elf = tmp_path / "some.hsaco"; elf.write_bytes(b"\x7fELF" + bytes(60))
    for field in ("norm_obs", "norm_reward"):
        cfg = capi.default_config(capi.ENV_MODULE); setattr(cfg, field, 1)
        h = C.c_void_p()
        assert lib.dril_create_with_env_module(C.byref(cfg), str(elf).encode(), C.byref(h)) == capi.ERR_UNSUPPORTED
        msg = lib.dril_last_error(None)
        assert b"NormalizeWrapperEnv" in msg and b"dril_normalize_enable" in msg


def test_the_julia_shim_passes_the_static_check():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0 and "check_shim: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    jl = (ROOT / "dril.jl_amd" / "julia" / "DRiLHIP.jl").read_text()
    for sym in (":dril_normalize_enable", ":dril_normalize_set_training", ":dril_normalize_get_stats", ":dril_normalize_set_stats"):
        assert sym in jl, sym
    assert "struct DrilNormalizeConfig" in jl and "normalize_enable!(h[], env.normalize)" in jl
