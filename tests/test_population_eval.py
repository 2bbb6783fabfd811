"""CPU: dril_population_evaluate_device (docs/population.md, "Evaluation"), without a GPU.

  * include/dril_hip.h declares the verb and struct dril_population_eval_info, and _capi.py mirrors both: same arity, same field order, offsets and size
    (a three-line C program compiled with g++ prints sizeof / offsetof);
  * the Julia shim's new ccall and struct pass the static check;
  * the library builds and exports the symbol;
  * evaluate_population refuses unequal or empty lists before any native call."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
VERB, ARITY = "dril_population_evaluate_device", 7


def test_header_and_ctypes_mirror(tmp_path):
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as entry
    capi = entry.load_package()._capi
    header = (ROOT / "include" / "dril_hip.h").read_text()
    assert "#define DRIL_ABI_VERSION 2u" in header and capi.ABI_VERSION == 2                     # untouched
    proto = re.search(r"\b" + VERB + r"\(([^;]*)\);", header)
    assert proto, f"{VERB} is not declared in include/dril_hip.h"
    assert len([a for a in proto.group(1).split(",") if a.strip()]) == ARITY
    assert VERB in capi.EXPORTED_SYMBOLS and len(capi._SIG[VERB][1]) == ARITY and capi._SIG[VERB][0] is C.c_int32
    cm = re.search(r"typedef struct dril_population_eval_info\s*\{(.*?)\}\s*dril_population_eval_info;", header, re.S)
    assert cm, "struct dril_population_eval_info is not declared in include/dril_hip.h"
    declared = []
    for decl in re.sub(r"/\*.*?\*/", "", cm.group(1), flags=re.S).split(";"):
        if decl.strip():
            declared += [re.sub(r"\[.*\]", "", n).strip() for n in decl.strip().split(None, 1)[1].split(",")]
    fields = [n for n, _ in capi.DrilPopulationEvalInfo._fields_]
    assert fields == declared == ["launches", "looks", "batched_members", "solo_members", "kernel_ms", "reserved"]
    body = 'printf("%zu", sizeof(dril_population_eval_info));' + "".join(f'printf(" %zu", offsetof(dril_population_eval_info, {f}));' for f in fields)
    src = tmp_path / "layout.cpp"; exe = tmp_path / "layout"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dril_hip.h"\nint main(){' + body + "return 0;}\n")
    subprocess.run(["g++", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    want = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert [C.sizeof(capi.DrilPopulationEvalInfo)] + [getattr(capi.DrilPopulationEvalInfo, f).offset for f in fields] == want


def test_shim_check_passes_with_the_evaluation_ccall():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0 and "check_shim: ok" in r.stdout, r.stdout[-2000:]
    shim = (ROOT / "dril.jl_amd" / "julia" / "DRiLHIP.jl").read_text()
    assert f"(:{VERB}, LIB[])" in shim and "struct DrilPopulationEvalInfo" in shim
    assert "function DRiL.evaluate_agent(agents::Vector, envs::Vector{<:DeviceParallelEnv};" in shim
    assert '("dril_population_eval_info", "DrilPopulationEvalInfo")' in (ROOT / "tools" / "check_shim.py").read_text()   # the struct's fields are among those the check compares


def test_library_builds_and_exports_the_verb():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as entry
    entry.build()
    so = ROOT / "dril.jl_amd" / "csrc" / "libdril_hip.so"
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    assert VERB in {line.split()[-1] for line in out.splitlines() if line.strip()}
    pkg = entry.load_package()
    assert {"evaluate_population", "Population"} <= set(dir(pkg)) and hasattr(pkg.Population, "evaluate")


def test_evaluate_population_argument_handling(pkg, monkeypatch):
    """lists of unequal length and an empty list raise before any native call"""
    def no_native(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(pkg.host.Handle, "__init__", no_native)
    monkeypatch.setattr(pkg.host.DeviceParallelEnv, "bind", no_native)
    alg = pkg.PPO()
    env = lambda: pkg.DeviceParallelEnv(pkg.CartPoleEnv(), 4)
    agent = lambda: pkg.Agent(pkg.ActorCriticLayer(pkg.CartPoleEnv().observation_space(), pkg.CartPoleEnv().action_space()), alg)
    with pytest.raises(ValueError, match="empty"):
        pkg.evaluate_population([], [])
    with pytest.raises(ValueError, match="2 agents and 1 envs"):
        pkg.evaluate_population([agent(), agent()], [env()])
    with pytest.raises(TypeError):
        pkg.evaluate_population([agent()], [object()])
