"""CPU: populations (dril_population_*, docs/population.md), without a GPU.

  * the block map of ppo_update_small_pop_kernel (dril.jl_amd/csrc/dril_pop_map.h), compiled with g++: member -> (actor block, critic block) for every launch size;
  * the prototypes in include/dril_hip.h (which still compiles as C), their ctypes bindings, the struct layout and the exports of the built library;
  * the Julia shim's new ccalls pass the static check;
  * train_population_ refuses unequal or empty lists before any native call."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
VERBS = {"dril_population_join": 3, "dril_population_destroy": 1, "dril_population_last_error": 1, "dril_population_collect_rollout": 2,
         "dril_population_ppo_update": 2, "dril_population_train": 5, "dril_population_info": 2}


@pytest.fixture(scope="module")
def block_map(tmp_path_factory):
    d = tmp_path_factory.mktemp("popmap")
    src = d / "map.cpp"
    src.write_text('#include <cstdio>\n#include "dril_pop_map.h"\nusing namespace dril;\n'
                   'int main() { for (int n = 1; n <= 64; ++n) { std::printf("%d %d", n, pop_grid(n)); for (int m = 0; m < n; ++m) std::printf(" %d:%d", pop_actor_block(m), pop_critic_block(m));\n'
                   ' std::printf(" |"); for (int b = 0; b < pop_grid(n); ++b) std::printf(" %d:%d", pop_block_member(b), pop_block_role(b)); std::printf("\\n"); } return 0; }\n')
    exe = d / "map"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "dril.jl_amd" / "csrc"), str(src), "-o", str(exe)], check=True)
    rows = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        head, inv = line.split(" |")
        f = head.split()
        rows[int(f[0])] = (int(f[1]), [tuple(int(x) for x in p.split(":")) for p in f[2:]], [tuple(int(x) for x in p.split(":")) for p in inv.split()])
    return rows


def test_block_map(block_map):
    assert sorted(block_map) == list(range(1, 65))
    for n, (grid, pairs, inverse) in block_map.items():
        assert grid == 16 * ((n + 7) // 8) and len(pairs) == n and len(inverse) == grid
        ids = [b for p in pairs for b in p]
        assert len(set(ids)) == 2 * n, f"n = {n}: the map is not injective"
        assert all(0 <= b < grid for b in ids)
        for m, (actor, critic) in enumerate(pairs):
            assert actor % 8 == critic % 8, f"n = {n}, member {m}: the pair does not share an XCD"
            assert (actor, critic) == (16 * (m // 8) + m % 8, 16 * (m // 8) + m % 8 + 8)
            assert inverse[actor] == (m, 0) and inverse[critic] == (m, 1)                          # what a block computes for itself
        idle = [b for b in range(grid) if inverse[b][0] >= n]
        assert sorted(idle) == sorted(set(range(grid)) - set(ids)), f"n = {n}: the blocks without a member are not exactly the rest"
    assert block_map[1][1] == [(0, 8)]                                                            # a lone member sits where ppo_update_small_kernel's pair sits


def test_prototypes_bindings_and_layout(pkg, tmp_path):
    capi = pkg._capi
    header = (ROOT / "include" / "dril_hip.h").read_text()
    assert "#define DRIL_ABI_VERSION 2u" in header and capi.ABI_VERSION == 2                     # untouched
    m = re.search(r"#define DRIL_POPULATION_MAX (\d+)", header)
    assert m and int(m.group(1)) >= 256
    for name, arity in VERBS.items():
        proto = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert proto, f"{name} is not declared in include/dril_hip.h"
        assert len([a for a in proto.group(1).split(",") if a.strip()]) == arity, name
        assert name in capi.EXPORTED_SYMBOLS and len(capi._SIG[name][1]) == arity, name
    fields = tuple(n for n, _ in capi.DrilPopulationInfo._fields_)
    body = 'printf("%zu", sizeof(struct dril_population_info));' + "".join(f'printf(" %zu", offsetof(struct dril_population_info, {f}));' for f in fields)
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_hip.h"\nint main(){' + body + "return 0;}")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)   # the header is C: a struct tag beside the verb of the same name
    want = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert [C.sizeof(capi.DrilPopulationInfo)] + [getattr(capi.DrilPopulationInfo, f).offset for f in fields] == want


def test_library_exports_the_verbs(pkg):
    so = ROOT / "dril.jl_amd" / "csrc" / "libdril_hip.so"
    assert so.exists()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(VERBS) <= exported, sorted(set(VERBS) - exported)
    assert {"Population", "train_population_"} <= set(dir(pkg))


def test_shim_check_passes_with_the_population_ccalls():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0 and "check_shim: ok" in r.stdout, r.stdout[-2000:]
    shim = (ROOT / "dril.jl_amd" / "julia" / "DRiLHIP.jl").read_text()
    for name in ("dril_population_join", "dril_population_destroy", "dril_population_last_error", "dril_population_collect_rollout", "dril_population_ppo_update", "dril_population_info"):
        assert f"(:{name}, LIB[])" in shim, name
    assert "function train!(agents::Vector, envs::Vector{<:DeviceParallelEnv}, algs::Vector{<:PPO}, max_steps::Int)" in shim


def test_train_population_argument_handling(pkg, monkeypatch):
    """lists of unequal length and an empty list raise before any native call (no handle is created, no library symbol is touched)"""
    def no_native(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(pkg.host.Handle, "__init__", no_native)
    monkeypatch.setattr(pkg.host.DeviceParallelEnv, "bind", no_native)
    alg = pkg.PPO()
    env = lambda: pkg.DeviceParallelEnv(pkg.CartPoleEnv(), 4)
    agent = lambda: pkg.Agent(pkg.ActorCriticLayer(pkg.CartPoleEnv().observation_space(), pkg.CartPoleEnv().action_space()), alg)
    with pytest.raises(ValueError, match="empty"):
        pkg.train_population_([], [], [], 8192)
    with pytest.raises(ValueError, match="2 agents, 1 envs and 2 algs"):
        pkg.train_population_([agent(), agent()], [env()], [alg, alg], 8192)
    with pytest.raises(ValueError, match="1 agents, 1 envs and 0 algs"):
        pkg.train_population_([agent()], [env()], [], 8192)
    with pytest.raises(TypeError):
        pkg.train_population_([agent()], [object()], [alg], 8192)
    with pytest.raises(ValueError):
        pkg.Population([])
