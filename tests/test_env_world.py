"""CPU: WORLDS — the multi-agent form of a device env plug-in (include/device/dril_env_world.h, DRIL_ENV_PLUGIN_WORLD: N agents, one shared state, one joint step; the
device form of MultiAgentParallelEnv) without a GPU.

  * the two examples cross-compile for gfx950 into the symbols of a classic plug-in, with `agents` = N in the descriptor's former `reserved` word (0 in cartpole's);
  * the header's host build (-DDRIL_ENV_PLUGIN_HOST, g++ -ffp-contract=off) against the NumPy float32 twins of tests/env_world_twins.py, exactly, and the wrapper's
    order per world: flags and counters shared by a world's rows, rewards per agent, terminal observations of all N rows, the world's seed, monitor sums per row;
  * what the library cannot take fails at the world's own compile, with a message that names the limit."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from env_world_twins import TWINS
from test_env_plugin import ENVS, GENCO, Desc, HostEnv, _PV


def _words(oracle_mod):
    def words(key, episode, block):
        w = np.zeros(4, np.uint32)
        oracle_mod.lib().orc_philox(int(key), int(episode), 0, 0, int(block), w.ctypes.data_as(_PV))
        return w
    return words


# ---- the examples as gfx950 code objects ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,agents", [("rendezvous3", 3), ("ringmeet4", 4), ("cartpole", 0)])
def test_worlds_compile_for_gfx950_into_the_symbols_of_a_plugin(name, agents, tmp_path):
    co = tmp_path / f"{name}.hsaco"
    subprocess.run(GENCO + [str(ENVS / f"{name}_plugin.hip"), "-o", str(co)], check=True)
    blob = co.read_bytes()
    assert blob[:4] == b"\x7fELF"
    syms = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "-s", str(co)], capture_output=True, text=True, check=True).stdout
    for s in ("dril_env_plugin_reset", "dril_env_plugin_observe", "dril_env_plugin_step"):
        assert f" {s}\n" in syms and f" {s}.kd\n" in syms, s
    if agents:
        for s in ("dril_env_plugin_obs_space", "dril_env_plugin_observe_scaled", "dril_env_plugin_step_scaled", "dril_env_plugin_rollout", "dril_env_plugin_evaluate"):
            assert f" {s}\n" not in syms, s                                    # a world emits no optional entry
    line = next(l for l in syms.splitlines() if l.endswith(" dril_env_plugin_desc"))
    assert int(line.split()[2]) == C.sizeof(Desc) == 608 and "OBJECT" in line and "GLOBAL" in line     # the descriptor's size is unchanged
    # the descriptor's bytes, read out of the ELF section that holds the symbol
    secs = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "-S", "-W", str(co)], capture_output=True, text=True, check=True).stdout
    ndx = int(line.split()[6]); addr = int(line.split()[1], 16)
    sec = next(l for l in secs.splitlines() if l.strip().startswith(f"[{ndx:2d}]") or l.strip().startswith(f"[{ndx}]"))
    cols = sec.split("]", 1)[1].split()
    sec_addr, sec_off = int(cols[2], 16), int(cols[3], 16)
    d = Desc.from_buffer_copy(blob[sec_off + addr - sec_addr: sec_off + addr - sec_addr + C.sizeof(Desc)])
    assert d.abi_version == 1 and d.reserved == agents, (d.abi_version, d.reserved)
    if agents:
        t = TWINS[name]
        assert (d.S, d.D, d.A, bool(d.discrete), d.episode_len) == (t.S, t.D, t.A, t.discrete, t.episode_len)


# ---- the host build against the twins ------------------------------------------------------------------------------------------------------------------
class WorldHost(HostEnv):
    """W worlds of a world plug-in's host build: E = W N rows; world w's state at float offset w S of the (over-allocated) E x S state array"""

    def __init__(self, twin, tmp, W, seed, **kw):
        super().__init__(twin.name, tmp, W * twin.N, seed, **kw)
        assert self.desc.reserved == twin.N and (self.S, self.D, self.A, self.discrete) == (twin.S, twin.D, twin.A, twin.discrete)
        self.W, self.N = W, twin.N

    @property
    def worlds(self):
        return self.state.reshape(-1)[: self.W * self.S].reshape(self.W, self.S)


@pytest.mark.parametrize("name", ["rendezvous3", "ringmeet4"])
def test_host_build_of_a_world_follows_the_numpy_twin_and_the_wrapper_keeps_its_order(oracle_mod, name, tmp_path):
    twin = TWINS[name]
    W, L, seed, T, N, D = 5, 7, 100, 60, twin.N, twin.D
    E = W * N
    words = _words(oracle_mod)
    m = WorldHost(twin, tmp_path, W, seed, episode_len=L, monitor=True); m.reset()
    assert m.desc.episode_len == twin.episode_len and not m.sc.any() and not m.ep.any() and not m.gs.any()
    for w in range(W):
        assert np.array_equal(m.worlds[w], twin.fresh(words, seed + w * N, 0)), w      # world w is keyed by the row index of its agent 0: seed0 + w N
    assert not m.state.reshape(-1)[W * twin.S:].any()                                   # nothing is written past the W states
    st = m.worlds.copy()
    if name == "rendezvous3":                                                          # world 0: agent 1 leaves the arena at once — a termination of the whole world
        m.worlds[0, 4] = st[0, 4] = np.float32(2.99); m.worlds[0, 6] = st[0, 6] = np.float32(1.0)
    else:                                                                              # world 0: three agents on cell 3, the fourth steps onto it
        m.worlds[0] = st[0] = np.array([3, 3, 3, 4], np.float32)
    rng = np.random.default_rng(3)
    cur_ret = np.zeros(E, np.float32); cur_len = np.zeros(E, np.int64); episode = np.zeros(W, np.int64)
    saw_term = saw_trunc = differ = False
    for t in range(T):
        assert np.array_equal(m.observe(), twin.obs(st).reshape(E, D)), t
        if twin.discrete:
            raw = rng.integers(1, 4, (W, N)).astype(np.int32)                          # Discrete(3, action_start = 1): 1..3
            if t == 0:
                raw[0] = [2, 2, 2, 1]                                                  # stay, stay, stay, left
            env_act = raw - 1
        else:
            raw = rng.uniform(-1.5, 1.5, (W, N, twin.A)).astype(np.float32)            # beyond the Box: the clamp per agent and dimension is exercised
            env_act = raw
        before = raw.copy()
        want_st, want_r, want_term = twin.step(st, env_act)
        sc_before = m.sc.copy()
        rew, term, trunc, tobs, nxt = m.step(raw.reshape(E, -1) if not twin.discrete else raw.reshape(E))
        assert np.array_equal(raw, before)                                             # the raw action stays as it was
        assert np.array_equal(rew, want_r.reshape(E))                                  # each agent its own reward ...
        differ |= bool((np.ptp(rew.reshape(W, N), axis=1) > 0).any())
        assert np.array_equal(term, np.repeat(want_term, N))                           # ... the world's flags in all N rows
        want_trunc = sc_before.reshape(W, N)[:, 0] + 1 >= L
        assert np.array_equal(trunc, np.repeat(want_trunc, N))
        cur_ret += rew; cur_len += 1
        done = want_term | want_trunc
        rows_trunc = np.repeat(want_trunc, N)
        assert np.array_equal(tobs[rows_trunc], twin.obs(want_st).reshape(E, D)[rows_trunc])      # terminal observations of ALL N rows, of the state before the reset
        assert not tobs[~rows_trunc].any()
        for w in np.nonzero(done)[0]:
            rows = slice(w * N, (w + 1) * N)
            assert np.array_equal(m.ep_ret[rows], cur_ret[rows]) and np.array_equal(m.ep_len[rows], cur_len[rows])       # the monitor's sums are per row
            cur_ret[rows] = 0; cur_len[rows] = 0; episode[w] += 1
            want_st[w] = twin.fresh(words, seed + w * N, episode[w])                   # episode k of world w: key seed0 + w N, counter k
        assert np.array_equal(m.worlds, want_st) and np.array_equal(nxt, twin.obs(want_st).reshape(E, D))
        assert np.array_equal(m.mon_ret, cur_ret) and np.array_equal(m.mon_len, cur_len)
        for counter in (m.sc, m.ep, m.gs):                                             # the three counters: per-row arrays, equal within a world
            assert (counter.reshape(W, N) == counter.reshape(W, N)[:, :1]).all()
        assert np.array_equal(m.ep.reshape(W, N)[:, 0], episode) and (m.gs == t + 1).all()
        assert (m.sc.reshape(W, N)[done] == 0).all() and np.array_equal(m.sc.reshape(W, N)[~done, 0], sc_before.reshape(W, N)[~done, 0] + 1)
        st = want_st; saw_term |= bool(want_term.any()); saw_trunc |= bool(want_trunc.any())
    assert saw_term and saw_trunc and differ
    # fixed_length_episodes suppresses the world's termination
    g = WorldHost(twin, tmp_path, 2, seed, episode_len=3, fixed_len=True); g.reset()
    if name == "rendezvous3":
        g.worlds[:, 0] = 5.0
        act = np.zeros((2 * N, twin.A), np.float32)
    else:
        g.worlds[:] = 3.0
        act = np.full(2 * N, 2, np.int32)                                              # everybody stays on the shared cell
    _, want_term = twin.step(g.worlds.copy(), act.reshape(2, N, -1) if not twin.discrete else act.reshape(2, N) - 1)[1:]
    assert want_term.all()
    _, term, trunc, _, _ = g.step(act)
    assert not term.any() and not trunc.any()


# ---- what the library cannot take fails at the world's own compile ---------------------------------------------------------------------------------------
BAD = """#include "device/dril_env_world.h"
%s
struct Bad {
    static constexpr int N = %d;
    static constexpr int S = %d, D = 2, A = 2;
    static constexpr bool discrete = %s;
    static constexpr int episode_len = 10;
    %s
    static constexpr const char* name = "Bad";
    DRIL_ENV_FN static void reset(const DrilEnvRng&, float* st) { st[0] = 0.f; }
    DRIL_ENV_FN static void observe(const float* st, int agent, float* obs) { obs[0] = st[0]; obs[1] = (float)agent; }
    DRIL_ENV_FN static void step(float* st, const float*, const int*, float* rew, bool* t) { for (int i = 0; i < N; ++i) rew[i] = st[0]; *t = false; }
};
DRIL_ENV_PLUGIN_WORLD(Bad)
%s
"""
BOUNDS = "static constexpr float action_low[A] = {-1, -1}, action_high[A] = {1, 1};"


@pytest.mark.parametrize("N,S,discrete,bounds,fused,message", [
    (1, 4, "false", BOUNDS, "", "N (agents per world) must be 2..16"),
    (17, 4, "false", BOUNDS, "", "N (agents per world) must be 2..16"),
    (3, 257, "false", BOUNDS, "", "S (state floats per world) must be 1..256"),
    (3, 4, "false", "", "", "a continuous world (discrete = false) must define static constexpr float action_low[A] and action_high[A]"),
    (3, 4, "false", BOUNDS, "DRIL_ENV_PLUGIN_ROLLOUT(Bad)", "a world (DRIL_ENV_PLUGIN_WORLD) has no fused rollout or evaluation yet"),
])
def test_a_world_the_library_cannot_take_fails_at_its_own_compile(N, S, discrete, bounds, fused, message, tmp_path):
    src = tmp_path / "bad.hip"
    src.write_text(BAD % ('#include "device/dril_env_rollout.h"' if fused else "", N, S, discrete, bounds, fused))
    r = subprocess.run(GENCO + [str(src), "-o", str(tmp_path / "bad.hsaco")], capture_output=True, text=True)
    assert r.returncode != 0 and message in r.stderr, r.stderr[-2000:]
    if fused:
        assert r.stderr.count("error:") == 1, r.stderr[-3000:]                         # the one static_assert, nothing after it


def test_the_control_world_compiles(tmp_path):
    """the same source with acceptable numbers: the refusals above are the limits' and nothing else's (N = 16 and S = 256 are the last sizes taken)"""
    ok = tmp_path / "ok.hip"
    ok.write_text(BAD % ("", 16, 256, "false", BOUNDS, ""))
    subprocess.run(GENCO + [str(ok), "-o", str(tmp_path / "ok.hsaco")], check=True)


@pytest.mark.parametrize("name", ["rendezvous3", "ringmeet4"])
def test_the_gpu_verb_tests_action_seed_keeps_the_twin_clear_of_the_termination_edge(oracle_mod, name):
    """tests/test_gpu_env_world.py leaves a row's termination flag out where the twin's state is within 1e-5 of the edge (the device may contract a product into an
    FMA); with its action seed the twin alone leaves out at most 2 % of the rows"""
    import env_world_twins as tw
    left_out, rows = tw.twin_alone_rows_near_the_edge(TWINS[name], _words(oracle_mod), tw.VERB_CASES[name])
    assert rows == 60 * tw.VERB_CASES[name] * TWINS[name].N and left_out <= tw.LEFT_OUT_CAP * rows, (left_out, rows)
