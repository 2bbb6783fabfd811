"""NumPy float32 twins of the two example WORLDS (include/device/dril_env_world.h): examples/envs/rendezvous3_plugin.hip and examples/envs/ringmeet4_plugin.hip, one
statement per product / sum like the sources, vectorised over worlds.  Shared by tests/test_env_world.py (the header's host build, exact) and
tests/test_gpu_env_world.py (the code objects on the device).  A twin is a class with N, S, D, A, discrete and
    fresh(words, key, episode) -> state (S,)         the reset of one world; words(key, episode, block) -> 4 uint32 of Philox stream 0
    obs(st)                    -> (W, N, D)
    step(st, act)              -> state', reward (W, N), terminated (W,)      act: (W, N, A) raw Box actions | (W, N) env-space Discrete actions (0-based)"""
import numpy as np

f = np.float32


def u01(words):
    """DrilEnvRng::u01: [0, 1) from the top 24 bits"""
    return (np.asarray(words, np.uint32) >> 8).astype(f) * f(1.0 / 16777216.0)


class Rendezvous3:
    name, N, S, D, A, discrete, episode_len = "rendezvous3", 3, 12, 8, 2, False, 50
    edge = f(3.0)

    @staticmethod
    def fresh(words, key, episode):
        st = np.zeros(12, f)
        for i in range(3):
            u = u01(words(key, episode, i))
            for k in range(2):
                st[4 * i + k] = (u[k] - f(0.5)) * f(6.0)
                st[4 * i + 2 + k] = u[2 + k] * f(2.0) - f(1.0)
        return st

    @staticmethod
    def obs(st):
        st = st.astype(f).reshape(-1, 3, 4)
        out = np.empty((len(st), 3, 8), f)
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            out[:, i, 0:4] = st[:, i]
            out[:, i, 4:6] = st[:, j, 0:2] - st[:, i, 0:2]
            out[:, i, 6:8] = st[:, k, 0:2] - st[:, i, 0:2]
        return out

    @staticmethod
    def step(st, act):
        st = st.astype(f).reshape(-1, 3, 4).copy(); a = np.clip(act.astype(f), f(-1), f(1)).reshape(-1, 3, 2)
        out = np.zeros(len(st), bool)
        for i in range(3):
            for c in range(2):
                push = f(0.1) * a[:, i, c]
                v = (st[:, i, 2 + c] + push) * f(0.95)
                move = f(0.1) * v
                p = st[:, i, c] + move
                st[:, i, c] = p; st[:, i, 2 + c] = v
                out |= (p < f(-3)) | (p > f(3))
        d2 = np.empty((len(st), 3), f)
        for i in range(3):
            j = (i + 1) % 3
            dx = st[:, j, 0] - st[:, i, 0]
            dy = st[:, j, 1] - st[:, i, 1]
            d2[:, i] = dx * dx + dy * dy
        rew = np.empty((len(st), 3), f)
        for i in range(3):
            h = (i - 1) % 3
            mean = (d2[:, i] + d2[:, h]) * f(0.5)
            act2 = a[:, i, 0] * a[:, i, 0] + a[:, i, 1] * a[:, i, 1]
            rew[:, i] = -mean - f(0.01) * act2
        return st.reshape(-1, 12), rew, out

    @staticmethod
    def near_edge(st, eps):
        """worlds in which some position is within eps of the termination edge (the device may contract a product into an FMA and land on the other side)"""
        p = st.reshape(-1, 3, 4)[:, :, 0:2].reshape(len(st), -1)
        return (np.abs(np.abs(p) - f(3)) < eps).any(axis=1)


class RingMeet4:
    name, N, S, D, A, discrete, episode_len = "ringmeet4", 4, 4, 5, 3, True, 40
    sine = np.array([0.0, 0.382683432, 0.707106781, 0.923879533, 1.0, 0.923879533, 0.707106781, 0.382683432,
                     0.0, -0.382683432, -0.707106781, -0.923879533, -1.0, -0.923879533, -0.707106781, -0.382683432], f)

    @staticmethod
    def offset(a, b):
        d = (b - a + 16) % 16
        return np.where(d > 8, d - 16, d)

    @staticmethod
    def fresh(words, key, episode):
        return (np.asarray(words(key, episode, 0), np.uint32) >> 28).astype(f)

    @classmethod
    def obs(cls, st):
        c = st.astype(np.int64).reshape(-1, 4)
        out = np.empty((len(c), 4, 5), f)
        for i in range(4):
            out[:, i, 0] = cls.sine[c[:, i]]
            out[:, i, 1] = cls.sine[(c[:, i] + 4) % 16]
            for k in range(1, 4):
                out[:, i, 1 + k] = cls.offset(c[:, i], c[:, (i + k) % 4]).astype(f) * f(0.125)
        return out

    @classmethod
    def step(cls, st, act):
        c = st.astype(np.int64).reshape(-1, 4); act = np.asarray(act).reshape(-1, 4)
        move = np.where(act == 0, -1, np.where(act == 2, 1, 0))
        c = (c + move + 16) % 16
        rew = np.empty((len(c), 4), f)
        for i in range(4):
            total = sum(np.abs(cls.offset(c[:, i], c[:, (i + k) % 4])) for k in range(1, 4))
            rew[:, i] = -total.astype(f) * f(0.125)
        return c.astype(f), rew, (c == c[:, :1]).all(axis=1)

    @staticmethod
    def near_edge(st, eps):
        return np.zeros(len(st), bool)                      # integer state: exact throughout


TWINS = {"rendezvous3": Rendezvous3, "ringmeet4": RingMeet4}


# ---- the case the GPU test of the env verbs runs (tests/test_gpu_env_world.py), shared with the CPU check that the twin alone stays clear of the edge ---------
VERB_CASES = {"rendezvous3": 86, "ringmeet4": 65}           # W: E = 258 (world 85 = rows 255..257 straddles the observe launch's workgroup boundary) and E = 260
VERB_STEPS, VERB_LIMIT, VERB_ENV_SEED, VERB_ACTION_SEED, EDGE_EPS, LEFT_OUT_CAP = 60, 7, 3, 1, 1e-5, 0.02


def raw_actions(twin, rng, W):
    """raw policy actions of one step: Discrete(3, action_start = 1) -> 1..3; Box -> beyond the bounds, so that the clamp is exercised"""
    return rng.integers(1, 4, (W, twin.N)).astype(np.int32) if twin.discrete else rng.uniform(-1.5, 1.5, (W, twin.N, twin.A)).astype(f)


def env_actions(twin, raw):
    return raw - 1 if twin.discrete else raw


def twin_alone_rows_near_the_edge(twin, words, W, steps=VERB_STEPS, limit=VERB_LIMIT, env_seed=VERB_ENV_SEED, action_seed=VERB_ACTION_SEED):
    """the verb test's run on the twin alone -> (rows whose termination flag would be left out, rows in all)"""
    N = twin.N
    st = np.stack([twin.fresh(words, env_seed + w * N, 0) for w in range(W)])
    sc = np.zeros(W, np.int64); ep = np.zeros(W, np.int64)
    rng = np.random.default_rng(action_seed)
    left_out = 0
    for _ in range(steps):
        st, _, term = twin.step(st, env_actions(twin, raw_actions(twin, rng, W)))
        left_out += int(twin.near_edge(st, EDGE_EPS).sum()) * N
        sc += 1
        for w in np.nonzero(term | (sc >= limit))[0]:
            ep[w] += 1; sc[w] = 0
            st[w] = twin.fresh(words, env_seed + w * N, ep[w])
    return left_out, steps * W * N
