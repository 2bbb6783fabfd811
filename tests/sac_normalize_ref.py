"""NumPy restatement of NormalizeWrapperEnv (src/environment_wrappers/normalizeWrapperEnv.jl) in the reference's float32 arithmetic and call order, for
tests/test_sac_normalize.py (checked there against a float64 Welford) and tests/test_gpu_sac_normalize.py (the SAC handle's device wrapper is compared with it).
Not a test module.  Batch moments come from float64 sums, as on the device (docs/deviations.md); everything after them is float32."""
import numpy as np

F = np.float32


def merge(mean, var, count, bmean, bvar, bcount):
    """update_from_moments! (:28-50) -> (mean, var, count)"""
    bmean, bvar = np.asarray(bmean, F), np.asarray(bvar, F)
    if count == 0:
        return bmean.copy(), bvar.copy(), bcount
    tot = count + bcount
    delta = bmean - mean
    new_mean = mean + delta * F(bcount) / F(tot)
    m2 = var * F(count) + bvar * F(bcount) + delta * delta * F(count) * F(bcount) / F(tot)
    return new_mean.astype(F), (m2 / F(tot)).astype(F), tot


def batch_moments(x):
    """mean / var(corrected = false) over the env axis (axis 0) from float64 sums -> float32"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    m = x.sum(0) / n
    v = np.maximum((x * x).sum(0) / n - m * m, 0.0)
    return m.astype(F), v.astype(F)


class Wrapper:
    def __init__(self, E, D, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8):
        self.E, self.D = E, D
        self.training, self.norm_obs, self.norm_reward = bool(training), bool(norm_obs), bool(norm_reward)
        self.clip_obs, self.clip_reward, self.gamma, self.eps = F(clip_obs), F(clip_reward), F(gamma), F(epsilon)
        self.obs_mean, self.obs_var, self.obs_count = np.zeros(D, F), np.ones(D, F), 0
        self.ret_mean, self.ret_var, self.ret_count = np.zeros((), F), np.ones((), F), 0
        self.returns = np.zeros(E, F)
        self.old_obs, self.old_rew = np.zeros((E, D), F), np.zeros(E, F)

    def set_stats(self, st):
        self.obs_mean, self.obs_var, self.obs_count = np.array(st["obs_mean"], F), np.array(st["obs_var"], F), int(st["obs_count"])
        self.ret_mean, self.ret_var, self.ret_count = np.array(st["ret_mean"], F), np.array(st["ret_var"], F), int(st["ret_count"])

    def normalize_obs(self, x):
        x = np.asarray(x, F)
        if not self.norm_obs:
            return x.copy()
        return np.clip((x - self.obs_mean) / np.sqrt(self.obs_var + self.eps), -self.clip_obs, self.clip_obs).astype(F)

    def observe(self, raw):
        """observe (:123-137): raw (E, D)"""
        self.old_obs = np.array(raw, F)
        if self.training and self.norm_obs:
            self.obs_mean, self.obs_var, self.obs_count = merge(self.obs_mean, self.obs_var, self.obs_count, *batch_moments(raw), self.E)
        return self.normalize_obs(raw)

    def act(self, rew, term, trunc, terminal_obs):
        """act! (:139-165) after the env's own act!: -> (normalised rewards, normalised terminal observations (rows of truncated envs are meaningful))"""
        rew = np.asarray(rew, F)
        self.old_rew = rew.copy()
        if self.training and self.norm_reward:
            self.returns = (self.returns * self.gamma + rew).astype(F)
            self.ret_mean, self.ret_var, self.ret_count = merge(self.ret_mean, self.ret_var, self.ret_count, *batch_moments(self.returns), self.E)
        out = rew.copy()
        if self.norm_reward:
            out = np.clip(rew / np.sqrt(self.ret_var + self.eps), -self.clip_reward, self.clip_reward).astype(F)
        done = np.asarray(term, bool) | np.asarray(trunc, bool)
        self.returns[done] = 0
        return out, self.normalize_obs(terminal_obs)

    def stats(self):
        return dict(obs_mean=self.obs_mean, obs_var=self.obs_var, obs_count=self.obs_count, ret_mean=float(self.ret_mean), ret_var=float(self.ret_var), ret_count=self.ret_count)


def replay_through(w, raw, cur_obs, T, k):
    """the ring a wrapped handle must hold after k collections of T steps, from the raw ring of a twin handle without the wrapper (time-major fields shaped
    (k T, E, ...)) and the twin's current observation: collect_trajectories' call order (off_policy_collection.jl:42-61)"""
    E = w.E
    O = np.concatenate([raw["obs"], cur_obs[None]], 0)
    exp = dict(obs=np.empty_like(raw["obs"]), rew=np.empty_like(raw["rew"]), next=np.empty_like(raw["next"]))
    for c in range(k):
        cur = w.observe(O[c * T])
        for t in range(c * T, (c + 1) * T):
            rn, tob = w.act(raw["rew"][t], raw["term"][t], raw["trunc"][t], raw["next"][t])
            nxt = w.observe(O[t + 1])
            exp["obs"][t], exp["rew"][t] = cur, rn
            exp["next"][t] = np.where(raw["trunc"][t].astype(bool)[:, None], tob, nxt)
            cur = nxt
    return exp
