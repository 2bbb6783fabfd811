"""NumPy restatement of the verb-level call order of a DRIL_ENV_EXTERNAL SAC handle under NormalizeWrapperEnv / MonitorWrapperEnv (dril_sac_ext_collection_begin /
dril_sac_ext_act_device / dril_sac_ext_push_device / dril_sac_predict_actions_device, include/dril_sac.h) over tests/sac_normalize_ref.py's Wrapper and
tests/ext_wrap_ref.py's Monitor, for tests/test_sac_ext_wrap.py (checked there against replay_through) and tests/test_gpu_sac_ext_wrap.py.  Not a test module."""
import numpy as np

F = np.float32


class NotBegun(RuntimeError):
    """an act with the normaliser on and no collection begun since enable / set_stats / reset: DRIL_ERR_NOT_INITIALISED on the device"""


class ExtVerbs:
    """w: sac_normalize_ref.Wrapper or None (normaliser off); monitor: ext_wrap_ref.Monitor or None.  push returns the ring row of the step"""

    def __init__(self, w=None, monitor=None):
        self.w, self.mon, self.begun, self.live, self.pending = w, monitor, False, False, None

    def collection_begin(self):
        if self.w is not None:
            self.begun = True

    def invalidate(self):
        """enable / set_stats / normalize_reset"""
        self.begun = self.live = False

    def reset(self):
        self.w.returns[:] = 0
        self.invalidate()

    def act(self, d_obs):
        """-> the observation the actor reads (the handle's pending observation)"""
        d_obs = np.asarray(d_obs, F)
        if self.w is None:
            self.pending = d_obs.copy()
            return self.pending
        if not (self.begun or self.live):
            raise NotBegun("dril_sac_ext_collection_begin")
        if self.begun:
            cur = self.w.observe(d_obs)                                              # the opening observe(env): the one act that updates the statistics
        else:
            self.w.old_obs = d_obs.copy(); cur = self.w.normalize_obs(d_obs)         # the statistics in force: what the preceding push stored as next observation
        self.begun, self.live, self.pending = False, True, cur
        return cur

    def predict_obs(self, d_obs):
        """what dril_sac_predict_actions_device feeds the actor: the statistics in force, nothing updated"""
        return np.asarray(d_obs, F).copy() if self.w is None else self.w.normalize_obs(d_obs)

    def push(self, rew, term, trunc, next_obs, terminal_obs=None):
        """terminal_obs None: the caller states that nobody was truncated; a truncated flag set all the same keeps next_obs in the row (the sticky error)"""
        rew, next_obs = np.asarray(rew, F), np.asarray(next_obs, F)
        tr = np.asarray(trunc, bool)
        if self.mon is not None:
            self.mon.act(rew, term, trunc)                                           # inside the normaliser: raw rewards
        use_t = tr & (terminal_obs is not None)
        if self.w is None:
            nxt = np.where(use_t[:, None], next_obs if terminal_obs is None else terminal_obs, next_obs)
            return dict(obs=self.pending, rew=rew.copy(), next=nxt.astype(F), term=np.asarray(term, np.uint8), trunc=np.asarray(trunc, np.uint8), sticky=bool((tr & ~use_t).any()))
        with np.errstate(invalid="ignore"):                                          # rows of terminal_obs that are not the env's to give may hold NaN: never selected
            rn, tn = self.w.act(rew, term, trunc, next_obs if terminal_obs is None else terminal_obs)   # the statistics BEFORE this push's observe
        nxt = self.w.observe(next_obs)
        return dict(obs=self.pending, rew=rn, next=np.where(use_t[:, None], tn, nxt).astype(F), term=np.asarray(term, np.uint8), trunc=np.asarray(trunc, np.uint8),
                    sticky=bool((tr & ~use_t).any()))


def run_script(v, sc, T, k, first=0, tobs_none=()):
    """k collections of T steps of a script (obs[steps + 1], rew, term, trunc, tobs per step) through the verbs, from step `first` -> the ring fields, time-major.
    Steps in tobs_none, and steps in which nobody is truncated, pass terminal_obs = None"""
    rows = []
    for c in range(k):
        v.collection_begin()
        for t in range(first + c * T, first + (c + 1) * T):
            v.act(sc["obs"][t])
            tobs = sc["tobs"][t] if sc["trunc"][t].any() and t not in tobs_none else None
            rows.append(v.push(sc["rew"][t], sc["term"][t], sc["trunc"][t], sc["obs"][t + 1], tobs))
    return {f: np.stack([r[f] for r in rows]) for f in ("obs", "rew", "next", "term", "trunc")}
