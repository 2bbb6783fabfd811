"""NumPy restatement of MonitorWrapperEnv (src/environment_wrappers/monitorWrapperEnv.jl) for tests/test_ext_wrap.py (the record kernel's per-env rules under
g++) and tests/test_gpu_ext_wrap.py (the monitor of an external handle on the device).  Not a test module."""
import numpy as np

F = np.float32


class Monitor:
    """MonitorWrapperEnv (monitorWrapperEnv.jl): per-env running return (float32, step order) and length; finished episodes enter a CircularBuffer of W in
    (step, env) order; log_stats reports the means over it"""

    def __init__(self, E, W):
        self.cur_ret, self.cur_len, self.W, self.window = np.zeros(E, F), np.zeros(E, np.int32), W, []

    def act(self, rew, term, trunc):
        self.cur_ret = (self.cur_ret + np.asarray(rew, F)).astype(F); self.cur_len = self.cur_len + 1
        for e in np.nonzero(np.asarray(term, bool) | np.asarray(trunc, bool))[0]:
            self.window.append((F(self.cur_ret[e]), int(self.cur_len[e]))); self.window = self.window[-self.W:]
            self.cur_ret[e] = 0; self.cur_len[e] = 0

    def stats(self):
        n = len(self.window)
        if n == 0:
            return 0.0, 0.0, 0
        return float(F(np.sum([float(r) for r, _ in self.window]) / n)), float(F(np.sum([l for _, l in self.window]) / n)), n
