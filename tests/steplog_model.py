"""The step log's rules (include/agx_steplog.h) on top of tests/history_model.py's HistoryModel: which rows a record writes, and
the walk of gather with its fold in np.float32, one rounding per operation.  Bookkeeping only, no pixels."""
import numpy as np

from history_model import HistoryModel  # noqa: F401  (the model this one sits on)

TERMINATED, TRUNCATED = 1, 2
F32 = np.float32


class StepLogModel:
    def __init__(self, history, payload_bytes=0):
        self.h, self.W = history, int(payload_bytes)
        T, N = history.T, history.N
        self.reward = np.zeros((T, N), F32)
        self.flags = np.zeros((T, N), np.uint8)
        self.stamp = np.full((T, N), -1, np.int64)
        self.payload = np.zeros((T, N, self.W), np.uint8)

    def clear(self):
        self.stamp[:] = -1

    def record(self, index, reward, flags, payload=None):
        h = self.h
        for n in range(h.N):
            k, cnt = int(index[n]), int(h.count[n])
            if k < 0 or not cnt - h.T <= k < cnt:
                continue
            t = k % h.T
            self.reward[t, n], self.flags[t, n], self.stamp[t, n] = F32(reward[n]), flags[n], k
            if self.W:
                self.payload[t, n] = payload[n]

    def gather(self, n, k, nstep, gamma):
        """-> (steps, next_index, ret f32, discount f32, flags, payload row | None); steps = 0: the rest is None."""
        h, gamma = self.h, F32(gamma)
        m, G, disc, last = 0, F32(0), F32(1), 0
        if 0 <= n < h.N and 0 <= k < int(h.count[n]) and k >= int(h.count[n]) - h.T:
            cnt = int(h.count[n])
            for i in range(1, nstep + 1):
                j = k + i
                if j >= cnt or h.age[j % h.T, n] == 0 or self.stamp[j % h.T, n] != j:
                    break
                G = F32(G + F32(disc * self.reward[j % h.T, n]))
                disc = F32(disc * gamma)
                m, last = i, int(self.flags[j % h.T, n])
                if last & (TERMINATED | TRUNCATED):
                    break
        if m == 0:
            return 0, -1, None, None, None, None
        return m, k + m, G, F32(0) if last & TERMINATED else disc, last, self.payload[(k + 1) % h.T, n].copy()


def fold(rewards, gamma):
    """The float32 fold of a list of rewards -> (ret, gamma ** len) as np.float32."""
    G, disc, gamma = F32(0), F32(1), F32(gamma)
    for r in rewards:
        G = F32(G + F32(disc * F32(r)))
        disc = F32(disc * gamma)
    return G, disc


def bits(x):
    """The int32 bit pattern(s) of float32 value(s)."""
    return np.asarray(x, F32).view(np.int32)
