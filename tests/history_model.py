"""NumPy model of the frame history's bookkeeping only (include/agx_history.h): per-env count, age per row, the index a push
returns, validity of a sample, and which row feeds stack position j.  No pixels: the tests compare pixels against what the
step itself returned."""
import numpy as np

CLEAR, SKIP = 0x04, 0x08


class HistoryModel:
    def __init__(self, num_envs, frame_stack, capacity):
        self.N, self.fs, self.T = int(num_envs), int(frame_stack), int(capacity)
        self.count = np.zeros(self.N, np.int64)
        self.age = np.zeros((self.T, self.N), np.int64)
        self.start_age = -1          # a new history: zeros before an env's first append; after clear(): unknown (254 -> 255)

    def clear(self):
        self.count[:] = 0
        self.start_age = 254

    def push(self, cmd):
        """cmd u8 [N] as the ingest read it -> index i64 [N] (-1: skipped)."""
        out = np.full(self.N, -1, np.int64)
        for n, c in enumerate(np.asarray(cmd)):
            if c & SKIP:
                continue
            k = self.count[n]
            prev = self.age[(k - 1) % self.T, n] if k > 0 else self.start_age
            self.age[k % self.T, n] = 0 if c & CLEAR else min(prev + 1, 255)
            out[n] = k
            self.count[n] = k + 1
        return out

    def valid(self, n, k):
        if not (0 <= n < self.N and 0 <= k < self.count[n] and k >= self.count[n] - self.T):
            return False
        first = k - min(self.age[k % self.T, n], self.fs - 1)
        return bool(first >= max(self.count[n] - self.T, 0))

    def rows(self, n, k):
        """For a valid sample: the history index that feeds stack position j (0 = oldest), None for a zero frame."""
        a = self.age[k % self.T, n]
        return [k - (self.fs - 1 - j) if self.fs - 1 - j <= a else None for j in range(self.fs)]
