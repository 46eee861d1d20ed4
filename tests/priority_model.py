"""The prioritized sampler's rules (include/agx_priority.h) on top of tests/history_model.py's HistoryModel, in NumPy and Python
ints: quantise, the table (stamps, weights, wmax), update, lookup and the draw of one call.  Acceptance, SM and the env search
are tests/replay_model.py's, by import: the prioritized and the uniform sampler share one statement of them.  Not a test."""
import bisect

import numpy as np

from replay_model import M64, SM, accepted, find_env

ONE = 65536                       # the weight of priority 1.0; wmax of a new / cleared table
WEIGHT_MAX = 0xFFFFFFFF


def quantise(p):
    """f32 priority -> fixed-point weight (never 0), in float32 arithmetic as the header states it."""
    p = np.float32(p)
    if not p > 0:
        return 1
    with np.errstate(over="ignore"):
        q = np.float32(p * np.float32(65536.0))
    if q >= np.float32(4294967296.0):
        return WEIGHT_MAX
    return max(int(q), 1)


class Table:
    """stamp i64 / weight per history row, [T][N] like the model's age (the layout is nobody's business), and wmax."""

    def __init__(self, model):
        self.model = model
        self.clear()

    def clear(self):
        m = self.model
        self.stamp = np.full((m.T, m.N), -1, np.int64)
        self.weight = np.zeros((m.T, m.N), np.int64)
        self.wmax = ONE


def retained(model, n, k):
    return 0 <= n < model.N and max(int(model.count[n]) - model.T, 0) <= k < int(model.count[n])


def update(model, table, env, index, priority):
    """One agx_priority_update.  Duplicates must carry equal priorities (which one is stored is unspecified)."""
    for n, k, p in zip(np.asarray(env).tolist(), np.asarray(index).tolist(), np.asarray(priority, np.float32)):
        if retained(model, n, k):
            w = quantise(p)
            table.stamp[k % model.T, n], table.weight[k % model.T, n] = k, w
            table.wmax = max(table.wmax, w)


def effective(model, table, n, k):
    """The effective weight of a retained (n, k)."""
    return int(table.weight[k % model.T, n]) if table.stamp[k % model.T, n] == k else table.wmax


def lookup(model, table, n, k):
    return effective(model, table, n, k) if retained(model, n, k) else -1


def weights(model, table, back, forward):
    """Per env: (lo_n, [W(n, k) for k = lo_n .. cnt - 1]) as Python ints."""
    out = []
    for n in range(model.N):
        cnt = int(model.count[n])
        lo = max(cnt - model.T, 0)
        out.append((lo, [effective(model, table, n, k) if accepted(model, n, k, back, forward) else 0 for k in range(lo, cnt)]))
    return out


def draw(model, table, back, forward, seed, call, B):
    """One call of agx_priority_sample -> (env i32 [B], index i64 [B], ok u8 [B], weight i64 [B], total, accepted)."""
    per_env = weights(model, table, back, forward)
    off, incl = [0], []
    for _, w in per_env:
        acc, run = [], 0
        for v in w:
            run += v
            acc.append(run)                       # P(n, k) + W(n, k)
        incl.append(acc)
        off.append(off[-1] + run)
    total = off[-1]
    n_acc = sum(v > 0 for _, w in per_env for v in w)
    key = SM(seed & M64, call)
    env, idx, ok, wt = np.full(B, -1, np.int32), np.full(B, -1, np.int64), np.zeros(B, np.uint8), np.zeros(B, np.int64)
    if total > 0:
        for b in range(B):
            u = (SM(key, b) * total) >> 64
            n = find_env(off, u)
            v = u - off[n]
            at = bisect.bisect_right(incl[n], v)      # the first row with P + W > v: P <= v < P + W
            env[b], idx[b], ok[b], wt[b] = n, per_env[n][0] + at, 1, per_env[n][1][at]
    return env, idx, ok, wt, total, n_acc
