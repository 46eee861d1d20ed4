"""The replay sampler's rules (include/agx_replay.h) on top of tests/history_model.py's HistoryModel, in NumPy and Python ints:
the candidates, the acceptance predicate, SM, the draw of one call, and inspect.  Bookkeeping only, no pixels."""
import bisect

import numpy as np

from history_model import CLEAR, SKIP

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def commands(seed, N, steps, p_clear=0.15, p_skip=0.15):
    """The command bytes of a run, u8 [steps][N]: nvalid 1 | 2, about p_clear CLEAR, about p_skip SKIP (as
    tests/test_gpu_history.py draws them: the seed of a case is chosen on the model alone)."""
    rng = np.random.default_rng(seed)
    cmd = rng.integers(1, 3, (steps, N)).astype(np.uint8)
    cmd |= (rng.random((steps, N)) < p_clear).astype(np.uint8) * CLEAR
    cmd |= (rng.random((steps, N)) < p_skip).astype(np.uint8) * SKIP
    return cmd


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def SM(s, i):
    """The i-th output (i = 0 first) of splitmix64 seeded with s."""
    return mix((s + (i + 1) * GOLDEN) & M64)


def splitmix64(s, count):
    """The definition: the generator's state advances by the golden gamma, each output is the finaliser of the new state."""
    out = []
    for _ in range(count):
        s = (s + GOLDEN) & M64
        out.append(mix(s))
    return out


def age(model, n, k):
    return int(model.age[k % model.T, n])


def candidates(model, forward):
    """(lo [N], L [N], off [N + 1]) as Python ints."""
    lo = [max(int(c) - model.T, 0) for c in model.count]
    L = [max(int(c) - int(forward) - l, 0) for c, l in zip(model.count, lo)]
    off = [0]
    for l in L:
        off.append(off[-1] + l)
    return lo, L, off


def accepted(model, n, k, back, forward):
    """The three conditions of the header, each by its own statement."""
    if not model.valid(n, k):
        return False
    b = min(int(back), age(model, n, k))
    if not model.valid(n, k - b):
        return False
    cnt = int(model.count[n])
    return k + forward < cnt and age(model, n, k + forward) >= forward


def accepted_set(model, back, forward):
    return [(n, k) for n in range(model.N) for k in range(-1, int(model.count[n]) + 1) if accepted(model, n, k, back, forward)]


def find_env(off, u):
    """The env n with off[n] <= u < off[n + 1] (Python ints: no width to overflow)."""
    return bisect.bisect_right(off, u) - 1


def pick(key, b, attempts, a, lo, off):
    """Attempt a of sample b -> the candidate (n, k) it lands on (total > 0)."""
    z = SM(key, (b * attempts + a) & M64)
    u = (z * off[-1]) >> 64
    n = find_env(off, u)
    return n, lo[n] + u - off[n]


def draw(model, back, forward, attempts, seed, call, B):
    """One call of agx_replay_sample -> (env i32 [B], index i64 [B], ok u8 [B], total)."""
    lo, _, off = candidates(model, forward)
    total = off[-1]
    key = SM(seed & M64, call)
    env, idx, ok = np.full(B, -1, np.int32), np.full(B, -1, np.int64), np.zeros(B, np.uint8)
    if total > 0:
        for b in range(B):
            for a in range(attempts):
                n, k = pick(key, b, attempts, a, lo, off)
                if accepted(model, n, k, back, forward):
                    env[b], idx[b], ok[b] = n, k, 1
                    break
    return env, idx, ok, total


def inspect(model, n, k):
    """(age, ahead) of a sample: (-1, -1) for an invalid one."""
    if not model.valid(n, k):
        return -1, -1
    cnt, f = int(model.count[n]), 0
    while f < 255 and k + f + 1 < cnt and age(model, n, k + f + 1) != 0:
        f += 1
    return age(model, n, k), f
