"""The minibatcher of include/agx_minibatch.h in NumPy and Python integers: the rule of the LIVE and BOOT lists, their offsets,
the keyed permutation (Python ints masked to 64 bits), take with its wrap and its invalid rows, and scatter.  Nothing here is
shared with active-gym_amd/csrc/agx_minibatch_math.h."""
import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
LIVE, BOOT = 0, 1
BOOT_BIT = 8
STREAMS = 8
ROUNDS = 6


def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sm(s, i):
    return mix(s + (i + 1) * GOLD)


def clamp_len(length, L):
    return np.clip(np.asarray(length, np.int64), 0, L)


def selected(which, length, ends, L):
    """bool [L, N]: the rule."""
    live = np.arange(L)[:, None] >= L - clamp_len(length, L)[None, :]
    return live if which == LIVE else live & ((np.asarray(ends) & BOOT_BIT) != 0)


def offsets(which, length, ends, L):
    """off i64 [N + 1]: the exclusive prefix sum of the per-env counts."""
    return np.concatenate([[0], np.cumsum(selected(which, length, ends, L).sum(0))]).astype(np.int64)


def half_bits(total):
    return max(1, (int(total - 1).bit_length() + 1) // 2)


def perm(ek, total, m, rounds=ROUNDS):
    hb = half_bits(total)
    mask = (1 << hb) - 1
    x = m
    while True:
        l, r = x >> hb, x & mask
        for i in range(rounds):
            l, r = r, l ^ (mix(ek + (i + 1) * GOLD + r) & mask)
        x = (l << hb) | r
        if x < total:
            return x


def slot_at(which, off, length, ends, L, m):
    """(slot element or -1, env) at list position m of the offsets `off`, looked up in these length / ends."""
    N = len(off) - 1
    n = int(np.searchsorted(off, m, side="right")) - 1          # the last n with off[n] <= m: an env without slots is never found
    n = min(max(n, 0), N - 1)
    r = m - int(off[n])
    live = int(clamp_len(length, L)[n])
    if which == LIVE:
        return ((L - live + r) * N + n, n) if r < live else (-1, n)
    seen = 0
    for t in range(L - live, L):
        if int(ends[t, n]) & BOOT_BIT:
            if seen == r:
                return t * N + n, n
            seen += 1
    return -1, n


class Model:
    """The state of one agx_minibatch: base and calls per list, and what the last select of each list left."""

    def __init__(self, N, seed):
        self.N = N
        self.base = [sm(seed & M64, w) for w in (LIVE, BOOT)]
        self.calls = [0, 0]
        self.key = [0, 0]
        self.off = [np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64)]

    def select(self, which, length, ends, L):
        self.off[which] = offsets(which, length, ends, L)
        self.key[which] = sm(self.base[which], self.calls[which])
        self.calls[which] += 1
        return int(self.off[which][-1])

    def take(self, which, permute, length, ends, L, first, S, obs_index=None, next_index=None, payload=None, streams=()):
        """-> dict of slot, env, valid, obs_index, next_index, payload [S, W], streams (a list of f32 [S])."""
        off, total = self.off[which], int(self.off[which][-1])
        W = 0 if payload is None else payload.shape[-1]
        out = dict(slot=np.full(S, -1, np.int32), env=np.zeros(S, np.int32), valid=np.zeros(S, np.uint8), obs_index=np.full(S, -1, np.int64),
                   next_index=np.full(S, -1, np.int64), payload=np.zeros((S, W), np.uint8), streams=[np.zeros(S, np.float32) for _ in streams])
        if total == 0:
            return out
        for i in range(S):
            p = first + i
            m = p % total
            if permute:
                m = perm(self.key[which], total, m)
            e, n = slot_at(which, off, length, ends, L, m)
            if e < 0:
                continue
            out["slot"][i], out["env"][i], out["valid"][i] = e, n, p < total
            if obs_index is not None:
                out["obs_index"][i] = obs_index.reshape(-1)[e]
            if next_index is not None:
                out["next_index"][i] = next_index.reshape(-1)[e]
            if W:
                out["payload"][i] = payload.reshape(-1, W)[e]
            for k, src in enumerate(streams):
                out["streams"][k][i] = src.reshape(-1)[e]
        return out


def scatter(slot, valid, src, dst):
    """dst (f32 [L, N]) with src[i] at element slot[i] where valid[i] and the slot is in range; returns the copy."""
    dst = dst.copy()
    flat = dst.reshape(-1)
    for i in range(len(slot)):
        if valid[i] and 0 <= slot[i] < flat.size:
            flat[slot[i]] = src[i]
    return dst


def rollout_arrays(seed, N, L, W=12, n_f32=8):
    """Synthetic arrays of a gathered rollout for the minibatcher: len mixes 0, L and values between (and, where N allows, one
    below 0 and one above L, which are clamped), ends carries random bits - BOOT on slots that are not live included -, the
    indices, the payload and the f32 streams are random."""
    rng = np.random.default_rng(seed)
    length = rng.integers(0, L + 1, N).astype(np.int32)
    length[rng.random(N) < 0.25] = 0
    length[rng.random(N) < 0.25] = L
    if N >= 5:
        length[1], length[3] = -2, L + 3
    ends = rng.integers(0, 16, (L, N)).astype(np.uint8)
    return dict(len=length, ends=ends, obs_index=rng.integers(0, 1 << 40, (L, N)).astype(np.int64),
                next_index=rng.integers(0, 1 << 40, (L, N)).astype(np.int64), payload=rng.integers(0, 256, (L, N, W), dtype=np.uint8),
                streams=[rng.standard_normal((L, N)).astype(np.float32) for _ in range(n_f32)])
