"""The chunker of include/agx_chunks.h in NumPy and Python integers: which chunks of a gathered rollout hold a live step, their
list and its offsets, take with its wrap, its null rows and its padding.  The keyed permutation is tests/minibatch_model.py's (the
header says it is the minibatcher's); nothing here is shared with active-gym_amd/csrc/agx_chunk_math.h."""
import numpy as np

import minibatch_model as mm

LIST = 2                                  # AGX_CHUNK_LIST
LIMIT = 256                               # AGX_CHUNK_LIMIT
START_CHUNK, START_EPISODE = 1, 2
BREAK = 7

STEP_KEYS = ("slot", "env", "obs_index", "next_index", "payload", "ends", "start", "mask")
CHUNK_KEYS = ("chunk", "first", "steps", "state_index", "valid")


def groups(L, C):
    return -(-L // C)


def live_steps(length, L, C):
    """bool [G, C, N]: step (g, l) of env n is live."""
    t = np.arange(groups(L, C) * C).reshape(-1, C)[:, :, None]
    t0 = (L - mm.clamp_len(length, L))[None, None, :]
    return (t >= t0) & (t < L)


def selected(length, L, C):
    """bool [G, N]: the chunk holds a live step (the definition, not the closed form)."""
    return live_steps(length, L, C).any(1)


def offsets(length, L, C):
    return np.concatenate([[0], np.cumsum(selected(length, L, C).sum(0))]).astype(np.int64)


def chunk_at(off, length, L, C, m):
    """(n, g) at list position m of the offsets `off`, looked up in this length, or None: the r-th chunk of env n that holds a
    live step, by walking the env's chunks."""
    N = len(off) - 1
    n = min(max(int(np.searchsorted(off, m, side="right")) - 1, 0), N - 1)
    r = m - int(off[n])
    mine = np.nonzero(selected(np.asarray(length)[n:n + 1], L, C)[:, 0])[0]
    return (n, int(mine[r])) if 0 <= r < len(mine) else None


class Model:
    """The state of one agx_chunks: base, calls, and what the last select left."""

    def __init__(self, N, seed):
        self.N = N
        self.base = mm.sm(seed & mm.M64, LIST)
        self.calls = 0
        self.key = 0
        self.off = np.zeros(N + 1, np.int64)
        self.seen = (0, 0)                # (L, C)

    def select(self, length, L, C):
        self.off = offsets(length, L, C)
        self.seen = (L, C)
        self.key = mm.sm(self.base, self.calls)
        self.calls += 1
        return int(self.off[-1])

    def take(self, permute, length, ends, L, C, first, S, obs_index=None, next_index=None, payload=None, streams=()):
        """-> dict of the per-step outputs [C, S] (payload [C, S, W], streams a list of f32 [C, S]) and the per-chunk ones [S]."""
        N, total = self.N, int(self.off[-1])
        W = 0 if payload is None else payload.shape[-1]
        out = dict(slot=np.full((C, S), -1, np.int32), env=np.zeros((C, S), np.int32), obs_index=np.full((C, S), -1, np.int64),
                   next_index=np.full((C, S), -1, np.int64), payload=np.zeros((C, S, W), np.uint8), ends=np.zeros((C, S), np.uint8),
                   start=np.zeros((C, S), np.uint8), mask=np.zeros((C, S), np.uint8), streams=[np.zeros((C, S), np.float32) for _ in streams],
                   chunk=np.full(S, -1, np.int32), first=np.zeros(S, np.int32), steps=np.zeros(S, np.int32), state_index=np.full(S, -1, np.int64),
                   valid=np.zeros(S, np.uint8))
        if total == 0 or self.seen != (L, C):
            return out
        clamped = mm.clamp_len(length, L)
        for s in range(S):
            p = first + s
            m = p % total
            if permute:
                m = mm.perm(self.key, total, m)
            at = chunk_at(self.off, length, L, C, m)
            if at is None:
                continue
            n, g = at
            t0 = L - int(clamped[n])
            ts = [t for t in range(g * C, (g + 1) * C) if t0 <= t < L]
            valid = p < total
            out["chunk"][s], out["first"][s], out["steps"][s], out["valid"][s] = g, ts[0] - g * C, len(ts), valid
            if obs_index is not None:
                out["state_index"][s] = obs_index[ts[0], n]
            out["env"][:, s] = n
            for t in ts:
                l = t - g * C
                out["slot"][l, s] = t * N + n
                out["ends"][l, s] = ends[t, n]
                out["mask"][l, s] = valid
                out["start"][l, s] = (START_CHUNK if t == ts[0] else 0) | (START_EPISODE if t > t0 and int(ends[t - 1, n]) & BREAK else 0)
                if obs_index is not None:
                    out["obs_index"][l, s] = obs_index[t, n]
                if next_index is not None:
                    out["next_index"][l, s] = next_index[t, n]
                if W:
                    out["payload"][l, s] = payload[t, n]
                for k, src in enumerate(streams):
                    out["streams"][k][l, s] = src[t, n]
        return out


def rollout_arrays(seed, N, L, W=12, n_f32=8, empty=False):
    """Synthetic arrays of a gathered rollout for the chunker: len mixes 0, L and values between and, where N allows, -3 and L + 7
    (both clamped); ends carries random bits, 1 / 2 / 4 inside live runs included; the f32 streams hold NaN and inf at the slots
    that are not live; the indices and the payload are random.  empty: every len is 0."""
    rng = np.random.default_rng(seed)
    length = rng.integers(0, L + 1, N).astype(np.int32)
    length[rng.random(N) < 0.2] = 0
    length[rng.random(N) < 0.2] = L
    if N >= 3:
        length[0], length[2] = L + 7, -3
    if N >= 5:
        length[4] = max(L - 1, 0)
    if empty:
        length[:] = 0
    ends = rng.integers(0, 16, (L, N)).astype(np.uint8)
    ends[rng.random((L, N)) < 0.5] &= 8
    live = np.arange(L)[:, None] >= L - np.clip(length, 0, L)[None, :]
    streams = []
    for k in range(n_f32):
        s = rng.standard_normal((L, N)).astype(np.float32)
        s[~live] = (np.nan, np.inf, -np.inf)[k % 3]
        streams.append(s)
    return dict(len=length, ends=ends, obs_index=rng.integers(0, 1 << 40, (L, N)).astype(np.int64),
                next_index=rng.integers(0, 1 << 40, (L, N)).astype(np.int64), payload=rng.integers(0, 256, (L, N, W), dtype=np.uint8),
                streams=streams)
