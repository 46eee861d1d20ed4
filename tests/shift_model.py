"""The random-shift augmentation's rules (include/agx_augment.h) in Python ints and NumPy: the shift map, the draw of one call,
and the gather of an unshifted batch that the GPU tests hold the kernel against.  Bookkeeping only."""
import numpy as np

from replay_model import M64, SM

PAD_LIMIT = 32


def shift_src(i, d, pad, n):
    """The source coordinate of output coordinate i under shift d (0 .. 2 * pad) along an axis of n elements."""
    return min(max(i + d - pad, 0), n - 1)


def clamp(d, pad):
    """A shift component as the device takes it."""
    return min(max(int(d), 0), 2 * pad)


def pair(key, b, pad):
    """Sample b of the draw with `key` -> (dy, dx)."""
    z = SM(key, b & M64)
    m = 2 * pad + 1
    return ((z >> 32) * m) >> 32, ((z & 0xFFFFFFFF) * m) >> 32


def draw(seed, call, B, pad):
    """Call number `call` (0 first) of a source seeded with `seed` -> i32 [B, 2] as (dy, dx)."""
    key = SM(seed & M64, call)
    return np.array([pair(key, b, pad) for b in range(B)], np.int32).reshape(B, 2)


def src_index(shift, pad, n):
    """shift components d [B] -> the source coordinates i64 [B][n] of an axis of n elements."""
    d = np.clip(np.asarray(shift, np.int64), 0, 2 * pad)
    return np.clip(np.arange(n, dtype=np.int64)[None, :] + d[:, None] - pad, 0, n - 1)
