"""Host (NumPy) observations: the way home from the device.  :class:`_HostObsPool` recycles pinned buffers behind fresh-array
semantics; :class:`HostObs` is what a vector env with ``device=None`` owns - the ``copy_obs=False`` pinned pair or the pool,
and the pageable copy where neither serves."""
from __future__ import annotations

import numpy as np
import torch


class _HostObsPool:
    """Fresh-array semantics for host (NumPy) observations at pinned-buffer cost.

    The reference's envs hand out a new array per call (atari_env.py:143 ``np.stack``), so a caller may keep any of them.  A
    device-to-PAGEABLE copy into a fresh 115 MB array costs 30+ ms per step at N = 1024 (page faults of the fresh mapping +
    the staged copy); a copy into PINNED memory 2 ms.  The pool hands out NumPy views of pinned buffers and takes a buffer back
    only when the array it handed out - and every view derived from it - has been garbage collected (``weakref.finalize`` on
    the array: derived views keep their base alive).  A caller that drops its observations as it goes (the usual loop) cycles
    through 2-3 buffers; one that keeps them all gets ``max_buffers`` pinned ones and ordinary pageable arrays after that.
    """

    def __init__(self, max_buffers: int):
        import collections
        self.max_buffers = int(max_buffers)
        self._free = collections.deque()         # append / pop are atomic: finalizers may run on any thread
        self._made = 0
        self._shape = None

    def take(self, shape, dtype):
        """A pinned tensor no array refers to, or None (budget spent: the caller falls back to a pageable array)."""
        shape = tuple(shape)
        if self._shape != (shape, dtype):       # another observation shape: start over (outstanding arrays keep their buffers)
            self._free.clear()
            self._made = 0
            self._shape = (shape, dtype)
        try:
            return self._free.pop()
        except IndexError:
            pass
        if self._made >= self.max_buffers:
            return None
        self._made += 1
        return torch.empty(shape, dtype=dtype, pin_memory=True)

    def hand_out(self, buf: torch.Tensor) -> np.ndarray:
        import weakref
        arr = buf.numpy()
        key = self._shape
        weakref.finalize(arr, self._give_back, buf, key).atexit = False      # nothing to recycle at interpreter shutdown
        return arr

    def _give_back(self, buf, key):
        if key == self._shape:
            self._free.append(buf)


class HostObs:
    """``pinned_pair``: args.copy_obs = False (gymnasium's SyncVectorEnv(copy=False)) - views of two PINNED host buffers used
    alternately (4 ms at N = 1024): an observation then stays valid until the step after next, as with device outputs.
    Otherwise a fresh array per call, like the reference's envs: fresh-array SEMANTICS from a pool of ``pool_buffers`` pinned
    buffers that are recycled once the caller has dropped the array (_HostObsPool; 0 restores the pageable copy per call)."""

    # below 1 MB of observations (the single-env wrappers: 113 KB) a pageable copy is as cheap as the pool's bookkeeping
    min_elems = 1 << 18

    def __init__(self, device, pinned_pair: bool, pool_buffers: int):
        self.device = device
        self.pinned_pair = bool(pinned_pair)
        self.pool = _HostObsPool(pool_buffers) if (not self.pinned_pair and pool_buffers > 0) else None
        self._pair = None
        self._pair_i = 0

    def take(self, obs: torch.Tensor):
        """A pinned destination for an observation like ``obs``: the next buffer of the pinned pair, or one from the pool.  None
        when the pool's budget is spent, or there is no pool."""
        if self.pinned_pair:
            if self._pair is None or tuple(self._pair[0].shape) != tuple(obs.shape):
                self._pair = [torch.empty(tuple(obs.shape), dtype=obs.dtype, pin_memory=True) for _ in range(2)]
            self._pair_i ^= 1
            return self._pair[self._pair_i]
        return self.pool.take(obs.shape, obs.dtype) if self.pool is not None else None

    def hand_out(self, h: torch.Tensor) -> np.ndarray:
        """The array the caller gets for a filled destination of take()."""
        return h.numpy() if self.pinned_pair else self.pool.hand_out(h)

    def fetch(self, obs: torch.Tensor) -> np.ndarray:
        """Copy a device observation to the host: through take() - the pool only from ``min_elems`` elements up - or, without a
        pinned destination, into a pageable array."""
        h = self.take(obs) if (self.pinned_pair or obs.numel() >= self.min_elems) else None
        if h is None:
            return obs.cpu().numpy()
        h.copy_(obs, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self.hand_out(h)
