"""PrioritizedSampler — ctypes view of include/agx_priority.h: a device-side prioritized replay sampler on the frame history.

The uniform ReplaySampler draws every accepted (env, index) pair alike; learners of the Rainbow / Ape-X / R2D2 family draw
proportionally to a priority and correct with importance weights.  The priorities live in a table next to the history, a stamp
and a fixed-point weight per retained env-step; a pair nobody has updated yet has the largest weight seen so far::

    hist = FrameHistory(pipe, capacity=100_000)
    log = StepLog(hist, payload_bytes=4)
    per = PrioritizedSampler(hist, back=0, forward=1, seed=0)
    ...
    batch = log.batch(per, 256, nstep=3)                        # the rows are drawn with probability weight / total
    w = per.importance(beta=0.4)                                # f32 [256], 1.0 for the rarest row drawn, 0 where ok == 0
    loss = (w * huber(td_error)).mean()
    per.update_td(batch["env"], batch["index"], td_error)       # (|td| + eps) ** alpha; rows that were evicted are skipped

``(n, k)`` can be drawn iff the uniform sampler would accept it (replay.py); its probability is its weight over the sum of all
such weights, exactly: the weights are integers (priority 1.0 is 65536) and the draw is the pure integer function of (seed, call
number, device state) the header spells out; ``tests/priority_model.py`` restates it in Python ints.

The entry points live in libagx.so, in a header and a binding of their own (active_gym/_native.py is unchanged)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native as nat
from .lifetime import Owner
from .replay import SPAN_LIMIT

_P = C.c_void_p
ONE = 65536                           # the weight of priority 1.0

SIGNATURES = {
    "agx_priority_create": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(_P)]),
    "agx_priority_destroy": (C.c_int, [_P]),
    "agx_priority_bytes": (C.c_int64, [_P]),
    "agx_priority_seed": (C.c_int, [_P, C.c_uint64, _P]),
    "agx_priority_clear": (C.c_int, [_P, _P]),
    "agx_priority_update": (C.c_int, [_P, _P, _P, _P, C.c_int32, _P]),
    "agx_priority_lookup": (C.c_int, [_P, _P, _P, C.c_int32, _P, _P]),
    "agx_priority_sample": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def check_priority_args(back: int, forward: int):
    """ValueError, before any GPU work, for arguments outside the header's ranges.  Returns them as ints."""
    back, forward = int(back), int(forward)
    if not 0 <= back <= SPAN_LIMIT:
        raise ValueError(f"back must be 0 .. {SPAN_LIMIT}, got {back}")
    if not 0 <= forward <= SPAN_LIMIT:
        raise ValueError(f"forward must be 0 .. {SPAN_LIMIT}, got {forward}")
    return back, forward


def check_td_args(alpha, eps):
    """ValueError, before any GPU work, for an exponent or offset that gives no priority."""
    alpha, eps = float(alpha), float(eps)
    if not alpha >= 0:
        raise ValueError(f"alpha must be >= 0, got {alpha}")
    if not eps >= 0:
        raise ValueError(f"eps must be >= 0, got {eps}")
    return alpha, eps


class PrioritizedSampler(Owner):
    _closed_what = "the prioritized sampler or its history"

    def __init__(self, history, back: int = 0, forward: int = 1, seed: int = 0):
        """history: a FrameHistory; back / forward: as ReplaySampler's (what may be drawn at all); seed: the sequence's seed (u64)."""
        self.back, self.forward = check_priority_args(back, forward)
        self._lib = lib()
        self.history = history
        self.pipe = history.pipe
        self.device = history.device
        self._t = _P()
        nat.check(self._lib.agx_priority_create(history.handle, self.back, self.forward, C.byref(self._t)), self.pipe._ctx)
        # the table holds the history's raw handle: it goes before the history does, which also clears it with itself
        self._own(self._t, self._lib.agx_priority_destroy, (history,))
        self._total = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self._accepted = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self.weight = torch.zeros((0,), dtype=torch.int64, device=self.device)      # the integer weights of the last draw
        self._ok = torch.zeros((0,), dtype=torch.uint8, device=self.device)
        if int(seed):
            self.seed(seed)

    def _check(self, rc):
        nat.check(rc, self.pipe._ctx)

    def seed(self, s: int):
        """Restart the sequence: (seed, calls = 0), on the current stream."""
        self._live()
        self._check(self._lib.agx_priority_seed(self._t, int(s) & 0xFFFFFFFFFFFFFFFF, self.pipe._stream()))

    def clear(self):
        """Every row unset, wmax back to priority 1.0, on the current stream.  FrameHistory.clear() calls this."""
        self._live()
        self._check(self._lib.agx_priority_clear(self._t, self.pipe._stream()))

    def bytes(self) -> int:
        """Device bytes the table and its scratch hold (their own allocation: history.nbytes is unchanged)."""
        self._live()
        return int(self._lib.agx_priority_bytes(self._t))

    def sample(self, B: int, env_out: Optional[torch.Tensor] = None, index_out: Optional[torch.Tensor] = None,
               ok_out: Optional[torch.Tensor] = None, weight_out: Optional[torch.Tensor] = None):
        """Draw B samples on the current stream -> (env i32 [B], index i64 [B], ok u8 [B]), each with probability weight / total
        (ReplaySampler.sample's triple: StepLog.batch takes either).  With nothing to draw every sample is (-1, -1, 0).
        ``.weight``, ``.total()``, ``.accepted()`` describe this draw until the next one."""
        self._live()
        B = int(B)
        if B < 0:
            raise ValueError(f"B must be >= 0, got {B}")
        new = self.pipe._out
        env_out, pe = new(env_out, (B,), torch.int32, "env_out")
        index_out, pi = new(index_out, (B,), torch.int64, "index_out")
        ok_out, po = new(ok_out, (B,), torch.uint8, "ok_out")
        weight_out, pw = new(weight_out, (B,), torch.int64, "weight_out")
        self._check(self._lib.agx_priority_sample(self._t, B, pe, pi, po, pw, _P(self._total.data_ptr()), _P(self._accepted.data_ptr()),
                                                  self.pipe._stream()))
        self.weight, self._ok = weight_out, ok_out
        return env_out, index_out, ok_out

    def total(self) -> torch.Tensor:
        """i64 [1] on the device: the sum of the weights the last sample() drew from (0 before the first)."""
        return self._total

    def accepted(self) -> torch.Tensor:
        """i64 [1] on the device: the number of pairs the last sample() could draw."""
        return self._accepted

    def probability(self) -> torch.Tensor:
        """f64 [B]: weight / total of the last draw's rows (0 where ok == 0)."""
        return self.weight.to(torch.float64) / self._total.clamp(min=1).to(torch.float64)

    def importance(self, beta: float = 0.4) -> torch.Tensor:
        """f32 [B]: the importance weights of the last draw, (accepted * weight / total) ** -beta in float64, divided by their
        maximum over the ok rows, rounded once to float32; 0 where ok == 0."""
        ok = self._ok != 0
        zero = torch.zeros((), dtype=torch.float64, device=self.device)
        p = self._accepted.to(torch.float64) * self.weight.to(torch.float64) / self._total.to(torch.float64)
        raw = torch.where(ok, p ** -float(beta), zero)              # (0 / 0 where nothing could be drawn: no row is ok there)
        if raw.numel():
            raw = torch.where(ok, raw / raw.max(), zero)
        return raw.to(torch.float32)

    def update(self, env: torch.Tensor, index: torch.Tensor, priority: torch.Tensor):
        """Set the priority (f32 [B], already raised to the caller's alpha) of the samples (env[b], index[b]).  A sample that is
        no longer retained, or has env or index -1, is skipped; a sample that occurs twice gets one of its priorities."""
        self._live()
        b, pe, pi = self.pipe._pair(env, index)
        pp = self.pipe._chk(priority, (b,), torch.float32, "priority")
        self._check(self._lib.agx_priority_update(self._t, pe, pi, pp, b, self.pipe._stream()))

    def update_td(self, env: torch.Tensor, index: torch.Tensor, td_error: torch.Tensor, alpha: float = 0.6, eps: float = 1e-6):
        """update() with priority = (|td_error| + eps) ** alpha."""
        alpha, eps = check_td_args(alpha, eps)
        self.update(env, index, ((td_error.to(torch.float32).abs() + eps) ** alpha).contiguous())

    def lookup(self, env: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
        """i64 [B]: the integer weight a draw would give each retained sample (ONE = 65536 is priority 1.0; an unset row has
        the largest weight written so far), -1 for a sample that is not retained."""
        self._live()
        b, pe, pi = self.pipe._pair(env, index)
        out = torch.empty((b,), dtype=torch.int64, device=self.device)
        self._check(self._lib.agx_priority_lookup(self._t, pe, pi, b, _P(out.data_ptr()), self.pipe._stream()))
        return out
