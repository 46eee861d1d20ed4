"""SequenceReplay — ctypes view of include/agx_sequence.h: sequences of L consecutive steps of one episode on a FrameHistory and
its StepLog, padded and masked, for recurrent learners (R2D2 and its family)::

    hist = FrameHistory(pipe, capacity=100_000)
    log = StepLog(hist, payload_bytes=4)
    seq = SequenceReplay(log)
    sampler = ReplaySampler(hist, forward=9, seed=0)             # every drawn start has at least 10 steps of its episode
    ...
    batch = seq.batch(sampler, 64, 80, nstep=5, planes=1)         # obs [64, 80, 1, h, w], live [64, 80], ret, discount, ...
    td = ...                                                      # [64, 80]
    priority = mixed_priority(td.abs(), batch["live"])            # R2D2's eta * max + (1 - eta) * mean over the live steps

Step ``l`` of sample ``b`` is the env-step ``(env[b], index[b] + l)``.  A sequence never crosses a reset, stops at the end of the
history and starts only at a valid sample; ``length[b]`` says how far it goes and step ``l`` is live iff ``l < length[b]``.  Every
other step is padding with DEFINED contents: all-zero observations, ``steps = 0``, ``next_index = -1``, zeros elsewhere - no
output needs a memset.  A live step's rows are bit for bit ``StepLog.gather``'s and ``FrameHistory.observe``'s for that env-step;
``planes = p`` keeps the newest ``p`` stacked frames of each observation (``planes = 1``: the newest frame alone, a quarter of the
bytes at frame_stack 4).  ``tests/sequence_model.py`` restates the length rule in Python ints.

The entry points live in libagx.so, in a header and a binding of their own (active_gym/_native.py is unchanged).  A
SequenceReplay owns no native handle."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native as nat
from .history import _WHAT
from .steplog import check_nstep

_P = C.c_void_p
SEQUENCE_LIMIT = 256                  # AGX_SEQUENCE_LIMIT

SIGNATURES = {
    "agx_sequence_lengths": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "agx_sequence_gather": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "agx_sequence_observe": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int, _P, _P, _P, _P]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def check_length(L) -> int:
    """ValueError, before any GPU work, for a sequence length outside the header's range."""
    n = int(L)
    if not 1 <= n <= SEQUENCE_LIMIT:
        raise ValueError(f"L must be 1 .. {SEQUENCE_LIMIT}, got {n}")
    return n


def check_planes(planes, frame_stack: int) -> int:
    """``planes`` of an observe (None: the whole stack) -> int; ValueError, before any GPU work, outside 1 .. frame_stack."""
    p = int(frame_stack) if planes is None else int(planes)
    if not 1 <= p <= int(frame_stack):
        raise ValueError(f"planes must be 1 .. frame_stack = {int(frame_stack)}, got {p}")
    return p


def check_sequence_draw(length, min_length=None) -> int:
    """The ``forward`` of the sampler that draws the starts of ``env.sequence_batch``: (min_length or length) - 1; ValueError,
    before any GPU work, where a sampler cannot guarantee that many steps."""
    from .replay import SPAN_LIMIT
    L = check_length(length)
    m = L if min_length is None else int(min_length)
    if not 1 <= m <= L:
        raise ValueError(f"min_length must be 1 .. length = {L}, got {m}")
    if m - 1 > SPAN_LIMIT:
        raise ValueError(f"a sampler guarantees at most {SPAN_LIMIT + 1} steps of one episode: pass min_length <= {SPAN_LIMIT + 1} "
                         f"(sequences of length {L} are then padded where their episode is shorter), got min_length = {m}")
    return m - 1


def mixed_priority(td_abs: torch.Tensor, live: torch.Tensor, eta: float = 0.9) -> torch.Tensor:
    """R2D2's sequence priority, [B]: ``eta * max + (1 - eta) * mean`` of ``td_abs`` ([B, L], >= 0) over the live steps of each
    sequence (``live`` [B, L], non-zero = live); 0 for a sequence without a live step.  Plain torch."""
    m = live != 0
    t = torch.where(m, td_abs.to(torch.float32), torch.zeros((), dtype=torch.float32, device=td_abs.device))
    mean = t.sum(1) / m.sum(1).clamp(min=1).to(torch.float32)
    return float(eta) * t.max(1).values + (1.0 - float(eta)) * mean


class SequenceReplay:
    def __init__(self, steplog):
        """steplog: a StepLog; its history is the one the sequences are read from."""
        self._lib = lib()
        self.steplog = steplog
        self.history = steplog.history
        self.pipe = steplog.pipe
        self.device = steplog.device

    def _live(self):
        self.steplog._live()          # (the history closes its logs first: an open log has an open history)

    def _check(self, rc):
        nat.check(rc, self.pipe._ctx)

    def _shape(self, b: int, L: int, time_major: bool):
        return (L, b) if time_major else (b, L)

    def lengths(self, env: torch.Tensor, index: torch.Tensor, L: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """i32 [B]: how many of the L steps from (env[b], index[b]) are live - 0 for a start that is not valid."""
        L = check_length(L)
        self._live()
        b, pe, pi = self.pipe._pair(env, index)
        out, po = self.pipe._out(out, (b,), torch.int32, "out")
        self._check(self._lib.agx_sequence_lengths(self.history.handle, pe, pi, b, L, po, self.pipe._stream()))
        return out

    def gather(self, env: torch.Tensor, index: torch.Tensor, L: int, nstep: int = 1, gamma: float = 0.99, time_major: bool = False) -> dict:
        """The step-log rows of all L steps of each sequence, as a dict: ``length`` i32 [B], and per step ([B, L], or [L, B] with
        time_major) ``steps`` i32, ``next_index`` i64, ``ret`` f32, ``discount`` f32, ``flags`` u8 and ``payload`` u8 [.., W].  A
        live step's row is ``StepLog.gather(nstep, gamma)`` at ``(env, index + l)``; every other row is steps = 0, next_index = -1,
        zeros."""
        L, nstep = check_length(L), check_nstep(nstep)
        self._live()
        b, pe, pi = self.pipe._pair(env, index)
        w, dev, shp = self.steplog.payload_bytes, self.device, self._shape(b, L, time_major)
        out = {"length": torch.empty((b,), dtype=torch.int32, device=dev), "steps": torch.empty(shp, dtype=torch.int32, device=dev),
               "next_index": torch.empty(shp, dtype=torch.int64, device=dev), "ret": torch.empty(shp, dtype=torch.float32, device=dev),
               "discount": torch.empty(shp, dtype=torch.float32, device=dev), "flags": torch.empty(shp, dtype=torch.uint8, device=dev),
               "payload": torch.empty(shp + (w,), dtype=torch.uint8, device=dev)}
        p = {key: _P(t.data_ptr()) for key, t in out.items()}
        self._check(self._lib.agx_sequence_gather(self.steplog._s, pe, pi, b, L, nstep, float(gamma), int(bool(time_major)), p["length"], p["steps"],
                                                  p["next_index"], p["ret"], p["discount"], p["flags"], p["payload"] if w > 0 else None,
                                                  self.pipe._stream()))
        return out

    def obs_row_shape(self, what: str = "fovea", planes: Optional[int] = None):
        """Shape of one step's observation: (planes, h, w)."""
        return (check_planes(planes, self.pipe.frame_stack),) + tuple(self.history.obs_row_shape(what)[1:])

    def observe(self, env: torch.Tensor, index: torch.Tensor, length: torch.Tensor, L: int, what: str = "fovea", planes: Optional[int] = None,
                time_major: bool = False, out: Optional[torch.Tensor] = None, loc_out: Optional[torch.Tensor] = None,
                live_out: Optional[torch.Tensor] = None):
        """The observations of all L steps of each sequence -> (obs [B, L, planes, h, w], fov_loc i32 [B, L, 2], live u8 [B, L]);
        [L, B, ...] with time_major.  ``length``: i32 [B], what ``lengths`` / ``gather`` returned.  Plane p is stack position
        frame_stack - planes + p (planes = None: the whole stack).  A live step holds ``history.observe``'s planes at the recorded
        fov_loc; every other step is all zeros, fov_loc (0, 0), live 0.  fov_loc is not written by a base pipeline."""
        if what not in _WHAT:
            raise ValueError(f"what must be 'fovea' or 'full', got {what!r}")
        L = check_length(L)
        self._live()
        row = self.obs_row_shape(what, planes)
        pipe = self.pipe
        b, pe, pi = pipe._pair(env, index)
        pn = pipe._chk(length, (b,), torch.int32, "length")
        shp = self._shape(b, L, time_major)
        out, po = pipe._out(out, shp + row, pipe.obs_dtype, "out")
        loc_out, pl = pipe._out(loc_out, shp + (2,), torch.int32, "loc_out")
        live_out, pv = pipe._out(live_out, shp, torch.uint8, "live_out")
        self._check(self._lib.agx_sequence_observe(self.history.handle, _WHAT[what], pe, pi, pn, b, L, row[0], int(bool(time_major)), po, pl, pv,
                                                   pipe._stream()))
        return out, loc_out, live_out

    def batch(self, sampler, B: int, L: int, nstep: int = 1, gamma: float = 0.99, planes: Optional[int] = None, time_major: bool = False,
              what: Optional[str] = None) -> dict:
        """``sampler.sample(B)`` (a ReplaySampler or PrioritizedSampler on this history: its ``forward`` + 1 is the guaranteed
        length), ``gather`` and ``observe`` as one dict: env, index, ok (the sampler's ok AND length > 0), length, live, obs,
        fov_loc (fixed pipelines), steps, next_index, ret, discount, flags, payload and next_step - the step of the same sequence
        an n-step target bootstraps from: l + steps where steps > 0 and that step is live, else -1.  what: None takes "fovea" on a
        fixed pipeline and "full" on a base one."""
        L, nstep = check_length(L), check_nstep(nstep)
        check_planes(planes, self.pipe.frame_stack)
        if sampler.history is not self.history:
            raise ValueError("the sampler draws from another history than the one this log is on")
        if what is None:
            what = "fovea" if self.pipe.kind == "fixed" else "full"
        env, index, ok = sampler.sample(B)
        out = self.gather(env, index, L, nstep, gamma, time_major)
        length = out["length"]
        obs, loc, live = self.observe(env, index, length, L, what, planes, time_major)
        steps = out["steps"]
        at = torch.arange(L, dtype=torch.int32, device=self.device)
        at = (at[:, None] if time_major else at[None, :]) + steps
        inside = (steps > 0) & (at < (length[None, :] if time_major else length[:, None]))
        out.update(env=env, index=index, ok=ok & (length > 0).to(torch.uint8), obs=obs, live=live,
                   next_step=torch.where(inside, at, torch.full_like(at, -1)))
        if self.pipe.kind == "fixed":
            out["fov_loc"] = loc
        return out
