"""StepLog — ctypes view of include/agx_steplog.h: reward, end flags and an opaque payload (the action) per retained env-step,
next to a FrameHistory, and one device gather that turns drawn samples into learner rows with n-step targets::

    hist = FrameHistory(pipe, capacity=100_000)
    log = StepLog(hist, payload_bytes=4)                       # 4 bytes per row: the action as one int32
    sampler = ReplaySampler(hist, forward=1, seed=0)
    ...
    index = hist.push(cmd)                                      # observation `index` was produced by `action`, with `reward`
    log.record(index, reward, flags, action.view(torch.uint8).reshape(N, 4))
    ...
    batch = log.batch(sampler, 256, nstep=3, gamma=0.99)        # env, index, ok, obs, next_obs, ret, discount, steps, payload ...
    target = batch["ret"] + batch["discount"] * q(batch["next_obs"]).max(1).values

Row ``k`` of an env holds the data of the step that PRODUCED observation ``k``: the action taken on seeing ``k - 1`` (payload), the
reward received and the end flags of ``k``.  ``gather`` folds rows ``k + 1 .. k + nstep`` of sample ``(env, k)`` and stops at the
episode's end, at a reset, at the end of the history and at a row that was never recorded: a sample with no such row has
``steps = 0`` and its other outputs are left untouched.  The fold is single precision with one rounding per operation;
``tests/steplog_model.py`` restates it in NumPy.  Sequences of L consecutive steps, for recurrent learners, are read through
``active_gym/sequence.py`` (SequenceReplay) on the same log.

The entry points live in libagx.so, in a header and a binding of their own (active_gym/_native.py is unchanged)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _native as nat
from .lifetime import Owner

_P = C.c_void_p
PAYLOAD_LIMIT = 64                    # AGX_STEPLOG_PAYLOAD_LIMIT
NSTEP_LIMIT = 64                      # AGX_STEPLOG_NSTEP_LIMIT
TERMINATED, TRUNCATED = 1, 2          # AGX_STEP_*

SIGNATURES = {
    "agx_steplog_create": (C.c_int, [_P, C.c_int32, C.POINTER(_P)]),
    "agx_steplog_destroy": (C.c_int, [_P]),
    "agx_steplog_clear": (C.c_int, [_P, _P]),
    "agx_steplog_bytes": (C.c_int64, [_P]),
    "agx_steplog_record": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "agx_steplog_gather": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_float, _P, _P, _P, _P, _P, _P, _P]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def check_payload_bytes(payload_bytes) -> int:
    """ValueError, before any GPU work, for a payload width outside the header's range."""
    w = int(payload_bytes)
    if not 0 <= w <= PAYLOAD_LIMIT or w % 4:
        raise ValueError(f"payload_bytes must be 0 .. {PAYLOAD_LIMIT} and a multiple of 4, got {w}")
    return w


def check_nstep(nstep) -> int:
    """ValueError, before any GPU work, for an nstep outside the header's range."""
    m = int(nstep)
    if not 1 <= m <= NSTEP_LIMIT:
        raise ValueError(f"nstep must be 1 .. {NSTEP_LIMIT}, got {m}")
    return m


def check_env_step_log(step_log, history_len, discrete_motor: bool = True) -> bool:
    """``args.step_log`` of a vector env; ValueError, before any GPU work, without a frame history to log next to or on an env
    whose motor action is not one integer per env (the env's payload is the motor action as int32: a float action vector
    would be logged wrong)."""
    on = bool(step_log)
    if on and int(history_len or 0) <= 0:
        raise ValueError("step_log=True needs a frame history (history_len > 0)")
    if on and not discrete_motor:
        raise ValueError("step_log=True needs a discrete motor action (one integer per env): this env's motor actions are float "
                         "vectors, which the env's int32 payload does not hold (keep them in a StepLog of your own)")
    return on


class StepLog(Owner):
    _closed_what = "the step log or its history"

    def __init__(self, history, payload_bytes: int = 0):
        """history: a FrameHistory; payload_bytes: opaque bytes kept per row (0 .. 64, a multiple of 4), the action usually."""
        self.payload_bytes = check_payload_bytes(payload_bytes)
        self._lib = lib()
        self.history = history
        self.pipe = history.pipe
        self.device = history.device
        self.num_envs = history.num_envs
        self._s = _P()
        nat.check(self._lib.agx_steplog_create(history.handle, self.payload_bytes, C.byref(self._s)), self.pipe._ctx)
        # the log holds the history's raw handle: it goes before the history does, which also clears it with itself (its
        # indices restart there)
        self._own(self._s, self._lib.agx_steplog_destroy, (history,))

    def _check(self, rc):
        nat.check(rc, self.pipe._ctx)

    def clear(self):
        """Every row becomes unrecorded, on the current stream.  FrameHistory.clear() calls this for the logs on it."""
        self._live()
        self._check(self._lib.agx_steplog_clear(self._s, self.pipe._stream()))

    def bytes(self) -> int:
        """Device bytes the log holds (its own allocation: history.nbytes is unchanged)."""
        self._live()
        return int(self._lib.agx_steplog_bytes(self._s))

    def record(self, index: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor, payload: Optional[torch.Tensor] = None):
        """Write the rows ``index`` (i64 [N], what history.push returned; -1 skips an env): ``reward`` f32 [N], ``flags`` u8 [N]
        (TERMINATED | TRUNCATED) and ``payload`` u8 [N, W] (None when W = 0).  An index that is not retained is skipped."""
        self._live()
        n, w, chk = self.num_envs, self.payload_bytes, self.pipe._chk
        pi, pr, pf = chk(index, (n,), torch.int64, "index"), chk(reward, (n,), torch.float32, "reward"), chk(flags, (n,), torch.uint8, "flags")
        pp = None
        if w > 0:
            if payload is None:
                raise ValueError(f"this log keeps {w} payload bytes per row: payload must be a uint8 [{n}, {w}] tensor")
            pp = chk(payload, (n, w), torch.uint8, "payload")
        self._check(self._lib.agx_steplog_record(self._s, pi, pr, pf, pp, self.pipe._stream()))

    def gather(self, env: torch.Tensor, index: torch.Tensor, nstep: int = 1, gamma: float = 0.99):
        """The n-step rows of the samples (env[b], index[b]) - i32 [B], i64 [B] - as a dict: ``steps`` i32 [B] (rows folded, 0: none),
        ``next_index`` i64 [B] (index + steps, the observation to bootstrap from; -1 where steps = 0), ``ret`` f32 [B] (the
        discounted reward sum), ``discount`` f32 [B] (gamma ** steps, 0 behind a terminal row), ``flags`` u8 [B] (the last row's) and
        ``payload`` u8 [B, W] (the row of index + 1: the action taken on seeing ``index``).  Where steps = 0, ret, discount,
        flags and payload are 0."""
        nstep = check_nstep(nstep)
        self._live()
        b, pe, pi = self.pipe._pair(env, index)
        w, dev = self.payload_bytes, self.device
        out = {"ret": torch.zeros((b,), dtype=torch.float32, device=dev), "discount": torch.zeros((b,), dtype=torch.float32, device=dev),
               "steps": torch.empty((b,), dtype=torch.int32, device=dev), "next_index": torch.empty((b,), dtype=torch.int64, device=dev),
               "flags": torch.zeros((b,), dtype=torch.uint8, device=dev), "payload": torch.zeros((b, w), dtype=torch.uint8, device=dev)}
        p = {key: _P(t.data_ptr()) for key, t in out.items()}
        self._check(self._lib.agx_steplog_gather(self._s, pe, pi, b, nstep, float(gamma), p["ret"], p["discount"], p["steps"], p["next_index"],
                                                 p["flags"], p["payload"] if w > 0 else None, self.pipe._stream()))
        return out

    def batch(self, sampler, B: int, nstep: int = 1, gamma: float = 0.99, glimpses: Optional[int] = None, memory=None, shift=None):
        """``sampler.sample(B)``, ``gather``, then the observations at ``index`` (obs) and at ``next_index`` (next_obs), as one dict:
        env, index, next_index, ok, obs, next_obs, ret, discount, steps, flags, payload and, on a fixed pipeline, fov_loc and
        next_fov_loc.  ``ok`` is the sampler's ok AND steps > 0.  glimpses = None reads through history.observe; glimpses = P
        through ``memory`` - a GlimpseMemory of P glimpses on this history that the caller owns - or, without one, through
        ``history.memory(P)``, and needs a sampler with back >= P - 1.  shift: an augment.RandomShift on this history - obs and
        next_obs are read through it, two independent draws in that order, and the dict gains obs_shift and next_obs_shift (not
        together with glimpses).  Rows with ok = 0 are left as allocated."""
        nstep = check_nstep(nstep)
        from .augment import check_shift_read
        check_shift_read(shift, glimpses, self.history)
        if sampler.history is not self.history:
            raise ValueError("the sampler draws from another history than the one this log is on")
        if memory is not None and (glimpses is None or memory.history is not self.history or memory.glimpses != int(glimpses)):
            raise ValueError("memory must be a GlimpseMemory of `glimpses` glimpses on this log's history")
        if glimpses is not None and sampler.back < int(glimpses) - 1:
            raise ValueError(f"glimpses = {glimpses} needs a sampler with back >= {int(glimpses) - 1} (so that every memory is full), "
                             f"got back = {sampler.back}")
        env, index, ok = sampler.sample(B)
        out = self.gather(env, index, nstep, gamma)
        if shift is not None:
            read = shift.observe
        elif glimpses is None:
            read = self.history.observe
        else:
            read = (memory if memory is not None else self.history.memory(glimpses)).observe
        obs = self.history.transition_obs(read, env, index, out["next_index"], shift)
        out.update(env=env, index=index, ok=ok & (out["steps"] > 0).to(torch.uint8))
        out.update(obs)
        return out


class EnvStepLog:
    """A vector env's per-step upload into its StepLog: what the step returned on the host - motor action, reward, done -
    travels in one pinned i32 [3, N] buffer; two sets (pinned, device, event), used alternately, each rewritten only after the
    event behind its last copy.  The payload is the motor action as int32, followed on a fixed env by the sensory action as two
    float32."""

    def __init__(self, log: StepLog, fixed: bool, autoreset: bool):
        self.log, self.autoreset = log, bool(autoreset)
        n, dev = log.num_envs, log.device
        self._sets = [(torch.empty((3, n), dtype=torch.int32, pin_memory=True), torch.empty((3, n), dtype=torch.int32, device=dev),
                       torch.cuda.Event()) for _ in range(2)]
        self._i = 0
        self._payload = torch.empty((n, 3), dtype=torch.int32, device=dev) if fixed else None

    def record(self, motor, sens, reward, done):
        """Record what this step returned, after its pushes - one upload of (motor, reward, done), then device work only.  Row =
        the newest index, or the one before it for an env that was autoreset in this step (its terminal observation: the reset
        observation has no step behind it)."""
        log = self.log
        n = log.num_envs
        h, d, ev = self._sets[self._i]
        self._i ^= 1
        ev.synchronize()                        # the copy that last read this pinned buffer, two steps ago
        host = h.numpy()
        host[0] = np.asarray(motor).reshape(n)          # (the cast the runner itself makes)
        host[1] = np.asarray(reward, dtype=np.float32).reshape(n).view(np.int32)
        host[2] = np.asarray(done, dtype=bool).reshape(n)
        d.copy_(h, non_blocking=True)
        ev.record()
        index = log.history.last_index()
        if self.autoreset:
            index -= d[2]
        if sens is None:
            payload = d[0].reshape(n, 1)
        else:
            payload = self._payload
            payload[:, 0] = d[0]
            payload[:, 1:] = sens.to(torch.float32).view(torch.int32)
        log.record(index, d[1].view(torch.float32), d[2].to(torch.uint8), payload.view(torch.uint8))      # TERMINATED == 1
