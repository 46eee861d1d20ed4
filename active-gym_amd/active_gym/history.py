"""FrameHistory — ctypes view of include/agx_history.h: an on-device history of the u8 frames and fov_loc behind every
observation, and the kernel that re-creates the observation of any retained env-step.

An observation is ``[fs][h][w]`` elements (113 KB per env-step at float32 84 x 84 x 4): too large to keep.  It is a pure
function of the env's last ``fs`` u8 frames (7 KB each, one new one per env-step) and its fov_loc (8 bytes); the history
keeps those, ``capacity`` env-steps per env, in HBM::

    hist = FrameHistory(pipe, capacity=100_000)           # hist.nbytes: about capacity * N * (obs_h * obs_w + 9) bytes
    pipe.ingest(frames, cmd); obs, loc = pipe.fovea(action)
    index = hist.push(cmd)                                  # i64 [N]: store (env, index) in the replay buffer, not obs
    ...
    obs, loc, valid = hist.observe(env, index)              # bit for bit what the step returned, where still retained
    obs, loc, valid = hist.observe(env, index, action=a)    # ... had the env looked at `a` (absolute) instead

The entry points live in libagx.so, in a header and a binding of their own (active_gym/_native.py is unchanged)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native as nat
from .lifetime import Owner

_P = C.c_void_p
HIST_FOVEA, HIST_FULL = 0, 1          # AGX_HIST_*
_WHAT = {"fovea": HIST_FOVEA, "full": HIST_FULL}

SIGNATURES = {
    "agx_history_create": (C.c_int, [_P, C.c_int32, C.POINTER(_P)]),
    "agx_history_destroy": (C.c_int, [_P]),
    "agx_history_clear": (C.c_int, [_P, _P]),
    "agx_history_bytes": (C.c_int64, [_P]),
    "agx_history_push": (C.c_int, [_P, _P, _P, _P]),
    "agx_history_last_index": (C.c_int, [_P, _P, _P]),
    "agx_history_observe": (C.c_int, [_P, C.c_int, _P, _P, C.c_int32, _P, C.c_int, _P, _P, _P, _P]),
    "agx_loop_set_history": (C.c_int, [_P, _P]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def check_env_history(kind: str, history_len, channels: int = 1, ragged_obs: str = "padded") -> int:
    """``args.history_len`` of a vector env -> T (0: no history); ValueError, before any GPU work, for what the history does
    not serve: kinds other than base / fixed, colour frames, packed ragged observations."""
    t = int(history_len or 0)
    if t < 0:
        raise ValueError(f"history_len must be >= 0, got {t}")
    if t > 0:
        if kind not in ("base", "fixed"):
            raise ValueError(f"history_len > 0 needs kind 'base' or 'fixed', got {kind!r} (peripheral / flexible re-observation is not built)")
        if int(channels) != 1:
            raise ValueError("history_len > 0 needs gray frames (colour re-observation is not built)")
        if ragged_obs == "packed":
            raise ValueError("history_len > 0 with ragged_obs='packed': packed ragged crops are not re-observed")
    return t


class FrameHistory(Owner):
    def __init__(self, pipe, capacity: int):
        """pipe: an ObsPipeline of kind "base" or "fixed" with gray frames; capacity: env-steps kept per env (>= frame_stack).
        Create it before the pipeline's first ingest (a new history takes the frames before an env's first append to be zero,
        which is what a new pipeline's stack holds), or start every env with a CMD_CLEAR ingest as a reset does."""
        self._lib = lib()
        self.pipe = pipe
        self.device = pipe.device
        self.capacity = int(capacity)
        self.num_envs = pipe.num_envs
        self._h = _P()
        nat.check(self._lib.agx_history_create(pipe._ctx, self.capacity, C.byref(self._h)), pipe._ctx)
        # the history holds the context's raw handle: it goes before the pipeline does; the samplers, step logs and shift sources on it
        # are its children and go before it
        self._own(self._h, self._lib.agx_history_destroy, (pipe,))
        self._memories, self._samplers, self._shifts = {}, {}, {}

    @property
    def handle(self):
        """The agx_history* (for agx_loop_set_history)."""
        return self._h

    @property
    def nbytes(self) -> int:
        return int(self._lib.agx_history_bytes(self._h))

    def _chk(self, t, shape, dtype, name):
        return self.pipe._chk(t, shape, dtype, name)

    def _check(self, rc):
        nat.check(rc, self.pipe._ctx)

    def clear(self):
        """Every index becomes invalid, the per-env indices restart at 0.  The step logs on this history are cleared with it (a
        row recorded before the clear must not pass for one of a new index), and so are the prioritized samplers' tables."""
        self._check(self._lib.agx_history_clear(self._h, self.pipe._stream()))
        from .priority import PrioritizedSampler
        from .steplog import StepLog
        for child in self._children:
            if isinstance(child, (StepLog, PrioritizedSampler)):          # (a uniform sampler keeps no rows)
                child.clear()

    def push(self, cmd: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """After one ingest(.., cmd) and its observation: append each env's newest frame and current fov_loc.  Returns the i64 [N]
        index of the append (-1 for an env whose command byte carries CMD_SKIP).  One push per ingest."""
        pc = self._chk(cmd, (self.num_envs,), torch.uint8, "cmd")
        out, po = self.pipe._out(out, (self.num_envs,), torch.int64, "out")
        self._check(self._lib.agx_history_push(self._h, pc, po, self.pipe._stream()))
        return out

    def last_index(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """i64 [N]: the index of each env's newest append (-1: none yet)."""
        out, po = self.pipe._out(out, (self.num_envs,), torch.int64, "out")
        self._check(self._lib.agx_history_last_index(self._h, po, self.pipe._stream()))
        return out

    def obs_row_shape(self, what: str = "fovea"):
        """Shape of one re-created observation: the pipeline's own row, or (fs, obs_h, obs_w) for what="full"."""
        return tuple(self.pipe.full_shape[1:] if what == "full" else self.pipe.obs_shape[1:])

    def observe(self, env: torch.Tensor, index: torch.Tensor, action: Optional[torch.Tensor] = None, what: str = "fovea",
                out: Optional[torch.Tensor] = None, loc_out: Optional[torch.Tensor] = None, valid_out: Optional[torch.Tensor] = None):
        """Re-create the observations of the samples (env[b], index[b]) - i32 [B], i64 [B]; any order, repeats allowed.
        action: None (the recorded fov_loc: bit for bit the step's observation) or [B, 2] f32 / f64 / i32 / i64, an ABSOLUTE
        sensory action to look at instead.  what: "fovea" (the pipeline's own observation) or "full" (the stack, k/255).
        Returns (obs [B, ...], fov_loc i32 [B, 2], valid u8 [B]); rows of invalid samples (never issued, or evicted) are left as
        they were in `out` / `loc_out` (uninitialised when this call allocated them).  fov_loc is not written by a base pipeline."""
        if what not in _WHAT:
            raise ValueError(f"what must be 'fovea' or 'full', got {what!r}")
        pipe = self.pipe
        b, pe, pi = pipe._pair(env, index)
        pa, dt = pipe._action(action, b)
        out, po = pipe._out(out, (b,) + self.obs_row_shape(what), pipe.obs_dtype, "out")
        loc_out, pl = pipe._out(loc_out, (b, 2), torch.int32, "loc_out")
        valid_out, pv = pipe._out(valid_out, (b,), torch.uint8, "valid_out")
        self._check(self._lib.agx_history_observe(self._h, _WHAT[what], pe, pi, b, pa, dt, po, pl, pv, self.pipe._stream()))
        return out, loc_out, valid_out

    def attach(self, loop):
        """The native step loop pushes from now on (agx_loop_set_history); ``loop``: a NativeStepLoop of the same pipeline."""
        loop.check(self._lib.agx_loop_set_history(loop.handle, self._h))
        # the loop pushes through the raw handle: a history that closes under a live loop takes itself out of it first
        self._while_both_alive(loop, lambda: self._lib.agx_loop_set_history(loop.handle, None))

    def memory(self, glimpses: int):
        """The one glimpse.GlimpseMemory of ``glimpses`` glimpses on this history, made at first use (ValueError for a kind or
        mode that is not served): what ReplaySampler.transitions, StepLog.batch and the env's glimpse_memory read through."""
        mem = self._memories.get(int(glimpses))
        if mem is None:
            from .glimpse import GlimpseMemory
            mem = self._memories[int(glimpses)] = GlimpseMemory(self, glimpses)
        return mem

    def sampler(self, back: int = 0, forward: int = 1, attempts: int = 16, seed: int = 0):
        """The one replay.ReplaySampler of this argument tuple on this history, made at first use."""
        key = (int(back), int(forward), int(attempts), int(seed))
        smp = self._samplers.get(key)
        if smp is None:
            from .replay import ReplaySampler
            smp = self._samplers[key] = ReplaySampler(self, back, forward, attempts, seed)
        return smp

    def prioritized(self, back: int = 0, forward: int = 1, seed: int = 0):
        """The one priority.PrioritizedSampler of this argument tuple on this history, made at first use."""
        key = ("prioritized", int(back), int(forward), int(seed))
        smp = self._samplers.get(key)
        if smp is None:
            from .priority import PrioritizedSampler
            smp = self._samplers[key] = PrioritizedSampler(self, back, forward, seed)
        return smp

    def shift(self, pad: int = 4, seed: int = 0):
        """The one augment.RandomShift of this argument tuple on this history, made at first use."""
        key = (int(pad), int(seed))
        aug = self._shifts.get(key)
        if aug is None:
            from .augment import RandomShift
            aug = self._shifts[key] = RandomShift(self, pad, seed)
        return aug

    def behaviour(self, width: int = 1):
        """The one vtrace.BehaviourLog of this width on this history, made at first use."""
        key = ("behaviour", int(width))
        log = self._samplers.get(key)
        if log is None:
            from .vtrace import BehaviourLog
            log = self._samplers[key] = BehaviourLog(self, width)
        return log

    def minibatcher(self, rollout, seed: int = 0):
        """The one minibatch.Minibatcher of this seed on this history, made at first use (``rollout``: the Rollout it is made on)."""
        key = ("minibatch", int(seed))
        mb = self._samplers.get(key)
        if mb is None:
            mb = self._samplers[key] = rollout.minibatcher(seed)
        return mb

    def chunker(self, rollout, seed: int = 0):
        """The one chunks.Chunker of this seed on this history, made at first use (``rollout``: the Rollout it is made on)."""
        key = ("chunks", int(seed))
        ch = self._samplers.get(key)
        if ch is None:
            ch = self._samplers[key] = rollout.chunker(seed)
        return ch

    def transition_obs(self, read, env, index, next_index, shift=None) -> dict:
        """The observation part of a transition batch through ``read`` (``self.observe`` or a GlimpseMemory's): obs, next_obs
        and, on a fixed pipeline, fov_loc, next_fov_loc.  ``shift``: the augment.RandomShift whose ``observe`` ``read`` is - two
        independent draws, obs first; the shifts of each are added as obs_shift and next_obs_shift (i32 [B, 2])."""
        obs, loc, _ = read(env, index)
        out = {"obs": obs}
        if shift is not None:
            out["obs_shift"] = shift.last_shift
        nobs, nloc, _ = read(env, next_index)
        out["next_obs"] = nobs
        if shift is not None:
            out["next_obs_shift"] = shift.last_shift
        if self.pipe.kind == "fixed":
            out["fov_loc"], out["next_fov_loc"] = loc, nloc
        return out
