"""Retrace — ctypes view of include/agx_retrace.h: the Retrace-family Q-return (Retrace of Reactor / ACER / MPO / Agent57, Peng's
Q(lambda), Tree-backup) folded backward along the sequences of a sequence-replay batch, cut where the sequence is cut::

    seq, rt = SequenceReplay(log), Retrace(log)
    batch = seq.batch(sampler, 64, 80, nstep=1)                   # nstep = 1: ret is the step's reward, steps says which rows exist
    q_all, pi = learner(batch["obs"])                              # [64, 80, A] each
    a = batch["payload"].view(torch.int32)[..., 0].long()
    q = q_all.gather(-1, a[..., None])[..., 0]                     # Q of the action taken
    v = (pi * q_all).sum(-1)                                       # the expected value under the target policy
    c = coefficients(pi.log().gather(-1, a[..., None])[..., 0], logp_mu, lam=0.95)
    out = rt.targets(batch, q, v, c, boot)                         # target, td, valid: [64, 80]

The arrays are ``SequenceReplay.gather``'s, ``[B, L]`` or ``[L, B]`` with ``time_major``; ``boot`` ([B]) is the expected value at
the observation behind the last step.  A step is valid iff it is live and its row was recorded (``steps == 1``); the return of a
valid step bootstraps from ``v`` of the next step, or ``boot`` behind the sequence, and carries the corrected error of the next
step only where that step is valid too.  Every other step is 0 in all three outputs.  The fold is single precision with one
rounding per operation: ``tests/retrace_model.py`` restates it in NumPy.

The entry point lives in libagx.so, in a header and a binding of its own (active_gym/_native.py is unchanged).  A Retrace owns no
native handle."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native as nat
from .sequence import check_length

_P = C.c_void_p
KINDS = ("retrace", "qlambda", "tree")

SIGNATURES = {
    "agx_sequence_retrace": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def check_kind(kind) -> str:
    """ValueError, before any GPU work, for a trace family that is not one of KINDS."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {', '.join(repr(k) for k in KINDS)}, got {kind!r}")
    return kind


def check_lambda(lam) -> float:
    """ValueError for a lambda outside 0 .. 1 (NaN included)."""
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lam must be 0 .. 1, got {lam}")
    return lam


def coefficients(logp_pi: torch.Tensor, logp_mu: Optional[torch.Tensor] = None, lam: float = 1.0, kind: str = "retrace") -> torch.Tensor:
    """The trace coefficient of every step's action, f32, in ``logp_pi``'s shape.  ``logp_pi``: the log-probability of the action
    taken under the target policy; ``logp_mu``: under the behaviour policy (what ``BehaviourLog`` kept).
    ``"retrace"``: lam * min(1, pi / mu); ``"qlambda"``: lam; ``"tree"``: lam * pi.  Plain torch."""
    kind, lam = check_kind(kind), check_lambda(lam)
    if not isinstance(logp_pi, torch.Tensor) or not logp_pi.is_floating_point():
        raise ValueError("logp_pi must be a floating-point torch.Tensor")
    logp_pi = logp_pi.to(torch.float32)
    if kind == "qlambda":
        return torch.full_like(logp_pi, lam)
    if kind == "tree":
        return lam * torch.exp(logp_pi)
    if not isinstance(logp_mu, torch.Tensor) or not logp_mu.is_floating_point() or tuple(logp_mu.shape) != tuple(logp_pi.shape):
        raise ValueError("kind 'retrace' needs logp_mu, a floating-point torch.Tensor of logp_pi's shape")
    return lam * torch.exp(logp_pi - logp_mu.to(torch.float32)).clamp(max=1.0)


def check_batch(batch, time_major: bool = False):
    """The entries of a ``SequenceReplay.gather`` / ``batch`` dict the fold reads -> (B, L); ValueError, before any GPU work, for a
    missing entry, a wrong dtype or shapes that do not fit each other."""
    for key in ("length", "steps", "ret", "discount"):
        if not isinstance(batch, dict) or not isinstance(batch.get(key), torch.Tensor):
            raise ValueError(f"batch must be the dict of SequenceReplay.gather / batch: no tensor {key!r}")
    length, steps = batch["length"], batch["steps"]
    if length.dim() != 1 or length.dtype != torch.int32:
        raise ValueError("batch['length'] must be int32 [B]")
    if steps.dim() != 2 or steps.dtype != torch.int32:
        raise ValueError("batch['steps'] must be int32 [B, L] ([L, B] with time_major)")
    B = int(length.shape[0])
    L = int(steps.shape[0] if time_major else steps.shape[1])
    if tuple(steps.shape) != ((L, B) if time_major else (B, L)):
        raise ValueError(f"batch['steps'] has shape {tuple(steps.shape)}, which is not {'[L, B]' if time_major else '[B, L]'} for B = {B}: "
                         f"pass the time_major the batch was gathered with")
    check_length(L)
    for key in ("ret", "discount"):
        if batch[key].dtype != torch.float32 or tuple(batch[key].shape) != tuple(steps.shape):
            raise ValueError(f"batch[{key!r}] must be float32 of shape {tuple(steps.shape)}")
    return B, L


def check_outputs(out, shape):
    """``out=`` of ``targets``: None, or an earlier result - a dict with target, td and valid of the right shape."""
    if out is None:
        return None
    if not isinstance(out, dict) or sorted(out) != ["target", "td", "valid"]:
        raise ValueError("out must be a dict returned by an earlier targets(): target, td, valid")
    for key, dt in (("target", torch.float32), ("td", torch.float32), ("valid", torch.uint8)):
        t = out[key]
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != tuple(shape):
            raise ValueError(f"out[{key!r}] must be {dt} of shape {tuple(shape)}")
    return out


class Retrace:
    def __init__(self, source):
        """source: a SequenceReplay or the StepLog it reads; its history supplies the device and the error channel."""
        self._lib = lib()
        self.steplog = getattr(source, "steplog", source)
        self.history = self.steplog.history
        self.pipe = self.steplog.pipe
        self.device = self.steplog.device

    def _live(self):
        self.steplog._live()          # (the history closes its logs first: an open log has an open history)

    def targets(self, batch: dict, q: torch.Tensor, v: torch.Tensor, c: torch.Tensor, boot: Optional[torch.Tensor] = None,
                out: Optional[dict] = None, time_major: bool = False) -> dict:
        """The Q-return of every step of a gathered ``batch`` (``nstep = 1``) -> dict of ``target`` f32, ``td`` f32 (target - q)
        and ``valid`` u8, each [B, L] ([L, B] with ``time_major``, which must be the batch's).  ``q``: f32, the learner's Q of the
        action taken; ``v``: f32, its expected value under the target policy at the step's observation; ``c``: f32, the trace
        coefficient (``coefficients``); ``boot``: f32 [B], the expected value at ``next_index[:, -1]`` (None reads as 0).
        ``out``: the dict of an earlier call, written in place - a captured graph keeps its addresses.  A step that is not valid is
        0 in all three."""
        B, L = check_batch(batch, time_major)
        shape = tuple(batch["steps"].shape)
        for name, t in (("q", q), ("v", v), ("c", c)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape:
                raise ValueError(f"{name} must be float32 of shape {shape}")
        if boot is not None and (not isinstance(boot, torch.Tensor) or boot.dtype != torch.float32 or tuple(boot.shape) != (B,)):
            raise ValueError(f"boot must be float32 of shape {(B,)}, or None")
        out = check_outputs(out, shape)
        self._live()
        pipe = self.pipe
        ins = [pipe._chk(batch["length"], (B,), torch.int32, "batch['length']"), pipe._chk(batch["steps"], shape, torch.int32, "batch['steps']"),
               pipe._chk(batch["ret"], shape, torch.float32, "batch['ret']"), pipe._chk(batch["discount"], shape, torch.float32, "batch['discount']"),
               pipe._chk(q, shape, torch.float32, "q"), pipe._chk(v, shape, torch.float32, "v"), pipe._chk(c, shape, torch.float32, "c"),
               None if boot is None else pipe._chk(boot, (B,), torch.float32, "boot")]
        out = {} if out is None else out
        outs = []
        for key, dt in (("target", torch.float32), ("td", torch.float32), ("valid", torch.uint8)):
            out[key], ptr = pipe._out(out.get(key), shape, dt, f"out[{key!r}]")
            outs.append(ptr)
        nat.check(self._lib.agx_sequence_retrace(self.history.handle, B, L, int(bool(time_major)), *ins, *outs, pipe._stream()), pipe._ctx)
        return out
