"""VTrace — ctypes view of include/agx_vtrace.h: V-trace targets and policy-gradient advantages (Espeholt et al. 2018) over a
gathered rollout, for actor-learner training (IMPALA, APPO, PPO with lagging actors) - and BehaviourLog, the place to remember
the behaviour policy's log-probability of every retained step::

    hist = FrameHistory(pipe, capacity=256)
    log = StepLog(hist, payload_bytes=4)
    roll, vt, mu = Rollout(log), VTrace(log), BehaviourLog(hist)
    ...
    mu.write(index, logp_mu[:, None])                                # at every act: index is the observation acted on
    ...                                                              # 128 env steps, pushed and recorded
    batch = roll.gather(128)
    ...                                                              # value, boot as for Rollout.gae; logp of the learner's policy
    rho = torch.exp(logp - mu.read(batch["obs_index"])[..., 0])
    vs, pg_adv = vt.returns(batch, value, boot, rho, gamma=0.99)

Every array is time-major ``[L, N]`` as ``Rollout.gather`` writes it; ``rho`` is the ratio pi / mu of the slot's action, not its
logarithm, so the fold holds no transcendental and is bit-reproducible.  With ``rho == 1`` and levels >= 1, ``vs`` is
``Rollout.gae``'s ``ret`` bit for bit.  ``tests/vtrace_model.py`` restates the float32 fold in NumPy.

The entry point lives in libagx.so, in a header and a binding of its own (active_gym/_native.py is unchanged).  A VTrace is
a Rollout with ``returns`` next to ``gae``; it owns no native handle; a BehaviourLog is one torch tensor and has no native code."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _native as nat
from .rollout import Rollout

_P = C.c_void_p

SIGNATURES = {
    "agx_vtrace_returns": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P, _P]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def check_bars(rho_bar, c_bar, pg_rho_bar):
    """ValueError, before any GPU work, for a truncation level that is not > 0 (NaN, zero, negative); inf means no clipping."""
    out = []
    for name, bar in (("rho_bar", rho_bar), ("c_bar", c_bar), ("pg_rho_bar", pg_rho_bar)):
        bar = float(bar)
        if math.isnan(bar) or not bar > 0.0:
            raise ValueError(f"{name} must be > 0, got {bar}")
        out.append(bar)
    return tuple(out)


class VTrace(Rollout):
    def __init__(self, steplog):
        """steplog: the StepLog whose gathered rollouts are folded; its history supplies N and the device.  The constructor, the
        liveness check and the marshalling of a batch are Rollout's."""
        super().__init__(steplog)
        self._lib = lib()             # (the same library, with this module's SIGNATURES bound too)

    def returns(self, batch: dict, value: torch.Tensor, boot_value: Optional[torch.Tensor], rho: torch.Tensor, gamma: float = 0.99,
                lam: float = 1.0, rho_bar: float = 1.0, c_bar: float = 1.0, pg_rho_bar: float = 1.0,
                vs_out: Optional[torch.Tensor] = None, pg_adv_out: Optional[torch.Tensor] = None):
        """V-trace over a gathered ``batch`` -> (vs, pg_adv), f32 [L, N]: the value targets and the advantages of the policy
        gradient.  ``value``: f32 [L, N], the learner's value of ``obs_index``; ``boot_value``: f32 [L, N], its value of
        ``next_index``, used only at the slots ``Rollout.boot_rows`` names (None reads as 0); ``rho``: f32 [L, N], pi / mu of the
        action taken.  ``rho_bar``, ``c_bar``, ``pg_rho_bar`` truncate the ratio of the temporal difference, of the trace and of
        the policy gradient; each must be > 0 and ``inf`` means no clipping.  A slot that is not live gets 0.  The fold is single
        precision with one rounding per operation, in the order of the header."""
        rho_bar, c_bar, pg_rho_bar = check_bars(rho_bar, c_bar, pg_rho_bar)
        L, args = self._fold_args(batch, value, boot_value)
        n = self.num_envs
        pw = self.pipe._chk(rho, (L, n), torch.float32, "rho")
        vs_out, ps = self.pipe._out(vs_out, (L, n), torch.float32, "vs_out")
        pg_adv_out, pg = self.pipe._out(pg_adv_out, (L, n), torch.float32, "pg_adv_out")
        self._check(self._lib.agx_vtrace_returns(self.history.handle, L, *args, pw, float(gamma), float(lam), rho_bar, c_bar, pg_rho_bar, ps, pg,
                                                 self.pipe._stream()))
        return vs_out, pg_adv_out


class BehaviourLog:
    """What the behaviour policy mu said about every retained step: one f32 tensor ``[T, N, width]`` keyed like the history, row =
    ``index mod T`` (``width = 1``: the log-probability of the action taken; more: its logits).  A retained index is unique mod T,
    so a live slot's ``obs_index`` always reads what was written for it.  Neither method synchronises or uses ``nonzero``: both
    run inside captured graphs."""

    def __init__(self, history, width: int = 1):
        """history: the FrameHistory whose indices key the log (its capacity, num_envs and device are used)."""
        width = int(width)
        if width < 1:
            raise ValueError(f"width must be >= 1, got {width}")
        self.history = history
        self.capacity, self.num_envs, self.width, self.device = int(history.capacity), int(history.num_envs), width, history.device
        self.values = torch.zeros((self.capacity, self.num_envs, width), dtype=torch.float32, device=self.device)
        self._envs = torch.arange(self.num_envs, dtype=torch.int64, device=self.device)

    def _index(self, t, shape, name):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
            raise TypeError(f"{name} must be an int64 torch.Tensor")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        if t.device != self.values.device:
            raise ValueError(f"{name} is on {t.device}, the log is on {self.values.device}")
        return t

    def write(self, index: torch.Tensor, values: torch.Tensor):
        """index: i64 [N], the ``info["history_index"]`` of the observation the policy acted on; values: f32 [N, width].  An env
        whose index is -1 is skipped."""
        self.history._live()
        index = self._index(index, (self.num_envs,), "index")
        if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or tuple(values.shape) != (self.num_envs, self.width):
            raise ValueError(f"values must be float32 of shape {(self.num_envs, self.width)}")
        skip = index < 0
        row = torch.where(skip, torch.zeros_like(index), index) % self.capacity
        kept = self.values[row, self._envs]                           # (one (row, env) per env: the scatter below has no duplicates)
        self.values[row, self._envs] = torch.where(skip[:, None], kept, values.to(self.values.device))

    def read(self, obs_index: torch.Tensor, env: Optional[torch.Tensor] = None) -> torch.Tensor:
        """obs_index: i64 [L, N] (the env of element (t, n) is n), or i64 [B] with ``env`` i32 / i64 [B] -> f32 [L, N, width] or
        [B, width]: what was written for that index; zeros where the index is -1."""
        self.history._live()
        if env is None:
            if not isinstance(obs_index, torch.Tensor) or obs_index.dim() != 2:
                raise ValueError("obs_index must be [L, N], or [B] together with env")
            index = self._index(obs_index, (obs_index.shape[0], self.num_envs), "obs_index")
            env = self._envs[None, :].expand_as(index)
        else:
            if not isinstance(obs_index, torch.Tensor) or obs_index.dim() != 1:
                raise ValueError("obs_index must be [B] where env is given")
            index = self._index(obs_index, None, "obs_index")
            if not isinstance(env, torch.Tensor) or env.dtype not in (torch.int32, torch.int64) or tuple(env.shape) != tuple(index.shape):
                raise ValueError("env must be an int32 / int64 tensor of obs_index's shape")
            env = env.to(torch.int64).clamp(0, self.num_envs - 1)     # (an id that is no env reads some env's row, never out of range)
        skip = index < 0
        row = torch.where(skip, torch.zeros_like(index), index) % self.capacity
        got = self.values[row, env]
        return torch.where(skip[..., None], torch.zeros_like(got), got)
