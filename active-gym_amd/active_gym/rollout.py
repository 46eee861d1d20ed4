"""Rollout — ctypes view of include/agx_rollout.h: the last L transitions of EVERY env of a FrameHistory's StepLog, cut at
episode ends, and GAE(lambda) over them, for on-policy learners (PPO, A2C and their family)::

    hist = FrameHistory(pipe, capacity=256)
    log = StepLog(hist, payload_bytes=4)
    roll = Rollout(log)
    ...                                                              # 128 env steps, pushed and recorded
    batch = roll.gather(128)                                         # len [N]; obs_index, next_index, reward, ends, live [128, N]
    env, index = roll.flat(batch)                                    # the live rows, for FrameHistory.observe
    value = torch.zeros(128, N, device=dev)
    value[batch["live"].bool()] = critic(hist.observe(env, index)[0])
    at, benv, bindex = roll.boot_rows(batch)                         # the rows whose V(next observation) is needed
    boot = torch.zeros(128, N, device=dev)
    boot[at[:, 0], at[:, 1]] = critic(hist.observe(benv, bindex)[0])
    adv, ret = roll.gae(batch, value, boot, gamma=0.99, lam=0.95)

Every array is time-major ``[L, N]``; slot ``L - 1`` is an env's newest transition and slot ``t`` is live iff
``t >= L - len[n]``.  A slot is the transition ``(obs_index, next_index)`` of env ``n``: the observation the action was taken on
and the one the step returned - at an episode's end the terminal observation, never the reset observation.  ``ends`` holds
TERMINATED (1), TRUNCATED (2), CUT (4: a reset behind this step that no end flag announced) and BOOT (8: the return bootstraps
from the learner's value of ``next_index``); where a live slot ``t < L - 1`` has none of them, ``next_index[t] ==
obs_index[t + 1]``.  Every other slot is padding with DEFINED contents: indices -1 and zeros - no output needs a memset.
``tests/rollout_model.py`` restates the rule and the float32 fold in NumPy.

The entry points live in libagx.so, in a header and a binding of their own (active_gym/_native.py is unchanged).  A Rollout
owns no native handle."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native as nat

_P = C.c_void_p
ROLLOUT_LIMIT = 4096                  # AGX_ROLLOUT_LIMIT
TERMINATED, TRUNCATED, CUT, BOOT = 1, 2, 4, 8          # AGX_STEP_*, AGX_ROLLOUT_*

SIGNATURES = {
    "agx_rollout_gather": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "agx_rollout_gae": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, C.c_float, C.c_float, _P, _P, _P]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def check_rollout_length(L, num_envs: Optional[int] = None) -> int:
    """ValueError, before any GPU work, for a rollout length outside the header's range."""
    n = int(L)
    if not 1 <= n <= ROLLOUT_LIMIT:
        raise ValueError(f"L must be 1 .. {ROLLOUT_LIMIT}, got {n}")
    if num_envs is not None and n * int(num_envs) > 2 ** 31 - 1:
        raise ValueError(f"L * num_envs = {n * int(num_envs)} exceeds {2 ** 31 - 1}")
    return n


def check_which(which) -> str:
    if which not in ("obs", "next"):
        raise ValueError(f"which must be 'obs' or 'next', got {which!r}")
    return which


class Rollout:
    def __init__(self, steplog):
        """steplog: a StepLog; its history is the one the rollouts are read from."""
        self._lib = lib()
        self.steplog = steplog
        self.history = steplog.history
        self.pipe = steplog.pipe
        self.device = steplog.device
        self.num_envs = steplog.num_envs

    def _live(self):
        self.steplog._live()          # (the history closes its logs first: an open log has an open history)

    def _check(self, rc):
        nat.check(rc, self.pipe._ctx)

    def _fold_args(self, batch: dict, value: torch.Tensor, boot_value: Optional[torch.Tensor]):
        """For gae and vtrace.VTrace.returns: (L, [the checked pointers of len, reward, ends, value, boot_value (None stays None)])."""
        self._live()
        L = check_rollout_length(batch["ends"].shape[0], self.num_envs)
        n, chk = self.num_envs, self.pipe._chk
        return L, [chk(batch["len"], (n,), torch.int32, "len"), chk(batch["reward"], (L, n), torch.float32, "reward"),
                   chk(batch["ends"], (L, n), torch.uint8, "ends"), chk(value, (L, n), torch.float32, "value"),
                   None if boot_value is None else chk(boot_value, (L, n), torch.float32, "boot_value")]

    def gather(self, L: int, out: Optional[dict] = None) -> dict:
        """The last L transitions of every env, as a dict: ``len`` i32 [N], and per slot ([L, N]) ``obs_index`` i64,
        ``next_index`` i64, ``reward`` f32, ``ends`` u8, ``payload`` u8 [L, N, W] (the action taken on seeing ``obs_index``) and
        ``live`` bool (t >= L - len).  ``out``: a dict of an earlier ``gather(L)`` to write into (its ``live`` is rewritten in
        place too), so that a captured graph keeps its addresses."""
        L = check_rollout_length(L, self.num_envs)
        self._live()
        n, w, o = self.num_envs, self.steplog.payload_bytes, self.pipe._out
        out = {} if out is None else out
        ptr = {}
        for key, shape, dtype in (("len", (n,), torch.int32), ("obs_index", (L, n), torch.int64), ("next_index", (L, n), torch.int64),
                                  ("reward", (L, n), torch.float32), ("ends", (L, n), torch.uint8), ("payload", (L, n, w), torch.uint8)):
            out[key], ptr[key] = o(out.get(key), shape, dtype, key)
        self._check(self._lib.agx_rollout_gather(self.steplog._s, L, ptr["len"], ptr["obs_index"], ptr["next_index"], ptr["reward"],
                                                 ptr["ends"], ptr["payload"] if w > 0 else None, self.pipe._stream()))
        live = out["obs_index"] >= 0
        if "live" in out:
            out["live"].copy_(live)
        else:
            out["live"] = live
        return out

    def gae(self, batch: dict, value: torch.Tensor, boot_value: Optional[torch.Tensor], gamma: float = 0.99, lam: float = 0.95,
            adv_out: Optional[torch.Tensor] = None, ret_out: Optional[torch.Tensor] = None):
        """GAE(lambda) over a gathered ``batch`` -> (adv, ret), f32 [L, N].  ``value``: f32 [L, N], the learner's value of
        ``obs_index``; ``boot_value``: f32 [L, N], its value of ``next_index``, used only at the slots ``boot_rows`` names (None
        only for a batch without such a slot).  A slot that is not live gets 0.  The fold is single precision with one rounding
        per operation, in the order of the header."""
        L, args = self._fold_args(batch, value, boot_value)
        adv_out, pa = self.pipe._out(adv_out, (L, self.num_envs), torch.float32, "adv_out")
        ret_out, pt = self.pipe._out(ret_out, (L, self.num_envs), torch.float32, "ret_out")
        self._check(self._lib.agx_rollout_gae(self.history.handle, L, *args, float(gamma), float(lam), pa, pt, self.pipe._stream()))
        return adv_out, ret_out

    def minibatcher(self, seed: int = 0):
        """A minibatch.Minibatcher on this rollout's history: the device-side lists of a batch's LIVE and BOOT slots and their
        seeded shuffles - what ``flat`` and ``boot_rows`` give, without their synchronisation."""
        from .minibatch import Minibatcher
        return Minibatcher(self, seed)

    def chunker(self, seed: int = 0):
        """A chunks.Chunker on this rollout's history: the device-side list of a batch's chunks of consecutive steps and its
        seeded shuffles, for a recurrent learner."""
        from .chunks import Chunker
        return Chunker(self, seed)

    def flat(self, batch: dict, which: str = "obs"):
        """(env i32 [M], index i64 [M]) of the M live slots, in [L, N] order: the samples of ``FrameHistory.observe`` for the
        observations the actions were taken on (``which = "obs"``) or the ones the steps returned (``"next"``).  A minibatch of
        them is an ordinary observe.  ``batch["live"].nonzero()`` gives their (t, n).  Synchronises (the count is data)."""
        key = check_which(which) + "_index"
        at = batch["live"].nonzero()
        return at[:, 1].to(torch.int32), batch[key][at[:, 0], at[:, 1]]

    def boot_rows(self, batch: dict):
        """The slots whose ``next`` value is needed (BOOT) -> (at i64 [M, 2] as (t, n), env i32 [M], index i64 [M]): evaluate the
        critic on ``history.observe(env, index)`` and scatter it into ``boot_value[at[:, 0], at[:, 1]]``.  Synchronises."""
        at = (batch["ends"] & BOOT).nonzero()
        return at, at[:, 1].to(torch.int32), batch["next_index"][at[:, 0], at[:, 1]]
