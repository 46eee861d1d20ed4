"""ctypes view of include/agx_hostout.h: launches over a range of envs (``agx_env_range``) and the chunked host-output step
of the native loop (``agx_loop_step_host``).

With host (NumPy) observations a step is a serial chain - emulators, H2D of the screens, kernels, D2H of the observations -
and PCIe carries one direction at a time.  ``agx_loop_step_host`` cuts the batch into env chunks: chunk c's observations go
home while chunk c + 1's screens arrive and its kernels run.  ``AtariVecEnv`` selects it with ``args.host_obs_chunks = C``.
The entry points live in libagx.so next to include/agx.h and include/agx_loop.h, in a header and a binding of their own."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _native as nat
from . import native_loop as nl

_P = C.c_void_p
MAX_CHUNKS = 64          # AGX_HOSTOUT_MAX_CHUNKS

SIGNATURES = {
    "agx_env_range": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "agx_hostout_partition": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "agx_loop_host_prepare": (C.c_int, [_P, C.c_int]),
    "agx_loop_step_host": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, _P, C.POINTER(nl.AgxLoopResult), _P, _P, _P, _P, C.c_int]),
    "agx_loop_host_wait": (C.c_int, [_P]),
    "agx_loop_host_final": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
}


def lib():
    return nat.bind(nat.lib(), SIGNATURES)


def partition(num_envs: int, chunks: int):
    """The env ranges ``agx_loop_step_host`` cuts a step into: [(lo, n), ...], ascending, covering [0, num_envs) exactly
    (min(chunks, num_envs, MAX_CHUNKS) of them; no alignment of lo is needed, include/agx_hostout.h)."""
    cap = max(1, min(int(chunks), MAX_CHUNKS))
    lo, n = (C.c_int32 * cap)(), (C.c_int32 * cap)()
    c = lib().agx_hostout_partition(int(num_envs), int(chunks), lo, n)
    if c < 0:
        raise nat.AgxError(c, f"agx_hostout_partition({num_envs}, {chunks})")
    return [(int(lo[k]), int(n[k])) for k in range(c)]


class HostOutStep:
    """``NativeStepLoop.step`` with host outputs.  Owns the pinned fov_loc / fov_res destinations; the observation destination
    is the caller's.  Built where the loop is built (bound to the rank's CPUs): ``agx_loop_host_prepare`` pins the loop's side
    buffers there, not inside the first step.  ``steps`` counts the steps that went through ``agx_loop_step_host``."""

    def __init__(self, loop: nl.NativeStepLoop, chunks: int):
        self._lib = lib()
        self.loop = loop
        self.chunks = int(chunks)
        self.steps = 0
        loop.check(self._lib.agx_loop_host_prepare(loop.handle, self.chunks))
        n = loop.n
        self._fov = [torch.zeros((2, n, 2), dtype=torch.int32).pin_memory() for _ in range(2)]
        self._fov_i = 0
        self._views = {}

    def step(self, motor, action: Optional[torch.Tensor], action_dt: int, action_type: Optional[torch.Tensor], obs: torch.Tensor,
             loc: Optional[torch.Tensor], res: Optional[torch.Tensor], h_obs: torch.Tensor):
        """One chunked step into the pinned tensor ``h_obs``; waits for the host copies.  Returns (reward, raw, done, done_idx,
        final_obs [k, ...] | None, final_loc i32 [k, 2] | None, final_res | None, fov_loc i32 [N, 2] | None, fov_res | None) - all
        NumPy; the final_* arrays and fov_* are copies."""
        lp = self.loop
        self._fov_i ^= 1
        hf = self._fov[self._fov_i]
        h_loc = _P(hf[0].data_ptr()) if loc is not None else None
        h_res = _P(hf[1].data_ptr()) if res is not None else None
        reward, raw, done, idx, r = lp.call_step(self._lib.agx_loop_step_host, motor, action, action_dt, action_type, obs, loc, res,
                                                 _P(h_obs.data_ptr()), h_loc, h_res, self.chunks)
        lp.check(self._lib.agx_loop_host_wait(lp.handle))
        self.steps += 1
        n, k = lp.n, len(idx)
        fo = fl = fr = None
        if k and r.d_final_obs:
            po, pl, pr = _P(), _P(), _P()
            lp.check(self._lib.agx_loop_host_final(lp.handle, C.byref(po), C.byref(pl), C.byref(pr)))
            row = int(np.prod(obs.shape[1:]))
            npdt = {torch.float32: np.float32, torch.float16: np.float16}[obs.dtype]
            fo = self._rows(po.value, n * row, npdt)[:k * row].reshape((k,) + tuple(obs.shape[1:])).copy()
            if pl.value:
                fl = self._rows(pl.value, 2 * n, np.int32)[:2 * k].reshape(k, 2).copy()
            if pr.value:
                fr = self._rows(pr.value, 2 * n, np.int32)[:2 * k].reshape(k, 2).copy()
        h_loc_np = hf[0].numpy().copy() if loc is not None else None
        h_res_np = hf[1].numpy().copy() if res is not None else None
        return reward, raw, done, idx, fo, fl, fr, h_loc_np, h_res_np

    def _rows(self, addr, count, dtype):
        """One NumPy view per side buffer (they never move), sliced per step: see NativeStepLoop._host."""
        hit = self._views.get(addr)
        if hit is None:
            buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(addr)
            hit = self._views[addr] = np.frombuffer(buf, dtype=dtype, count=count)
        return hit
