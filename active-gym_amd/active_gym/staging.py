"""Host-to-device staging of the Python step loop: the pinned screens the host runner writes, their device twins, and the
streams and events that order the copies against the kernels.  :class:`~active_gym.vector.AtariVecEnv` (when the native step
loop does not drive it) and :class:`~active_gym.dmc_env.DMCVecEnv` each own one :class:`Staging`; they differ in the screen
shapes, in where a reset screen lands, and in whether the sets are doubled."""
from __future__ import annotations

import contextlib

import numpy as np
import torch


class Staging:
    """``step_shape`` / ``reset_shape``: the u8 screens of all N envs for a step / for a reset.  ``reset_slot0``: a reset screen
    lands in slot 0 of its env's step screens (Atari: ``reset_shape`` [N, 1, ...], ``step_shape`` [N, 2, ...]) instead of being
    the env's whole buffer (DMC: both [N, H, W, 3]).  ``doubled``: two pinned and two device sets and a copy stream (outputs
    that stay on the device: step() returns without synchronising); otherwise one of each on the current stream.

    Per step: ``begin_step()`` -> the runner writes the array it returns -> ``upload(cmd)`` (or ``upload_rows`` per chunk and
    ``upload_cmd``) -> kernels on ``d_frames`` / ``d_cmd`` -> ``reset_envs`` for the envs that ended (kernels on ``d_rcmd``)
    -> ``release()``."""

    def __init__(self, num_envs: int, step_shape, reset_shape, reset_slot0: bool, doubled: bool, device):
        n = self.num_envs = int(num_envs)
        self.device = device
        self._slot0 = bool(reset_slot0)
        self.doubled = bool(doubled)
        # Two pinned staging sets (screens, command bytes, copy-done event), used alternately: with device outputs step()
        # returns without synchronising, so the emulators of step t+1 fill one set while the H2D copy of step t still
        # drains the other (host-side double buffering; on the device the copies are stream-ordered behind the kernels
        # that read the previous screens, so one device buffer is enough)
        nsets = 2 if self.doubled else 1
        self._stages = [{"frames": torch.empty(step_shape, dtype=torch.uint8, pin_memory=True),
                         "cmd": torch.empty((n,), dtype=torch.uint8, pin_memory=True),
                         "ev": torch.cuda.Event()} for _ in range(nsets)]
        # Device side.  With device outputs (no synchronisation inside step()) the step screens are double-buffered on the
        # device too and travel on a COPY STREAM of their own: the H2D copy of step t+1 then runs under the kernels (and the
        # autoreset pass) of step t instead of queueing behind them on the one stream - on a PCIe-bound step that is the
        # difference between 87 % and ~95 % of the link.  Two events per buffer order the streams: `copied` (copy stream ->
        # the kernels wait for their screens) and `free` (launch stream -> the copy that overwrites a buffer waits for the
        # kernels that read it two steps earlier).  NumPy outputs synchronise every step anyway: one buffer, one stream.
        self._dsets = [{"frames": torch.empty(step_shape, dtype=torch.uint8, device=device),
                        "cmd": torch.empty((n,), dtype=torch.uint8, device=device),
                        "free": torch.cuda.Event()} for _ in range(nsets)]
        self._copy_stream = torch.cuda.Stream(device=device) if self.doubled else None
        self._set_i = 0                         # the pinned set and the device set of this step (they turn together)
        # reset screens get their own pinned buffer: the autoreset inside step() must not overwrite step
        # screens whose asynchronous H2D copy may still be in flight
        self._h_rframes = torch.empty(reset_shape, dtype=torch.uint8, pin_memory=True)
        self._h_rcmd = torch.empty((n,), dtype=torch.uint8, pin_memory=True)
        # Staging for resets of a SUBSET of the envs (the autoreset inside step(), reset_envs()).  The runner writes the K reset
        # screens PACKED into the first K rows of a pinned buffer: one contiguous H2D copy into _d_rframes, one index_copy_ into
        # slot 0 of the step screens.  Env indices, command bytes and the done mask travel together in one small pinned buffer
        # (one copy; a pageable .to(device) would be a synchronous one).  TWO pinned sets, used alternately: the set a reset
        # writes was last read by the copies of the reset before the previous one - waiting on the previous reset's event
        # instead would wait for that whole step's H2D copy and kernels, i.e. serialise the host with the GPU.
        self._rsets = [{"frames": self._h_rframes if k == 0 else torch.empty_like(self._h_rframes).pin_memory(),
                        "meta": torch.empty((10 * n,), dtype=torch.uint8, pin_memory=True),        # idx i64 [N] | cmd [N] | mask [N]
                        "ev": torch.cuda.Event()} for k in range(2)]
        self._rset_i = 0
        self._rfree = torch.cuda.Event()        # launch stream: the kernels of the last partial reset have read the device-side staging
        self._d_rframes = None                  # allocated at the first partial reset
        self._d_rmeta = torch.empty((10 * n,), dtype=torch.uint8, device=device)
        self._d_ridx = self._d_rmeta[:8 * n].view(torch.int64)
        self.d_rcmd = self._d_rmeta[8 * n:9 * n]                # the command bytes of the last reset_envs()
        self._d_rmask = self._d_rmeta[9 * n:]

    _stage = property(lambda self: self._stages[self._set_i])
    _dset = property(lambda self: self._dsets[self._set_i])
    h_frames = property(lambda self: self._stage["frames"], doc="the pinned step screens the runner writes (this step's set)")
    d_frames = property(lambda self: self._dset["frames"], doc="the device step screens to ingest (this step's set)")
    d_cmd = property(lambda self: self._dset["cmd"], doc="their command bytes")

    def _reset_rows(self, frames):
        """One reset screen per env: of a pinned reset buffer, or (the device step screens) where they land."""
        return frames[:, 0] if self._slot0 else frames

    @contextlib.contextmanager
    def _copies(self, after, done):
        """The H2D copies enqueued inside, then ``done``: on the copy stream when there is one - behind ``after`` (the launch
        stream's last reader of their destination), and the launch stream waits for ``done`` - on the current stream otherwise."""
        cur = torch.cuda.current_stream(self.device)
        cs = self._copy_stream
        if cs is not None:
            cs.wait_event(after)
        with torch.cuda.stream(cs):             # (None: the current stream stays)
            yield
            done.record(cs or cur)
        if cs is not None:
            cur.wait_event(done)

    def begin_step(self) -> np.ndarray:
        """Turn to the other pinned set - waiting only for the copy issued from it two steps ago - and the other device screen
        buffer.  Returns the host screens the runner writes in this step."""
        if self.doubled:
            self._set_i ^= 1
        self._stage["ev"].synchronize()         # this set's previous screens have left the pinned buffer
        return self.h_frames.numpy()

    def upload(self, cmd: np.ndarray):
        """Asynchronous H2D of the step screens and the command bytes (pinned -> HBM): on the copy stream when there is one
        (device outputs), ordered against the launch stream by events; on the current stream otherwise."""
        st, ds = self._stage, self._dset
        st["cmd"].numpy()[:] = cmd
        with self._copies(after=ds["free"], done=st["ev"]):    # after: the kernels that read this device buffer two steps ago
            ds["cmd"].copy_(st["cmd"], non_blocking=True)
            ds["frames"].copy_(st["frames"], non_blocking=True)

    def upload_rows(self, lo: int, hi: int):
        """Chunked H2D (args.h2d_chunk_envs): the step screens of envs [lo, hi), on the current stream."""
        self.d_frames[lo:hi].copy_(self.h_frames[lo:hi], non_blocking=True)

    def upload_cmd(self, cmd: np.ndarray):
        """... and, after the last chunk, the command bytes."""
        st = self._stage
        st["cmd"].numpy()[:] = cmd
        self.d_cmd.copy_(st["cmd"], non_blocking=True)
        st["ev"].record(torch.cuda.current_stream(self.device))

    def release(self):
        """Call when the last kernel that reads the current device screens has been enqueued."""
        if self._copy_stream is not None:
            cur = torch.cuda.current_stream(self.device)
            self._dset["free"].record(cur)
            self._rfree.record(cur)

    def drain(self):
        """Wait until no copy out of a pinned buffer is in flight."""
        for st in self._stages + self._rsets:
            st["ev"].synchronize()

    def reset_all(self, runner_reset):
        """``runner_reset(out=)`` of every env + H2D of the reset screens (slot 0 only: one strided copy) and the command bytes,
        which land in ``d_cmd``."""
        self.drain()
        self._h_rcmd.numpy()[:] = runner_reset(out=self._h_rframes.numpy())
        self.d_cmd.copy_(self._h_rcmd, non_blocking=True)
        self._reset_rows(self.d_frames).copy_(self._reset_rows(self._h_rframes), non_blocking=True)
        self._rsets[0]["ev"].record(torch.cuda.current_stream(self.device))

    def reset_envs(self, idx, runner_reset):
        """``runner_reset(idx, out=, packed=True)`` of the envs in `idx` + H2D of their screens, command bytes, indices and mask.
        Returns (done mask, env indices) as device tensors; the command bytes of this pass are in ``d_rcmd``."""
        idx = np.asarray(idx, dtype=np.int64)
        k, n = len(idx), self.num_envs
        self._rset_i ^= 1
        st = self._rsets[self._rset_i]
        st["ev"].synchronize()                  # the reset before the previous one has left this pinned set
        cmd = runner_reset(idx, out=st["frames"].numpy(), packed=True)
        meta = st["meta"].numpy()
        meta[:8 * n].view(np.int64)[:k] = idx
        meta[8 * n:9 * n] = cmd
        m = meta[9 * n:]
        m[:] = 0
        m[idx] = 1
        rows = self._reset_rows(st["frames"])
        if self._d_rframes is None:
            self._d_rframes = torch.empty(rows.shape, dtype=torch.uint8, device=self.device)
        # on the COPY stream (when there is one), i.e. queued between this step's screens and the next step's: a small copy issued
        # on the launch stream would reach the DMA engine behind the next step's 200 MB copy and stall this step's reset kernels
        # (and everything ordered after them) for a whole copy time - measured: 5.1 ms per RGB step instead of 4.1
        with self._copies(after=self._rfree, done=st["ev"]):    # after: the previous reset's index_copy_ has read _d_rframes / _d_rmeta
            self._d_rmeta.copy_(st["meta"], non_blocking=True)
            self._d_rframes[:k].copy_(rows[:k], non_blocking=True)
        self._reset_rows(self.d_frames).index_copy_(0, self._d_ridx[:k], self._d_rframes[:k])
        return self._d_rmask, self._d_ridx[:k]
