"""Batched active-vision Atari envs on one MI355X.

The reference has no vectorization of its own; callers loop N Python envs
through ``gymnasium.vector.SyncVectorEnv`` (reference atari_env.py:241,276).
:class:`AtariVecEnv` replaces that loop: N emulators on host cores
(:class:`~active_gym.runner.AtariHostRunner`), raw screens staged through a
pinned buffer and copied asynchronously to HBM, and the whole observation
pipeline as HIP kernels (:class:`~active_gym.pipeline.ObsPipeline`).

It keeps the SyncVectorEnv conventions of gymnasium<1.0 (setup.py:15 of the
reference pins ``gymnasium>=0.28.1,<1.0.0``):
  * ``step({"motor_action": (N,), "sensory_action": (N,2)[, "sensory_action_type": (N,)|(N,1)]})``
    -> ``obs (N,fs,h,w) f32, reward (N,), terminated (N,), truncated (N,), infos``
  * infos is a dict of arrays with ``_key`` masks; done envs are reset inside
    the same call and their last observation / info are returned under
    ``final_observation`` / ``final_info``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native as nat
from .hostobs import HostObs, _HostObsPool  # noqa: F401  (the pool's tests reach it as vector._HostObsPool)
from .infos import attach_final, fov_entries, terminal_rows, with_masks
from .pipeline import ObsPipeline, resolve_obs_dtype
from .runner import AtariHostRunner
from .spaces import Box, Dict, Discrete, batch_space
from .staging import Staging

_KINDS = ("base", "fixed", "flexible", "peripheral")
_COUNTERS = ("raw_reward", "reward", "ep_len")          # the RecordWrapper entries of an info


def _resolve_antialias(args):
    """torchvision's Resize default: antialias=True from 0.17 on (the reference leaves the version
    unpinned, setup.py:17).  ``args.antialias`` overrides."""
    return bool(getattr(args, "antialias", True))


def wants_packed(args):
    """``args.ragged_obs = "packed"``: the request for the ragged crops themselves (served for flexible raw crops)."""
    return getattr(args, "ragged_obs", "padded") == "packed"


def _resolve_env_obs_dtype(args):
    """``args.obs_dtype`` ("float32" by default, "bfloat16", "float16" or the torch dtype) -> the torch dtype, with the
    combinations the 16-bit outputs do not serve refused up front (before any GPU work)."""
    dt = resolve_obs_dtype(getattr(args, "obs_dtype", "float32"))
    if dt is not torch.float32:
        if dt is torch.bfloat16 and getattr(args, "device", None) is None:
            raise ValueError("obs_dtype bfloat16 needs device outputs (args.device): NumPy has no bfloat16 "
                             "(host outputs take float32 or float16)")
        if wants_packed(args):
            raise ValueError(f"obs_dtype {dt} with ragged_obs='packed': the packed ragged crops are float32 only")
        if bool(getattr(args, "record", False)):
            raise ValueError(f"obs_dtype {dt} with record=True: the record buffers keep the reference's float32 format")
    return dt


def obs_space_dtype(obs_dtype):
    """NumPy dtype of the observation Box: float16 for float16 outputs; float32 otherwise - bfloat16 has no NumPy dtype, its
    Box says float32 (the values it holds are float32 values) and ``env.obs_dtype`` names the element type."""
    return np.float16 if obs_dtype is torch.float16 else np.float32


class AtariVecEnv:
    """N envs of one kind.  ``args`` is an ``AtariEnvArgs``; extra optional attributes:
    ``frame_source`` ("ale" | "synthetic" | factory), ``device`` (None -> NumPy outputs on the host like
    the reference; a cuda device -> torch tensors that stay in HBM), ``antialias``, ``num_workers``,
    ``host_obs_chunks`` (C > 0 with ``device=None`` and a native frame source: step() runs in the native loop and
    brings the observations home in C env chunks, each chunk's device-to-host copy under the next chunk's
    host-to-device copy and kernels; ``env.host_obs_chunks`` is the value in effect, 0 = the unchunked path),
    ``history_len`` (T > 0, kinds base / fixed: the env owns a :class:`~active_gym.history.FrameHistory` of T env-steps per
    env as ``env.history``, pushes after every observation it returns - in the Python loop and in the native loop - and
    ``info["history_index"]`` is the index of the observation ``step`` / ``reset`` returned; for an env that was autoreset in
    this step the terminal observation is ``index - 1``.  0, the default: no history, no key),
    ``step_log`` (True, needs ``history_len`` > 0: the env owns a :class:`~active_gym.steplog.StepLog` on its history as
    ``env.steplog`` and records after every ``step`` - in the Python loop and in the native loop - the step's returned reward,
    flags = TERMINATED for ``done`` and the action as payload, at the index of the observation the step produced (the
    terminal observation's for an env autoreset in this step).  The payload is the motor action as int32 (4 bytes, base env)
    followed on a fixed env by the sensory action as two float32 (12 bytes): exact for integer-valued and float32 sensory
    actions, a float64 one is rounded to float32.  It needs a discrete motor action (one integer per env): ``DMCVecEnv``, whose
    motor actions are float vectors, refuses ``step_log`` in its constructor's first lines.  ``reset`` / ``reset_envs`` record
    nothing.  ``env.replay_batch`` draws
    learner batches from it.  False, the default: nothing new runs in ``step``)."""

    _loop = None             # NativeStepLoop when the native step loop drives this env (subclasses with their own source: never)
    _staging = None          # staging.Staging when the Python loop does
    _host_pool = property(lambda self: self._host.pool if self._host is not None else None)      # hostobs._HostObsPool | None
    _want_loop = False
    host_obs_chunks = 0      # chunks of the host-output step in effect (args.host_obs_chunks where its conditions hold, else 0)
    _host_step = None        # native_hostout.HostOutStep when host_obs_chunks > 0
    history = None           # history.FrameHistory when args.history_len > 0
    history_len = 0
    steplog = None           # steplog.StepLog when args.step_log
    step_log = False
    _env_log = None          # steplog.EnvStepLog when args.step_log: the per-step upload into it
    _per = None              # priority.PrioritizedSampler the last prioritized replay_batch drew from
    _discrete_motor = True   # the motor action is one integer per env (what the step log's payload holds)

    def __init__(self, args, num_envs: int, kind: str = "fixed", env_offset: int = 0, noop_fn=None,
                 autoreset: bool = True, noop_per_env: bool = False):
        self._noop_per_env = bool(noop_per_env)
        self.autoreset = bool(autoreset)        # False: single-env semantics, the caller calls reset()
        if kind not in _KINDS:
            raise ValueError(f"kind must be one of {_KINDS}")
        self.obs_dtype = _resolve_env_obs_dtype(args)
        from .history import check_env_history
        self.history_len = check_env_history(kind, getattr(args, "history_len", 0), 1, getattr(args, "ragged_obs", "padded"))
        from .steplog import check_env_step_log
        self.step_log = check_env_step_log(getattr(args, "step_log", False), self.history_len, self._discrete_motor)
        if not torch.cuda.is_available():
            raise RuntimeError("active_gym envs need a ROCm GPU: the observation pipeline has no CPU implementation")
        self.args = args
        self.kind = kind
        self.num_envs = int(num_envs)
        self.obs_size = tuple(int(v) for v in args.obs_size)
        self._check_obs_size()
        self.channels = self._resolve_channels(args)     # planes per stacked frame: 1 gray, 3 colour (DMC grey=False)
        self.frame_stack = int(args.frame_stack)
        self.action_repeat = int(args.action_repeat)
        dev = getattr(args, "device", None)
        self._numpy_out = dev is None
        self.device = torch.device(dev) if dev is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

        self._build_pipeline()
        self._setup_source(args, noop_fn, env_offset)
        self._build_spaces()

    def rekind(self, kind: str):
        """Swap the wrapper kind before the first reset, keeping the host runner and its emulators (the single-env fovea
        wrappers build on the base env's core: one ALE / MuJoCo construction per env, not two)."""
        if kind not in _KINDS:
            raise ValueError(f"kind must be one of {_KINDS}")
        if self._was_reset:
            raise RuntimeError("rekind() after reset()")
        if kind != self.kind:
            if self._loop is not None:
                self._loop.close()
                self._loop = None
                self._host_step = None
            self.pipe.close()
            self.kind = kind
            self._build_pipeline()
            self._make_loop()
            self._build_spaces()
        return self

    def _build_pipeline(self):
        args, kind = self.args, self.kind
        from .history import FrameHistory, check_env_history
        check_env_history(kind, self.history_len, self.channels, getattr(args, "ragged_obs", "padded"))
        kw = dict(num_envs=self.num_envs, kind=kind, obs_size=self.obs_size, frame_stack=self.frame_stack,
                  device=self.device, obs_dtype=self.obs_dtype, channels=self.channels)
        if kind != "base":
            # these have no defaults in the reference and are read unconditionally (fov_env.py:110-120)
            self.fov_size = tuple(int(v) for v in args.fov_size)
            self.fov_init_loc = tuple(args.fov_init_loc)
            self.sensory_action_mode = args.sensory_action_mode
            if self.sensory_action_mode == "relative":
                self.sensory_action_space = np.array(args.sensory_action_space)          # fov_env.py:116
            elif self.sensory_action_mode == "absolute":
                self.sensory_action_space = np.array(self.obs_size) - np.array(self.fov_size)   # fov_env.py:118
            else:
                raise ValueError("sensory_action_mode must be 'absolute' or 'relative'")
            resize_to_full = bool(args.resize_to_full)
            mask_out = bool(args.mask_out)
            kw.update(fov_size=self.fov_size, fov_init_loc=self.fov_init_loc,
                      sensory_action_mode=self.sensory_action_mode,
                      sensory_action_space=tuple(np.asarray(args.sensory_action_space, dtype=float))
                      if self.sensory_action_mode == "relative" else None,
                      resize_to_full=resize_to_full, mask_out=mask_out, antialias=_resolve_antialias(args))
            if kind == "peripheral":
                self.peripheral_res = tuple(int(v) for v in args.peripheral_res)
                kw["peripheral_res"] = self.peripheral_res
                mask_out, resize_to_full = False, True                                  # fov_env.py:361-362
            self.mask_out, self.resize_to_full = mask_out, resize_to_full
        # raw-crop mode: the observation is the fovea's pixels themselves ([fov_h, fov_w] fixed; ragged [res_h, res_w] flexible)
        self._raw_crop = kind != "base" and not (self.mask_out or self.resize_to_full)
        # flexible env, raw-crop mode: args.ragged_obs = "packed" returns the ragged crops themselves - a list of N
        # arrays [fs, res_h, res_w] (views into one packed device buffer), what the reference's env returns per env
        # (fov_env.py:283-298) - instead of the zero-padded [N, fs, obs_h, obs_w] batch
        self._ragged_packed = kind == "flexible" and self._raw_crop and wants_packed(args)
        self.pipe = ObsPipeline(**kw)
        self.history = FrameHistory(self.pipe, self.history_len) if self.history_len > 0 else None
        self.steplog = self._env_log = self._per = None      # (the samplers and shift sources are cached on the history: rebuilt with it)
        if self.step_log:
            from .steplog import EnvStepLog, StepLog
            self.steplog = StepLog(self.history, 12 if kind == "fixed" else 4)      # motor i32 [, sensory 2 x f32]
            self._env_log = EnvStepLog(self.steplog, kind == "fixed", self.autoreset)
        self._env_ids = torch.arange(self.num_envs, dtype=torch.int32, device=self.device) if self.history is not None else None

    def _build_spaces(self):
        kind = self.kind
        # spaces (reference atari_env.py:69-70, fov_env.py:125-142,243)
        self.single_motor_space = self._motor_space()
        chan = (self.frame_stack, 3) if self.channels == 3 else (self.frame_stack,)   # colour: (fs, 3, H, W)
        full = chan + self.obs_size
        if kind == "base":
            self.single_action_space = self.single_motor_space
            self.single_observation_space = Box(low=-1., high=1., shape=full, dtype=obs_space_dtype(self.obs_dtype))
        else:
            sas = self.sensory_action_space
            spaces = {"motor_action": self.single_motor_space,
                      "sensory_action": Box(low=sas[0], high=sas[1], dtype=int)}      # scalar Box, as the reference
            if kind == "flexible":
                spaces["sensory_action_type"] = Discrete(2)
            self.single_action_space = Dict(spaces)
            shp = chan + (self.fov_size if (kind == "fixed" and self._raw_crop) else self.obs_size)
            self.single_observation_space = Box(low=-1., high=1., shape=shp, dtype=obs_space_dtype(self.obs_dtype))
        # SyncVectorEnv conventions (gymnasium<1.0): batched spaces under action_space / observation_space
        self.action_space = batch_space(self.single_action_space, self.num_envs)
        self.observation_space = batch_space(self.single_observation_space, self.num_envs)

        # RecordWrapper bookkeeping (fov_env.py:29-32,58-63)
        self.cumulative_reward = np.zeros(self.num_envs, np.float64)
        self.ep_len = np.zeros(self.num_envs, np.int64)
        # Device-tensor outputs are double-buffered: step() returns buffer t % 2, so an observation stays valid until the
        # step after next without a 115 MB clone per step (args.copy_obs=True restores a fresh tensor per call)
        shp = self.pipe.obs_shape if kind != "base" else self.pipe.full_shape
        self._copy_obs = bool(getattr(self.args, "copy_obs", False))
        # Host (NumPy) outputs: a fresh array per call by default, like the reference's envs, from the recycled pinned pool
        # (args.host_obs_buffers); args.copy_obs = False: views of a pinned pair (hostobs.py)
        self._host = HostObs(self.device, pinned_pair=getattr(self.args, "copy_obs", True) is False,
                             pool_buffers=int(getattr(self.args, "host_obs_buffers", 4) or 0)) if self._numpy_out else None
        self._obs_bufs = [torch.empty(shp, dtype=self.obs_dtype, device=self.device)
                          for _ in range(1 if (self._numpy_out or self._copy_obs) else 2)]
        self._obs_i = 0
        self._obs = self._obs_bufs[0]
        if self._ragged_packed:
            self._packed = torch.empty((self.num_envs * self.frame_stack * self.obs_size[0] * self.obs_size[1],),
                                       dtype=torch.float32, device=self.device)
            self._poff = torch.zeros((self.num_envs + 1,), dtype=torch.int64, device=self.device)
        self._loc = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.device)
        self._res = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.device)
        self._was_reset = False

    def _check_obs_size(self):
        if self.obs_size[0] != self.obs_size[1]:
            # reference: cv2.resize(dsize=obs_size) yields (obs_size[1], obs_size[0]) and the assignment into
            # frame_buffer raises (atari_env.py:74,121-128)
            raise ValueError(f"obs_size {self.obs_size} must be square for Atari (cv2.resize takes (width, height))")

    def _resolve_channels(self, args):
        """Atari observations are luminance only (the reference's Atari path, atari_env.py:74): a colour request is refused."""
        if getattr(args, "grey", True) is False or int(getattr(args, "channels", 1)) != 1:
            raise ValueError("colour observations (grey=False) are built for the DMC envs only: the Atari path is luminance only")
        return 1

    def _motor_space(self):
        return Discrete(self.runner.num_actions)

    def _ingest(self, cmd=None):
        frames, cmd = self._staging.d_frames, self._staging.d_cmd if cmd is None else cmd
        if self._compact:
            (self.pipe.ingest_gray_raw_compact if self._gray else self.pipe.ingest_compact)(frames, cmd)
        elif self._gray:
            self.pipe.ingest_gray_raw(frames, cmd)
        else:
            self.pipe.ingest(frames, cmd)

    def _extra_info(self, info):
        return info

    def _setup_source(self, args, noop_fn, env_offset):
        # host side: pinned staging for step frames and for reset frames, device twins
        from .frame_source import resolve_frame_format
        fmt = resolve_frame_format(args)         # real emulators default to ALE's own grayscale screens (atari_env.py:74)
        self._gray = fmt == "gray"
        px = () if self._gray else (3,)
        # Compact staging (default; args.compact_rows = False restores whole screens): the runner stages only the screen rows
        # the vertical resize reads (168 of 210 at 84 x 84 - SURVEY.md 8d's algorithmic bytes already leave the other 42 out),
        # so a step's H2D copy is 165 MB instead of 206 MB on the PCIe-bound RGB path
        self._compact = bool(getattr(args, "compact_rows", True))
        self._src_rows = self.pipe.source_rows() if self._compact else None
        rows = len(self._src_rows) if self._compact else nat.RAW_H
        shape = (self.num_envs, 2, rows, nat.RAW_W) + px
        rshape = (self.num_envs, 1, rows, nat.RAW_W) + px
        # Host placement (hostplan.py): this rank's share of the CPUs of its GPU's NUMA node; the pinned staging below is
        # allocated while bound to them (first touch on that node), the native runner pins one worker per CPU
        from . import hostplan
        self.host_plan = hostplan.plan_for_process(self.device.index, workers=getattr(args, "num_workers", None))
        src = getattr(args, "frame_source", "ale")
        native = isinstance(src, str) and src.startswith("native")
        # The native step loop (libagx.so: agx_loop_*, include/agx_loop.h) owns staging, copy stream, launches and the autoreset:
        # step() is then ONE C call.  Used with the native runner and device outputs (args.native_loop = False keeps the Python
        # loop below); the chunked-H2D form and the ragged packed observations stay on the Python loop.
        self._loop = None
        loop_ok = bool(native and getattr(args, "native_loop", True)
                       and not int(getattr(args, "h2d_chunk_envs", 0) or 0)
                       and not self._ragged_packed)
        # Host outputs stay on the Python loop unless args.host_obs_chunks = C > 0 asks for the chunked host-output step
        # (agx_loop_step_host, include/agx_hostout.h: gray Atari contexts, padded observations)
        hc = int(getattr(args, "host_obs_chunks", 0) or 0)
        if hc < 0:
            raise ValueError(f"host_obs_chunks must be >= 0, got {hc}")
        self.host_obs_chunks = hc if (loop_ok and self._numpy_out and self.channels == 1) else 0
        self._want_loop = loop_ok and (not self._numpy_out or self.host_obs_chunks > 0)
        if not self._want_loop:
            with hostplan.bound_to(self.host_plan["cpus"] and self.host_plan["domain"]):
                # sets doubled, with a copy stream, exactly when step() does not synchronise: outputs that stay on the device
                self._staging = Staging(self.num_envs, shape, rshape, reset_slot0=True, doubled=not self._numpy_out,
                                        device=self.device)
        if native:
            # C++ thread-per-core runner (libagx_runner.so): "native" = built-in scripted emulator,
            # "native:ale" = real ALE through atari_py's libale_c.so
            from .native_runner import NativeHostRunner
            self.runner = NativeHostRunner(args, self.num_envs, frames=None if self._want_loop else self._staging.h_frames.numpy(),
                                           workers=self.host_plan["workers"], noop_fn=noop_fn,
                                           env_offset=env_offset, backend="ale_c" if src == "native:ale" else "scripted",
                                           noop_per_env=self._noop_per_env, src_rows=self._src_rows,
                                           cpus=self.host_plan["cpus"], alloc_frames=not self._want_loop)
            self._make_loop()
        else:
            self.runner = AtariHostRunner(args, self.num_envs, frames=self._staging.h_frames.numpy(),
                                          workers=self.host_plan["workers"], noop_fn=noop_fn,
                                          env_offset=env_offset, noop_per_env=self._noop_per_env, src_rows=self._src_rows)

    def _make_loop(self):
        if getattr(self, "_want_loop", False):
            from . import hostplan
            from .native_loop import NativeStepLoop
            # its pinned staging is allocated inside: bound to this rank's CPUs (first touch on the GPU's NUMA node)
            with hostplan.bound_to(self.host_plan["cpus"] and self.host_plan["domain"]):
                self._loop = NativeStepLoop(self.pipe, self.runner, gray=self._gray, compact=self._compact, autoreset=self.autoreset)
                if self.history is not None:
                    self.history.attach(self._loop)          # the loop pushes after every observation it writes
                self._host_step = None
                if self.host_obs_chunks > 0:
                    from .native_hostout import HostOutStep
                    self._host_step = HostOutStep(self._loop, self.host_obs_chunks)      # (its pinned fov rows: same binding)

    # ------------------------------------------------------------------ plumbing
    def close(self):
        if getattr(self, "_loop", None) is not None:
            self._loop.close()
            self._loop = None
            self._host_step = None
        self.runner.close()
        self.pipe.close()

    def train(self):
        self.runner.train()

    def eval(self):
        self.runner.eval()

    @property
    def fov_loc(self) -> np.ndarray:
        return self.pipe.fov_state()[0].cpu().numpy()

    @property
    def fov_res(self) -> np.ndarray:
        return self.pipe.fov_state()[1].cpu().numpy()

    def _as_device_action(self, a, cols):
        if isinstance(a, torch.Tensor):
            t = a.detach()
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
        if t.dtype == torch.float16 or t.dtype == torch.bfloat16:
            t = t.float()
        if t.dtype in (torch.int8, torch.int16, torch.uint8, torch.bool):
            t = t.to(torch.int32)
        n = self.num_envs
        if cols and t.numel() in (n, 1) and t.numel() != n * cols:
            # the reference's sensory_action space is a SCALAR Box (fov_env.py:125-129): `action_space.sample()` gives one
            # number per env, which `np.clip(loc, 0, obs - fov)` broadcasts to (a, a) (fov_env.py:166-167)
            t = t.reshape(-1, 1).expand(n, cols)
        t = t.reshape(n, cols) if cols else t.reshape(n)
        return t.to(self.device, non_blocking=True).contiguous()

    def _observe(self, action=None, action_type=None, mask=None, out=None):
        out = self._obs if out is None else out
        if self.kind == "base":
            self.pipe.observe_full(out)
        elif self._ragged_packed:
            # no mask in the packed layout: every env is re-observed; an env without an action keeps its state
            self.pipe.fovea_packed(action, action_type=action_type, packed=self._packed, offsets=self._poff,
                                   loc_out=self._loc, res_out=self._res)
        elif self.kind == "flexible":
            self.pipe.fovea(action, action_type=action_type, mask=mask, out=out, loc_out=self._loc, res_out=self._res)
        else:
            self.pipe.fovea(action, mask=mask, out=out, loc_out=self._loc)
        return out

    def _out(self, t: torch.Tensor):
        return t.cpu().numpy() if self._numpy_out else t

    def _hist_push(self, cmd):
        """Python loop: append to the frame history after an ingest(cmd) + observation (the native loop pushes itself)."""
        if self.history is not None:
            self.history.push(cmd)

    def _hist_index(self):
        """i64 [N]: the history index of each env's newest observation (NumPy with host outputs)."""
        return self._out(self.history.last_index())

    def replay_batch(self, B: int, nstep: int = 1, gamma: float = 0.99, glimpses: Optional[int] = None, prioritized: bool = False,
                     beta: float = 0.4, shift_pad: Optional[int] = None, **sampler_kw):
        """B learner rows from the env's step log: ``steplog.batch(env.replay_sampler(**sampler_kw), B, nstep, gamma, glimpses)``
        with the payload split into ``motor_action`` (i32 [B]) and, on a fixed env, ``sensory_action`` (f32 [B, 2]): the action
        taken on seeing ``obs``.  ``ret`` / ``discount`` / ``next_obs`` are the n-step target's parts: target = ret + discount *
        value(next_obs).  ``glimpses = P`` reads the observations through the glimpse memory (the sampler's ``back`` defaults to
        P - 1 then).  ``prioritized=True`` draws through ``env.prioritized_sampler(**sampler_kw)`` instead and adds ``weight``
        (f32 [B], the importance weights at ``beta``) and ``priority`` (i64 [B], the drawn integer weights);
        ``env.update_priorities(batch, td_error)`` writes the new priorities back.  ``shift_pad = p`` reads ``obs`` and
        ``next_obs`` through ``env.random_shift(p)`` - DrQ's random shift, drawn independently for the two - and adds
        ``obs_shift`` / ``next_obs_shift`` (i32 [B, 2]); not together with ``glimpses``.  Rows with ok = 0 are to be ignored.
        Needs ``step_log``: ValueError otherwise."""
        from .augment import check_no_glimpses, check_pad
        from .steplog import check_nstep
        nstep = check_nstep(nstep)
        if shift_pad is not None:
            check_pad(shift_pad)
            check_no_glimpses(glimpses)
        if self.steplog is None:
            raise ValueError("replay_batch needs a step log (AtariEnvArgs.step_log = True, history_len > 0)")
        if glimpses is not None:
            sampler_kw.setdefault("back", int(glimpses) - 1)
            self.history.memory(glimpses)                        # ValueError for a kind or mode that is not served, before a draw
        if prioritized:
            sampler = self._per = self.prioritized_sampler(**sampler_kw)
        else:
            sampler = self.replay_sampler(**sampler_kw)
        out = self.steplog.batch(sampler, B, nstep, gamma, glimpses, shift=None if shift_pad is None else self.random_shift(shift_pad))
        words = out.pop("payload").view(torch.int32)
        out["motor_action"] = words[:, 0].contiguous()
        if self.kind == "fixed":
            out["sensory_action"] = words[:, 1:3].contiguous().view(torch.float32)
        if prioritized:
            out["weight"], out["priority"] = sampler.importance(beta), sampler.weight
        return out

    def sequence_batch(self, B: int, length: int, nstep: int = 1, gamma: float = 0.99, min_length: Optional[int] = None,
                       prioritized: bool = False, beta: float = 0.4, planes: Optional[int] = None, time_major: bool = False, **sampler_kw):
        """B sequences of ``length`` consecutive steps of one episode each, for a recurrent learner:
        ``sequence.SequenceReplay(env.steplog).batch(...)`` with the starts drawn by ``env.replay_sampler(forward = (min_length or
        length) - 1, **sampler_kw)``, so that every ok sequence has at least ``min_length`` live steps; a sampler guarantees at
        most 65, so a longer ``length`` needs ``min_length`` (ValueError otherwise) and its sequences are padded where the episode
        or the history ends.  Per step ([B, length], or [length, B] with ``time_major``): ``obs`` (``planes`` newest stacked
        frames, None: all), ``live``, ``fov_loc``, ``steps`` / ``next_index`` / ``next_step`` / ``ret`` / ``discount`` / ``flags``
        of the n-step target, and the payload split into ``motor_action`` (i32) and, on a fixed env, ``sensory_action`` (f32
        [.., 2]): the action taken on seeing that step's observation.  Padded steps are zeros.  ``prioritized=True`` draws through
        ``env.prioritized_sampler`` and adds ``weight`` / ``priority`` as ``replay_batch`` does;
        ``env.update_priorities(batch, sequence.mixed_priority(td_abs, batch["live"]))`` writes a sequence's priority back to
        its start.  Needs ``step_log``: ValueError otherwise."""
        from .sequence import SequenceReplay, check_sequence_draw
        from .steplog import check_nstep
        nstep = check_nstep(nstep)
        forward = check_sequence_draw(length, min_length)
        if self.steplog is None:
            raise ValueError("sequence_batch needs a step log (AtariEnvArgs.step_log = True, history_len > 0)")
        if "forward" in sampler_kw:
            raise ValueError("sequence_batch sets the sampler's forward itself: pass min_length")
        if prioritized:
            sampler = self._per = self.prioritized_sampler(forward=forward, **sampler_kw)
        else:
            sampler = self.replay_sampler(forward=forward, **sampler_kw)
        out = SequenceReplay(self.steplog).batch(sampler, B, length, nstep, gamma, planes, time_major)
        words = out.pop("payload").view(torch.int32)
        out["motor_action"] = words[..., 0].contiguous()
        if self.kind == "fixed":
            out["sensory_action"] = words[..., 1:3].contiguous().view(torch.float32)
        if prioritized:
            out["weight"], out["priority"] = sampler.importance(beta), sampler.weight
        return out

    def sequence_retrace(self, batch: dict, q: torch.Tensor, v: torch.Tensor, c: torch.Tensor, boot: Optional[torch.Tensor] = None,
                         out: Optional[dict] = None, time_major: bool = False) -> dict:
        """The Retrace-family Q-return over a ``sequence_batch(nstep=1)`` -> dict of ``target``, ``td`` (f32) and ``valid`` (u8),
        [B, length]: ``retrace.Retrace(env.steplog).targets(...)``, for an off-policy recurrent learner.  The whole recipe::

            batch = env.sequence_batch(B, L, nstep=1)                             # ret = the step's reward, steps = 1 where a row exists
            q_all, pi = learner(batch["obs"])                                      # [B, L, A]: the Q values and the target policy
            a = batch["motor_action"].long()[..., None]
            q, v = q_all.gather(-1, a)[..., 0], (pi * q_all).sum(-1)
            last = batch["next_index"][:, -1]                                      # -1 where the sequence stops short: boot is not read there
            boot_obs = env.history.observe(batch["env"], last)[0]                  # the observation behind the last step
            q_b, pi_b = learner.single(boot_obs)
            boot = (pi_b * q_b).sum(-1)
            at = batch["index"][:, None] + torch.arange(L, device=device)         # step l is the env-step (env, index + l)
            logp_mu = env.behaviour_log().read(at.reshape(-1), batch["env"].repeat_interleave(L)).reshape(B, L)     # mu, as written at every act
            c = retrace.coefficients(pi.log().gather(-1, a)[..., 0], logp_mu, lam=0.95, kind="retrace")
            out = env.sequence_retrace(batch, q, v, c, boot)
            loss = ((q - out["target"].detach()) ** 2 * out["valid"]).sum() / out["valid"].sum().clamp(min=1)
            priority = sequence.mixed_priority(out["td"].abs(), batch["live"])     # then env.update_priorities(batch, priority)

        ``kind="qlambda"`` and ``"tree"`` need no behaviour policy.  ``valid`` is ``live & (steps == 1)``; every other step is 0
        in all three outputs.  ``out``: the dict of an earlier call, written in place.  Needs ``step_log``: ValueError otherwise."""
        if self.steplog is None:
            raise ValueError("sequence_retrace needs a step log (AtariEnvArgs.step_log = True, history_len > 0)")
        from .retrace import Retrace
        return Retrace(self.steplog).targets(batch, q, v, c, boot, out, time_major)

    def _rollout(self, who: str, vtrace: bool = False):
        """The env's rollout.Rollout (vtrace: vtrace.VTrace) on its step log; ValueError without one."""
        if self.steplog is None:
            raise ValueError(f"{who} needs a step log (AtariEnvArgs.step_log = True, history_len > 0)")
        from .rollout import Rollout
        from .vtrace import VTrace
        return (VTrace if vtrace else Rollout)(self.steplog)

    def rollout_batch(self, L: int) -> dict:
        """The last ``L`` transitions of every env, for an on-policy learner: ``rollout.Rollout(env.steplog).gather(L)`` with the
        payload split into ``motor_action`` (i32 [L, N]) and, on a fixed env, ``sensory_action`` (f32 [L, N, 2]): the action taken
        on seeing ``obs_index``.  Time-major; ``live`` marks the slots that hold a transition, ``ends`` where an episode ended
        behind one and whether the return bootstraps there (rollout.TERMINATED / TRUNCATED / CUT / BOOT).  Read the observations
        with ``env.history.observe(*Rollout.flat(batch))``.  Needs ``step_log``: ValueError otherwise."""
        from .rollout import check_rollout_length
        L = check_rollout_length(L)
        out = self._rollout("rollout_batch").gather(L)
        words = out.pop("payload").view(torch.int32)
        out["motor_action"] = words[..., 0].contiguous()
        if self.kind == "fixed":
            out["sensory_action"] = words[..., 1:3].contiguous().view(torch.float32)
        return out

    def rollout_gae(self, batch: dict, value: torch.Tensor, boot_value: Optional[torch.Tensor], gamma: float = 0.99, lam: float = 0.95):
        """GAE(lambda) over a ``rollout_batch`` -> (adv, ret), f32 [L, N]: ``rollout.Rollout(env.steplog).gae(...)``.  ``value`` is
        the critic on ``obs_index``, ``boot_value`` the critic on ``next_index`` at the slots ``Rollout.boot_rows(batch)`` names."""
        return self._rollout("rollout_gae").gae(batch, value, boot_value, gamma, lam)

    def rollout_vtrace(self, batch: dict, value: torch.Tensor, boot_value: Optional[torch.Tensor], rho: torch.Tensor, gamma: float = 0.99,
                       lam: float = 1.0, rho_bar: float = 1.0, c_bar: float = 1.0, pg_rho_bar: float = 1.0):
        """V-trace over a ``rollout_batch`` -> (vs, pg_adv), f32 [L, N]: ``vtrace.VTrace(env.steplog).returns(...)``, for a learner
        whose actors lag it.  ``value`` and ``boot_value`` are ``rollout_gae``'s; ``rho`` is pi / mu of the action of every slot,
        mu's log-probability being what ``env.behaviour_log()`` kept.  Needs ``step_log``: ValueError otherwise."""
        return self._rollout("rollout_vtrace", vtrace=True).returns(batch, value, boot_value, rho, gamma, lam, rho_bar, c_bar, pg_rho_bar)

    def _minibatcher(self, who: str, seed: Optional[int]):
        """The env's minibatch.Minibatcher of this seed (None: ``args.seed``), cached on the history; ValueError without a step log."""
        roll = self._rollout(who)
        seed = int(getattr(self.args, "seed", 0) or 0) if seed is None else int(seed)
        return self.history.minibatcher(roll, seed)

    def _with_payload(self, batch: dict) -> dict:
        """A ``rollout_batch`` with its actions put back into one payload u8 [L, N, W], as the step log holds them."""
        parts = [batch["motor_action"].view(torch.uint8).reshape(*batch["motor_action"].shape, 4)]
        if self.kind == "fixed":
            parts.append(batch["sensory_action"].view(torch.uint8).reshape(*batch["motor_action"].shape, 8))
        return dict(batch, payload=torch.cat(parts, -1))

    def _split_payload(self, rows: dict) -> dict:
        words = rows.pop("payload").view(torch.int32)
        rows["motor_action"] = words[:, 0].contiguous()
        if self.kind == "fixed":
            rows["sensory_action"] = words[:, 1:3].contiguous().view(torch.float32)
        return rows

    def rollout_boot(self, batch: dict, capacity: Optional[int] = None, seed: Optional[int] = None) -> dict:
        """The slots of a ``rollout_batch`` whose return bootstraps (BOOT), in list order and without a shuffle, at the fixed
        shape ``[capacity]`` (default ``2 * N``): ``minibatch.Minibatcher.take(batch, 0, capacity, "boot", permute=False)`` plus
        ``total``, the device i32 [1] number of such slots - the host never waits for it, so an overflow (``total > capacity``)
        is visible later.  The capture-safe replacement for ``Rollout.boot_rows``::

            rows = env.rollout_boot(batch)
            obs = env.history.observe(rows["env"], rows["next_index"])[0]         # 1. observe the list (rows past it: valid = 0)
            v = critic(obs)                                                        # 2. evaluate the critic
            boot_value = torch.zeros_like(batch["reward"])
            env.rollout_scatter(rows, v, boot_value)                               # 3. scatter into a zeroed boot_value

        Needs ``step_log``: ValueError otherwise."""
        from .minibatch import check_minibatch_size
        mb = self._minibatcher("rollout_boot", seed)
        _, capacity = check_minibatch_size(2 * self.num_envs if capacity is None else capacity)
        total = mb.select(batch, "boot")
        rows = mb.take(self._with_payload(batch), 0, capacity, "boot", permute=False)
        rows["total"] = total
        return self._split_payload(rows)

    def rollout_scatter(self, rows: dict, values: torch.Tensor, dst: torch.Tensor, seed: Optional[int] = None) -> torch.Tensor:
        """``minibatch.Minibatcher.scatter``: ``values`` (f32 [S]) of the valid ``rows`` into ``dst`` (f32 [L, N]) at their slots."""
        return self._minibatcher("rollout_scatter", seed).scatter(rows, values, dst)

    def rollout_minibatches(self, batch: dict, size: int, streams=None, seed: Optional[int] = None):
        """One epoch over the live slots of a ``rollout_batch``, freshly shuffled on the device: a generator of
        ``ceil(L * N / size)`` dicts of ``size`` rows each - ``slot``, ``env``, ``obs_index``, ``next_index``, ``valid``,
        ``motor_action`` (i32 [size]) and, on a fixed env, ``sensory_action`` (f32 [size, 2]), and one f32 [size] entry per name
        in ``streams`` (a dict name -> f32 [L, N] such as adv / ret / value / logp, or names of entries of ``batch``).  The number
        of minibatches is that of a full rollout, so it is no data: rows past the live slots wrap to real samples with
        ``valid = 0``, and a learner multiplies its per-row loss by ``valid``.  Every live slot is in exactly one row with
        ``valid = 1``.  Nothing synchronises.  Needs ``step_log``: ValueError otherwise."""
        from .minibatch import check_epoch_size, check_streams
        mb = self._minibatcher("rollout_minibatches", seed)
        size = check_epoch_size(size)
        streams = check_streams(streams, batch)
        return self._minibatch_epoch(mb, self._with_payload(batch), size, streams)

    def _minibatch_epoch(self, mb, batch, size, streams):
        cells = int(batch["ends"].shape[0]) * self.num_envs
        mb.select(batch, "live")
        for first in range(0, cells, size):
            yield self._split_payload(mb.take(batch, first, size, "live", True, streams))

    def rollout_chunks(self, batch: dict, C: int, size: int, streams=None, seed: Optional[int] = None):
        """One epoch over the chunks of a ``rollout_batch`` - runs of ``C`` consecutive steps of one env that hold a live slot -
        freshly shuffled on the device, for a RECURRENT on-policy learner: a generator of ``ceil(N * ceil(L / C) / size)`` dicts
        of ``size`` chunks each (the number is that of a full rollout, so it is no data).  Per step, time-major ``[C, size]``:
        ``slot``, ``env``, ``obs_index``, ``next_index``, ``ends``, ``start``, ``mask``, ``motor_action`` (i32) and, on a fixed env,
        ``sensory_action`` (f32 [C, size, 2]), and one f32 entry per name in ``streams`` (a dict name -> f32 [L, N] such as adv /
        ret / value / logp, or names of entries of ``batch``).  Per chunk, ``[size]``: ``chunk``, ``first``, ``steps``,
        ``state_index``, ``valid``.  Every live slot is in exactly one step with ``mask = 1``; chunks past the list wrap to real
        ones with ``mask = 0``, padding steps hold -1 / zeros.  Nothing synchronises.  The whole recipe::

            blog = env.behaviour_log(width=H)
            ...                                                        # at every act: the state the actor entered the step with
            blog.write(info["history_index"], h)                       # 1. store the actor's hidden state
            batch = env.rollout_batch(L)
            for rows in env.rollout_chunks(batch, C, size, {"adv": adv, "ret": ret}):
                stored = blog.read(rows["state_index"], rows["env"][0])     # 2. read it back at (env[0], state_index)
                obs = env.history.observe(rows["env"].flatten(), rows["obs_index"].flatten())[0]    # 3. index -1 is left untouched
                h = stored
                for l in range(C):                                     # 4. the RNN over l
                    h = torch.where((rows["start"][l] & 1).bool()[:, None], stored, h)  #    load the stored state where start & 1 ...
                    h = torch.where((rows["start"][l] & 2).bool()[:, None], h0, h)      #    ... restart where start & 2
                    out, h = rnn(obs.view(C, size, *obs.shape[1:])[l], h)
                loss = (per_step_loss * rows["mask"]).sum() / rows["mask"].sum().clamp(min=1)        # 5. multiply by mask

        Needs ``step_log``: ValueError otherwise."""
        from .chunks import check_chunk_length, check_rows, check_streams
        from .minibatch import check_epoch_size
        roll = self._rollout("rollout_chunks")
        seed = int(getattr(self.args, "seed", 0) or 0) if seed is None else int(seed)
        ch = self.history.chunker(roll, seed)
        L = int(batch["ends"].shape[0])
        C = check_chunk_length(C, L)
        size = check_epoch_size(size)
        check_rows(C, size)
        streams = check_streams(streams, batch)
        return self._chunk_epoch(ch, self._with_payload(batch), C, size, streams)

    def _chunk_epoch(self, ch, batch, C, size, streams):
        cells = self.num_envs * (-(-int(batch["ends"].shape[0]) // C))
        ch.select(batch, C)
        for first in range(0, cells, size):
            rows = ch.take(batch, first, size, C, True, streams)
            words = rows.pop("payload").view(torch.int32)
            rows["motor_action"] = words[..., 0].contiguous()
            if self.kind == "fixed":
                rows["sensory_action"] = words[..., 1:3].contiguous().view(torch.float32)
            yield rows

    def behaviour_log(self, width: int = 1):
        """A vtrace.BehaviourLog on the env's frame history, cached per width: ``write(info["history_index"], logp)`` at every
        act, ``read(batch["obs_index"])`` after ``rollout_batch``.  Needs ``history_len`` > 0: ValueError otherwise."""
        if self.history is None:
            raise ValueError("behaviour_log needs a frame history (AtariEnvArgs.history_len > 0)")
        return self.history.behaviour(width)

    def update_priorities(self, batch: dict, td_error: torch.Tensor, alpha: float = 0.6, eps: float = 1e-6, **sampler_kw):
        """Write priority = (|td_error| + eps) ** alpha for the rows of a ``replay_batch(..., prioritized=True)`` batch; rows with
        ok = 0 are skipped, and so are rows evicted since the draw.  The table is that of the sampler the last prioritized
        ``replay_batch`` drew from, or of ``env.prioritized_sampler(**sampler_kw)`` where arguments are given."""
        sampler = self.prioritized_sampler(**sampler_kw) if sampler_kw else self._per
        if sampler is None:
            raise ValueError("update_priorities needs a batch of replay_batch(..., prioritized=True), or the sampler's arguments")
        skip = batch["ok"] == 0
        env = torch.where(skip, torch.full_like(batch["env"], -1), batch["env"])
        index = torch.where(skip, torch.full_like(batch["index"], -1), batch["index"])
        sampler.update_td(env, index, td_error, alpha, eps)

    def glimpse_memory(self, glimpses: int = 3, out: Optional[torch.Tensor] = None):
        """The glimpse memory of the observation the last ``reset`` / ``step`` returned, for all N envs: the elementwise
        maximum over each env's last up-to-``glimpses`` observations since its last reset (``history.memory(glimpses).observe`` at
        ``history.last_index()``; an env autoreset in the last step gives just its returned observation).  Needs
        ``history_len`` > 0, kind "fixed" and mask_out or resize_to_full mode: ValueError otherwise."""
        if self.history is None:
            raise ValueError("glimpse_memory needs a frame history (AtariEnvArgs.history_len > 0)")
        obs, _, _ = self.history.memory(glimpses).observe(self._env_ids, self.history.last_index(), out=out)
        return self._out(obs)

    def replay_sampler(self, back: int = 0, forward: int = 1, attempts: int = 16, seed: Optional[int] = None):
        """A replay.ReplaySampler on the env's frame history, cached per argument tuple: ``sample(B)`` draws (env, index) pairs
        that are retained, have ``back`` valid earlier glimpses of their episode and ``forward`` later appends of it, and
        ``transitions(B)`` re-creates both observations (index and index + forward never straddle a reset).  ``seed=None``
        takes ``args.seed``.  Needs ``history_len`` > 0: ValueError otherwise."""
        if self.history is None:
            raise ValueError("replay_sampler needs a frame history (AtariEnvArgs.history_len > 0)")
        seed = int(getattr(self.args, "seed", 0) or 0) if seed is None else int(seed)
        return self.history.sampler(back, forward, attempts, seed)

    def random_shift(self, pad: int = 4, seed: Optional[int] = None):
        """An augment.RandomShift on the env's frame history, cached per argument tuple: ``observe(env, index)`` is
        ``history.observe`` with every sample moved by a freshly drawn shift of up to ``pad`` pixels either way.  ``seed=None``
        takes ``args.seed``.  Needs ``history_len`` > 0: ValueError otherwise."""
        if self.history is None:
            raise ValueError("random_shift needs a frame history (AtariEnvArgs.history_len > 0)")
        seed = int(getattr(self.args, "seed", 0) or 0) if seed is None else int(seed)
        return self.history.shift(pad, seed)

    def prioritized_sampler(self, back: int = 0, forward: int = 1, seed: Optional[int] = None):
        """A priority.PrioritizedSampler on the env's frame history, cached per argument tuple: ``sample(B)`` draws the pairs
        ``replay_sampler`` accepts with probability proportional to their priority, ``update_td`` sets priorities.  ``seed=None``
        takes ``args.seed``.  Needs ``history_len`` > 0: ValueError otherwise."""
        if self.history is None:
            raise ValueError("prioritized_sampler needs a frame history (AtariEnvArgs.history_len > 0)")
        seed = int(getattr(self.args, "seed", 0) or 0) if seed is None else int(seed)
        return self.history.prioritized(back, forward, seed)

    def _next_obs_buffer(self, keep=False):
        """Turn to the other output buffer; keep: with the current observations in it (before a masked observe: the envs that
        are not reset keep their observation in the fresh buffer)."""
        prev = self._obs
        self._obs_i = (self._obs_i + 1) % len(self._obs_bufs)
        self._obs = self._obs_bufs[self._obs_i]
        if keep and len(self._obs_bufs) > 1:
            self._obs.copy_(prev)

    def _outs(self):
        """(observation buffer, fov_loc | None, fov_res | None): the device outputs this kind writes."""
        return self._obs, self._loc if self.kind != "base" else None, self._res if self.kind == "flexible" else None

    def _ret_obs(self, obs):
        if self._ragged_packed:
            off = self._poff.cpu().numpy()
            res = self._res.cpu().numpy()
            flat = self._packed[:int(off[-1])]
            flat = flat.cpu().numpy() if self._numpy_out else flat.clone()   # (the packed buffer is not double-buffered)
            return [flat[int(off[i]):int(off[i + 1])].reshape(self.frame_stack, int(res[i, 0]), int(res[i, 1]))
                    for i in range(self.num_envs)]
        if self._numpy_out:
            return self._host.fetch(obs)
        return obs.clone() if self._copy_obs else obs

    def _info(self, raw_reward, h_loc=None, h_res=None):
        """The per-env info of the current state; h_loc / h_res: fov rows the chunked host-output step already brought home."""
        info = {"raw_reward": np.asarray(raw_reward, dtype=np.float64).copy(),
                "reward": self.cumulative_reward.copy(), "ep_len": self.ep_len.copy()}
        info.update(fov_entries(*self._outs()[1:], self._numpy_out, h_loc, h_res))
        if self.history is not None:
            info["history_index"] = self._hist_index()
        return self._extra_info(info)

    def _after_reset(self, idx=slice(None)):
        """What reset() and reset_envs() return, once the observation of the envs in `idx` is enqueued."""
        self.cumulative_reward[idx] = 0
        self.ep_len[idx] = 0
        self._was_reset = True
        return self._ret_obs(self._obs), with_masks(self._info(np.zeros(self.num_envs)), self.num_envs)

    # ------------------------------------------------------------------ API
    def reset(self, seed=None, options=None):
        """Reset every env (the reference ignores seed/options too, atari_env.py:150-152)."""
        if self._loop is not None:
            self._next_obs_buffer()
            self._loop.reset(*self._outs())
            return self._after_reset()
        self._staging.reset_all(self.runner.reset)
        self._ingest()
        if self.kind != "base":
            self.pipe.fovea_reset()
        # a fresh output buffer: the observation a caller still holds from the previous step() (valid until the step after
        # next) must not be overwritten by the reset observation
        self._next_obs_buffer()
        self._observe()
        self._hist_push(self._staging.d_cmd)
        self._staging.release()
        return self._after_reset()

    def step(self, action):
        if not self._was_reset:
            raise RuntimeError("call reset() before step()")
        n = self.num_envs
        if self.kind == "base":
            motor, sens, stype = action, None, None
        else:
            motor = action["motor_action"]
            sens = self._as_device_action(action["sensory_action"], 2)
            stype = None
            if self.kind == "flexible":
                stype = self._as_device_action(action["sensory_action_type"], 0).to(torch.int32)
        if isinstance(motor, torch.Tensor):
            motor = motor.detach().cpu().numpy()
        if self._loop is not None:
            return self._step_native(motor, sens, stype)
        st = self._staging
        h_frames = st.begin_step()              # the other pinned set and device screen buffer
        if st.doubled:
            self.runner.set_frames(h_frames)
        self._next_obs_buffer()
        chunk = int(getattr(self.args, "h2d_chunk_envs", 0) or 0)
        if chunk > 0 and hasattr(self.runner, "step_begin"):
            # native runner: chunk c's screens cross PCIe while chunk c+1 is still emulating
            nc = self.runner.step_begin(motor, chunk)
            for c in range(nc):
                self.runner.step_wait(c)
                st.upload_rows(c * chunk, min(n, (c + 1) * chunk))
            reward, done, cmd, raw = self.runner.step_finish()
            st.upload_cmd(cmd)
        else:
            reward, done, cmd, raw = self.runner.step(motor)
            st.upload(cmd)
        if self._ragged_packed and sens is not None:
            # packed ragged observations: ingest + state / scan + crops as one ABI call, two launches (agx_step_flexible_packed)
            self.pipe.step_flexible_packed(st.d_frames, st.d_cmd, sens, action_type=stype, packed=self._packed,
                                           offsets=self._poff, loc_out=self._loc, res_out=self._res)
            obs = self._obs
        else:
            self._ingest()
            obs = self._observe(sens, stype)
            self._hist_push(st.d_cmd)
        self.ep_len += 1
        self.cumulative_reward += raw                   # unclipped, fov_env.py:62
        info = self._info(raw)
        truncated = np.zeros(n, bool)                   # always False, atari_env.py:145
        infos = with_masks(info, n)
        if self.autoreset and done.any():
            idx = np.nonzero(done)[0]
            # env.reset() of the done envs inside the same step (SyncVectorEnv, gymnasium<1.0).  Host first (emulators, pinned
            # staging), then ONE batch of device work: uploads, the gathers of the terminal observations / infos (the kernels
            # below overwrite them), ingest of the reset screens, masked re-observation.
            mask, d_idx = st.reset_envs(idx, self.runner.reset)
            if self._ragged_packed:
                cur = self._ret_obs(obs)
                fo = [cur[i].copy() if isinstance(cur[i], np.ndarray) else cur[i].clone() for i in idx]
            else:
                fo = self._out(obs.index_select(0, d_idx))
            # device-tensor info entries (fov_loc / fov_res with device outputs): one gather per key, rows handed out as views
            gathered = {key: val.index_select(0, d_idx) for key, val in info.items() if isinstance(val, torch.Tensor)}
            final = terminal_rows(n, idx, fo, info, gathered)
            self._ingest(st.d_rcmd)
            self.cumulative_reward[idx] = 0
            self.ep_len[idx] = 0
            if self.kind == "base":
                self._observe()
            else:
                self.pipe.fovea_reset(mask)
                self._observe(None, None, mask=mask)
            self._hist_push(st.d_rcmd)
            rinfo = self._info(np.zeros(n))
            for key in info:
                if isinstance(info[key], torch.Tensor):
                    infos[key] = torch.where(mask.bool().reshape((n,) + (1,) * (info[key].ndim - 1)), rinfo[key], info[key])
                else:
                    infos[key] = np.where(done.reshape((n,) + (1,) * (info[key].ndim - 1)), rinfo[key], info[key])
            attach_final(infos, done, *final)
        if self.steplog is not None:
            self._env_log.record(motor, sens, reward, done)
        st.release()
        return self._ret_obs(obs), reward, done, truncated, infos

    def _step_native(self, motor, sens, stype):
        """step() through the native loop: one C call does emulators -> staging -> H2D -> ingest -> fovea -> autoreset; what is
        left here is the bookkeeping the reference's RecordWrapper / SyncVectorEnv do in Python (counters, info dicts)."""
        from .pipeline import action_dt
        from .runner import check_motor_actions
        n = self.num_envs
        motor = check_motor_actions(motor, self.runner.num_actions).reshape(n)
        self._next_obs_buffer()
        dt = action_dt(sens)
        # host outputs in env chunks (args.host_obs_chunks): straight into a pinned buffer, observations, fov rows and terminal
        # rows as NumPy; without a pinned destination (pool budget spent) this call is the unchunked step + copy
        h = self._host.take(self._obs) if self._host_step is not None else None
        h_loc = h_res = None
        if h is not None:
            reward, raw, done, idx, fo, fl, fr, h_loc, h_res = self._host_step.step(motor, sens, dt, stype, *self._outs(), h)
        else:
            reward, raw, done, idx, fo, fl, fr = self._loop.step(motor, sens, dt, stype, *self._outs())
            if self._numpy_out:
                fo, fl, fr = (None if t is None else t.cpu().numpy() for t in (fo, fl, fr))
        self.ep_len += 1
        self.cumulative_reward += raw                   # unclipped, fov_env.py:62
        truncated = np.zeros(n, bool)                   # always False, atari_env.py:145
        # after the loop's step and reset pushes, and its masked re-observation: self._loc / self._res and the history index hold
        # the step's values, overwritten for the envs that were reset; the counters are still the terminal ones
        info = self._info(raw, h_loc, h_res)
        final = None
        if self.autoreset and len(idx):
            # terminal observations / infos of the envs that ended an episode: rows of the loop's side buffers (cloned: the loop
            # reuses them next step; NumPy rows already are copies), handed out as views like the Python loop's index_select rows
            if not self._numpy_out:
                fo = fo.clone()
            # the terminal observation's history index: the append before the reset's
            final = terminal_rows(n, idx, fo, {key: info[key] for key in _COUNTERS}, fov_entries(fl, fr, self._numpy_out),
                                  info["history_index"] - 1 if self.history is not None else None)
            self.cumulative_reward[idx] = 0
            self.ep_len[idx] = 0
            # the returned infos carry the reset values for those envs (SyncVectorEnv overwrites them with the reset infos)
            for key in _COUNTERS:
                info[key][idx] = 0
        infos = with_masks(info, n)
        if final is not None:
            attach_final(infos, done, *final)
        if self.steplog is not None:
            self._env_log.record(motor, sens, reward, done)
        obs = self._host.hand_out(h) if h is not None else self._ret_obs(self._obs)
        return obs, reward, done, truncated, infos

    def reset_envs(self, idx):
        """Reset only the envs in `idx` (what a caller without autoreset does after `done`)."""
        idx = [int(i) for i in idx]
        if self._loop is not None:
            self._next_obs_buffer(keep=True)
            self._loop.reset_envs(idx, *self._outs())
            return self._after_reset(idx)
        st = self._staging
        mask, _ = st.reset_envs(idx, self.runner.reset)
        self._ingest(st.d_rcmd)
        # a fresh output buffer, as in reset(): the terminal observation the caller holds from step() stays untouched
        self._next_obs_buffer(keep=self.kind != "base")
        if self.kind == "base":
            self._observe()
        else:
            self.pipe.fovea_reset(mask)
            self._observe(None, None, mask=mask)
        self._hist_push(st.d_rcmd)
        st.release()
        return self._after_reset(idx)

    def render(self, index=0):
        return self.runner.render(index)
