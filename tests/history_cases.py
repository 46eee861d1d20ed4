"""The sweep of tests/test_gpu_history_geometry.py, derived from tests/golden/geometry_cases.json (no second table), and the
parts of a run that the CPU check (tests/test_history_cases_cpu.py) and the GPU module share: the command bytes, the NumPy frames
and float actions, and a NumPy re-derivation of every env's stack and of the oracle's fov_loc - so that a history reader can be
held against oracle.FixedFovealOracle in float64 from the inputs alone, without any kernel of ours in between.

A sweep entry is one (geometry, fs, aa, mode): every distinct (obs, fov, fs, aa) of the table whose plan has a fixed_resize /
fixed_raw / fixed_mask label that is not a refusal, in each such mode; the compile-time geometry 84 / 30 at fs = 4 for aa 0 and
aa 1 (the table's fixed rows are all run-time geometries); and "full" on a base context once per distinct obs.  Pure NumPy."""
import json
import os
import re
import zlib
from collections import namedtuple

import numpy as np

from glimpse_model import taken_count
from history_model import CLEAR, SKIP, HistoryModel

TABLE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry_cases.json")))
FIXED_KEYS = {"fixed_resize": "resize", "fixed_raw": "raw", "fixed_mask": "mask"}
HEADLINE = ((84, 84), (30, 30))      # agx_plan.h: headline_fixed
K_WIN_REGS = 3                       # agx_fixed_phases.h: kWinRegs, window dwords a thread stages in registers (x 256 threads)
K_THREADS = 256
K_MEM_TABLE_BYTES = 8 * 16           # agx_fixed_phases.h: kMemTableBytes = AGX_GLIMPSE_LIMIT * 16
K_MAX_LDS = 160 * 1024               # agx_plan.h: kMaxLds

# kind: "fixed" | "base"; mode: "resize" | "raw" | "mask" | "full"; label: the table's plan label ("" where the table has none)
Case = namedtuple("Case", "obs fov fs aa kind mode label")


def _label(v):
    """tests/test_gpu_geometry.py's: a plan label as part of a test id, without the LDS bytes."""
    v = re.sub(r" lds=\d+", "", v)
    return re.sub(r"[^A-Za-z0-9.+]+", ".", v.replace("<", "_").replace(">", "")).strip(".")


def case_id(c):
    if c.kind == "base":
        return "o{}x{}_fs{}-full".format(*c.obs, c.fs)
    return "o{}x{}_f{}x{}_fs{}_aa{}-fixed_{}-{}".format(*c.obs, *c.fov, c.fs, c.aa, c.mode, _label(c.label))


def lds_bytes(c):
    """The LDS the table states for the case's launch (0 where it states none: the headline rows and "full")."""
    m = re.search(r"lds=(\d+)", c.label)
    return int(m.group(1)) if m else 0


def fixed_pad(fh, ow):
    return (fh * ow + 15) & ~15


def memory_lds(c, glimpses):
    """agx_plan.h's memory_lds, restated for the decision which glimpse counts a case can run; the GPU module holds the restatement
    against the library's own number wherever it refuses."""
    (oh, ow), (fh, fw) = c.obs, c.fov
    b = K_MEM_TABLE_BYTES + glimpses * fixed_pad(fh, ow)
    if c.mode == "resize":
        b += oh * 16 + 2 * fh * ow * 4
        if (c.obs, c.fov) != HEADLINE:
            b += oh * ow * 4
    return b


def sweep():
    """The (case, mode) list, in table order."""
    out, seen = [], set()
    for row in TABLE:
        geo = (tuple(row["obs"]), tuple(row["fov"]), row["fs"], row["aa"])
        for key, mode in FIXED_KEYS.items():
            label = row["plan"].get(key)
            if label is None or label.startswith("refused") or geo + (mode,) in seen:
                continue
            seen.add(geo + (mode,))
            out.append(Case(*geo, "fixed", mode, label))
    for aa in (0, 1):
        for mode in FIXED_KEYS.values():
            if HEADLINE + (4, aa, mode) not in seen:
                seen.add(HEADLINE + (4, aa, mode))
                out.append(Case(*HEADLINE, 4, aa, "fixed", mode, "fixed<GeomS>"))
    full = {}
    for c in out:
        full.setdefault(c.obs, Case(c.obs, (0, 0), c.fs, 1, "base", "full", ""))
    return out + list(full.values())


SWEEP = sweep()


# ---------------------------------------------------------------------------------------------- the run of a case
def shape_of_run(c):
    """(N, T, steps): N = 3 and T = fs + 2, and enough steps for every env's indices to wrap more than once.  At 256 x 256 (an
    observation is 256 KB) N = 2, and T = fs + 3: two envs retain 2 T rows, and 8 valid samples are asked of every case."""
    big = c.obs[0] * c.obs[1] >= 256 * 256
    T = c.fs + (3 if big else 2)
    return (2 if big else 3), T, 2 * T + 3


def commands(seed, N, steps, p_clear=0.15, p_skip=0.15):
    from test_gpu_history import commands as cmds       # (the one statement of the command bytes)
    return cmds(seed, N, steps, p_clear, p_skip)


def model_of(c, cmds, shape=None):
    N, T, _ = shape or shape_of_run(c)
    m = HistoryModel(N, c.fs, T)
    issued = []
    for cmd in cmds:
        idx = m.push(cmd)
        issued += [(n, int(k)) for n, k in enumerate(idx) if k >= 0]
    return m, issued


def kinds(c, m, issued):
    """(valid, zero-frame, evicted) counts of the issued samples."""
    valid = [s for s in issued if m.valid(*s)]
    return len(valid), sum(None in m.rows(*s) for s in valid), len(issued) - len(valid)


MIN_VALID = 8


def seed_ok(c, cmds):
    """The condition on a case's command bytes, on the model alone: enough valid samples, an evicted one, a zero frame inside a
    valid stack (fs >= 2: a stack of one frame has no older frame to be zero), every env's indices wrap, some sample's
    glimpse memory takes more than its own glimpse, and CLEAR and SKIP both occur."""
    N, T, _ = shape_of_run(c)
    m, issued = model_of(c, cmds)
    valid, zero, evicted = kinds(c, m, issued)
    older = any(taken_count(m, n, k, 3) >= 2 for n, k in issued)            # a glimpse memory with an older glimpse in it
    return bool(valid >= MIN_VALID and evicted >= 1 and (zero >= 1 or c.fs == 1) and int(m.count.min()) > T and older
                and (cmds & SKIP).any() and (cmds & CLEAR).any())


SEED_TRIES = 64


def seed_of(c):
    """The seed of a case: derived from its id - crc32 of the id and a counter - and chosen on the model: the first of
    SEED_TRIES candidates whose command bytes satisfy seed_ok.  None if none does (the CPU test fails then)."""
    N, _, steps = shape_of_run(c)
    for i in range(SEED_TRIES):
        seed = zlib.crc32(f"{case_id(c)}/{i}".encode())
        if seed_ok(c, commands(seed, N, steps)):
            return seed
    return None


def action_mode(seed):
    return "relative" if seed & 1 else "absolute"


def init_loc(c):
    return (min(2, c.obs[0] - c.fov[0]), min(3, c.obs[1] - c.fov[1]))


def inputs(c, seed, shape=None):
    """(cmds u8 [steps][N], frames u8 [steps][N][2][oh][ow], actions f32 [steps][N][2]).  The actions leave the frame on both
    sides and a third of them sit on exact .5 ties; in relative mode they are steps of the same kind around zero."""
    N, _, steps = shape or shape_of_run(c)
    cmds = commands(seed, N, steps)
    rng = np.random.default_rng(seed + 1000)
    frames = rng.integers(0, 256, (steps, N, 2) + c.obs, dtype=np.uint8)
    if action_mode(seed) == "absolute":
        acts = rng.uniform(-6.0, max(c.obs) + 6.0, (steps, N, 2))
    else:
        acts = rng.uniform(-12.0, 12.0, (steps, N, 2))
    flat = acts.reshape(-1, 2)
    flat[::3] = np.floor(flat[::3]) + 0.5
    return cmds, frames, acts.astype(np.float32)


def oracle_of(c, mode="absolute"):
    from oracle import oracle as O
    return O.FixedFovealOracle(c.obs, c.fov, init_loc(c), mode, resize_to_full=c.mode == "resize", mask_out=c.mode == "mask",
                               sensory_action_space=(-7.0, 9.0) if mode == "relative" else None, antialias=bool(c.aa))


def replay(c, seed, shape=None):
    """{(n, index): (stack u8 [fs][oh][ow], fov_loc (r, c) or None)} of every append of the run, from the inputs alone, as
    tests/test_gpu_glimpse.py::_oracle_memories re-derives them: a CLEAR zeroes the stack, the new frame is frame 0 or the maximum
    of the two, a skipped env keeps its stack, and every fovea call moves every env's fov_loc - skipped or not."""
    cmds, frames, acts = inputs(c, seed, shape)
    N = cmds.shape[1]
    fov = [oracle_of(c, action_mode(seed)) for _ in range(N)] if c.kind == "fixed" else None
    stack = np.zeros((N, c.fs) + c.obs, np.uint8)
    count = np.zeros(N, np.int64)
    seen = {}
    for step in range(len(cmds)):
        for n in range(N):
            b = int(cmds[step, n])
            if not b & SKIP:
                if b & CLEAR:
                    stack[n] = 0
                new = frames[step, n, 0] if (b & 3) == 1 else np.maximum(frames[step, n, 0], frames[step, n, 1])
                stack[n] = np.concatenate([stack[n, 1:], new[None]], 0)
            if fov is not None:
                fov[n].update_loc(acts[step, n])
            if not b & SKIP:
                seen[(n, int(count[n]))] = (stack[n].copy(), None if fov is None else (int(fov[n].fov_loc[0]), int(fov[n].fov_loc[1])))
                count[n] += 1
    return seen


def oracle_obs(c, stack, loc, transposed=False, flip_aa=False):
    """float64: the observation of the u8 stack with the window at loc - oracle.FixedFovealOracle.get_fov_state of
    float32(stack) / 255 widened to float64; "full": that stack itself.  transposed / flip_aa: a deliberately wrong oracle - (r, c)
    exchanged, antialias flipped - for showing that the checker tells them apart."""
    from oracle import oracle as O
    unit = O.u8_to_unit(stack).astype(np.float64)
    if c.kind == "base":
        return unit
    orc = oracle_of(c._replace(aa=1 - c.aa) if flip_aa else c)
    orc.fov_loc = np.array(loc[::-1] if transposed else loc, np.int32)
    return orc.get_fov_state(unit)


def action_loc(c, action):
    """The fov_loc of a read-time (absolute) action: the oracle's update_loc."""
    orc = oracle_of(c)
    orc.update_loc(np.asarray(action))
    return int(orc.fov_loc[0]), int(orc.fov_loc[1])


def check_obs(c, got, want):
    """One observation (float32 NumPy) against the float64 oracle's: bit-exact to float32(want) where nothing is resampled, within
    the project's FLOAT_TOL = 1e-5 (tests/test_gpu_parity.py) where it is.  Returns (ok, max abs error)."""
    if got.shape != want.shape:
        return False, float("inf")
    if c.mode == "resize":
        err = float(np.abs(got.astype(np.float64) - want).max())
        return err <= 1e-5, err
    return bool(np.array_equal(got, want.astype(np.float32))), 0.0
