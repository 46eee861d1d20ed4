"""The length rule of a sequence (include/agx_sequence.h) in Python ints, on tests/history_model.py's HistoryModel, and the
command bytes of the cases tests/test_gpu_sequence.py runs: their seeds are chosen - and checked, in tests/test_sequence_cpu.py -
on the model alone.  Bookkeeping only, no pixels."""
import numpy as np

from history_model import CLEAR, SKIP, HistoryModel

SEQUENCE_LIMIT = 256


def length(model, n, k, L):
    """len of the sequence (n, k, L): 0 for a start that is not valid, else 1 + the largest f <= L - 1 with k + f < count[n] and
    no age == 0 row in (k, k + f]."""
    if not model.valid(n, k):
        return 0
    cnt, f = int(model.count[n]), 0
    while f < L - 1 and k + f + 1 < cnt and int(model.age[(k + f + 1) % model.T, n]) != 0:
        f += 1
    return 1 + f


def kind(model, n, k, L):
    """What ends the sequence: "zero" (an invalid start), "full" (L live steps), "end" (the end of the history) or "episode" (the
    first append of another episode)."""
    m = length(model, n, k, L)
    if m == 0:
        return "zero"
    if m == L:
        return "full"
    return "end" if k + m >= int(model.count[n]) else "episode"


def starts(model, outside=True):
    """Every (n, k), k in [-1, count[n]], plus - outside - the envs -1 and N."""
    out = [(n, k) for n in range(model.N) for k in range(-1, int(model.count[n]) + 1)]
    return out + [(-1, 0), (model.N, 0), (-1, 3), (model.N, 1)] if outside else out


def kinds(model, L, samples=None):
    """{kind: how many of the samples (default: starts(model)) end that way}."""
    out = {"zero": 0, "full": 0, "end": 0, "episode": 0}
    for n, k in starts(model) if samples is None else samples:
        out[kind(model, n, k, L)] += 1
    return out


def commands(seed, N, steps, p_clear=0.15, p_skip=0.15):
    """tests/test_gpu_history.py's commands(), restated so that the CPU tests need no torch: the same draws in the same order."""
    rng = np.random.default_rng(seed)
    cmd = rng.integers(1, 3, (steps, N)).astype(np.uint8)
    cmd |= (rng.random((steps, N)) < p_clear).astype(np.uint8) * CLEAR
    cmd |= (rng.random((steps, N)) < p_skip).astype(np.uint8) * SKIP
    return cmd


# ---------------------------------------------------------------------------------------------- the GPU cases
# name: (seed, N, fs, T, steps, the largest L the case asks for)
CASES = {
    "main": (3, 5, 4, 16, 25, 8),
    "dtype": (5, 3, 4, 8, 12, 5),
    "geometry": (11, 4, 3, 6, 11, 4),
    "base": (8, 4, 3, 6, 11, 4),
    "graph": (7, 5, 4, 16, 25, 6),
}


def case_model(name):
    """(cmds, model after the case's pushes)."""
    seed, N, fs, T, steps, _ = CASES[name]
    cmds = commands(seed, N, steps)
    model = HistoryModel(N, fs, T)
    for cmd in cmds:
        model.push(cmd)
    return cmds, model


# The L > 64 case: N = 2, T = 320, 300 appends, no SKIP.  Env 0 starts episodes at 0, 70 and 198, env 1 at 0 alone, so from
# the starts below the sequences run 64, 65, 70, 128 and 256 steps (and 102 to the end of the history).
LONG_N, LONG_FS, LONG_T, LONG_STEPS = 2, 2, 320, 300
LONG_CLEARS = {0: (0, 70, 198), 1: (0,)}
LONG_LS = (64, 65, 70, 128, 256)
LONG_WITNESS = {(0, 6): 64, (0, 5): 65, (0, 0): 70, (0, 70): 128, (1, 0): 256, (1, 44): 256, (0, 198): 102, (1, 45): 255}      # at L = 256


def long_commands():
    cmd = np.full((LONG_STEPS, LONG_N), 2, np.uint8)
    for n, at in LONG_CLEARS.items():
        cmd[list(at), n] |= CLEAR
    return cmd
