"""The rule of an on-policy rollout and the float32 GAE fold (include/agx_rollout.h) in NumPy, on tests/history_model.py's
HistoryModel and tests/steplog_model.py's StepLogModel, and the scripted scenarios of the cases tests/test_gpu_rollout.py runs:
their seeds are chosen - and checked, in tests/test_rollout_cpu.py - on the model alone.  Bookkeeping only, no pixels.  Nothing
here is shared with active-gym_amd/csrc/agx_rollout_math.h."""
import numpy as np

from history_model import CLEAR, SKIP, HistoryModel
from steplog_model import F32, TERMINATED, TRUNCATED, StepLogModel

ROLLOUT_LIMIT = 4096
CUT, BOOT = 4, 8


# ---------------------------------------------------------------------------------------------- the rule
def rollout(log, n, L):
    """The live slots of env n, newest first: [(obs_index, next_index, ends)]."""
    h = log.h
    T, cnt = h.T, int(h.count[n])
    lo, slots, j = max(cnt - T, 0), [], cnt - 1
    while j > lo and len(slots) < L:
        if int(h.age[j % T, n]) == 0:                       # a reset observation: no transition
            j -= 1
            continue
        if int(log.stamp[j % T, n]) != j or not h.valid(n, j - 1):
            break
        e = int(log.flags[j % T, n]) & (TERMINATED | TRUNCATED)
        if e == 0 and j + 1 < cnt and int(h.age[(j + 1) % T, n]) == 0:
            e = CUT
        if not e & TERMINATED and (not slots or e & (TRUNCATED | CUT)):
            e |= BOOT
        slots.append((j - 1, j, e))
        j -= 1
    return slots


def gather(log, L):
    """agx_rollout_gather's outputs as a dict of arrays: len [N]; obs_index, next_index, reward, ends [L, N]; payload [L, N, W]."""
    h = log.h
    N, T = h.N, h.T
    out = dict(len=np.zeros(N, np.int32), obs_index=np.full((L, N), -1, np.int64), next_index=np.full((L, N), -1, np.int64),
               reward=np.zeros((L, N), F32), ends=np.zeros((L, N), np.uint8), payload=np.zeros((L, N, log.W), np.uint8))
    for n in range(N):
        slots = rollout(log, n, L)
        out["len"][n] = len(slots)
        for i, (a, b, e) in enumerate(slots):
            t = L - 1 - i
            out["obs_index"][t, n], out["next_index"][t, n], out["ends"][t, n] = a, b, e
            out["reward"][t, n] = log.reward[b % T, n]
            out["payload"][t, n] = log.payload[b % T, n]
    return out


def gae(length, reward, ends, value, boot, gamma, lam):
    """agx_rollout_gae in np.float32, one rounding per operation -> (adv, ret) f32 [L, N].  boot: [L, N] or None."""
    L, N = reward.shape
    gamma, lam = F32(gamma), F32(lam)
    gl = F32(gamma * lam)
    adv, ret = np.zeros((L, N), F32), np.zeros((L, N), F32)
    with np.errstate(all="ignore"):
        for n in range(N):
            A = F32(0)
            for t in range(L - 1, L - 1 - min(max(int(length[n]), 0), L), -1):
                e, v = int(ends[t, n]), F32(value[t, n])
                if e & BOOT:
                    nv = F32(boot[t, n]) if boot is not None else F32(0)
                elif e & TERMINATED or t == L - 1:
                    nv = F32(0)
                else:
                    nv = F32(value[t + 1, n])
                delta = F32(F32(F32(reward[t, n]) + F32(gamma * nv)) + F32(-v))
                carry = F32(0) if (t == L - 1 or e & 7) else F32(gl * A)
                A = F32(delta + carry)
                adv[t, n], ret[t, n] = A, F32(A + v)
    return adv, ret


def gae_vec(length, reward, ends, value, boot, gamma, lam):
    """gae() with the envs as one np.float32 array per step: the same operations in the same order, one rounding each (NumPy
    rounds every float32 array operation on its own), for the shapes a Python loop over L * N is too slow for.
    tests/test_limit_cases_cpu.py holds it bit-equal to gae() on the cases above."""
    L, N = reward.shape
    gamma, lam = F32(gamma), F32(lam)
    gl = F32(gamma * lam)
    reward, value, ends = np.asarray(reward, F32), np.asarray(value, F32), np.asarray(ends)
    first = L - np.clip(np.asarray(length, np.int64), 0, L)
    adv, ret = np.zeros((L, N), F32), np.zeros((L, N), F32)
    zero = np.zeros(N, F32)
    A = zero
    with np.errstate(all="ignore"):
        for t in range(L - 1, -1, -1):
            e, v = ends[t], value[t]
            after = zero if t == L - 1 else np.where(e & TERMINATED, zero, value[t + 1])
            nv = np.where(e & BOOT, zero if boot is None else np.asarray(boot[t], F32), after).astype(F32)
            delta = ((reward[t] + gamma * nv).astype(F32) + (-v)).astype(F32)
            carry = zero if t == L - 1 else np.where(e & 7, zero, (gl * A).astype(F32))
            A = (delta + carry).astype(F32)
            live = t >= first
            adv[t], ret[t] = np.where(live, A, zero), np.where(live, (A + v).astype(F32), zero)
            A = np.where(live, A, zero)                   # a slot that is not live is older than every live one: nothing reads this
    return adv, ret


# ---------------------------------------------------------------------------------------------- scripted scenarios
# What one env does in one scripted step.  A step is up to two pushes and one record between them:
#   STEP     push a frame, record it                                   TERM / TRUNC   ... with the end flag, then push the reset frame
#   SILENT   push a reset frame alone: nothing announced it            SKIPPED        nothing at all
#   UNREC    push a frame that is never recorded
STEP, TERM, TRUNC, SILENT, SKIPPED, UNREC = range(6)
P_KINDS = (0.66, 0.08, 0.06, 0.07, 0.07, 0.06)


def scenario(seed, N, steps, p=P_KINDS):
    """kind u8 [steps, N]; step 0 resets every env."""
    rng = np.random.default_rng(seed)
    kind = rng.choice(len(p), size=(steps, N), p=np.asarray(p) / np.sum(p)).astype(np.uint8)
    kind[0] = SILENT
    return kind


def script(kind_row, rng, W):
    """One scripted step -> (cmd_a u8 [N], recorded bool [N], reward f32 [N], flags u8 [N], payload u8 [N, W], cmd_b u8 [N] | None).
    Rewards are of mixed magnitude: normal draws scaled by 1e-3, 1 or 1e3."""
    k = np.asarray(kind_row)
    N = len(k)
    cmd_a = np.where(k == SKIPPED, SKIP | 2, np.where(k == SILENT, CLEAR | 2, 2)).astype(np.uint8)
    recorded = (k == STEP) | (k == TERM) | (k == TRUNC)
    reward = (rng.standard_normal(N) * np.array([1e-3, 1.0, 1e3])[rng.integers(0, 3, N)]).astype(F32)
    flags = np.where(k == TERM, TERMINATED, np.where(k == TRUNC, TRUNCATED, 0)).astype(np.uint8)
    payload = rng.integers(0, 256, (N, W), dtype=np.uint8)
    auto = (k == TERM) | (k == TRUNC)
    cmd_b = np.where(auto, CLEAR | 2, SKIP | 2).astype(np.uint8) if auto.any() else None
    return cmd_a, recorded, reward, flags, payload, cmd_b


def play(kind, fs, T, W, seed, clear_at=None, push=None, models=None):
    """Run a scenario on the models -> (HistoryModel, StepLogModel).  push(cmd, index_or_None, record_or_None) mirrors every push
    and record onto a device (tests/test_gpu_rollout.py); clear_at: the step in front of which the history is cleared; models: the
    pair of an earlier play to go on with."""
    steps, N = kind.shape
    hm = HistoryModel(N, fs, T) if models is None else models[0]
    lm = StepLogModel(hm, W) if models is None else models[1]
    rng = np.random.default_rng(seed + 1000)
    for s in range(steps):
        if clear_at is not None and s == clear_at:
            hm.clear()
            lm.clear()
            if push:
                push(None, None, None)
        cmd_a, recorded, reward, flags, payload, cmd_b = script(kind[s], rng, W)
        idx = hm.push(cmd_a)
        rec_idx = np.where(recorded, idx, -1).astype(np.int64)
        lm.record(rec_idx, reward, flags, payload)
        if push:
            push(cmd_a, idx, (rec_idx, reward, flags, payload))
        if cmd_b is not None:
            idx = hm.push(cmd_b)
            if push:
                push(cmd_b, idx, None)
    return hm, lm


# name: (seed, N, fs, T, steps, the case's Ls, the step in front of which the history is cleared | None, the kinds' weights)
W = 12
LONG_P = (0.90, 0.03, 0.02, 0.02, 0.02, 0.01)
CASES = {
    "small": (2, 5, 3, 16, 30, (1, 5), None, P_KINDS),
    "cleared": (2, 5, 3, 16, 24, (1, 5), 13, P_KINDS),
    "long": (6, 5, 3, 160, 190, (5, 64, 65, 130), None, LONG_P),
}


def case_models(name, push=None):
    seed, N, fs, T, steps, _, clear_at, p = CASES[name]
    kind = scenario(seed, N, steps, p)
    return (kind,) + play(kind, fs, T, W, seed, clear_at, push)


def gae_inputs(out, seed):
    """Random-normal values and boot values of mixed magnitude for a gathered rollout; the boot values are NaN where BOOT is not
    set, which must never reach an output."""
    rng = np.random.default_rng(seed)
    shape = out["reward"].shape
    value = (rng.standard_normal(shape) * np.array([1e-3, 1.0, 1e3])[rng.integers(0, 3, shape)]).astype(F32)
    boot = (rng.standard_normal(shape) * np.array([1e-3, 1.0, 1e3])[rng.integers(0, 3, shape)]).astype(F32)
    boot[(out["ends"] & BOOT) == 0] = np.nan
    return value, boot


GAMMA_LAMBDA = ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0))


def features(log, L):
    """Which of the things the GPU cases are there for a rollout of length L holds, as a set of names."""
    h, out = log.h, set()
    for n in range(h.N):
        slots = rollout(log, n, L)
        m = len(slots)
        out.add("full" if m == L else "partial" if m else "empty")
        if int(h.count[n]) > h.T:
            out.add("wrapped")
        for i, (a, b, e) in enumerate(slots):
            out |= {name for bit, name in ((CUT, "cut"), (TRUNCATED, "truncated"), (TERMINATED, "terminated")) if e & bit}
            if e & BOOT and i > 0:
                out.add("boot_inside")
            if i > 0 and slots[i - 1][0] > b:                 # the newer slot's observation is not this one's next: rows were skipped
                out.add("skipped")
    return out


FEATURES = {"full", "partial", "empty", "skipped", "cut", "truncated", "terminated", "boot_inside", "wrapped"}
