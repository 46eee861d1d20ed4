"""The scenarios of the tests that hold the replay, step-log and rollout kernels (K7, K8, K9, K11's gather, K12) at the limits
their headers state - tests/test_gpu_sampler_limits.py, tests/test_gpu_steplog_limits.py, tests/test_gpu_rollout_launch.py - and
the parts the CPU check (tests/test_limit_cases_cpu.py) shares with them: the command bytes and scripted kinds, the models after
the run, the special-float value set, and the float64 DEFINITIONS of the n-step return and of GAE, written from
include/agx_steplog.h and include/agx_rollout.h and sharing nothing with tests/steplog_model.py / tests/rollout_model.py's folds.
Every seed is chosen on the models alone; the CPU test pins what each scenario is there for.  Pure NumPy, no GPU."""
import numpy as np

import priority_model as pm
import replay_model as rm
import rollout_model as ro
import steplog_model as sm
from history_model import CLEAR, HistoryModel

F32 = np.float32
U24 = 2.0 ** -24                      # the unit roundoff of float32
TINY = 2.0 ** -100                    # the float64 checks leave out a sample with a non-zero term below this: the bounds do not model underflow

# ---------------------------------------------------------------------------------------------- span, span17 (K7, K9)
SPAN_LIMIT = 64                       # AGX_REPLAY_SPAN_LIMIT
CHUNK = 64                            # kPrioChunk: positions k - lo per workgroup of k_priority_weights
SPAN_CONFIGS = [(64, 64), (64, 0), (0, 64), (63, 1)]          # (back, forward)
# name: (N, fs, T, steps, the steps (0-based) after which a draw is made: the last one, and two while every count is below T)
SPAN = {"span": (5, 4, 320, 400, (99, 249, 399)), "span17": (17, 4, 200, 260, (259,))}
SPAN_SEED, SPAN_B, SPAN_SET_B = 1, 2048, 32768
SAMPLER_SEED = 7


def span_commands(name):
    """rm.commands(1, N, steps, p_clear = 0.006, p_skip = 0.1) with env 0 never cleared after step 0: one episode of more than 255
    appends, so its age byte and inspect's `ahead` saturate."""
    N, _, _, steps, _ = SPAN[name]
    cmds = rm.commands(SPAN_SEED, N, steps, p_clear=0.006, p_skip=0.1)
    cmds[1:, 0] &= np.uint8(0xFF ^ CLEAR)
    return cmds


def span_model(name, upto=None):
    """(cmds, model after the first `upto` steps - default: all)."""
    N, fs, T, _, _ = SPAN[name]
    cmds = span_commands(name)
    model = HistoryModel(N, fs, T)
    for cmd in cmds[:upto]:
        model.push(cmd)
    return cmds, model


def retained_rows(model):
    return [(n, k) for n in range(model.N) for k in range(max(int(model.count[n]) - model.T, 0), int(model.count[n]))]


def span_priorities(model, rng):
    """tests/test_gpu_priority.py's _update_all: every retained row, a random priority over 2^-18 .. 2^14."""
    rows = retained_rows(model)
    return rows, (2.0 ** rng.uniform(-18, 14, len(rows))).astype(F32)


def span_table(model, draw_no):
    """The table of the draw number draw_no (0 first): every row retained then gets a priority, seeded by the draw's number."""
    table = pm.Table(model)
    rows, prio = span_priorities(model, np.random.default_rng(100 + draw_no))
    pm.update(model, table, [r[0] for r in rows], [r[1] for r in rows], prio)
    return table, rows, prio


def chunk_of(model, n, k):
    """The chunk of 64 positions (k - lo_n) that k_priority_weights files row k of env n under; below lo: negative."""
    return (k - max(int(model.count[n]) - model.T, 0)) // CHUNK


def span_reach(model, back, forward):
    """What the accepted set of (back, forward) holds: its size, the candidates' number, how many members' `back` window starts in
    an earlier chunk, how many look at age[k + forward] in a later chunk, and how many have a saturated age."""
    acc = rm.accepted_set(model, back, forward)
    _, L, _ = rm.candidates(model, forward)
    behind = sum(chunk_of(model, n, k - min(back, rm.age(model, n, k))) < chunk_of(model, n, k) for n, k in acc)
    ahead = sum(chunk_of(model, n, k + forward) > chunk_of(model, n, k) for n, k in acc)
    saturated = sum(rm.age(model, n, k) == 255 for n, k in acc)
    return dict(accepted=len(acc), candidates=sum(L), behind=behind, ahead=ahead, saturated=saturated)


# ---------------------------------------------------------------------------------------------- deepfold, deeproll (K8, K11, K12)
OBS, FOV, FS = (10, 12), (3, 5), 3    # the small run-time geometry the rollout tests use
NSTEP_LIMIT = 64                      # AGX_STEPLOG_NSTEP_LIMIT
PAYLOAD_LIMIT = 64                    # AGX_STEPLOG_PAYLOAD_LIMIT
WIDTHS = (4, 64)                      # the payload widths of the logs of one deepfold run
WIDTH_LS = (5, 160)                   # the rollout lengths the payload test gathers at: every env full, every env padded
# kinds' weights (rollout_model's STEP, TERM, TRUNC, SILENT, SKIPPED, UNREC): ends rare enough for 64 clean rows in a row
DEEP_P = (0.982, 0.004, 0.003, 0.004, 0.004, 0.003)
ROLL_P = (0.92, 0.03, 0.02, 0.015, 0.014, 0.001)
# name: (seed, N, T, steps, weights)
DEEP = {"deepfold": (0, 5, 160, 200, DEEP_P), "deeproll": (0, 9, 1100, 1200, ROLL_P), "wide": (4, 257, 16, 24, ro.P_KINDS)}

# The special rewards of the second log: signed zeros, the smallest subnormal and the smallest normal, the largest finite
# magnitudes, infinities, NaN - and ordinary normals in between (half of all draws).
SPECIAL = np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126, -2.0 ** -126, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan], F32)
SPECIAL_GAMMA = 2.0 ** -3             # gamma ** m is subnormal for m = 43 .. 49 and 0 from m = 50 on
SPECIAL_GAMMAS = (SPECIAL_GAMMA, 1.0)  # ... and undiscounted: two rewards of 3.4e38 in one fold overflow to inf
SPECIAL_SEED = 9


def special_values(rng, shape, p_special=0.5):
    """float32 values of `shape`: about p_special of them from SPECIAL, the rest normal draws of mixed magnitude."""
    normal = (rng.standard_normal(shape) * np.array([1e-3, 1.0, 1e3])[rng.integers(0, 3, shape)]).astype(F32)
    pick = SPECIAL[rng.integers(0, len(SPECIAL), shape)]
    return np.where(rng.random(shape) < p_special, pick, normal).astype(F32)


def special_rewards(rng, N):
    """The special log's rewards of one step: mostly tiny and zero values - so that subnormal sums survive for many rows - with the
    occasional huge, infinite or NaN one."""
    small, huge, u = SPECIAL[rng.integers(0, 6, N)], SPECIAL[rng.integers(6, 8, N)], rng.random(N)
    return np.where(u < 0.90, small, np.where(u < 0.95, huge, special_values(rng, N, 0.7))).astype(F32)


class Deep:
    """One scripted run (rollout_model's kinds and script) on the models: the history, a log per payload width of WIDTHS - the same
    rows, rewards and flags, the payload of width W being the first W of the step's 64 random bytes - and the special log
    (W = 0): the same rows and flags with special_rewards.  `device`, if given, mirrors every call: device.clear(),
    device.push(cmd, index) and device.record(index, reward, flags, payload64, special_reward)."""

    def __init__(self, name, device=None, N=None):
        seed, full_N, T, steps, p = DEEP[name]
        N = full_N if N is None else N
        self.name, self.N, self.T = name, N, T
        self.kind = ro.scenario(seed, full_N, steps, p)[:, :N]      # the first N envs of the one scripted run
        self.hm = HistoryModel(N, FS, T)
        self.logs = {W: sm.StepLogModel(self.hm, W) for W in WIDTHS}
        self.special = sm.StepLogModel(self.hm, 0)
        self.rows = {}                # (n, j) -> (reward f32, flags): what was recorded, kept apart from the models
        rng, srng = np.random.default_rng(seed + 1000), np.random.default_rng(SPECIAL_SEED + 77)
        for s in range(steps):
            cmd_a, recorded, reward, flags, payload, cmd_b = ro.script(self.kind[s], rng, PAYLOAD_LIMIT)
            idx = self.hm.push(cmd_a)
            if device:
                device.push(cmd_a, idx)
            rec = np.where(recorded, idx, -1).astype(np.int64)
            special = special_rewards(srng, N)
            for W, lm in self.logs.items():
                lm.record(rec, reward, flags, payload[:, :W])
            self.special.record(rec, special, flags)
            for n in np.nonzero(rec >= 0)[0]:
                self.rows[(int(n), int(rec[n]))] = (reward[n], int(flags[n]))
            if device:
                device.record(rec, reward, flags, payload, special)
            if cmd_b is not None:
                idx = self.hm.push(cmd_b)
                if device:
                    device.push(cmd_b, idx)

    def samples(self):
        """Every (n, k), k in [-1, cnt], env-major: 64 consecutive ones are one wave of k_steplog_gather."""
        return [(n, k) for n in range(self.N) for k in range(-1, int(self.hm.count[n]) + 1)]


def stop_reason(hm, lm, n, k, nstep):
    """(m, why) of the walk of sample (n, k): why the fold stopped behind m rows - "invalid" (the sample itself is not retained),
    "nstep", "history" (its end), "age0" (another episode), "unrecorded" or "flag" - from the header's stop rules."""
    cnt = int(hm.count[n]) if 0 <= n < hm.N else 0
    if not (0 <= n < hm.N and 0 <= k < cnt and k >= cnt - hm.T):
        return 0, "invalid"
    for i in range(1, nstep + 1):
        j = k + i
        if j >= cnt:
            return i - 1, "history"
        if hm.age[j % hm.T, n] == 0:
            return i - 1, "age0"
        if lm.stamp[j % hm.T, n] != j:
            return i - 1, "unrecorded"
        if lm.flags[j % hm.T, n] & (sm.TERMINATED | sm.TRUNCATED):
            return i, "flag"
    return nstep, "nstep"


def gather_table(hm, lm, nstep, gamma):
    """StepLogModel.gather of every (n, k), 0 <= k < cnt, as per-env arrays indexed by k - for the composition of a sequence's
    steps: dict of lists over n of steps i32, next_index i64, ret f32, discount f32, flags u8, payload u8 [cnt, W]; zeros, and
    next_index -1, where nothing was folded (what agx_sequence_gather writes there)."""
    out = {key: [] for key in ("steps", "next_index", "ret", "discount", "flags", "payload")}
    for n in range(hm.N):
        cnt = int(hm.count[n])
        t = dict(steps=np.zeros(cnt, np.int32), next_index=np.full(cnt, -1, np.int64), ret=np.zeros(cnt, F32), discount=np.zeros(cnt, F32),
                 flags=np.zeros(cnt, np.uint8), payload=np.zeros((cnt, lm.W), np.uint8))
        for k in range(cnt):
            m, nxt, G, disc, last, pay = lm.gather(n, k, nstep, gamma)
            if m:
                t["steps"][k], t["next_index"][k], t["ret"][k], t["discount"][k], t["flags"][k], t["payload"][k] = m, nxt, G, disc, last, pay
        for key in out:
            out[key].append(t[key])
    return out


# ---------------------------------------------------------------------------------------------- the n-step return, in float64
def nstep_definition(rows, n, k, m, gamma):
    """include/agx_steplog.h's DEFINITION of a sample that folded m >= 1 rows, in float64 from the recorded rewards themselves:
    ret = sum_{i = 1 .. m} g^(i - 1) r_i and discount = g^m (0 behind TERMINATED), g = float64(float32(gamma)), with the sum of the
    terms' magnitudes and the smallest non-zero one -> (ret, discount, terminated, S, smallest)."""
    g = float(F32(gamma))
    ret, S, smallest, p = 0.0, 0.0, np.inf, 1.0
    for i in range(1, m + 1):
        r, fl = rows[(n, k + i)]
        term = p * float(r)
        ret += term
        S += abs(term)
        if term != 0.0:
            smallest = min(smallest, abs(term))
        p *= g
    return ret, p, bool(fl & sm.TERMINATED), S, smallest


def nstep_bounds(m, S, gm):
    """The error bounds of a float32 fold of m terms against the float64 definition.

    ret: term i is fl(disc_{i-1} * r_i), where disc_{i-1} = fl(fl(..fl(1 * g)..) * g) carries i - 1 roundings (the product by 1 is
    exact), one more for the product with r_i, and the partial sums it then passes through add m - i + 1 roundings: at most
    (i - 1) + 1 + (m - i + 1) = m + 1 <= 2 m relative errors of at most u = 2^-24 each, so, to first order in u,
    |ret32 - ret| <= 2 m u sum_i |g^(i-1) r_i|.  (The second-order term is below (2 m u)^2 / 2 < 3e-11 of that at m = 64.)
    discount: m products by g, m roundings: |disc32 - g^m| <= m u g^m.  g itself is exact: the definition uses float32(gamma)."""
    return 2 * m * U24 * S, m * U24 * gm


# ---------------------------------------------------------------------------------------------- GAE: inputs, and the definition
def gae_lengths(rng, N, L):
    """len i32 [N]: random in [0, L], with the wild values of the existing test (-3, L + 7, 0, L, 1) on the first envs."""
    length = rng.integers(0, L + 1, N).astype(np.int32)
    wild = np.array([-3, L + 7, 0, L, 1], np.int32)[:N]
    length[:len(wild)] = wild
    if N > 6:
        length[-1] = L                                   # the last lane of the last block folds every slot
    return length


def gae_case(N, L, seed, special=False):
    """Synthetic inputs of agx_rollout_gae: len (gae_lengths), ends random over the legal bytes - 0, TERMINATED, and BOOT alone
    or with TRUNCATED or CUT - reward / value / boot random normal of mixed magnitude (special: from special_values), and NaN
    where a value must not reach an output: boot where BOOT is not set, reward / value of the slots that are not live (the
    kernel folds those and must write 0).  -> (len, reward, ends, value, boot, live)."""
    rng = np.random.default_rng(seed)
    length = gae_lengths(rng, N, L)
    legal = np.array([0, 0, 0, 0, 0, sm.TERMINATED, ro.BOOT, ro.BOOT | sm.TRUNCATED, ro.BOOT | ro.CUT], np.uint8)
    ends = legal[rng.integers(0, len(legal), (L, N))]

    def draw():
        if special:
            return special_values(rng, (L, N))
        return (rng.standard_normal((L, N)) * np.array([1e-3, 1.0, 1e3])[rng.integers(0, 3, (L, N))]).astype(F32)

    reward, value, boot = draw(), draw(), draw()
    live = np.arange(L)[:, None] >= L - np.clip(length, 0, L)[None, :]
    boot[(ends & ro.BOOT) == 0] = np.nan
    reward[~live] = np.nan
    value[~live] = np.nan
    return length, reward, ends, value, boot, live


def gae_definition(length, reward, ends, value, boot, gamma, lam):
    """include/agx_rollout.h's definition of the advantage in float64, vectorised over the envs: for a live slot t,
    adv_t = sum_l (g lam)^l delta_(t+l) over the chain from t up to the first slot with an episode break (ends & 7) or t = L - 1,
    delta_t = r_t + g nv_t - v_t, nv_t = boot_t (BOOT), 0 (TERMINATED, or t = L - 1 without BOOT), else v_(t+1); g and lam are
    float64(float32(.)) and g lam is their exact product.  -> (adv f64 [L, N], S: the sum of the magnitudes of every term that
    enters adv_t, chain: the number of slots in the sum, smallest: the smallest non-zero term's magnitude, live bool [L, N])."""
    L, N = reward.shape
    g, gl = float(F32(gamma)), float(F32(gamma)) * float(F32(lam))
    live = np.arange(L)[:, None] >= L - np.clip(np.asarray(length, np.int64), 0, L)[None, :]
    r, v = np.where(live, reward, 0).astype(np.float64), np.where(live, value, 0).astype(np.float64)
    b = np.zeros((L, N)) if boot is None else np.where(ends & ro.BOOT, boot, 0).astype(np.float64)
    adv, S, chain, smallest = (np.zeros((L, N)) for _ in range(4))
    A, SS, C, M = np.zeros(N), np.zeros(N), np.zeros(N), np.full(N, np.inf)
    with np.errstate(all="ignore"):
        for t in range(L - 1, -1, -1):
            e = ends[t]
            nv = np.where(e & ro.BOOT, b[t], np.where((e & sm.TERMINATED) | (t == L - 1), 0.0, v[t + 1] if t < L - 1 else 0.0))
            terms = np.stack([r[t], g * nv, -v[t]])
            brk = ((e & 7) != 0) | (t == L - 1)
            mag = np.abs(terms)
            low = np.where(mag > 0, mag, np.inf).min(0)
            A = terms.sum(0) + np.where(brk, 0.0, gl * A)
            SS = mag.sum(0) + np.where(brk, 0.0, gl * SS)
            M = np.minimum(low, np.where(brk | (gl == 0.0) | np.isinf(M), np.inf, gl * np.where(np.isinf(M), 0.0, M)))
            C = 1 + np.where(brk, 0, C)
            adv[t], S[t], chain[t], smallest[t] = A, SS, C, M
    return adv, S, chain, smallest, live


def gae_bound(S, chain):
    """|adv32 - adv| <= k u S with k = 4 chain + 4 and u = 2^-24.

    A term of delta_(t+l) - r, g nv or v - is formed with at most one rounding (the product g nv), passes the two additions of
    its delta (two roundings) and the addition of the carry (one), and is then multiplied by fl(g lam) - itself one rounding off
    g lam - and added to the next delta once per slot it is carried over: three relative errors per carried slot, l of them.
    That is at most 4 + 3 l <= 4 (l + 1) <= 4 chain + 4 factors (1 + d), |d| <= u, on a term of magnitude (g lam)^l |x|; summed over
    the terms, to first order in u, the error is at most (4 chain + 4) u S."""
    return (4 * chain + 4) * U24 * S
