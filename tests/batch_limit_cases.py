"""The scenarios that take the minibatch (K15), Retrace (K16) and chunk (K17) kernels to the limits their headers state, and a
SECOND writing of each definition to hold them against.  tests/test_batch_limits_cpu.py pins on the models alone what every
scenario holds; tests/test_gpu_minibatch_limits.py, tests/test_gpu_chunks_limits.py and tests/test_gpu_retrace_limits.py run them
on the device.  Every case is made once per process and handed out read-only.  Pure NumPy.

THE LISTS AND THE PERMUTATION, vectorised (Minibatches, Chunks).  Written from include/agx_minibatch.h and include/agx_chunks.h;
nothing is shared with csrc/agx_minibatch_math.h and nothing with tests/minibatch_model.py / tests/chunks_model.py beyond the
constants.  mix, SM and the six Feistel rounds run on uint64 arrays (which wrap modulo 2^64 by themselves), cycle walking iterates
over the positions that are not below total yet and counts each position's rounds.  A list is np.nonzero of the rule, transposed
to env-major - not offsets plus a search - and every per-step output of a chunk take comes by broadcasting over [C][S].

THE Q-RETURN, as the papers write it (definition): in float64, for every step l with a row,

    T[l] = q[l] + sum over j >= l of P(l, j) delta[j],   P(l, j) = prod over i = l + 1 .. j of discount[i - 1] c[i],
    delta[j] = reward[j] + discount[j] vnext[j] - q[j],  vnext[j] = (j + 1 < len') ? v[j + 1] : boot,

the sum stopping in front of the first j + 1 without a row.  The header's recursion is never written here.

THE BOUND of float32 against that sum is derived, not measured.  With u = 2^-24, every fadd / fsub / fmul of the fold returns
its exact result times (1 + e), |e| <= u (no operation of the cases underflows: see below).  Expanding the header's fold, T[l] is
the sum over j of P(l, j) (reward[j] + discount[j] vnext[j]) minus, for j > l, P(l, j) q[j].  A term of step j, k = j - l steps
up the chain, passes at its own step at most 3 roundings (fadd(vnext, carry), the product with discount, the sum with reward) and
at each of the k steps below it 5 (fsub(T, q), the product with c, and those three): at most 5 k + 3.  So

    |T32[l] - T[l]| <= sum over j of g(5 (j - l) + 3) |P(l, j)| (|reward[j]| + |discount[j] vnext[j]| + |q[j]|),  g(k) = k u / (1 - k u)

(the standard bound on (1 + e_1) .. (1 + e_k) - 1), and td = fsub(T, q[l]) adds one rounding to every term and |q[l]| to the sum:
g(5 (j - l) + 4).  The bound is therefore in units of 2^-24 times the ABSOLUTE sums the coefficients multiply, which is what a
cancelling sum needs.  The float64 sum itself is off by some 2^-53 times the same absolute sums: u is taken as 2^-24 + 2^-40 to
cover it.  Underflow is outside this model, so a step whose chain holds a non-zero term below 2^-100 would be left out of the
comparison; the cases (ordinary normals, |c| <= 1, discount 0.99 or 0, chains cut by steps without a row) leave NONE out, and
the CPU test asserts that on the float32 model alone.
"""
import functools

import numpy as np

import chunks_model as cm
import minibatch_model as mm
import retrace_model as rm

U64 = np.uint64
F32 = np.float32
INT32_MAX = 2 ** 31 - 1
GOLD, MUL_A, MUL_B = U64(mm.GOLD), U64(0xBF58476D1CE4E5B9), U64(0x94D049BB133111EB)
LIVE, BOOT = mm.LIVE, mm.BOOT


# ---------------------------------------------------------------------------------------------- the permutation, on arrays
def mix(z):
    """splitmix64's finaliser on a uint64 array."""
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * MUL_A
        z = (z ^ (z >> U64(27))) * MUL_B
    return z ^ (z >> U64(31))


def sm(s, i):
    """SM(s, i) -> uint64 [1]."""
    with np.errstate(over="ignore"):
        return mix(np.array([s], U64).reshape(1) + np.array([i + 1], U64) * GOLD)


def half_bits(total):
    """hb: the least h >= 1 with 4^h >= total, which is max(1, ceil(bitlen(total - 1) / 2))."""
    hb = 1
    while (1 << (2 * hb)) < total:
        hb += 1
    return hb


def permutation(ek, total, m):
    """perm(m) of every position of the array m under the key ek (uint64 [1]) -> (i64 like m, the rounds each position walked)."""
    hb = half_bits(total)
    shift, mask, bound = U64(hb), U64((1 << hb) - 1), U64(total)
    with np.errstate(over="ignore"):
        keys = [ek + U64(i + 1) * GOLD for i in range(mm.ROUNDS)]
    x = np.asarray(m).astype(U64).reshape(-1).copy()
    walks = np.zeros(x.size, np.int32)
    todo = np.arange(x.size)
    while todo.size:
        v = x[todo]
        left, right = v >> shift, v & mask
        for k in keys:
            with np.errstate(over="ignore"):
                left, right = right, left ^ (mix(k + right) & mask)
        v = (left << shift) | right
        x[todo] = v
        walks[todo] += 1
        todo = todo[v >= bound]
    return x.astype(np.int64).reshape(np.shape(m)), walks.reshape(np.shape(m))


def _positions(key, total, permute, first, S):
    """(p, m, walks) of the rows of a take: p = first + row, m = p mod total, through the permutation where asked."""
    p = first + np.arange(S, dtype=np.int64)
    m = p % total
    if permute:
        m, walks = permutation(key, total, m)
    else:
        walks = np.zeros(S, np.int32)
    return p, m, walks


# ---------------------------------------------------------------------------------------------- the minibatcher, on arrays
class Minibatches:
    """agx_minibatch: select keeps THE LIST itself (slot elements and envs in list order), take indexes it."""

    def __init__(self, N, seed):
        self.N = N
        self.base = [sm(seed & mm.M64, w) for w in (LIVE, BOOT)]
        self.calls = [0, 0]
        self.key = [None, None]
        self.slots = [np.zeros(0, np.int64), np.zeros(0, np.int64)]
        self.envs = [np.zeros(0, np.int64), np.zeros(0, np.int64)]

    def select(self, which, length, ends, L):
        t0 = L - np.clip(np.asarray(length, np.int64), 0, L)
        rule = np.arange(L)[None, :] >= t0[:, None]                       # [N, L]: env-major
        if which == BOOT:
            rule = rule & ((np.asarray(ends).T & mm.BOOT_BIT) != 0)
        n, t = np.nonzero(rule)                                          # row-major: env by env, ascending t
        self.slots[which], self.envs[which] = t * self.N + n, n
        self.key[which] = sm(self.base[which], self.calls[which])
        self.calls[which] += 1
        return int(n.size)

    def total(self, which):
        return int(self.slots[which].size)

    def take(self, which, permute, first, S, obs_index=None, next_index=None, payload=None, streams=()):
        """-> dict of slot, env, valid, obs_index, next_index, payload [S, W], streams (a list of f32 [S]) and walks."""
        total = self.total(which)
        W = 0 if payload is None else payload.shape[-1]
        out = dict(slot=np.full(S, -1, np.int32), env=np.zeros(S, np.int32), valid=np.zeros(S, np.uint8), obs_index=np.full(S, -1, np.int64),
                   next_index=np.full(S, -1, np.int64), payload=np.zeros((S, W), np.uint8), streams=[np.zeros(S, F32) for _ in streams],
                   walks=np.zeros(S, np.int32))
        if total == 0:
            return out
        p, m, out["walks"] = _positions(self.key[which], total, permute, first, S)
        e = self.slots[which][m]
        out["slot"], out["env"], out["valid"] = e.astype(np.int32), self.envs[which][m].astype(np.int32), (p < total).astype(np.uint8)
        if obs_index is not None:
            out["obs_index"] = obs_index.reshape(-1)[e]
        if next_index is not None:
            out["next_index"] = next_index.reshape(-1)[e]
        if W:
            out["payload"] = payload.reshape(-1, W)[e]
        out["streams"] = [src.reshape(-1)[e] for src in streams]
        return out


# ---------------------------------------------------------------------------------------------- the chunker, on arrays
class Chunks:
    """agx_chunks: select keeps the (n, g) pairs in list order, take broadcasts every per-step output over [C][S]."""

    def __init__(self, N, seed):
        self.N = N
        self.base = sm(seed & mm.M64, cm.LIST)
        self.calls = 0
        self.key = None
        self.n = self.g = self.t0 = np.zeros(0, np.int64)
        self.seen = (0, 0)

    def select(self, length, L, C):
        live = np.clip(np.asarray(length, np.int64), 0, L)
        t0, G = L - live, -(-L // C)
        holds = (np.arange(G)[None, :] >= (t0 // C)[:, None]) & (live > 0)[:, None]      # [N, G]: g from t0 // C to G - 1
        self.n, self.g = np.nonzero(holds)
        self.t0, self.seen = t0, (L, C)
        self.key = sm(self.base, self.calls)
        self.calls += 1
        return int(self.n.size)

    def total(self):
        return int(self.n.size)

    def take(self, permute, ends, L, C, first, S, obs_index=None, next_index=None, payload=None, streams=()):
        N, total = self.N, self.total()
        W = 0 if payload is None else payload.shape[-1]
        out = dict(slot=np.full((C, S), -1, np.int32), env=np.zeros((C, S), np.int32), obs_index=np.full((C, S), -1, np.int64),
                   next_index=np.full((C, S), -1, np.int64), payload=np.zeros((C, S, W), np.uint8), ends=np.zeros((C, S), np.uint8),
                   start=np.zeros((C, S), np.uint8), mask=np.zeros((C, S), np.uint8), streams=[np.zeros((C, S), F32) for _ in streams],
                   chunk=np.full(S, -1, np.int32), first=np.zeros(S, np.int32), steps=np.zeros(S, np.int32), state_index=np.full(S, -1, np.int64),
                   valid=np.zeros(S, np.uint8), walks=np.zeros(S, np.int32))
        if total == 0 or self.seen != (L, C):
            return out
        p, m, out["walks"] = _positions(self.key, total, permute, first, S)
        n, g = self.n[m], self.g[m]                                       # [S]
        t0 = self.t0[n]
        t = g[None, :] * C + np.arange(C)[:, None]                        # [C, S]
        live = (t >= t0[None, :]) & (t < L)
        e = np.where(live, t, 0) * N + n[None, :]                         # a slot element wherever live; element n elsewhere (never shown)
        valid = p < total
        lead = np.maximum(t0 - g * C, 0)
        flat_ends = np.asarray(ends).reshape(-1)
        behind = np.where(live & (t > t0[None, :]), t - 1, 0) * N + n[None, :]
        restart = live & (t > t0[None, :]) & ((flat_ends[behind] & cm.BREAK) != 0)
        out["slot"] = np.where(live, e, -1).astype(np.int32)
        out["env"] = np.broadcast_to(n[None, :], (C, S)).astype(np.int32)
        out["ends"] = np.where(live, flat_ends[e], 0).astype(np.uint8)
        out["start"] = (np.where(live & (np.arange(C)[:, None] == lead[None, :]), cm.START_CHUNK, 0) | np.where(restart, cm.START_EPISODE, 0)).astype(np.uint8)
        out["mask"] = (live & valid[None, :]).astype(np.uint8)
        out["chunk"], out["first"], out["steps"] = g.astype(np.int32), lead.astype(np.int32), live.sum(0).astype(np.int32)
        out["valid"] = valid.astype(np.uint8)
        if obs_index is not None:
            out["obs_index"] = np.where(live, obs_index.reshape(-1)[e], -1)
            out["state_index"] = obs_index.reshape(-1)[(g * C + lead) * N + n]
        if next_index is not None:
            out["next_index"] = np.where(live, next_index.reshape(-1)[e], -1)
        if W:
            out["payload"] = np.where(live[:, :, None], payload.reshape(-1, W)[e], 0).astype(np.uint8)
        out["streams"] = [np.where(live, src.reshape(-1)[e], F32(0)).astype(F32) for src in streams]
        return out


# ---------------------------------------------------------------------------------------------- rollouts
def _frozen(a):
    for v in a.values():
        for x in (v if isinstance(v, list) else [v]):
            if isinstance(x, np.ndarray):
                x.flags.writeable = False
    return a


def _rollout(seed, N, L, length, W=12, n_f32=8):
    """The arrays of a gathered rollout around a given len: ends is random over 0 .. 15 (as minibatch_model.rollout_arrays), BREAK
    bits inside live runs included; the f32 streams hold NaN / inf at the slots that are not live (as chunks_model.rollout_arrays);
    the indices and the payload are random."""
    rng = np.random.default_rng(seed)
    length = np.asarray(length, np.int32)
    ends = rng.integers(0, 16, (L, N)).astype(np.uint8)
    live = np.arange(L)[:, None] >= L - np.clip(length, 0, L)[None, :]
    streams = []
    for k in range(n_f32):
        s = rng.standard_normal((L, N)).astype(F32)
        s[~live] = (np.nan, np.inf, -np.inf)[k % 3]
        streams.append(s)
    return dict(len=length, ends=ends, obs_index=rng.integers(0, 1 << 40, (L, N)).astype(np.int64),
                next_index=rng.integers(0, 1 << 40, (L, N)).astype(np.int64), payload=rng.integers(0, 256, (L, N, W), dtype=np.uint8), streams=streams)


# scan: more than one run of 256 envs in k_mb_scan / k_chunk_scan, at L = 5
SCAN_NS = (255, 256, 257, 512, 513, 1025)
SCAN_VARIANTS = ("live", "dead", "full")
SCAN_L = 5


def scan_zero_runs(N, variant):
    """The [from, to) env ranges of `scan` whose len is 0 by construction.  "live": envs 0 and N - 1 are live, "dead": they are
    not.  From N = 512 on envs 128 .. 383 are a run of 256 across the first run boundary of the scan; from N = 513 on a second
    run of 256 ends at the last env ("dead") or in front of it ("live")."""
    runs = []
    if variant == "full":
        return runs
    if N >= 512:
        runs.append((128, 384))
    if N >= 513:
        runs.append((N - 256, N) if variant == "dead" else (N - 257, N - 1))
    if variant == "dead":
        runs += [(0, 1), (N - 1, N)]
    return runs


@functools.lru_cache(maxsize=None)
def scan(N, variant):
    rng = np.random.default_rng(7000 + N * 3 + SCAN_VARIANTS.index(variant))
    L = SCAN_L
    if variant == "full":
        length = np.full(N, L, np.int32)
    else:
        length = rng.integers(1, L + 1, N).astype(np.int32)
        length[rng.random(N) < 0.2] = 0
        length[0] = length[N - 1] = L - 1
        length[1], length[N - 2] = L + 3, 1                     # (clamped)
        for a, b in scan_zero_runs(N, variant):
            length[a:b] = 0
        if variant == "dead":
            length[N - 1] = -2                                    # (clamped)
    return _frozen(_rollout(7100 + N, N, L, length, n_f32=2))


# deep: L = AGX_MB_LIMIT
DEEP = ((65, 4096), (257, 4096))
DEEP_TOP, DEEP_BOTTOM = 2, 5                 # the envs whose only BOOT bit sits at t = 0 / at t = L - 1


@functools.lru_cache(maxsize=None)
def deep(N, L):
    rng = np.random.default_rng(7200 + N)
    length = rng.integers(0, L + 1, N).astype(np.int32)
    length[rng.random(N) < 0.2] = 0
    length[rng.random(N) < 0.4] = L
    length[[DEEP_TOP, DEEP_BOTTOM]] = L
    a = _rollout(7300 + N, N, L, length, n_f32=2)
    a["ends"][:, [DEEP_TOP, DEEP_BOTTOM]] &= 7
    a["ends"][0, DEEP_TOP] |= 8                                   # the longest column walk ends here: position off[n] walks L slots ...
    a["ends"][L - 1, DEEP_BOTTOM] |= 8                            # ... and the shortest list of a full column is the last slot alone
    return _frozen(a)


# totals: the LIVE total is exactly this, at (N, L)
TOTALS = {1: (3, 2), 2: (3, 2), 3: (3, 2), 4: (3, 2), 5: (3, 2), 16: (5, 5), 17: (5, 5), 4097: (65, 64), 65537: (257, 256), 2 ** 20: (257, 4096),
          2 ** 20 + 1: (257, 4096)}
TOTALS_HB = {1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 16: 2, 17: 3, 4097: 7, 65537: 9, 2 ** 20: 10, 2 ** 20 + 1: 11}


@functools.lru_cache(maxsize=None)
def totals(total):
    """len fills envs from the last one down with L, the remainder goes to the env in front of them, every other env stays 0."""
    N, L = TOTALS[total]
    length = np.zeros(N, np.int32)
    full, rest = divmod(total, L)
    assert full + (rest > 0) <= N
    if full:
        length[N - full:] = L
    if rest:
        length[N - full - 1] = rest
    assert int(np.clip(length, 0, L).sum()) == total
    return _frozen(_rollout(7400 + total % 1000, N, L, length, n_f32=1))


# chunky: the chunk limits
CHUNKY = ((256, 256), (257, 256), (4096, 256), (4096, 255), (4096, 1), (4095, 256))
CHUNKY_NS = (5, 257)


def chunky_t0(L, C):
    """The t0 of envs 0 .. 3: 0, the first step of a chunk behind the first one (where there is one), the last step of the chunk
    in front of that one, L - 1."""
    G = -(-L // C)
    k = G // 2
    return (0, k * C, min(max(k - 1, 0) * C + C - 1, L - 1), L - 1)


@functools.lru_cache(maxsize=None)
def chunky(N, L, C):
    rng = np.random.default_rng(7500 + N + L * 7 + C)
    length = rng.integers(0, L + 1, N).astype(np.int32)
    length[rng.random(N) < 0.2] = 0
    length[rng.random(N) < 0.2] = L
    length[:4] = [L - t0 for t0 in chunky_t0(L, C)]
    length[4] = 0
    a = _rollout(7600 + N + L, N, L, length, n_f32=8 if N * L < 100000 else 2)
    a["ends"][rng.random((L, N)) < 0.5] &= 8                      # (episodes a few steps long, not one step)
    return _frozen(a)


# bytes / far / small: a mid-sized rollout
MID = (65, 37)
BYTE_WIDTHS = (1, 3, 5, 6, 66, 260)
BYTE_SHIFTS = ((4, 1, 0), (4, 0, 2), (4, 1, 2), (12, 1, 0), (12, 0, 2), (12, 1, 2))          # (W, input offset, output offset) in bytes
FAR_SIZES = (1, 64, 300)


@functools.lru_cache(maxsize=None)
def mid(W=12):
    N, L = MID
    rng = np.random.default_rng(7700)
    length = rng.integers(0, L + 1, N).astype(np.int32)
    length[rng.random(N) < 0.25] = 0
    length[rng.random(N) < 0.25] = L
    length[1], length[3] = -2, L + 3
    return _frozen(_rollout(7800 + W, N, L, length, W=W, n_f32=2))


# ---------------------------------------------------------------------------------------------- Retrace
EDGE_BS, EDGE_LS = (1, 63, 64, 65, 257), (7, 8, 9, 15, 16, 17)
EDGE_EXTRA = ((4097, 9), (4097, 17), (65, 256))               # 65 workgroups with one lane in the last; AGX_SEQUENCE_LIMIT
EDGES = tuple((B, L) for B in EDGE_BS for L in EDGE_LS) + EDGE_EXTRA
DEFINITION_SHAPES = ((257, 17), (65, 256), (4097, 9))
SPECIAL_SHAPE = (257, 17)
SPECIAL_VALUES = np.array([0.0, -0.0, 0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126, -2.0 ** -126, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan], F32)
SPECIAL_SEED = 7                           # chosen on the model (tests/test_batch_limits_cpu.py asserts what it gives)
TINY = 2.0 ** -100


@functools.lru_cache(maxsize=None)
def edge(B, L):
    return _frozen(rm.case(B, L, 5000 + 1000 * B + L, live_specials=(B + L) % 2 == 1))


@functools.lru_cache(maxsize=None)
def special(seed=None):
    """retrace_model.case at SPECIAL_SHAPE with SPECIAL_VALUES in 40 % of the live reward, discount, q, v, c and boot, the rest
    ordinary normals; NaN wherever the rule says a value is not read (case() puts inf / NaN there in places: here it is NaN
    everywhere)."""
    B, L = SPECIAL_SHAPE
    seed = SPECIAL_SEED if seed is None else seed
    k = rm.case(B, L, 900 + seed)
    rng = np.random.default_rng(9100 + seed)
    inside = np.arange(L)[None, :] < np.clip(k["length"], 0, L)[:, None]
    has = rm.has_row(k["length"], k["steps"])
    for name in ("reward", "discount", "q", "v", "c"):
        read = inside if name == "v" else has
        hit = read & (rng.random((B, L)) < 0.4)
        k[name][hit] = SPECIAL_VALUES[rng.integers(0, len(SPECIAL_VALUES), int(hit.sum()))]
        k[name][~read] = np.nan
    hit = rng.random(B) < 0.4
    k["boot"][hit] = SPECIAL_VALUES[rng.integers(0, len(SPECIAL_VALUES), int(hit.sum()))]
    return _frozen(k)


def kinds(x):
    """How many NaN, infinite, subnormal and negative-zero elements x (f32) holds."""
    x = np.asarray(x, F32)
    mag = np.abs(x)
    return dict(nan=int(np.isnan(x).sum()), inf=int(np.isinf(x).sum()), subnormal=int(((mag > 0) & (mag < F32(2.0 ** -126))).sum()),
                negzero=int((rm.bits(x) == np.int32(-2 ** 31)).sum()))


@functools.lru_cache(maxsize=None)
def plain(B, L):
    """The case of the float64 check: retrace_model.case with c from {0, 1, uniform}: ordinary normals wherever a value is read,
    |c| <= 1, discount 0.99 or 0."""
    return _frozen(rm.case(B, L, 6000 + B + L))


U = 2.0 ** -24 + 2.0 ** -40


def _gamma(k):
    return k * U / (1.0 - k * U)


@functools.lru_cache(maxsize=None)
def definition(B, L, boot=True):
    """The paper's sum over plain(B, L) in float64 -> dict(target, td f64 [B, L]; bound_target, bound_td f64 [B, L] (the derived
    bounds of the module docstring); has bool [B, L]; left_out bool [B, L]: a non-zero term of the step's sum is below 2^-100;
    longest: the longest chain, in steps)."""
    k = plain(B, L)
    n = np.clip(k["length"].astype(np.int64), 0, L)
    has = (np.arange(L)[None, :] < n[:, None]) & (k["steps"] == 1)
    f = {name: np.where(has if name != "v" else np.arange(L)[None, :] < n[:, None], k[name].astype(np.float64), 0.0) for name in ("reward", "discount", "q", "v", "c")}
    behind = k["boot"].astype(np.float64) if boot else np.zeros(B)
    v_up = np.concatenate([f["v"][:, 1:], np.zeros((B, 1))], 1)
    vnext = np.where(np.arange(1, L + 1)[None, :] < n[:, None], v_up, behind[:, None])
    delta = f["reward"] + f["discount"] * vnext - f["q"]
    mass = np.abs(f["reward"]) + np.abs(f["discount"] * vnext) + np.abs(f["q"])
    parts = (np.abs(f["reward"]), np.abs(f["discount"] * vnext), np.abs(f["q"]))
    target, bound_t, bound_d = np.zeros((B, L)), np.zeros((B, L)), np.zeros((B, L))
    left_out = np.zeros((B, L), bool)
    longest = 0
    for l in range(L):
        coef, on = np.ones(B), has[:, l].copy()
        total, bt, bd = np.zeros(B), np.zeros(B), np.zeros(B)
        for j in range(l, L):
            if not on.any():
                break
            longest = max(longest, j - l + 1)
            total += np.where(on, coef * delta[:, j], 0.0)
            own = mass[:, j] - (np.abs(f["q"][:, j]) if j == l else 0.0)      # q[l] itself is added outside the fold's chain
            bt += np.where(on, _gamma(5 * (j - l) + 3) * np.abs(coef) * own, 0.0)
            bd += np.where(on, _gamma(5 * (j - l) + 4) * np.abs(coef) * mass[:, j], 0.0)
            for part in parts:
                term = np.abs(coef) * part[:, j]
                left_out[:, l] |= on & (term != 0) & (term < TINY)
            if j + 1 < L:
                coef = coef * f["discount"][:, j] * f["c"][:, j + 1]
                on &= has[:, j + 1]
        target[:, l] = np.where(has[:, l], f["q"][:, l] + total, 0.0)
        bound_t[:, l], bound_d[:, l] = bt, bd
    out = dict(target=target, td=np.where(has, target - f["q"], 0.0), bound_target=bound_t, bound_td=bound_d, has=has, left_out=left_out)
    for x in out.values():
        x.flags.writeable = False
    out["longest"] = longest
    return out


def worst_ratio(got_target, got_td, d):
    """(worst |target - definition| / bound, the same of td) over the steps with a row that are not left out."""
    at = d["has"] & ~d["left_out"]
    with np.errstate(all="ignore"):
        rt = np.abs(np.asarray(got_target, np.float64) - d["target"])[at] / d["bound_target"][at]
        rd = np.abs(np.asarray(got_td, np.float64) - d["td"])[at] / d["bound_td"][at]
    return float(np.nanmax(rt)) if rt.size else 0.0, float(np.nanmax(rd)) if rd.size else 0.0
