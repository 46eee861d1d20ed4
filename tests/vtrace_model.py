"""The float32 V-trace fold of include/agx_vtrace.h in NumPy, one rounding per operation, written from the header and sharing
nothing with active-gym_amd/csrc/agx_vtrace_math.h; the paper's DEFINITION (Espeholt et al. 2018, eq. 1) in float64 as the explicit
sum - not the recursion - cut at episode ends; the error bound of the one against the other, derived from the operation count;
and the synthetic cases tests/test_vtrace_cpu.py and tests/test_gpu_vtrace.py share.  Pure NumPy, no GPU."""
import numpy as np

import limit_cases as lc
from limit_cases import F32, U24

TERMINATED, BOOT, BREAK = 1, 8, 7

# (gamma, lambda, (rho_bar, c_bar, pg_rho_bar)) of the GPU cases
PARAMS = ((0.99, 1.0, (1.0, 1.0, 1.0)), (0.9, 0.95, (1.0, 1.0, 1.0)), (1.0, 1.0, (np.inf, np.inf, np.inf)), (0.99, 0.5, (2.0, 0.5, 1.0)))
NS, LS = (5, 70), (1, 5, 8, 9, 16, 17, 33, 130)


def vmin(x, bar):
    """x < bar ? x : bar: a NaN x gives bar."""
    return np.where(np.less(x, bar), x, bar).astype(F32)


def vtrace(length, reward, ends, value, boot, rho, gamma, lam, bars, with_A=False):
    """agx_vtrace_returns in np.float32 -> (vs, pg_adv) f32 [L, N] (with_A: and A = vs - value before its last rounding's sum).
    The envs are one float32 array per step and NumPy rounds every float32 array operation on its own: the header's operations in
    the header's order.  boot: [L, N] or None; bars: (rho_bar, c_bar, pg_rho_bar)."""
    L, N = reward.shape
    gamma, lam = F32(gamma), F32(lam)
    rho_bar, c_bar, pg_bar = (F32(b) for b in bars)
    reward, value, rho, ends = np.asarray(reward, F32), np.asarray(value, F32), np.asarray(rho, F32), np.asarray(ends)
    first = L - np.clip(np.asarray(length, np.int64), 0, L)
    vs, pg, adv = np.zeros((L, N), F32), np.zeros((L, N), F32), np.zeros((L, N), F32)
    zero = np.zeros(N, F32)
    A = zero
    with np.errstate(all="ignore"):
        for t in range(L - 1, -1, -1):
            e, v, r, w = ends[t], value[t], reward[t], rho[t]
            newest = t == L - 1
            after = zero if newest else np.where(e & TERMINATED, zero, value[t + 1])
            nv = np.where(e & BOOT, zero if boot is None else np.asarray(boot[t], F32), after).astype(F32)
            carry = zero if newest else np.where(e & BREAK, zero, A).astype(F32)
            td = ((r + (gamma * nv).astype(F32)).astype(F32) + (-v)).astype(F32)
            cc = (lam * vmin(w, c_bar)).astype(F32)
            A = ((vmin(w, rho_bar) * td).astype(F32) + ((gamma * cc).astype(F32) * carry).astype(F32)).astype(F32)
            q = ((r + (gamma * (nv + carry).astype(F32)).astype(F32)).astype(F32) + (-v)).astype(F32)
            live = t >= first
            vs[t] = np.where(live, (A + v).astype(F32), zero)
            pg[t] = np.where(live, (vmin(w, pg_bar) * q).astype(F32), zero)
            A = np.where(live, A, zero)                   # a slot that is not live is older than every live one: nothing reads this
            adv[t] = A
    return (vs, pg, adv) if with_A else (vs, pg)


def case(N, L, seed):
    """limit_cases.gae_case - len with the wild values, ends over the legal bytes, reward / value / boot of mixed magnitude, NaN in
    boot where BOOT is unset and in reward / value where the slot is not live - plus rho: uniform in [0, 4] with exact 0, 1 and 4
    among them, and NaN in the slots that are not live.  -> (len, reward, ends, value, boot, rho, live)."""
    length, reward, ends, value, boot, live = lc.gae_case(N, L, seed)
    rng = np.random.default_rng(seed + 5000)
    rho = rng.uniform(0.0, 4.0, (L, N)).astype(F32)
    pick = rng.random((L, N))
    rho = np.where(pick < 0.05, F32(0), np.where(pick < 0.15, F32(1), np.where(pick < 0.2, F32(4), rho))).astype(F32)
    rho[~live] = np.nan
    return length, reward, ends, value, boot, rho, live


# ---------------------------------------------------------------------------------------------- the definition, in float64
def definition(length, reward, ends, value, boot, rho, gamma, lam, bars):
    """The paper's V-trace target as the explicit sum, in float64, vectorised over the envs.  For a live slot s, over the chain of
    slots s .. e from s to the first one that breaks it (ends & 7, or L - 1):

        vs_s = V_s + sum_{k = s .. e} g^(k - s) (prod_{i = s .. k - 1} c_i) rho_k td_k,     td_k = r_k + g nv_k - V_k,
        rho_k = min(rho_bar, w_k),  c_i = lam min(c_bar, w_i),  nv_k = boot_k (BOOT) | 0 (TERMINATED, or k = L - 1) | V_(k+1)

    and pg_adv_s = min(pg_rho_bar, w_s) (r_s + g vs_(s+1) - V_s), vs_(s+1) = nv_s + (vs - V)_(s+1) inside a chain and nv_s where slot
    s breaks it.  g, lam and the levels are float64(float32(.)); a NaN ratio reads as the level, as the header says.
    -> dict: A (= vs - V), vs, pg f64 [L, N]; S: the sum of the magnitudes of every term that enters A_s; chain: the slots in the
    sum; smallest: the smallest non-zero term's magnitude; Q: |r| + g |nv| + |V| of slot s; brk, live bool [L, N]."""
    L, N = reward.shape
    g, la = float(F32(gamma)), float(F32(lam))
    rho_bar, c_bar, pg_bar = (float(F32(b)) for b in bars)
    live = np.arange(L)[:, None] >= L - np.clip(np.asarray(length, np.int64), 0, L)[None, :]
    r, v = np.where(live, reward, 0).astype(np.float64), np.where(live, value, 0).astype(np.float64)
    b = np.zeros((L, N)) if boot is None else np.where(ends & BOOT, boot, 0).astype(np.float64)
    w = np.asarray(rho, np.float64)
    clip = lambda bar: np.where(np.less(w, bar), w, bar)
    with np.errstate(all="ignore"):
        rho_k, c_k, rho_pg = clip(rho_bar), la * clip(c_bar), clip(pg_bar)
        brk = (ends & BREAK) != 0
        brk[L - 1] = True
        nxt_v = np.concatenate([v[1:], np.zeros((1, N))])
        last = np.zeros((L, N), bool)
        last[L - 1] = True
        nv = np.where(ends & BOOT, b, np.where(((ends & TERMINATED) != 0) | last, 0.0, nxt_v))
        td, Q = r + g * nv - v, np.abs(r) + g * np.abs(nv) + np.abs(v)
        A, S, chain, smallest = np.zeros((L, N)), np.zeros((L, N)), np.zeros((L, N)), np.full((L, N), np.inf)
        for s in range(L):
            coef, on = np.ones(N), live[s].copy()
            for k in range(s, L):
                if not on.any():
                    break
                A[s] += np.where(on, coef * rho_k[k] * td[k], 0.0)
                S[s] += np.where(on, np.abs(coef * rho_k[k]) * Q[k], 0.0)
                mags = np.abs(coef * rho_k[k])[None, :] * np.stack([np.abs(r[k]), g * np.abs(nv[k]), np.abs(v[k])])
                mags = np.where(on[None, :] & (mags > 0), mags, np.inf).min(0)
                smallest[s] = np.minimum(smallest[s], mags)
                chain[s] += on
                on = on & ~brk[k]
                coef = coef * g * c_k[k]
        vs = np.where(live, v + A, 0.0)
        nxt_vs = nv + np.where(brk, 0.0, np.concatenate([A[1:], np.zeros((1, N))]))
        pg = np.where(live, rho_pg * (r + g * nxt_vs - v), 0.0)
    return dict(A=A, vs=vs, pg=pg, S=S, chain=chain, smallest=smallest, Q=Q, brk=brk, live=live, g=g, rho_pg=rho_pg, nv=nv)


def gamma_k(k):
    """Higham's gamma_k = k u / (1 - k u): the bound of a product of k factors (1 + d), |d| <= u = 2^-24, minus 1."""
    ku = np.asarray(k, np.float64) * U24
    return ku / (1.0 - ku)


def bounds(d):
    """The error bounds of the float32 fold against definition()'s dict d -> (bound on A, on vs, on pg_adv), each [L, N].

    A: a term x of td_k (r_k, g nv_k or V_k) meets at most one rounding when it is formed (the product g nv), two in the additions
    of td_k, one in the product with rho_k and one in the addition of the carry: 5.  Each of the l slots it is then carried over
    multiplies it by fl(gamma fl(lam min(c_bar, w))) - two roundings off the exact coefficient - rounds that product and rounds the
    addition: 4 per slot.  5 + 4 l <= 5 (l + 1) <= 5 chain factors (1 + d) on a term of magnitude g^l (prod c) rho_k |x|, so
    |A32 - A| <= gamma_(5 chain) S.  (The selects and min are exact.)
    vs = fl(A32 + V): |vs32 - vs| <= (1 + u) bA + u |vs|.
    pg_adv = fl(rho_pg fl(fl(r + fl(g fl(nv + carry32))) - V)): every term of r + g (nv + carry) - V meets at most 5 roundings (nv
    and carry: the sum, the product, two additions, the product with rho_pg), and carry32 is A32 of slot s + 1, off by at most its
    own bound: |pg32 - pg| <= rho_pg (gamma_5 (|r| + g |nv| + g |A_(s+1)| + |V|) + (1 + gamma_5) g bA_(s+1)), carry and its bound
    being 0 where the slot breaks the chain."""
    bA = gamma_k(5 * d["chain"]) * d["S"]
    bvs = (1 + U24) * bA + U24 * np.abs(d["vs"])
    L, N = bA.shape
    zero = np.zeros((1, N))
    nxtA, nxtb = np.where(d["brk"], 0.0, np.concatenate([d["A"][1:], zero])), np.where(d["brk"], 0.0, np.concatenate([bA[1:], zero]))
    g5 = gamma_k(5)
    with np.errstate(invalid="ignore"):               # (an infinite level times 0 in a slot that is not live)
        bpg = np.abs(d["rho_pg"]) * (g5 * (d["Q"] + d["g"] * np.abs(nxtA)) + (1 + g5) * d["g"] * nxtb)
    return bA, bvs, bpg
