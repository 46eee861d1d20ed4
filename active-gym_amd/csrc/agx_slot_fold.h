// agx_slot_fold.h - the one kernel behind every backward fold over a gathered rollout: GAE (K12, agx_k12_rollout.h's GaeFold) and
// V-trace (K13, agx_k13_vtrace.h's VtraceFold) are policies of it.  Every device write is an ordinary vector store.
#pragma once
#include "agx_common.h"

namespace agx {

// ---------------------------------------------------------------------------------------------
// k_slot_fold<F, BOOT>: block = 64 = one wave, one env per thread, grid = ceil(N / 64): N = 1024 spreads over 16 CUs.  The arrays
// are time-major, so every load and store of a step is coalesced across the envs of a wave.  The fold is a serial chain per env,
// so the loads must not sit on it: the kernel keeps two register sets of F::kAhead steps, issues the loads of the next set
// - they depend on nothing but t - and then folds the current one (F::step, in the order of its math header: nothing is
// reassociated).  A slot is addressed by its 32-bit element number (L * N <= INT32_MAX), which goes down by N per step: the
// step offsets are wave-uniform and stay on the scalar unit.  value[t + 1] is the register of the step before, not a load.
// Only the last set can be short (the L mod F::kAhead oldest slots): its loads are clamped to its oldest slot and its fold
// stops there (FULL = false).  A slot that is not live is folded too and then written as 0: the live slots are the newest
// ones, so nothing the fold made of a padded slot reaches them.  BOOT = false: d_boot_value is NULL and reads as 0.
//
// A policy F supplies
//   Params                           the kernel's argument: len [N], N, L, the streams in and out, the coefficients
//   kAhead                           the set depth
//   Set                              one register set, a struct of arrays [kAhead]; v is the value stream
//   coef(q)                          what every step needs and is formed once per thread (GAE's gamma * lambda)
//   load<BOOT>(set, i, q, a)         entry i of a set from element a, streams in the order r, v, e, b[, w]
//   step(A, set, i, newest, vnext, q, coef) -> Out   and   store(q, a, live, out)
// ---------------------------------------------------------------------------------------------
constexpr int kFoldThreads = 64;

// the cnt slots from element `at` (slot t0 of the thread's env) downward; FULL: cnt == F::kAhead
template <class F, bool BOOT, bool FULL>
__device__ __forceinline__ void fold_load(typename F::Set &s, const typename F::Params &q, uint32_t at, int cnt) {
#pragma unroll
    for (int i = 0; i < F::kAhead; ++i) F::template load<BOOT>(s, i, q, at - (uint32_t)(FULL ? i : min(i, cnt - 1)) * (uint32_t)q.N);
}

template <class F, bool FULL, class Coef>
__device__ __forceinline__ void fold_set(const typename F::Set &s, const typename F::Params &q, uint32_t at, int t0, int cnt, int first,
                                         const Coef &c, float &A, float &vnext) {
#pragma unroll
    for (int i = 0; i < F::kAhead; ++i) {
        if (FULL || i < cnt) {                                       // (uniform: cnt depends on nothing of the env)
            const int t = t0 - i;
            const auto g = F::step(A, s, i, t == q.L - 1, vnext, q, c);
            vnext = s.v[i];
            const uint32_t a = at - (uint32_t)i * (uint32_t)q.N;
            F::store(q, a, t >= first, g);
        }
    }
}

template <class F, bool BOOT>
__global__ __launch_bounds__(kFoldThreads) void k_slot_fold(typename F::Params q) {
    constexpr int kAhead = F::kAhead;
    const int n = blockIdx.x * kFoldThreads + threadIdx.x;
    if (n >= q.N) return;
    const int first = q.L - min(max(q.len[n], 0), q.L);
    const auto c = F::coef(q);
    const uint32_t stride = (uint32_t)kAhead * (uint32_t)q.N;
    float A = 0.0f, vnext = 0.0f;
    int t0 = q.L - 1, cnt = min(kAhead, q.L);
    uint32_t at = (uint32_t)t0 * (uint32_t)q.N + (uint32_t)n;
    typename F::Set cur, nxt;
    if (cnt == kAhead)
        fold_load<F, BOOT, true>(cur, q, at, cnt);
    else
        fold_load<F, BOOT, false>(cur, q, at, cnt);
    for (;;) {
        const int ahead = min(kAhead, t0 + 1 - cnt);                 // the slots of the next set; a short set is the last one
        if (ahead == kAhead)
            fold_load<F, BOOT, true>(nxt, q, at - stride, ahead);
        else if (ahead > 0)
            fold_load<F, BOOT, false>(nxt, q, at - stride, ahead);
        if (cnt == kAhead)
            fold_set<F, true>(cur, q, at, t0, cnt, first, c, A, vnext);
        else
            fold_set<F, false>(cur, q, at, t0, cnt, first, c, A, vnext);
        if (ahead == 0) break;
        cur = nxt;
        t0 -= kAhead;
        at -= stride;
        cnt = ahead;
    }
}

}  // namespace agx
