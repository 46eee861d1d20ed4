// agx_k13_vtrace.h - K13: V-trace targets and policy-gradient advantages over a gathered rollout (include/agx_vtrace.h).  The fold
// is agx_vtrace_math.h's vtrace_step: nothing is restated here.  Every device write is an ordinary vector store.
#pragma once
#include "agx_common.h"
#include "agx_vtrace_math.h"

namespace agx {

// ---------------------------------------------------------------------------------------------
// k_vtrace<BOOT>: the form of K12's GAE kernel with one more stream in and the same two out.  block = 64 = one wave, one env per
// thread, grid = ceil(N / 64).  The arrays are time-major, so every load and store of a step is coalesced across the envs of a
// wave.  The fold is a serial chain per env - a select, a product and a sum per step - so the loads must not sit on it: the kernel
// keeps two register sets of kVtraceAhead steps, issues the loads of the next set - they depend on nothing but t - and then
// folds the current one (vtrace_step, in the order of the header: nothing is reassociated).  A slot is addressed by its 32-bit
// element number (L * N <= INT32_MAX), which goes down by N per step: the step offsets are wave-uniform and stay on the scalar
// unit.  value[t + 1] is the register of the step before, not a load.  Only the last set can be short (the L mod kVtraceAhead
// oldest slots): its loads are clamped to its oldest slot and its fold stops there (FULL = false).  A slot that is not live is
// folded too and then written as 0: the live slots are the newest ones, so nothing the fold made of a padded slot reaches them.
// BOOT = false: d_boot_value is NULL and reads as 0.
// ---------------------------------------------------------------------------------------------
#ifndef AGX_VTRACE_AHEAD
#define AGX_VTRACE_AHEAD 8           // the set depth: 21.0 us against 21.8 us at 16 (tools/vtrace_bench.py)
#endif
constexpr int kVtraceThreads = 64, kVtraceAhead = AGX_VTRACE_AHEAD;

struct VtraceParams {
    const int32_t *len;                // [N]
    const float *reward;               // [L][N]
    const uint8_t *ends;               // [L][N]
    const float *value, *boot, *rho;   // [L][N]; boot or nullptr
    float *vs, *pg_adv;                // [L][N]
    int32_t N, L;
    VtraceCoef c;
};

struct VtraceSet {
    float r[kVtraceAhead], v[kVtraceAhead], b[kVtraceAhead], w[kVtraceAhead];
    uint32_t e[kVtraceAhead];
};

// the cnt slots from element `at` (slot t0 of the thread's env) downward; FULL: cnt == kVtraceAhead
template <bool BOOT, bool FULL>
__device__ __forceinline__ void vtrace_load(VtraceSet &s, const VtraceParams &q, uint32_t at, int cnt) {
#pragma unroll
    for (int i = 0; i < kVtraceAhead; ++i) {
        const uint32_t a = at - (uint32_t)(FULL ? i : min(i, cnt - 1)) * (uint32_t)q.N;
        s.r[i] = q.reward[a];
        s.v[i] = q.value[a];
        s.e[i] = q.ends[a];
        s.b[i] = BOOT ? q.boot[a] : 0.0f;
        s.w[i] = q.rho[a];
    }
}

template <bool FULL>
__device__ __forceinline__ void vtrace_fold_set(const VtraceSet &s, const VtraceParams &q, uint32_t at, int t0, int cnt, int first, float &A,
                                                float &vnext) {
#pragma unroll
    for (int i = 0; i < kVtraceAhead; ++i) {
        if (FULL || i < cnt) {                                       // (uniform: cnt depends on nothing of the env)
            const int t = t0 - i;
            const VtraceOut g = vtrace_step(A, s.e[i], t == q.L - 1, s.r[i], s.v[i], vnext, s.b[i], s.w[i], q.c);
            vnext = s.v[i];
            const uint32_t a = at - (uint32_t)i * (uint32_t)q.N;
            q.vs[a] = t >= first ? g.vs : 0.0f;
            q.pg_adv[a] = t >= first ? g.pg_adv : 0.0f;
        }
    }
}

template <bool BOOT>
__global__ __launch_bounds__(kVtraceThreads) void k_vtrace(VtraceParams q) {
    const int n = blockIdx.x * kVtraceThreads + threadIdx.x;
    if (n >= q.N) return;
    const int first = q.L - min(max(q.len[n], 0), q.L);
    const uint32_t stride = (uint32_t)kVtraceAhead * (uint32_t)q.N;
    float A = 0.0f, vnext = 0.0f;
    int t0 = q.L - 1, cnt = min(kVtraceAhead, q.L);
    uint32_t at = (uint32_t)t0 * (uint32_t)q.N + (uint32_t)n;
    VtraceSet cur, nxt;
    if (cnt == kVtraceAhead)
        vtrace_load<BOOT, true>(cur, q, at, cnt);
    else
        vtrace_load<BOOT, false>(cur, q, at, cnt);
    for (;;) {
        const int ahead = min(kVtraceAhead, t0 + 1 - cnt);           // the slots of the next set; a short set is the last one
        if (ahead == kVtraceAhead)
            vtrace_load<BOOT, true>(nxt, q, at - stride, ahead);
        else if (ahead > 0)
            vtrace_load<BOOT, false>(nxt, q, at - stride, ahead);
        if (cnt == kVtraceAhead)
            vtrace_fold_set<true>(cur, q, at, t0, cnt, first, A, vnext);
        else
            vtrace_fold_set<false>(cur, q, at, t0, cnt, first, A, vnext);
        if (ahead == 0) break;
        cur = nxt;
        t0 -= kVtraceAhead;
        at -= stride;
        cnt = ahead;
    }
}

}  // namespace agx
