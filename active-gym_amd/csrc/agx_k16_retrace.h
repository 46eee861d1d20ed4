// agx_k16_retrace.h - K16: Retrace-family Q-returns over a sequence-replay batch (include/agx_retrace.h).  One sequence per
// thread, block = 64 = one wave, grid = ceil(B / 64).  The fold is agx_retrace_math.h's retrace_step - two sums, two products
// and two selects per step on the chain: nothing is restated here.  The chain per sequence is serial, so no load may sit on
// it: the kernel keeps two register sets of kRetraceAhead steps, issues the loads of the next set - they depend on nothing but
// l - and then folds the current one: k_slot_fold's shape (agx_slot_fold.h), walked over another rule.  A sequence's padding is
// at its NEWEST end (has(l) is false from len' on), so unlike a rollout fold nothing is skipped: every step is folded, and a
// step without a row leaves a zero carry behind.  Only the last set can be short (the L mod kRetraceAhead first steps): its
// loads are clamped to step 0 and its fold stops there.  Two addressing forms of the one text, chosen on the host:
//
//   k_retrace_direct<true>    time-major, element l * B + b: each step's loads and stores are coalesced across the wave's
//                             sequences as they stand, and the step offsets are wave-uniform.
//   k_retrace_direct<false>   batch-major, element b * L + l: a thread's row is L floats from its neighbour's, so a load touches
//                             a cache line per lane - and the 32 steps of that line are served from the cache afterwards.  A
//                             form that stages tiles of 64 sequences x 16 steps through LDS, so that a wave reads and writes
//                             along l, was built and measured 1.14 x SLOWER at both benchmark shapes; it
//                             is experiments/agx_retrace_tiled.h, in the experiments build only.
//
// Every device write is an ordinary vector store.
#pragma once
#include "agx_common.h"
#include "agx_retrace_math.h"

namespace agx {

#ifndef AGX_RETRACE_AHEAD
#define AGX_RETRACE_AHEAD 8          // the set depth (k_slot_fold's for V-trace): 96 of the kernel's 110 VGPRs
#endif

constexpr int kRetraceThreads = 64;
constexpr int kRetraceAhead = AGX_RETRACE_AHEAD;

struct RetraceParams {
    const int32_t *len;                            // [B]
    const int32_t *steps;                          // [B][L] or [L][B], as every per-step array
    const float *reward, *discount, *q, *v, *c;
    const float *boot;                             // [B] or nullptr
    float *target, *td;                            // td or nullptr
    uint8_t *valid;                                // or nullptr
    int32_t B, L;
};

struct RetraceSet {
    float r[kRetraceAhead], d[kRetraceAhead], q[kRetraceAhead], v[kRetraceAhead], c[kRetraceAhead];
    int32_t s[kRetraceAhead];
};

// the cnt steps from element `at` (step l0 of the thread's sequence) downward, `stride` elements apart; FULL: cnt == kRetraceAhead
template <bool FULL>
__device__ __forceinline__ void retrace_load(RetraceSet &s, const RetraceParams &p, uint32_t at, uint32_t stride, int cnt) {
#pragma unroll
    for (int i = 0; i < kRetraceAhead; ++i) {
        const uint32_t a = at - (uint32_t)(FULL ? i : min(i, cnt - 1)) * stride;
        s.s[i] = p.steps[a];
        s.r[i] = p.reward[a];
        s.d[i] = p.discount[a];
        s.q[i] = p.q[a];
        s.v[i] = p.v[a];
        s.c[i] = p.c[a];
    }
}

template <bool FULL>
__device__ __forceinline__ void retrace_fold_set(const RetraceSet &s, const RetraceParams &p, uint32_t at, uint32_t stride, int l0, int cnt, int len,
                                                 float boot, float &carry, float &vabove) {
#pragma unroll
    for (int i = 0; i < kRetraceAhead; ++i) {
        if (FULL || i < cnt) {                                       // (uniform: cnt depends on nothing of the sequence)
            const int l = l0 - i;
            const float vnext = l + 1 < len ? vabove : boot;
            const RetraceOut o = retrace_step(carry, retrace_has(l, len, s.s[i]), s.r[i], s.d[i], vnext, s.q[i], s.c[i]);
            vabove = s.v[i];
            const uint32_t a = at - (uint32_t)i * stride;
            p.target[a] = o.target;
            if (p.td) p.td[a] = o.td;
            if (p.valid) p.valid[a] = (uint8_t)o.valid;
        }
    }
}

template <bool TM>
__global__ __launch_bounds__(kRetraceThreads) void k_retrace_direct(RetraceParams p) {
    const int b = blockIdx.x * kRetraceThreads + threadIdx.x;
    if (b >= p.B) return;
    const int len = retrace_len(p.len[b], p.L);
    const float boot = p.boot ? p.boot[b] : 0.0f;
    const uint32_t stride = TM ? (uint32_t)p.B : 1u;                 // one step down (B * L <= INT32_MAX: every element number fits)
    const uint32_t jump = (uint32_t)kRetraceAhead * stride;
    float carry = 0.0f, vabove = 0.0f;
    int l0 = p.L - 1, cnt = min(kRetraceAhead, p.L);
    uint32_t at = TM ? (uint32_t)l0 * (uint32_t)p.B + (uint32_t)b : (uint32_t)b * (uint32_t)p.L + (uint32_t)l0;
    RetraceSet cur, nxt;
    if (cnt == kRetraceAhead)
        retrace_load<true>(cur, p, at, stride, cnt);
    else
        retrace_load<false>(cur, p, at, stride, cnt);
    for (;;) {
        const int ahead = min(kRetraceAhead, l0 + 1 - cnt);          // the steps of the next set; a short set is the last one
        if (ahead == kRetraceAhead)
            retrace_load<true>(nxt, p, at - jump, stride, ahead);
        else if (ahead > 0)
            retrace_load<false>(nxt, p, at - jump, stride, ahead);
        if (cnt == kRetraceAhead)
            retrace_fold_set<true>(cur, p, at, stride, l0, cnt, len, boot, carry, vabove);
        else
            retrace_fold_set<false>(cur, p, at, stride, l0, cnt, len, boot, carry, vabove);
        if (ahead == 0) break;
        cur = nxt;
        l0 -= kRetraceAhead;
        at -= jump;
        cnt = ahead;
    }
}

}  // namespace agx
