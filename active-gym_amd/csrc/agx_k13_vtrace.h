// agx_k13_vtrace.h - K13: V-trace targets and policy-gradient advantages over a gathered rollout (include/agx_vtrace.h):
// k_slot_fold<VtraceFold, BOOT> (agx_slot_fold.h), GAE's kernel with one more stream in (rho) and the same two out.  The fold is
// agx_vtrace_math.h's vtrace_step - a select, a product and a sum per step on the chain: nothing is restated here.
#pragma once
#include "agx_slot_fold.h"
#include "agx_vtrace_math.h"

namespace agx {

#ifndef AGX_VTRACE_AHEAD
#define AGX_VTRACE_AHEAD 8           // the set depth: 21.0 us against 21.8 us at 16 (tools/vtrace_bench.py)
#endif

struct VtraceParams {
    const int32_t *len;                // [N]
    const float *reward;               // [L][N]
    const uint8_t *ends;               // [L][N]
    const float *value, *boot, *rho;   // [L][N]; boot or nullptr
    float *vs, *pg_adv;                // [L][N]
    int32_t N, L;
    VtraceCoef c;
};

struct VtraceFold {
    using Params = VtraceParams;
    using Out = VtraceOut;
    static constexpr int kAhead = AGX_VTRACE_AHEAD;
    struct Set {
        float r[kAhead], v[kAhead], b[kAhead], w[kAhead];
        uint32_t e[kAhead];
    };
    struct NoCoef {};                  // (every coefficient is in Params)
    static __device__ __forceinline__ NoCoef coef(const Params &) { return {}; }
    template <bool BOOT>
    static __device__ __forceinline__ void load(Set &s, int i, const Params &q, uint32_t a) {
        s.r[i] = q.reward[a];
        s.v[i] = q.value[a];
        s.e[i] = q.ends[a];
        s.b[i] = BOOT ? q.boot[a] : 0.0f;
        s.w[i] = q.rho[a];
    }
    static __device__ __forceinline__ Out step(float &A, const Set &s, int i, bool newest, float vnext, const Params &q, NoCoef) {
        return vtrace_step(A, s.e[i], newest, s.r[i], s.v[i], vnext, s.b[i], s.w[i], q.c);
    }
    static __device__ __forceinline__ void store(const Params &q, uint32_t a, bool live, const Out &g) {
        q.vs[a] = live ? g.vs : 0.0f;
        q.pg_adv[a] = live ? g.pg_adv : 0.0f;
    }
};

}  // namespace agx
