// agx_vtrace_math.h - the V-trace fold over a gathered rollout (include/agx_vtrace.h), as __host__ __device__ functions over an
// accessor argument: k_vtrace (agx_k13_vtrace.h) folds every step with vtrace_step, and a plain C++ program
// (tests/vtrace_harness.cpp) runs vtrace_fold, the loop over the very same function.  Nothing here touches the GPU.
#pragma once
#include "agx_steplog_fold.h"

namespace agx {

constexpr int32_t kVtraceLimit = 4096;                           // AGX_VTRACE_LIMIT
constexpr uint32_t kVtraceBoot = 8;                              // the BOOT bit of the ends byte
constexpr uint32_t kVtraceBreak = 7;                             // TERMINATED | TRUNCATED | CUT: the bits that end an episode's chain

// the three truncation levels and the two discounts of one call
struct VtraceCoef {
    float gamma, lambda, rho_bar, c_bar, pg_rho_bar;
};

struct VtraceOut {
    float vs, pg_adv;
};

// x < bar ? x : bar: a NaN x gives bar
AGX_HD float vtrace_min(float x, float bar) { return x < bar ? x : bar; }

// One step of the backward fold of one env: A is vs - value of slot t + 1 on entry and of slot t on return.
// value_next = value[t + 1] (anything at t = L - 1), boot = boot_value[t] (anything where BOOT is not set).
AGX_HD VtraceOut vtrace_step(float &A, uint32_t e, bool newest, float reward, float value, float value_next, float boot, float rho,
                             const VtraceCoef &c) {
    const float nv = (e & kVtraceBoot) ? boot : ((e & kStepTerminated) || newest) ? 0.0f : value_next;
    const float carry = (newest || (e & kVtraceBreak)) ? 0.0f : A;
    const float td = steplog_fadd(steplog_fadd(reward, steplog_fmul(c.gamma, nv)), -value);
    const float cc = steplog_fmul(c.lambda, vtrace_min(rho, c.c_bar));
    A = steplog_fadd(steplog_fmul(vtrace_min(rho, c.rho_bar), td), steplog_fmul(steplog_fmul(c.gamma, cc), carry));
    const float q = steplog_fadd(steplog_fadd(reward, steplog_fmul(c.gamma, steplog_fadd(nv, carry))), -value);
    return VtraceOut{steplog_fadd(A, value), steplog_fmul(vtrace_min(rho, c.pg_rho_bar), q)};
}

// The whole fold of one env.  at(t) places slot t of the env in the [L][N] arrays; boot may be nullptr (reads as 0).
template <class At>
AGX_HD void vtrace_fold(const At &at, int32_t L, int32_t len, const float *reward, const uint8_t *ends, const float *value, const float *boot,
                        const float *rho, const VtraceCoef &c, float *vs, float *pg_adv) {
    const int32_t first = L - (len < 0 ? 0 : len > L ? L : len);
    float A = 0.0f;
    for (int32_t t = L - 1; t >= 0; --t) {
        const auto i = at(t);
        VtraceOut o{0.0f, 0.0f};
        if (t >= first)
            o = vtrace_step(A, ends[i], t == L - 1, reward[i], value[i], t == L - 1 ? 0.0f : value[at(t + 1)], boot ? boot[i] : 0.0f, rho[i], c);
        vs[i] = o.vs;
        pg_adv[i] = o.pg_adv;
    }
}

}  // namespace agx
