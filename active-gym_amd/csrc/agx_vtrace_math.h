// agx_vtrace_math.h - the V-trace fold over a gathered rollout (include/agx_vtrace.h), as __host__ __device__ functions over an
// accessor argument: k_slot_fold<VtraceFold> (agx_k13_vtrace.h) folds every step with vtrace_step, and a plain C++ program
// (tests/vtrace_harness.cpp) runs vtrace_fold, the loop over the very same function (agx_fold_math.h's slot_fold).  Nothing here touches the GPU.
#pragma once
#include "agx_fold_math.h"

namespace agx {

constexpr int32_t kVtraceLimit = 4096;                           // AGX_VTRACE_LIMIT

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
    const float nv = fold_next_value(e, newest, value_next, boot);
    const float carry = fold_breaks(e, newest) ? 0.0f : A;
    const float td = steplog_fadd(steplog_fadd(reward, steplog_fmul(c.gamma, nv)), -value);
    const float cc = steplog_fmul(c.lambda, vtrace_min(rho, c.c_bar));
    A = steplog_fadd(steplog_fmul(vtrace_min(rho, c.rho_bar), td), steplog_fmul(steplog_fmul(c.gamma, cc), carry));
    const float q = steplog_fadd(steplog_fadd(reward, steplog_fmul(c.gamma, steplog_fadd(nv, carry))), -value);
    return VtraceOut{steplog_fadd(A, value), steplog_fmul(vtrace_min(rho, c.pg_rho_bar), q)};
}

// The whole fold of one env: slot_fold over vtrace_step.  at(t) places slot t of the env in the [L][N] arrays; boot may be nullptr
// (reads as 0).
template <class At>
AGX_HD void vtrace_fold(const At &at, int32_t L, int32_t len, const float *reward, const uint8_t *ends, const float *value, const float *boot,
                        const float *rho, const VtraceCoef &c, float *vs, float *pg_adv) {
    slot_fold<VtraceOut>(
        at, L, len,
        [&](float &A, auto i, bool newest, auto i_next) {
            return vtrace_step(A, ends[i], newest, reward[i], value[i], newest ? 0.0f : value[i_next], boot ? boot[i] : 0.0f, rho[i], c);
        },
        [&](auto i, const VtraceOut &o) { vs[i] = o.vs, pg_adv[i] = o.pg_adv; });
}

}  // namespace agx
