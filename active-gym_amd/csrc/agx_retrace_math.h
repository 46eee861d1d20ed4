// agx_retrace_math.h - the Retrace-family Q-return fold over a sequence-replay batch (include/agx_retrace.h), as
// __host__ __device__ functions: both kernels of agx_k16_retrace.h fold every step with retrace_step, and a plain C++ program
// (tests/retrace_harness.cpp) runs retrace_fold, the loop over the very same functions.  It sits beside agx_fold_math.h, whose
// folds walk a rollout (padding at the OLDEST end, an ends byte per slot); a sequence is padded at its NEWEST end and cut by
// its steps.  Nothing here touches the GPU.
#pragma once
#include "agx_steplog_fold.h"

namespace agx {

constexpr int32_t kRetraceLimit = 256;                           // AGX_SEQUENCE_LIMIT

struct RetraceOut {
    float target, td;
    uint32_t valid;
};

// len' = clamp(len, 0, L)
AGX_HD int32_t retrace_len(int32_t len, int32_t L) { return len < 0 ? 0 : len > L ? L : len; }

// has(l): step l is inside the sequence and its row was recorded by a one-step gather.  Any other `steps` (0: padded, never
// recorded, the terminal observation's own step; > 1: a batch gathered with nstep > 1) is "no row".  len is len'.
AGX_HD bool retrace_has(int32_t l, int32_t len, int32_t steps) { return l < len && steps == 1; }

// a - b with one rounding (IEEE: a + (-b))
AGX_HD float retrace_fsub(float a, float b) { return steplog_fadd(a, -b); }

// One step l of the backward fold of one sequence.  carry is has(l + 1) ? c[l + 1] (T[l + 1] - q[l + 1]) : 0 on entry (0 at
// l = L - 1) and the same of step l on return; vnext is (l + 1 < len') ? v[l + 1] : boot.  A step without a row gives zeros by a
// select, so whatever its inputs hold - a NaN included - reaches neither an output nor the carry.
AGX_HD RetraceOut retrace_step(float &carry, bool has, float reward, float discount, float vnext, float q, float c) {
    const float T = steplog_fadd(reward, steplog_fmul(discount, steplog_fadd(vnext, carry)));
    const float td = retrace_fsub(T, q);
    carry = has ? steplog_fmul(c, td) : 0.0f;
    return has ? RetraceOut{T, td, 1u} : RetraceOut{0.0f, 0.0f, 0u};
}

// The whole fold of one sequence, newest step first.  at(l) places step l of the sequence in the [B][L] or [L][B] arrays;
// boot is the value behind step L - 1 (0 where the caller has none); td and valid may be nullptr.
template <class At>
AGX_HD void retrace_fold(const At &at, int32_t L, int32_t len, const int32_t *steps, const float *reward, const float *discount, const float *q,
                         const float *v, const float *c, float boot, float *target, float *td, uint8_t *valid) {
    len = retrace_len(len, L);
    float carry = 0.0f;
    for (int32_t l = L - 1; l >= 0; --l) {
        const auto i = at(l);
        const float vnext = l + 1 < len ? v[at(l + 1)] : boot;
        const RetraceOut o = retrace_step(carry, retrace_has(l, len, steps[i]), reward[i], discount[i], vnext, q[i], c[i]);
        target[i] = o.target;
        if (td) td[i] = o.td;
        if (valid) valid[i] = (uint8_t)o.valid;
    }
}

}  // namespace agx
