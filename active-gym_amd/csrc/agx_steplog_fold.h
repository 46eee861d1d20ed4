// agx_steplog_fold.h - the walk of the step log's gather (include/agx_steplog.h): the stop rules and the fadd / fmul fold, as
// __host__ __device__ functions over an accessor argument: k_steplog_gather (agx_k8_steplog.h) and a plain C++ program
// (tests/steplog_harness.cpp) run the very same code.  Nothing here touches the GPU.
#pragma once
#include "agx_hist_rule.h"

namespace agx {

constexpr uint32_t kStepTerminated = 1, kStepTruncated = 2;      // AGX_STEP_TERMINATED, AGX_STEP_TRUNCATED

// One rounding each, never contracted: __fmul_rn / __fadd_rn are plain operators in this toolchain's headers, which the
// compiler may still fuse into a multiply-add where they are inlined, so the contraction is switched off here by pragma (a
// compiler other than clang takes -ffp-contract=off on its command line).
AGX_HD float steplog_fmul(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a * b;
}
AGX_HD float steplog_fadd(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a + b;
}

// the state of one sample's walk: m rows folded so far, their discounted sum, gamma^m and the flags of the last one
struct StepFold {
    int32_t m = 0;
    float G = 0.0f, disc = 1.0f;
    uint32_t last = 0;
};

// ok0: n is an env and row k is still retained (cnt = count[n], read only when n is an env)
AGX_HD bool steplog_ok0(int64_t k, int64_t cnt, int32_t T) { return hist_retained(k, cnt, T); }

// Step i (1 first) of the walk from k.  r = rows.at(j) places row j of the sample's env (j mod T, once per step); rows.age(r),
// rows.stamp(r), rows.reward(r), rows.flags(r) read it.  They are called for retained j only, and reward / flags only behind a
// matching stamp.  Returns whether the walk goes on.
template <class Rows>
AGX_HD bool steplog_step(StepFold &f, const Rows &rows, int64_t k, int64_t cnt, int32_t i, float gamma) {
    const int64_t j = k + i;
    if (j >= cnt) return false;                                   // the end of the history
    const auto r = rows.at(j);
    if (rows.age(r) == 0 || rows.stamp(r) != j) return false;     // another episode; never recorded
    f.G = steplog_fadd(f.G, steplog_fmul(f.disc, rows.reward(r)));
    f.disc = steplog_fmul(f.disc, gamma);
    f.m = i;
    f.last = rows.flags(r);
    return (f.last & (kStepTerminated | kStepTruncated)) == 0;
}

// the whole walk of one sample (the kernel runs the loop itself, to leave it by wave)
template <class Rows>
AGX_HD StepFold steplog_walk(const Rows &rows, bool ok0, int64_t k, int64_t cnt, int32_t nstep, float gamma) {
    StepFold f;
    bool go = ok0;
    for (int32_t i = 1; i <= nstep && go; ++i) go = steplog_step(f, rows, k, cnt, i, gamma);
    return f;
}

AGX_HD float steplog_discount(const StepFold &f) { return (f.last & kStepTerminated) ? 0.0f : f.disc; }

}  // namespace agx
