// agx_fold_math.h - what every backward fold over a gathered rollout shares (GAE in agx_rollout_math.h, V-trace in
// agx_vtrace_math.h): the bits of the ends byte the gather writes, the two tests every step opens with, and the host loop over
// the slots of one env.  __host__ __device__ functions; nothing here touches the GPU.
#pragma once
#include "agx_steplog_fold.h"

namespace agx {

constexpr uint32_t kRolloutCut = 4, kRolloutBoot = 8;            // AGX_ROLLOUT_CUT, AGX_ROLLOUT_BOOT
constexpr uint32_t kRolloutBreak = kStepTerminated | kStepTruncated | kRolloutCut;      // the bits that end an episode's chain

// the value a step of slot t bootstraps from: value_next = value[t + 1] (anything at t = L - 1), boot = boot_value[t] (anything
// where BOOT is not set)
AGX_HD float fold_next_value(uint32_t e, bool newest, float value_next, float boot) {
    return (e & kRolloutBoot) ? boot : ((e & kStepTerminated) || newest) ? 0.0f : value_next;
}

// whether nothing of slot t + 1 is carried into slot t
AGX_HD bool fold_breaks(uint32_t e, bool newest) { return newest || (e & kRolloutBreak); }

// The whole fold of one env, newest slot first.  at(t) places slot t of the env in the [L][N] arrays; step(A, i, newest, i_next)
// folds the live slot at i (i_next: the place of slot t + 1, i itself at t = L - 1, where it is not to be used) and returns what
// write(i, out) stores; a slot that is not live gets a zeroed Out.
template <class Out, class At, class Step, class Write>
AGX_HD void slot_fold(const At &at, int32_t L, int32_t len, Step &&step, Write &&write) {
    const int32_t first = L - (len < 0 ? 0 : len > L ? L : len);
    float A = 0.0f;
    for (int32_t t = L - 1; t >= 0; --t) {
        const auto i = at(t);
        Out o{};
        if (t >= first) o = step(A, i, t == L - 1, t == L - 1 ? i : at(t + 1));
        write(i, o);
    }
}

}  // namespace agx
