// agx_rollout_math.h - the rule of an on-policy rollout on the step log and the GAE fold (include/agx_rollout.h), as
// __host__ __device__ functions over an accessor argument: k_rollout_gather / k_slot_fold<GaeFold> (agx_k12_rollout.h) decide every row
// with rollout_row and rollout_ends and fold every step with gae_step, and a plain C++ program (tests/rollout_harness.cpp) runs
// rollout_walk and gae_fold, the loops over the very same three (gae_fold is agx_fold_math.h's slot_fold).  Nothing here touches the GPU.
#pragma once
#include "agx_fold_math.h"

namespace agx {

constexpr int32_t kRolloutLimit = 4096;                          // AGX_ROLLOUT_LIMIT

enum RolloutRow : int { kRolloutTake = 0, kRolloutSkip = 1, kRolloutStop = 2 };

// What row j < cnt of an env means to the walk.  It stops where observation j - 1 is no longer retained (the walk's j > lo,
// by the history's own rule), the row was never recorded, or observation j - 1 is not valid; it skips a reset observation.
// r = rows.at(j) places row j of the env; rows.age(r) and rows.stamp(r) read it, for retained j and j - 1 only.
template <class Rows>
AGX_HD RolloutRow rollout_row(const Rows &rows, int64_t j, int64_t cnt, int32_t T, int32_t fs) {
    if (j >= cnt || !hist_retained(j - 1, cnt, T)) return kRolloutStop;
    const auto r = rows.at(j);
    if (rows.age(r) == 0) return kRolloutSkip;
    if (rows.stamp(r) != j) return kRolloutStop;
    return hist_stack_ok(j - 1, cnt, T, fs, rows.age(rows.at(j - 1))) ? kRolloutTake : kRolloutStop;
}

// the ends byte of the transition row j that rollout_row took; newest: it fills slot L - 1
template <class Rows>
AGX_HD uint32_t rollout_ends(const Rows &rows, int64_t j, int64_t cnt, bool newest) {
    uint32_t e = rows.flags(rows.at(j)) & (kStepTerminated | kStepTruncated);
    if (e == 0 && j + 1 < cnt && rows.age(rows.at(j + 1)) == 0) e = kRolloutCut;
    if (!(e & kStepTerminated) && (newest || e != 0)) e |= kRolloutBoot;
    return e;
}

// The whole walk of one env: emit(t, j, ends) for every live slot, newest first; returns len.
template <class Rows, class Emit>
AGX_HD int32_t rollout_walk(const Rows &rows, int64_t cnt, int32_t T, int32_t fs, int32_t L, Emit &&emit) {
    int32_t len = 0;
    for (int64_t j = cnt - 1; len < L; --j) {
        const RolloutRow w = rollout_row(rows, j, cnt, T, fs);
        if (w == kRolloutStop) break;
        if (w == kRolloutSkip) continue;
        emit(L - 1 - len, j, rollout_ends(rows, j, cnt, len == 0));
        ++len;
    }
    return len;
}

// ---- GAE.  One step of the backward fold of one env: A is the advantage of slot t + 1 on entry and of slot t on return.
// value_next = value[t + 1] (anything at t = L - 1), boot = boot_value[t] (anything where BOOT is not set).
struct GaeOut {
    float adv, ret;
};
AGX_HD GaeOut gae_step(float &A, uint32_t e, bool newest, float reward, float value, float value_next, float boot, float gamma, float gl) {
    const float nv = fold_next_value(e, newest, value_next, boot);
    const float delta = steplog_fadd(steplog_fadd(reward, steplog_fmul(gamma, nv)), -value);
    const float carry = fold_breaks(e, newest) ? 0.0f : steplog_fmul(gl, A);
    A = steplog_fadd(delta, carry);
    return GaeOut{A, steplog_fadd(A, value)};
}

// The whole fold of one env: slot_fold over gae_step.  at(t) places slot t of the env in the [L][N] arrays; boot may be nullptr
// (reads as 0).
template <class At>
AGX_HD void gae_fold(const At &at, int32_t L, int32_t len, const float *reward, const uint8_t *ends, const float *value, const float *boot,
                     float gamma, float lambda, float *adv, float *ret) {
    const float gl = steplog_fmul(gamma, lambda);
    slot_fold<GaeOut>(
        at, L, len,
        [&](float &A, auto i, bool newest, auto i_next) {
            return gae_step(A, ends[i], newest, reward[i], value[i], newest ? 0.0f : value[i_next], boot ? boot[i] : 0.0f, gamma, gl);
        },
        [&](auto i, const GaeOut &o) { adv[i] = o.adv, ret[i] = o.ret; });
}

}  // namespace agx
