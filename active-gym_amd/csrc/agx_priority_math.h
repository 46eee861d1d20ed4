// agx_priority_math.h - the arithmetic of the prioritized sampler (include/agx_priority.h) as __host__ __device__ functions:
// quantise, the effective weight, the acceptance predicate over an age accessor, the weight of a row and the row search.  The
// kernels of agx_k9_priority.h and a plain C++ program (tests/priority_harness.cpp) run the very same code.  Integers and one
// f32 multiply; nothing here touches the GPU.
#pragma once
#include "agx_replay_draw.h"

namespace agx {

constexpr uint32_t kPriorityOne = 65536u;            // the weight of priority 1.0, and wmax of a new / cleared table

// f32 priority -> fixed-point weight, never 0
AGX_HD uint32_t priority_quantise(float p) {
    if (!(p > 0.0f)) return 1u;                      // zero, negative, NaN
    const float q = p * 65536.0f;                    // exact short of overflow
    if (q >= 4294967296.0f) return 0xFFFFFFFFu;      // (+inf included)
    const uint32_t w = (uint32_t)q;
    return w > 0u ? w : 1u;
}

// the weight of a retained (n, k) whose row holds (stamp, weight)
AGX_HD uint32_t priority_effective(int64_t stamp, uint32_t weight, int64_t k, uint32_t wmax) { return stamp == k ? weight : wmax; }

AGX_HD int32_t priority_min(int32_t a, int32_t b) { return a < b ? a : b; }

// accepted(n, k) of include/agx_replay.h for a retained k (lo <= k < cnt, lo = replay_lo(cnt, T)); ages.age(j) is the age byte
// of row j of the same env and is called for retained j only.  fs1 = frame_stack - 1.
template <class Ages>
AGX_HD bool priority_accepted(const Ages &ages, int64_t k, int64_t cnt, int64_t lo, int32_t fs1, int32_t back, int32_t forward) {
    const int32_t age = ages.age(k);
    if (k - priority_min(age, fs1) < lo) return false;                          // 1. (n, k) is valid
    const int64_t kb = k - priority_min(back, age);
    if (kb < lo) return false;                                                  // 2. (n, k - b) is retained and valid
    if (kb != k && kb - priority_min(ages.age(kb), fs1) < lo) return false;
    if (k + forward >= cnt) return false;                                       // 3. the same episode forward appends on
    return forward == 0 || ages.age(k + forward) >= forward;
}

// W(n, k) of a retained k
template <class Ages>
AGX_HD int64_t priority_row_weight(const Ages &ages, int64_t k, int64_t cnt, int64_t lo, int32_t fs1, int32_t back, int32_t forward, int64_t stamp,
                                   uint32_t weight, uint32_t wmax) {
    return priority_accepted(ages, k, cnt, lo, fs1, back, forward) ? (int64_t)priority_effective(stamp, weight, k, wmax) : 0;
}

// the first position p of incl[0 .. len) with incl[p] > v; incl is an inclusive prefix sum (nondecreasing) with
// incl[len - 1] > v >= 0.  Positions of weight 0 (incl[p] == incl[p - 1]) are never found.
AGX_HD int32_t priority_find_row(const int64_t *incl, int32_t len, int64_t v) {
    int32_t lo = 0, hi = len - 1;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (incl[mid] > v)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

}  // namespace agx
