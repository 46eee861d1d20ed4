// agx_sequence_math.h - the length rule of a sequence on the frame history (include/agx_sequence.h), as __host__ __device__
// functions over an accessor argument: k_sequence_gather / k_sequence_lengths (agx_k11_sequence.h) decide every step with
// sequence_start_ok and sequence_breaks, and a plain C++ program (tests/sequence_harness.cpp) runs sequence_length, the loop
// over the very same two.  Nothing here touches the GPU.
#pragma once
#include "agx_steplog_fold.h"

namespace agx {

constexpr int32_t kSequenceLimit = 256;      // AGX_SEQUENCE_LIMIT

// (n, k) is valid by the history's own rule (agx_hist_rule.h): retained, and so is the oldest row its stack needs.  age_k = the
// age byte of row k, read only where steplog_ok0(k, cnt, T) holds; cnt = count[n].
AGX_HD bool sequence_start_ok(int64_t k, int64_t cnt, int32_t T, int32_t fs, int32_t age_k) {
    return hist_stack_ok(k, cnt, T, fs, age_k);
}

// Row j > k ends the sequence in front of it: the end of the history, or the first append of another episode.  rows.at(j) places
// row j of the sample's env and rows.age(r) reads its age byte; both are called for j < cnt only.
template <class Rows>
AGX_HD bool sequence_breaks(const Rows &rows, int64_t j, int64_t cnt) {
    return j >= cnt || rows.age(rows.at(j)) == 0;
}

// len of the sequence (env, k, L): 0 for an invalid start, else 1 + the number of steps behind k in front of the first break,
// at most L.  is_env: n names an env (cnt is 0 and no row is read otherwise).
template <class Rows>
AGX_HD int32_t sequence_length(const Rows &rows, bool is_env, int64_t k, int64_t cnt, int32_t T, int32_t fs, int32_t L) {
    if (!is_env || !steplog_ok0(k, cnt, T)) return 0;
    if (!sequence_start_ok(k, cnt, T, fs, rows.age(rows.at(k)))) return 0;
    int32_t len = 1;
    while (len < L && !sequence_breaks(rows, k + len, cnt)) ++len;
    return len;
}

}  // namespace agx
