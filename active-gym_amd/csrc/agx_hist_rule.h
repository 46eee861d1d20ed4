// agx_hist_rule.h - which samples (env, index k) of the frame history (include/agx_history.h) are valid, as __host__ __device__
// functions: every reader of the history (agx_hist_plane.h, agx_k6_glimpse.h, agx_k8_steplog.h, agx_k11_sequence.h) and the plain
// C++ programs under tests/ decide it with these two.  Nothing here touches the GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef AGX_HD
#if defined(__HIPCC__)
#define AGX_HD __host__ __device__ inline
#else
#define AGX_HD inline
#endif
#endif

namespace agx {

// row k of an env with cnt appends so far is still retained in a history of T rows per env
AGX_HD bool hist_retained(int64_t k, int64_t cnt, int32_t T) { return k >= 0 && k < cnt && k >= cnt - T; }

// ... and so is the oldest row its stack of fs frames needs.  age_k = the age byte of row k, read only where
// hist_retained(k, cnt, T) holds.
AGX_HD bool hist_stack_ok(int64_t k, int64_t cnt, int32_t T, int32_t fs, int32_t age_k) {
    const int64_t first = k - (age_k < fs - 1 ? age_k : fs - 1);
    return first >= 0 && first >= cnt - T;
}

}  // namespace agx
