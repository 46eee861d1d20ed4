// agx_range.h - launches over a range of envs (agx_env_range, include/agx_hostout.h): the one kernel they add.
//
// The range itself reaches the kernels on the HOST: every per-env array is a whole number of elements per env, so an entry
// point advances its base pointers by `lo` envs and shrinks the grid's env dimension to `n` - the kernels, and with the default
// range their arguments and grids, are what they were.  What is left is the double-buffered state (ring heads, fov_loc, fov_res):
// a launch reads buffer `cur` and writes buffer `cur ^ 1` for the envs it runs over, then the context flips.  k_range_carry
// copies the entries of the envs OUTSIDE the range from `cur` to `cur ^ 1` in front of the flip, so that every env's state is
// current in the buffer the next call reads, whatever order the ranges come in.  (A launch of its own: the fovea kernels read
// the state through the scalar cache, which is coherent at kernel boundaries only - agx_fov_common.h.)
#pragma once
#include "agx_common.h"

namespace agx {

struct RangeCarryParams {
    const int32_t *src[2];   // up to two arrays of `words` i32 per env (second may be null)
    int32_t *dst[2];
    int32_t words;           // 1 (head) | 2 (fov_loc, fov_res)
    int32_t lo, n, total;    // envs [lo, lo + n) are skipped; total = num_envs
};
// grid = ceil(total * words / 256)
__global__ __launch_bounds__(kThreads) void k_range_carry(RangeCarryParams p) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.total * p.words) return;
    const int env = p.words == 2 ? i >> 1 : i;
    if (env >= p.lo && env < p.lo + p.n) return;
    p.dst[0][i] = p.src[0][i];
    if (p.src[1]) p.dst[1][i] = p.src[1][i];
}

}  // namespace agx
