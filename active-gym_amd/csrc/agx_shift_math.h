// agx_shift_math.h - the shift map and the draw arithmetic of the random-shift augmentation (include/agx_augment.h), as
// __host__ __device__ functions: the kernels of agx_k10_augment.h and a plain C++ program (tests/shift_harness.cpp) run the very
// same code.  Integers only; nothing here touches the GPU.
#pragma once
#include "agx_replay_draw.h"

namespace agx {

// a shift component as the device takes it: clamped into 0 .. 2 * pad
AGX_HD int32_t shift_clamp(int32_t d, int32_t pad) { return d < 0 ? 0 : (d > 2 * pad ? 2 * pad : d); }

// the source coordinate of output coordinate i under shift d (0 .. 2 * pad) along an axis of n elements: replicate-pad by pad,
// crop at offset d
AGX_HD int32_t shift_src(int32_t i, int32_t d, int32_t pad, int32_t n) {
    const int32_t s = i + d - pad;
    return s < 0 ? 0 : (s > n - 1 ? n - 1 : s);
}

// the key of a draw: SM(seed, calls)
AGX_HD uint64_t shift_key(uint64_t seed, uint64_t calls) { return replay_sm(seed, calls); }

// sample b of the draw with `key`: the halves of z = SM(key, b), each mapped onto 0 .. 2 * pad by a multiply-high
struct ShiftPair {
    int32_t dy, dx;
};
AGX_HD ShiftPair shift_draw(uint64_t key, uint64_t b, int32_t pad) {
    const uint64_t z = replay_sm(key, b), m = (uint64_t)(2 * pad + 1);
    ShiftPair s;
    s.dy = (int32_t)(((z >> 32) * m) >> 32);
    s.dx = (int32_t)(((z & 0xFFFFFFFFull) * m) >> 32);
    return s;
}

}  // namespace agx
