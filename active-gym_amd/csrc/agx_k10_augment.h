// agx_k10_augment.h - K10: random-shift augmentation on the frame history's observe (include/agx_augment.h).
// k_history_observe_shifted is k_history_observe's workgroup (agx_k5_history.h: hist_observe_plane) under the PlaneShift policy:
// every plane is moved by the sample's shift on the way out (what that means per mode: agx_hist_plane.h, hist_plane_write);
// k_shift_draw draws the shifts.  The shift map and the draw are agx_shift_math.h's.  Every device write is an ordinary vector
// store.
#pragma once
#include "agx_k5_history.h"
#include "agx_shift_math.h"

namespace agx {

struct ShiftObsParams {
    const int32_t *shift;     // i32 [B][2] (dy, dx)
    int32_t pad;
};

// ---------------------------------------------------------------------------------------------
// k_history_observe_shifted<G, MODE, OT>: grid = (fs, B), block = 256.  Workgroup (j, b) with the sample's (dy, dx): two more
// workgroup-uniform values through the scalar cache, clamped into 0 .. 2 * pad.
// ---------------------------------------------------------------------------------------------
template <class G, int MODE, class OT>
__global__ __launch_bounds__(kThreads) void k_history_observe_shifted(G g, FovParams p, HistObsParams q, ShiftObsParams sh) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // every row of d_shift is there, whatever the sample turns out to be
    const int2 d2 = uniform_load_i32x2(sh.shift + 2 * (size_t)blockIdx.y);
    hist_observe_plane<G, MODE, OT>(g, p, q, smem, PlaneShift{shift_clamp(d2.x, sh.pad), shift_clamp(d2.y, sh.pad), sh.pad});
}

// ---------------------------------------------------------------------------------------------
// k_shift_draw: grid = ceil(B / 256), one shift per thread, one launch.  Every thread reads (seed, calls) and forms the key;
// behind the workgroup's barrier thread 0 takes a ticket, and the workgroup that takes the last one - every other workgroup
// has read the state by then - advances calls and returns the ticket counter to zero: a replayed graph draws anew.
// (agx_k7_replay.h publishes the key in a launch of its own, in front of the draw; one launch cannot do that, because its
// workgroups start in no order - so the key is formed per thread, and what needs care is when `calls` may change.)
// state: u64 [3] = seed, calls, tickets.
// Why no workgroup can read the advanced `calls`: the last ticket is taken after every workgroup's thread 0 has passed its
// own barrier.  A wave arrives at that barrier only after its store of the shifts, whose data depends on the loaded `calls`, so
// the load has returned by then (a wave with no thread below B has no use for the value: its load may still be in flight, and
// whatever it returns is dropped).  The acq_rel ticket orders the store to `calls` behind the last ticket.  Nothing orders it
// against another stream: a source is used on one stream at a time, like the samplers.
// ---------------------------------------------------------------------------------------------
__global__ void k_shift_seed(uint64_t *state, uint64_t seed) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        state[0] = seed;
        state[1] = 0;
        state[2] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_shift_draw(uint64_t *state, int32_t pad, int32_t B, int32_t *shift_out) {
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t seed = __hip_atomic_load(state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t calls = __hip_atomic_load(state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b < B) {
        const ShiftPair s = shift_draw(shift_key(seed, calls), (uint64_t)b, pad);
        *reinterpret_cast<int2 *>(shift_out + 2 * b) = make_int2(s.dy, s.dx);
    }
    __syncthreads();                                      // every thread of the workgroup holds `calls` in a register
    if (threadIdx.x == 0) {
        unsigned long long *tickets = reinterpret_cast<unsigned long long *>(state + 2);
        const unsigned long long t = __hip_atomic_fetch_add(tickets, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (t == (unsigned long long)gridDim.x - 1) {
            __hip_atomic_store(state + 1, calls + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(tickets, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace agx
