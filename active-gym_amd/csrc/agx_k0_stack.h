// agx_k0_stack.h - K0: ring <-> stack order (k_stack_u8, k_set_stack, k_full).
#pragma once
#include "agx_common.h"

namespace agx {

// ---------------------------------------------------------------------------------------------
// K0: stack-order views of the ring
// ---------------------------------------------------------------------------------------------
struct StackParams {
    uint8_t *ring;
    int32_t *head;           // current head (read), or written by k_set_stack
    const uint8_t *in_u8;
    uint8_t *out_u8;
    float *out_f32;
    int32_t words, fs;       // words = oh*ow/4
};

// grid = (ceil(words/256), NC * fs, N).  NC = planes per frame (1: gray, 3: colour, AGX_FRAME_RGB): env n's ring holds
// NC * fs planes, frame slot s as planes s * NC .. s * NC + NC - 1; stack-order plane y = k * NC + ch is ring plane
// ((head + k) % fs) * NC + ch.  With NC = 1 every expression below folds to the gray form.
template <int NC = 1>
__global__ __launch_bounds__(kThreads) void k_stack_u8(StackParams p) {
    const int n = blockIdx.z, y = blockIdx.y, j = y / NC, ch = y - j * NC;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.words) return;
    int slot = p.head[n] + j;
    if (slot >= p.fs) slot -= p.fs;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(p.ring) + (((size_t)n * p.fs + slot) * NC + ch) * p.words;
    reinterpret_cast<uint32_t *>(p.out_u8)[((size_t)n * p.fs * NC + y) * p.words + i] = src[i];
}

template <int NC = 1>
__global__ __launch_bounds__(kThreads) void k_set_stack(StackParams p) {
    const int n = blockIdx.z, y = blockIdx.y;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i == 0 && y == 0) p.head[n] = 0;
    if (i >= p.words) return;
    const size_t o = ((size_t)n * p.fs * NC + y) * p.words + i;
    reinterpret_cast<uint32_t *>(p.ring)[o] = reinterpret_cast<const uint32_t *>(p.in_u8)[o];
}

// OT: the observation element type (agx_common.h, obs4_t): at 16 bits each lane stores its 4 outputs as 8 B, lane-linear
template <class OT = float, int NC = 1>
__global__ __launch_bounds__(kThreads) void k_full(StackParams p) {
    const int n = blockIdx.z, y = blockIdx.y, j = y / NC, ch = y - j * NC;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.words) return;
    int slot = p.head[n] + j;
    if (slot >= p.fs) slot -= p.fs;
    const uint32_t v = (reinterpret_cast<const uint32_t *>(p.ring) + (((size_t)n * p.fs + slot) * NC + ch) * p.words)[i];
    const float4 o = unit4(v);
    // write-once observation stream: written through (sc1) like the fovea kernels' (store_obs, agx_obs_store.h); the frame of
    // (n, y) is the buffer - wave-uniform by construction
    const uintptr_t a = reinterpret_cast<uintptr_t>(reinterpret_cast<obs4_t<OT> *>(p.out_f32) + ((size_t)n * p.fs * NC + y) * p.words);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((uintptr_t)hi << 32) | lo), 0,
                                                                        p.words * (int)sizeof(obs4_t<OT>), 0x00027000);
    if constexpr (sizeof(OT) == 2) {
        typedef uint32_t u2v __attribute__((ext_vector_type(2)));
        const u2v w = {pack2<OT>(o.x, o.y), pack2<OT>(o.z, o.w)};
        __builtin_amdgcn_raw_buffer_store_b64(w, rs, i * 8, 0, 16 /* sc1 */);
    } else {
        typedef uint32_t u4v __attribute__((ext_vector_type(4)));
        const u4v w = {__float_as_uint(o.x), __float_as_uint(o.y), __float_as_uint(o.z), __float_as_uint(o.w)};
        __builtin_amdgcn_raw_buffer_store_b128(w, rs, i * 16, 0, 16 /* sc1 */);
    }
}

}  // namespace agx
