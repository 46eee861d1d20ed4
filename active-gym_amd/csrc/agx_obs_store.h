// agx_obs_store.h - the written-through (sc1) observation stores every fovea kernel family shares: store_obs (one store unit of
// a full-size observation) and store_packed (one element of a raw crop).
#pragma once
#include "agx_common.h"

namespace agx {

// The observation is a write-once stream of 115 MB per launch.  Rounds 1 / 2 wrote it with nontemporal stores, so that the
// next launch (K1) does not queue behind ~115 MB of dirty L2 / Infinity-Cache lines (K1 ran ~6 us slower after plain stores).
// Round 3 measured the cache-policy bits on this very store shape (tools/storebench.hip, 115.6 MB, same box): nt 20.1 us
// (5.76 TB/s), plain 18.0 (6.41), sc0 18.0, **sc1 17.0 us (6.80 TB/s)**, sc1 nt 19.6.  An agent-scope (sc1) store is written
// through the XCD's L2 towards memory at once - nothing stays dirty behind the launch either.  In the real step (same box,
// bench.py's kernel events / us per step): K2 22.0 -> 19.9 / 52.5-53.1 -> 51.0-51.2; K3 24.5-25.0 -> 22.6-23.8 / 55.4-56.0 ->
// 53.4-55.2; K4 24.2-25.0 -> 22.0-22.4 / 55.1-56.3 -> 53.7-53.8; K1 behind them unchanged.
// A raw buffer store carries the bit (aux 16 = sc1 on gfx940+) and stays an ordinary store for the compiler (an inline-asm store
// does not: the hazard recogniser cannot see that its four data VGPRs must not be overwritten by the very next VALU
// instruction, and the first sc1 build produced a few hundred wrong observation values per launch that way).  One buffer
// resource per workgroup = its output frame: the pointer is wave-uniform by construction, out-of-range offsets are dropped.
template <class OT = float>
struct ObsOut {
    __amdgpu_buffer_rsrc_t rs;
#ifdef AGX_CANARY_ASM_OBS_STORE
    obs4_t<OT> *base;
#endif
};
template <class OT = float>
__device__ __forceinline__ ObsOut<OT> obs_out(obs4_t<OT> *frame, int n_float4) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(frame);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    void *p = reinterpret_cast<void *>(((uintptr_t)hi << 32) | lo);
    ObsOut<OT> o;
    o.rs = __builtin_amdgcn_make_buffer_rsrc(p, 0, n_float4 * (int)sizeof(obs4_t<OT>), 0x00027000);
#ifdef AGX_CANARY_ASM_OBS_STORE
    o.base = frame;
#endif
    return o;
}
template <class OT>
__device__ __forceinline__ void store_obs(const ObsOut<OT> &o, int q, const float4 &v) {
    if constexpr (sizeof(OT) == 2) {
        // 8 B per lane, written through like the f32 store (sc1 against plain at this width)
        typedef uint32_t u2v __attribute__((ext_vector_type(2)));
        const u2v w = {pack2<OT>(v.x, v.y), pack2<OT>(v.z, v.w)};
        __builtin_amdgcn_raw_buffer_store_b64(w, o.rs, q * 8, 0, 16 /* sc1 */);
    } else {
#ifdef AGX_CANARY_ASM_OBS_STORE
    // The KNOWN-BAD store of commit 327a14a, kept as a canary for the tests only (build.py: build_canary() ->
    // lib/libagx_canary.so, never loaded by the product): an inline-asm store is invisible to the compiler's hazard
    // recogniser, and on gfx940+ the data VGPRs of a store of more than 64 bits must not be overwritten by the VALU
    // instructions right behind it.  tests/test_gpu_lowocc.py must FAIL on this build (tools/canary_probe.py shows it).
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v w = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(o.base + q), "v"(w));
#else
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    const u4v w = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(w, o.rs, q * 16, 0, 16 /* sc1 */);
#endif
    }
}

// one float of a raw crop (fixed: [fh][fw]; flexible, packed: [rh][rw] at an arbitrary 4-byte aligned offset - hence dword stores),
// written through like the full-size observations: the crop of one stacked frame is the buffer.  16-bit OT (fixed crops only:
// the packed ragged form is f32-only): one short per element.
template <class OT = float>
struct PackedOut {
    __amdgpu_buffer_rsrc_t rs;
};
template <class OT = float>
__device__ __forceinline__ PackedOut<OT> packed_out(OT *crop, int n_floats) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(crop);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    void *q = reinterpret_cast<void *>(((uintptr_t)hi << 32) | lo);
    PackedOut<OT> o;
    o.rs = __builtin_amdgcn_make_buffer_rsrc(q, 0, crop ? n_floats * (int)sizeof(OT) : 0, 0x00027000);
    return o;
}
template <class OT>
__device__ __forceinline__ void store_packed(const PackedOut<OT> &o, int i, float v) {
    if constexpr (sizeof(OT) == 2) {
        const OT h = (OT)v;
        __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(uint16_t, h), o.rs, i * 2, 0, 16 /* sc1 */);
    } else {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), o.rs, i * 4, 0, 16 /* sc1 */);
    }
}

}  // namespace agx
