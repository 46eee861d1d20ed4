// agx_common.h - constants, geometry descriptors and the small gfx950 helpers shared by every kernel family
// (scalar-cache loads, 24-bit multiplies, diagnostic stamps).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "agx.h"
#include "agx_taps.h"

namespace agx {

constexpr int kRawH = 210;
constexpr int kRawW = 160;
constexpr int kRawRowBytes = kRawW * 3;
constexpr int kRawFrameBytes = kRawH * kRawRowBytes;
constexpr int kThreads = 256;
// the band12 ingest form's LDS image (agx_k1_ingest.h: ingest_band12; agx_plan.h: band12_lds)
constexpr int kB12Rows = 12;
constexpr uint32_t kB12RowB = kRawW * 2;                                  // one u16 gray row
constexpr uint32_t kB12JobB = 2 * kB12RowB;                               // top + bottom source row of one output row
constexpr uint32_t kB12FrameB = kB12Rows * kB12JobB;
constexpr uint32_t kB12GrayB = 2 * kB12FrameB;                            // 15,360 B

// ---------------------------------------------------------------------------------------------
// geometry: compile-time for the headline 84x84 / 30x30 configuration, run-time otherwise
// ---------------------------------------------------------------------------------------------
template <int OH, int OW, int FH, int FW>
struct GeomS {
    __host__ __device__ constexpr int oh() const { return OH; }
    __host__ __device__ constexpr int ow() const { return OW; }
    __host__ __device__ constexpr int fh() const { return FH; }
    __host__ __device__ constexpr int fw() const { return FW; }
};
struct GeomR {
    int oh_, ow_, fh_, fw_;
    __host__ __device__ int oh() const { return oh_; }
    __host__ __device__ int ow() const { return ow_; }
    __host__ __device__ int fh() const { return fh_; }
    __host__ __device__ int fw() const { return fw_; }
};

// float32(k)/255 exactly as numpy's `state.astype(np.float32) / 255.` (atari_env.py:75):
// IEEE correctly-rounded single division (hipcc default -fhip-fp32-correctly-rounded-divide-sqrt;
// tests/test_gpu_parity.py checks all 256 values bit for bit).
__device__ __forceinline__ float unit(uint32_t k) { return (float)k / 255.0f; }
// the four bytes of a dword (k_full, k_history_observe's full-frame form)
__device__ __forceinline__ float4 unit4(uint32_t v) {
    return make_float4(unit(v & 0xFF), unit((v >> 8) & 0xFF), unit((v >> 16) & 0xFF), unit(v >> 24));
}


// float32(k) / 255 correctly rounded without the division sequence: q = k * y, r = k - 255 q (exact in an FMA),
// q + r * y with y = RN(1/255) (Markstein).  tests/host_tables_harness.cpp and the GPU parity tests check all 256
// values bit for bit against the IEEE quotient.
__host__ __device__ __forceinline__ float unit_fast(float k) {
    const float y = 1.0f / 255.0f;
    const float q = k * y;
    const float r = fmaf(-q, 255.0f, k);
    return fmaf(r, y, q);
}

// Observation element type OT (agx_config.out_mode bits AGX_OBS_*): float (the default and the reference's), __bf16 or
// _Float16.  The arithmetic is the f32 path's whatever OT; each value is rounded to nearest-even once, at the store (bf16: a
// plain cast, v_cvt_pk_bf16_f32; f16: v_cvt_f16_f32 in the default round-to-nearest mode with f16 denormals kept), so a
// 16-bit observation is bit for bit the f32 observation cast to OT.  One store unit = 4 outputs: a float4 (16 B per lane)
// at f32, 8 B per lane at 16 bits (obs4_t); the stores: store_obs in agx_obs_store.h, k_full in agx_k0_stack.h, lane-linear as before.
template <class OT>
using obs4_t = typename std::conditional<sizeof(OT) == 4, float4, uint2>::type;
template <class OT>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    const OT ha = (OT)a, hb = (OT)b;
    return (uint32_t)__builtin_bit_cast(uint16_t, ha) | ((uint32_t)__builtin_bit_cast(uint16_t, hb) << 16);
}

// Wave-uniform byte through the scalar cache.  hipcc emits a VECTOR load + s_waitcnt vmcnt(0) for
// `p.cmd[n]` (it cannot prove the buffer read-only), i.e. a full memory round trip in front of the
// first frame load of every workgroup; s_load_dword is counted on lgkmcnt and served by the scalar
// cache.  Reads the aligned dword that contains the byte (same 4-byte word, never crosses a page).
__device__ __forceinline__ uint32_t uniform_load_u8(const uint8_t *ptr) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
    const uint32_t *aligned = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
    uint32_t w;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(aligned) : "memory");
    return (w >> (8 * (uint32_t)(a & 3))) & 0xFFu;
}
// The wider forms, same contract: wave-uniform, naturally aligned, written by an earlier launch.
__device__ __forceinline__ int32_t uniform_load_i32(const int32_t *ptr) {
    int32_t w;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(ptr) : "memory");
    return w;
}
__device__ __forceinline__ int2 uniform_load_i32x2(const int32_t *ptr) {
    int2 w;
    asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(ptr) : "memory");
    return w;
}
__device__ __forceinline__ int64_t uniform_load_i64(const int64_t *ptr) {
    int2 w;
    asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(ptr) : "memory");
    return (int64_t)(((uint64_t)(uint32_t)w.y << 32) | (uint32_t)w.x);
}
// the age byte and the fov_loc of one history row (agx_k5_history.h), one wait
__device__ __forceinline__ void uniform_load_age_loc(const uint8_t *age, const int32_t *loc, int &a, int2 &rc) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(age);
    const uint32_t *aligned = reinterpret_cast<const uint32_t *>(at & ~(uintptr_t)3);
    uint32_t w;
    asm volatile("s_load_dword %0, %2, 0x0\n\ts_load_dwordx2 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(w), "=&s"(rc)
                 : "s"(aligned), "s"(loc)
                 : "memory");
    a = (int)((w >> (8 * (uint32_t)(at & 3))) & 0xFFu);
}
// 24-bit multiply at full rate.  hipcc lowers __mul24 / __umul24 to the quarter-rate v_mul_lo_u32
// whenever it cannot prove the operand ranges itself; every product on this path fits (operands < 2^24,
// result < 2^32).
__device__ __forceinline__ uint32_t mul_u24(uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_mul_u32_u24_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// (a[23:0] * b[23:0]) >> 32
__device__ __forceinline__ uint32_t mul_hi_u24(uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}


// i / d for 0 <= i < 2^20 and 1 <= d <= 1024 (agx_create caps obs at 1024 x 1024), exact: floor((i + 0.5) * (1/d)) in f32 - three full-rate VALU operations
// where a run-time 32-bit integer division is ~35 (K4 spent most of its 1.5 k VALU instructions per wave on them).
// The distance of (i + 0.5)/d from an integer is >= 0.5/d, the f32 error of the product is < (i + 0.5) * 2^-22 / d:
// exact for i < 2^21; verified exhaustively over the stated range, also with a reciprocal 1 ulp off (v_rcp_f32).
struct FastDiv {
    float rcp;
    int d;
    __device__ __forceinline__ explicit FastDiv(int d_) : rcp(__builtin_amdgcn_rcpf((float)d_)), d(d_) {}
    __device__ __forceinline__ int div(int i) const { return (int)(((float)i + 0.5f) * rcp); }
    __device__ __forceinline__ void divmod(int i, int &q, int &r) const {
        q = div(i);
        r = i - q * d;
    }
};

#ifdef AGX_STAMPS
// slot 5 of every wave's record holds where it ran: XCC_ID | HW_ID << 8 (se/cu/simd/wave slot)
#define AGX_STAMP(i)                                                                              \
    do {                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        unsigned long long t_;                                                                    \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        if (p.stamps && (threadIdx.x & 63) == 0) {                                                \
            unsigned long long *rec_ = p.stamps +                                                 \
                (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (T / 64) + (threadIdx.x >> 6)) * 8; \
            rec_[(i)] = t_;                                                                       \
            if ((i) == 0) {                                                                       \
                unsigned xcc_, hw_;                                                               \
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));               \
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));                 \
                unsigned long long rt_;                                                           \
                asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_)::"memory");  \
                rec_[5] = ((unsigned long long)hw_ << 8) | (xcc_ & 0xFF);                         \
                rec_[6] = rt_;                                                                    \
            }                                                                                     \
            if ((i) == 4) {                                                                       \
                unsigned long long rt_;                                                           \
                asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_)::"memory");  \
                rec_[7] = rt_;                                                                    \
            }                                                                                     \
        }                                                                                         \
    } while (0)
#else
#define AGX_STAMP(i) do {} while (0)
#endif

}  // namespace agx
