// agx_fixed_phases.h - the phases of the fixed fovea, each stated once: the LDS carve, the window and ytab staging, the
// raw-crop and mask-out writes, the horizontal pass (phase C) and the vertical lerp (phase D), and the shift policy the tap
// lookups take.  K2 (agx_k2_fixed.h) runs them on a ring slot; the history readers' plane body (agx_hist_plane.h: K5, K10, K11)
// and K6 (agx_k6_glimpse.h) on rows of the frame history: the same arithmetic on the same bytes, so what they write is bit for
// bit what K2 wrote.
#pragma once
#include "agx_common.h"
#include "agx_glimpse.h"
#include "agx_obs_store.h"
#include "agx_shift_math.h"

namespace agx {

// ---- LDS carve: `windows` window images u8 [fh][ow] (16-B padded each) | ytab[oh] | H[fh][ow] (and whatever the caller keeps
// behind it).  fixed_pad is the one expression of the padded window bytes (agx_plan.h: fixed_lds, memory_lds).
__host__ __device__ constexpr int fixed_pad(int fh, int ow) { return (fh * ow + 15) & ~15; }
constexpr int kMemTableBytes = AGX_GLIMPSE_LIMIT * 16;   // K6: the glimpse table int2[AGX_GLIMPSE_LIMIT] in front of the carve
struct FixedCarve {
    unsigned char *raw;
    Tap *ytab_s;
    float *H;
};
// (host too: tests/host_tables_harness.cpp holds K6's region ends against agx_plan.h's memory_lds)
__host__ __device__ __forceinline__ FixedCarve fixed_carve(unsigned char *raw, int oh, int ow, int fh, int windows = 1) {
    Tap *ytab_s = reinterpret_cast<Tap *>(raw + windows * fixed_pad(fh, ow));
    return {raw, ytab_s, reinterpret_cast<float *>(ytab_s + oh)};
}

// ---- window staging: the (fh * ow) / 4 dwords of the fh window rows, wsrc -> LDS image.  A thread issues kWinRegs loads into
// registers (window_reg, k = 0 .. kWinRegs - 1: dword tid + k * kThreads, clamped to the window), window_land writes them to LDS
// once whatever the caller wants in flight with them is out, and window_tail copies the dwords beyond kWinRegs * kThreads
// (none at the headline geometry).  zero: no source - a frame that is known to be zeros.  COHERENT: agent-scope loads
// (fovea_fixed_body).
constexpr int kWinRegs = 3;
template <bool COHERENT>
__device__ __forceinline__ uint32_t window_word(const uint32_t *q, bool zero) {
    if (zero) return 0u;
    return COHERENT ? __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *q;
}
template <bool COHERENT = false>
__device__ __forceinline__ uint32_t window_reg(const uint32_t *wsrc, int k, int wwords, int tid, bool zero = false) {
    return window_word<COHERENT>(wsrc + min(tid + k * kThreads, wwords - 1), zero);
}
__device__ __forceinline__ void window_land(unsigned char *raw, const uint32_t (&ww)[kWinRegs], int wwords, int tid) {
#pragma unroll
    for (int k = 0; k < kWinRegs; ++k)
        if (tid + k * kThreads < wwords) reinterpret_cast<uint32_t *>(raw)[tid + k * kThreads] = ww[k];
}
template <bool COHERENT = false>
__device__ __forceinline__ void window_tail(unsigned char *raw, const uint32_t *wsrc, int wwords, int tid, bool zero = false) {
    for (int i = tid + kWinRegs * kThreads; i < wwords; i += kThreads) reinterpret_cast<uint32_t *>(raw)[i] = window_word<COHERENT>(wsrc + i, zero);
}

// ---- the shift policy of a plane, a compile-time choice.  NoShift (K2, K5, K6, K11) is empty: row(y, n) and col(x, n) are y and
// x, and nothing of a shift is left in the code.  PlaneShift (K10): output row y of an axis of n rows takes source row
// shift_src(y, dy, pad, n), output column x source column shift_src(x, dx, pad, n) - in RESIZE a move of whole H columns (the tap
// of the source column) and of whole output rows (the row tap of the source row), so the arithmetic of phase C / D and its bits
// are unchanged.
struct NoShift {
    static constexpr bool shifted = false;
    __device__ __forceinline__ int row(int y, int) const { return y; }
    __device__ __forceinline__ int col(int x, int) const { return x; }
};
struct PlaneShift {
    static constexpr bool shifted = true;
    int dy, dx, pad;                                       // dy, dx in 0 .. 2 * pad
    __device__ __forceinline__ int row(int y, int n) const { return shift_src(y, dy, pad, n); }
    __device__ __forceinline__ int col(int x, int n) const { return shift_src(x, dx, pad, n); }
};

// ---- ytab staging: yt0 = this thread's row tap {lo, aux, a, b}, already in a register (ytab[sh.row(min(tid, oh - 1), oh)])
template <class SHIFT = NoShift>
__device__ __forceinline__ void ytab_stage(Tap *ytab_s, const int4 &yt0, const Tap *ytab, int oh, int tid, const SHIFT &sh = {}) {
    if (tid < oh) *reinterpret_cast<int4 *>(ytab_s + tid) = yt0;
    for (int i = tid + kThreads; i < oh; i += kThreads) ytab_s[i] = ytab[sh.row(i, oh)];
}

// ---- the raw crop [fh][fw] of the window at `win` (row pitch ow)
template <class OT>
__device__ __forceinline__ void raw_crop_write(OT *crop, const unsigned char *win, int ow, int fh, int fw, int tid) {
    const auto cout = packed_out<OT>(crop, fh * fw);
    for (int i = tid; i < fh * fw; i += kThreads) {
        const int y = i / fw, x = i - y * fw;
        store_packed(cout, i, unit_fast((float)win[y * ow + x]));
    }
}

// ---- mask-out: the window at (r, c) inside a zero frame; raw = its LDS image (row r of the frame = row 0)
template <class OT>
__device__ __forceinline__ void mask_out_write(const ObsOut<OT> &oout, const unsigned char *raw, int r, int c, int oh, int ow, int fh,
                                               int fw, int tid) {
    const int ow4 = ow >> 2;
    for (int k_ = 0; k_ < (oh * ow4 + kThreads - 1) / kThreads; ++k_) {
        const int q = tid + k_ * kThreads;
        if (q >= oh * ow4) break;
        const int row = q / ow4, x = (q - row * ow4) * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (row >= r && row < r + fh && x + 3 >= c && x < c + fw) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(raw + (row - r) * ow + x);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k >= c && x + k < c + fw) v[k] = unit_fast((float)((w >> (8 * k)) & 0xFF));
        }
        store_obs(oout, q, make_float4(v[0], v[1], v[2], v[3]));
    }
}

// ---- RESIZE, phase C: H[fh][ow] = horizontal lerp of the window rows.  A thread owns column xcol = tid % ow (its taps xt =
// xtab[sh.col(xcol, ow)] in registers), rows yb = tid / ow, yb + rstep, ...
template <class SHIFT = NoShift>
__device__ __forceinline__ void phase_c(float *H, const unsigned char *win, const int4 &xt, const Tap *xtab, int ow, int fh, int xcol,
                                        int yb, int tid, const SHIFT &sh = {}) {
    const int rstep = kThreads / ow;                                  // 3 for ow = 84
    if (rstep > 0) {
        if (yb < rstep) {
            const unsigned char *c0 = win + xt.x, *c1 = win + xt.y;
            const float wa = __int_as_float(xt.z), wb = __int_as_float(xt.w);
#pragma unroll 10
            for (int y = yb; y < fh; y += rstep)
                // u8 -> float32 k/255 by unit_fast (3 FMAs, the correctly rounded quotient) rather than through the LDS table:
                // one LDS round trip less in the chain byte -> value -> lerp (23.0-23.4 vs 23.2-23.8 us, a tie at worst)
                H[y * ow + xcol] = fmaf(wb, unit_fast((float)c1[y * ow]), wa * unit_fast((float)c0[y * ow]));
        }
    } else {                                                          // ow > 256: generic striding
        for (int i = tid; i < fh * ow; i += kThreads) {
            const int y = i / ow, x = i - y * ow;
            const Tap t = xtab[sh.col(x, ow)];
            H[i] = fmaf(t.b, unit_fast((float)win[y * ow + t.aux]), t.a * unit_fast((float)win[y * ow + t.lo]));
        }
    }
}

// ---- phase D, one output quad q: the vertical lerp of two ds_read_b128
__device__ __forceinline__ float4 phase_d_quad(const float4 *H4, const Tap *ytab_s, int q, int ow4) {
    const int row = q / ow4, x4 = q - row * ow4;
    const Tap t = ytab_s[row];
    const float4 a = H4[t.lo * ow4 + x4];
    const float4 b = H4[t.aux * ow4 + x4];
    // the lerp is written as mul + fma explicitly: every instantiation of this body (stand-alone, pair, fused, per-env
    // step, history, glimpse) then rounds the same way whatever contraction the optimiser would pick in its context
    float4 o;
    o.x = fmaf(t.b, b.x, t.a * a.x);
    o.y = fmaf(t.b, b.y, t.a * a.y);
    o.z = fmaf(t.b, b.z, t.a * a.z);
    o.w = fmaf(t.b, b.w, t.a * a.w);
    return o;
}
// the whole frame: 16 B per lane, lane-linear, written through
template <class OT>
__device__ __forceinline__ void phase_d_write(const ObsOut<OT> &oout, const float *H, const Tap *ytab_s, int oh, int ow4, int tid) {
    const float4 *H4 = reinterpret_cast<const float4 *>(H);
    // (a uniform trip count with the bound tested inside: inline asm is convergent, and a loop whose trip count differs per
    //  thread cannot be unrolled around it - with the compile-time geometry all 7 passes unroll and their LDS reads batch up)
    const int nq = oh * ow4, passes = (nq + kThreads - 1) / kThreads;
#pragma unroll 7
    for (int k = 0; k < passes; ++k) {
        const int q = tid + k * kThreads;
        if (q >= nq) break;
        store_obs(oout, q, phase_d_quad(H4, ytab_s, q, ow4));
    }
}

}  // namespace agx
