// agx_hist_plane.h - the frame history as its readers see it, each piece stated once: the storage (HistParams), the resolution of
// a sample (env n, index k) by the validity rule of agx_hist_rule.h, the source row of stack position j, the position of the
// window, and the write of one observation plane by the fixed fovea's phases (agx_fixed_phases.h, the ones K2 runs).
// k_history_observe (agx_k5_history.h), k_history_observe_shifted (agx_k10_augment.h) and k_sequence_observe
// (agx_k11_sequence.h) are this body under their own indexing and shift policy, so a plane of a sample at its recorded fov_loc is
// bit for bit the step's whichever of them writes it.  A new reader supplies: which (n, k, j) a workgroup owns, where its plane
// and its fov_loc row go, its own valid byte, and a shift policy (NoShift unless it moves planes).
#pragma once
#include "agx_fixed_phases.h"
#include "agx_fov_common.h"
#include "agx_hist_rule.h"

namespace agx {

// Rows are indexed [t][n], t = index mod T.
struct HistParams {
    uint8_t *frames;     // u8  [T][N][fbytes]
    uint8_t *age;        // u8  [T][N]   appends since the env's last CLEAR, saturating at 255
    int32_t *loc;        // i32 [T][N][2]
    int64_t *count;      // i64 [N]      appends so far == the next index
    int32_t T, N, fs, fbytes;
    int32_t start_age;   // the "previous age" of an env's first append: -1 (new history: zeros before it) or 254 (after a
                         // clear: unknown frames before it, so its first fs - 1 samples stay invalid until a CLEAR)
};

// index mod T (indices below 2^31 - every history younger than two billion appends per env - take the 32-bit form)
__device__ __forceinline__ int hist_row(int64_t k, int T) {
    return (k >> 31) == 0 ? (int)((uint32_t)k % (uint32_t)T) : (int)(k % T);
}

// ---- the sample.  Everything is workgroup-uniform and comes through the scalar cache.
// hist_at: n is an env and row k is still retained; cnt = the env's appends so far (0 if n is no env).  hist_sample: sample b of
// a call's (env, index) arrays.
struct HistSample {
    int n;
    int64_t k, cnt;
    bool ok;
};
__device__ __forceinline__ HistSample hist_at(const HistParams &h, int n, int64_t k) {
    HistSample s{n, k, 0, false};
    if (n >= 0 && n < h.N && k >= 0) {
        s.cnt = uniform_load_i64(h.count + n);
        s.ok = hist_retained(k, s.cnt, h.T);
    }
    return s;
}
__device__ __forceinline__ HistSample hist_sample(const int32_t *env, const int64_t *index, const HistParams &h, int b) {
    return hist_at(h, uniform_load_i32(env + b), uniform_load_i64(index + b));
}
// hist_resolve: ... and so is the oldest row the stack of row k needs.  row_k = k mod T, age = its age byte (0 unless retained).
struct HistStack {
    bool ok;
    int row_k, age;
    int64_t cnt;
};
__device__ __forceinline__ HistStack hist_resolve(const HistParams &h, int n, int64_t k) {
    const HistSample s = hist_at(h, n, k);
    HistStack st{false, 0, 0, s.cnt};
    if (s.ok) {
        st.row_k = hist_row(k, h.T);
        st.age = (int)uniform_load_u8(h.age + (size_t)st.row_k * h.N + n);
        st.ok = hist_stack_ok(k, s.cnt, h.T, h.fs, st.age);
    }
    return st;
}

// ---- the source of stack position j (fs - 1 = row k itself): the frame of history row k - (fs-1-j), or nothing - a frame older
// than the env's last CLEAR, whose image is zeros.  The frame's bytes come from the geometry (h.fbytes: a compile-time value
// where the geometry is one).
struct HistPlaneSrc {
    const uint32_t *fsrc;
    bool zero;
};
template <class G>
__device__ __forceinline__ HistPlaneSrc hist_plane_src(const G &g, const HistParams &h, const HistStack &st, int n, int j) {
    const int back = h.fs - 1 - j;
    int row = st.row_k - back;                            // back <= fs - 1 < T
    if (row < 0) row += h.T;
    return {reinterpret_cast<const uint32_t *>(h.frames + ((size_t)row * h.N + n) * (size_t)(g.oh() * g.ow())), back > st.age};
}

// ---- RESIZE: this thread's taps, xtab[column tid % ow] and ytab[row min(tid, oh - 1)] under the shift policy.  They go out
// first, as in K2 (a shifted reader's wait for its shift: one scalar hop).
struct HistTaps {
    int4 xt, yt0;
};
template <int MODE, class SHIFT>
__device__ __forceinline__ HistTaps hist_taps(const FovParams &p, int oh, int ow, int tid, const SHIFT &sh) {
    HistTaps t{make_int4(0, 0, 0, 0), make_int4(0, 0, 0, 0)};
    if (MODE == AGX_OUT_RESIZE) {
        t.xt = *reinterpret_cast<const int4 *>(p.xtab + sh.col(tid % ow, ow));
        t.yt0 = *reinterpret_cast<const int4 *>(p.ytab + sh.row(min(tid, oh - 1), oh));
    }
    return t;
}

// ---- position: the recorded fov_loc of row (row_k, n), or - ACTION - the read-time action of row b through compute_loc (K2's
// arithmetic; FovParams carries what K2's carries, relative = 0: a read-time action is absolute).  first: this thread writes
// the position to row `out_row` of user_loc (a shift is not reflected in it).  A context without a fovea (has_loc = 0): (0, 0).
template <bool ACTION, class ROW>
__device__ __forceinline__ void hist_position(const FovParams &p, const HistParams &h, int has_loc, int row_k, int n, int b, int bound_r,
                                              int bound_c, bool first, ROW out_row, int &r, int &c) {
    r = c = 0;
    if (!has_loc) return;
    const int2 rc = uniform_load_i32x2(h.loc + 2 * ((size_t)row_k * h.N + n));
    r = rc.x;
    c = rc.y;
    if constexpr (ACTION) {
        LocIn lin;
        lin.r = rc.x;
        lin.c = rc.y;
        lin.w[0] = lin.w[1] = lin.w[2] = lin.w[3] = 0u;
        if (p.action) {
            const bool wide = p.action_dt == AGX_DT_F64 || p.action_dt == AGX_DT_I64;
            const char *base = static_cast<const char *>(p.action) + (size_t)b * (wide ? 16 : 8);
            const int2 a0 = uniform_load_i32x2(reinterpret_cast<const int32_t *>(base));
            const int2 a1 = uniform_load_i32x2(reinterpret_cast<const int32_t *>(base + (wide ? 8 : 0)));
            lin.w[0] = (uint32_t)a0.x;
            lin.w[1] = wide ? (uint32_t)a0.y : 0u;
            lin.w[2] = wide ? (uint32_t)a1.x : (uint32_t)a0.y;
            lin.w[3] = wide ? (uint32_t)a1.y : 0u;
        }
        compute_loc(p, lin, bound_r, bound_c, r, c);
        r = __builtin_amdgcn_readfirstlane(r);
        c = __builtin_amdgcn_readfirstlane(c);
    }
    // a recorded fov_loc is in range unless the caller set one that is not (agx_set_fov_state): the window stays inside the frame
    r = min(max(r, 0), bound_r);
    c = min(max(c, 0), bound_c);
    if (first && p.user_loc) {
        p.user_loc[2 * out_row] = r;
        p.user_loc[2 * out_row + 1] = c;
    }
}

// ---- the plane.  MODE = AGX_OUT_RAW / AGX_OUT_RESIZE / AGX_OUT_MASK, or kHistFull: the full-frame k/255 write of k_full.
constexpr int kHistFull = 3;   // next to AGX_OUT_RAW / AGX_OUT_RESIZE / AGX_OUT_MASK (0, 1, 2)
static_assert(AGX_OUT_RAW != kHistFull && AGX_OUT_RESIZE != kHistFull && AGX_OUT_MASK != kHistFull, "kHistFull must not be an AGX_OUT_* value");

// elements of one plane: the crop [fh][fw] in raw mode, the frame [oh][ow] otherwise
template <int MODE, class G>
__device__ __forceinline__ int hist_plane_elems(const G &g) {
    return MODE == AGX_OUT_RAW ? g.fh() * g.fw() : g.oh() * g.ow();
}

// hist_plane_write<G, MODE, OT>: all 256 threads of the workgroup write plane `plane` from the frame `src` with the window at
// (r, c): the fh window rows go to LDS (FixedCarve at smem: agx_plan.h's fixed_lds; kHistFull takes no LDS and no barrier - a
// frame of 1024 x 1024 would not fit), then the mode's tail runs.  Under PlaneShift, with cy(y) = sh.row(y, rows) and cx(x) =
// sh.col(x, columns), output element (y, x) is element (cy(y), cx(x)) of the unshifted plane:
//   RESIZE    the shift is in the taps (hist_taps, ytab_stage, phase_c): phase C and phase D run as they are - the same mul + fma
//             on the same operands, the same bits - and the store stream is the unshifted one.
//   MASK      per output element the byte of the LDS window image at (cy(y) - r, cx(x)), or zero outside the window; shifted
//             columns are not dword-aligned, so these are byte reads.  The stores are the 16-B quads of mask_out_write.
//   RAW       the crop [fh][fw] is the plane: byte (cy(y), cx(x)) of the window, clamped to the crop.
//   kHistFull byte cy(y) * ow + cx(x) of the history row, read from L2.  A quad whose columns are not clamped takes its four
//             bytes from the two aligned dwords around them (v_alignbyte); a quad at the edge reads bytes.
template <class G, int MODE, class OT, class SHIFT>
__device__ __forceinline__ void hist_plane_write(const G &g, const FovParams &p, unsigned char *smem, const HistPlaneSrc &src, int r, int c,
                                                 const HistTaps &taps, OT *plane, const SHIFT &sh) {
    const int tid = threadIdx.x;
    const int oh = g.oh(), ow = g.ow(), fh = g.fh(), fw = g.fw();
    const int ow4 = ow >> 2, nq = oh * ow4;
    const uint32_t *fsrc = src.fsrc;
    const bool zero = src.zero;
    const auto quads = [&] { return obs_out<OT>(reinterpret_cast<obs4_t<OT> *>(plane), nq); };      // (every mode but RAW)
    if (MODE == kHistFull) {
        // the base observation: k_full's arithmetic (unit: the IEEE quotient) and its written-through store
        const auto oout = quads();
        for (int i = tid; i < nq; i += kThreads) {
            if constexpr (!SHIFT::shifted) {
                store_obs(oout, i, unit4(zero ? 0u : fsrc[i]));
            } else {
                const uint8_t *fbyte = reinterpret_cast<const uint8_t *>(fsrc);
                const int y = i / ow4, x = (i - y * ow4) * 4;
                uint32_t w = 0u;                                         // the quad's four source bytes, as k_full's dword holds them
                if (!zero) {
                    const int so = sh.row(y, oh) * ow, x0 = x + sh.dx - sh.pad;
                    if (x0 >= 0 && x0 + 3 < ow) {
                        // no column clamps: four consecutive bytes at an offset that is not dword-aligned - the two aligned
                        // dwords around them (the second one clamped into the frame: it is not used where it would lie outside)
                        const int o = so + x0, wi = o >> 2;
                        w = __builtin_amdgcn_alignbyte(fsrc[min(wi + 1, nq - 1)], fsrc[wi], (uint32_t)(o & 3));
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) w |= (uint32_t)fbyte[so + sh.col(x + e, ow)] << (8 * e);
                    }
                }
                store_obs(oout, i, unit4(w));
            }
        }
        return;
    }
    const FixedCarve lds = fixed_carve(smem, oh, ow, fh);
    {
        const uint32_t *wsrc = fsrc + r * ow4;
        const int wwords = (fh * ow) >> 2;
        uint32_t ww[kWinRegs];
#pragma unroll
        for (int i = 0; i < kWinRegs; ++i) ww[i] = window_reg(wsrc, i, wwords, tid, zero);
        if (MODE == AGX_OUT_RESIZE) ytab_stage(lds.ytab_s, taps.yt0, p.ytab, oh, tid, sh);
        window_land(lds.raw, ww, wwords, tid);
        window_tail(lds.raw, wsrc, wwords, tid, zero);
        __syncthreads();
    }
    const unsigned char *win = lds.raw + c;
    if (MODE == AGX_OUT_RAW) {
        if constexpr (!SHIFT::shifted) {
            raw_crop_write(plane, win, ow, fh, fw, tid);
        } else {
            const auto cout = packed_out<OT>(plane, fh * fw);
            for (int i = tid; i < fh * fw; i += kThreads) {
                const int y = i / fw, x = i - y * fw;
                store_packed(cout, i, unit_fast((float)win[sh.row(y, fh) * ow + sh.col(x, fw)]));
            }
        }
        return;
    }
    const auto oout = quads();
    if (MODE == AGX_OUT_MASK) {
        if constexpr (!SHIFT::shifted) {
            mask_out_write(oout, lds.raw, r, c, oh, ow, fh, fw, tid);
        } else {
            for (int i = tid; i < nq; i += kThreads) {
                const int y = i / ow4, x = (i - y * ow4) * 4;
                const int sy = sh.row(y, oh) - r;                        // the source row inside the window image, if 0 <= sy < fh
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (sy >= 0 && sy < fh) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int sx = sh.col(x + e, ow);
                        if (sx >= c && sx < c + fw) v[e] = unit_fast((float)lds.raw[sy * ow + sx]);
                    }
                }
                store_obs(oout, i, make_float4(v[0], v[1], v[2], v[3]));
            }
        }
        return;
    }
    const int xcol = tid % ow, yb = tid / ow;
    phase_c(lds.H, win, taps.xt, p.xtab, ow, fh, xcol, yb, tid, sh);
    __syncthreads();
    phase_d_write(oout, lds.H, lds.ytab_s, oh, ow4, tid);
}

}  // namespace agx
