// agx_k10_augment.h - K10: random-shift augmentation on the frame history's observe (include/agx_augment.h).
// k_history_observe_shifted re-creates the observation of retained env-steps as k_history_observe does and moves every plane by
// the sample's shift on the way out; k_shift_draw draws the shifts.  The shift map and the draw are agx_shift_math.h's.  Every
// device write is an ordinary vector store.
#pragma once
#include "agx_fixed_phases.h"
#include "agx_fov_common.h"
#include "agx_k5_history.h"
#include "agx_shift_math.h"

namespace agx {

struct ShiftObsParams {
    const int32_t *shift;     // i32 [B][2] (dy, dx)
    int32_t pad;
};

// ---------------------------------------------------------------------------------------------
// k_history_observe_shifted<G, MODE, OT>: grid = (fs, B), block = 256.  k_history_observe's workgroup (j, b) - sample, age rule,
// compute_loc, zero frames, the LDS carve and the written-through stores are its own - with the sample's (dy, dx), two more
// workgroup-uniform values through the scalar cache, clamped into 0 .. 2 * pad.  With cy(y) = shift_src(y, dy, pad, rows) and
// cx(x) = shift_src(x, dx, pad, columns), output element (y, x) of the plane is element (cy(y), cx(x)) of k_history_observe's:
//   RESIZE    the shift is folded into the taps: the thread that owns H column x takes xtab[cx(x)], ytab_s[y] is staged from
//             ytab[cy(y)]; phase C and phase D then run as they are (the same mul + fma on the same operands: the same bits),
//             and the store stream is k_history_observe's.  The tap loads wait for the shift: one scalar hop.
//   MASK      per output element the byte of the LDS window image at (cy(y) - r, cx(x)), or zero outside the window; shifted
//             columns are not dword-aligned, so these are byte reads.  The stores are the 16-B quads of mask_out_write.
//   RAW       the crop [fh][fw] is the plane: byte (cy(y), cx(x)) of the window, clamped to the crop.
//   kHistFull byte cy(y) * ow + cx(x) of the history row, read from L2 (no LDS, no barrier: the launch has none, as
//             k_history_observe's full form, and a frame of 1024 x 1024 would not fit).  A quad whose columns are not clamped
//             takes its four bytes from the two aligned dwords around them (v_alignbyte); a quad at the edge reads bytes.
// ---------------------------------------------------------------------------------------------
template <class G, int MODE, class OT>
__global__ __launch_bounds__(kThreads) void k_history_observe_shifted(G g, FovParams p, HistObsParams q, ShiftObsParams sh) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int oh = g.oh(), ow = g.ow(), fh = g.fh(), fw = g.fw();
    const int T = q.h.T, N = q.h.N, fs = q.h.fs;
    // ---- the shift (every row of d_shift is there, whatever the sample turns out to be), the sample, the age of row k
    const int pad = sh.pad;
    const int2 d2 = uniform_load_i32x2(sh.shift + 2 * (size_t)b);
    const int dy = shift_clamp(d2.x, pad), dx = shift_clamp(d2.y, pad);
    const HistSample s = hist_sample(q.env, q.index, q.h, b);
    const int n = s.n;
    const int64_t k = s.k, cnt = s.cnt;
    bool ok = s.ok;
    int row_k = 0, age = 0;
    if (ok) {
        row_k = hist_row(k, T);
        age = (int)uniform_load_u8(q.h.age + (size_t)row_k * N + n);
        const int64_t first = k - min(age, fs - 1);      // the oldest row the stack needs
        ok = first >= 0 && first >= cnt - T;
    }
    if (!ok) {
        if (j == 0 && tid == 0 && q.valid) q.valid[b] = 0;
        return;
    }
    if (j == 0 && tid == 0 && q.valid) q.valid[b] = 1;
    const int back = fs - 1 - j;
    const bool zero = back > age;
    int row = row_k - back;                               // back <= fs - 1 < T
    if (row < 0) row += T;
    const int fbytes = oh * ow;
    const uint8_t *fbyte = q.h.frames + ((size_t)row * N + n) * (size_t)fbytes;
    const uint32_t *fsrc = reinterpret_cast<const uint32_t *>(fbyte);

    // ---- position: the recorded fov_loc of row k, or the read-time action through compute_loc (K2's arithmetic)
    int r = 0, c = 0;
    int4 xt = make_int4(0, 0, 0, 0);
    int4 yt0 = make_int4(0, 0, 0, 0);
    if (MODE == AGX_OUT_RESIZE) {                         // this thread's taps, at the shifted column / row
        xt = *reinterpret_cast<const int4 *>(p.xtab + shift_src(tid % ow, dx, pad, ow));
        yt0 = *reinterpret_cast<const int4 *>(p.ytab + shift_src(min(tid, oh - 1), dy, pad, oh));
    }
    if (q.has_loc) {
        const int2 rc = uniform_load_i32x2(q.h.loc + 2 * ((size_t)row_k * N + n));
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
        compute_loc(p, lin, oh - fh, ow - fw, r, c);
        r = __builtin_amdgcn_readfirstlane(r);
        c = __builtin_amdgcn_readfirstlane(c);
        r = min(max(r, 0), oh - fh);                      // (k_history_observe: the window stays inside the frame)
        c = min(max(c, 0), ow - fw);
        if (j == 0 && tid == 0 && p.user_loc) {           // the shift is not reflected in fov_loc
            p.user_loc[2 * b] = r;
            p.user_loc[2 * b + 1] = c;
        }
    }
    const int ow4 = ow >> 2;
    if (MODE == kHistFull) {
        obs4_t<OT> *out4 = reinterpret_cast<obs4_t<OT> *>(p.obs) + ((size_t)b * fs + j) * (size_t)(oh * ow4);
        const auto oout = obs_out<OT>(out4, oh * ow4);
        const int nwords = oh * ow4;
        for (int i = tid; i < nwords; i += kThreads) {
            const int y = i / ow4, x = (i - y * ow4) * 4;
            uint32_t w = 0u;                                         // the quad's four source bytes, as k_full's dword holds them
            if (!zero) {
                const int so = shift_src(y, dy, pad, oh) * ow, x0 = x + dx - pad;
                if (x0 >= 0 && x0 + 3 < ow) {
                    // no column clamps: four consecutive bytes at an offset that is not dword-aligned - the two aligned
                    // dwords around them (the second one clamped into the frame: it is not used where it would lie outside)
                    const int o = so + x0, wi = o >> 2;
                    w = __builtin_amdgcn_alignbyte(fsrc[min(wi + 1, nwords - 1)], fsrc[wi], (uint32_t)(o & 3));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) w |= (uint32_t)fbyte[so + shift_src(x + e, dx, pad, ow)] << (8 * e);
                }
            }
            store_obs(oout, i, unit4(w));
        }
        return;
    }
    const FixedCarve lds = fixed_carve(smem, oh, ow, fh);            // (agx_plan.h: fixed_lds - the carve does not grow)
    {
        const uint32_t *wsrc = fsrc + r * ow4;
        const int wwords = (fh * ow) >> 2;
        uint32_t ww[kWinRegs];
#pragma unroll
        for (int i = 0; i < kWinRegs; ++i) ww[i] = window_reg(wsrc, i, wwords, tid, zero);
        if (MODE == AGX_OUT_RESIZE) ytab_stage_shifted(lds.ytab_s, yt0, p.ytab, oh, tid, dy, pad);
        window_land(lds.raw, ww, wwords, tid);
        window_tail(lds.raw, wsrc, wwords, tid, zero);
        __syncthreads();
    }
    const unsigned char *win = lds.raw + c;
    if (MODE == AGX_OUT_RAW) {
        const auto cout = packed_out<OT>(reinterpret_cast<OT *>(p.obs) + ((size_t)b * fs + j) * (size_t)(fh * fw), fh * fw);
        for (int i = tid; i < fh * fw; i += kThreads) {
            const int y = i / fw, x = i - y * fw;
            store_packed(cout, i, unit_fast((float)win[shift_src(y, dy, pad, fh) * ow + shift_src(x, dx, pad, fw)]));
        }
        return;
    }
    obs4_t<OT> *out4 = reinterpret_cast<obs4_t<OT> *>(p.obs) + ((size_t)b * fs + j) * (size_t)(oh * ow4);
    const auto oout = obs_out<OT>(out4, oh * ow4);
    if (MODE == AGX_OUT_MASK) {
        for (int i = tid; i < oh * ow4; i += kThreads) {
            const int y = i / ow4, x = (i - y * ow4) * 4;
            const int sy = shift_src(y, dy, pad, oh) - r;            // the source row inside the window image, if 0 <= sy < fh
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (sy >= 0 && sy < fh) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int sx = shift_src(x + e, dx, pad, ow);
                    if (sx >= c && sx < c + fw) v[e] = unit_fast((float)lds.raw[sy * ow + sx]);
                }
            }
            store_obs(oout, i, make_float4(v[0], v[1], v[2], v[3]));
        }
        return;
    }
    const int xcol = tid % ow, yb = tid / ow;
    phase_c_shifted(lds.H, win, xt, p.xtab, ow, fh, xcol, yb, tid, dx, pad);
    __syncthreads();
    phase_d_write(oout, lds.H, lds.ytab_s, oh, ow4, tid);
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
