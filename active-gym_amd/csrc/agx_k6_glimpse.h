// agx_k6_glimpse.h - K6: the glimpse memory (include/agx_glimpse.h): k_history_memory writes the elementwise maximum of a
// sample's last P observations, each re-created from the frame history by the fixed fovea's phases (agx_fixed_phases.h), as
// k_history_observe (agx_k5_history.h) re-creates one.
#pragma once
#include "agx_glimpse.h"
#include "agx_k5_history.h"

namespace agx {

struct HistMemParams {
    HistParams h;
    const int32_t *env;       // [B]
    const int64_t *index;     // [B]
    int32_t *loc_out;         // [B][P][2] or nullptr
    uint8_t *taken;           // [B] or nullptr
    int32_t glimpses;         // P, 1 .. AGX_GLIMPSE_LIMIT
};

// Where the running maximum of the resize form lives: in registers when the number of output passes is a compile-time
// constant (the headline geometry: 7 float4 per thread), in an LDS image [oh][ow] f32 otherwise.
template <class G>
struct MemPasses {
    static constexpr int value = 0;
};
template <int OH, int OW, int FH, int FW>
struct MemPasses<GeomS<OH, OW, FH, FW>> {
    static constexpr int value = (OH * (OW / 4) + kThreads - 1) / kThreads;
};

// ---------------------------------------------------------------------------------------------
// k_history_memory<G, MODE, OT>: grid = (fs, B), block = 256.  Workgroup (j, b) owns stack position j of sample b = (n, k).
// Glimpse i (0 = newest) is the observation of (n, k - i); it is taken when i <= age[k] (same episode) and (n, k - i) is a
// valid sample of the history.  Both conditions only get harder with i, so the taken glimpses are 0 .. nt - 1 and the loop
// stops at the first one that is not.  An invalid sample (nt = 0) leaves its rows untouched.
//   staging: per taken glimpse its own age and fov_loc (scalar loads), then the fh window rows of history row
//            k - i - (fs-1-j) into an LDS image of its own (zeros for a frame older than that glimpse's last CLEAR); the
//            loads of all glimpses are in flight together, one barrier.
//   MASK:    an output byte is the max over the glimpses whose window covers it; unit_fast is monotone: one conversion.
//   RESIZE:  per glimpse phase C (H, double-buffered: one barrier per glimpse) and phase D with the running maximum;
//            one pass of store_obs at the end.  The first glimpse assigns, so P = 1 is k_history_observe bit for bit.
// LDS carve: glimpse table int2[AGX_GLIMPSE_LIMIT] (r, c) | P windows u8 [fh][ow] (16-B padded each) | ytab[oh] | H[2][fh][ow]
//            (fixed_carve with P windows) | acc[oh][ow] (run-time geometry only)            (agx_plan.h: memory_lds)
// ---------------------------------------------------------------------------------------------
// (kMemTableBytes, the glimpse table's bytes: agx_fixed_phases.h, beside fixed_pad)

template <class G, int MODE, class OT>
__global__ __launch_bounds__(kThreads) void k_history_memory(G g, FovParams p, HistMemParams q) {
    static_assert(MODE == AGX_OUT_MASK || MODE == AGX_OUT_RESIZE, "the glimpse memory serves mask-out and resize_to_full");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int oh = g.oh(), ow = g.ow(), fh = g.fh(), fw = g.fw();
    const int T = q.h.T, N = q.h.N, fs = q.h.fs, P = q.glimpses;
    // ---- the sample, as k_history_observe resolves it
    const HistSample s = hist_sample(q.env, q.index, q.h, b);
    if (!s.ok) {
        if (j == 0 && tid == 0 && q.taken) q.taken[b] = 0;
        return;
    }
    const int n = s.n;
    const int64_t k = s.k, oldest = s.cnt - T > 0 ? s.cnt - T : 0;     // the oldest retained index
    const int row_k = hist_row(k, T);
    const int back = fs - 1 - j;
    const int fbytes = oh * ow, ow4 = ow >> 2;
    const int raw_pad = fixed_pad(fh, ow);
    const int wwords = (fh * ow) >> 2;
    int2 *tab = reinterpret_cast<int2 *>(smem);
    const FixedCarve lds = fixed_carve(smem + kMemTableBytes, oh, ow, fh, P);

    int4 xt = make_int4(0, 0, 0, 0);
    int4 yt0 = make_int4(0, 0, 0, 0);
    if (MODE == AGX_OUT_RESIZE) {                         // this thread's taps go out first, as in K2
        xt = *reinterpret_cast<const int4 *>(p.xtab + tid % ow);
        yt0 = *reinterpret_cast<const int4 *>(p.ytab + min(tid, oh - 1));
    }
    // ---- staging: resolve glimpse i, issue its window loads; the LDS writes follow once every glimpse's loads are out
    uint32_t ww[AGX_GLIMPSE_LIMIT][kWinRegs];
    int nt = 0, age_k = 0;
    bool live = true;
#pragma unroll
    for (int i = 0; i < AGX_GLIMPSE_LIMIT; ++i) {
#pragma unroll
        for (int k_ = 0; k_ < kWinRegs; ++k_) ww[i][k_] = 0u;
        if (live && i < P && k - i >= oldest) {
            int row_i = row_k - i;                        // i < AGX_GLIMPSE_LIMIT; T may be smaller
            while (row_i < 0) row_i += T;
            const size_t hrow = (size_t)row_i * N + n;
            int age_i;
            int2 rc;
            uniform_load_age_loc(q.h.age + hrow, q.h.loc + 2 * hrow, age_i, rc);
            if (i == 0) age_k = age_i;
            // (hist_stack_ok(k - i, cnt, T, fs, age_i) against the loop's own `oldest`: calling it here costs 11 instructions and 3 SGPRs)
            live = i <= age_k && k - i - min(age_i, fs - 1) >= oldest;
            if (live) {
                nt = i + 1;
                // a recorded fov_loc is in range unless the caller set one that is not (agx_set_fov_state)
                const int r = min(max(rc.x, 0), oh - fh), c = min(max(rc.y, 0), ow - fw);
                if (tid == 0) {
                    tab[i] = make_int2(r, c);
                    if (j == 0 && q.loc_out) *reinterpret_cast<int2 *>(q.loc_out + 2 * ((size_t)b * P + i)) = make_int2(r, c);
                }
                if (back <= age_i) {
                    int row = row_i - back;               // back <= fs - 1 < T
                    if (row < 0) row += T;
                    const uint32_t *wsrc = reinterpret_cast<const uint32_t *>(q.h.frames + ((size_t)row * N + n) * (size_t)fbytes) + r * ow4;
#pragma unroll
                    for (int k_ = 0; k_ < kWinRegs; ++k_) ww[i][k_] = window_reg(wsrc, k_, wwords, tid);
                    window_tail(lds.raw + i * raw_pad, wsrc, wwords, tid);
                } else {                                  // a frame older than this glimpse's last CLEAR: zeros
                    window_tail(lds.raw + i * raw_pad, nullptr, wwords, tid, /*zero*/ true);
                }
            }
        } else {
            live = false;
        }
    }
    if (j == 0 && tid == 0 && q.taken) q.taken[b] = (uint8_t)nt;
    if (nt == 0) return;
    if (MODE == AGX_OUT_RESIZE) ytab_stage(lds.ytab_s, yt0, p.ytab, oh, tid);
#pragma unroll
    for (int i = 0; i < AGX_GLIMPSE_LIMIT; ++i)
        if (i < nt) window_land(lds.raw + i * raw_pad, ww[i], wwords, tid);
    __syncthreads();

    const int nq = oh * ow4, passes = (nq + kThreads - 1) / kThreads;
    obs4_t<OT> *out4 = reinterpret_cast<obs4_t<OT> *>(p.obs) + ((size_t)b * fs + j) * (size_t)nq;
    const auto oout = obs_out<OT>(out4, nq);
    if (MODE == AGX_OUT_MASK) {
        for (int k_ = 0; k_ < passes; ++k_) {
            const int qd = tid + k_ * kThreads;
            if (qd >= nq) break;
            const int yrow = qd / ow4, x = (qd - yrow * ow4) * 4;
            uint32_t m[4] = {0u, 0u, 0u, 0u};
            for (int i = 0; i < nt; ++i) {
                const int2 rc = tab[i];
                const int r = rc.x, c = rc.y;
                if (yrow >= r && yrow < r + fh && x + 3 >= c && x < c + fw) {
                    const uint32_t w = *reinterpret_cast<const uint32_t *>(lds.raw + i * raw_pad + (yrow - r) * ow + x);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (x + e >= c && x + e < c + fw) m[e] = max(m[e], (w >> (8 * e)) & 0xFFu);
                }
            }
            store_obs(oout, qd, make_float4(unit_fast((float)m[0]), unit_fast((float)m[1]), unit_fast((float)m[2]), unit_fast((float)m[3])));
        }
        return;
    }
    // ---- RESIZE
    constexpr int kRegPasses = MemPasses<G>::value;
    constexpr bool kRegs = kRegPasses > 0 && kRegPasses <= 8;
    float4 *accL = reinterpret_cast<float4 *>(lds.H + 2 * fh * ow);   // run-time geometry: this thread's own quads only
    float4 acc[kRegs ? kRegPasses : 1];
    const int xcol = tid % ow, yb = tid / ow;
    for (int i = 0; i < nt; ++i) {
        const int c = __builtin_amdgcn_readfirstlane(tab[i].y);
        float *H = lds.H + (i & 1) * (fh * ow);
        phase_c(H, lds.raw + i * raw_pad + c, xt, p.xtab, ow, fh, xcol, yb, tid);
        // one barrier per glimpse: phase C of glimpse i + 1 writes the other H, and whoever writes this H again (glimpse
        // i + 2) has passed the barrier of glimpse i + 1, behind every thread's phase D of glimpse i
        __syncthreads();
        // phase D, maxed into the running maximum
        const float4 *H4 = reinterpret_cast<const float4 *>(H);
        if constexpr (kRegs) {
#pragma unroll
            for (int k_ = 0; k_ < kRegPasses; ++k_) {
                const int qd = min(tid + k_ * kThreads, nq - 1);
                const float4 o = phase_d_quad(H4, lds.ytab_s, qd, ow4);
                if (i == 0) {
                    acc[k_] = o;
                } else {
                    acc[k_].x = fmaxf(acc[k_].x, o.x);
                    acc[k_].y = fmaxf(acc[k_].y, o.y);
                    acc[k_].z = fmaxf(acc[k_].z, o.z);
                    acc[k_].w = fmaxf(acc[k_].w, o.w);
                }
            }
        } else {
            for (int k_ = 0; k_ < passes; ++k_) {
                const int qd = tid + k_ * kThreads;
                if (qd >= nq) break;
                float4 o = phase_d_quad(H4, lds.ytab_s, qd, ow4);
                if (i > 0) {
                    const float4 m = accL[qd];
                    o.x = fmaxf(m.x, o.x);
                    o.y = fmaxf(m.y, o.y);
                    o.z = fmaxf(m.z, o.z);
                    o.w = fmaxf(m.w, o.w);
                }
                if (i == nt - 1)
                    store_obs(oout, qd, o);
                else
                    accL[qd] = o;
            }
        }
    }
    if constexpr (kRegs) {
#pragma unroll
        for (int k_ = 0; k_ < kRegPasses; ++k_) {
            const int qd = tid + k_ * kThreads;
            if (qd < nq) store_obs(oout, qd, acc[k_]);
        }
    }
}

}  // namespace agx
