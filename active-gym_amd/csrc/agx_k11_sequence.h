// agx_k11_sequence.h - K11: sequence replay on the frame history (include/agx_sequence.h).  k_sequence_gather finds where each
// sequence ends and runs the step log's walk for every live step, k_sequence_observe re-creates the observation planes of every
// step and writes zeros for the padded ones.  The length rule is agx_sequence_math.h's, the walk agx_steplog_fold.h's, the
// observation phases agx_fixed_phases.h's: nothing is restated here.  Every device write is an ordinary vector store.
#pragma once
#include "agx_k5_history.h"
#include "agx_k8_steplog.h"
#include "agx_sequence_math.h"

namespace agx {

struct SeqParams {
    const int32_t *env;       // [B]
    const int64_t *index;     // [B]
    int32_t *len;             // [B] or nullptr
    int32_t B, L, time_major;
};

// row of step (b, l) in a [B][L] output
__device__ __forceinline__ size_t seq_row(int64_t b, int l, int32_t B, int32_t L, int32_t time_major) {
    return time_major ? (size_t)l * (size_t)B + (size_t)b : (size_t)b * (size_t)L + (size_t)l;
}

// One chunk of 64 steps of a wave's sequence: this lane's step is l = base + lane.  A lane stops the sequence if its step is
// past L or its row breaks it (sequence_breaks); the ballot's first set bit is the first such step of the chunk.  alive (no
// stop in an earlier chunk) and len are wave-uniform and carried across the chunks.  Returns whether step l is live.
template <class Rows>
__device__ __forceinline__ bool sequence_chunk(const Rows &rows, int64_t k, int64_t cnt, int L, int base, int lane, bool &alive, int &len) {
    const int l = base + lane;
    bool stop = !alive || l >= L;
    if (!stop && l > 0) stop = sequence_breaks(rows, k + l, cnt);
    const unsigned long long m = __ballot(stop);
    const int first = m ? __ffsll(m) - 1 : 64;
    const bool live = alive && lane < first;
    if (alive && first < 64) {
        len = base + first;
        alive = false;
    }
    return live;
}

// ---------------------------------------------------------------------------------------------
// k_sequence_gather<WALK>: block = 256 = four waves, one wave per sample, grid = ceil(B / 4): B is not bound by a grid dimension
// beyond gridDim.x.  The lanes of a wave are 64 consecutive steps l; L > 64 takes ceil(L / 64) chunks with the carried
// (alive, len).  Per chunk: each lane reads the age byte of row k + l, ballot + find-first give the first break, and the live
// lanes run steplog_step from (n, k + l), leaving the loop by wave as k_steplog_gather does.  Every step l < L of every output
// is written - a step that is not live, or folded no row, gets steps = 0, next_index = -1 and zeros - lane-consecutive rows
// for [B][L].  WALK = false: the lengths alone (agx_sequence_lengths: p carries the history only).
// ---------------------------------------------------------------------------------------------
template <bool WALK>
__global__ __launch_bounds__(kThreads) void k_sequence_gather(StepLogParams p, SeqParams q, int32_t nstep, float gamma, StepLogOut o) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (b >= q.B) return;                                            // (by whole waves: nothing below synchronises the block)
    int n = q.env[b];
    const int64_t k = q.index[b];
    int64_t cnt = 0;
    bool ok = false;
    if (n >= 0 && n < p.h.N) {
        cnt = p.h.count[n];
        ok = steplog_ok0(k, cnt, p.h.T);
    } else {
        n = 0;
    }
    const StepLogRows rows{p, n};
    if (ok) ok = sequence_start_ok(k, cnt, p.h.T, p.h.fs, rows.age(rows.at(k)));
    bool alive = ok;
    int len = 0;
    for (int base = 0; base < q.L; base += 64) {
        const int l = base + lane;
        const bool live = sequence_chunk(rows, k, cnt, q.L, base, lane, alive, len);
        if (WALK) {
            const int64_t kl = live ? k + l : 0;
            StepFold f;
            bool go = live;                                          // (a live step is retained: steplog_ok0(kl, cnt, T) holds)
            for (int i = 1; i <= nstep; ++i) {
                if (go) go = steplog_step(f, rows, kl, cnt, i, gamma);
                if (!__any(go)) break;
            }
            if (l < q.L) {
                const size_t row = seq_row(b, l, q.B, q.L, q.time_major);
                const bool some = f.m > 0;
                o.steps[row] = f.m;
                if (o.next_index) o.next_index[row] = some ? kl + f.m : -1;
                if (o.ret) o.ret[row] = some ? f.G : 0.0f;
                if (o.discount) o.discount[row] = some ? steplog_discount(f) : 0.0f;
                if (o.flags) o.flags[row] = some ? (uint8_t)f.last : (uint8_t)0;
                if (o.payload) {
                    const int words = p.W >> 2;
                    const uint32_t *src = reinterpret_cast<const uint32_t *>(p.payload) + (some ? rows.at(kl + 1) : 0) * words;
                    uint32_t *dst = o.payload + row * words;
                    for (int w = 0; w < words; ++w) dst[w] = some ? src[w] : 0u;
                }
            }
        }
    }
    if (alive) len = q.L;
    if (lane == 0 && q.len) q.len[b] = len;
}

// ---------------------------------------------------------------------------------------------
// k_sequence_observe<G, MODE, OT>: grid = (planes, rows of this launch), block = 256.  Workgroup (pl, y) owns plane pl - stack
// position j = fs - planes + pl - of output row row0 + y, which is step (b, l) of the call's layout.  b, l, the start index and
// d_len[b] are workgroup-uniform and come through the scalar cache.  The step is live iff l < min(len, L) and (n, k + l) is
// valid by k_history_observe's own rule, re-checked here whatever d_len says.  A live plane is k_history_observe's plane j of
// sample (n, k + l) at the recorded fov_loc: the same sample resolution, age rule, zero-frame path, FixedCarve, phases and
// stores.  Every other plane is written as literal zeros through the same stores (store_obs / store_packed), not through the
// phases on a zero window: the contract is all-zero BYTES, and it holds whatever the signs of a context's taps.
// MODE = kHistFull: the full-frame k/255 write.
// ---------------------------------------------------------------------------------------------
struct SeqObsParams {
    HistParams h;
    const int32_t *env;       // [B]
    const int64_t *index;     // [B]
    const int32_t *len;       // [B]
    uint8_t *live;            // [rows] or nullptr
    int32_t B, L, planes, time_major;
    int32_t has_loc;          // the context records fov_loc (fixed kind)
    int32_t row0;             // the first output row of this launch
};

template <class G, int MODE, class OT>
__global__ __launch_bounds__(kThreads) void k_sequence_observe(G g, FovParams p, SeqObsParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int pl = blockIdx.x, tid = threadIdx.x;
    const int oh = g.oh(), ow = g.ow(), fh = g.fh(), fw = g.fw();
    const int T = q.h.T, N = q.h.N, fs = q.h.fs;
    const int ow4 = ow >> 2;
    // ---- the step this row is
    const int row = q.row0 + (int)blockIdx.y;
    int b, l;
    if (q.time_major) {
        l = row / q.B;
        b = row - l * q.B;
    } else {
        b = row / q.L;
        l = row - b * q.L;
    }
    const int n = uniform_load_i32(q.env + b);
    const int64_t k0 = uniform_load_i64(q.index + b);
    const int len = uniform_load_i32(q.len + b);
    // ---- the sample (n, k0 + l) by the history's rule, and the age of its row
    bool ok = l < min(len, q.L) && n >= 0 && n < N && k0 >= -(int64_t)kSequenceLimit && k0 <= INT64_MAX - kSequenceLimit;
    int64_t k = 0;
    int row_k = 0, age = 0;
    if (ok) {
        k = k0 + l;
        const int64_t cnt = uniform_load_i64(q.h.count + n);
        ok = steplog_ok0(k, cnt, T);
        if (ok) {
            row_k = hist_row(k, T);
            age = (int)uniform_load_u8(q.h.age + (size_t)row_k * N + n);
            ok = sequence_start_ok(k, cnt, T, fs, age);
        }
    }
    const bool crop = MODE == AGX_OUT_RAW;
    const size_t plane = ((size_t)row * q.planes + pl) * (size_t)(crop ? fh * fw : oh * ow);       // in elements
    if (pl == 0 && tid == 0 && q.live) q.live[row] = ok ? 1 : 0;
    if (!ok) {
        if (pl == 0 && tid == 0 && p.user_loc) {
            p.user_loc[2 * (size_t)row] = 0;
            p.user_loc[2 * (size_t)row + 1] = 0;
        }
        if (crop) {
            const auto cout = packed_out<OT>(reinterpret_cast<OT *>(p.obs) + plane, fh * fw);
            for (int i = tid; i < fh * fw; i += kThreads) store_packed(cout, i, 0.0f);
        } else {
            const auto oout = obs_out<OT>(reinterpret_cast<obs4_t<OT> *>(reinterpret_cast<OT *>(p.obs) + plane), oh * ow4);
            for (int i = tid; i < oh * ow4; i += kThreads) store_obs(oout, i, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        }
        return;
    }
    const int j = fs - q.planes + pl;
    const int back = fs - 1 - j;
    const bool zero = back > age;
    int hrow = row_k - back;                              // back <= fs - 1 < T
    if (hrow < 0) hrow += T;
    const int fbytes = oh * ow;
    const uint32_t *fsrc = reinterpret_cast<const uint32_t *>(q.h.frames + ((size_t)hrow * N + n) * (size_t)fbytes);

    // ---- position: the recorded fov_loc of row k
    int r = 0, c = 0;
    int4 xt = make_int4(0, 0, 0, 0);
    int4 yt0 = make_int4(0, 0, 0, 0);
    if (MODE == AGX_OUT_RESIZE) {                         // this thread's taps go out first, as in K2
        xt = *reinterpret_cast<const int4 *>(p.xtab + tid % ow);
        yt0 = *reinterpret_cast<const int4 *>(p.ytab + min(tid, oh - 1));
    }
    if (q.has_loc) {
        const int2 rc = uniform_load_i32x2(q.h.loc + 2 * ((size_t)row_k * N + n));
        // a recorded fov_loc is in range unless the caller set one that is not (agx_set_fov_state): the window stays inside the frame
        r = min(max(rc.x, 0), oh - fh);
        c = min(max(rc.y, 0), ow - fw);
        if (pl == 0 && tid == 0 && p.user_loc) {
            p.user_loc[2 * (size_t)row] = r;
            p.user_loc[2 * (size_t)row + 1] = c;
        }
    }
    if (MODE == kHistFull) {
        // the base observation: k_full's arithmetic (unit: the IEEE quotient) and its written-through store
        const auto oout = obs_out<OT>(reinterpret_cast<obs4_t<OT> *>(reinterpret_cast<OT *>(p.obs) + plane), oh * ow4);
        for (int i = tid; i < oh * ow4; i += kThreads) store_obs(oout, i, unit4(zero ? 0u : fsrc[i]));
        return;
    }
    const FixedCarve lds = fixed_carve(smem, oh, ow, fh);            // (agx_api.hip: fixed_lds)
    {
        const uint32_t *wsrc = fsrc + r * ow4;
        const int wwords = (fh * ow) >> 2;
        uint32_t ww[kWinRegs];
#pragma unroll
        for (int i = 0; i < kWinRegs; ++i) ww[i] = window_reg(wsrc, i, wwords, tid, zero);
        if (MODE == AGX_OUT_RESIZE) ytab_stage(lds.ytab_s, yt0, p.ytab, oh, tid);
        window_land(lds.raw, ww, wwords, tid);
        window_tail(lds.raw, wsrc, wwords, tid, zero);
        __syncthreads();
    }
    const unsigned char *win = lds.raw + c;
    if (MODE == AGX_OUT_RAW) {
        raw_crop_write(reinterpret_cast<OT *>(p.obs) + plane, win, ow, fh, fw, tid);
        return;
    }
    const auto oout = obs_out<OT>(reinterpret_cast<obs4_t<OT> *>(reinterpret_cast<OT *>(p.obs) + plane), oh * ow4);
    if (MODE == AGX_OUT_MASK) {
        mask_out_write(oout, lds.raw, r, c, oh, ow, fh, fw, tid);
        return;
    }
    const int xcol = tid % ow, yb = tid / ow;
    phase_c(lds.H, win, xt, p.xtab, ow, fh, xcol, yb, tid);
    __syncthreads();
    phase_d_write(oout, lds.H, lds.ytab_s, oh, ow4, tid);
}

}  // namespace agx
