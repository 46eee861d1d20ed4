// agx_k11_sequence.h - K11: sequence replay on the frame history (include/agx_sequence.h).  k_sequence_gather finds where each
// sequence ends and runs the step log's walk for every live step, k_sequence_observe re-creates the observation planes of every
// step and writes zeros for the padded ones.  The length rule is agx_sequence_math.h's, the walk agx_steplog_fold.h's, the
// observation plane agx_hist_plane.h's: nothing is restated here.  Every device write is an ordinary vector store.
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
// valid by the history's rule (hist_resolve), re-checked here whatever d_len says.  A live plane is plane j of sample (n, k + l)
// at the recorded fov_loc, by the history readers' shared body (agx_hist_plane.h) with no action and no shift.  Every other
// plane is written as literal zeros through the same stores (store_obs / store_packed), not through the phases on a zero
// window: the contract is all-zero BYTES, and it holds whatever the signs of a context's taps.
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
    const bool first = pl == 0 && tid == 0;
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
    // ---- the sample (n, k0 + l) by the history's rule, re-checked here whatever d_len says
    const bool in_len = l < min(len, q.L) && k0 >= -(int64_t)kSequenceLimit && k0 <= INT64_MAX - kSequenceLimit;
    const HistStack st = in_len ? hist_resolve(q.h, n, k0 + l) : HistStack{false, 0, 0, 0};
    const int elems = hist_plane_elems<MODE>(g);
    OT *plane = reinterpret_cast<OT *>(p.obs) + ((size_t)row * q.planes + pl) * (size_t)elems;
    if (first && q.live) q.live[row] = st.ok ? 1 : 0;
    if (!st.ok) {
        if (first && p.user_loc) {
            p.user_loc[2 * (size_t)row] = 0;
            p.user_loc[2 * (size_t)row + 1] = 0;
        }
        if (MODE == AGX_OUT_RAW) {
            const auto cout = packed_out<OT>(plane, elems);
            for (int i = tid; i < elems; i += kThreads) store_packed(cout, i, 0.0f);
        } else {
            const int nq = g.oh() * (g.ow() >> 2);
            const auto oout = obs_out<OT>(reinterpret_cast<obs4_t<OT> *>(plane), nq);
            for (int i = tid; i < nq; i += kThreads) store_obs(oout, i, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        }
        return;
    }
    const HistPlaneSrc src = hist_plane_src(g, q.h, st, n, q.h.fs - q.planes + pl);
    const HistTaps taps = hist_taps<MODE>(p, g.oh(), g.ow(), tid, NoShift{});
    int r, c;
    hist_position<false>(p, q.h, q.has_loc, st.row_k, n, 0, g.oh() - g.fh(), g.ow() - g.fw(), first, (size_t)row, r, c);
    hist_plane_write<G, MODE, OT>(g, p, smem, src, r, c, taps, plane, NoShift{});
}

}  // namespace agx
