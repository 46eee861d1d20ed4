// agx_k5_history.h - K5: the frame history (include/agx_history.h): k_history_push appends each env's newest ring frame,
// k_history_observe re-creates the observation of retained env-steps by running the fixed fovea's phases (agx_fixed_phases.h,
// the ones K2 runs) on history rows.
#pragma once
#include "agx_fixed_phases.h"
#include "agx_fov_common.h"

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

// ---------------------------------------------------------------------------------------------
// k_history_push: grid = (N), block = 256.  Workgroup n copies ring slot head - 1 (the frame the ingest before this launch
// wrote: L2-resident) into row count % T: LANE-wide lane-linear accesses (uint4 where the frame is a multiple of 16 bytes -
// 7056 at 84 x 84 - dwords otherwise).  The env-uniform state (cmd, head, count, previous age, fov_loc: the CURRENT halves of
// the double buffers, all written by earlier launches) comes through the scalar cache; lane 0 writes the small outputs.
// ---------------------------------------------------------------------------------------------
struct HistPushParams {
    HistParams h;
    const uint8_t *ring;
    const int32_t *head;      // current (post-ingest) head
    const int32_t *loc_cur;   // current fov_loc [N][2], nullptr on a base context
    const uint8_t *cmd;
    int64_t *index_out;       // [N] or nullptr
};
template <class LANE>
__global__ __launch_bounds__(kThreads) void k_history_push(HistPushParams p) {
    const int n = blockIdx.x, tid = threadIdx.x;
    const uint32_t cmd = uniform_load_u8(p.cmd + n);
    if (cmd & AGX_CMD_SKIP) {
        if (tid == 0 && p.index_out) p.index_out[n] = -1;
        return;
    }
    const int T = p.h.T, N = p.h.N;
    const int head = uniform_load_i32(p.head + n);
    const int64_t cnt = uniform_load_i64(p.h.count + n);
    const int row = hist_row(cnt, T);
    int prev = p.h.start_age;
    if (cnt > 0) prev = (int)uniform_load_u8(p.h.age + (size_t)(row == 0 ? T - 1 : row - 1) * N + n);
    const int age = (cmd & AGX_CMD_CLEAR) ? 0 : min(prev + 1, 255);
    int2 rc = make_int2(0, 0);
    if (p.loc_cur) rc = uniform_load_i32x2(p.loc_cur + 2 * n);
    int slot = head - 1;
    if (slot < 0) slot += p.h.fs;
    const size_t dst_row = (size_t)row * N + n;
    const LANE *src = reinterpret_cast<const LANE *>(p.ring + ((size_t)n * p.h.fs + slot) * (size_t)p.h.fbytes);
    LANE *dst = reinterpret_cast<LANE *>(p.h.frames + dst_row * (size_t)p.h.fbytes);
    const int lanes = p.h.fbytes / (int)sizeof(LANE);
    for (int i = tid; i < lanes; i += kThreads) dst[i] = src[i];
    if (tid == 0) {
        p.h.age[dst_row] = (uint8_t)age;
        p.h.count[n] = cnt + 1;
        if (p.loc_cur) *reinterpret_cast<int2 *>(p.h.loc + 2 * dst_row) = rc;
        if (p.index_out) p.index_out[n] = cnt;
    }
}

__global__ __launch_bounds__(kThreads) void k_history_last(const int64_t *count, int64_t *out, int n_envs) {
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n < n_envs) out[n] = count[n] - 1;
}

// A sample b = (env n, index k) of the history, as k_history_observe and k_history_memory resolve it (scalar loads: everything is
// workgroup-uniform).  ok: n is an env and row k is still retained; cnt = the env's appends so far (0 if n is no env).
struct HistSample {
    int n;
    int64_t k, cnt;
    bool ok;
};
__device__ __forceinline__ HistSample hist_sample(const int32_t *env, const int64_t *index, const HistParams &h, int b) {
    HistSample s{uniform_load_i32(env + b), uniform_load_i64(index + b), 0, false};
    if (s.n >= 0 && s.n < h.N && s.k >= 0) {
        s.cnt = uniform_load_i64(h.count + s.n);
        s.ok = s.k < s.cnt && s.k >= s.cnt - h.T;
    }
    return s;
}

// ---------------------------------------------------------------------------------------------
// k_history_observe<G, MODE, OT>: grid = (fs, B), block = 256.  Workgroup (j, b) owns stack position j of sample b directly
// (no ring head here): it resolves the sample and the age of row k, leaves an invalid one untouched, and otherwise fetches
// only the fh window rows of history row k - (fs-1-j) - nothing for a frame older than the env's last CLEAR, whose LDS image
// is zeros - and runs the shared phases on them with the context's own xtab / ytab.  The phases are the very code
// fovea_fixed_body runs, so the output of a sample at its recorded fov_loc is bit for bit the step's.  MODE = kHistFull: the
// full-frame k/255 write of k_full.
// FovParams carries what K2's carries (obs, user_loc, xtab, ytab, action, action_dt; relative = 0: a read-time action is
// absolute); the action row is b's.
// ---------------------------------------------------------------------------------------------
constexpr int kHistFull = 3;   // next to AGX_OUT_RAW / AGX_OUT_RESIZE / AGX_OUT_MASK (0, 1, 2)
static_assert(AGX_OUT_RAW != kHistFull && AGX_OUT_RESIZE != kHistFull && AGX_OUT_MASK != kHistFull, "kHistFull must not be an AGX_OUT_* value");

struct HistObsParams {
    HistParams h;
    const int32_t *env;       // [B]
    const int64_t *index;     // [B]
    uint8_t *valid;           // [B] or nullptr
    int32_t has_loc;          // the context records fov_loc (fixed kind)
};

template <class G, int MODE, class OT>
__global__ __launch_bounds__(kThreads) void k_history_observe(G g, FovParams p, HistObsParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int oh = g.oh(), ow = g.ow(), fh = g.fh(), fw = g.fw();
    const int T = q.h.T, N = q.h.N, fs = q.h.fs;
    // ---- the sample, and the age of row k
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
    const uint32_t *fsrc = reinterpret_cast<const uint32_t *>(q.h.frames + ((size_t)row * N + n) * (size_t)fbytes);

    // ---- position: the recorded fov_loc of row k, or the read-time action through compute_loc (K2's arithmetic)
    int r = 0, c = 0;
    int4 xt = make_int4(0, 0, 0, 0);
    int4 yt0 = make_int4(0, 0, 0, 0);
    if (MODE == AGX_OUT_RESIZE) {                         // this thread's taps go out first, as in K2
        xt = *reinterpret_cast<const int4 *>(p.xtab + tid % ow);
        yt0 = *reinterpret_cast<const int4 *>(p.ytab + min(tid, oh - 1));
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
        // a recorded fov_loc is in range unless the caller set one that is not (agx_set_fov_state): the window stays inside the frame
        r = min(max(r, 0), oh - fh);
        c = min(max(c, 0), ow - fw);
        if (j == 0 && tid == 0 && p.user_loc) {
            p.user_loc[2 * b] = r;
            p.user_loc[2 * b + 1] = c;
        }
    }
    const int ow4 = ow >> 2;
    if (MODE == kHistFull) {
        // the base observation: k_full's arithmetic (unit: the IEEE quotient) and its written-through store
        obs4_t<OT> *out4 = reinterpret_cast<obs4_t<OT> *>(p.obs) + ((size_t)b * fs + j) * (size_t)(oh * ow4);
        const auto oout = obs_out<OT>(out4, oh * ow4);
        for (int i = tid; i < oh * ow4; i += kThreads) store_obs(oout, i, unit4(zero ? 0u : fsrc[i]));
        return;
    }
    const FixedCarve lds = fixed_carve(smem, oh, ow, fh);            // (agx_api.hip: fixed_lds)
    {
        const uint32_t *wsrc = fsrc + r * ow4;
        const int wwords = (fh * ow) >> 2;
        uint32_t ww[kWinRegs];
#pragma unroll
        for (int k = 0; k < kWinRegs; ++k) ww[k] = window_reg(wsrc, k, wwords, tid, zero);
        if (MODE == AGX_OUT_RESIZE) ytab_stage(lds.ytab_s, yt0, p.ytab, oh, tid);
        window_land(lds.raw, ww, wwords, tid);
        window_tail(lds.raw, wsrc, wwords, tid, zero);
        __syncthreads();
    }
    const unsigned char *win = lds.raw + c;
    if (MODE == AGX_OUT_RAW) {
        raw_crop_write(reinterpret_cast<OT *>(p.obs) + ((size_t)b * fs + j) * (size_t)(fh * fw), win, ow, fh, fw, tid);
        return;
    }
    obs4_t<OT> *out4 = reinterpret_cast<obs4_t<OT> *>(p.obs) + ((size_t)b * fs + j) * (size_t)(oh * ow4);
    const auto oout = obs_out<OT>(out4, oh * ow4);
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
