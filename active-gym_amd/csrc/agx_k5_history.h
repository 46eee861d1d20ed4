// agx_k5_history.h - K5: the frame history (include/agx_history.h): k_history_push appends each env's newest ring frame,
// k_history_observe re-creates the observation of retained env-steps with K2's own phases (agx_k2_fixed.h).
#pragma once
#include "agx_k2_fixed.h"

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

// wave-uniform 8-byte loads through the scalar cache (uniform_load_i32's contract: written by an earlier launch, naturally aligned)
__device__ __forceinline__ int64_t uniform_load_i64(const int64_t *ptr) {
    int2 w;
    asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(ptr) : "memory");
    return (int64_t)(((uint64_t)(uint32_t)w.y << 32) | (uint32_t)w.x);
}
__device__ __forceinline__ int2 uniform_load_i32x2(const int32_t *ptr) {
    int2 w;
    asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(ptr) : "memory");
    return w;
}
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

// ---------------------------------------------------------------------------------------------
// k_history_observe<G, MODE, OT>: grid = (fs, B), block = 256.  Workgroup (j, b) owns stack position j of sample b directly
// (no ring head here): it resolves the sample (env, index, count, age: scalar loads), leaves an invalid one untouched, and
// otherwise fetches only the fh window rows of history row k - (fs-1-j) - nothing for a frame older than the env's last CLEAR,
// whose LDS image is zeros - and runs K2's phases on them as fovea_fixed_body does: the context's own xtab / ytab, unit_fast,
// the explicit mul + fma lerps, store_obs / store_packed (sc1 buffer stores).  Same arithmetic on the same bytes: the output
// of a sample at its recorded fov_loc is bit for bit the step's.  MODE = kHistFull: the full-frame k/255 write of k_full.
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
    // ---- the sample: env, index, the env's count, the age of row k.  Everything is workgroup-uniform.
    const int n = uniform_load_i32(q.env + b);
    const int64_t k = uniform_load_i64(q.index + b);
    bool ok = n >= 0 && n < N && k >= 0;
    int64_t cnt = 0;
    if (ok) {
        cnt = uniform_load_i64(q.h.count + n);
        ok = k < cnt && k >= cnt - T;
    }
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
        for (int i = tid; i < oh * ow4; i += kThreads) {
            const uint32_t v = zero ? 0u : fsrc[i];
            float4 o;
            o.x = unit(v & 0xFF);
            o.y = unit((v >> 8) & 0xFF);
            o.z = unit((v >> 16) & 0xFF);
            o.w = unit(v >> 24);
            store_obs(oout, i, o);
        }
        return;
    }
    // LDS carve: window rows u8 [fh][ow] (16-B padded) | ytab[oh] | H[fh][ow]     (fovea_fixed_body's; agx_api.hip: fixed_lds)
    unsigned char *raw = smem;
    const int raw_pad = (fh * ow + 15) & ~15;
    Tap *ytab_s = reinterpret_cast<Tap *>(raw + raw_pad);
    float *H = reinterpret_cast<float *>(ytab_s + oh);
    const int wp = ow;
    {
        const uint32_t *wsrc = fsrc + r * ow4;
        const int wwords = (fh * ow) >> 2;
        constexpr int kW = 3;
        uint32_t ww[kW];
#pragma unroll
        for (int k_ = 0; k_ < kW; ++k_) ww[k_] = zero ? 0u : wsrc[min(tid + k_ * kThreads, wwords - 1)];
        if (MODE == AGX_OUT_RESIZE) {
            if (tid < oh) *reinterpret_cast<int4 *>(ytab_s + tid) = yt0;
            for (int i = tid + kThreads; i < oh; i += kThreads) ytab_s[i] = p.ytab[i];
        }
#pragma unroll
        for (int k_ = 0; k_ < kW; ++k_)
            if (tid + k_ * kThreads < wwords) reinterpret_cast<uint32_t *>(raw)[tid + k_ * kThreads] = ww[k_];
        for (int i = tid + kW * kThreads; i < wwords; i += kThreads) reinterpret_cast<uint32_t *>(raw)[i] = zero ? 0u : wsrc[i];
        __syncthreads();
    }
    const int xcol = tid % ow, yb = tid / ow;
    const unsigned char *win = raw + c;
    if (MODE == AGX_OUT_RAW) {
        const auto cout = packed_out<OT>(reinterpret_cast<OT *>(p.obs) + ((size_t)b * fs + j) * (size_t)(fh * fw), fh * fw);
        for (int i = tid; i < fh * fw; i += kThreads) {
            const int y = i / fw, x = i - y * fw;
            store_packed(cout, i, unit_fast((float)win[y * wp + x]));
        }
        return;
    }
    obs4_t<OT> *out4 = reinterpret_cast<obs4_t<OT> *>(p.obs) + ((size_t)b * fs + j) * (size_t)(oh * ow4);
    const auto oout = obs_out<OT>(out4, oh * ow4);
    if (MODE == AGX_OUT_MASK) {
        for (int k_ = 0; k_ < (oh * ow4 + kThreads - 1) / kThreads; ++k_) {
            const int qd = tid + k_ * kThreads;
            if (qd >= oh * ow4) break;
            const int yrow = qd / ow4, x = (qd - yrow * ow4) * 4;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (yrow >= r && yrow < r + fh && x + 3 >= c && x < c + fw) {
                const uint32_t w = *reinterpret_cast<const uint32_t *>(raw + (yrow - r) * wp + x);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (x + e >= c && x + e < c + fw) v[e] = unit_fast((float)((w >> (8 * e)) & 0xFF));
            }
            store_obs(oout, qd, make_float4(v[0], v[1], v[2], v[3]));
        }
        return;
    }
    // ---- RESIZE, phase C: thread owns column xcol (taps in registers), rows yb, yb + rstep, ...
    const int rstep = kThreads / ow;
    if (rstep > 0) {
        if (yb < rstep) {
            const unsigned char *c0 = win + xt.x, *c1 = win + xt.y;
            const float wa = __int_as_float(xt.z), wb = __int_as_float(xt.w);
#pragma unroll 10
            for (int y = yb; y < fh; y += rstep)
                H[y * ow + xcol] = fmaf(wb, unit_fast((float)c1[y * wp]), wa * unit_fast((float)c0[y * wp]));
        }
    } else {                                                          // ow > 256: generic striding
        for (int i = tid; i < fh * ow; i += kThreads) {
            const int y = i / ow, x = i - y * ow;
            const Tap t = p.xtab[x];
            H[i] = fmaf(t.b, unit_fast((float)win[y * wp + t.aux]), t.a * unit_fast((float)win[y * wp + t.lo]));
        }
    }
    __syncthreads();
    // ---- phase D: each output float4 is the vertical lerp (mul + fma, as K2 writes it) of two ds_read_b128
    const float4 *H4 = reinterpret_cast<const float4 *>(H);
    const int nq = oh * ow4, passes = (nq + kThreads - 1) / kThreads;
#pragma unroll 7
    for (int k_ = 0; k_ < passes; ++k_) {
        const int qd = tid + k_ * kThreads;
        if (qd >= nq) break;
        const int yrow = qd / ow4, x4 = qd - yrow * ow4;
        const Tap t = ytab_s[yrow];
        const float4 a = H4[t.lo * ow4 + x4];
        const float4 bb = H4[t.aux * ow4 + x4];
        float4 o;
        o.x = fmaf(t.b, bb.x, t.a * a.x);
        o.y = fmaf(t.b, bb.y, t.a * a.y);
        o.z = fmaf(t.b, bb.z, t.a * a.z);
        o.w = fmaf(t.b, bb.w, t.a * a.w);
        store_obs(oout, qd, o);
    }
}

}  // namespace agx
