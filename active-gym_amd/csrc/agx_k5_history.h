// agx_k5_history.h - K5: the frame history (include/agx_history.h): k_history_push appends each env's newest ring frame,
// k_history_observe re-creates the observation of retained env-steps: the history readers' shared plane body (agx_hist_plane.h,
// where the storage and the sample resolution are stated too) under (j, b) indexing, unshifted.
#pragma once
#include "agx_hist_plane.h"

namespace agx {

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
// (no ring head here): it resolves the sample, leaves an invalid one untouched but for its valid byte, and otherwise writes plane
// (b, j) by the shared body, at the recorded fov_loc or the read-time action of row b.  MODE = kHistFull: the full frame.
// ---------------------------------------------------------------------------------------------
struct HistObsParams {
    HistParams h;
    const int32_t *env;       // [B]
    const int64_t *index;     // [B]
    uint8_t *valid;           // [B] or nullptr
    int32_t has_loc;          // the context records fov_loc (fixed kind)
};

// workgroup (j, b) of k_history_observe and of its shifted form (agx_k10_augment.h), which differ in the policy alone
template <class G, int MODE, class OT, class SHIFT>
__device__ __forceinline__ void hist_observe_plane(const G &g, const FovParams &p, const HistObsParams &q, unsigned char *smem,
                                                   const SHIFT &sh) {
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const bool first = j == 0 && tid == 0;
    const int n = uniform_load_i32(q.env + b);
    const HistStack st = hist_resolve(q.h, n, uniform_load_i64(q.index + b));
    if (!st.ok) {
        if (first && q.valid) q.valid[b] = 0;
        return;
    }
    if (first && q.valid) q.valid[b] = 1;
    const HistPlaneSrc src = hist_plane_src(g, q.h, st, n, j);
    const HistTaps taps = hist_taps<MODE>(p, g.oh(), g.ow(), tid, sh);
    int r, c;
    hist_position<true>(p, q.h, q.has_loc, st.row_k, n, b, g.oh() - g.fh(), g.ow() - g.fw(), first, b, r, c);
    OT *plane = reinterpret_cast<OT *>(p.obs) + ((size_t)b * q.h.fs + j) * (size_t)hist_plane_elems<MODE>(g);
    hist_plane_write<G, MODE, OT>(g, p, smem, src, r, c, taps, plane, sh);
}

template <class G, int MODE, class OT>
__global__ __launch_bounds__(kThreads) void k_history_observe(G g, FovParams p, HistObsParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    hist_observe_plane<G, MODE, OT>(g, p, q, smem, NoShift{});
}

}  // namespace agx
