// agx_k2_fixed.h - K2: FixedFovealEnv (k_fovea_fixed, the two-slot form, and the fused step launches).  The body is K2's own
// prologue (mask, fused-step phase, state, compute_loc) around the shared phases of agx_fixed_phases.h.
#pragma once
#include "agx_fixed_phases.h"
#include "agx_fov_common.h"
#include "agx_k1_ingest.h"

namespace agx {

// ---------------------------------------------------------------------------------------------
// K2: FixedFovealEnv
// grid = (fs, N): one workgroup per (env, stacked frame); block = 256
//   MODE = AGX_OUT_RESIZE: LDS s[fh][fw] -> H[fh][ow] (horizontal lerp) -> float4 rows of the
//          84x84 output = vertical lerp of two ds_read_b128; every store is 16 B/lane, lane-linear.
// ---------------------------------------------------------------------------------------------
// grid = (fs, N): workgroup (sl, n) owns PHYSICAL ring slot sl of env n, block = 256.
// Prologue: the small state loads (action, fov_loc, head) and this thread's taps go out first; the scalar chain action ->
// rint(clip(..)) -> (r, c) runs as soon as the state has arrived and moves to SGPRs; then ONLY the window of the slot is
// fetched, for every MODE: its fh rows (LDS image u8 [fh][ow]).  u8 -> float32 k/255 is unit_fast (3 FMAs, the correctly
// rounded quotient).
//   RESIZE: H[fh][ow] = horizontal lerp of the window rows (thread = fixed column x, rows y = yb+3k),
//           then each output float4 is the vertical lerp of two ds_read_b128; stores are 16 B per
//           lane, lane-linear, 1 KiB per wave at 1-KiB steps, written through (sc1, store_obs above).
// (ablation of the previous serial version at N=1024: loc chain 5.8 us, loc-dependent window load
//  6.3 us, H pass with a tap load per iteration 7.3 us, row-tap loads 2.1 us of a 32.7 us launch.)
// COHERENT: the frame is read with agent-scope loads (global_load_dword sc1: served by L2, never by this CU's L1) - for a
// slot that the same launch has just written (k_step_env); phase 3: `head` is the pre-ingest head, every slot is processed.
// NC: planes per frame (1 gray, 3 colour: AGX_FRAME_RGB).  grid = (NC * fs, N); workgroup (q, n) owns ring plane q of env n,
// i.e. channel ch = q % NC of physical slot sl = q / NC, and writes stack-order plane j * NC + ch.  The window, state and arithmetic
// are the gray ones; only workgroup q == 0 writes the env's state.  NC = 1 folds to the gray form instruction for instruction.  The
// fused-step phases (p.phase != 0) are gray-only.
template <class G, int MODE, bool COHERENT = false, class OT = float, int NC = 1>
__device__ __forceinline__ void fovea_fixed_body(const G g, const FovParams &p, const int q_, const int n,
                                                 unsigned char *smem, const int tid) {
    const int sl = q_ / NC, ch = q_ - sl * NC;
    constexpr int T = kThreads;
    (void)T;
    AGX_STAMP(0);
    const int oh = g.oh(), ow = g.ow(), fh = g.fh(), fw = g.fw();
    if (p.mask && !p.mask[n]) {
        if (q_ == 0 && tid < 2) p.loc_out[2 * n + tid] = p.loc_in[2 * n + tid];
        return;
    }
    int head_fixup = 0;                      // what to add to p.head[n] to get the post-ingest head
    if (p.phase != 0) {
        const uint32_t cmd = uniform_load_u8(p.cmd + n);
        const bool skip = (cmd & AGX_CMD_SKIP) != 0, clear = (cmd & AGX_CMD_CLEAR) != 0 && !skip;
        const int h = uniform_load_i32(p.head + n);
        // slot the ingest writes: the pre-ingest head (fs-1 after a clear, which also zeroes the others)
        int wslot;
        if (p.phase == 1 || p.phase == 3) {
            wslot = h;
            head_fixup = skip ? 0 : (clear ? -h : (h + 1 == p.fs ? 1 - p.fs : 1));
        } else {
            wslot = skip ? h : (h == 0 ? p.fs - 1 : h - 1);
        }
        const bool touched = clear || sl == wslot;
        if (p.phase != 3 && (p.phase == 1) == touched) return;   // phase 1 takes the untouched slots, phase 2 the rest
    }
    const FixedCarve lds = fixed_carve(smem, oh, ow, fh);            // (agx_api.hip: fixed_lds)
    const int fbytes = oh * ow;                                       // multiple of 4 (ow % 4 == 0)

    // ---- State first (vmcnt retires in order), then only the fh window rows of the slot (2.5 KB of the 7 KB frame), for every
    // MODE: every resident workgroup of the launch starts with this burst, and a third of the bytes returns sooner than the
    // extra dependent round trip costs (round 1 fetched the whole frame to avoid that dependency: 3.6 us of a wave's 6.7 us
    // life were the load chain; K2 23.1 -> 21.9 us).  Round 3 also built the narrower form - of each row only the
    // dword-aligned column span that holds [c, c + fw), 1.1 KB - and measured a tie (23.4-23.5 us both, same box): the rows of
    // a window are 84 bytes apart, so the span touches the same cache lines as the whole rows; not kept.
    const uint32_t *fsrc = reinterpret_cast<const uint32_t *>(p.ring + (((size_t)n * p.fs + sl) * NC + ch) * (size_t)fbytes);
    int r, c, j;
    int4 xt = make_int4(0, 0, 0, 0);                                  // this thread's column taps {lo, aux, a, b}
    {
        // this thread's taps go out first (vector loads, in flight through the scalar wait below), then the state through the
        // scalar cache
        int4 yt0 = make_int4(0, 0, 0, 0);
        if (MODE == AGX_OUT_RESIZE) {
            xt = *reinterpret_cast<const int4 *>(p.xtab + tid % ow);
            yt0 = *reinterpret_cast<const int4 *>(p.ytab + min(tid, oh - 1));
        }
        int head0;
        const LocIn lin = load_loc_inputs_scalar(p, n, p.head, head0);
        const int head = head0 + head_fixup;
        compute_loc(p, lin, oh - fh, ow - fw, r, c);
        r = __builtin_amdgcn_readfirstlane(r);
        c = __builtin_amdgcn_readfirstlane(c);
        j = sl - __builtin_amdgcn_readfirstlane(head);
        if (j < 0) j += p.fs;
        const uint32_t *wsrc = fsrc + r * (ow >> 2);
        const int wwords = (fh * ow) >> 2;
        uint32_t ww[kWinRegs];
#pragma unroll
        for (int k = 0; k < kWinRegs; ++k) ww[k] = window_reg<COHERENT>(wsrc, k, wwords, tid);
        if (q_ == 0 && tid == 0) {
            p.loc_out[2 * n] = r;
            p.loc_out[2 * n + 1] = c;
            if (p.user_loc) {
                p.user_loc[2 * n] = r;
                p.user_loc[2 * n + 1] = c;
            }
        }
        if (MODE == AGX_OUT_RESIZE) ytab_stage(lds.ytab_s, yt0, p.ytab, oh, tid);
        window_land(lds.raw, ww, wwords, tid);
        window_tail<COHERENT>(lds.raw, wsrc, wwords, tid);
        AGX_STAMP(1);
        __syncthreads();
        AGX_STAMP(2);
    }
    const unsigned char *win = lds.raw + c;                           // window origin inside the LDS image (row r of the frame = row 0)
    if (MODE == AGX_OUT_RAW) {
        raw_crop_write(reinterpret_cast<OT *>(p.obs) + (((size_t)n * p.fs + j) * NC + ch) * (size_t)(fh * fw), win, ow, fh, fw, tid);
        return;
    }
    const int ow4 = ow >> 2;
    obs4_t<OT> *out4 = reinterpret_cast<obs4_t<OT> *>(p.obs) + (((size_t)n * p.fs + j) * NC + ch) * (size_t)(oh * ow4);
    const auto oout = obs_out<OT>(out4, oh * ow4);
    if (MODE == AGX_OUT_MASK) {
        mask_out_write(oout, lds.raw, r, c, oh, ow, fh, fw, tid);
        return;
    }
    const int xcol = tid % ow, yb = tid / ow;
    phase_c(lds.H, win, xt, p.xtab, ow, fh, xcol, yb, tid);
    __syncthreads();
    AGX_STAMP(3);
    phase_d_write(oout, lds.H, lds.ytab_s, oh, ow4, tid);
    AGX_STAMP(4);
}

template <class G, int MODE, class OT = float, int NC = 1>
__device__ __forceinline__ void fovea_fixed_body(const G g, const FovParams &p, const int sl, const int n,
                                                 unsigned char *smem) {
    fovea_fixed_body<G, MODE, false, OT, NC>(g, p, sl, n, smem, (int)threadIdx.x);
}

template <class G, int MODE, class OT = float, int NC = 1>
__global__ __launch_bounds__(kThreads) void k_fovea_fixed(G g, FovParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    fovea_fixed_body<G, MODE, OT, NC>(g, p, blockIdx.x, blockIdx.y, smem);
}

}  // namespace agx
