// agx_retrace_impl.h - the Q-return fold declared in include/agx_retrace.h (included at the end of agx_api.hip, behind the frame
// history and agx_sequence_impl.h, whose arrays it reads and whose argument checks it shares): the checks of K16
// (agx_k16_retrace.h) and the choice of its form.  It owns no handle and no memory.
#pragma once
#include "agx_retrace.h"

static_assert(AGX_SEQUENCE_LIMIT == agx::kRetraceLimit, "agx_retrace_math.h's limit is that of a gathered sequence");

#ifdef AGX_EXPERIMENTS
static bool exp_retrace_tiled() {                 // AGX_RETRACE_TILED=1, read once
    static const bool on = [] {
        const char *e = getenv("AGX_RETRACE_TILED");
        return e && e[0] == '1';
    }();
    return on;
}
#endif

extern "C" {

int agx_sequence_retrace(agx_history *h, int32_t B, int32_t L, int time_major, const int32_t *d_len, const int32_t *d_steps, const float *d_reward,
                         const float *d_discount, const float *d_q, const float *d_v, const float *d_c, const float *d_boot, float *d_target,
                         float *d_td, uint8_t *d_valid, void *stream) {
    agx_ctx *ctx = h ? h->ctx : nullptr;          // (the argument checks need no history: they come first)
    const char *who = "agx_sequence_retrace";
    if (L < 1 || L > AGX_SEQUENCE_LIMIT) return seq_bad_L(ctx, who, L);
    if (int rc = seq_bad_B(ctx, who, B, L)) return rc;
    if (B > 0 && (!d_len || !d_steps || !d_reward || !d_discount || !d_q || !d_v || !d_c || !d_target))
        return fail(ctx, AGX_E_INVALID, "%s: null buffer (%s)", who,
                    !d_len ? "d_len" : !d_steps ? "d_steps" : !d_reward ? "d_reward" : !d_discount ? "d_discount" : !d_q ? "d_q" : !d_v ? "d_v" : !d_c ? "d_c" : "d_target");
    if (!h) return fail(ctx, AGX_E_INVALID, "%s: null argument (h)", who);
    if (B == 0) return AGX_OK;                    // (before the range check, as in agx_sequence_observe)
    if (!full_range(ctx)) return hist_refuse_range(h, who);
    DeviceGuard g(ctx->cfg.device);
    const agx::RetraceParams p{d_len, d_steps, d_reward, d_discount, d_q, d_v, d_c, d_boot, d_target, d_td, d_valid, B, L};
    const dim3 grid((uint32_t)(((int64_t)B + agx::kRetraceThreads - 1) / agx::kRetraceThreads)), block(agx::kRetraceThreads);      // (below 2^25 blocks)
    if (time_major)
        hipLaunchKernelGGL(agx::k_retrace_direct<true>, grid, block, 0, S(stream), p);
#ifdef AGX_EXPERIMENTS                            // the LDS-tiled batch-major form: measured slower, experiments build only
    else if (exp_retrace_tiled())
        hipLaunchKernelGGL(agx::k_retrace_tiled, grid, block, 0, S(stream), p);
#endif
    else
        hipLaunchKernelGGL(agx::k_retrace_direct<false>, grid, block, 0, S(stream), p);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

}  // extern "C"
