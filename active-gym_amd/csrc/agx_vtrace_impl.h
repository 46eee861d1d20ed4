// agx_vtrace_impl.h - the V-trace fold declared in include/agx_vtrace.h (included at the end of agx_api.hip, behind the frame
// history and agx_rollout_impl.h, whose arrays it reads and whose L check and fold launch it shares): the checks of K13
// (agx_k13_vtrace.h).  It owns no handle and no memory.
#pragma once
#include "agx_vtrace.h"

static_assert(AGX_VTRACE_LIMIT == agx::kVtraceLimit && AGX_VTRACE_LIMIT == AGX_ROLLOUT_LIMIT, "the limit is that of a gathered rollout");

extern "C" {

int agx_vtrace_returns(agx_history *h, int32_t L, const int32_t *d_len, const float *d_reward, const uint8_t *d_ends, const float *d_value,
                       const float *d_boot_value, const float *d_rho, float gamma, float lambda, float rho_bar, float c_bar,
                       float pg_rho_bar, float *d_vs, float *d_pg_adv, void *stream) {
    const char *who = "agx_vtrace_returns";
    if (!h) return fail(nullptr, AGX_E_INVALID, "%s: null argument (h)", who);
    agx_ctx *ctx = h->ctx;
    const int32_t N = h->p.N;
    if (int rc = rollout_bad_L(ctx, who, L, N)) return rc;
    if (!d_len || !d_reward || !d_ends || !d_value || !d_rho || !d_vs || !d_pg_adv)
        return fail(ctx, AGX_E_INVALID, "%s: null buffer (%s)", who,
                    !d_len ? "d_len" : !d_reward ? "d_reward" : !d_ends ? "d_ends" : !d_value ? "d_value" : !d_rho ? "d_rho" : !d_vs ? "d_vs" : "d_pg_adv");
    if (!(rho_bar > 0.0f) || !(c_bar > 0.0f) || !(pg_rho_bar > 0.0f))          // (a NaN is not > 0)
        return fail(ctx, AGX_E_INVALID, "%s: %s must be > 0, got %g", who, !(rho_bar > 0.0f) ? "rho_bar" : !(c_bar > 0.0f) ? "c_bar" : "pg_rho_bar",
                    (double)(!(rho_bar > 0.0f) ? rho_bar : !(c_bar > 0.0f) ? c_bar : pg_rho_bar));
    if (!full_range(ctx)) return hist_refuse_range(h, who);
    DeviceGuard g(ctx->cfg.device);
    const agx::VtraceParams q{d_len, d_reward, d_ends, d_value, d_boot_value, d_rho, d_vs, d_pg_adv, N, L, {gamma, lambda, rho_bar, c_bar, pg_rho_bar}};
    return launch_slot_fold<agx::VtraceFold>(ctx, q, d_boot_value != nullptr, stream);
}

}  // extern "C"
