// agx_glimpse_impl.h - the glimpse memory declared in include/agx_glimpse.h (included at the end of agx_api.hip, behind the
// frame history it reads): the checks and the launches of k_history_memory (agx_k6_glimpse.h).
#pragma once
#include "agx_glimpse.h"

extern "C" {

int agx_history_observe_memory(agx_history *h, int32_t glimpses, const int32_t *d_env, const int64_t *d_index, int32_t B, float *d_obs,
                               int32_t *d_fov_loc, uint8_t *d_taken, void *stream) {
    if (!h) return AGX_E_INVALID;
    agx_ctx *ctx = h->ctx;
    const agx_config &c = ctx->cfg;
    if (glimpses < 1 || glimpses > AGX_GLIMPSE_LIMIT)
        return fail(ctx, AGX_E_INVALID, "agx_history_observe_memory: glimpses must be 1 .. %d, got %d", AGX_GLIMPSE_LIMIT, glimpses);
    if (B < 0) return fail(ctx, AGX_E_INVALID, "agx_history_observe_memory: B = %d", B);
    if (c.kind != AGX_KIND_FIXED)
        return fail(ctx, AGX_E_STATE, "agx_history_observe_memory: a context without a fovea has no glimpses (AGX_KIND_FIXED only)");
    if (c.out_mode == AGX_OUT_RAW)
        return fail(ctx, AGX_E_STATE, "agx_history_observe_memory: raw-crop mode is not served (a maximum over crops at different positions means nothing; mask-out and resize_to_full are)");
    if (!full_range(ctx)) return hist_refuse_range(h, "agx_history_observe_memory");
    const bool headline = ctx->plan.headline;
    const size_t lds = memory_lds(c, glimpses, headline);
    if (lds > kMaxLds)
        return fail(ctx, AGX_E_STATE, "agx_history_observe_memory: %d glimpses of this geometry need %zu B of LDS per workgroup (limit %zu)", glimpses, lds,
                    kMaxLds);
    if (B == 0) return AGX_OK;
    if (!d_env || !d_index || !d_obs) return fail(ctx, AGX_E_INVALID, "agx_history_observe_memory: null buffer");
    DeviceGuard g(c.device);
    const FovParams p = hist_fov_params(ctx, nullptr, 0, d_obs, nullptr);
    agx::HistMemParams q;
    q.h = h->p;
    q.glimpses = glimpses;
    const size_t row_bytes = obs_row_bytes(ctx, false);
    return hist_chunks(ctx, c.frame_stack, B, lds, stream, [&](const HistLaunch &L) {
        FovParams pp = p;
        pp.obs = reinterpret_cast<float *>(reinterpret_cast<char *>(d_obs) + (size_t)L.at * row_bytes);
        q.env = d_env + L.at;
        q.index = d_index + L.at;
        q.loc_out = d_fov_loc ? d_fov_loc + 2 * (size_t)L.at * glimpses : nullptr;
        q.taken = d_taken ? d_taken + L.at : nullptr;
        with_obs_type(ctx->obs_type, [&](auto tag) {
            return with_geom(headline, geom_r(c), [&](auto g) {
                using G = decltype(g);
                using OT = decltype(tag);
                if (c.out_mode == AGX_OUT_MASK)
                    hipLaunchKernelGGL((agx::k_history_memory<G, AGX_OUT_MASK, OT>), L.grid, dim3(kThreads), L.lds, L.stream, g, pp, q);
                else
                    hipLaunchKernelGGL((agx::k_history_memory<G, AGX_OUT_RESIZE, OT>), L.grid, dim3(kThreads), L.lds, L.stream, g, pp, q);
                return 0;
            });
        });
    });
}

}  // extern "C"
