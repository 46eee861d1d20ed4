// agx_history_impl.h - the frame history declared in include/agx_history.h (included at the end of agx_api.hip, behind the
// native loop it attaches to): storage, the push / observe launches (agx_k5_history.h) and agx_loop_set_history.
#pragma once
#include "agx_history.h"

struct agx_history {
    agx_ctx *ctx = nullptr;
    int T = 0;
    uint8_t *block = nullptr;       // the one device allocation: frames | loc | count | age
    size_t bytes = 0;
    agx::HistParams p{};
};

namespace {

size_t hist_align(size_t b) { return (b + 255) & ~(size_t)255; }

int hist_refuse_range(agx_history *h, const char *who) { return refuse_range(h->ctx, who); }

}  // namespace

extern "C" {

int agx_history_create(agx_ctx *ctx, int32_t capacity, agx_history **out) {
    if (!ctx || !out) return fail(ctx, AGX_E_INVALID, "agx_history_create: null argument");
    *out = nullptr;
    const agx_config &c = ctx->cfg;
    if (ctx->planes != 1)
        return fail(ctx, AGX_E_STATE, "agx_history_create: an AGX_FRAME_RGB context is not supported (gray base / fixed contexts only)");
    if (c.kind != AGX_KIND_BASE && c.kind != AGX_KIND_FIXED)
        return fail(ctx, AGX_E_STATE, "agx_history_create: a context of kind %d is not supported (AGX_KIND_BASE and AGX_KIND_FIXED only)", c.kind);
    if (!full_range(ctx)) return refuse_range(ctx, "agx_history_create");
    if (capacity < c.frame_stack)
        return fail(ctx, AGX_E_INVALID, "agx_history_create: capacity %d is below frame_stack %d", capacity, c.frame_stack);
    agx_history *h = new (std::nothrow) agx_history;
    if (!h) return fail(ctx, AGX_E_NOMEM, "out of host memory");
    h->ctx = ctx;
    h->T = capacity;
    const size_t T = (size_t)capacity, N = (size_t)c.num_envs, fbytes = (size_t)c.obs_h * c.obs_w;
    const size_t b_frames = hist_align(T * N * fbytes), b_loc = hist_align(T * N * 2 * sizeof(int32_t)), b_count = hist_align(N * sizeof(int64_t)),
                 b_age = hist_align(T * N);      // (whole dwords: the scalar byte load reads the aligned dword around a byte)
    h->bytes = b_frames + b_loc + b_count + b_age;
    DeviceGuard g(c.device);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&h->block), h->bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        const size_t want = h->bytes;
        delete h;
        if (e == hipErrorOutOfMemory)
            return fail(ctx, AGX_E_NOMEM, "agx_history_create: %zu bytes of device memory for %d x %d env-steps: %s", want, capacity, c.num_envs,
                        hipGetErrorString(e));
        return fail(ctx, AGX_E_HIP, "agx_history_create: hipMalloc(%zu): %s", want, hipGetErrorString(e));
    }
    agx::HistParams &p = h->p;
    p.frames = h->block;
    p.loc = reinterpret_cast<int32_t *>(h->block + b_frames);
    p.count = reinterpret_cast<int64_t *>(h->block + b_frames + b_loc);
    p.age = h->block + b_frames + b_loc + b_count;
    p.T = capacity;
    p.N = c.num_envs;
    p.fs = c.frame_stack;
    p.fbytes = (int32_t)fbytes;
    p.start_age = -1;
    e = hipMemset(p.count, 0, b_count + b_age);
    if (e != hipSuccess) {
        (void)hipFree(h->block);
        delete h;
        return fail(ctx, AGX_E_HIP, "agx_history_create: hipMemset: %s", hipGetErrorString(e));
    }
    *out = h;
    return AGX_OK;
}

int agx_history_destroy(agx_history *h) {
    if (!h) return AGX_OK;
    DeviceGuard g(h->ctx->cfg.device);
    if (h->block) (void)hipFree(h->block);
    delete h;
    return AGX_OK;
}

int agx_history_clear(agx_history *h, void *stream) {
    if (!h) return AGX_E_INVALID;
    DeviceGuard g(h->ctx->cfg.device);
    AGX_HIP(h->ctx, hipMemsetAsync(h->p.count, 0, (size_t)h->p.N * sizeof(int64_t), S(stream)));
    h->p.start_age = 254;      // the frames before an env's next append are no longer known to be zero
    return AGX_OK;
}

int64_t agx_history_bytes(const agx_history *h) { return h ? (int64_t)h->bytes : AGX_E_INVALID; }

int agx_history_push(agx_history *h, const uint8_t *d_cmd, int64_t *d_index, void *stream) {
    if (!h) return AGX_E_INVALID;
    agx_ctx *ctx = h->ctx;
    if (!d_cmd) return fail(ctx, AGX_E_INVALID, "agx_history_push: null command bytes");
    if (!full_range(ctx)) return hist_refuse_range(h, "agx_history_push");
    const agx_config &c = ctx->cfg;
    DeviceGuard g(c.device);
    agx::HistPushParams q;
    q.h = h->p;
    q.ring = ctx->ring;
    q.head = ctx->head[ctx->cur_head];
    q.loc_cur = has_fovea(c) ? ctx->loc[ctx->cur_fov] : nullptr;
    q.cmd = d_cmd;
    q.index_out = d_index;
    if (h->p.fbytes % 16 == 0)
        hipLaunchKernelGGL(agx::k_history_push<uint4>, dim3(c.num_envs), dim3(kThreads), 0, S(stream), q);
    else
        hipLaunchKernelGGL(agx::k_history_push<uint32_t>, dim3(c.num_envs), dim3(kThreads), 0, S(stream), q);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_history_last_index(agx_history *h, int64_t *d_index, void *stream) {
    if (!h) return AGX_E_INVALID;
    if (!d_index) return fail(h->ctx, AGX_E_INVALID, "agx_history_last_index: null buffer");
    DeviceGuard g(h->ctx->cfg.device);
    const int N = h->p.N;
    hipLaunchKernelGGL(agx::k_history_last, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, S(stream), h->p.count, d_index, N);
    AGX_HIP(h->ctx, hipGetLastError());
    return AGX_OK;
}

int agx_history_observe(agx_history *h, int what, const int32_t *d_env, const int64_t *d_index, int32_t B, const void *d_action,
                        int action_dtype, float *d_obs, int32_t *d_fov_loc, uint8_t *d_valid, void *stream) {
    if (!h) return AGX_E_INVALID;
    agx_ctx *ctx = h->ctx;
    const agx_config &c = ctx->cfg;
    if (what != AGX_HIST_FOVEA && what != AGX_HIST_FULL) return fail(ctx, AGX_E_INVALID, "agx_history_observe: what must be AGX_HIST_FOVEA or AGX_HIST_FULL, got %d", what);
    if (what == AGX_HIST_FOVEA && c.kind != AGX_KIND_FIXED)
        return fail(ctx, AGX_E_STATE, "agx_history_observe: AGX_HIST_FOVEA on a context without a fovea (a base context takes AGX_HIST_FULL only)");
    if (B < 0) return fail(ctx, AGX_E_INVALID, "agx_history_observe: B = %d", B);
    if (B == 0) return AGX_OK;
    if (!d_env || !d_index || !d_obs) return fail(ctx, AGX_E_INVALID, "agx_history_observe: null buffer");
    int rc = check_dt(ctx, d_action, action_dtype);
    if (rc) return rc;
    if (!full_range(ctx)) return hist_refuse_range(h, "agx_history_observe");
    DeviceGuard g(c.device);
    const bool fixed = c.kind == AGX_KIND_FIXED;
    FovParams p = fov_params(ctx, fixed ? d_action : nullptr, action_dtype, nullptr, nullptr, d_obs, fixed ? d_fov_loc : nullptr, nullptr);
    p.relative = 0;            // a read-time action is absolute whatever the context's action mode
    p.ring = nullptr;
    p.head = nullptr;
    p.loc_in = p.loc_out = nullptr;
    agx::HistObsParams q;
    q.h = h->p;
    q.has_loc = fixed ? 1 : 0;
    const bool fovea = what == AGX_HIST_FOVEA;
    const size_t lds = fovea ? ctx->plan.lds : 0;
    const size_t row_bytes = obs_row_bytes(ctx, fovea && c.out_mode == AGX_OUT_RAW);
    // the sample index rides on gridDim.y: launches of at most 65535 samples
    for (int32_t at = 0; at < B; at += 65535) {
        const int nb = std::min<int32_t>(B - at, 65535);
        FovParams pp = p;
        pp.obs = reinterpret_cast<float *>(reinterpret_cast<char *>(d_obs) + (size_t)at * row_bytes);
        if (pp.action) pp.action = static_cast<const char *>(pp.action) + (size_t)at * action_stride(action_dtype);
        if (pp.user_loc) pp.user_loc += 2 * (size_t)at;
        q.env = d_env + at;
        q.index = d_index + at;
        q.valid = d_valid ? d_valid + at : nullptr;
        const dim3 grid(c.frame_stack, nb), block(kThreads);
        with_obs_type(ctx->obs_type, [&](auto tag) {
            return with_geom(ctx->plan.headline, geom_r(c), [&](auto g) {
                auto launch = [&](auto mode) {
                    hipLaunchKernelGGL((agx::k_history_observe<decltype(g), decltype(mode)::value, decltype(tag)>), grid, block, lds, S(stream), g, pp, q);
                    return 0;
                };
                return fovea ? with_mode(c.out_mode, launch) : launch(std::integral_constant<int, agx::kHistFull>{});
            });
        });
    }
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_loop_set_history(agx_loop *l, agx_history *h) {
    if (!l) return AGX_E_INVALID;
    if (h && h->ctx != l->ctx) return lfail(l, AGX_E_INVALID, "agx_loop_set_history: the history belongs to another context");
    l->hist = h;
    return AGX_OK;
}

}  // extern "C"
