// agx_history_impl.h - the frame history declared in include/agx_history.h (included at the end of agx_api.hip, behind the
// native loop it attaches to): storage, the push / observe launches (agx_k5_history.h) and agx_loop_set_history.
#pragma once
#include "agx_history.h"

struct agx_history {
    explicit agx_history(int device) : own(device) {}
    Resources own;                  // the one device block: frames | loc | count | age
    agx_ctx *ctx = nullptr;
    int T = 0;
    size_t bytes = 0;
    agx::HistParams p{};
};

namespace {

// The one device block of a handle on the history side (the history itself, replay, step log, priorities, shifts,
// minibatches): `bytes` from the handle's owner, then fill(block) sets its initial contents.  When either fails the handle is
// deleted (which gives the block back), the runtime's sticky error is cleared and the message is ctx's.
template <class H, class Fill>
int hist_block(agx_ctx *ctx, const char *who, H *handle, size_t bytes, uint8_t **block, Fill &&fill) {
    hipError_t e = handle->own.device_mem(block, bytes);
    if (e == hipSuccess) e = fill(*block);
    if (e == hipSuccess) return AGX_OK;
    (void)hipGetLastError();
    delete handle;
    return fail(ctx, e == hipErrorOutOfMemory ? AGX_E_NOMEM : AGX_E_HIP, "%s: %zu bytes of device memory: %s", who, bytes, hipGetErrorString(e));
}

int hist_refuse_range(agx_history *h, const char *who) { return refuse_range(h->ctx, who); }

// ---- what the readers of the history share (observe, observe_shifted, sequence_observe, observe_memory): the two checks of
// `what` (each entry point calls them where its own header places them), the FovParams, and the launches
int hist_bad_what(agx_ctx *ctx, const char *who, int what) {
    if (what != AGX_HIST_FOVEA && what != AGX_HIST_FULL) return fail(ctx, AGX_E_INVALID, "%s: what must be AGX_HIST_FOVEA or AGX_HIST_FULL, got %d", who, what);
    return AGX_OK;
}
int hist_no_fovea(agx_ctx *ctx, const char *who, int what) {
    if (what == AGX_HIST_FOVEA && ctx->cfg.kind != AGX_KIND_FIXED)
        return fail(ctx, AGX_E_STATE, "%s: AGX_HIST_FOVEA on a context without a fovea (a base context takes AGX_HIST_FULL only)", who);
    return AGX_OK;
}

// K2's parameters for a kernel that reads history rows: no ring, no head, no fov state; a base context takes no action and
// writes no fov_loc
FovParams hist_fov_params(agx_ctx *ctx, const void *d_action, int action_dtype, void *d_obs, int32_t *d_fov_loc) {
    const bool fixed = ctx->cfg.kind == AGX_KIND_FIXED;
    FovParams p = fov_params(ctx, fixed ? d_action : nullptr, action_dtype, nullptr, nullptr, static_cast<float *>(d_obs), fixed ? d_fov_loc : nullptr, nullptr);
    p.relative = 0;            // a read-time action is absolute whatever the context's action mode
    p.ring = nullptr;
    p.head = nullptr;
    p.loc_in = p.loc_out = nullptr;
    return p;
}

// One launch of a history reader: rows [at, at + grid.y) of the call ride on gridDim.y, at most 65535 of them.
struct HistLaunch {
    int64_t at;
    dim3 grid;
    size_t lds;
    hipStream_t stream;
};
constexpr int64_t kHistRowsPerLaunch = 65535;
template <class F>
int hist_chunks(agx_ctx *ctx, int grid_x, int64_t rows, size_t lds, void *stream, F &&fn) {
    for (int64_t at = 0; at < rows; at += kHistRowsPerLaunch)
        fn(HistLaunch{at, dim3(grid_x, (unsigned)std::min<int64_t>(rows - at, kHistRowsPerLaunch)), lds, S(stream)});
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}
// ... of one that writes planes by agx_hist_plane.h: fn(tag, g, mode, L) launches its kernel <decltype(g), mode, decltype(tag)>
// for the context's observation type and geometry and the mode `what` asks for, with its own per-row pointers advanced to L.at
template <class F>
int launch_hist_planes(agx_ctx *ctx, int what, int grid_x, int64_t rows, void *stream, F &&fn) {
    const agx_config &c = ctx->cfg;
    const bool fovea = what == AGX_HIST_FOVEA;
    return hist_chunks(ctx, grid_x, rows, fovea ? ctx->plan.lds : 0, stream, [&](const HistLaunch &L) {
        with_obs_type(ctx->obs_type, [&](auto tag) {
            return with_geom(ctx->plan.headline, geom_r(c), [&](auto g) {
                auto launch = [&](auto mode) {
                    fn(tag, g, mode, L);
                    return 0;
                };
                return fovea ? with_mode(c.out_mode, launch) : launch(std::integral_constant<int, agx::kHistFull>{});
            });
        });
    });
}
// ... and of one on grid (fs, B) over a call's per-sample arrays (observe and its shifted form): fn(tag, g, mode, L, p, q)
template <class F>
int launch_hist_observe(agx_history *h, int what, const int32_t *d_env, const int64_t *d_index, int32_t B, const void *d_action, int action_dtype,
                        float *d_obs, int32_t *d_fov_loc, uint8_t *d_valid, void *stream, F &&fn) {
    agx_ctx *ctx = h->ctx;
    const agx_config &c = ctx->cfg;
    const FovParams p = hist_fov_params(ctx, d_action, action_dtype, d_obs, d_fov_loc);
    agx::HistObsParams q;
    q.h = h->p;
    q.has_loc = c.kind == AGX_KIND_FIXED ? 1 : 0;
    const size_t row_bytes = obs_row_bytes(ctx, what == AGX_HIST_FOVEA && c.out_mode == AGX_OUT_RAW);
    return launch_hist_planes(ctx, what, c.frame_stack, B, stream, [&](auto tag, auto g, auto mode, const HistLaunch &L) {
        FovParams pp = p;
        pp.obs = reinterpret_cast<float *>(reinterpret_cast<char *>(d_obs) + (size_t)L.at * row_bytes);
        if (pp.action) pp.action = static_cast<const char *>(pp.action) + (size_t)L.at * action_stride(action_dtype);
        if (pp.user_loc) pp.user_loc += 2 * (size_t)L.at;
        q.env = d_env + L.at;
        q.index = d_index + L.at;
        q.valid = d_valid ? d_valid + L.at : nullptr;
        fn(tag, g, mode, L, pp, q);
    });
}

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
    agx_history *h = new (std::nothrow) agx_history(c.device);
    if (!h) return fail(ctx, AGX_E_NOMEM, "out of host memory");
    h->ctx = ctx;
    h->T = capacity;
    const size_t T = (size_t)capacity, N = (size_t)c.num_envs, fbytes = (size_t)c.obs_h * c.obs_w;
    agx::BlockLayout lay;
    const size_t o_frames = lay.add(T * N * fbytes), o_loc = lay.add(T * N * 2 * sizeof(int32_t)), o_count = lay.add(N * sizeof(int64_t)),
                 o_age = lay.add(T * N);         // (padded to whole dwords: the scalar byte load reads the aligned dword around a byte)
    h->bytes = lay.bytes();
    DeviceGuard g(c.device);
    uint8_t *block = nullptr;
    if (int rc = hist_block(ctx, "agx_history_create", h, lay.bytes(), &block,          // counts and ages zero; frames and loc as they come
                            [&](uint8_t *b) { return hipMemset(b + o_count, 0, lay.bytes() - o_count); }))
        return rc;
    agx::HistParams &p = h->p;
    p.frames = lay.at<uint8_t>(block, o_frames);
    p.loc = lay.at<int32_t>(block, o_loc);
    p.count = lay.at<int64_t>(block, o_count);
    p.age = lay.at<uint8_t>(block, o_age);
    p.T = capacity;
    p.N = c.num_envs;
    p.fs = c.frame_stack;
    p.fbytes = (int32_t)fbytes;
    p.start_age = -1;
    *out = h;
    return AGX_OK;
}

int agx_history_destroy(agx_history *h) {
    if (!h) return AGX_OK;
    DeviceGuard g(h->own.device);
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
    const char *who = "agx_history_observe";
    if (int rc = hist_bad_what(ctx, who, what)) return rc;
    if (int rc = hist_no_fovea(ctx, who, what)) return rc;
    if (B < 0) return fail(ctx, AGX_E_INVALID, "agx_history_observe: B = %d", B);
    if (B == 0) return AGX_OK;
    if (!d_env || !d_index || !d_obs) return fail(ctx, AGX_E_INVALID, "agx_history_observe: null buffer");
    int rc = check_dt(ctx, d_action, action_dtype);
    if (rc) return rc;
    if (!full_range(ctx)) return hist_refuse_range(h, who);
    DeviceGuard g(c.device);
    return launch_hist_observe(h, what, d_env, d_index, B, d_action, action_dtype, d_obs, d_fov_loc, d_valid, stream,
                               [&](auto tag, auto g, auto mode, const HistLaunch &L, const FovParams &pp, const agx::HistObsParams &q) {
                                   hipLaunchKernelGGL((agx::k_history_observe<decltype(g), decltype(mode)::value, decltype(tag)>), L.grid,
                                                      dim3(kThreads), L.lds, L.stream, g, pp, q);
                               });
}

int agx_loop_set_history(agx_loop *l, agx_history *h) {
    if (!l) return AGX_E_INVALID;
    if (h && h->ctx != l->ctx) return lfail(l, AGX_E_INVALID, "agx_loop_set_history: the history belongs to another context");
    l->hist = h;
    return AGX_OK;
}

}  // extern "C"
