// agx_augment_impl.h - the random-shift augmentation declared in include/agx_augment.h (included at the end of agx_api.hip,
// behind the frame history it reads): the checks, the shift source's own scratch and the launches of agx_k10_augment.h.
#pragma once
#include "agx_augment.h"

struct agx_shift {
    explicit agx_shift(int device) : own(device) {}
    Resources own;                  // the one device block, below (on the history's device: destroy needs no live history)
    agx_history *h = nullptr;
    int32_t pad = 0;
    uint64_t *state = nullptr;      // u64 [3] seed, calls, the draw launch's ticket counter
};

namespace {

int shift_bad_pad(agx_ctx *ctx, const char *who, int32_t pad) {
    return fail(ctx, AGX_E_INVALID, "%s: pad must be 0 .. %d, got %d", who, AGX_SHIFT_PAD_LIMIT, pad);
}

}  // namespace

extern "C" {

int agx_shift_create(agx_history *h, int32_t pad, agx_shift **out) {
    agx_ctx *ctx = h ? h->ctx : nullptr;          // (no history: the message goes to agx_last_error(NULL))
    if (out) *out = nullptr;
    if (pad < 0 || pad > AGX_SHIFT_PAD_LIMIT) return shift_bad_pad(ctx, "agx_shift_create", pad);
    if (!out) return fail(ctx, AGX_E_INVALID, "agx_shift_create: null out");
    if (!h) return fail(ctx, AGX_E_INVALID, "agx_shift_create: null h");
    if (!full_range(ctx)) return hist_refuse_range(h, "agx_shift_create");
    agx_shift *s = new (std::nothrow) agx_shift(ctx->cfg.device);
    if (!s) return fail(ctx, AGX_E_NOMEM, "out of host memory");
    s->h = h;
    s->pad = pad;
    agx::BlockLayout lay;
    const size_t o_state = lay.add(3 * sizeof(uint64_t));
    DeviceGuard g(s->own.device);
    uint8_t *block = nullptr;
    if (int rc = hist_block(ctx, "agx_shift_create", s, lay.bytes(), &block, [&](uint8_t *b) { return hipMemset(b, 0, lay.bytes()); }))      // seed 0, calls 0, no ticket taken
        return rc;
    s->state = lay.at<uint64_t>(block, o_state);
    *out = s;
    return AGX_OK;
}

int agx_shift_destroy(agx_shift *s) {
    if (!s) return AGX_OK;
    DeviceGuard g(s->own.device);
    delete s;
    return AGX_OK;
}

int agx_shift_seed(agx_shift *s, uint64_t seed, void *stream) {
    if (!s) return fail(nullptr, AGX_E_INVALID, "agx_shift_seed: null s");
    agx_ctx *ctx = s->h->ctx;
    if (!full_range(ctx)) return hist_refuse_range(s->h, "agx_shift_seed");
    DeviceGuard g(s->own.device);
    hipLaunchKernelGGL(agx::k_shift_seed, dim3(1), dim3(64), 0, S(stream), s->state, seed);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_shift_draw(agx_shift *s, int32_t B, int32_t *d_shift, void *stream) {
    agx_ctx *ctx = s ? s->h->ctx : nullptr;       // (the argument checks need no source: they come first)
    if (B < 0) return fail(ctx, AGX_E_INVALID, "agx_shift_draw: B = %d", B);
    if (B > 0 && !d_shift) return fail(ctx, AGX_E_INVALID, "agx_shift_draw: null d_shift");
    if (!s) return fail(ctx, AGX_E_INVALID, "agx_shift_draw: null s");
    if (!full_range(ctx)) return hist_refuse_range(s->h, "agx_shift_draw");
    if (B == 0) return AGX_OK;
    DeviceGuard g(s->own.device);
    hipLaunchKernelGGL(agx::k_shift_draw, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, S(stream), s->state, s->pad, B, d_shift);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_history_observe_shifted(agx_history *h, int what, const int32_t *d_env, const int64_t *d_index, int32_t B, const void *d_action,
                                int action_dtype, int32_t pad, const int32_t *d_shift, float *d_obs, int32_t *d_fov_loc, uint8_t *d_valid,
                                void *stream) {
    agx_ctx *ctx = h ? h->ctx : nullptr;          // (the argument checks need no history: they come first)
    const char *who = "agx_history_observe_shifted";
    if (int rc = hist_bad_what(ctx, who, what)) return rc;
    if (pad < 0 || pad > AGX_SHIFT_PAD_LIMIT) return shift_bad_pad(ctx, who, pad);
    if (B < 0) return fail(ctx, AGX_E_INVALID, "agx_history_observe_shifted: B = %d", B);
    if (B > 0) {
        if (!d_env) return fail(ctx, AGX_E_INVALID, "agx_history_observe_shifted: null d_env");
        if (!d_index) return fail(ctx, AGX_E_INVALID, "agx_history_observe_shifted: null d_index");
        if (!d_shift) return fail(ctx, AGX_E_INVALID, "agx_history_observe_shifted: null d_shift");
        if (!d_obs) return fail(ctx, AGX_E_INVALID, "agx_history_observe_shifted: null d_obs");
    }
    int rc = check_dt(ctx, d_action, action_dtype);
    if (rc) return rc;
    if (!h) return fail(ctx, AGX_E_INVALID, "agx_history_observe_shifted: null h");
    if (int rc2 = hist_no_fovea(ctx, who, what)) return rc2;
    if (B == 0) return AGX_OK;                    // (before the range check, as in agx_history_observe)
    if (!full_range(ctx)) return hist_refuse_range(h, who);
    DeviceGuard g(ctx->cfg.device);
    return launch_hist_observe(h, what, d_env, d_index, B, d_action, action_dtype, d_obs, d_fov_loc, d_valid, stream,
                               [&](auto tag, auto g, auto mode, const HistLaunch &L, const FovParams &pp, const agx::HistObsParams &q) {
                                   const agx::ShiftObsParams sh{d_shift + 2 * (size_t)L.at, pad};
                                   hipLaunchKernelGGL((agx::k_history_observe_shifted<decltype(g), decltype(mode)::value, decltype(tag)>), L.grid,
                                                      dim3(kThreads), L.lds, L.stream, g, pp, q, sh);
                               });
}

}  // extern "C"
