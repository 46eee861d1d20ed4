// agx_replay_impl.h - the replay sampler declared in include/agx_replay.h (included at the end of agx_api.hip, behind the frame
// history it reads): the checks, the sampler's own scratch and the launches of agx_k7_replay.h.
#pragma once
#include "agx_replay.h"

struct agx_replay {
    explicit agx_replay(int device) : own(device) {}
    Resources own;                  // the one device block: off i64 [N + 1] | state u64 [3] (on the history's device: destroy needs no live history)
    agx_history *h = nullptr;
    int32_t back = 0, forward = 0, attempts = 0;
    int64_t *off = nullptr;
    uint64_t *state = nullptr;
};

namespace {

agx::ReplayParams replay_params(const agx_replay *r) {
    agx::ReplayParams p;
    p.h = r->h->p;
    p.off = r->off;
    p.state = r->state;
    p.back = r->back;
    p.forward = r->forward;
    p.attempts = r->attempts;
    return p;
}

}  // namespace

extern "C" {

int agx_replay_create(agx_history *h, int32_t back, int32_t forward, int32_t attempts, agx_replay **out) {
    agx_ctx *ctx = h ? h->ctx : nullptr;          // (no history: the message goes to agx_last_error(NULL))
    if (out) *out = nullptr;
    if (back < 0 || back > AGX_REPLAY_SPAN_LIMIT) return fail(ctx, AGX_E_INVALID, "agx_replay_create: back must be 0 .. %d, got %d", AGX_REPLAY_SPAN_LIMIT, back);
    if (forward < 0 || forward > AGX_REPLAY_SPAN_LIMIT)
        return fail(ctx, AGX_E_INVALID, "agx_replay_create: forward must be 0 .. %d, got %d", AGX_REPLAY_SPAN_LIMIT, forward);
    if (attempts < 0 || attempts > AGX_REPLAY_ATTEMPT_LIMIT)
        return fail(ctx, AGX_E_INVALID, "agx_replay_create: attempts must be 1 .. %d (0: 16), got %d", AGX_REPLAY_ATTEMPT_LIMIT, attempts);
    if (!h || !out) return fail(ctx, AGX_E_INVALID, "agx_replay_create: null argument");
    if (!full_range(ctx)) return hist_refuse_range(h, "agx_replay_create");
    agx_replay *r = new (std::nothrow) agx_replay(ctx->cfg.device);
    if (!r) return fail(ctx, AGX_E_NOMEM, "out of host memory");
    r->h = h;
    r->back = back;
    r->forward = forward;
    r->attempts = attempts == 0 ? 16 : attempts;
    agx::BlockLayout lay;
    const size_t o_off = lay.add(((size_t)h->p.N + 1) * sizeof(int64_t)), o_state = lay.add(3 * sizeof(uint64_t));
    DeviceGuard g(r->own.device);
    uint8_t *block = nullptr;
    if (int rc = hist_block(ctx, "agx_replay_create", r, lay.bytes(), &block, [&](uint8_t *b) { return hipMemset(b, 0, lay.bytes()); }))      // seed 0, calls 0
        return rc;
    r->off = lay.at<int64_t>(block, o_off);
    r->state = lay.at<uint64_t>(block, o_state);
    *out = r;
    return AGX_OK;
}

int agx_replay_destroy(agx_replay *r) {
    if (!r) return AGX_OK;
    DeviceGuard g(r->own.device);
    delete r;
    return AGX_OK;
}

int agx_replay_seed(agx_replay *r, uint64_t seed, void *stream) {
    if (!r) return AGX_E_INVALID;
    agx_ctx *ctx = r->h->ctx;
    if (!full_range(ctx)) return hist_refuse_range(r->h, "agx_replay_seed");
    DeviceGuard g(r->own.device);
    hipLaunchKernelGGL(agx::k_replay_seed, dim3(1), dim3(64), 0, S(stream), r->state, seed);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_replay_sample(agx_replay *r, int32_t B, int32_t *d_env, int64_t *d_index, uint8_t *d_ok, int64_t *d_total, void *stream) {
    if (!r) return AGX_E_INVALID;
    agx_ctx *ctx = r->h->ctx;
    if (B < 0) return fail(ctx, AGX_E_INVALID, "agx_replay_sample: B = %d", B);
    if (B > 0 && (!d_env || !d_index)) return fail(ctx, AGX_E_INVALID, "agx_replay_sample: null buffer");
    if (!full_range(ctx)) return hist_refuse_range(r->h, "agx_replay_sample");
    if (B == 0) return AGX_OK;
    DeviceGuard g(r->own.device);
    const agx::ReplayParams p = replay_params(r);
    hipLaunchKernelGGL(agx::k_replay_scan, dim3(1), dim3(kThreads), 0, S(stream), p, d_total);
    hipLaunchKernelGGL(agx::k_replay_draw, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, S(stream), p, B, d_env, d_index, d_ok);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_replay_inspect(agx_history *h, const int32_t *d_env, const int64_t *d_index, int32_t B, int32_t *d_age, int32_t *d_ahead, void *stream) {
    if (!h) return AGX_E_INVALID;
    agx_ctx *ctx = h->ctx;
    if (B < 0) return fail(ctx, AGX_E_INVALID, "agx_replay_inspect: B = %d", B);
    if (B > 0 && (!d_env || !d_index)) return fail(ctx, AGX_E_INVALID, "agx_replay_inspect: null buffer");
    if (!full_range(ctx)) return hist_refuse_range(h, "agx_replay_inspect");
    if (B == 0 || (!d_age && !d_ahead)) return AGX_OK;
    DeviceGuard g(ctx->cfg.device);
    hipLaunchKernelGGL(agx::k_replay_inspect, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, S(stream), h->p, d_env, d_index, B, d_age, d_ahead);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

}  // extern "C"
