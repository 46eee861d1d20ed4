// agx_steplog_impl.h - the step log declared in include/agx_steplog.h (included at the end of agx_api.hip, behind the replay
// sampler): the checks, the log's own storage and the launches of agx_k8_steplog.h.
#pragma once
#include "agx_steplog.h"

static_assert(AGX_STEP_TERMINATED == agx::kStepTerminated && AGX_STEP_TRUNCATED == agx::kStepTruncated, "agx_steplog_fold.h's flag bits are the header's");

struct agx_steplog {
    explicit agx_steplog(int device) : own(device) {}
    Resources own;                  // the one device block: stamp | reward | flags | payload (on the history's device: destroy needs no live history)
    agx_history *h = nullptr;
    int32_t W = 0;
    size_t bytes = 0, stamp_bytes = 0;
    float *reward = nullptr;
    uint8_t *flags = nullptr;
    int64_t *stamp = nullptr;
    uint8_t *payload = nullptr;
};

namespace {

agx::StepLogParams steplog_params(const agx_steplog *s) {
    agx::StepLogParams p;
    p.h = s->h->p;
    p.reward = s->reward;
    p.flags = s->flags;
    p.stamp = s->stamp;
    p.payload = s->payload;
    p.W = s->W;
    return p;
}

}  // namespace

extern "C" {

int agx_steplog_create(agx_history *h, int32_t payload_bytes, agx_steplog **out) {
    agx_ctx *ctx = h ? h->ctx : nullptr;          // (no history: the message goes to agx_last_error(NULL))
    if (out) *out = nullptr;
    if (payload_bytes < 0 || payload_bytes > AGX_STEPLOG_PAYLOAD_LIMIT || payload_bytes % 4)
        return fail(ctx, AGX_E_INVALID, "agx_steplog_create: payload_bytes must be 0 .. %d and a multiple of 4, got %d", AGX_STEPLOG_PAYLOAD_LIMIT,
                    payload_bytes);
    if (!h || !out) return fail(ctx, AGX_E_INVALID, "agx_steplog_create: null argument (%s)", !h ? "h" : "out");
    if (!full_range(ctx)) return hist_refuse_range(h, "agx_steplog_create");
    agx_steplog *s = new (std::nothrow) agx_steplog(ctx->cfg.device);
    if (!s) return fail(ctx, AGX_E_NOMEM, "out of host memory");
    s->h = h;
    s->W = payload_bytes;
    const size_t rows = (size_t)h->p.T * h->p.N;
    agx::BlockLayout lay;
    const size_t o_stamp = lay.add(rows * sizeof(int64_t)), o_reward = lay.add(rows * sizeof(float)), o_flags = lay.add(rows),
                 o_payload = lay.add(rows * (size_t)payload_bytes);
    s->bytes = lay.bytes();
    s->stamp_bytes = rows * sizeof(int64_t);
    DeviceGuard g(s->own.device);
    uint8_t *block = nullptr;
    if (int rc = hist_block(ctx, "agx_steplog_create", s, lay.bytes(), &block, [&](uint8_t *b) {
            const hipError_t e = hipMemset(b, 0xFF, o_reward);                              // the stamp section: every row unrecorded
            return e != hipSuccess ? e : hipMemset(b + o_reward, 0, lay.bytes() - o_reward);
        }))
        return rc;
    s->stamp = lay.at<int64_t>(block, o_stamp);
    s->reward = lay.at<float>(block, o_reward);
    s->flags = lay.at<uint8_t>(block, o_flags);
    s->payload = lay.at<uint8_t>(block, o_payload);
    *out = s;
    return AGX_OK;
}

int agx_steplog_destroy(agx_steplog *s) {
    if (!s) return AGX_OK;
    DeviceGuard g(s->own.device);
    delete s;
    return AGX_OK;
}

int agx_steplog_clear(agx_steplog *s, void *stream) {
    if (!s) return fail(nullptr, AGX_E_INVALID, "agx_steplog_clear: null argument (s)");
    DeviceGuard g(s->own.device);
    AGX_HIP(s->h->ctx, hipMemsetAsync(s->stamp, 0xFF, s->stamp_bytes, S(stream)));
    return AGX_OK;
}

int64_t agx_steplog_bytes(const agx_steplog *s) { return s ? (int64_t)s->bytes : AGX_E_INVALID; }

int agx_steplog_record(agx_steplog *s, const int64_t *d_index, const float *d_reward, const uint8_t *d_flags, const void *d_payload,
                       void *stream) {
    if (!s) return fail(nullptr, AGX_E_INVALID, "agx_steplog_record: null argument (s)");
    agx_ctx *ctx = s->h->ctx;
    if (!d_index || !d_reward || !d_flags)
        return fail(ctx, AGX_E_INVALID, "agx_steplog_record: null buffer (%s)", !d_index ? "d_index" : !d_reward ? "d_reward" : "d_flags");
    if (s->W > 0 && !d_payload) return fail(ctx, AGX_E_INVALID, "agx_steplog_record: null buffer (d_payload) on a log with %d payload bytes", s->W);
    if (!full_range(ctx)) return hist_refuse_range(s->h, "agx_steplog_record");
    DeviceGuard g(s->own.device);
    const int N = s->h->p.N;
    const uint32_t blocks = (uint32_t)(((int64_t)N + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(agx::k_steplog_record, dim3(blocks), dim3(kThreads), 0, S(stream), steplog_params(s), d_index, d_reward,
                       d_flags, static_cast<const uint32_t *>(d_payload));
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_steplog_gather(agx_steplog *s, const int32_t *d_env, const int64_t *d_index, int32_t B, int32_t nstep, float gamma, float *d_return,
                       float *d_discount, int32_t *d_steps, int64_t *d_next_index, uint8_t *d_flags, void *d_payload, void *stream) {
    agx_ctx *ctx = s ? s->h->ctx : nullptr;
    if (nstep < 1 || nstep > AGX_STEPLOG_NSTEP_LIMIT)
        return fail(ctx, AGX_E_INVALID, "agx_steplog_gather: nstep must be 1 .. %d, got %d", AGX_STEPLOG_NSTEP_LIMIT, nstep);
    if (B < 0) return fail(ctx, AGX_E_INVALID, "agx_steplog_gather: B must be >= 0, got %d", B);
    if (!s) return fail(ctx, AGX_E_INVALID, "agx_steplog_gather: null argument (s)");
    if (B > 0 && (!d_env || !d_index || !d_steps))
        return fail(ctx, AGX_E_INVALID, "agx_steplog_gather: null buffer (%s)", !d_env ? "d_env" : !d_index ? "d_index" : "d_steps");
    if (!full_range(ctx)) return hist_refuse_range(s->h, "agx_steplog_gather");
    if (B == 0) return AGX_OK;
    DeviceGuard g(s->own.device);
    agx::StepLogOut o;
    o.ret = d_return;
    o.discount = d_discount;
    o.steps = d_steps;
    o.next_index = d_next_index;
    o.flags = d_flags;
    o.payload = s->W > 0 ? static_cast<uint32_t *>(d_payload) : nullptr;
    const uint32_t blocks = (uint32_t)(((int64_t)B + kThreads - 1) / kThreads);      // (in 64 bits: B may be INT32_MAX)
    hipLaunchKernelGGL(agx::k_steplog_gather, dim3(blocks), dim3(kThreads), 0, S(stream), steplog_params(s), d_env, d_index, B,
                       nstep, gamma, o);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

}  // extern "C"
