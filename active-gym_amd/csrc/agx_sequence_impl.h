// agx_sequence_impl.h - sequence replay declared in include/agx_sequence.h (included at the end of agx_api.hip, behind the frame
// history and the step log it reads): the checks and the launches of agx_k11_sequence.h.  It owns no handle and no memory.
#pragma once
#include "agx_sequence.h"

static_assert(AGX_SEQUENCE_LIMIT == agx::kSequenceLimit, "agx_sequence_math.h's limit is the header's");

namespace {

// the argument checks the three entry points share, in the header's order: L, then (the caller's own in between), B, B * L
int seq_bad_L(agx_ctx *ctx, const char *who, int32_t L) {
    return fail(ctx, AGX_E_INVALID, "%s: L must be 1 .. %d, got %d", who, AGX_SEQUENCE_LIMIT, L);
}
int seq_bad_B(agx_ctx *ctx, const char *who, int32_t B, int32_t L) {
    if (B < 0) return fail(ctx, AGX_E_INVALID, "%s: B must be >= 0, got %d", who, B);
    if ((int64_t)B * L > INT32_MAX) return fail(ctx, AGX_E_INVALID, "%s: B * L = %lld exceeds %d", who, (long long)B * L, INT32_MAX);
    return AGX_OK;
}

int seq_launch_gather(agx_ctx *ctx, bool walk, const agx::StepLogParams &p, const agx::SeqParams &q, int32_t nstep, float gamma,
                      const agx::StepLogOut &o, void *stream) {
    const uint32_t blocks = (uint32_t)(((int64_t)q.B + kThreads / 64 - 1) / (kThreads / 64));      // (B <= INT32_MAX: below 2^29 blocks)
    if (walk)
        hipLaunchKernelGGL(agx::k_sequence_gather<true>, dim3(blocks), dim3(kThreads), 0, S(stream), p, q, nstep, gamma, o);
    else
        hipLaunchKernelGGL(agx::k_sequence_gather<false>, dim3(blocks), dim3(kThreads), 0, S(stream), p, q, nstep, gamma, o);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

}  // namespace

extern "C" {

int agx_sequence_lengths(agx_history *h, const int32_t *d_env, const int64_t *d_index, int32_t B, int32_t L, int32_t *d_len, void *stream) {
    agx_ctx *ctx = h ? h->ctx : nullptr;          // (the argument checks need no history: they come first)
    const char *who = "agx_sequence_lengths";
    if (L < 1 || L > AGX_SEQUENCE_LIMIT) return seq_bad_L(ctx, who, L);
    if (int rc = seq_bad_B(ctx, who, B, L)) return rc;
    if (B > 0 && (!d_env || !d_index || !d_len))
        return fail(ctx, AGX_E_INVALID, "%s: null buffer (%s)", who, !d_env ? "d_env" : !d_index ? "d_index" : "d_len");
    if (!h) return fail(ctx, AGX_E_INVALID, "%s: null argument (h)", who);
    if (B == 0) return AGX_OK;                    // (before the range check, as in agx_history_observe)
    if (!full_range(ctx)) return hist_refuse_range(h, who);
    DeviceGuard g(ctx->cfg.device);
    agx::StepLogParams p{};
    p.h = h->p;
    const agx::SeqParams q{d_env, d_index, d_len, B, L, 0};
    return seq_launch_gather(ctx, false, p, q, 1, 0.0f, agx::StepLogOut{}, stream);
}

int agx_sequence_gather(agx_steplog *log, const int32_t *d_env, const int64_t *d_index, int32_t B, int32_t L, int32_t nstep, float gamma,
                        int time_major, int32_t *d_len, int32_t *d_steps, int64_t *d_next_index, float *d_ret, float *d_discount,
                        uint8_t *d_flags, void *d_payload, void *stream) {
    agx_ctx *ctx = log ? log->h->ctx : nullptr;
    const char *who = "agx_sequence_gather";
    if (L < 1 || L > AGX_SEQUENCE_LIMIT) return seq_bad_L(ctx, who, L);
    if (nstep < 1 || nstep > AGX_STEPLOG_NSTEP_LIMIT)
        return fail(ctx, AGX_E_INVALID, "%s: nstep must be 1 .. %d, got %d", who, AGX_STEPLOG_NSTEP_LIMIT, nstep);
    if (int rc = seq_bad_B(ctx, who, B, L)) return rc;
    if (B > 0 && (!d_env || !d_index || !d_steps))
        return fail(ctx, AGX_E_INVALID, "%s: null buffer (%s)", who, !d_env ? "d_env" : !d_index ? "d_index" : "d_steps");
    if (!log) return fail(ctx, AGX_E_INVALID, "%s: null argument (log)", who);
    if (B == 0) return AGX_OK;
    if (!full_range(ctx)) return hist_refuse_range(log->h, who);
    DeviceGuard g(log->own.device);
    agx::StepLogOut o;
    o.ret = d_ret;
    o.discount = d_discount;
    o.steps = d_steps;
    o.next_index = d_next_index;
    o.flags = d_flags;
    o.payload = log->W > 0 ? static_cast<uint32_t *>(d_payload) : nullptr;
    const agx::SeqParams q{d_env, d_index, d_len, B, L, time_major ? 1 : 0};
    return seq_launch_gather(ctx, true, steplog_params(log), q, nstep, gamma, o, stream);
}

int agx_sequence_observe(agx_history *h, int what, const int32_t *d_env, const int64_t *d_index, const int32_t *d_len, int32_t B, int32_t L,
                         int32_t planes, int time_major, void *d_obs, int32_t *d_fov_loc, uint8_t *d_live, void *stream) {
    agx_ctx *ctx = h ? h->ctx : nullptr;
    const char *who = "agx_sequence_observe";
    if (L < 1 || L > AGX_SEQUENCE_LIMIT) return seq_bad_L(ctx, who, L);
    if (int rc = hist_bad_what(ctx, who, what)) return rc;
    if (planes < 1) return fail(ctx, AGX_E_INVALID, "%s: planes must be >= 1, got %d", who, planes);
    if (int rc = seq_bad_B(ctx, who, B, L)) return rc;
    if (B > 0 && (!d_env || !d_index || !d_len || !d_obs))
        return fail(ctx, AGX_E_INVALID, "%s: null buffer (%s)", who, !d_env ? "d_env" : !d_index ? "d_index" : !d_len ? "d_len" : "d_obs");
    if (!h) return fail(ctx, AGX_E_INVALID, "%s: null argument (h)", who);
    const agx_config &c = ctx->cfg;
    if (planes > c.frame_stack) return fail(ctx, AGX_E_INVALID, "%s: planes = %d exceeds frame_stack %d", who, planes, c.frame_stack);
    if (int rc = hist_no_fovea(ctx, who, what)) return rc;
    if (B == 0) return AGX_OK;                    // (before the range check, as in agx_history_observe)
    if (!full_range(ctx)) return hist_refuse_range(h, who);
    DeviceGuard g(c.device);
    const FovParams p = hist_fov_params(ctx, nullptr, 0, d_obs, d_fov_loc);
    agx::SeqObsParams q;
    q.h = h->p;
    q.env = d_env;
    q.index = d_index;
    q.len = d_len;
    q.live = d_live;
    q.B = B;
    q.L = L;
    q.planes = planes;
    q.time_major = time_major ? 1 : 0;
    q.has_loc = c.kind == AGX_KIND_FIXED ? 1 : 0;
    // the output row rides on gridDim.y: each launch is told its first row, and the kernel places its own outputs
    return launch_hist_planes(ctx, what, planes, (int64_t)B * L, stream, [&](auto tag, auto g, auto mode, const HistLaunch &ln) {
        q.row0 = (int32_t)ln.at;
        hipLaunchKernelGGL((agx::k_sequence_observe<decltype(g), decltype(mode)::value, decltype(tag)>), ln.grid, dim3(kThreads), ln.lds, ln.stream, g, p, q);
    });
}

}  // extern "C"
