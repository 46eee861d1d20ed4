// agx_rollout_impl.h - on-policy rollouts declared in include/agx_rollout.h (included at the end of agx_api.hip, behind the
// frame history and the step log it reads): the checks and the launches of agx_k12_rollout.h.  It owns no handle and no memory.
#pragma once
#include "agx_rollout.h"

static_assert(AGX_ROLLOUT_LIMIT == agx::kRolloutLimit && AGX_ROLLOUT_CUT == agx::kRolloutCut && AGX_ROLLOUT_BOOT == agx::kRolloutBoot,
              "agx_rollout_math.h's limit and bits are the header's");

namespace {

// the argument checks every entry point here and in agx_vtrace_impl.h shares behind the handle, in the headers' order: L, then L * N
int rollout_bad_L(agx_ctx *ctx, const char *who, int32_t L, int32_t N) {
    if (L < 1 || L > AGX_ROLLOUT_LIMIT) return fail(ctx, AGX_E_INVALID, "%s: L must be 1 .. %d, got %d", who, AGX_ROLLOUT_LIMIT, L);
    if ((int64_t)L * N > INT32_MAX) return fail(ctx, AGX_E_INVALID, "%s: L * N = %lld exceeds %d", who, (long long)L * N, INT32_MAX);
    return AGX_OK;
}

// the launch of k_slot_fold<F, BOOT> over the N envs of q: one env per thread
template <class F>
int launch_slot_fold(agx_ctx *ctx, const typename F::Params &q, bool boot, void *stream) {
    const uint32_t blocks = (uint32_t)((q.N + agx::kFoldThreads - 1) / agx::kFoldThreads);
    if (boot)
        hipLaunchKernelGGL((agx::k_slot_fold<F, true>), dim3(blocks), dim3(agx::kFoldThreads), 0, S(stream), q);
    else
        hipLaunchKernelGGL((agx::k_slot_fold<F, false>), dim3(blocks), dim3(agx::kFoldThreads), 0, S(stream), q);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

}  // namespace

extern "C" {

int agx_rollout_gather(agx_steplog *log, int32_t L, int32_t *d_len, int64_t *d_obs_index, int64_t *d_next_index, float *d_reward,
                       uint8_t *d_ends, void *d_payload, void *stream) {
    const char *who = "agx_rollout_gather";
    if (!log) return fail(nullptr, AGX_E_INVALID, "%s: null argument (log)", who);
    agx_ctx *ctx = log->h->ctx;
    const int32_t N = log->h->p.N;
    if (int rc = rollout_bad_L(ctx, who, L, N)) return rc;
    if (!d_obs_index) return fail(ctx, AGX_E_INVALID, "%s: null buffer (d_obs_index)", who);
    if (!full_range(ctx)) return hist_refuse_range(log->h, who);
    DeviceGuard g(log->own.device);
    agx::RolloutOut o;
    o.len = d_len;
    o.obs_index = d_obs_index;
    o.next_index = d_next_index;
    o.reward = d_reward;
    o.ends = d_ends;
    o.payload = log->W > 0 ? static_cast<uint32_t *>(d_payload) : nullptr;
    const uint32_t blocks = (uint32_t)((N + kThreads / 64 - 1) / (kThreads / 64));
    hipLaunchKernelGGL(agx::k_rollout_gather, dim3(blocks), dim3(kThreads), 0, S(stream), steplog_params(log), L, o);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_rollout_gae(agx_history *h, int32_t L, const int32_t *d_len, const float *d_reward, const uint8_t *d_ends, const float *d_value,
                    const float *d_boot_value, float gamma, float lambda, float *d_adv, float *d_ret, void *stream) {
    const char *who = "agx_rollout_gae";
    if (!h) return fail(nullptr, AGX_E_INVALID, "%s: null argument (h)", who);
    agx_ctx *ctx = h->ctx;
    const int32_t N = h->p.N;
    if (int rc = rollout_bad_L(ctx, who, L, N)) return rc;
    if (!d_len || !d_reward || !d_ends || !d_value || !d_adv || !d_ret)
        return fail(ctx, AGX_E_INVALID, "%s: null buffer (%s)", who,
                    !d_len ? "d_len" : !d_reward ? "d_reward" : !d_ends ? "d_ends" : !d_value ? "d_value" : !d_adv ? "d_adv" : "d_ret");
    if (!full_range(ctx)) return hist_refuse_range(h, who);
    DeviceGuard g(ctx->cfg.device);
    const agx::GaeParams q{d_len, d_reward, d_ends, d_value, d_boot_value, d_adv, d_ret, N, L, gamma, lambda};
    return launch_slot_fold<agx::GaeFold>(ctx, q, d_boot_value != nullptr, stream);
}

}  // extern "C"
