// agx_priority_impl.h - the prioritized sampler declared in include/agx_priority.h (included at the end of agx_api.hip, behind
// the step log): the checks, the table's own storage and the launches of agx_k9_priority.h.
#pragma once
#include "agx_priority.h"

static_assert(agx::kPrioChunk + 2 * AGX_REPLAY_SPAN_LIMIT <= agx::kPrioRow, "the age tile of k_priority_weights holds a chunk and both spans");

struct agx_priority {
    explicit agx_priority(int device) : own(device) {}
    Resources own;                  // the one device block: stamp | incl | csum | envsum | envacc | off | state | weight | cacc | wmax
                                    // (on the history's device: destroy needs no live history)
    agx_history *h = nullptr;
    int32_t back = 0, forward = 0, CH = 0;
    size_t bytes = 0;
    int64_t rows = 0;               // T * N
    int64_t *stamp = nullptr, *incl = nullptr, *csum = nullptr, *envsum = nullptr, *envacc = nullptr, *off = nullptr;
    uint64_t *state = nullptr;
    uint32_t *weight = nullptr, *wmax = nullptr;
    int32_t *cacc = nullptr;
};

namespace {

agx::PriorityParams priority_params(const agx_priority *t) {
    agx::PriorityParams p;
    p.h = t->h->p;
    p.stamp = t->stamp;
    p.weight = t->weight;
    p.wmax = t->wmax;
    p.incl = t->incl;
    p.csum = t->csum;
    p.cacc = t->cacc;
    p.envsum = t->envsum;
    p.envacc = t->envacc;
    p.off = t->off;
    p.state = t->state;
    p.back = t->back;
    p.forward = t->forward;
    p.CH = t->CH;
    return p;
}

uint32_t priority_blocks(int64_t items, int per_block) { return (uint32_t)((items + per_block - 1) / per_block); }

// the checks update and lookup share; 1: go on, otherwise the value to return
int priority_pairs(agx_priority *t, const char *who, const void *d_env, const void *d_index, const void *d_third, const char *third, int32_t B) {
    agx_ctx *ctx = t ? t->h->ctx : nullptr;
    if (B < 0) return fail(ctx, AGX_E_INVALID, "%s: B must be >= 0, got %d", who, B);
    if (!t) return fail(ctx, AGX_E_INVALID, "%s: null argument (p)", who);
    if (B > 0 && (!d_env || !d_index || !d_third))
        return fail(ctx, AGX_E_INVALID, "%s: null buffer (%s)", who, !d_env ? "d_env" : !d_index ? "d_index" : third);
    if (!full_range(ctx)) return hist_refuse_range(t->h, who);
    return B == 0 ? AGX_OK : 1;
}

}  // namespace

extern "C" {

int agx_priority_create(agx_history *h, int32_t back, int32_t forward, agx_priority **out) {
    agx_ctx *ctx = h ? h->ctx : nullptr;          // (no history: the message goes to agx_last_error(NULL))
    if (out) *out = nullptr;
    if (back < 0 || back > AGX_REPLAY_SPAN_LIMIT)
        return fail(ctx, AGX_E_INVALID, "agx_priority_create: back must be 0 .. %d, got %d", AGX_REPLAY_SPAN_LIMIT, back);
    if (forward < 0 || forward > AGX_REPLAY_SPAN_LIMIT)
        return fail(ctx, AGX_E_INVALID, "agx_priority_create: forward must be 0 .. %d, got %d", AGX_REPLAY_SPAN_LIMIT, forward);
    if (!h || !out) return fail(ctx, AGX_E_INVALID, "agx_priority_create: null argument (%s)", !h ? "h" : "out");
    const int64_t T = h->p.T, N = h->p.N;
    if (T * N >= ((int64_t)1 << 31))
        return fail(ctx, AGX_E_INVALID, "agx_priority_create: T * N must be below 2^31 rows (the i64 sums of u32 weights), got %lld x %lld",
                    (long long)T, (long long)N);
    if (!full_range(ctx)) return hist_refuse_range(h, "agx_priority_create");
    agx_priority *t = new (std::nothrow) agx_priority(ctx->cfg.device);
    if (!t) return fail(ctx, AGX_E_NOMEM, "out of host memory");
    t->h = h;
    t->back = back;
    t->forward = forward;
    t->rows = T * N;
    t->CH = (int32_t)((T + agx::kPrioChunk - 1) / agx::kPrioChunk);
    const size_t rows = (size_t)t->rows, chunks = (size_t)N * t->CH;
    agx::BlockLayout lay;
    const size_t o_stamp = lay.add(rows * sizeof(int64_t)), o_incl = lay.add(rows * sizeof(int64_t)), o_csum = lay.add(chunks * sizeof(int64_t)),
                 o_envsum = lay.add((size_t)N * sizeof(int64_t)), o_envacc = lay.add((size_t)N * sizeof(int64_t)),
                 o_off = lay.add(((size_t)N + 1) * sizeof(int64_t)), o_state = lay.add(3 * sizeof(uint64_t)),
                 o_weight = lay.add(rows * sizeof(uint32_t)), o_cacc = lay.add(chunks * sizeof(int32_t)), o_wmax = lay.add(sizeof(uint32_t));
    t->bytes = lay.bytes();
    const uint32_t one = agx::kPriorityOne;
    DeviceGuard g(t->own.device);
    uint8_t *block = nullptr;
    if (int rc = hist_block(ctx, "agx_priority_create", t, lay.bytes(), &block, [&](uint8_t *b) {
            hipError_t e = hipMemset(b, 0xFF, o_incl);                                      // the stamp section: every row unset
            if (e == hipSuccess) e = hipMemset(b + o_incl, 0, lay.bytes() - o_incl);        // seed 0, calls 0
            return e != hipSuccess ? e : hipMemcpy(b + o_wmax, &one, sizeof(one), hipMemcpyHostToDevice);
        }))
        return rc;
    t->stamp = lay.at<int64_t>(block, o_stamp);
    t->incl = lay.at<int64_t>(block, o_incl);
    t->csum = lay.at<int64_t>(block, o_csum);
    t->envsum = lay.at<int64_t>(block, o_envsum);
    t->envacc = lay.at<int64_t>(block, o_envacc);
    t->off = lay.at<int64_t>(block, o_off);
    t->state = lay.at<uint64_t>(block, o_state);
    t->weight = lay.at<uint32_t>(block, o_weight);
    t->cacc = lay.at<int32_t>(block, o_cacc);
    t->wmax = lay.at<uint32_t>(block, o_wmax);
    *out = t;
    return AGX_OK;
}

int agx_priority_destroy(agx_priority *t) {
    if (!t) return AGX_OK;
    DeviceGuard g(t->own.device);
    delete t;
    return AGX_OK;
}

int64_t agx_priority_bytes(const agx_priority *t) { return t ? (int64_t)t->bytes : AGX_E_INVALID; }

int agx_priority_seed(agx_priority *t, uint64_t seed, void *stream) {
    if (!t) return fail(nullptr, AGX_E_INVALID, "agx_priority_seed: null argument (p)");
    agx_ctx *ctx = t->h->ctx;
    if (!full_range(ctx)) return hist_refuse_range(t->h, "agx_priority_seed");
    DeviceGuard g(t->own.device);
    hipLaunchKernelGGL(agx::k_priority_seed, dim3(1), dim3(64), 0, S(stream), t->state, seed);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_priority_clear(agx_priority *t, void *stream) {
    if (!t) return fail(nullptr, AGX_E_INVALID, "agx_priority_clear: null argument (p)");
    agx_ctx *ctx = t->h->ctx;
    if (!full_range(ctx)) return hist_refuse_range(t->h, "agx_priority_clear");
    DeviceGuard g(t->own.device);
    hipLaunchKernelGGL(agx::k_priority_clear, dim3(priority_blocks(t->rows, kThreads)), dim3(kThreads), 0, S(stream), t->stamp, t->wmax, t->rows);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_priority_update(agx_priority *t, const int32_t *d_env, const int64_t *d_index, const float *d_priority, int32_t B, void *stream) {
    const int rc = priority_pairs(t, "agx_priority_update", d_env, d_index, d_priority, "d_priority", B);
    if (rc != 1) return rc;
    DeviceGuard g(t->own.device);
    hipLaunchKernelGGL(agx::k_priority_update, dim3(priority_blocks(B, kThreads)), dim3(kThreads), 0, S(stream), priority_params(t), d_env, d_index,
                       d_priority, B);
    AGX_HIP(t->h->ctx, hipGetLastError());
    return AGX_OK;
}

int agx_priority_lookup(agx_priority *t, const int32_t *d_env, const int64_t *d_index, int32_t B, int64_t *d_weight, void *stream) {
    const int rc = priority_pairs(t, "agx_priority_lookup", d_env, d_index, d_weight, "d_weight", B);
    if (rc != 1) return rc;
    DeviceGuard g(t->own.device);
    hipLaunchKernelGGL(agx::k_priority_lookup, dim3(priority_blocks(B, kThreads)), dim3(kThreads), 0, S(stream), priority_params(t), d_env, d_index,
                       B, d_weight);
    AGX_HIP(t->h->ctx, hipGetLastError());
    return AGX_OK;
}

int agx_priority_sample(agx_priority *t, int32_t B, int32_t *d_env, int64_t *d_index, uint8_t *d_ok, int64_t *d_weight, int64_t *d_total,
                        int64_t *d_accepted, void *stream) {
    agx_ctx *ctx = t ? t->h->ctx : nullptr;
    if (B < 0) return fail(ctx, AGX_E_INVALID, "agx_priority_sample: B must be >= 0, got %d", B);
    if (!t) return fail(ctx, AGX_E_INVALID, "agx_priority_sample: null argument (p)");
    if (B > 0 && (!d_env || !d_index)) return fail(ctx, AGX_E_INVALID, "agx_priority_sample: null buffer (%s)", !d_env ? "d_env" : "d_index");
    if (!full_range(ctx)) return hist_refuse_range(t->h, "agx_priority_sample");
    if (B == 0) return AGX_OK;
    DeviceGuard g(t->own.device);
    const agx::PriorityParams p = priority_params(t);
    const int64_t groups = ((int64_t)p.h.N + agx::kPrioGroup - 1) / agx::kPrioGroup;      // groups * CH < 2^31 / 1024 + N + CH
    hipLaunchKernelGGL(agx::k_priority_weights, dim3((uint32_t)(groups * p.CH)), dim3(kThreads), 0, S(stream), p);
    hipLaunchKernelGGL(agx::k_priority_chunks, dim3(priority_blocks(p.h.N, kThreads / 64)), dim3(kThreads), 0, S(stream), p);
    hipLaunchKernelGGL(agx::k_priority_scan, dim3(1), dim3(kThreads), 0, S(stream), p, d_total, d_accepted);
    hipLaunchKernelGGL(agx::k_priority_draw, dim3(priority_blocks(B, kThreads)), dim3(kThreads), 0, S(stream), p, B, d_env, d_index, d_ok, d_weight);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

}  // extern "C"
