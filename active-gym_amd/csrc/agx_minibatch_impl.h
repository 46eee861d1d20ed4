// agx_minibatch_impl.h - the minibatcher declared in include/agx_minibatch.h (included at the end of agx_api.hip, behind the frame
// history and agx_vtrace_impl.h; the L check is agx_rollout_impl.h's): the checks, the minibatcher's own scratch and the launches
// of agx_k15_minibatch.h.
#pragma once
#include "agx_minibatch.h"

static_assert(AGX_MB_LIMIT == agx::kMbLimit && AGX_MB_LIMIT == AGX_ROLLOUT_LIMIT, "the limit is that of a gathered rollout");
static_assert(AGX_MB_LIVE == agx::kMbLive && AGX_MB_BOOT == agx::kMbBoot && AGX_MB_STREAMS == agx::kMbStreams, "agx_minibatch_math.h's constants are the header's");
static_assert(agx::kMbBootBit == AGX_ROLLOUT_BOOT, "the BOOT bit is the gather's");

struct agx_minibatch {
    explicit agx_minibatch(int device) : own(device) {}
    Resources own;                  // the one device block: off i32 [2][N + 1] | cnt i32 [N] | state u64 [2][3] (on the history's device: destroy
                                    // needs no live history)
    agx_history *h = nullptr;
    int32_t *off = nullptr, *cnt = nullptr;
    uint64_t *state = nullptr;
};

namespace {

// the checks select and take share behind the handle, in the header's order: which, then L and L * N
int mb_bad_list(agx_ctx *ctx, const char *who, int which, int32_t L, int32_t N) {
    if (which != AGX_MB_LIVE && which != AGX_MB_BOOT)
        return fail(ctx, AGX_E_INVALID, "%s: which must be AGX_MB_LIVE (0) or AGX_MB_BOOT (1), got %d", who, which);
    return rollout_bad_L(ctx, who, L, N);
}

}  // namespace

extern "C" {

int agx_minibatch_create(agx_history *h, uint64_t seed, agx_minibatch **out) {
    agx_ctx *ctx = h ? h->ctx : nullptr;          // (no history: the message goes to agx_last_error(NULL))
    if (out) *out = nullptr;
    if (!h || !out) return fail(ctx, AGX_E_INVALID, "agx_minibatch_create: null argument");
    if (!full_range(ctx)) return hist_refuse_range(h, "agx_minibatch_create");
    agx_minibatch *mb = new (std::nothrow) agx_minibatch(ctx->cfg.device);
    if (!mb) return fail(ctx, AGX_E_NOMEM, "out of host memory");
    mb->h = h;
    const size_t N = (size_t)h->p.N;
    agx::BlockLayout lay;
    const size_t o_off = lay.add(2 * (N + 1) * sizeof(int32_t)), o_cnt = lay.add(N * sizeof(int32_t)), o_state = lay.add(6 * sizeof(uint64_t));
    uint64_t state[6];
    for (int which = 0; which < 2; ++which) {
        state[which * 3 + 0] = agx::replay_sm(seed, (uint64_t)which);     // base
        state[which * 3 + 1] = 0;                                         // calls
        state[which * 3 + 2] = 0;                                         // the key in flight: none yet (both totals are 0)
    }
    DeviceGuard g(mb->own.device);
    uint8_t *block = nullptr;
    if (int rc = hist_block(ctx, "agx_minibatch_create", mb, lay.bytes(), &block, [&](uint8_t *b) {
            const hipError_t e = hipMemset(b, 0, lay.bytes());
            return e != hipSuccess ? e : hipMemcpy(b + o_state, state, sizeof state, hipMemcpyHostToDevice);
        }))
        return rc;
    mb->off = lay.at<int32_t>(block, o_off);
    mb->cnt = lay.at<int32_t>(block, o_cnt);
    mb->state = lay.at<uint64_t>(block, o_state);
    *out = mb;
    return AGX_OK;
}

int agx_minibatch_destroy(agx_minibatch *mb) {
    if (!mb) return AGX_OK;
    DeviceGuard g(mb->own.device);
    delete mb;
    return AGX_OK;
}

int agx_minibatch_select(agx_minibatch *mb, int which, int32_t L, const int32_t *d_len, const uint8_t *d_ends, int32_t *d_total, void *stream) {
    const char *who = "agx_minibatch_select";
    if (!mb) return fail(nullptr, AGX_E_INVALID, "%s: null argument (mb)", who);
    agx_ctx *ctx = mb->h->ctx;
    const int32_t N = mb->h->p.N;
    if (int rc = mb_bad_list(ctx, who, which, L, N)) return rc;
    if (!d_len || (which == AGX_MB_BOOT && !d_ends)) return fail(ctx, AGX_E_INVALID, "%s: null buffer (%s)", who, !d_len ? "d_len" : "d_ends");
    if (!full_range(ctx)) return hist_refuse_range(mb->h, who);
    DeviceGuard g(mb->own.device);
    int32_t *off = mb->off + (size_t)which * (N + 1);
    if (which == AGX_MB_BOOT)
        hipLaunchKernelGGL(agx::k_mb_count, dim3((N + agx::kMbCountThreads - 1) / agx::kMbCountThreads), dim3(agx::kMbCountThreads), 0, S(stream), d_len,
                           d_ends, N, L, mb->cnt);
    hipLaunchKernelGGL(agx::k_mb_scan, dim3(1), dim3(kThreads), 0, S(stream), which, which == AGX_MB_BOOT ? mb->cnt : d_len, N, L, off,
                       mb->state + which * 3, d_total);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_minibatch_take(agx_minibatch *mb, int which, int permute, int32_t L, const int32_t *d_len, const uint8_t *d_ends, int32_t first, int32_t S_,
                       const agx_minibatch_io *io, void *stream) {
    const char *who = "agx_minibatch_take";
    if (!mb) return fail(nullptr, AGX_E_INVALID, "%s: null argument (mb)", who);
    agx_ctx *ctx = mb->h->ctx;
    const int32_t N = mb->h->p.N;
    if (int rc = mb_bad_list(ctx, who, which, L, N)) return rc;
    if (S_ < 0 || first < 0 || (int64_t)first + S_ > INT32_MAX)
        return fail(ctx, AGX_E_INVALID, "%s: first = %d, S = %d (both >= 0, first + S <= %d)", who, first, S_, INT32_MAX);
    if (!io) return fail(ctx, AGX_E_INVALID, "%s: null argument (io)", who);
    if (io->n_f32 < 0 || io->n_f32 > AGX_MB_STREAMS) return fail(ctx, AGX_E_INVALID, "%s: n_f32 must be 0 .. %d, got %d", who, AGX_MB_STREAMS, io->n_f32);
    if (!d_len || (which == AGX_MB_BOOT && !d_ends) || !io->d_slot)
        return fail(ctx, AGX_E_INVALID, "%s: null buffer (%s)", who, !d_len ? "d_len" : !io->d_slot ? "d_slot" : "d_ends");
    if (!full_range(ctx)) return hist_refuse_range(mb->h, who);
    if (S_ == 0) return AGX_OK;
    DeviceGuard g(mb->own.device);
    agx::MbTake q;
    q.off = mb->off + (size_t)which * (N + 1);
    q.state = mb->state + which * 3;
    q.len = d_len;
    q.ends = d_ends;
    q.obs_index = io->d_obs_index;
    q.next_index = io->d_next_index;
    q.payload = static_cast<const uint8_t *>(io->d_payload);
    q.slot = io->d_slot;
    q.env = io->d_env;
    q.obs_index_out = io->d_obs_index_out;
    q.next_index_out = io->d_next_index_out;
    q.payload_out = static_cast<uint8_t *>(io->d_payload_out);
    for (int k = 0; k < AGX_MB_STREAMS; ++k) {
        q.src[k] = k < io->n_f32 ? io->src_f32[k] : nullptr;
        q.dst[k] = k < io->n_f32 ? io->dst_f32[k] : nullptr;
    }
    q.valid = io->d_valid;
    q.N = N;
    q.L = L;
    q.which = which;
    q.permute = permute;
    q.first = first;
    q.S = S_;
    q.W = io->payload_bytes > 0 ? io->payload_bytes : 0;
    q.n_f32 = io->n_f32;
    hipLaunchKernelGGL(agx::k_mb_take, dim3((uint32_t)(((int64_t)S_ + kThreads - 1) / kThreads)), dim3(kThreads), 0, S(stream), q);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_minibatch_scatter(agx_minibatch *mb, int32_t S_, const int32_t *d_slot, const uint8_t *d_valid, const float *d_src, int32_t L, float *d_dst,
                          void *stream) {
    const char *who = "agx_minibatch_scatter";
    if (!mb) return fail(nullptr, AGX_E_INVALID, "%s: null argument (mb)", who);
    agx_ctx *ctx = mb->h->ctx;
    const int32_t N = mb->h->p.N;
    if (int rc = rollout_bad_L(ctx, who, L, N)) return rc;
    if (S_ < 0) return fail(ctx, AGX_E_INVALID, "%s: S = %d", who, S_);
    if (!d_slot || !d_valid || !d_src || !d_dst)
        return fail(ctx, AGX_E_INVALID, "%s: null buffer (%s)", who, !d_slot ? "d_slot" : !d_valid ? "d_valid" : !d_src ? "d_src" : "d_dst");
    if (!full_range(ctx)) return hist_refuse_range(mb->h, who);
    if (S_ == 0) return AGX_OK;
    DeviceGuard g(mb->own.device);
    hipLaunchKernelGGL(agx::k_mb_scatter, dim3((uint32_t)(((int64_t)S_ + kThreads - 1) / kThreads)), dim3(kThreads), 0, S(stream), S_, d_slot, d_valid, d_src,
                       L * N, d_dst);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

}  // extern "C"
