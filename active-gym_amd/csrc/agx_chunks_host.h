// agx_chunks_host.h - the chunker declared in include/agx_chunks.h (included at the end of agx_api.hip, behind the frame history;
// the L check is agx_rollout_impl.h's): the checks, the chunker's own scratch and the launches of agx_k17_chunks.h.
#pragma once
#include "agx_chunks.h"

static_assert(AGX_CHUNK_L_LIMIT == AGX_ROLLOUT_LIMIT, "the limit is that of a gathered rollout");
static_assert(AGX_CHUNK_LIMIT == agx::kChunkLimit && AGX_CHUNK_LIST == agx::kChunkList && AGX_CHUNK_STREAMS == agx::kChunkStreams,
              "agx_chunk_math.h's constants are the header's");
static_assert(AGX_CHUNK_LIST > agx::kMbBoot, "the chunker's list number lies behind the minibatcher's");
static_assert(AGX_CHUNK_START_CHUNK == agx::kChunkStartChunk && AGX_CHUNK_START_EPISODE == agx::kChunkStartEpisode, "the START bits");
static_assert(agx::kChunkBreakBits == (AGX_STEP_TERMINATED | AGX_STEP_TRUNCATED | AGX_ROLLOUT_CUT), "the bits that end an episode are the gather's");

struct agx_chunks {
    explicit agx_chunks(int device) : own(device) {}
    Resources own;                  // the one device block: off i32 [N + 1] | state u64 [3] | seen i32 [3] (on the history's device: destroy
                                    // needs no live history)
    agx_history *h = nullptr;
    int32_t *off = nullptr, *seen = nullptr;
    uint64_t *state = nullptr;
};

namespace {

// the checks select and take share behind the handle, in the header's order: L and L * N, then C
int chunks_bad_shape(agx_ctx *ctx, const char *who, int32_t L, int32_t C, int32_t N) {
    if (int rc = rollout_bad_L(ctx, who, L, N)) return rc;
    const int32_t most = L < AGX_CHUNK_LIMIT ? L : AGX_CHUNK_LIMIT;
    if (C < 1 || C > most) return fail(ctx, AGX_E_INVALID, "%s: C must be 1 .. min(L, %d) = %d, got %d", who, AGX_CHUNK_LIMIT, most, C);
    return AGX_OK;
}

}  // namespace

extern "C" {

int agx_chunks_create(agx_history *h, uint64_t seed, agx_chunks **out) {
    agx_ctx *ctx = h ? h->ctx : nullptr;          // (no history: the message goes to agx_last_error(NULL))
    if (out) *out = nullptr;
    if (!h || !out) return fail(ctx, AGX_E_INVALID, "agx_chunks_create: null argument");
    if (!full_range(ctx)) return hist_refuse_range(h, "agx_chunks_create");
    agx_chunks *c = new (std::nothrow) agx_chunks(ctx->cfg.device);
    if (!c) return fail(ctx, AGX_E_NOMEM, "out of host memory");
    c->h = h;
    const size_t N = (size_t)h->p.N;
    agx::BlockLayout lay;
    const size_t o_off = lay.add((N + 1) * sizeof(int32_t)), o_state = lay.add(3 * sizeof(uint64_t)), o_seen = lay.add(3 * sizeof(int32_t));
    const uint64_t state[3] = {agx::replay_sm(seed, (uint64_t)AGX_CHUNK_LIST), 0, 0};     // base, calls, the key in flight: none yet (total is 0)
    DeviceGuard g(c->own.device);
    uint8_t *block = nullptr;
    if (int rc = hist_block(ctx, "agx_chunks_create", c, lay.bytes(), &block, [&](uint8_t *b) {
            const hipError_t e = hipMemset(b, 0, lay.bytes());
            return e != hipSuccess ? e : hipMemcpy(b + o_state, state, sizeof state, hipMemcpyHostToDevice);
        }))
        return rc;
    c->off = lay.at<int32_t>(block, o_off);
    c->state = lay.at<uint64_t>(block, o_state);
    c->seen = lay.at<int32_t>(block, o_seen);
    *out = c;
    return AGX_OK;
}

int agx_chunks_destroy(agx_chunks *c) {
    if (!c) return AGX_OK;
    DeviceGuard g(c->own.device);
    delete c;
    return AGX_OK;
}

int agx_chunks_select(agx_chunks *c, int32_t L, int32_t C, const int32_t *d_len, int32_t *d_total, void *stream) {
    const char *who = "agx_chunks_select";
    if (!c) return fail(nullptr, AGX_E_INVALID, "%s: null argument (c)", who);
    agx_ctx *ctx = c->h->ctx;
    const int32_t N = c->h->p.N;
    if (int rc = chunks_bad_shape(ctx, who, L, C, N)) return rc;
    if (!d_len) return fail(ctx, AGX_E_INVALID, "%s: null buffer (d_len)", who);
    if (!full_range(ctx)) return hist_refuse_range(c->h, who);
    DeviceGuard g(c->own.device);
    hipLaunchKernelGGL(agx::k_chunk_scan, dim3(1), dim3(kThreads), 0, S(stream), d_len, N, L, C, c->off, c->state, c->seen, d_total);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_chunks_take(agx_chunks *c, int permute, int32_t L, int32_t C, const int32_t *d_len, const uint8_t *d_ends, int32_t first, int32_t S_,
                    const agx_chunks_io *io, void *stream) {
    const char *who = "agx_chunks_take";
    if (!c) return fail(nullptr, AGX_E_INVALID, "%s: null argument (c)", who);
    agx_ctx *ctx = c->h->ctx;
    const int32_t N = c->h->p.N;
    if (int rc = chunks_bad_shape(ctx, who, L, C, N)) return rc;
    if (S_ < 0 || first < 0 || (int64_t)first + S_ > INT32_MAX)
        return fail(ctx, AGX_E_INVALID, "%s: first = %d, S = %d (both >= 0, first + S <= %d)", who, first, S_, INT32_MAX);
    if ((int64_t)C * S_ > INT32_MAX) return fail(ctx, AGX_E_INVALID, "%s: C * S = %lld exceeds %d", who, (long long)C * S_, INT32_MAX);
    if (!io) return fail(ctx, AGX_E_INVALID, "%s: null argument (io)", who);
    if (io->n_f32 < 0 || io->n_f32 > AGX_CHUNK_STREAMS) return fail(ctx, AGX_E_INVALID, "%s: n_f32 must be 0 .. %d, got %d", who, AGX_CHUNK_STREAMS, io->n_f32);
    if (!d_len) return fail(ctx, AGX_E_INVALID, "%s: null buffer (d_len)", who);
    if (!d_ends || !io->d_slot) return fail(ctx, AGX_E_INVALID, "%s: null buffer (%s)", who, !d_ends ? "d_ends" : "d_slot");
    if (!full_range(ctx)) return hist_refuse_range(c->h, who);
    if (S_ == 0) return AGX_OK;
    DeviceGuard g(c->own.device);
    agx::ChunkTake q;
    q.off = c->off;
    q.state = c->state;
    q.seen = c->seen;
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
    for (int k = 0; k < AGX_CHUNK_STREAMS; ++k) {
        q.src[k] = k < io->n_f32 ? io->src_f32[k] : nullptr;
        q.dst[k] = k < io->n_f32 ? io->dst_f32[k] : nullptr;
    }
    q.ends_out = io->d_ends_out;
    q.start = io->d_start;
    q.mask = io->d_mask;
    q.chunk = io->d_chunk;
    q.first_out = io->d_first;
    q.steps = io->d_steps;
    q.state_index = io->d_state_index;
    q.valid = io->d_valid;
    q.N = N;
    q.L = L;
    q.C = C;
    q.permute = permute;
    q.first = first;
    q.S = S_;
    q.W = io->payload_bytes > 0 ? io->payload_bytes : 0;
    q.n_f32 = io->n_f32;
    hipLaunchKernelGGL(agx::k_chunk_take, dim3((uint32_t)(((int64_t)S_ + agx::kChunkRows - 1) / agx::kChunkRows)), dim3(kThreads), 0,
                       S(stream), q);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

}  // extern "C"
