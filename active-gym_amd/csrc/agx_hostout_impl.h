// agx_hostout_impl.h - include/agx_hostout.h: agx_env_range and the chunked host-output step of the native loop (included at
// the end of agx_api.hip, behind agx_loop_impl.h: it is built on that loop's staging, its copy stream and its autoreset tail).
//
// Streams of one agx_loop_step_host:
//   copy stream (the loop's)   cmd | screens of chunk 0 | screens of chunk 1 | ...          (+ the tail's reset screens)
//   launch stream (caller's)        wait 0: ingest, observe [range 0] | wait 1: ingest, observe [range 1] | ... | tail
//   d2h stream (the ONE new one)         wait 0: obs, fov rows of chunk 0 | wait 1: ... | terminal rows, re-observed rows
// so chunk c's observations leave the device while chunk c + 1's screens arrive and its kernels run.
#pragma once
#include "agx_hostout.h"

struct agx_hostout {
    explicit agx_hostout(int device) : own(device) {}
    Resources own;                                    // owns the stream, events and pinned side sets below
    hipStream_t d2h = nullptr;
    hipEvent_t ev_h2d[AGX_HOSTOUT_MAX_CHUNKS] = {};   // copy stream: chunk c's screens are on the device
    hipEvent_t ev_k[AGX_HOSTOUT_MAX_CHUNKS] = {};     // launch stream: chunk c's rows are written
    hipEvent_t ev_chunks = nullptr;                   // d2h stream: every chunk copy has read its rows of d_obs
    hipEvent_t ev_tail = nullptr;                     // launch stream: the autoreset tail has run
    hipEvent_t ev_done[2] = {nullptr, nullptr};       // d2h stream: the step that used side set s has landed on the host
    // terminal rows of the envs that ended an episode, two pinned sets used alternately (valid until the step after next)
    void *h_final_obs[2] = {nullptr, nullptr};
    int32_t *h_final_loc[2] = {nullptr, nullptr}, *h_final_res[2] = {nullptr, nullptr};
    int set = 0;
    bool stepped = false;
    bool has_final = false;                           // the last step filled side set `set`
};

static void hostout_free(agx_hostout *h) { delete h; }

namespace {

// agx_loop_host_prepare (or the first agx_loop_step_host of a loop that was not prepared): its stream, events and pinned side
// buffers; no allocation in later steps
int hostout_alloc(agx_loop *l, agx_hostout *h) {
    const size_t N = (size_t)l->N;
    LOOP_HIP(l, h->own.stream(&h->d2h, hipStreamNonBlocking));
    LOOP_HIP(l, h->own.event(&h->ev_chunks, hipEventDisableTiming));
    LOOP_HIP(l, h->own.event(&h->ev_tail, hipEventDisableTiming));
    for (int b = 0; b < 2; ++b) {
        LOOP_HIP(l, h->own.event(&h->ev_done[b], hipEventDisableTiming));
        LOOP_HIP(l, h->own.pinned(&h->h_final_obs[b], N * l->obs_row_bytes));
        if (l->fovea) {
            LOOP_HIP(l, h->own.pinned(&h->h_final_loc[b], N * 2 * sizeof(int32_t)));
            LOOP_HIP(l, h->own.pinned(&h->h_final_res[b], N * 2 * sizeof(int32_t)));
        }
    }
    return AGX_OK;
}
int hostout_make(agx_loop *l, int nchunks) {
    if (!l->ho) {
        agx_hostout *h = new (std::nothrow) agx_hostout(l->own.device);
        if (!h) return lfail(l, AGX_E_NOMEM, "out of host memory");
        const int rc = hostout_alloc(l, h);
        if (rc != AGX_OK) {                       // all or nothing: a later call starts over
            hostout_free(h);
            return rc;
        }
        l->ho = h;
    }
    for (int c = 0; c < nchunks; ++c) {
        if (!l->ho->ev_h2d[c]) LOOP_HIP(l, l->ho->own.event(&l->ho->ev_h2d[c], hipEventDisableTiming));
        if (!l->ho->ev_k[c]) LOOP_HIP(l, l->ho->own.event(&l->ho->ev_k[c], hipEventDisableTiming));
    }
    return AGX_OK;
}

// whatever way a chunked step leaves, the context is back on the whole batch
struct RangeRestore {
    agx_ctx *ctx;
    ~RangeRestore() {
        ctx->rng_lo = 0;
        ctx->rng_n = ctx->cfg.num_envs;
    }
};

}  // namespace

extern "C" {

int agx_env_range(agx_ctx *ctx, int32_t lo, int32_t n) {
    if (!ctx) return AGX_E_INVALID;
    const int N = ctx->cfg.num_envs;
    if (lo < 0 || n < 1 || (int64_t)lo + n > N)
        return fail(ctx, AGX_E_INVALID, "agx_env_range: [%d, %d + %d) is not a non-empty range inside [0, %d)", lo, lo, n, N);
    if (ctx->planes != 1 && !(lo == 0 && n == N))
        return fail(ctx, AGX_E_STATE, "agx_env_range: an AGX_FRAME_RGB context acts on the whole batch only");
    ctx->rng_lo = lo;
    ctx->rng_n = n;
    return AGX_OK;
}

int agx_hostout_partition(int32_t num_envs, int32_t chunks, int32_t *lo, int32_t *n) {
    if (!lo || !n || num_envs < 1 || chunks < 1) return AGX_E_INVALID;
    const int c = std::min(std::min(chunks, num_envs), (int32_t)AGX_HOSTOUT_MAX_CHUNKS);
    const int base = num_envs / c, extra = num_envs % c;
    int at = 0;
    for (int k = 0; k < c; ++k) {
        lo[k] = at;
        n[k] = base + (k < extra ? 1 : 0);
        at += n[k];
    }
    return c;
}

int agx_loop_host_prepare(agx_loop *l, int chunks) {
    if (!l) return AGX_E_INVALID;
    if (chunks < 1) return lfail(l, AGX_E_INVALID, "agx_loop_host_prepare: chunks must be >= 1 (got %d)", chunks);
    DeviceGuard g(l->ctx->cfg.device);
    return hostout_make(l, std::min(std::min(chunks, l->N), (int)AGX_HOSTOUT_MAX_CHUNKS));
}

int agx_loop_step_host(agx_loop *l, const int32_t *motor, const void *d_action, int action_dtype, const int32_t *d_action_type,
                       float *d_obs, int32_t *d_fov_loc, int32_t *d_fov_res, agx_loop_result *res, void *stream, void *h_obs,
                       int32_t *h_fov_loc, int32_t *h_fov_res, int chunks) {
    if (!l) return AGX_E_INVALID;
    if (!motor || !d_obs || !res || !h_obs) return lfail(l, AGX_E_INVALID, "agx_loop_step_host: null argument");
    if (l->fovea && (!d_fov_loc || !h_fov_loc))
        return lfail(l, AGX_E_INVALID, "agx_loop_step_host: a fovea context needs d_fov_loc and h_fov_loc");
    if (l->flexible && (!d_fov_res || !h_fov_res))
        return lfail(l, AGX_E_INVALID, "agx_loop_step_host: a flexible context needs d_fov_res and h_fov_res");
    if (chunks < 1) return lfail(l, AGX_E_INVALID, "agx_loop_step_host: chunks must be >= 1 (got %d)", chunks);
    DeviceGuard g(l->ctx->cfg.device);
    hipStream_t st = S(stream);
    const int N = l->N;
    int32_t lo[AGX_HOSTOUT_MAX_CHUNKS], cn[AGX_HOSTOUT_MAX_CHUNKS];
    const int nc = agx_hostout_partition(N, chunks, lo, cn);
    int rc = hostout_make(l, nc);
    if (rc != AGX_OK) return rc;
    agx_hostout *h = l->ho;
    const size_t env_bytes = 2 * l->screen_bytes, row = l->obs_row_bytes, fov_row = 2 * sizeof(int32_t);
    char *hob = static_cast<char *>(h_obs);
    const char *dob = reinterpret_cast<const char *>(d_obs);
    int64_t h2d = 0;
    // the other side set: what it held was handed out two steps ago; and this step's kernels write d_obs only after the previous
    // step's copies have read it
    h->set ^= 1;
    const int hs = h->set;
    LOOP_HIP(l, hipEventSynchronize(h->ev_done[hs]));
    if (h->stepped) LOOP_HIP(l, hipStreamWaitEvent(st, h->ev_done[hs ^ 1], 0));
    h->has_final = false;
    // ---- 1. emulators, as agx_loop_step: the other pinned set, the other device set
    l->stage_i ^= 1;
    l->dset_i ^= 1;
    const int sg = l->stage_i, ds = l->dset_i;
    LOOP_HIP(l, hipEventSynchronize(l->ev_copy[sg]));
    if (l->src.step(l->src.self, motor, l->h_frames[sg], l->h_cmd[sg], l->reward.data(), l->raw.data(), l->done.data()) != 0)
        return lfail(l, AGX_E_STATE, "host source: step failed");
    // ---- 2. per chunk.  All the H2D copies first, back to back on the copy stream, one event each ...
    LOOP_HIP(l, hipStreamWaitEvent(l->copy_stream, l->ev_free[ds], 0));
    LOOP_HIP(l, hipMemcpyAsync(l->d_cmd[ds], l->h_cmd[sg], (size_t)N, hipMemcpyHostToDevice, l->copy_stream));
    for (int c = 0; c < nc; ++c) {
        const size_t off = (size_t)lo[c] * env_bytes;
        LOOP_HIP(l, hipMemcpyAsync(l->d_frames[ds] + off, l->h_frames[sg] + off, (size_t)cn[c] * env_bytes, hipMemcpyHostToDevice,
                                   l->copy_stream));
        LOOP_HIP(l, hipEventRecord(h->ev_h2d[c], l->copy_stream));
    }
    LOOP_HIP(l, hipEventRecord(l->ev_copy[sg], l->copy_stream));
    h2d += (int64_t)N + (int64_t)N * (int64_t)env_bytes;
    // ... then, per chunk, its kernels over its env range on the launch stream and its rows home on the d2h stream
    {
        RangeRestore back{l->ctx};
        for (int c = 0; c < nc; ++c) {
            LOOP_HIP(l, hipStreamWaitEvent(st, h->ev_h2d[c], 0));
            LOOP_AGX(l, agx_env_range(l->ctx, lo[c], cn[c]));
            LOOP_AGX(l, loop_ingest(l, l->d_frames[ds], l->d_cmd[ds], st));
            LOOP_AGX(l, loop_observe(l, l->fovea ? d_action : nullptr, action_dtype, d_action_type, nullptr, d_obs, d_fov_loc, d_fov_res, st));
            LOOP_HIP(l, hipEventRecord(h->ev_k[c], st));
            LOOP_HIP(l, hipStreamWaitEvent(h->d2h, h->ev_k[c], 0));
            LOOP_HIP(l, hipMemcpyAsync(hob + (size_t)lo[c] * row, dob + (size_t)lo[c] * row, (size_t)cn[c] * row, hipMemcpyDeviceToHost, h->d2h));
            if (l->fovea)
                LOOP_HIP(l, hipMemcpyAsync(h_fov_loc + 2 * (size_t)lo[c], d_fov_loc + 2 * (size_t)lo[c], (size_t)cn[c] * fov_row,
                                           hipMemcpyDeviceToHost, h->d2h));
            if (l->flexible)
                LOOP_HIP(l, hipMemcpyAsync(h_fov_res + 2 * (size_t)lo[c], d_fov_res + 2 * (size_t)lo[c], (size_t)cn[c] * fov_row,
                                           hipMemcpyDeviceToHost, h->d2h));
        }
    }   // ---- 3. the whole batch again
    if (l->hist) LOOP_AGX(l, agx_history_push(l->hist, l->d_cmd[ds], nullptr, st));      // (include/agx_history.h: whole-batch, behind the last chunk)
    l->done_idx.clear();
    for (int i = 0; i < N; ++i)
        if (l->done[i]) l->done_idx.push_back(i);
    const int k = (int)l->done_idx.size();
    res->reward = l->reward.data();
    res->raw = l->raw.data();
    res->done = l->done.data();
    res->n_done = k;
    res->done_idx = l->done_idx.data();
    res->d_final_obs = nullptr;
    res->d_final_loc = res->d_final_res = nullptr;
    if (k > 0 && l->cfg.autoreset) {
        if (l->src.draw_noops) {
            if (l->src.draw_noops(l->src.noops_user, l->done_idx.data(), k, l->noops.data()) != 0)
                return lfail(l, AGX_E_STATE, "host source: draw_noops failed");
        } else {
            std::fill(l->noops.begin(), l->noops.begin() + k, 0);
        }
        // the tail rewrites the done envs' rows of d_obs / d_fov_*: behind the chunk copies that read them (their terminal values
        // reach h_obs first and are replaced below; final_observation comes from the side buffers)
        LOOP_HIP(l, hipEventRecord(h->ev_chunks, h->d2h));
        LOOP_HIP(l, hipStreamWaitEvent(st, h->ev_chunks, 0));
        rc = loop_reset_subset(l, k, d_obs, d_fov_loc, d_fov_res, st, &h2d, true);
        res->d_final_obs = l->d_final_obs;
        if (l->fovea) res->d_final_loc = l->d_final_loc;
        if (l->flexible) res->d_final_res = l->d_final_res;
        if (rc != AGX_OK) return rc;
        // ---- 4. the k terminal rows to the side set, the k re-observed rows to their rows of h_obs (runs of consecutive envs as
        // one copy each): k rows, never the whole batch again
        LOOP_HIP(l, hipEventRecord(h->ev_tail, st));
        LOOP_HIP(l, hipStreamWaitEvent(h->d2h, h->ev_tail, 0));
        LOOP_HIP(l, hipMemcpyAsync(h->h_final_obs[hs], l->d_final_obs, (size_t)k * row, hipMemcpyDeviceToHost, h->d2h));
        if (l->fovea) LOOP_HIP(l, hipMemcpyAsync(h->h_final_loc[hs], l->d_final_loc, (size_t)k * fov_row, hipMemcpyDeviceToHost, h->d2h));
        if (l->flexible) LOOP_HIP(l, hipMemcpyAsync(h->h_final_res[hs], l->d_final_res, (size_t)k * fov_row, hipMemcpyDeviceToHost, h->d2h));
        for (int j = 0; j < k;) {
            int e = j + 1;
            while (e < k && l->done_idx[e] == l->done_idx[e - 1] + 1) ++e;
            const size_t i0 = (size_t)l->done_idx[j], len = (size_t)(e - j);
            LOOP_HIP(l, hipMemcpyAsync(hob + i0 * row, dob + i0 * row, len * row, hipMemcpyDeviceToHost, h->d2h));
            if (l->fovea)
                LOOP_HIP(l, hipMemcpyAsync(h_fov_loc + 2 * i0, d_fov_loc + 2 * i0, len * fov_row, hipMemcpyDeviceToHost, h->d2h));
            if (l->flexible)
                LOOP_HIP(l, hipMemcpyAsync(h_fov_res + 2 * i0, d_fov_res + 2 * i0, len * fov_row, hipMemcpyDeviceToHost, h->d2h));
            j = e;
        }
        h->has_final = true;
    }
    LOOP_HIP(l, hipEventRecord(l->ev_free[ds], st));
    LOOP_HIP(l, hipEventRecord(h->ev_done[hs], h->d2h));
    h->stepped = true;
    res->h2d_bytes = h2d;
    return AGX_OK;
}

int agx_loop_host_wait(agx_loop *l) {
    if (!l) return AGX_E_INVALID;
    if (!l->ho || !l->ho->stepped) return AGX_OK;
    DeviceGuard g(l->ctx->cfg.device);
    LOOP_HIP(l, hipEventSynchronize(l->ho->ev_done[l->ho->set]));
    return AGX_OK;
}

int agx_loop_host_final(agx_loop *l, const void **h_final_obs, const int32_t **h_final_loc, const int32_t **h_final_res) {
    if (!l) return AGX_E_INVALID;
    const agx_hostout *h = l->ho;
    const bool has = h && h->has_final;
    if (h_final_obs) *h_final_obs = has ? h->h_final_obs[h->set] : nullptr;
    if (h_final_loc) *h_final_loc = has && l->fovea ? h->h_final_loc[h->set] : nullptr;
    if (h_final_res) *h_final_res = has && l->flexible ? h->h_final_res[h->set] : nullptr;
    return AGX_OK;
}

}  // extern "C"
