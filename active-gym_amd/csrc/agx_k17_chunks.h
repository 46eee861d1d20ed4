// agx_k17_chunks.h - K17: device-side minibatches of chunks on a gathered rollout (include/agx_chunks.h).  k_chunk_scan turns the
// per-env chunk counts into the list's offsets, records (total, L, C) and publishes the epoch's key; k_chunk_take writes the rows of
// S list positions, time-major.  The rule, the chunk at a list position and the bytes of a step are agx_chunk_math.h's, the
// permutation is agx_minibatch_math.h's: nothing is restated here.  Every device write is an ordinary vector store.
#pragma once
#include "agx_common.h"
#include "agx_chunk_math.h"

namespace agx {

constexpr int kChunkRows = 64;                   // k_chunk_take: the rows (chunks) of one workgroup, one per lane
constexpr int kChunkWaves = kThreads / 64;       // ... and the waves that share the steps of those rows

// ---------------------------------------------------------------------------------------------
// k_chunk_scan: one workgroup of 256, k_mb_scan's shape.  It walks the envs in runs of 256 with a carried i32 total (at most
// N * G <= L * N <= INT32_MAX): a wave64 __shfl_up scan and one LDS step across the four waves.  The counts are chunk_count(len).
// Thread 0 closes off[N], writes total, records (total, L, C), publishes key = SM(base, calls) and advances calls: the only
// launch that writes the state, so a replayed graph shuffles anew.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_chunk_scan(const int32_t *len, int32_t N, int32_t L, int32_t C, int32_t *off, uint64_t *state,
                                                         int32_t *seen, int32_t *total_out) {
    __shared__ int32_t wave_tot[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t carry = 0;
    for (int base = 0; base < N; base += kThreads) {
        const int n = base + tid;
        const int32_t mine = n < N ? chunk_count(len[n], L, C) : 0;
        int32_t incl = mine;                                        // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            const int32_t t = wave_tot[w];
            if (w < wave) before += t;
            all += t;
        }
        if (n < N) off[n] = carry + before + incl - mine;
        carry += all;
        __syncthreads();                                            // wave_tot is rewritten by the next run
    }
    if (tid == 0) {
        off[N] = carry;
        if (total_out) *total_out = carry;
        seen[0] = carry;
        seen[1] = L;
        seen[2] = C;
        const uint64_t calls = state[1];
        state[2] = replay_sm(state[0], calls);
        state[1] = calls + 1;
    }
}

struct ChunkTake {
    const int32_t *off;                  // i32 [N + 1]
    const uint64_t *state;               // u64 [3]: [2] is the key in flight
    const int32_t *seen;                 // i32 [3]: total, L, C of the last select
    const int32_t *len;                  // [N]
    const uint8_t *ends;                 // [L][N]
    const int64_t *obs_index, *next_index;   // [L][N] or nullptr
    const uint8_t *payload;              // [L][N][W] or nullptr
    const float *src[kChunkStreams];     // [L][N]
    int32_t *slot, *env;                 // [C][S]; every output but slot may be nullptr
    int64_t *obs_index_out, *next_index_out;
    uint8_t *payload_out;                // [C][S][W]
    float *dst[kChunkStreams];           // [C][S]
    uint8_t *ends_out, *start, *mask;    // [C][S]
    int32_t *chunk, *first_out, *steps;  // [S]
    int64_t *state_index;
    uint8_t *valid;
    int32_t N, L, C, permute, first, S, W, n_f32;
};

// ---------------------------------------------------------------------------------------------
// k_chunk_take: grid = ceil(S / 64), block = 256: 64 rows (chunks), one per lane, and four waves that share the steps of those rows.
// Wave 0 resolves each row's chunk ONCE - the permutation (integer work on the thread's own registers), the binary search over off
// (L2-resident: 4 KB at N = 1024), t0, first and steps -, writes the per-chunk outputs and leaves the chunk in LDS; behind one
// barrier wave w walks the steps l = w, w + 4, ... of the same 64 rows, once per output array: the step bytes (slot, env, ends,
// start, mask) in one walk, then each index, each f32 stream and the payload in a walk of its own.  A walk holds two or three
// pointers, where one walk over everything holds thirty and spills scalar registers; whether a step is live is two compares on
// the chunk's registers; and the loads of a walk are independent of each other and of its stores (__restrict__), so four of them
// are in flight per thread.  The kernel is a chain of L2 latencies, not of bytes: one thread per row walking all C steps read
// 37 us per take at S = 256, C = 16.  The lanes of a wave are consecutive rows s, and step l of row s is
// element l * S + s, so every per-step store of a wave is one run of consecutive elements.  The gathers from the [L][N] arrays are
// element-granular by nature: a row's steps are N elements apart and the rows of a wave are unrelated envs; the arrays are a few
// hundred KB and sit in L2.  The number of f32 streams is a run-time bound on an unrolled loop of kChunkStreams, so the pointers
// stay kernel arguments and are never indexed through memory.
// ---------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void chunk_walk(const ChunkAt &c, const T *__restrict__ src, T *__restrict__ dst, T none, int32_t N, int32_t L, int32_t C,
                                           int32_t S, int64_t s, int32_t l0) {
#pragma unroll 4
    for (int32_t l = l0; l < C; l += kChunkWaves) {
        const bool have = src && chunk_live(c, L, C, l);              // (not found: never live)
        dst[(size_t)l * S + (size_t)s] = have ? src[(size_t)(c.g * C + l) * N + c.n] : none;      // C * S <= INT32_MAX
    }
}

__global__ __launch_bounds__(kThreads) void k_chunk_take(ChunkTake q) {
    __shared__ ChunkAt row_chunk[kChunkRows];
    __shared__ uint8_t row_valid[kChunkRows];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t s = (int64_t)blockIdx.x * kChunkRows + lane;
    if (wave == 0 && s < q.S) {
        const int32_t total = q.seen[0];
        const int32_t p = q.first + (int32_t)s;                      // first + S <= INT32_MAX
        ChunkAt c{0, -1, q.L, 0, 0, false};
        if (total > 0 && q.seen[1] == q.L && q.seen[2] == q.C)
            c = chunk_at(q.off, q.len, q.N, q.L, q.C, mb_position(q.state[2], total, p, q.permute != 0));
        const bool valid = c.found && p < total;
        if (q.chunk) q.chunk[s] = c.g;
        if (q.first_out) q.first_out[s] = c.first;
        if (q.steps) q.steps[s] = c.steps;
        if (q.state_index) q.state_index[s] = c.found && q.obs_index ? q.obs_index[(size_t)(c.g * q.C + c.first) * q.N + c.n] : -1;
        if (q.valid) q.valid[s] = valid ? 1 : 0;
        row_chunk[lane] = c;
        row_valid[lane] = valid ? 1 : 0;
    }
    __syncthreads();
    if (s >= q.S) return;
    const ChunkAt c = row_chunk[lane];
    const bool valid = row_valid[lane] != 0;
    for (int32_t l = wave; l < q.C; l += kChunkWaves) {              // the step bytes
        const size_t i = (size_t)l * q.S + (size_t)s;
        const ChunkStep st = chunk_step(c, q.ends, q.N, q.L, q.C, l, valid);
        q.slot[i] = st.live ? st.t * q.N + c.n : -1;
        if (q.env) q.env[i] = c.n;
        if (q.ends_out) q.ends_out[i] = st.ends;
        if (q.start) q.start[i] = st.start;
        if (q.mask) q.mask[i] = st.mask;
    }
    if (q.obs_index_out) chunk_walk<int64_t>(c, q.obs_index, q.obs_index_out, -1, q.N, q.L, q.C, q.S, s, wave);
    if (q.next_index_out) chunk_walk<int64_t>(c, q.next_index, q.next_index_out, -1, q.N, q.L, q.C, q.S, s, wave);
#pragma unroll
    for (int k = 0; k < kChunkStreams; ++k)
        if (k < q.n_f32 && q.dst[k]) chunk_walk<float>(c, q.src[k], q.dst[k], 0.0f, q.N, q.L, q.C, q.S, s, wave);
    if (q.payload_out && q.W > 0) {
        const bool words = ((q.W | (int32_t)(uintptr_t)q.payload | (int32_t)(uintptr_t)q.payload_out) & 3) == 0;   // a step log's payload: whole words
        for (int32_t l = wave; l < q.C; l += kChunkWaves) {
            const size_t i = (size_t)l * q.S + (size_t)s;
            const bool have = q.payload && chunk_live(c, q.L, q.C, l);
            const size_t e = have ? (size_t)(c.g * q.C + l) * q.N + c.n : 0;                      // read only where live
            if (words) {
                const int nw = q.W >> 2;
                const uint32_t *src = reinterpret_cast<const uint32_t *>(q.payload) + e * nw;
                uint32_t *dst = reinterpret_cast<uint32_t *>(q.payload_out) + i * nw;
                for (int k = 0; k < nw; ++k) dst[k] = have ? src[k] : 0u;
            } else {
                const uint8_t *src = q.payload + e * q.W;
                uint8_t *dst = q.payload_out + i * q.W;
                for (int k = 0; k < q.W; ++k) dst[k] = have ? src[k] : (uint8_t)0;
            }
        }
    }
}

}  // namespace agx
