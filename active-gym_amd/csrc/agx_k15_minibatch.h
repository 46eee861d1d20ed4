// agx_k15_minibatch.h - K15: device-side minibatches on a gathered rollout (include/agx_minibatch.h).  k_mb_count counts every
// env's BOOT slots, k_mb_scan turns the per-env counts into the list's offsets and publishes the epoch's key, k_mb_take writes the
// rows of S list positions, k_mb_scatter puts per-row values back at their slots.  The rule, the permutation and the slot at a
// list position are agx_minibatch_math.h's: nothing is restated here.  Every device write is an ordinary vector store.
#pragma once
#include "agx_common.h"
#include "agx_minibatch_math.h"

namespace agx {

constexpr int kMbCountThreads = 64;

// ---------------------------------------------------------------------------------------------
// k_mb_count (BOOT only): block = 64 = one wave, one env per thread, grid = ceil(N / 64) - the fold's shape.  The ends bytes are
// time-major, so every load of a step is coalesced across the envs of a wave.  Each thread walks the live range of its column.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMbCountThreads) void k_mb_count(const int32_t *len, const uint8_t *ends, int32_t N, int32_t L, int32_t *cnt) {
    const int n = blockIdx.x * kMbCountThreads + threadIdx.x;
    if (n >= N) return;
    cnt[n] = mb_count(kMbBoot, len, ends, N, L, n);
}

// ---------------------------------------------------------------------------------------------
// k_mb_scan: one workgroup of 256.  It walks the envs in chunks of 256 with a carried i32 total (at most L * N <= INT32_MAX):
// k_replay_scan's wave64 __shfl_up scan and its one LDS step across the four waves.  The counts are len' for LIVE (from len) and cnt
// as k_mb_count left it for BOOT.  Thread 0 closes off[N], writes total, publishes key = SM(base, calls) and
// advances calls: the only launch that writes the state, so a replayed graph shuffles anew.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_mb_scan(int which, const int32_t *counts, int32_t N, int32_t L, int32_t *off, uint64_t *state, int32_t *total_out) {
    __shared__ int32_t wave_tot[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t carry = 0;
    for (int base = 0; base < N; base += kThreads) {
        const int n = base + tid;
        const int32_t mine = n < N ? (which == kMbLive ? mb_len(counts[n], L) : counts[n]) : 0;
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
        __syncthreads();                                            // wave_tot is rewritten by the next chunk
    }
    if (tid == 0) {
        off[N] = carry;
        if (total_out) *total_out = carry;
        const uint64_t calls = state[1];
        state[2] = replay_sm(state[0], calls);
        state[1] = calls + 1;
    }
}

struct MbTake {
    const int32_t *off;                  // i32 [N + 1] of the list
    const uint64_t *state;               // u64 [3] of the list: [2] is the key in flight
    const int32_t *len;                  // [N]
    const uint8_t *ends;                 // [L][N]; read for BOOT only
    const int64_t *obs_index, *next_index;   // [L][N] or nullptr
    const uint8_t *payload;              // [L][N][W] or nullptr
    const float *src[kMbStreams];        // [L][N]
    int32_t *slot, *env;                 // [S]; env or nullptr
    int64_t *obs_index_out, *next_index_out;
    uint8_t *payload_out;                // [S][W]
    float *dst[kMbStreams];              // [S]
    uint8_t *valid;
    int32_t N, L, which, permute, first, S, W, n_f32;
};

// ---------------------------------------------------------------------------------------------
// k_mb_take: grid = ceil(S / 256), one position per thread.  The position goes through the permutation (integer work on the
// thread's own registers), a binary search over off (L2-resident: 4 KB at N = 1024) gives its env, the closed form (LIVE) or the
// column walk (BOOT) its slot.  The gathers from the [L][N] arrays are element-granular and uncoalesced by nature; the arrays are
// a few hundred KB and sit in L2.  The stores are coalesced.  The number of f32 streams is a run-time bound on an unrolled loop of
// kMbStreams, so the pointers stay kernel arguments and are never indexed through memory.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_mb_take(MbTake q) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= q.S) return;
    const int32_t total = q.off[q.N];
    const int32_t p = q.first + (int32_t)i;                          // first + S <= INT32_MAX
    int32_t e = -1, n = 0;
    if (total > 0) {
        const int32_t m = mb_position(q.state[2], total, p, q.permute != 0);
        e = mb_slot(q.which, q.off, q.len, q.ends, q.N, q.L, m, &n);
        if (e < 0) n = 0;
    }
    const bool found = e >= 0;
    q.slot[i] = e;
    if (q.env) q.env[i] = n;
    if (q.valid) q.valid[i] = found && p < total ? 1 : 0;
    if (q.obs_index_out) q.obs_index_out[i] = found && q.obs_index ? q.obs_index[e] : -1;
    if (q.next_index_out) q.next_index_out[i] = found && q.next_index ? q.next_index[e] : -1;
#pragma unroll
    for (int k = 0; k < kMbStreams; ++k)
        if (k < q.n_f32 && q.dst[k]) q.dst[k][i] = found && q.src[k] ? q.src[k][e] : 0.0f;
    if (q.payload_out && q.W > 0) {
        const bool have = found && q.payload;
        if (((q.W | (int32_t)(uintptr_t)q.payload | (int32_t)(uintptr_t)q.payload_out) & 3) == 0) {   // a step log's payload: whole words
            const int words = q.W >> 2;
            const uint32_t *src = reinterpret_cast<const uint32_t *>(q.payload) + (size_t)(have ? e : 0) * words;
            uint32_t *dst = reinterpret_cast<uint32_t *>(q.payload_out) + (size_t)i * words;
            for (int k = 0; k < words; ++k) dst[k] = have ? src[k] : 0u;
        } else {
            const uint8_t *src = q.payload + (size_t)(have ? e : 0) * q.W;
            uint8_t *dst = q.payload_out + (size_t)i * q.W;
            for (int k = 0; k < q.W; ++k) dst[k] = have ? src[k] : (uint8_t)0;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_mb_scatter: one row per thread.  dst[slot[i]] = src[i] where the row is valid and its slot lies in [0, cells).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_mb_scatter(int32_t S, const int32_t *slot, const uint8_t *valid, const float *src, int32_t cells,
                                                         float *dst) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= S) return;
    const int32_t e = slot[i];
    if (e < 0 || e >= cells || !valid[i]) return;
    dst[e] = src[i];
}

}  // namespace agx
