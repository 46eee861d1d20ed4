// agx_k7_replay.h - K7: the replay sampler on the frame history (include/agx_replay.h).  k_replay_scan turns the per-env append
// counts into candidate offsets and advances the call counter, k_replay_draw draws B accepted (env, index) pairs by rejection,
// k_replay_inspect reports age / ahead of samples the caller drew itself.  The arithmetic of the draw is agx_replay_draw.h's.
// Every device write is an ordinary vector store.
#pragma once
#include "agx_k5_history.h"
#include "agx_replay_draw.h"

namespace agx {

struct ReplayParams {
    HistParams h;
    int64_t *off;          // i64 [N + 1]  exclusive prefix sum of the per-env candidate counts
    uint64_t *state;       // u64 [3]      seed, calls, the key of the call in flight
    int32_t back, forward, attempts;
};

__global__ void k_replay_seed(uint64_t *state, uint64_t seed) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        state[0] = seed;
        state[1] = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// k_replay_scan: one workgroup of 256.  It walks the envs in chunks of 256 with a carried i64 total: the wave64 __shfl_up scan
// and the one LDS step across the four waves of flex_state_scan_block (agx_k4_raw3.h).  Thread 0 closes off[N], publishes
// key = SM(seed, calls) and advances calls: the only launch of a call that writes the state, so a replayed graph draws anew.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_replay_scan(ReplayParams p, int64_t *total_out) {
    __shared__ int64_t wave_tot[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.h.N;
    int64_t carry = 0;
    for (int base = 0; base < N; base += kThreads) {
        const int n = base + tid;
        const int64_t mine = n < N ? replay_len(p.h.count[n], p.h.T, p.forward) : 0;
        int64_t incl = mine;                                        // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int64_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            const int64_t t = wave_tot[w];
            if (w < wave) before += t;
            all += t;
        }
        if (n < N) p.off[n] = carry + before + incl - mine;
        carry += all;
        __syncthreads();                                            // wave_tot is rewritten by the next chunk
    }
    if (tid == 0) {
        p.off[N] = carry;
        if (total_out) *total_out = carry;
        const uint64_t calls = p.state[1];
        p.state[2] = replay_sm(p.state[0], calls);
        p.state[1] = calls + 1;
    }
}

// the age byte of a retained row
__device__ __forceinline__ int replay_age(const HistParams &h, int n, int64_t k) {
    return (int)h.age[(size_t)hist_row(k, h.T) * h.N + n];
}

// ---------------------------------------------------------------------------------------------
// k_replay_draw: grid = ceil(B / 256), one sample per thread.  Per attempt: the candidate (binary search over off, L2-resident),
// then the predicate of include/agx_replay.h from the byte loads of age[k], age[k - b] and age[k + forward].  The loop ends when
// every lane of the wave has accepted or run out of attempts.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_replay_draw(ReplayParams p, int32_t B, int32_t *env_out, int64_t *index_out, uint8_t *ok_out) {
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int N = p.h.N, T = p.h.T, fs1 = p.h.fs - 1;
    const int64_t total = p.off[N];
    const uint64_t key = p.state[2];
    bool done = b >= B || total <= 0;
    int32_t res_n = -1;
    int64_t res_k = -1;
    for (int a = 0; a < p.attempts; ++a) {
        if (!done) {
            const ReplayCandidate c = replay_candidate(key, b, p.attempts, a, p.off, N, total);
            const int n = c.n;
            const int64_t cnt = p.h.count[n], lo = replay_lo(cnt, T), k = lo + c.at;    // lo <= k, k + forward < cnt
            const int age = replay_age(p.h, n, k);
            bool ok = k - min(age, fs1) >= lo;                                          // 1. (n, k) is valid
            const int64_t kb = k - min(p.back, age);
            ok = ok && kb >= lo;                                                        // 2. (n, k - b) is retained and valid
            if (ok && kb != k) ok = kb - min(replay_age(p.h, n, kb), fs1) >= lo;
            if (ok && p.forward > 0) ok = replay_age(p.h, n, k + p.forward) >= p.forward;   // 3. the same episode forward appends on
            if (ok) {
                res_n = n;
                res_k = k;
                done = true;
            }
        }
        if (__all(done)) break;
    }
    if (b < B) {
        env_out[b] = res_n;
        index_out[b] = res_k;
        if (ok_out) ok_out[b] = res_n >= 0 ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------
// k_replay_inspect: one sample per thread.  age[k] of a valid sample and the number of later appends of its episode that the
// history already holds (the largest f <= 255 with k + f < count and no age == 0 in (k, k + f]); -1 for an invalid sample.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_replay_inspect(HistParams h, const int32_t *env, const int64_t *index, int32_t B, int32_t *age_out,
                                                             int32_t *ahead_out) {
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    const int n = env[b];
    const int64_t k = index[b];
    int age = -1, ahead = -1;
    if (n >= 0 && n < h.N && k >= 0) {
        const int64_t cnt = h.count[n], lo = replay_lo(cnt, h.T);
        if (k < cnt && k >= lo) {
            const int a = replay_age(h, n, k);
            if (k - min(a, h.fs - 1) >= lo) {
                age = a;
                ahead = 0;
                while (ahead < 255 && k + ahead + 1 < cnt && replay_age(h, n, k + ahead + 1) != 0) ++ahead;
            }
        }
    }
    if (age_out) age_out[b] = age;
    if (ahead_out) ahead_out[b] = ahead;
}

}  // namespace agx
