// agx_k9_priority.h - K9: the prioritized sampler on the frame history (include/agx_priority.h).  k_priority_update / _lookup /
// _clear / _seed keep the table; a sample call is four launches in stream order: k_priority_weights turns every retained row
// into its weight W and a prefix inside its chunk of 64 rows, k_priority_chunks scans each env's chunk sums, k_priority_scan
// scans the envs, k_priority_draw searches env -> chunk -> row.  The arithmetic is agx_priority_math.h's.  Every device write is
// an ordinary vector store, but for the one vector atomicMax per wave on wmax; no workgroup waits for another inside a launch.
#pragma once
#include "agx_k5_history.h"
#include "agx_priority_math.h"

namespace agx {

constexpr int kPrioGroup = 16;                                   // adjacent envs a workgroup of k_priority_weights owns
constexpr int kPrioChunk = 64;                                   // rows (in index order) per chunk: one wave scan
constexpr int kPrioRow = 196;                                    // bytes per env of the age tile: 64 + back + forward <= 192 (a
                                                                 // row of 49 dwords: the 16 rows start on 16 different banks)
static_assert(kThreads / 64 * 4 == kPrioGroup, "four waves of four envs each");

// The table and the scratch are env-major: row k of env n sits at n * T + k mod T, its prefix at n * T + (k - lo_n).
struct PriorityParams {
    HistParams h;
    int64_t *stamp;        // i64 [N][T]   the index the weight was written for, -1: unset
    uint32_t *weight;      // u32 [N][T]
    uint32_t *wmax;        // u32 [1]
    int64_t *incl;         // i64 [N][T]   inclusive prefix of W inside the row's chunk, by position k - lo_n
    int64_t *csum;         // i64 [N][CH]  the chunks' sums (k_priority_weights), then their exclusive prefix (k_priority_chunks)
    int32_t *cacc;         // i32 [N][CH]  rows with W > 0 per chunk
    int64_t *envsum;       // i64 [N]
    int64_t *envacc;       // i64 [N]
    int64_t *off;          // i64 [N + 1]  exclusive prefix sum of envsum
    uint64_t *state;       // u64 [3]      seed, calls, the key of the call in flight
    int32_t back, forward;
    int32_t CH;            // chunks per env: ceil(T / 64)
};

__global__ void k_priority_seed(uint64_t *state, uint64_t seed) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        state[0] = seed;
        state[1] = 0;
    }
}

// grid = ceil(T * N / 256): every stamp -1, wmax as new
__global__ __launch_bounds__(kThreads) void k_priority_clear(int64_t *stamp, uint32_t *wmax, int64_t rows) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < rows) stamp[i] = -1;
    if (i == 0) *wmax = kPriorityOne;
}

// is (n, k) a retained row?  cnt is read only when n is an env
__device__ __forceinline__ bool priority_retained(const HistParams &h, int n, int64_t k, int64_t &cnt) {
    if (n < 0 || n >= h.N) return false;
    cnt = h.count[n];
    return k >= replay_lo(cnt, h.T) && k < cnt;
}

// ---------------------------------------------------------------------------------------------
// k_priority_update: grid = ceil(B / 256), one sample per thread.  The maximum of the weights written is reduced in the wave
// and lane 0 issues one atomicMax: a maximum does not depend on the order, so wmax is deterministic.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_priority_update(PriorityParams p, const int32_t *env, const int64_t *index, const float *priority,
                                                              int32_t B) {
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t m = 0;
    if (b < B) {
        const int n = env[b];
        const int64_t k = index[b];
        int64_t cnt = 0;
        if (priority_retained(p.h, n, k, cnt)) {
            const size_t row = (size_t)n * p.h.T + hist_row(k, p.h.T);
            m = priority_quantise(priority[b]);
            p.weight[row] = m;
            p.stamp[row] = k;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(p.wmax, m);
}

// k_priority_lookup: one sample per thread; the effective weight of a retained row, -1 otherwise
__global__ __launch_bounds__(kThreads) void k_priority_lookup(PriorityParams p, const int32_t *env, const int64_t *index, int32_t B, int64_t *out) {
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    const int n = env[b];
    const int64_t k = index[b];
    int64_t cnt = 0, w = -1;
    if (priority_retained(p.h, n, k, cnt)) {
        const size_t row = (size_t)n * p.h.T + hist_row(k, p.h.T);
        w = (int64_t)priority_effective(p.stamp[row], p.weight[row], k, *p.wmax);
    }
    out[b] = w;
}

// the row of position pos (0 <= pos < T) behind an env whose oldest retained index sits in row slot0: (slot0 + pos) mod T
__device__ __forceinline__ int priority_slot(int slot0, int64_t pos, int T) {
    const uint32_t s = (uint32_t)slot0 + (uint32_t)pos;             // below 2 T < 2^32
    return (int)(s >= (uint32_t)T ? s - (uint32_t)T : s);
}

// the ages of one env out of the workgroup's LDS tile: byte j - base of its row
struct PriorityTileAges {
    const uint8_t *row;
    int64_t base;
    __device__ __forceinline__ int32_t age(int64_t j) const { return (int32_t)row[j - base]; }
};

// ---------------------------------------------------------------------------------------------
// k_priority_weights: grid = ceil(N / 16) * CH, block = 256.  Workgroup (g, c) owns chunk c - positions 64 c .. 64 c + 63 in
// index order, position = k - lo_n - of the 16 adjacent envs 16 g .. 16 g + 15.
//   1. It stages the age bytes the predicate can ask for, positions 64 c - back .. 64 c + 63 + forward of each env, into LDS:
//      consecutive lanes take consecutive envs, so a wave's byte loads fall into 4 lines of the history's [T][N] age array (16
//      adjacent bytes each while the envs' counts agree) where a workgroup per env would touch 64 lines for 64 bytes.
//   2. Wave w takes envs 4 w .. 4 w + 3 in turn, a lane per row: stamp and weight come lane-linear out of the env-major table (two
//      segments where the ring wraps), W is priority_row_weight over the tile, the inclusive prefix of the chunk is one wave64
//      __shfl_up scan, written lane-linear; lane 63 writes the chunk's sum and its count of rows with W > 0.
// No carry, no wait on another workgroup: the chunk sums are scanned by the next launch.  Thread 0 of workgroup 0 publishes
// key = SM(seed, calls) and advances calls - the call's first launch, so a replayed graph draws anew.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_priority_weights(PriorityParams p) {
    __shared__ uint8_t tile[kPrioGroup][kPrioRow];
    __shared__ int64_t s_cnt[kPrioGroup];
    __shared__ int32_t s_slot[kPrioGroup];                          // the row of each env's oldest retained index
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.h.N, T = p.h.T, fs1 = p.h.fs - 1;
    const int g = (int)(blockIdx.x / (uint32_t)p.CH), c = (int)(blockIdx.x - (uint32_t)g * (uint32_t)p.CH);
    const int n0 = g * kPrioGroup;
    if (blockIdx.x == 0 && tid == 0) {
        const uint64_t calls = p.state[1];
        p.state[2] = replay_sm(p.state[0], calls);
        p.state[1] = calls + 1;
    }
    if (tid < kPrioGroup) {                                         // the one division per env: rows are slot[e] + position, mod T
        const int64_t cnt = n0 + tid < N ? p.h.count[n0 + tid] : 0;
        s_cnt[tid] = cnt;
        s_slot[tid] = hist_row(replay_lo(cnt, T), T);
    }
    __syncthreads();
    const int win = kPrioChunk + p.back + p.forward;
    const int64_t pos0 = (int64_t)c * kPrioChunk - p.back;          // the position behind byte 0 of a tile row
    for (int i = tid; i < kPrioGroup * win; i += kThreads) {
        const int e = i & (kPrioGroup - 1), r = i >> 4;
        const int64_t cnt = s_cnt[e], pos = pos0 + r;
        if (pos >= 0 && replay_lo(cnt, T) + pos < cnt) tile[e][r] = p.h.age[(size_t)priority_slot(s_slot[e], pos, T) * N + (n0 + e)];
    }
    __syncthreads();
    const uint32_t wmax = *p.wmax;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = wave * 4 + q, n = n0 + e;
        if (n >= N) break;                                          // (wave-uniform; nothing behind it synchronises)
        const int64_t cnt = s_cnt[e], lo = replay_lo(cnt, T);
        const int64_t pos = (int64_t)c * kPrioChunk + lane, k = lo + pos;
        const bool live = k < cnt;
        int64_t w = 0;
        if (live) {
            const size_t row = (size_t)n * T + priority_slot(s_slot[e], pos, T);
            const int64_t stamp = p.stamp[row];
            const uint32_t weight = p.weight[row];
            w = priority_row_weight(PriorityTileAges{tile[e], lo + pos0}, k, cnt, lo, fs1, p.back, p.forward, stamp, weight, wmax);
        }
        int64_t incl = w;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        const unsigned long long drawable = __ballot(w > 0);
        if (live) p.incl[(size_t)n * T + pos] = incl;
        if (lane == 63) {
            p.csum[(size_t)n * p.CH + c] = incl;
            p.cacc[(size_t)n * p.CH + c] = __popcll(drawable);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_priority_chunks: grid = ceil(N / 4), block = 256, a wave per env.  The env's chunk sums become their exclusive prefix, in
// place, 64 chunks per turn with a carried i64; lane 0 writes the env's sum and its count of rows with W > 0.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_priority_chunks(PriorityParams p) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (n >= p.h.N) return;                                         // (wave-uniform)
    int64_t *cs = p.csum + (size_t)n * p.CH;
    const int32_t *ca = p.cacc + (size_t)n * p.CH;
    int64_t carry = 0;
    int32_t acc = 0;
    for (int base = 0; base < p.CH; base += 64) {
        const int c = base + lane;
        const int64_t mine = c < p.CH ? cs[c] : 0;
        if (c < p.CH) acc += ca[c];
        int64_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (c < p.CH) cs[c] = carry + incl - mine;
        carry += __shfl(incl, 63, 64);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane == 0) {
        p.envsum[n] = carry;
        p.envacc[n] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// k_priority_scan: one workgroup of 256, k_replay_scan's shape over the per-env sums: off, total, and the number of rows with
// W > 0 (a plain sum: every thread adds its envs', the workgroup adds those through LDS).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_priority_scan(PriorityParams p, int64_t *total_out, int64_t *accepted_out) {
    __shared__ int64_t wave_tot[kThreads / 64];
    __shared__ int64_t wave_acc[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.h.N;
    int64_t carry = 0, acc = 0;
    for (int base = 0; base < N; base += kThreads) {
        const int n = base + tid;
        const int64_t mine = n < N ? p.envsum[n] : 0;
        if (n < N) acc += p.envacc[n];
        int64_t incl = mine;
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
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane == 0) wave_acc[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        p.off[N] = carry;
        if (total_out) *total_out = carry;
        if (accepted_out) {
            int64_t a = 0;
#pragma unroll
            for (int w = 0; w < kThreads / 64; ++w) a += wave_acc[w];
            *accepted_out = a;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_priority_draw: grid = ceil(B / 256), one sample per thread, one attempt: the env (binary search over off), the chunk (over
// the env's chunk prefix), the row (over the chunk's inclusive prefix: at most 64 entries of one 512-byte run).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_priority_draw(PriorityParams p, int32_t B, int32_t *env_out, int64_t *index_out, uint8_t *ok_out,
                                                            int64_t *weight_out) {
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    const int N = p.h.N, T = p.h.T;
    const int64_t total = p.off[N];
    int32_t res_n = -1;
    int64_t res_k = -1, res_w = 0;
    if (total > 0) {
        const int64_t u = replay_pick(replay_sm(p.state[2], (uint64_t)b), total);
        const int n = replay_find_env(p.off, N, u);
        int64_t v = u - p.off[n];
        const int64_t cnt = p.h.count[n], lo = replay_lo(cnt, T);
        const int32_t len = (int32_t)(cnt - lo);                                   // 1 .. T: the env has weight
        const int64_t *cs = p.csum + (size_t)n * p.CH;
        const int32_t c = replay_find_env(cs, (len + kPrioChunk - 1) / kPrioChunk, v);
        v -= cs[c];
        const int64_t *in = p.incl + (size_t)n * T + (size_t)c * kPrioChunk;
        const int32_t at = priority_find_row(in, min(kPrioChunk, len - c * kPrioChunk), v);
        res_n = n;
        res_k = lo + (int64_t)c * kPrioChunk + at;
        res_w = in[at] - (at > 0 ? in[at - 1] : 0);
    }
    env_out[b] = res_n;
    index_out[b] = res_k;
    if (ok_out) ok_out[b] = res_n >= 0 ? 1 : 0;
    if (weight_out) weight_out[b] = res_w;
}

}  // namespace agx
