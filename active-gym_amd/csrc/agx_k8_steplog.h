// agx_k8_steplog.h - K8: the step log next to the frame history (include/agx_steplog.h).  k_steplog_record writes one row per
// env, k_steplog_gather walks up to nstep rows per sample and writes the learner's row.  The walk is agx_steplog_fold.h's.
// Every device write is an ordinary vector store.
#pragma once
#include "agx_k5_history.h"
#include "agx_steplog_fold.h"

namespace agx {

// Rows are indexed [t][n], t = index mod T, like the history's.
struct StepLogParams {
    HistParams h;
    float *reward;       // f32 [T][N]
    uint8_t *flags;      // u8  [T][N]
    int64_t *stamp;      // i64 [T][N]   the index the row was recorded for, -1: never
    uint8_t *payload;    // u8  [T][N][W], dword-aligned rows
    int32_t W;           // payload bytes per row: 0 .. 64, a multiple of 4
};

// ---------------------------------------------------------------------------------------------
// k_steplog_record: grid = ceil(N / 256), one env per thread.  An env whose index is -1, not yet issued or already evicted is
// skipped; the payload goes as dwords.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_steplog_record(StepLogParams p, const int64_t *index, const float *reward, const uint8_t *flags,
                                                             const uint32_t *payload) {
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= p.h.N) return;
    const int64_t k = index[n];
    if (!steplog_ok0(k, p.h.count[n], p.h.T)) return;
    const size_t row = (size_t)hist_row(k, p.h.T) * p.h.N + n;
    p.reward[row] = reward[n];
    p.flags[row] = flags[n];
    const int words = p.W >> 2;
    const uint32_t *src = payload + (size_t)n * words;
    uint32_t *dst = reinterpret_cast<uint32_t *>(p.payload) + row * words;
    for (int w = 0; w < words; ++w) dst[w] = src[w];
    p.stamp[row] = k;
}

// the rows of env n, as steplog_step reads them: at(j) is the [t][n] position of row j
struct StepLogRows {
    const StepLogParams &p;
    int n;
    __device__ __forceinline__ size_t at(int64_t j) const { return (size_t)hist_row(j, p.h.T) * p.h.N + n; }
    __device__ __forceinline__ int age(size_t r) const { return (int)p.h.age[r]; }
    __device__ __forceinline__ int64_t stamp(size_t r) const { return p.stamp[r]; }
    __device__ __forceinline__ float reward(size_t r) const { return p.reward[r]; }
    __device__ __forceinline__ uint32_t flags(size_t r) const { return p.flags[r]; }
};

// ---------------------------------------------------------------------------------------------
// k_steplog_gather: grid = ceil(B / 256), one sample per thread.  The loop ends when every lane of the wave has stopped;
// a sample that folded no row writes steps = 0 and next_index = -1 and nothing else.
// ---------------------------------------------------------------------------------------------
struct StepLogOut {
    float *ret, *discount;
    int32_t *steps;
    int64_t *next_index;
    uint8_t *flags;
    uint32_t *payload;
};
__global__ __launch_bounds__(kThreads) void k_steplog_gather(StepLogParams p, const int32_t *env, const int64_t *index, int32_t B, int32_t nstep,
                                                             float gamma, StepLogOut o) {
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int n = 0;
    int64_t k = -1, cnt = 0;
    bool go = false;
    if (b < B) {
        n = env[b];
        k = index[b];
        if (n >= 0 && n < p.h.N) {
            cnt = p.h.count[n];
            go = steplog_ok0(k, cnt, p.h.T);
        } else {
            n = 0;
        }
    }
    const StepLogRows rows{p, n};
    StepFold f;
    for (int i = 1; i <= nstep; ++i) {
        if (go) go = steplog_step(f, rows, k, cnt, i, gamma);
        if (!__any(go)) break;
    }
    if (b >= B) return;
    o.steps[b] = f.m;
    if (o.next_index) o.next_index[b] = f.m > 0 ? k + f.m : -1;
    if (f.m == 0) return;
    if (o.ret) o.ret[b] = f.G;
    if (o.discount) o.discount[b] = steplog_discount(f);
    if (o.flags) o.flags[b] = (uint8_t)f.last;
    if (o.payload) {
        const int words = p.W >> 2;
        const uint32_t *src = reinterpret_cast<const uint32_t *>(p.payload) + rows.at(k + 1) * words;
        uint32_t *dst = o.payload + (size_t)b * words;
        for (int w = 0; w < words; ++w) dst[w] = src[w];
    }
}

}  // namespace agx
