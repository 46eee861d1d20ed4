// agx_k12_rollout.h - K12: on-policy rollouts on the step log (include/agx_rollout.h).  k_rollout_gather walks every env's rows
// backward from its newest and writes the last L transitions, k_slot_fold<GaeFold> folds GAE(lambda) over them.  The rule and the
// fold are agx_rollout_math.h's, the validity of an observation agx_hist_rule.h's: nothing is restated here.  Every device write is
// an ordinary vector store.
#pragma once
#include "agx_k8_steplog.h"
#include "agx_rollout_math.h"
#include "agx_slot_fold.h"

namespace agx {

struct RolloutOut {
    int32_t *len;                      // [N] or nullptr
    int64_t *obs_index, *next_index;   // [L][N]; next_index or nullptr
    float *reward;                     // [L][N] or nullptr
    uint8_t *ends;                     // [L][N] or nullptr
    uint32_t *payload;                 // [L][N][W / 4] or nullptr
};

// ---------------------------------------------------------------------------------------------
// k_rollout_gather: block = 256 = four waves, one wave per env, grid = ceil(N / 4).  The env and its count are wave-uniform and
// come through the scalar cache.  The lanes of a wave are 64 consecutive rows j = top - lane, newest first; per pass each lane
// classifies its row (rollout_row: stop, skip or take), ballot + find-first give the first stop, and a prefix count over the
// taken rows in front of a lane gives its slot, so the age-0 rows drop out with no serial step.  A lane whose slot is still
// inside L writes the transition; the passes go on until a stop or L slots.  Then the wave writes the slots in front of the
// live ones as padding, so every element of every output is written exactly once.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_rollout_gather(StepLogParams p, int32_t L, RolloutOut o) {
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)));
    if (n >= p.h.N) return;                                          // (by whole waves: nothing below synchronises the block)
    const int64_t cnt = uniform_load_i64(p.h.count + n);
    const StepLogRows rows{p, n};
    const int words = p.W >> 2;
    int filled = 0;
    bool go = true;
    for (int64_t top = cnt - 1; go; top -= 64) {
        const int64_t j = top - lane;
        const RolloutRow w = rollout_row(rows, j, cnt, p.h.T, p.h.fs);
        const unsigned long long stop = __ballot(w == kRolloutStop);
        const int first = stop ? __ffsll(stop) - 1 : 64;
        const bool take = w == kRolloutTake && lane < first;
        const unsigned long long taken = __ballot(take);
        const int t = L - 1 - filled - __popcll(taken & ((1ull << lane) - 1ull));
        if (take && t >= 0) {
            const size_t i = (size_t)t * p.h.N + n, r = rows.at(j);
            o.obs_index[i] = j - 1;
            if (o.next_index) o.next_index[i] = j;
            if (o.reward) o.reward[i] = rows.reward(r);
            if (o.ends) o.ends[i] = (uint8_t)rollout_ends(rows, j, cnt, t == L - 1);
            if (o.payload) {
                const uint32_t *src = reinterpret_cast<const uint32_t *>(p.payload) + r * words;
                uint32_t *dst = o.payload + i * words;
                for (int k = 0; k < words; ++k) dst[k] = src[k];
            }
        }
        filled += __popcll(taken);
        go = first == 64 && filled < L;
    }
    const int len = min(filled, L);
    for (int t = lane; t < L - len; t += 64) {
        const size_t i = (size_t)t * p.h.N + n;
        o.obs_index[i] = -1;
        if (o.next_index) o.next_index[i] = -1;
        if (o.reward) o.reward[i] = 0.0f;
        if (o.ends) o.ends[i] = 0;
        if (o.payload)
            for (int k = 0; k < words; ++k) o.payload[i * words + k] = 0u;
    }
    if (lane == 0 && o.len) o.len[n] = len;
}

// ---------------------------------------------------------------------------------------------
// GAE(lambda) over the gathered slots: k_slot_fold<GaeFold, BOOT> (agx_slot_fold.h), folding every step with gae_step.
// ---------------------------------------------------------------------------------------------
#ifndef AGX_GAE_AHEAD
#define AGX_GAE_AHEAD 16             // the set depth; 8 has not been measured in this form (DESIGN.md sections 21 and 23)
#endif

struct GaeParams {
    const int32_t *len;          // [N]
    const float *reward;         // [L][N]
    const uint8_t *ends;         // [L][N]
    const float *value, *boot;   // [L][N]; boot or nullptr
    float *adv, *ret;            // [L][N]
    int32_t N, L;
    float gamma, lambda;
};

struct GaeFold {
    using Params = GaeParams;
    using Out = GaeOut;
    static constexpr int kAhead = AGX_GAE_AHEAD;
    struct Set {
        float r[kAhead], v[kAhead], b[kAhead];
        uint32_t e[kAhead];
    };
    static __device__ __forceinline__ float coef(const Params &q) { return steplog_fmul(q.gamma, q.lambda); }
    template <bool BOOT>
    static __device__ __forceinline__ void load(Set &s, int i, const Params &q, uint32_t a) {
        s.r[i] = q.reward[a];
        s.v[i] = q.value[a];
        s.e[i] = q.ends[a];
        s.b[i] = BOOT ? q.boot[a] : 0.0f;
    }
    static __device__ __forceinline__ Out step(float &A, const Set &s, int i, bool newest, float vnext, const Params &q, float gl) {
        return gae_step(A, s.e[i], newest, s.r[i], s.v[i], vnext, s.b[i], q.gamma, gl);
    }
    static __device__ __forceinline__ void store(const Params &q, uint32_t a, bool live, const Out &g) {
        q.adv[a] = live ? g.adv : 0.0f;
        q.ret[a] = live ? g.ret : 0.0f;
    }
};

}  // namespace agx
