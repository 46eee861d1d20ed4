// agx_k12_rollout.h - K12: on-policy rollouts on the step log (include/agx_rollout.h).  k_rollout_gather walks every env's rows
// backward from its newest and writes the last L transitions, k_rollout_gae folds GAE(lambda) over them.  The rule and the fold
// are agx_rollout_math.h's, the validity of an observation agx_hist_rule.h's: nothing is restated here.  Every device write is
// an ordinary vector store.
#pragma once
#include "agx_k8_steplog.h"
#include "agx_rollout_math.h"

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
// k_rollout_gae<BOOT>: block = 64 = one wave, one env per thread, grid = ceil(N / 64): N = 1024 spreads over 16 CUs.  The arrays
// are time-major, so every load and store of a step is coalesced across the envs of a wave.  The fold is a serial chain per env,
// so the loads must not sit on it: the kernel keeps two register sets of kGaeAhead steps, issues the loads of the next set
// - they depend on nothing but t - and then folds the current one (gae_step, in the order of the header: nothing is
// reassociated).  A slot is addressed by its 32-bit element number (L * N <= INT32_MAX), which goes down by N per step: the
// step offsets are wave-uniform and stay on the scalar unit.  Only the last set can be short (the L mod kGaeAhead oldest
// slots): its loads are clamped to its oldest slot and its fold stops there (FULL = false).  A slot that is not live is folded
// too and then written as 0: the live slots are the newest ones, so nothing the fold made of a padded slot reaches them.
// BOOT = false: d_boot_value is NULL and reads as 0.
// ---------------------------------------------------------------------------------------------
constexpr int kGaeThreads = 64, kGaeAhead = 16;

struct GaeParams {
    const int32_t *len;          // [N]
    const float *reward;         // [L][N]
    const uint8_t *ends;         // [L][N]
    const float *value, *boot;   // [L][N]; boot or nullptr
    float *adv, *ret;            // [L][N]
    int32_t N, L;
    float gamma, lambda;
};

struct GaeSet {
    float r[kGaeAhead], v[kGaeAhead], b[kGaeAhead];
    uint32_t e[kGaeAhead];
};

// the cnt slots from element `at` (slot t0 of the thread's env) downward; FULL: cnt == kGaeAhead
template <bool BOOT, bool FULL>
__device__ __forceinline__ void gae_load(GaeSet &s, const GaeParams &q, uint32_t at, int cnt) {
#pragma unroll
    for (int i = 0; i < kGaeAhead; ++i) {
        const uint32_t a = at - (uint32_t)(FULL ? i : min(i, cnt - 1)) * (uint32_t)q.N;
        s.r[i] = q.reward[a];
        s.v[i] = q.value[a];
        s.e[i] = q.ends[a];
        s.b[i] = BOOT ? q.boot[a] : 0.0f;
    }
}

template <bool FULL>
__device__ __forceinline__ void gae_fold_set(const GaeSet &s, const GaeParams &q, uint32_t at, int t0, int cnt, int first, float gl, float &A,
                                             float &vnext) {
#pragma unroll
    for (int i = 0; i < kGaeAhead; ++i) {
        if (FULL || i < cnt) {                                       // (uniform: cnt depends on nothing of the env)
            const int t = t0 - i;
            const GaeOut g = gae_step(A, s.e[i], t == q.L - 1, s.r[i], s.v[i], vnext, s.b[i], q.gamma, gl);
            vnext = s.v[i];
            const uint32_t a = at - (uint32_t)i * (uint32_t)q.N;
            q.adv[a] = t >= first ? g.adv : 0.0f;
            q.ret[a] = t >= first ? g.ret : 0.0f;
        }
    }
}

template <bool BOOT>
__global__ __launch_bounds__(kGaeThreads) void k_rollout_gae(GaeParams q) {
    const int n = blockIdx.x * kGaeThreads + threadIdx.x;
    if (n >= q.N) return;
    const int first = q.L - min(max(q.len[n], 0), q.L);
    const float gl = steplog_fmul(q.gamma, q.lambda);
    const uint32_t stride = (uint32_t)kGaeAhead * (uint32_t)q.N;
    float A = 0.0f, vnext = 0.0f;
    int t0 = q.L - 1, cnt = min(kGaeAhead, q.L);
    uint32_t at = (uint32_t)t0 * (uint32_t)q.N + (uint32_t)n;
    GaeSet cur, nxt;
    if (cnt == kGaeAhead)
        gae_load<BOOT, true>(cur, q, at, cnt);
    else
        gae_load<BOOT, false>(cur, q, at, cnt);
    for (;;) {
        const int ahead = min(kGaeAhead, t0 + 1 - cnt);              // the slots of the next set; a short set is the last one
        if (ahead == kGaeAhead)
            gae_load<BOOT, true>(nxt, q, at - stride, ahead);
        else if (ahead > 0)
            gae_load<BOOT, false>(nxt, q, at - stride, ahead);
        if (cnt == kGaeAhead)
            gae_fold_set<true>(cur, q, at, t0, cnt, first, gl, A, vnext);
        else
            gae_fold_set<false>(cur, q, at, t0, cnt, first, gl, A, vnext);
        if (ahead == 0) break;
        cur = nxt;
        t0 -= kGaeAhead;
        at -= stride;
        cnt = ahead;
    }
}

}  // namespace agx
