// agx_replay_draw.h - the pick and draw arithmetic of the replay sampler (include/agx_replay.h), as __host__ __device__
// functions: the kernels of agx_k7_replay.h and a plain C++ program (tests/replay_harness.cpp) run the very same code.
// Integers only; nothing here touches the GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AGX_HD __host__ __device__ inline
#else
#define AGX_HD inline
#endif

namespace agx {

// splitmix64's finaliser
AGX_HD uint64_t replay_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// SM(s, i): the i-th output (i = 0 first) of splitmix64 seeded with s
AGX_HD uint64_t replay_sm(uint64_t s, uint64_t i) { return replay_mix(s + (i + 1) * 0x9E3779B97F4A7C15ull); }

// the high 64 bits of a * b
AGX_HD uint64_t replay_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// the oldest retained index of an env with cnt appends, and the number of its candidates: k in [lo, lo + L) leaves k + forward
// below cnt
AGX_HD int64_t replay_lo(int64_t cnt, int32_t T) { return cnt > T ? cnt - T : 0; }
AGX_HD int64_t replay_len(int64_t cnt, int32_t T, int32_t forward) {
    const int64_t l = cnt - forward - replay_lo(cnt, T);
    return l > 0 ? l : 0;
}

// u = (z * total) >> 64: uniform over 0 .. total - 1 up to a bias of at most total / 2^64
AGX_HD int64_t replay_pick(uint64_t z, int64_t total) { return (int64_t)replay_mulhi(z, (uint64_t)total); }

// the env n with off[n] <= u < off[n + 1]; off[0 .. N] is an exclusive prefix sum (off[0] = 0 <= u < off[N]).  Envs without
// candidates (off[n] == off[n + 1]) are never found.
AGX_HD int32_t replay_find_env(const int64_t *off, int32_t N, int64_t u) {
    int32_t lo = 0, hi = N;
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= u)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// One attempt: z = SM(key, b * attempts + a) in 64 bits, then the candidate it lands on.
struct ReplayCandidate {
    int32_t n;
    int64_t at;      // u - off[n]: the candidate's position among env n's; k = lo_n + at
};
AGX_HD ReplayCandidate replay_candidate(uint64_t key, int64_t b, int32_t attempts, int32_t a, const int64_t *off, int32_t N, int64_t total) {
    const uint64_t z = replay_sm(key, (uint64_t)b * (uint64_t)attempts + (uint64_t)a);
    const int64_t u = replay_pick(z, total);
    ReplayCandidate c;
    c.n = replay_find_env(off, N, u);
    c.at = u - off[c.n];
    return c;
}

}  // namespace agx
