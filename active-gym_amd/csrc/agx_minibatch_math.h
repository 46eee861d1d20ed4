// agx_minibatch_math.h - the arithmetic of the minibatcher (include/agx_minibatch.h), as __host__ __device__ functions beside
// agx_replay_draw.h, whose splitmix64 it uses: which slots of a gathered rollout are selected, the seeded permutation of their
// list and the slot at a list position.  The kernels of agx_k15_minibatch.h and a plain C++ program (tests/minibatch_harness.cpp)
// run the very same code.  Integers only; nothing here touches the GPU.
#pragma once
#include "agx_replay_draw.h"

namespace agx {

constexpr int kMbLive = 0, kMbBoot = 1;          // AGX_MB_LIVE, AGX_MB_BOOT
constexpr int kMbStreams = 8;                    // AGX_MB_STREAMS
constexpr int kMbLimit = 4096;                   // AGX_MB_LIMIT: L, the limit of a gathered rollout
constexpr uint32_t kMbBootBit = 8;               // the BOOT bit of the rollout gather's ends byte
constexpr int kMbRounds = 6;                     // Feistel rounds: four leave a 4.2 sigma cell with 2-bit halves

// len'(n): the fold's clamp
AGX_HD int32_t mb_len(int32_t len, int32_t L) { return len < 0 ? 0 : len > L ? L : len; }

// the number of selected slots of env n: len' for LIVE, for BOOT the live slots of the column whose ends byte carries BOOT
AGX_HD int32_t mb_count(int which, const int32_t *len, const uint8_t *ends, int32_t N, int32_t L, int32_t n) {
    const int32_t m = mb_len(len[n], L);
    if (which == kMbLive) return m;
    int32_t c = 0;
    for (int32_t t = L - m; t < L; ++t) c += (ends[(size_t)t * N + n] & kMbBootBit) != 0;
    return c;
}

// hb = max(1, ceil(bitlen(total - 1) / 2)): the bits of one half of the Feistel network's domain, 1 .. 16 (total >= 1)
AGX_HD int32_t mb_half_bits(int32_t total) {
    int32_t bits = 0;
    for (uint32_t v = (uint32_t)(total - 1); v; v >>= 1) ++bits;
    const int32_t hb = (bits + 1) >> 1;
    return hb < 1 ? 1 : hb;
}

// perm(m): a bijection on [0, total) keyed by ek, 0 <= m < total.  Six Feistel rounds on 2 * hb bits, walked along the cycle
// that holds m until the value is below total again: the walk ends because m itself lies on that cycle.
AGX_HD int32_t mb_perm(uint64_t ek, int32_t total, int32_t m) {
    const int32_t hb = mb_half_bits(total);
    const uint64_t mask = (1ull << hb) - 1ull;
    uint64_t x = (uint64_t)m;
    do {
        uint64_t l = x >> hb, r = x & mask;
        for (int i = 0; i < kMbRounds; ++i) {
            const uint64_t f = replay_mix(ek + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull + r) & mask;
            const uint64_t nr = l ^ f;
            l = r;
            r = nr;
        }
        x = (l << hb) | r;
    } while (x >= (uint64_t)total);
    return (int32_t)x;
}

// the env n with off[n] <= m < off[n + 1]; off[0 .. N] is an exclusive prefix sum (off[0] = 0 <= m < off[N]).  Envs without
// selected slots are never found.  (replay_find_env in i32.)
AGX_HD int32_t mb_find_env(const int32_t *off, int32_t N, int32_t m) {
    int32_t lo = 0, hi = N;
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= m)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// the slot element t * N + n at list position m (0 <= m < off[N]), or -1 where the r-th selected slot of its env does not exist
// in these len / ends (they are not the ones the offsets were made from).  *env receives n.
AGX_HD int32_t mb_slot(int which, const int32_t *off, const int32_t *len, const uint8_t *ends, int32_t N, int32_t L, int32_t m, int32_t *env) {
    const int32_t n = mb_find_env(off, N, m), r = m - off[n];
    const int32_t live = mb_len(len[n], L);
    *env = n;
    if (which == kMbLive) return r < live ? (L - live + r) * N + n : -1;
    int32_t seen = 0;
    for (int32_t t = L - live; t < L; ++t) {
        if (ends[(size_t)t * N + n] & kMbBootBit) {
            if (seen == r) return t * N + n;
            ++seen;
        }
    }
    return -1;
}

// the list position of row p of a take: p mod total, through the permutation where asked (total >= 1, p >= 0)
AGX_HD int32_t mb_position(uint64_t ek, int32_t total, int32_t p, bool permute) {
    const int32_t m = p % total;
    return permute ? mb_perm(ek, total, m) : m;
}

}  // namespace agx
