// agx_chunk_math.h - the arithmetic of the chunker (include/agx_chunks.h), as __host__ __device__ functions beside
// agx_minibatch_math.h, whose clamp (mb_len), search (mb_find_env) and permutation (mb_perm, mb_position) it calls: how many chunks
// of an env hold a live step, the chunk at a list position and the bytes of one step of it.  The kernels of agx_k17_chunks.h and a
// plain C++ program (tests/chunks_harness.cpp) run the very same code.  Integers only; nothing here touches the GPU.
#pragma once
#include "agx_minibatch_math.h"

namespace agx {

constexpr int kChunkLimit = 256;                 // AGX_CHUNK_LIMIT: C
constexpr int kChunkList = 2;                    // AGX_CHUNK_LIST: the list number in the key, behind kMbLive and kMbBoot
constexpr int kChunkStreams = 8;                 // AGX_CHUNK_STREAMS
constexpr uint32_t kChunkStartChunk = 1, kChunkStartEpisode = 2;   // AGX_CHUNK_START_*
constexpr uint32_t kChunkBreakBits = 7;          // the ends bits behind which an episode starts: terminated, truncated, cut

// G = ceil(L / C)
AGX_HD int32_t chunk_groups(int32_t L, int32_t C) { return (L + C - 1) / C; }

// the number of selected chunks of an env with this len: those from the one that holds t0 = L - len' on
AGX_HD int32_t chunk_count(int32_t len, int32_t L, int32_t C) {
    const int32_t live = mb_len(len, L);
    return live > 0 ? chunk_groups(L, C) - (L - live) / C : 0;
}

struct ChunkAt {
    int32_t n, g, t0, first, steps;              // found: env, chunk, the env's first live slot, the chunk's first live step and their number
    bool found;                                  // not found: n = 0, g = -1, t0 = L, first = steps = 0
};

// the chunk at list position m (0 <= m < off[N]) of the offsets `off`, looked up in this len: not found where the r-th selected
// chunk of its env does not exist there (len is not the one the offsets were made from)
AGX_HD ChunkAt chunk_at(const int32_t *off, const int32_t *len, int32_t N, int32_t L, int32_t C, int32_t m) {
    const int32_t n = mb_find_env(off, N, m);
    const int64_t r = (int64_t)m - off[n];
    const int32_t live = mb_len(len[n], L), t0 = L - live;
    const int64_t g64 = t0 / C + r;
    if (live <= 0 || r < 0 || g64 >= chunk_groups(L, C)) return ChunkAt{0, -1, L, 0, 0, false};
    const int32_t g = (int32_t)g64, lo = g * C, hi = (g + 1) * C;
    const int32_t from = lo > t0 ? lo : t0, to = hi < L ? hi : L;
    return ChunkAt{n, g, t0, from - lo, to - from, true};
}

// step l of chunk c is live: g * C + l lies in [t0, L).  Never where c is not found (t0 = L).
AGX_HD bool chunk_live(const ChunkAt &c, int32_t L, int32_t C, int32_t l) {
    const int32_t t = c.g * C + l;
    return t >= c.t0 && t < L;
}

struct ChunkStep {
    int32_t t;                                   // g * C + l: a slot of [L][N] iff live
    bool live;
    uint8_t ends, start, mask;                   // the slot's ends byte, the START bits and the loss mask: 0 where not live
};

// step l of chunk c (found) under these ends bytes ([L][N]); valid: the row's.  Loads ends[t][n] and, behind t0, ends[t - 1][n]:
// both inside the env's live range.
AGX_HD ChunkStep chunk_step(const ChunkAt &c, const uint8_t *ends, int32_t N, int32_t L, int32_t C, int32_t l, bool valid) {
    ChunkStep s{c.g * C + l, chunk_live(c, L, C, l), 0, 0, 0};
    if (!s.live) return s;
    s.ends = ends[(size_t)s.t * N + c.n];
    s.start = l == c.first ? (uint8_t)kChunkStartChunk : (uint8_t)0;
    if (s.t > c.t0 && (ends[(size_t)(s.t - 1) * N + c.n] & kChunkBreakBits)) s.start |= (uint8_t)kChunkStartEpisode;
    s.mask = valid ? 1 : 0;
    return s;
}

}  // namespace agx
