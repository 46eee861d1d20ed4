// The __host__ side of active-gym_amd/csrc/agx_chunk_math.h - the very functions k_chunk_scan and k_chunk_take count, look chunks
// up and walk their steps with - on host arrays.
//
//     chunks_harness <file>            the tokens below, whitespace separated, read from a file
//     chunks_harness <token> ...       ... or given as arguments
//
// A u64 travels as two tokens, its high and its low 32 bits.
// tokens, the counts:  1 N L C, len[N].  One line "count" per env.
// tokens, a take:      2 permute N L C first S seen_L seen_C ek_hi ek_lo, off[N+1], len[N], ends[L*N] (slots [t][n]).  Per row one line
//                      "chunk first steps valid env" followed by "slot ends start mask" for each of the C steps.  (seen_L, seen_C) are
//                      what the select that made off recorded; total is off[N].
// tokens, the keys:    3 seed_hi seed_lo calls.  One line "base_hi base_lo key_hi key_lo": SM(seed, the chunker's list number) and the
//                      key of select number `calls`.
// tokens, the struct:  4.  One line "sizeof(agx_chunks_io) offsetof(d_slot) offsetof(d_valid)", as the C compiler lays it out.
#include <cinttypes>
#include <cstddef>
#include <cstdio>

#include "agx_chunk_math.h"
#include "agx_chunks.h"
#include "harness_tokens.h"

namespace {

uint64_t next_u64(Tokens &in) {
    const uint64_t hi = (uint64_t)in.next() & 0xFFFFFFFFull, lo = (uint64_t)in.next() & 0xFFFFFFFFull;
    return (hi << 32) | lo;
}

int usage(const char *argv0) {
    fprintf(stderr, "usage: %s <file> | 1 N L C len[N] | 2 permute N L C first S seen_L seen_C ek_hi ek_lo off[N+1] len[N] ends[L*N]"
                    " | 3 seed_hi seed_lo calls | 4\n", argv0);
    return 2;
}

}  // namespace

int main(int argc, char **argv) {
    Tokens in;
    if (!in.read(argc, argv)) return 2;
    const int64_t what = in.next();
    if (what == 1 || what == 2) {
        const bool permute = what == 2 && in.next() != 0;
        const int32_t N = (int32_t)in.next(), L = (int32_t)in.next(), C = (int32_t)in.next();
        int64_t first = 0, S = 0, seen_L = 0, seen_C = 0;
        uint64_t ek = 0;
        if (what == 2) {
            first = in.next();
            S = in.next();
            seen_L = in.next();
            seen_C = in.next();
            ek = next_u64(in);
        }
        if (in.short_input || N <= 0 || L < 1 || L > agx::kMbLimit || (int64_t)L * N > INT32_MAX || C < 1 || C > L || C > agx::kChunkLimit || first < 0 ||
            S < 0 || first + S > INT32_MAX || C * S > INT32_MAX)
            return usage(argv[0]);
        std::vector<int32_t> off(what == 2 ? (size_t)N + 1 : 0), len(N);
        std::vector<uint8_t> ends(what == 2 ? (size_t)L * N : 0);
        for (auto &v : off) v = (int32_t)in.next();
        for (auto &v : len) v = (int32_t)in.next();
        for (auto &v : ends) v = (uint8_t)in.next();
        if (!in.complete()) {
            fprintf(stderr, "%s: the arrays are incomplete or over-long\n", argv[0]);
            return 2;
        }
        if (what == 1) {
            for (int32_t n = 0; n < N; ++n) printf("%d\n", agx::chunk_count(len[n], L, C));
            return 0;
        }
        const int32_t total = off[N];
        for (int64_t i = 0; i < S; ++i) {
            const int32_t p = (int32_t)(first + i);
            agx::ChunkAt c{0, -1, L, 0, 0, false};
            if (total > 0 && seen_L == L && seen_C == C) c = agx::chunk_at(off.data(), len.data(), N, L, C, agx::mb_position(ek, total, p, permute));
            const bool valid = c.found && p < total;
            printf("%d %d %d %d %d", c.g, c.first, c.steps, valid ? 1 : 0, c.n);
            for (int32_t l = 0; l < C; ++l) {
                const agx::ChunkStep st = agx::chunk_step(c, ends.data(), N, L, C, l, valid);
                if (st.live != agx::chunk_live(c, L, C, l)) return 3;
                printf(" %d %d %d %d", st.live ? st.t * N + c.n : -1, (int)st.ends, (int)st.start, (int)st.mask);
            }
            printf("\n");
        }
        return 0;
    }
    if (what == 3) {
        const uint64_t seed = next_u64(in);
        const int64_t calls = in.next();
        if (!in.complete() || calls < 0) return usage(argv[0]);
        const uint64_t base = agx::replay_sm(seed, (uint64_t)agx::kChunkList), key = agx::replay_sm(base, (uint64_t)calls);
        printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", base >> 32, base & 0xFFFFFFFFull, key >> 32, key & 0xFFFFFFFFull);
        return 0;
    }
    if (what == 4) {
        printf("%zu %zu %zu\n", sizeof(agx_chunks_io), offsetof(agx_chunks_io, d_slot), offsetof(agx_chunks_io, d_valid));
        return 0;
    }
    return usage(argv[0]);
}
