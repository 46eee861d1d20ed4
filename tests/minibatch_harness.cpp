// The __host__ side of active-gym_amd/csrc/agx_minibatch_math.h - the very functions k_mb_count, k_mb_scan and k_mb_take count,
// permute and look slots up with - on host arrays.
//
//     minibatch_harness <file>            the tokens below, whitespace separated, read from a file
//     minibatch_harness <token> ...       ... or given as arguments
//
// A u64 travels as two tokens, its high and its low 32 bits.
// tokens, the permutation:  0 ek_hi ek_lo total.  One line "perm(m)" per m in [0, total).
// tokens, the counts:       1 which N L, len[N], ends[L*N] (slots [t][n]).  One line "count" per env.
// tokens, a take:           2 which permute N L first S ek_hi ek_lo, off[N+1], len[N], ends[L*N].  Per row one line "slot env valid".
// tokens, the keys:         3 seed_hi seed_lo which calls.  One line "base_hi base_lo key_hi key_lo": SM(seed, which) and the key of
//                           select number `calls` of that list.
// tokens, epochs:           4 s total epochs positions.  For e in [0, epochs) one line of perm(m), m in [0, positions), under
//                           ek = SM(s, e).
#include <cinttypes>
#include <cstdio>

#include "agx_minibatch_math.h"
#include "harness_tokens.h"

namespace {

uint64_t next_u64(Tokens &in) {
    const uint64_t hi = (uint64_t)in.next() & 0xFFFFFFFFull, lo = (uint64_t)in.next() & 0xFFFFFFFFull;
    return (hi << 32) | lo;
}

int usage(const char *argv0) {
    fprintf(stderr, "usage: %s <file> | 0 ek_hi ek_lo total | 1 which N L len[N] ends[L*N] | 2 which permute N L first S ek_hi ek_lo off[N+1] len[N] ends[L*N]"
                    " | 3 seed_hi seed_lo which calls | 4 s total epochs positions\n", argv0);
    return 2;
}

}  // namespace

int main(int argc, char **argv) {
    Tokens in;
    if (!in.read(argc, argv)) return 2;
    const int64_t what = in.next();
    if (what == 0) {
        const uint64_t ek = next_u64(in);
        const int64_t total = in.next();
        if (!in.complete() || total < 1 || total > INT32_MAX) return usage(argv[0]);
        for (int32_t m = 0; m < (int32_t)total; ++m) printf("%d\n", agx::mb_perm(ek, (int32_t)total, m));
        return 0;
    }
    if (what == 1 || what == 2) {
        const int which = (int)in.next();
        const bool permute = what == 2 && in.next() != 0;
        const int32_t N = (int32_t)in.next(), L = (int32_t)in.next();
        int64_t first = 0, S = 0;
        uint64_t ek = 0;
        if (what == 2) {
            first = in.next();
            S = in.next();
            ek = next_u64(in);
        }
        if (in.short_input || (which != agx::kMbLive && which != agx::kMbBoot) || N <= 0 || L < 1 || L > agx::kMbLimit || (int64_t)L * N > INT32_MAX ||
            first < 0 || S < 0 || first + S > INT32_MAX)
            return usage(argv[0]);
        std::vector<int32_t> off(what == 2 ? (size_t)N + 1 : 0), len(N);
        std::vector<uint8_t> ends((size_t)L * N);
        for (auto &v : off) v = (int32_t)in.next();
        for (auto &v : len) v = (int32_t)in.next();
        for (auto &v : ends) v = (uint8_t)in.next();
        if (!in.complete()) {
            fprintf(stderr, "%s: the arrays are incomplete or over-long\n", argv[0]);
            return 2;
        }
        if (what == 1) {
            for (int32_t n = 0; n < N; ++n) printf("%d\n", agx::mb_count(which, len.data(), ends.data(), N, L, n));
            return 0;
        }
        const int32_t total = off[N];
        for (int64_t i = 0; i < S; ++i) {
            const int32_t p = (int32_t)(first + i);
            int32_t e = -1, n = 0;
            if (total > 0) {
                e = agx::mb_slot(which, off.data(), len.data(), ends.data(), N, L, agx::mb_position(ek, total, p, permute), &n);
                if (e < 0) n = 0;
            }
            printf("%d %d %d\n", e, n, e >= 0 && p < total ? 1 : 0);
        }
        return 0;
    }
    if (what == 3) {
        const uint64_t seed = next_u64(in);
        const int64_t which = in.next(), calls = in.next();
        if (!in.complete() || which < 0 || calls < 0) return usage(argv[0]);
        const uint64_t base = agx::replay_sm(seed, (uint64_t)which), key = agx::replay_sm(base, (uint64_t)calls);
        printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", base >> 32, base & 0xFFFFFFFFull, key >> 32, key & 0xFFFFFFFFull);
        return 0;
    }
    if (what == 4) {
        const int64_t s = in.next(), total = in.next(), epochs = in.next(), positions = in.next();
        if (!in.complete() || s < 0 || total < 1 || total > INT32_MAX || epochs < 0 || positions < 0 || positions > total) return usage(argv[0]);
        for (int64_t e = 0; e < epochs; ++e) {
            const uint64_t ek = agx::replay_sm((uint64_t)s, (uint64_t)e);
            for (int64_t m = 0; m < positions; ++m) printf(m ? " %d" : "%d", agx::mb_perm(ek, (int32_t)total, (int32_t)m));
            printf("\n");
        }
        return 0;
    }
    return usage(argv[0]);
}
