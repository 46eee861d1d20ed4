// The __host__ side of active-gym_amd/csrc/agx_replay_draw.h - the very functions k_replay_scan / k_replay_draw call - on
// synthetic candidate counts, so that offsets beyond 2^32 are exercised without a history of that size.
//
//     replay_harness <key> <attempts> <draws> <lo_0> <L_0> [<lo_1> <L_1> ...]
//
// prints "sm <SM(1234567, 0)> <SM(1234567, 1)> <SM(1234567, 2)>", "total <off[N]>", then for b = 0 .. draws - 1 the candidate
// "n k" of attempt a = b % attempts of sample b.  `replay_harness len <cnt> <T> <forward>` prints "lo_n L_n" of one env.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "agx_replay_draw.h"

int main(int argc, char **argv) {
    if (argc == 5 && argv[1][0] == 'l') {          // replay_harness len <cnt> <T> <forward>: "lo L"
        const int64_t cnt = atoll(argv[2]);
        const int32_t T = (int32_t)atoi(argv[3]), forward = (int32_t)atoi(argv[4]);
        printf("%" PRId64 " %" PRId64 "\n", agx::replay_lo(cnt, T), agx::replay_len(cnt, T, forward));
        return 0;
    }
    if (argc < 6 || (argc - 4) % 2) {
        fprintf(stderr, "usage: %s key attempts draws lo L [lo L ...]\n", argv[0]);
        return 2;
    }
    const uint64_t key = strtoull(argv[1], nullptr, 10);
    const int32_t attempts = (int32_t)atoi(argv[2]);
    const int64_t draws = atoll(argv[3]);
    const int32_t N = (argc - 4) / 2;
    std::vector<int64_t> lo(N), off(N + 1, 0);
    for (int32_t n = 0; n < N; ++n) {
        lo[n] = atoll(argv[4 + 2 * n]);
        off[n + 1] = off[n] + atoll(argv[5 + 2 * n]);
    }
    printf("sm %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", agx::replay_sm(1234567, 0), agx::replay_sm(1234567, 1), agx::replay_sm(1234567, 2));
    printf("total %" PRId64 "\n", off[N]);
    if (off[N] <= 0) return 0;
    for (int64_t b = 0; b < draws; ++b) {
        const agx::ReplayCandidate c = agx::replay_candidate(key, b, attempts, (int32_t)(b % attempts), off.data(), N, off[N]);
        printf("%d %" PRId64 "\n", c.n, lo[c.n] + c.at);
    }
    return 0;
}
