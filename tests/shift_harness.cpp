// The __host__ side of active-gym_amd/csrc/agx_shift_math.h - the very functions k_history_observe_shifted / k_shift_draw call.
//
//     shift_harness draw <seed> <calls> <pad> <B>     "dy dx" of samples 0 .. B - 1 of call number <calls>
//     shift_harness src <pad> <n>                     one line per d = 0 .. 2 * pad: shift_src(i, d, pad, n) for i = 0 .. n - 1
//     shift_harness clamp <pad> <d> [<d> ...]         shift_clamp of each d
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "agx_shift_math.h"

int main(int argc, char **argv) {
    if (argc == 6 && !strcmp(argv[1], "draw")) {
        const uint64_t seed = strtoull(argv[2], nullptr, 10), calls = strtoull(argv[3], nullptr, 10);
        const int32_t pad = (int32_t)atoi(argv[4]);
        const int64_t B = atoll(argv[5]);
        const uint64_t key = agx::shift_key(seed, calls);
        for (int64_t b = 0; b < B; ++b) {
            const agx::ShiftPair s = agx::shift_draw(key, (uint64_t)b, pad);
            printf("%d %d\n", s.dy, s.dx);
        }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "src")) {
        const int32_t pad = (int32_t)atoi(argv[2]), n = (int32_t)atoi(argv[3]);
        for (int32_t d = 0; d <= 2 * pad; ++d) {
            for (int32_t i = 0; i < n; ++i) printf("%d%c", agx::shift_src(i, d, pad, n), i + 1 < n ? ' ' : '\n');
        }
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "clamp")) {
        const int32_t pad = (int32_t)atoi(argv[2]);
        for (int a = 3; a < argc; ++a) printf("%d%c", agx::shift_clamp((int32_t)atoi(argv[a]), pad), a + 1 < argc ? ' ' : '\n');
        return 0;
    }
    fprintf(stderr, "usage: %s draw seed calls pad B | src pad n | clamp pad d [d ...]\n", argv[0]);
    return 2;
}
