// The __host__ side of active-gym_amd/csrc/agx_priority_math.h - the very functions the kernels of agx_k9_priority.h call - over
// host arrays: a history's bookkeeping and a priority table come in as text, the draw of one call goes out.
//
//     priority_harness q <f32 bits> [<f32 bits> ...]      prints quantise() of each float, given by its bit pattern
//     priority_harness <file>                             the file holds, whitespace-separated:
//         N T fs back forward wmax key B
//         per env: cnt, then for each of the T rows (row = index mod T): age stamp <f32 bits of the priority>
//     prints "total <total> accepted <rows with W > 0>", then for b = 0 .. B - 1 "n k W" ("-1 -1 0" when total == 0), then
//     "lookup" and for every env and k = -1 .. cnt the effective weight of a retained (n, k), -1 otherwise.
// The weight of a row is quantise(priority), so the table is built by the code under test as well.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "agx_priority_math.h"

namespace {

float from_bits(uint32_t bits) {
    float f;
    memcpy(&f, &bits, sizeof(f));
    return f;
}

struct HostAges {                       // the age bytes of one env, by row
    const int32_t *rows;
    int32_t T;
    int32_t age(int64_t j) const { return rows[j % T]; }
};

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 3 && strcmp(argv[1], "q") == 0) {
        for (int i = 2; i < argc; ++i) printf("%u\n", agx::priority_quantise(from_bits((uint32_t)strtoul(argv[i], nullptr, 10))));
        return 0;
    }
    if (argc != 2) {
        fprintf(stderr, "usage: %s q bits... | %s file\n", argv[0], argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int32_t N, T, fs, back, forward;
    uint32_t wmax;
    uint64_t key;
    int64_t B;
    if (fscanf(f, "%d %d %d %d %d %u %" SCNu64 " %" SCNd64, &N, &T, &fs, &back, &forward, &wmax, &key, &B) != 8) return 2;
    std::vector<int64_t> cnt(N), stamp((size_t)N * T), off(N + 1, 0);
    std::vector<int32_t> age((size_t)N * T);
    std::vector<uint32_t> weight((size_t)N * T);
    for (int32_t n = 0; n < N; ++n) {
        if (fscanf(f, "%" SCNd64, &cnt[n]) != 1) return 2;
        for (int32_t t = 0; t < T; ++t) {
            uint32_t bits;
            if (fscanf(f, "%d %" SCNd64 " %u", &age[(size_t)n * T + t], &stamp[(size_t)n * T + t], &bits) != 3) return 2;
            weight[(size_t)n * T + t] = agx::priority_quantise(from_bits(bits));
        }
    }
    fclose(f);
    // W and its inclusive prefix per env, by position k - lo_n
    std::vector<std::vector<int64_t>> incl(N);
    int64_t accepted = 0;
    for (int32_t n = 0; n < N; ++n) {
        const int64_t lo = agx::replay_lo(cnt[n], T);
        const HostAges ages{age.data() + (size_t)n * T, T};
        int64_t run = 0;
        for (int64_t k = lo; k < cnt[n]; ++k) {
            const size_t row = (size_t)n * T + (size_t)(k % T);
            const int64_t w = agx::priority_row_weight(ages, k, cnt[n], lo, fs - 1, back, forward, stamp[row], weight[row], wmax);
            accepted += w > 0;
            run += w;
            incl[n].push_back(run);
        }
        off[n + 1] = off[n] + run;
    }
    const int64_t total = off[N];
    printf("total %" PRId64 " accepted %" PRId64 "\n", total, accepted);
    for (int64_t b = 0; b < B; ++b) {
        if (total <= 0) {
            printf("-1 -1 0\n");
            continue;
        }
        const int64_t u = agx::replay_pick(agx::replay_sm(key, (uint64_t)b), total);
        const int32_t n = agx::replay_find_env(off.data(), N, u);
        const int64_t v = u - off[n];
        const int32_t at = agx::priority_find_row(incl[n].data(), (int32_t)incl[n].size(), v);
        printf("%d %" PRId64 " %" PRId64 "\n", n, agx::replay_lo(cnt[n], T) + at, incl[n][at] - (at > 0 ? incl[n][at - 1] : 0));
    }
    printf("lookup\n");
    for (int32_t n = 0; n < N; ++n)
        for (int64_t k = -1; k <= cnt[n]; ++k) {
            const bool kept = k >= agx::replay_lo(cnt[n], T) && k < cnt[n];
            const size_t row = (size_t)n * T + (size_t)(kept ? k % T : 0);
            printf("%" PRId64 "\n", kept ? (int64_t)agx::priority_effective(stamp[row], weight[row], k, wmax) : (int64_t)-1);
        }
    return 0;
}
