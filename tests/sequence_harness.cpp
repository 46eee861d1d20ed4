// The __host__ side of active-gym_amd/csrc/agx_sequence_math.h - the very functions k_sequence_gather decides every step with -
// on host arrays.
//
//     sequence_harness <file>            the tokens below, whitespace separated, read from a file
//     sequence_harness <token> ...       ... or given as arguments
//
// tokens: T N fs L, count[N], age[T*N] (rows [t][n]), then any number of samples "n k".  Per sample one line: its length.
#include <cinttypes>
#include <cstdio>

#include "agx_sequence_math.h"
#include "harness_tokens.h"

namespace {

struct HostRows {
    int32_t T, N, n;
    const int64_t *age_;
    size_t at(int64_t j) const { return (size_t)(j % T) * N + n; }
    int age(size_t r) const { return (int)age_[r]; }
};

}  // namespace

int main(int argc, char **argv) {
    Tokens in;
    if (!in.read(argc, argv)) return 2;
    const int32_t T = (int32_t)in.next(), N = (int32_t)in.next(), fs = (int32_t)in.next(), L = (int32_t)in.next();
    if (in.short_input || T <= 0 || N <= 0 || fs < 1 || L < 1 || L > agx::kSequenceLimit) {
        fprintf(stderr, "usage: %s <file> | T N fs L count[N] age[T*N] [n k ...]\n", argv[0]);
        return 2;
    }
    const size_t rows = (size_t)T * N;
    std::vector<int64_t> count(N), age(rows);
    for (auto &v : count) v = in.next();
    for (auto &v : age) v = in.next();
    if (in.short_input || in.left() % 2) {
        fprintf(stderr, "%s: the arrays are incomplete or a sample lacks its index\n", argv[0]);
        return 2;
    }
    while (in.left()) {
        const int64_t n = in.next(), k = in.next();
        const bool env = n >= 0 && n < N;
        const HostRows r{T, N, env ? (int32_t)n : 0, age.data()};
        printf("%d\n", agx::sequence_length(r, env, k, env ? count[n] : 0, T, fs, L));
    }
    return 0;
}
