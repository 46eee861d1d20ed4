// The __host__ side of active-gym_amd/csrc/agx_rollout_math.h - the very functions k_rollout_gather and k_rollout_gae decide every
// row and fold every step with - on host arrays.
//
//     rollout_harness <file>            the tokens below, whitespace separated, read from a file
//     rollout_harness <token> ...       ... or given as arguments
//
// tokens, the walk:  0 T N fs L, count[N], age[T*N], stamp[T*N], flags[T*N] (rows [t][n]).  Per env one line "n len", then one
//                    line "t obs_index next_index ends" per live slot, newest first.
// tokens, the fold:  1 N L gamma_bits lambda_bits has_boot, len[N], reward_bits[L*N], ends[L*N], value_bits[L*N] and, with
//                    has_boot, boot_bits[L*N] (slots [t][n]).  Per slot, in [t][n] order, one line "adv_bits ret_bits".
// Floats travel as the decimal value of their 32-bit pattern.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "agx_rollout_math.h"

namespace {

float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}
uint32_t to_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

struct HostRows {
    int32_t T, N, n;
    const int64_t *age_, *stamp_, *flags_;
    size_t at(int64_t j) const { return (size_t)(j % T) * N + n; }
    int age(size_t r) const { return (int)age_[r]; }
    int64_t stamp(size_t r) const { return stamp_[r]; }
    uint32_t flags(size_t r) const { return (uint32_t)flags_[r]; }
};

}  // namespace

int main(int argc, char **argv) {
    std::vector<std::string> tok;
    if (argc == 2) {
        FILE *f = fopen(argv[1], "r");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        char buf[64];
        while (fscanf(f, "%63s", buf) == 1) tok.emplace_back(buf);
        fclose(f);
    } else {
        for (int i = 1; i < argc; ++i) tok.emplace_back(argv[i]);
    }
    size_t at = 0;
    bool short_input = false;
    auto next = [&]() -> int64_t {
        if (at >= tok.size()) {
            short_input = true;
            return 0;
        }
        return strtoll(tok[at++].c_str(), nullptr, 10);
    };
    const int64_t what = next();
    if (what == 0) {
        const int32_t T = (int32_t)next(), N = (int32_t)next(), fs = (int32_t)next(), L = (int32_t)next();
        if (short_input || T <= 0 || N <= 0 || fs < 1 || L < 1 || L > agx::kRolloutLimit) {
            fprintf(stderr, "usage: %s <file> | 0 T N fs L count[N] age[T*N] stamp[T*N] flags[T*N]\n", argv[0]);
            return 2;
        }
        const size_t rows = (size_t)T * N;
        std::vector<int64_t> count(N), age(rows), stamp(rows), flags(rows);
        for (auto &v : count) v = next();
        for (auto &v : age) v = next();
        for (auto &v : stamp) v = next();
        for (auto &v : flags) v = next();
        if (short_input || at != tok.size()) {
            fprintf(stderr, "%s: the arrays are incomplete or over-long\n", argv[0]);
            return 2;
        }
        for (int32_t n = 0; n < N; ++n) {
            const HostRows r{T, N, n, age.data(), stamp.data(), flags.data()};
            std::string lines;
            const int32_t len = agx::rollout_walk(r, count[n], T, fs, L, [&](int32_t t, int64_t j, uint32_t e) {
                char buf[96];
                snprintf(buf, sizeof buf, "%d %" PRId64 " %" PRId64 " %u\n", t, j - 1, j, e);
                lines += buf;
            });
            printf("%d %d\n%s", n, len, lines.c_str());
        }
        return 0;
    }
    if (what == 1) {
        const int32_t N = (int32_t)next(), L = (int32_t)next();
        const float gamma = from_bits((uint32_t)next()), lambda = from_bits((uint32_t)next());
        const bool has_boot = next() != 0;
        if (short_input || N <= 0 || L < 1 || L > agx::kRolloutLimit) {
            fprintf(stderr, "usage: %s <file> | 1 N L gamma_bits lambda_bits has_boot len[N] reward_bits[L*N] ends[L*N] value_bits[L*N] [boot_bits[L*N]]\n",
                    argv[0]);
            return 2;
        }
        const size_t slots = (size_t)L * N;
        std::vector<int32_t> len(N);
        std::vector<float> reward(slots), value(slots), boot(has_boot ? slots : 0), adv(slots), ret(slots);
        std::vector<uint8_t> ends(slots);
        for (auto &v : len) v = (int32_t)next();
        for (auto &v : reward) v = from_bits((uint32_t)next());
        for (auto &v : ends) v = (uint8_t)next();
        for (auto &v : value) v = from_bits((uint32_t)next());
        for (auto &v : boot) v = from_bits((uint32_t)next());
        if (short_input || at != tok.size()) {
            fprintf(stderr, "%s: the arrays are incomplete or over-long\n", argv[0]);
            return 2;
        }
        for (int32_t n = 0; n < N; ++n)
            agx::gae_fold([&](int32_t t) { return (size_t)t * N + n; }, L, len[n], reward.data(), ends.data(), value.data(),
                          has_boot ? boot.data() : nullptr, gamma, lambda, adv.data(), ret.data());
        for (size_t i = 0; i < slots; ++i) printf("%" PRIu32 " %" PRIu32 "\n", to_bits(adv[i]), to_bits(ret[i]));
        return 0;
    }
    fprintf(stderr, "%s: the first token is 0 (the walk) or 1 (the fold)\n", argv[0]);
    return 2;
}
