// The __host__ side of active-gym_amd/csrc/agx_vtrace_math.h - the very function k_vtrace folds every step with - on host arrays.
//
//     vtrace_harness <file>            the tokens below, whitespace separated, read from a file
//     vtrace_harness <token> ...       ... or given as arguments
//
// tokens:  N L gamma_bits lambda_bits rho_bar_bits c_bar_bits pg_rho_bar_bits has_boot, len[N], reward_bits[L*N], ends[L*N],
//          value_bits[L*N], rho_bits[L*N] and, with has_boot, boot_bits[L*N] (slots [t][n]).  Per slot, in [t][n] order, one line
//          "vs_bits pg_adv_bits".  Floats travel as the decimal value of their 32-bit pattern.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "agx_vtrace_math.h"

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
    const int32_t N = (int32_t)next(), L = (int32_t)next();
    agx::VtraceCoef c;
    c.gamma = from_bits((uint32_t)next());
    c.lambda = from_bits((uint32_t)next());
    c.rho_bar = from_bits((uint32_t)next());
    c.c_bar = from_bits((uint32_t)next());
    c.pg_rho_bar = from_bits((uint32_t)next());
    const bool has_boot = next() != 0;
    if (short_input || N <= 0 || L < 1 || L > agx::kVtraceLimit) {
        fprintf(stderr,
                "usage: %s <file> | N L gamma_bits lambda_bits rho_bar_bits c_bar_bits pg_rho_bar_bits has_boot len[N] reward_bits[L*N] "
                "ends[L*N] value_bits[L*N] rho_bits[L*N] [boot_bits[L*N]]\n",
                argv[0]);
        return 2;
    }
    const size_t slots = (size_t)L * N;
    std::vector<int32_t> len(N);
    std::vector<float> reward(slots), value(slots), rho(slots), boot(has_boot ? slots : 0), vs(slots), pg(slots);
    std::vector<uint8_t> ends(slots);
    for (auto &v : len) v = (int32_t)next();
    for (auto &v : reward) v = from_bits((uint32_t)next());
    for (auto &v : ends) v = (uint8_t)next();
    for (auto &v : value) v = from_bits((uint32_t)next());
    for (auto &v : rho) v = from_bits((uint32_t)next());
    for (auto &v : boot) v = from_bits((uint32_t)next());
    if (short_input || at != tok.size()) {
        fprintf(stderr, "%s: the arrays are incomplete or over-long\n", argv[0]);
        return 2;
    }
    for (int32_t n = 0; n < N; ++n)
        agx::vtrace_fold([&](int32_t t) { return (size_t)t * N + n; }, L, len[n], reward.data(), ends.data(), value.data(),
                         has_boot ? boot.data() : nullptr, rho.data(), c, vs.data(), pg.data());
    for (size_t i = 0; i < slots; ++i) printf("%" PRIu32 " %" PRIu32 "\n", to_bits(vs[i]), to_bits(pg[i]));
    return 0;
}
