// The __host__ side of active-gym_amd/csrc/agx_vtrace_math.h - the very function k_slot_fold<VtraceFold> folds every step with - on
// host arrays.
//
//     vtrace_harness <file>            the tokens below, whitespace separated, read from a file
//     vtrace_harness <token> ...       ... or given as arguments
//
// tokens:  N L gamma_bits lambda_bits rho_bar_bits c_bar_bits pg_rho_bar_bits has_boot, len[N], reward_bits[L*N], ends[L*N],
//          value_bits[L*N], rho_bits[L*N] and, with has_boot, boot_bits[L*N] (slots [t][n]).  Per slot, in [t][n] order, one line
//          "vs_bits pg_adv_bits".  Floats travel as the decimal value of their 32-bit pattern.
#include <cinttypes>
#include <cstdio>

#include "agx_vtrace_math.h"
#include "harness_tokens.h"

int main(int argc, char **argv) {
    Tokens in;
    if (!in.read(argc, argv)) return 2;
    const int32_t N = (int32_t)in.next(), L = (int32_t)in.next();
    agx::VtraceCoef c;
    c.gamma = in.next_float();
    c.lambda = in.next_float();
    c.rho_bar = in.next_float();
    c.c_bar = in.next_float();
    c.pg_rho_bar = in.next_float();
    const bool has_boot = in.next() != 0;
    if (in.short_input || N <= 0 || L < 1 || L > agx::kVtraceLimit) {
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
    for (auto &v : len) v = (int32_t)in.next();
    for (auto &v : reward) v = in.next_float();
    for (auto &v : ends) v = (uint8_t)in.next();
    for (auto &v : value) v = in.next_float();
    for (auto &v : rho) v = in.next_float();
    for (auto &v : boot) v = in.next_float();
    if (!in.complete()) {
        fprintf(stderr, "%s: the arrays are incomplete or over-long\n", argv[0]);
        return 2;
    }
    for (int32_t n = 0; n < N; ++n)
        agx::vtrace_fold([&](int32_t t) { return (size_t)t * N + n; }, L, len[n], reward.data(), ends.data(), value.data(),
                         has_boot ? boot.data() : nullptr, rho.data(), c, vs.data(), pg.data());
    for (size_t i = 0; i < slots; ++i) printf("%" PRIu32 " %" PRIu32 "\n", to_bits(vs[i]), to_bits(pg[i]));
    return 0;
}
