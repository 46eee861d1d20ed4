// What the *_harness.cpp programs next to this file share: their input is whitespace-separated decimal tokens, read from a file
// (one argument) or given as the arguments themselves, and floats travel as the decimal value of their 32-bit pattern.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

inline float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}
inline uint32_t to_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

struct Tokens {
    std::vector<std::string> tok;
    size_t at = 0;
    bool short_input = false;          // next() was asked for more than there is

    // false: the file of a one-argument call cannot be opened (said on stderr; the caller exits with 2)
    bool read(int argc, char **argv) {
        if (argc == 2) {
            FILE *f = fopen(argv[1], "r");
            if (!f) {
                fprintf(stderr, "cannot open %s\n", argv[1]);
                return false;
            }
            char buf[64];
            while (fscanf(f, "%63s", buf) == 1) tok.emplace_back(buf);
            fclose(f);
        } else {
            for (int i = 1; i < argc; ++i) tok.emplace_back(argv[i]);
        }
        return true;
    }
    int64_t next() {
        if (at >= tok.size()) {
            short_input = true;
            return 0;
        }
        return strtoll(tok[at++].c_str(), nullptr, 10);
    }
    float next_float() { return from_bits((uint32_t)next()); }
    size_t left() const { return tok.size() - at; }
    bool complete() const { return !short_input && left() == 0; }       // every array was there and nothing is behind them
};
