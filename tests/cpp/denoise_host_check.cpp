// denoise_host_check -- restir_denoise_host as a stand-alone program: csrc/denoise_host.cpp and csrc/abi_error.cpp alone,
// no HIP, no library.  tests/test_denoise_host.py builds it with -fsanitize=address,undefined and runs it on ragged
// sizes: every read of the filter -- the taps at the image's border at every step, the guides, the two scratch images --
// then happens under the sanitizers, with the input and output arrays allocated at their exact sizes.
//
//     denoise_host_check <w> <h> <iterations> <normal_power_log2>
//
// The inputs come from a 32-bit LCG (the test regenerates them): a wavy height field with three materials, some misses,
// a zero and a NaN normal, one NaN and one inf colour.  Prints "hash <fnv1a-64 of the output's bytes> nonfinite <count>".
#include "restir_c.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct Lcg {
    uint32_t x;
    float next() {   // [0, 1), 24 bits
        x = x * 1664525u + 1013904223u;
        return (float)(x >> 8) * (1.0f / 16777216.0f);
    }
};

float bits_float(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: denoise_host_check w h iterations normal_power_log2\n");
        return 2;
    }
    const uint32_t w = (uint32_t)std::atoi(argv[1]), h = (uint32_t)std::atoi(argv[2]);
    restir_denoise_params p;
    restir_denoise_params_default(&p);
    p.iterations = (uint32_t)std::atoi(argv[3]);
    p.normal_power_log2 = (uint32_t)std::atoi(argv[4]);
    const size_t npx = (size_t)w * h;
    const uint32_t miss = 3;
    std::vector<float> rgb(3 * npx), n_t(4 * npx), p_mat(4 * npx), out(3 * npx);
    Lcg g{w * 7919u + h};
    for (size_t i = 0; i < npx; i++) {
        const float x = (float)(i % w), y = (float)(i / w);
        n_t[4 * i + 0] = g.next() - 0.5f;
        n_t[4 * i + 1] = g.next() - 0.5f;
        n_t[4 * i + 2] = 1.0f + g.next();
        n_t[4 * i + 3] = 4.0f + g.next();
        p_mat[4 * i + 0] = 0.05f * x;
        p_mat[4 * i + 1] = 0.05f * y;
        p_mat[4 * i + 2] = 0.02f * g.next();
        const float m = g.next();
        p_mat[4 * i + 3] = bits_float(m < 0.1f ? miss : (uint32_t)(x * 3.0f / (float)w));
        for (int j = 0; j < 3; j++) rgb[3 * i + j] = 4.0f * g.next();
    }
    if (npx > 4) {
        n_t[4 * 1 + 0] = n_t[4 * 1 + 1] = n_t[4 * 1 + 2] = 0.0f;   // a normal without a direction
        n_t[4 * 2 + 1] = NAN;
        rgb[3 * 3 + 1] = NAN;
        rgb[3 * (npx - 1) + 2] = INFINITY;
    }
    const restir_status st = restir_denoise_host(rgb.data(), n_t.data(), p_mat.data(), w, h, miss, &p, out.data());
    if (st != RESTIR_OK) {
        std::fprintf(stderr, "restir_denoise_host: %d: %s\n", (int)st, restir_last_error());
        return 1;
    }
    uint64_t hash = 1469598103934665603ull;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(out.data());
    for (size_t i = 0; i < out.size() * 4; i++) hash = (hash ^ b[i]) * 1099511628211ull;
    size_t bad = 0;
    for (float v : out) bad += std::isfinite(v) ? 0 : 1;
    std::printf("hash %016llx nonfinite %zu\n", (unsigned long long)hash, bad);
    // the argument checks, under the sanitizers too
    restir_denoise_params q = p;
    q.iterations = 6;
    if (restir_denoise_host(rgb.data(), n_t.data(), p_mat.data(), w, h, miss, &q, out.data()) != RESTIR_ERR_INVALID) return 3;
    if (restir_denoise_host(nullptr, n_t.data(), p_mat.data(), w, h, miss, &p, out.data()) != RESTIR_ERR_INVALID) return 3;
    return 0;
}
