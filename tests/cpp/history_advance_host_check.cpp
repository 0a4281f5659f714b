// history_advance_host_check -- restir_history_advance_host as a stand-alone program: csrc/history_host.cpp,
// csrc/denoise_host.cpp and csrc/abi_error.cpp alone, no HIP, no library.  tests/test_history_bilinear_host.py builds it
// with -fsanitize=address,undefined and runs it on ragged sizes in both gather modes: the 2 x 2 taps at and beyond the
// image's border, the row flips between G-buffer and image rows and the optional map then happen under the sanitizers,
// with every array allocated at its exact size.
//
//     history_advance_host_check <w> <h> <max_frames>
//
// The inputs are tests/cpp/history_host_check.cpp's, from the same 32-bit LCG (the test regenerates them).  Prints
// "nearest <fnv1a-64 of mean, S, n, map> bilinear <the same>".
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

uint64_t fnv(uint64_t hash, const void* p, size_t bytes) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < bytes; i++) hash = (hash ^ b[i]) * 1099511628211ull;
    return hash;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: history_advance_host_check w h max_frames\n");
        return 2;
    }
    const uint32_t w = (uint32_t)std::atoi(argv[1]), h = (uint32_t)std::atoi(argv[2]), cap = (uint32_t)std::atoi(argv[3]);
    const size_t npx = (size_t)w * h;
    const uint32_t miss = 3;
    std::vector<float> n_t(4 * npx), p_mat(4 * npx), mean(3 * npx), S(3 * npx), x(3 * npx);
    std::vector<uint32_t> n(npx), mat(npx);
    Lcg g{w * 7919u + h};
    for (size_t i = 0; i < npx; i++) {
        const float cx = (float)(i % w), cy = (float)(i / w);
        n_t[4 * i + 0] = g.next() - 0.5f;
        n_t[4 * i + 1] = g.next() - 0.5f;
        n_t[4 * i + 2] = 1.0f + g.next();
        n_t[4 * i + 3] = 4.0f + g.next();
        p_mat[4 * i + 0] = 0.05f * cx;
        p_mat[4 * i + 1] = 0.05f * cy;
        p_mat[4 * i + 2] = 0.02f * g.next();
        mat[i] = g.next() < 0.1f ? miss : (uint32_t)(cx * 3.0f / (float)w);
        p_mat[4 * i + 3] = bits_float(mat[i]);
        for (int j = 0; j < 3; j++) {
            mean[3 * i + j] = 4.0f * g.next();
            S[3 * i + j] = g.next();
            x[3 * i + j] = 4.0f * g.next();
        }
        n[i] = (uint32_t)(g.next() * 6.0f);
        if (!(g.next() < 0.25f)) g.next();   // history_host_check's map entry: the stream stays the same
    }
    if (npx > 4) {
        x[3 * 3 + 1] = NAN;
        x[3 * (npx - 1) + 2] = INFINITY;
    }
    // a fixed camera in front of the height field (tests/test_history_host.py CHECK_CAMERA)
    restir_camera_frame cf{};
    cf.origin[0] = 0.1f; cf.origin[1] = 0.2f; cf.origin[2] = -3.0f;
    cf.quat[0] = 0.05f; cf.quat[1] = -0.1f; cf.quat[2] = 0.02f; cf.quat[3] = 0.99f;
    cf.half_w = 0.3f; cf.half_h = 0.2f;
    const uint64_t seed = 1469598103934665603ull;
    uint64_t hashes[2];
    std::vector<float> mo(3 * npx), so(3 * npx);
    std::vector<uint32_t> no(npx), smap(npx);
    for (uint32_t gather = 0; gather < 2; gather++) {
        const restir_status st =
            restir_history_advance_host(&cf, w, h, n_t.data(), p_mat.data(), n_t.data(), mat.data(), mean.data(), S.data(), n.data(),
                                        x.data(), miss, cap, gather, mo.data(), so.data(), no.data(), smap.data());
        if (st != RESTIR_OK) {
            std::fprintf(stderr, "restir_history_advance_host(%u): %d: %s\n", gather, (int)st, restir_last_error());
            return 1;
        }
        uint64_t hf = fnv(seed, mo.data(), mo.size() * 4);
        hf = fnv(hf, so.data(), so.size() * 4);
        hf = fnv(hf, no.data(), no.size() * 4);
        hashes[gather] = fnv(hf, smap.data(), smap.size() * 4);
        // without the map, and with nothing kept
        if (restir_history_advance_host(&cf, w, h, n_t.data(), p_mat.data(), n_t.data(), mat.data(), mean.data(), S.data(), n.data(),
                                        x.data(), miss, cap, gather, mo.data(), so.data(), no.data(), nullptr) != RESTIR_OK)
            return 1;
        if (restir_history_advance_host(&cf, w, h, n_t.data(), p_mat.data(), nullptr, nullptr, mean.data(), S.data(), n.data(),
                                        x.data(), miss, cap, gather, mo.data(), so.data(), no.data(), smap.data()) != RESTIR_OK)
            return 1;
        for (size_t i = 0; i < npx; i++)
            if (smap[i] != 0xFFFFFFFFu - 7u) return 4;
    }
    std::printf("nearest %016llx bilinear %016llx\n", (unsigned long long)hashes[0], (unsigned long long)hashes[1]);
    // the argument checks, under the sanitizers too
    if (restir_history_advance_host(&cf, w, h, n_t.data(), p_mat.data(), n_t.data(), nullptr, mean.data(), S.data(), n.data(), x.data(),
                                    miss, cap, 1, mo.data(), so.data(), no.data(), smap.data()) != RESTIR_ERR_INVALID)
        return 3;
    if (restir_history_advance_host(&cf, w, h, n_t.data(), p_mat.data(), n_t.data(), mat.data(), mean.data(), S.data(), n.data(), x.data(),
                                    miss, cap, 2, mo.data(), so.data(), no.data(), smap.data()) != RESTIR_ERR_INVALID)
        return 3;
    n[0] = 1u << 24;
    if (restir_history_advance_host(&cf, w, h, n_t.data(), p_mat.data(), n_t.data(), mat.data(), mean.data(), S.data(), n.data(), x.data(),
                                    miss, cap, 1, mo.data(), so.data(), no.data(), smap.data()) != RESTIR_ERR_INVALID)
        return 3;
    return 0;
}
