// route_rows.h -- the input half of a row of tests/golden/launch_routes.txt, shared by the recorder that wrote the file
// from the launchers and by the program that replays it over route.h (tests/cpp/route_check.cpp).
//
//   <stage> <num_lights>,<light_types>,<grid>,<pgram>,<regular>,<miss_shade_zero> <num_nodes>,<num_tris>,<nodes_q_ok>
//           <N>,<K>,<R>,<unbiased>,<spatial_vis>,<M> <vw>,<vh>,<rw>,<rh>,<ps>,<js> <ask bits, hex>
//           <MissTiles m>,<gbuf>,<skip_res> <passes>,<m0> <knob>:<value>[:<value>] | <outputs>
//
// stage: primary ris pris prist spatial final pred.  Knob "-": the defaults; "xcd": spatial.xcd_rows : spatial.xcd_cols.
// Any other group written "-" takes its default: 32 point lights (32,1,0,0,0,1), a BVH of 12.5 KB (100,200,1), N = 1,
// K = 5, R = 10, biased, M = 32 (1,5,10,0,0,32), a whole 1920 x 1080 view in planes (1920,1080,1920,1080,1,2073600),
// nothing asked (0), 0,0,0 and 1,0.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "restir_types.h"

namespace route_rows {

enum AskBit : uint32_t {
    kDbg = 1u << 0,    // debug plane
    kHin = 1u << 1,    // input handles
    kHout = 1u << 2,   // output handles
    kHrd = 1u << 3,    // ... whose res_dead is set
    kRpi = 1u << 4,    // pdf cache in (own pixel)
    kRpn = 1u << 5,    // pdf cache in (neighbours)
    kRpo = 1u << 6,    // pdf cache out
    kVis = 1u << 7,    // own-pixel ray plane (the pass's out, final shading's in)
    kMtf = 1u << 8,    // tile flags
    kFin = 1u << 9,    // fused final offered
    kFrd = 1u << 10,   // ... with dead reservoirs
    kNt2 = 1u << 11,   // second G-buffer copy
    kThw = 1u << 12,   // the temporal predecessor's handles
};

struct Row {
    std::string stage, knob;
    romis::SceneDev s{};
    romis::FeaturesDev f{};
    romis::Region rg{};
    romis::Tuning tu{};
    uint32_t ask = 0, mt_m = 0, mt_gbuf = 0, skip_res = 0, passes = 0;
    unsigned long long m0 = 0;
};

inline bool set_knob(romis::Tuning& t, const std::string& k, uint32_t v, uint32_t v2) {
    if (k == "-") return true;
    if (k == "xcd") { t.spatial_xcd_rows = v; t.spatial_xcd_cols = v2; return true; }
    struct { const char* name; uint32_t romis::Tuning::*field; } const tab[] = {
        {"spatial.lean", &romis::Tuning::spatial_lean}, {"spatial.th", &romis::Tuning::spatial_th},
        {"spatial.gather", &romis::Tuning::spatial_gather}, {"spatial.handles", &romis::Tuning::spatial_handles},
        {"spatial.n2h", &romis::Tuning::spatial_n2h}, {"ris.compact", &romis::Tuning::ris_compact},
        {"ris.lds", &romis::Tuning::ris_lds}, {"ris.late", &romis::Tuning::ris_late},
        {"primary.lds", &romis::Tuning::primary_lds}, {"primary.tl", &romis::Tuning::primary_tl},
        {"final.sort", &romis::Tuning::final_sort}, {"final.lds", &romis::Tuning::final_lds},
        {"final.qbvh", &romis::Tuning::final_qbvh}, {"final.fuse", &romis::Tuning::final_fuse},
        {"final.miss", &romis::Tuning::final_miss}, {"fuse.temporal", &romis::Tuning::fuse_temporal},
    };
    for (const auto& e : tab)
        if (k == e.name) { t.*e.field = v; return true; }
    return false;
}

// parses the part of `line` before " | "; false for comments, blank lines and malformed rows
inline bool parse(const char* line, Row& r) {
    static const char* const kDefault[8] = {"32,1,0,0,0,1", "100,200,1", "1,5,10,0,0,32", "1920,1080,1920,1080,1,2073600", "0",
                                            "0,0,0", "1,0", "-"};
    char stage[16], g[8][64], knob[64];
    if (line[0] == '#' || std::sscanf(line, "%15s %63s %63s %63s %63s %63s %63s %63s %63s", stage, g[0], g[1], g[2], g[3], g[4],
                                      g[5], g[6], g[7]) != 9)
        return false;
    std::string full;
    for (int i = 0; i < 8; i++) full += std::string(std::strcmp(g[i], "-") ? g[i] : kDefault[i]) + " ";
    unsigned nl, lt, lg, lpg, lreg, msz, nn, nt, qok, N, K, R, ub, sv, M, vw, vh, rw, rh, ps, js, ask, mtm, mtg, skip, passes;
    unsigned long long m0;
    if (std::sscanf(full.c_str(), "%u,%u,%u,%u,%u,%u %u,%u,%u %u,%u,%u,%u,%u,%u %u,%u,%u,%u,%u,%u %x %u,%u,%u %u,%llu %63s", &nl,
                    &lt, &lg, &lpg, &lreg, &msz, &nn, &nt, &qok, &N, &K, &R, &ub, &sv, &M, &vw, &vh, &rw, &rh, &ps, &js, &ask,
                    &mtm, &mtg, &skip, &passes, &m0, knob) != 28)
        return false;
    r = Row{};
    r.stage = stage;
    r.s.num_lights = nl; r.s.light_types = lt; r.s.lights_grid = lg; r.s.lights_pgram = lpg; r.s.lights_regular = lreg;
    r.s.miss_shade_zero = msz; r.s.num_nodes = nn; r.s.num_tris = nt; r.s.nodes_q_ok = qok;
    r.f.N = N; r.f.K = K; r.f.R = R; r.f.unbiased = ub; r.f.spatial_vis = sv; r.f.M = M;
    r.rg.W = vw; r.rg.H = vh; r.rg.vw = vw; r.rg.vh = vh; r.rg.rw = rw; r.rg.rh = rh; r.rg.ps = ps; r.rg.js = js;
    r.ask = ask; r.mt_m = mtm; r.mt_gbuf = mtg; r.skip_res = skip; r.passes = passes; r.m0 = m0;
    unsigned v = 0, v2 = 0;
    char* colon = std::strchr(knob, ':');
    if (colon) { *colon = 0; std::sscanf(colon + 1, "%u:%u", &v, &v2); }
    r.knob = knob;
    return set_knob(r.tu, r.knob, v, v2);
}

}  // namespace route_rows
