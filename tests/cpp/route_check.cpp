// route_check.cpp -- replays tests/golden/launch_routes.txt over the route functions (csrc/route.h): for every row read
// from stdin it prints the row's inputs, " | ", and what the routes decide, in the golden file's own format.
// tests/test_launch_routes.py compares the two.  A spatial row gets two fields more: hk=<spatial_handle_kind over the
// row's region, one pass>/<the kind the row's handles would be>; a fused primary + RIS row that names a kernel one:
// gb=<kernel>,<LDS bytes>,<grid>,<block>,<map2d>,<xcd_rows>,<xcd_cols> of the route over a cached G-buffer (Ask::gbuf_cached).
//
// Plain host C++ over the header alone (built by romis_amd/build.py as tools/route_check).
#include "ris_members.h"
#include "route.h"

#include <iostream>
#include <string>

#include "route_rows.h"

using namespace romis;
using namespace route_rows;

namespace {
enum Ptr : uint32_t {   // the golden file's ptrs bits
    pNt = 1u << 0, pPm = 1u << 1, pNt2 = 1u << 2, pIa = 1u << 3, pIb = 1u << 4, pOa = 1u << 5, pOb = 1u << 6, pDbg = 1u << 7,
    pRpi = 1u << 8, pRpn = 1u << 9, pRpo = 1u << 10, pVis = 1u << 11, pMtf = 1u << 12, pHiw = 1u << 13, pHim = 1u << 14,
    pHow = 1u << 15, pHom = 1u << 16, pRgb = 1u << 17, pPa = 1u << 18, pPb = 1u << 19, pThw = 1u << 20, pThm = 1u << 21,
};

// the kernel a route names (the RIS families: ris_members.h)
std::string kernel_name(const Route& r) {
    const std::string n = std::to_string(r.n), lds = r.staged ? "_lds" : "", dbg = r.dbg ? "_dbg" : "", t2 = r.th == 2 ? "_t2" : "";
    switch (r.kernel) {
    case Kernel::kNone: return "-";
    case Kernel::kPrimary: return "k_primary" + lds;
    case Kernel::kSpatial: return "k_spatial_n" + n + (r.unbiased ? "_unbiased" : "_biased");
    case Kernel::kSpatial1u: return std::string("k_spatial1u") + (r.vis_kernel ? "_vis" : "") + dbg;
    case Kernel::kSpatial1Ntl: return "k_spatial1_ntl" + t2 + dbg;
    case Kernel::kSpatial1g: return "k_spatial1g_t2" + dbg;
    case Kernel::kSpatial1hg: return "k_spatial1hg_t2" + dbg;
    case Kernel::kSpatial1hgFinal: return "k_spatial1hg_t2_final";
    case Kernel::kSpatial1h: return "k_spatial1h" + t2 + dbg;
    case Kernel::kSpatial2Ntl: return "k_spatial2_ntl" + dbg;
    case Kernel::kSpatial2hg: return "k_spatial2hg" + t2 + dbg;
    case Kernel::kFinal: return "k_final_n" + n + lds;
    case Kernel::kFinalSorted: return "k_final_n" + n + "_sorted";
    case Kernel::kFinalSortedQ: return "k_final_n" + n + "_sorted_q";
    default: return ris_kernel_name(r);
    }
}

bool handle_kernel(Kernel k) {
    return k == Kernel::kSpatial2hg || k == Kernel::kSpatial1g || k == Kernel::kSpatial1hg || k == Kernel::kSpatial1hgFinal ||
           k == Kernel::kSpatial1h;
}
}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        Row row;
        if (!parse(line.c_str(), row)) continue;
        const SceneDev& s = row.s;
        const FeaturesDev& f = row.f;
        const Tuning& tu = row.tu;
        const uint32_t a = row.ask;
        std::printf("%s", line.substr(0, line.find(" | ")).c_str());
        Ask ask;
        ask.dbg = a & kDbg;
        // the kind the frame paths would name for this scene's handles
        const int kind = f.N == 2 ? 2 : s.light_types == 1u ? 0 : 1;
        ask.hin = (a & kHin) ? kind : -1;
        ask.hout = a & kHout; ask.hout_dead = a & kHrd;
        ask.rp_in = a & kRpi; ask.rp_nb = a & kRpn; ask.rp_out = a & kRpo;
        ask.vis = a & kVis;
        ask.flags = a & kMtf; ask.flags_m = row.mt_m; ask.gbuf = row.mt_gbuf; ask.skip = row.skip_res;
        ask.fin = a & kFin; ask.fin_dead = a & kFrd;
        if (row.stage == "pred") {
            Ask flags;
            flags.flags = true;
            std::printf(" | srf=%d frf=%d prf=%d prtf=%d hk=%d\n", route_spatial(s, row.rg, f, tu, flags).bg_known,
                        route_final(s, row.rg, f, tu, flags).flags, route_primary_ris(s, row.rg, f, tu, Ask{}).ok,
                        route_primary_ris_temporal(s, row.rg, f, tu, Ask{}).ok,
                        spatial_handle_kind(s, row.rg, f, tu, row.passes, row.m0));
            continue;
        }
        Route r;
        uint32_t ptrs = pNt | pPm;
        std::string words, cached;
        bool mt = false;
        if (row.stage == "primary") {
            r = route_primary(s, row.rg, tu);
            ptrs |= (a & kNt2) ? pNt2 : 0;
        } else if (row.stage == "ris") {
            r = route_ris(s, row.rg, f, tu, ask);
            ptrs |= pOa | pOb | (r.dbg ? pDbg : 0) | (r.rp_out ? pRpo : 0);
        } else if (row.stage == "pris" || row.stage == "prist") {
            const bool temporal = row.stage == "prist";
            r = temporal ? route_primary_ris_temporal(s, row.rg, f, tu, ask) : route_primary_ris(s, row.rg, f, tu, ask);
            ptrs |= pOa | pOb | ((a & kNt2) ? pNt2 : 0) | (r.dbg ? pDbg : 0) | (r.rp_out ? pRpo : 0) | (r.flags ? pMtf : 0) |
                    (r.how ? pHow : 0) | (r.hom ? pHom : 0);
            if (temporal) ptrs |= pPa | pPb | ((a & kThw) ? pThw | pThm : 0);
            words = std::to_string(r.mode) + (temporal ? "" : "," + std::to_string(r.skip)) + "," + std::to_string(r.res_dead);
            if (r.ok && r.kernel != Kernel::kNone) {
                ask.gbuf_cached = true;
                const Route g = (temporal ? route_primary_ris_temporal : route_primary_ris)(s, row.rg, f, tu, ask);
                cached = " gb=" + kernel_name(g) + "," + std::to_string(g.lds);
                for (uint32_t v : {g.grid, g.block, g.map2d, g.xcd_rows, g.xcd_cols}) cached += "," + std::to_string(v);
            }
        } else if (row.stage == "spatial") {
            r = route_spatial(s, row.rg, f, tu, ask);
            ptrs |= pOa | pOb | (r.res_in ? pIa | pIb : 0) | (r.dbg ? pDbg : 0) | (r.rp_in ? pRpi : 0) | (r.rp_nb ? pRpn : 0) |
                    (r.rp_out ? pRpo : 0) | (r.vis ? pVis : 0) | (r.flags ? pMtf : 0) | (r.hin >= 0 ? pHiw : 0) |
                    (r.hin_m ? pHim : 0) | (r.how ? pHow : 0) | (r.hom ? pHom : 0) | (r.final_done ? pRgb : 0);
            if (r.kernel == Kernel::kSpatial) words = std::to_string(r.bvh_lds);
            if (handle_kernel(r.kernel)) words = std::to_string(r.res_dead);
            mt = r.kernel != Kernel::kSpatial;
        } else if (row.stage == "final") {
            r = route_final(s, row.rg, f, tu, ask);
            ptrs |= pIa | pIb | pRgb | (r.vis ? pVis : 0) | (r.flags ? pMtf : 0);
            mt = r.kernel != Kernel::kFinal;
        } else {
            std::fprintf(stderr, "unknown stage: %s\n", line.c_str());
            return 1;
        }
        if (r.kernel == Kernel::kNone) {
            std::printf(" | - 0 0 0 none 0000");
        } else {
            std::printf(" | %s %u %u %zu launch %d%d%d%d map=%u,%u,%u ptrs=%x u=%s", kernel_name(r).c_str(), r.grid, r.block,
                        r.lds, row.stage == "pris" && r.flags, row.stage == "spatial" && r.rp_out,
                        row.stage == "spatial" && r.vis, r.final_done, r.map2d, r.xcd_rows, r.xcd_cols, ptrs, words.c_str());
            if (mt) std::printf(" mt=%u,%u", r.flags_m, r.gbuf);
            // the sorted kernels get the scene with the miss shortcut switched off where final.miss is
            if (row.stage == "final") std::printf(" msz=%u", r.kernel == Kernel::kFinal || r.miss ? s.miss_shade_zero : 0u);
            if (r.final_done) std::printf(" fo=%u", r.miss);
        }
        if (row.stage == "spatial") std::printf(" hk=%d/%d", spatial_handle_kind(s, row.rg, f, tu, 1u), kind);
        if (row.stage == "pris" || row.stage == "prist") std::printf(" ok=%d%s", r.ok, cached.c_str());
        std::printf("\n");
    }
    return 0;
}
