// ris_members.h -- the members of the three RIS kernel families (ris_pixel unfused: k_ris_*, fused with the primary
// rays: k_primary_ris_*, over a cached G-buffer: k_gbuf_ris_*), listed once.  kernels.hip expands the list into each
// family's kernels and its table of kernel pointers, which the launchers index through ris_member; the name printed for
// a route (tests/cpp/route_check.cpp) is the same suffix token stringized.  Host only: no kernel symbols.
#pragma once

#include <string>

#include "route.h"

// A row: the family's prefix P as passed in, N (0: the any-N kernel), the light table staged in LDS, its form (ris_pixel's
// LT) and the name suffix as one token: the kernel is P##suffix.  X5: the three rows whose unfused kernel keeps the N = 2
// cap on waves per SIMD (kernels.hip, ROMIS_RIS_WPE).  No regular grid but at N = 1, no compact form at N = 0.
#define ROMIS_RIS_MEMBERS(X, X5, P)          \
    X(P, 1, false, kLtGeneral, n1)           \
    X(P, 2, false, kLtGeneral, n2)           \
    X(P, 0, false, kLtGeneral, n0)           \
    X(P, 1, true, kLtGeneral, n1_lds)        \
    X(P, 2, true, kLtGeneral, n2_lds)        \
    X(P, 0, true, kLtGeneral, n0_lds)        \
    X(P, 1, false, kLtPoint, n1_pt)          \
    X(P, 2, false, kLtPoint, n2_pt)          \
    X(P, 1, true, kLtPoint, n1_lds_pt)       \
    X(P, 2, true, kLtPoint, n2_lds_pt)       \
    X(P, 1, false, kLtGrid, n1_grid)         \
    X(P, 2, false, kLtGrid, n2_grid)         \
    X5(P, 1, true, kLtGrid, n1_lds_grid)     \
    X(P, 2, true, kLtGrid, n2_lds_grid)      \
    X(P, 1, false, kLtPgram, n1_pg)          \
    X(P, 2, false, kLtPgram, n2_pg)          \
    X5(P, 1, true, kLtPgram, n1_lds_pg)      \
    X(P, 2, true, kLtPgram, n2_lds_pg)       \
    X(P, 1, false, kLtRegular, n1_reg)       \
    X5(P, 1, true, kLtRegular, n1_lds_reg)
// ... with temporal reuse in the same kernel (the fused and the cached family)
#define ROMIS_RIS_TEMPORAL_MEMBERS(X, P) X(P, 1, true, kLtPoint, n1_lds_pt_temporal) X(P, 2, true, kLtPoint, n2_lds_pt_temporal)

namespace romis {

struct RisMember { uint32_t n; bool staged; int lt; const char* suffix; };
#define ROMIS_RIS_ROW(P, N, LDS, LT, SUFFIX) {N, LDS, LT, #SUFFIX},
constexpr RisMember kRisList[] = {ROMIS_RIS_MEMBERS(ROMIS_RIS_ROW, ROMIS_RIS_ROW, )};
constexpr RisMember kRisTemporalList[] = {ROMIS_RIS_TEMPORAL_MEMBERS(ROMIS_RIS_ROW, )};
constexpr int kRisMembers = sizeof(kRisList) / sizeof(kRisList[0]);
constexpr int kRisTemporalMembers = sizeof(kRisTemporalList) / sizeof(kRisTemporalList[0]);

// The member's index in list order (temporal: in the temporal list); -1: the families have no such member
constexpr int ris_member(uint32_t n, bool staged, int lt, bool temporal = false) {
    const RisMember* const list = temporal ? kRisTemporalList : kRisList;
    for (int i = 0; i < (temporal ? kRisTemporalMembers : kRisMembers); i++)
        if (list[i].n == n && list[i].staged == staged && list[i].lt == lt) return i;
    return -1;
}

// The kernel a route of a RIS family names ("?": none)
inline std::string ris_kernel_name(const Route& r) {
    const bool temporal = r.kernel == Kernel::kPrimaryRisTemporal || r.kernel == Kernel::kGbufRisTemporal;
    const int m = ris_member(r.n, r.staged, r.lt, temporal);
    if (m < 0) return "?";
    const char* const suffix = (temporal ? kRisTemporalList : kRisList)[m].suffix;
    switch (r.kernel) {
    case Kernel::kRis: return std::string("k_ris_") + suffix;
    case Kernel::kPrimaryRis: case Kernel::kPrimaryRisTemporal: return std::string("k_primary_ris_") + suffix;
    case Kernel::kGbufRis: case Kernel::kGbufRisTemporal: return std::string("k_gbuf_ris_") + suffix;
    default: return "?";
    }
}

}  // namespace romis
