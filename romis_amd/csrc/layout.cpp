// layout.cpp -- tile layouts and halo plans: every restir_layout_* / restir_tile_plan / restir_halo_plan / restir_*halo_ops entry
// (C ABI of include/restir_c.h).  No device call: plain C++.
#include "abi_error.h"
#include "layout.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

using namespace romis;

namespace romis {

// a layout's cuts are well formed: every column and every row of a column at least one pixel, the ends at the image
restir_status layout_check(const restir_tile_layout* L) {
    if (!L) return fail(RESTIR_ERR_INVALID, "tile layout is NULL");
    const uint32_t tx = L->tiles_x, ty = L->tiles_y;
    if (L->global_width == 0 || L->global_height == 0 || tx == 0 || ty == 0 || tx > RESTIR_MAX_TILES_X ||
        ty > RESTIR_MAX_TILES_Y)
        return fail(RESTIR_ERR_INVALID, "tile layout: bad size (W=%u H=%u tiles=%ux%u, at most %ux%u)", L->global_width,
                    L->global_height, tx, ty, RESTIR_MAX_TILES_X, RESTIR_MAX_TILES_Y);
    if (L->x_cuts[0] != 0 || L->x_cuts[tx] != L->global_width)
        return fail(RESTIR_ERR_INVALID, "tile layout: x cuts must run from 0 to the width");
    for (uint32_t c = 0; c < tx; c++) {
        if (L->x_cuts[c + 1] <= L->x_cuts[c]) return fail(RESTIR_ERR_INVALID, "tile layout: x cuts not increasing at %u", c);
        if (L->y_cuts[c][0] != 0 || L->y_cuts[c][ty] != L->global_height)
            return fail(RESTIR_ERR_INVALID, "tile layout: column %u's y cuts must run from 0 to the height", c);
        for (uint32_t r = 0; r < ty; r++)
            if (L->y_cuts[c][r + 1] <= L->y_cuts[c][r])
                return fail(RESTIR_ERR_INVALID, "tile layout: column %u's y cuts not increasing at %u", c, r);
    }
    return RESTIR_OK;
}

}  // namespace romis

namespace {
// pixels of cost cell i along an axis of n pixels split into m cells: x belongs to cell floor(x m / n)
inline uint32_t cell_of(uint32_t x, uint32_t m, uint32_t n) { return (uint32_t)((uint64_t)x * m / n); }
inline uint32_t cell_begin(uint32_t i, uint32_t m, uint32_t n) { return (uint32_t)(((uint64_t)i * n + m - 1) / m); }
// pixels of [a, b) in cell i
inline uint32_t cell_overlap(uint32_t i, uint32_t m, uint32_t n, uint32_t a, uint32_t b) {
    const uint32_t c0 = std::max(cell_begin(i, m, n), a), c1 = std::min(cell_begin(i + 1, m, n), b);
    return c1 > c0 ? c1 - c0 : 0u;
}
// the cost the grid puts on the rectangle [xa, xb) x [ya, yb) (each cell's cost spread evenly over its pixels)
double rect_cost(const float* cost, uint32_t cw, uint32_t ch, uint32_t W, uint32_t H, uint32_t xa, uint32_t xb,
                 uint32_t ya, uint32_t yb) {
    double sum = 0.0;
    const uint32_t j0 = cell_of(ya, ch, H), j1 = cell_of(yb - 1, ch, H), i0 = cell_of(xa, cw, W), i1 = cell_of(xb - 1, cw, W);
    for (uint32_t j = j0; j <= j1; j++) {
        const double fy = (double)cell_overlap(j, ch, H, ya, yb) / (cell_begin(j + 1, ch, H) - cell_begin(j, ch, H));
        for (uint32_t i = i0; i <= i1; i++) {
            const double fx = (double)cell_overlap(i, cw, W, xa, xb) / (cell_begin(i + 1, cw, W) - cell_begin(i, cw, W));
            sum += (double)cost[(size_t)j * cw + i] * fx * fy;
        }
    }
    return sum;
}
// cuts c[1..parts-1] of [0, n) at the equal-share points of the per-pixel prefix cost P (P[x] = cost of [0, x)),
// rounded to multiples of `align`, every part at least `align` wide (the last takes the remainder)
void share_cuts(const std::vector<double>& P, uint32_t n, uint32_t parts, uint32_t align, uint32_t* c) {
    c[0] = 0;
    c[parts] = n;
    const double total = P[n];
    for (uint32_t k = 1; k < parts; k++) {
        const double target = total * k / parts;
        const uint32_t x = (uint32_t)(std::lower_bound(P.begin(), P.begin() + n + 1, target) - P.begin());
        uint64_t q = ((uint64_t)x + align / 2) / align * align;
        const uint64_t lo = (uint64_t)c[k - 1] + align, hi = (uint64_t)n - (uint64_t)(parts - k) * align;
        q = std::min(std::max(q, lo), hi);
        c[k] = (uint32_t)q;
    }
}
void layout_rect(const restir_tile_layout& L, uint32_t rank, uint32_t& x0, uint32_t& y0, uint32_t& w, uint32_t& h) {
    const uint32_t tx = rank % L.tiles_x, ty = rank / L.tiles_x;
    x0 = L.x_cuts[tx]; w = L.x_cuts[tx + 1] - x0;
    y0 = L.y_cuts[tx][ty]; h = L.y_cuts[tx][ty + 1] - y0;
}
}  // namespace

extern "C" {

restir_status restir_layout_even(uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t tiles_y, restir_tile_layout* out) {
    if (!out || W == 0 || H == 0 || tiles_x == 0 || tiles_y == 0 || tiles_x > W || tiles_y > H ||
        tiles_x > RESTIR_MAX_TILES_X || tiles_y > RESTIR_MAX_TILES_Y)
        return fail(RESTIR_ERR_INVALID, "restir_tile_plan: bad arguments (W=%u H=%u tiles=%ux%u)", W, H, tiles_x, tiles_y);
    restir_tile_layout L{};
    L.global_width = W; L.global_height = H; L.tiles_x = tiles_x; L.tiles_y = tiles_y;
    // even split, remainder to the first tiles (deterministic, every pixel owned exactly once)
    auto start = [](uint32_t n, uint32_t parts, uint32_t i) { return i * (n / parts) + std::min(i, n % parts); };
    for (uint32_t c = 0; c <= tiles_x; c++) L.x_cuts[c] = start(W, tiles_x, c);
    for (uint32_t c = 0; c < tiles_x; c++)
        for (uint32_t r = 0; r <= tiles_y; r++) L.y_cuts[c][r] = start(H, tiles_y, r);
    *out = L;
    return RESTIR_OK;
}

restir_status restir_layout_balanced(uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t tiles_y, const float* cost,
                                     uint32_t cw, uint32_t ch, uint32_t align_x, uint32_t align_y, restir_tile_layout* out,
                                     double* efficiency) {
    if (!out || !cost || cw == 0 || ch == 0 || cw > W || ch > H)
        return fail(RESTIR_ERR_INVALID, "restir_layout_balanced: bad cost grid (%ux%u over %ux%u)", cw, ch, W, H);
    restir_tile_layout L{};
    ST_TRY(restir_layout_even(W, H, tiles_x, tiles_y, &L));
    align_x = std::max(align_x, 1u);
    align_y = std::max(align_y, 1u);
    if ((uint64_t)tiles_x * align_x > W || (uint64_t)tiles_y * align_y > H)
        return fail(RESTIR_ERR_INVALID, "restir_layout_balanced: %ux%u tiles of at least %ux%u px do not fit %ux%u", tiles_x,
                    tiles_y, align_x, align_y, W, H);
    for (size_t i = 0; i < (size_t)cw * ch; i++)
        if (!(cost[i] >= 0.0f) || !std::isfinite(cost[i]))
            return fail(RESTIR_ERR_INVALID, "restir_layout_balanced: cost cell %zu is negative or not finite", i);
    // columns: the per-pixel-column cost (each cell's column total spread over its pixel columns), prefix-summed
    std::vector<double> colsum(cw, 0.0);
    for (uint32_t j = 0; j < ch; j++)
        for (uint32_t i = 0; i < cw; i++) colsum[i] += cost[(size_t)j * cw + i];
    std::vector<double> P(W + 1, 0.0);
    for (uint32_t x = 0; x < W; x++) {
        const uint32_t i = cell_of(x, cw, W);
        P[x + 1] = P[x] + colsum[i] / (cell_begin(i + 1, cw, W) - cell_begin(i, cw, W));
    }
    share_cuts(P, W, tiles_x, align_x, L.x_cuts);
    // each column: its own rows' cost, prefix-summed over pixel rows
    std::vector<double> Q(H + 1, 0.0), rowsum(ch);
    for (uint32_t c = 0; c < tiles_x; c++) {
        const uint32_t xa = L.x_cuts[c], xb = L.x_cuts[c + 1];
        for (uint32_t j = 0; j < ch; j++) {
            double s = 0.0;
            for (uint32_t i = cell_of(xa, cw, W); i <= cell_of(xb - 1, cw, W); i++)
                s += (double)cost[(size_t)j * cw + i] * cell_overlap(i, cw, W, xa, xb) /
                     (cell_begin(i + 1, cw, W) - cell_begin(i, cw, W));
            rowsum[j] = s;
        }
        for (uint32_t y = 0; y < H; y++) {
            const uint32_t j = cell_of(y, ch, H);
            Q[y + 1] = Q[y] + rowsum[j] / (cell_begin(j + 1, ch, H) - cell_begin(j, ch, H));
        }
        share_cuts(Q, H, tiles_y, align_y, L.y_cuts[c]);
    }
    ST_TRY(layout_check(&L));
    if (efficiency) {
        std::vector<double> sh(tiles_x * tiles_y);
        ST_TRY(restir_layout_shares(&L, cost, cw, ch, sh.data()));
        double mx = 0.0, mean = 0.0;
        for (double v : sh) { mx = std::max(mx, v); mean += v / sh.size(); }
        *efficiency = mx > 0.0 ? mean / mx : 1.0;
    }
    *out = L;
    return RESTIR_OK;
}

restir_status restir_layout_shares(const restir_tile_layout* L, const float* cost, uint32_t cw, uint32_t ch, double* out) {
    ST_TRY(layout_check(L));
    if (!cost || !out || cw == 0 || ch == 0 || cw > L->global_width || ch > L->global_height)
        return fail(RESTIR_ERR_INVALID, "restir_layout_shares: bad cost grid");
    const uint32_t n = L->tiles_x * L->tiles_y;
    double total = 0.0;
    for (uint32_t q = 0; q < n; q++) {
        uint32_t x0, y0, w, h;
        layout_rect(*L, q, x0, y0, w, h);
        out[q] = rect_cost(cost, cw, ch, L->global_width, L->global_height, x0, x0 + w, y0, y0 + h);
        total += out[q];
    }
    for (uint32_t q = 0; q < n; q++) out[q] = total > 0.0 ? out[q] / total : 1.0 / n;
    return RESTIR_OK;
}

restir_status restir_layout_tile(const restir_tile_layout* L, uint32_t rank, uint32_t ghost, restir_tile* out) {
    ST_TRY(layout_check(L));
    if (!out || rank >= L->tiles_x * L->tiles_y)
        return fail(RESTIR_ERR_INVALID, "restir_tile_plan: bad arguments (rank %u of %ux%u tiles)", rank, L->tiles_x,
                    L->tiles_y);
    const uint32_t W = L->global_width, H = L->global_height;
    restir_tile t{};
    t.global_width = W;
    t.global_height = H;
    layout_rect(*L, rank, t.x0, t.y0, t.width, t.height);
    const uint32_t gx0 = t.x0 > ghost ? t.x0 - ghost : 0u;
    const uint32_t gy0 = t.y0 > ghost ? t.y0 - ghost : 0u;
    const uint32_t gx1 = std::min<uint64_t>((uint64_t)t.x0 + t.width + ghost, W);
    const uint32_t gy1 = std::min<uint64_t>((uint64_t)t.y0 + t.height + ghost, H);
    t.gx0 = gx0; t.gy0 = gy0; t.gwidth = gx1 - gx0; t.gheight = gy1 - gy0;
    *out = t;
    return RESTIR_OK;
}

restir_status restir_tile_plan(uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t tiles_y, uint32_t rank, uint32_t ghost,
                               restir_tile* out) {
    restir_tile_layout L;
    if (!out || rank >= tiles_x * tiles_y)
        return fail(RESTIR_ERR_INVALID, "restir_tile_plan: bad arguments (W=%u H=%u tiles=%ux%u rank=%u)", W, H, tiles_x,
                    tiles_y, rank);
    ST_TRY(restir_layout_even(W, H, tiles_x, tiles_y, &L));
    return restir_layout_tile(&L, rank, ghost, out);
}

restir_status restir_layout_halo_plan(const restir_tile_layout* L, uint32_t rank, uint32_t radius, uint32_t N,
                                      restir_halo_segment* send, restir_halo_segment* recv, uint32_t* count) {
    if (!count || !send || !recv || N == 0) return fail(RESTIR_ERR_INVALID, "restir_halo_plan: null argument / N = 0");
    const uint32_t W = L ? L->global_width : 0u, H = L ? L->global_height : 0u;
    restir_tile me{};
    ST_TRY(restir_layout_tile(L, rank, 0, &me));
    struct R { uint64_t x0, y0, x1, y1; };
    auto grow = [&](const restir_tile& t) {
        return R{t.x0 > radius ? t.x0 - radius : 0u, t.y0 > radius ? t.y0 - radius : 0u,
                 std::min<uint64_t>((uint64_t)t.x0 + t.width + radius, W), std::min<uint64_t>((uint64_t)t.y0 + t.height + radius, H)};
    };
    auto owned = [](const restir_tile& t) { return R{t.x0, t.y0, (uint64_t)t.x0 + t.width, (uint64_t)t.y0 + t.height}; };
    auto meet = [](R a, R b) {
        R r{std::max(a.x0, b.x0), std::max(a.y0, b.y0), std::min(a.x1, b.x1), std::min(a.y1, b.y1)};
        if (r.x1 <= r.x0 || r.y1 <= r.y0) r = R{0, 0, 0, 0};
        return r;
    };
    const uint32_t cap = *count;
    uint32_t n = 0;
    uint64_t so = 0, ro = 0;
    for (uint32_t q = 0; q < L->tiles_x * L->tiles_y; q++) {
        if (q == rank) continue;
        restir_tile tq{};
        ST_TRY(restir_layout_tile(L, q, 0, &tq));
        const R s_ = meet(owned(me), grow(tq)), r_ = meet(owned(tq), grow(me));
        if (s_.x1 == 0 || r_.x1 == 0) continue;
        if (n >= cap) return fail(RESTIR_ERR_INVALID, "restir_halo_plan: more than %u segments", cap);
        auto fill = [&](restir_halo_segment& g, R r, uint64_t& off) {
            g.rank = q;
            g.x0 = (uint32_t)r.x0; g.y0 = (uint32_t)r.y0;
            g.width = (uint32_t)(r.x1 - r.x0); g.height = (uint32_t)(r.y1 - r.y0);
            g.offset = off;
            g.bytes = (uint64_t)g.width * g.height * N * 32u;
            off += g.bytes;
        };
        fill(send[n], s_, so);
        fill(recv[n], r_, ro);
        n++;
    }
    *count = n;
    return RESTIR_OK;
}

restir_status restir_halo_plan(uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t tiles_y, uint32_t rank, uint32_t radius,
                               uint32_t N, restir_halo_segment* send, restir_halo_segment* recv, uint32_t* count) {
    restir_tile_layout L;
    ST_TRY(restir_layout_even(W, H, tiles_x, tiles_y, &L));
    return restir_layout_halo_plan(&L, rank, radius, N, send, recv, count);
}

}  // extern "C"

namespace romis {

// The operations restir_halo_pass posts, from a plan: send i then recv i per segment (restir_halo_ops)
void halo_ops_from(const restir_halo_segment* send, const restir_halo_segment* recv, uint32_t n, restir_halo_op* ops) {
    auto op = [](uint32_t kind, const restir_halo_segment& g) {
        restir_halo_op o{};
        o.kind = kind; o.peer = g.rank; o.offset = g.offset; o.bytes = g.bytes;
        o.x0 = g.x0; o.y0 = g.y0; o.width = g.width; o.height = g.height;
        return o;
    };
    for (uint32_t i = 0; i < n; i++) {
        ops[2 * i] = op(RESTIR_HALO_OP_SEND, send[i]);
        ops[2 * i + 1] = op(RESTIR_HALO_OP_RECV, recv[i]);
    }
}

}  // namespace romis

extern "C" {

restir_status restir_halo_ops(uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t tiles_y, uint32_t rank, uint32_t radius,
                              uint32_t N, restir_halo_op* ops, uint32_t* count) {
    restir_tile_layout L;
    ST_TRY(restir_layout_even(W, H, tiles_x, tiles_y, &L));
    return restir_layout_halo_ops(&L, rank, radius, N, ops, count);
}

restir_status restir_layout_halo_ops(const restir_tile_layout* L, uint32_t rank, uint32_t radius, uint32_t N,
                                     restir_halo_op* ops, uint32_t* count) {
    if (!count || !ops) return fail(RESTIR_ERR_INVALID, "restir_halo_ops: null argument");
    restir_halo_segment sg[RESTIR_MAX_HALO_SEGS], rg_[RESTIR_MAX_HALO_SEGS];
    uint32_t n = RESTIR_MAX_HALO_SEGS;
    ST_TRY(restir_layout_halo_plan(L, rank, radius, N, sg, rg_, &n));
    if (*count < 2 * n) {
        const uint32_t need = 2 * n;
        *count = need;
        return fail(RESTIR_ERR_INVALID, "restir_halo_ops: capacity for %u operations needed", need);
    }
    halo_ops_from(sg, rg_, n, ops);
    *count = 2 * n;
    return RESTIR_OK;
}

}  // extern "C"
