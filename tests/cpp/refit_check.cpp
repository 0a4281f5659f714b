// refit_check -- host checks of csrc/bvh.cpp refit_bvh: a tree built over one triangle list and refitted to the same
// triangles moved keeps every invariant bvh_check asks of a built tree, and its walks prune no hit.
// tests/test_bvh_refit.py writes the triangle files (bvh_check's format) and reads the lines printed here.
//
//   refit_check [--rays N] name original.tri moved.tri [name original.tri moved.tri ...]
//   refit_check --dump max_leaf original.tri moved.tri out.bin
//
// The second form writes the refitted tree for the device tests (tests/test_gpu_dynamic_scene.py): uint32 num_nodes,
// triangles, q_ok; 8 floats per node; 4 words per node (4 zero words when !q_ok); tri_order; q.lo[3], q.s[3].
//
// The invariants, the restated device walks and the hashed rays are bvh_check's own: its translation unit is included
// here with its main renamed, so the two tools cannot drift apart.
#define main bvh_check_main
#include "bvh_check.cpp"
#undef main

namespace {

// What build_and_check asks of a built tree, of tr.bvh (refitted) over the moved triangles `in`; tr.q and tr.tris are
// filled here.
bool check_refitted(const std::vector<BvhTriangle>& in, uint32_t max_leaf, const FlatBvh& built, Tree& tr) {
    const int before = g_fail.load();
    const uint32_t clamped = std::min(std::max(max_leaf, 1u), 255u);
    const size_t T = in.size();
    const FlatBvh& b = tr.bvh;
    // the topology is the built tree's: order, links, leaves
    CHECK(b.num_nodes == built.num_nodes && b.max_depth == built.max_depth && b.nodes.size() == built.nodes.size(),
          "%u nodes after the refit, %u before\n", b.num_nodes, built.num_nodes);
    CHECK(b.tri_order == built.tri_order, "tri_order changed\n");
    if (g_fail != before) return false;
    for (uint32_t i = 0; i < b.num_nodes; i++)
        CHECK(f2u(b.nodes[8 * i + 3]) == f2u(built.nodes[8 * i + 3]) && f2u(b.nodes[8 * i + 7]) == f2u(built.nodes[8 * i + 7]),
              "node %u: link or leaf word changed\n", i);
    tr.q = quantize_nodes(tr.bvh);
    tr.tris.resize(T);
    for (size_t k = 0; k < T; k++) {
        const BvhTriangle& t = in[b.tri_order[k]];
        Tri& d = tr.tris[k];
        d.v0 = mk(t.v0[0], t.v0[1], t.v0[2]);
        d.e1 = mk(t.v1[0] - t.v0[0], t.v1[1] - t.v0[1], t.v1[2] - t.v0[2]);
        d.e2 = mk(t.v2[0] - t.v0[0], t.v2[1] - t.v0[1], t.v2[2] - t.v0[2]);
        d.orig = b.tri_order[k];
    }
    bool structural_q = b.num_nodes > 0 && b.num_nodes < 65536u;
    if (T) {
        Span all;
        for (int a = 0; a < 3; a++) { all.lo[a] = FLT_MAX; all.hi[a] = -FLT_MAX; }
        for (const BvhTriangle& t : in)
            for (const float* v : {t.v0, t.v1, t.v2})
                for (int a = 0; a < 3; a++) { all.lo[a] = std::min(all.lo[a], v[a]); all.hi[a] = std::max(all.hi[a], v[a]); }
        float scale = 0.0f;
        for (int a = 0; a < 3; a++) scale = std::max({scale, std::fabs(all.lo[a]), std::fabs(all.hi[a]), all.hi[a] - all.lo[a]});
        const float pad = 1e-5f * scale + 1e-30f;
        std::vector<uint32_t> cover(T, 0);
        Span span;
        const uint32_t end = check_subtree(tr, in, 0, clamped, pad, cover, span, 0);
        CHECK(end == b.num_nodes, "the root's subtree ends at %u of %u nodes\n", end, b.num_nodes);
        for (size_t k = 0; k < T; k++) CHECK(cover[k] == 1, "triangle slot %zu lies in %u leaves\n", k, cover[k]);
        // the root box is exactly the moved scene's bounds with the pad: a refit that only grew boxes fails here
        for (int a = 0; a < 3; a++)
            CHECK(f2u(b.nodes[a]) == f2u(all.lo[a] - pad) && f2u(b.nodes[4 + a]) == f2u(all.hi[a] + pad),
                  "root axis %d: [%.9g, %.9g], the moved scene's padded bounds [%.9g, %.9g]\n", a, b.nodes[a], b.nodes[4 + a],
                  all.lo[a] - pad, all.hi[a] + pad);
        for (uint32_t i = 0; i < b.num_nodes; i++) {
            const uint32_t leaf = f2u(b.nodes[8 * i + 7]);
            structural_q = structural_q && (leaf == 0u || ((leaf >> 24) < 16u && (leaf & 0xFFFFFFu) + (leaf >> 24) <= 4096u));
        }
    }
    const QuantizedNodes& q = tr.q;
    CHECK(q.ok == structural_q, "quantized nodes ok = %d, the fields %s\n", (int)q.ok, structural_q ? "fit" : "do not fit");
    if (q.ok) {
        CHECK(q.words.size() == 4 * (size_t)b.num_nodes, "%zu words for %u nodes\n", q.words.size(), b.num_nodes);
        for (uint32_t i = 0; i < b.num_nodes && q.words.size() == 4 * (size_t)b.num_nodes; i++) {
            const uint32_t* w = &q.words[4 * i];
            const float* o = &b.nodes[8 * i];
            const uint32_t ql[3] = {w[0] & 0xFFFFu, w[0] >> 16, w[1] & 0xFFFFu}, qh[3] = {w[1] >> 16, w[2] & 0xFFFFu, w[2] >> 16};
            for (int a = 0; a < 3; a++) {
                const double lo = (double)q.lo[a] + (double)ql[a] * (double)q.s[a], hi = (double)q.lo[a] + (double)qh[a] * (double)q.s[a];
                CHECK(lo <= (double)o[a] && hi >= (double)o[4 + a], "node %u axis %d: quantized [%.9g, %.9g] inside float [%.9g, %.9g]\n",
                      i, a, lo, hi, o[a], o[4 + a]);
            }
            const uint32_t miss = f2u(o[3]), leaf = f2u(o[7]);
            CHECK((w[3] & 0xFFFFu) == miss && ((w[3] >> 16) & 0xFFFu) == (leaf & 0xFFFFFFu) && (w[3] >> 28) == (leaf >> 24),
                  "node %u: word %08x for miss %u leaf %08x\n", i, w[3], miss, leaf);
        }
    }
    return g_fail == before;
}

int dump(int argc, char** argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: refit_check --dump max_leaf original.tri moved.tri out.bin\n"); return 2; }
    const uint32_t ml = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    std::vector<BvhTriangle> orig, moved;
    if (!read_triangles(argv[3], orig) || !read_triangles(argv[4], moved) || orig.size() != moved.size()) {
        std::fprintf(stderr, "refit_check: cannot read the triangle files\n");
        return 1;
    }
    FlatBvh b = build_bvh(orig, ml);
    refit_bvh(b, moved);
    const QuantizedNodes q = quantize_nodes(b);
    FILE* fh = std::fopen(argv[5], "wb");
    if (!fh) return 1;
    const uint32_t head[3] = {b.num_nodes, (uint32_t)moved.size(), q.ok ? 1u : 0u};
    bool ok = std::fwrite(head, 4, 3, fh) == 3;
    ok = ok && std::fwrite(b.nodes.data(), 4, b.nodes.size(), fh) == b.nodes.size();
    ok = ok && std::fwrite(q.words.data(), 4, q.words.size(), fh) == q.words.size();
    ok = ok && std::fwrite(b.tri_order.data(), 4, b.tri_order.size(), fh) == b.tri_order.size();
    ok = ok && std::fwrite(q.lo, 4, 3, fh) == 3 && std::fwrite(q.s, 4, 3, fh) == 3;
    return std::fclose(fh) == 0 && ok ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--dump")) return dump(argc, argv);
    const uint32_t leaves[] = {1, 2, 3, 5, 15, 16};
    const uint32_t ray_leaves[] = {2, 3, 15, 16};
    uint32_t nrays = 100000;
    int first = 1;
    if (argc > 2 && !std::strcmp(argv[1], "--rays")) { nrays = (uint32_t)std::strtoul(argv[2], nullptr, 10); first = 3; }
    if (first >= argc || (argc - first) % 3) {
        std::fprintf(stderr, "usage: refit_check [--rays N] name original.tri moved.tri ...\n");
        return 2;
    }
    for (int a = first; a < argc; a += 3) {
        const char* name = argv[a];
        std::vector<BvhTriangle> orig, moved;
        if (!read_triangles(argv[a + 1], orig) || !read_triangles(argv[a + 2], moved) || orig.size() != moved.size()) {
            std::printf("FAIL %s: cannot read\n", name);
            g_fail++;
            continue;
        }
        const bool same = orig.empty() || !std::memcmp(orig.data(), moved.data(), orig.size() * sizeof(BvhTriangle));
        std::vector<Tree> ray_trees;
        for (uint32_t ml : leaves) {
            g_where = std::string(name) + " max_leaf " + std::to_string(ml);
            const FlatBvh built = build_bvh(orig, ml);
            Tree tr;
            tr.bvh = built;
            refit_bvh(tr.bvh, moved);
            const bool ok = check_refitted(moved, ml, built, tr);
            // how the boxes moved against the built tree's (the deformations are made to grow or to shrink them)
            uint32_t grew = 0, shrank = 0, equal = 0;
            for (uint32_t i = 0; i < built.num_nodes; i++) {
                const float *o = &built.nodes[8 * i], *r = &tr.bvh.nodes[8 * i];
                bool g = false, s = true, e = true;
                for (int c = 0; c < 3; c++) {
                    g = g || r[c] < o[c] || r[4 + c] > o[4 + c];
                    s = s && (r[4 + c] - r[c]) <= (o[4 + c] - o[c]);   // no wider on any axis
                    e = e && f2u(r[c]) == f2u(o[c]) && f2u(r[4 + c]) == f2u(o[4 + c]);
                }
                grew += g; shrank += s && !e; equal += e;
            }
            if (same) CHECK(equal == built.num_nodes, "the identity refit changed %u of %u boxes\n", built.num_nodes - equal, built.num_nodes);
            const bool ok2 = ok && (!same || equal == built.num_nodes);
            std::printf("refit %s max_leaf %u triangles %zu nodes %u grew %u shrank %u equal %u q_ok %d %s\n", name, ml, moved.size(),
                        tr.bvh.num_nodes, grew, shrank, equal, (int)tr.q.ok, ok2 ? "ok" : "BAD");
            if (ok2 && std::find(std::begin(ray_leaves), std::end(ray_leaves), ml) != std::end(ray_leaves)) ray_trees.push_back(std::move(tr));
        }
        if (nrays && ray_trees.size() == sizeof(ray_leaves) / sizeof(ray_leaves[0]) && !moved.empty()) {
            g_where = std::string(name) + " rays";
            const int before = g_fail.load();
            const uint32_t nthreads = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
            std::vector<RayStats> part(nthreads);
            std::vector<std::thread> pool;
            for (uint32_t t = 0; t < nthreads; t++)
                pool.emplace_back([&, t] { check_rays(moved, ray_trees, t, nthreads, nrays, part[t]); });
            for (std::thread& t : pool) t.join();
            RayStats st;
            for (const RayStats& p : part) {
                st.rays += p.rays; st.occluded += p.occluded; st.clear += p.clear; st.closest_found += p.closest_found;
            }
            std::printf("rays %s n %llu occluded %llu clear %llu closest %llu %s\n", name, (unsigned long long)st.rays,
                        (unsigned long long)st.occluded, (unsigned long long)st.clear, (unsigned long long)st.closest_found,
                        g_fail == before ? "ok" : "BAD");
        }
    }
    std::printf("%s: %d failures\n", g_fail ? "FAILED" : "PASSED", g_fail.load());
    return g_fail ? 1 : 0;
}
