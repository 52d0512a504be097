// distance_check.cpp -- the closest-point query's header (csrc/rt_distance_layout.hpp) on the host, under AddressSanitizer + UBSan
// (make -C raytracer-in-cpp_amd/csrc distance_check).  The header's one-point walk (near_walk: the pruning rule, the order of the children,
// the test of an entry when it is popped) over HostScene trees against brute force over the referenced faces, bit for bit; the pruning rule
// on its own, leaf box by leaf box; the routine's regions and its parameter ranges; the 64-bit index arithmetic and the argument rule.
// Scenes: the shipped cube and dodgeColorTest, seeded soups and sliver soups, a depth-capped tree with over-full leaves, lost nodes and
// unreachable faces -- each at the scales 2^-20, 1 and 2^20.  Points: random ones round the scene, vertices, edge midpoints and centroids of
// faces, points 1e4 extents away, non-finite ones.  Radii: +inf, 0, the median distance, one ulp round a point's own distance.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>
#include <unistd.h>

#include "host_scene.hpp"
#include "rt_distance_layout.hpp"

using namespace rtamd;

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static uint32_t bits(const float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// the query's bounds of a flattened HostScene, as the two kernels and the host sweep make them
struct Bounds {
    std::vector<NearTri> tris;
    std::vector<NearNode> nodes, chunks;
    std::vector<uint32_t> chunk0;
    float extent = 0.0f;
    int lost = 0, over_full = 0, unreachable = 0;
};
static Bounds make_bounds(const HostScene &hs) {
    Bounds b;
    rt_scene sc;
    hs.view(&sc);
    b.tris.resize(sc.n_face_refs);
    for (uint32_t k = 0; k < sc.n_face_refs; ++k) {
        const float *v = sc.tri_verts + static_cast<size_t>(sc.face_refs[k]) * 9;
        NearTri &t = b.tris[k];
        for (int q = 0; q < 3; ++q) { t.a[q] = v[q]; t.b[q] = v[3 + q]; t.c[q] = v[6 + q]; }
        t.face = sc.face_refs[k]; t.pad[0] = t.pad[1] = 0u;
    }
    b.nodes.resize(sc.n_nodes);
    b.chunk0.assign(sc.n_nodes, 0u);
    for (uint32_t j = 0; j < sc.n_nodes; ++j) {
        NearNode &n = b.nodes[j];
        n.first = sc.nodes[j].first; n.count_flags = sc.nodes[j].count_flags;
        near_box_clear(n);
        if (near_is_leaf(n)) {
            b.chunk0[j] = static_cast<uint32_t>(b.chunks.size());
            for (uint32_t c = 0; c < near_chunks(near_leaf_count(n)); ++c) {
                NearNode cb;
                cb.first = n.first + c * kNearChunk; cb.count_flags = near_min_u32(near_leaf_count(n) - c * kNearChunk, kNearChunk);
                near_box_clear(cb);
                for (uint32_t k = 0; k < cb.count_flags; ++k) near_box_add(cb, b.tris[cb.first + k]);
                b.chunks.push_back(cb);
            }
            for (uint32_t k = 0; k < near_leaf_count(n); ++k) near_box_add(n, b.tris[n.first + k]);
            if (static_cast<int>(near_leaf_count(n)) > hs.capacity) ++b.over_full;
        }
    }
    CHECK(near_sweep_nodes(b.nodes.data(), sc.n_nodes), "children must follow their parents");
    for (size_t i = 0; i < static_cast<size_t>(sc.n_faces) * 9; ++i) b.extent = std::fmax(b.extent, std::fabs(sc.tri_verts[i]));
    int32_t info[8];
    hs.info(info, nullptr);
    b.unreachable = info[5]; b.lost = info[7];
    return b;
}

static NearBest brute(const Bounds &b, const float p[3], const float r2) {
    NearBest best = near_none(p[0], p[1], p[2]);
    for (const NearTri &t : b.tris) near_take(best, near_point_triangle(p[0], p[1], p[2], t), t.face, r2);
    return best;
}

static bool same(const NearBest &x, const NearBest &y) {
    return x.face == y.face && bits(x.d2) == bits(y.d2) && bits(x.q[0]) == bits(y.q[0]) && bits(x.q[1]) == bits(y.q[1]) && bits(x.q[2]) == bits(y.q[2]);
}

struct Tally {
    uint64_t points = 0, none = 0, some = 0, walked = 0, all = 0, regions[7] = {}, ties = 0;
};

static std::vector<float> make_points(const Bounds &b, std::mt19937 &rng, const int n_random) {
    std::vector<float> P;
    const NearNode &root = b.nodes[0];
    float c[3], h[3];
    for (int q = 0; q < 3; ++q) { c[q] = 0.5f * (root.lo[q] + root.hi[q]); h[q] = root.hi[q] - root.lo[q]; }
    const float ext = std::fmax(h[0], std::fmax(h[1], h[2]));
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    for (int i = 0; i < n_random; ++i)
        for (int q = 0; q < 3; ++q) P.push_back(c[q] + U(rng) * ext);
    const size_t faces = std::min<size_t>(b.tris.size(), b.tris.size() > 4096 ? 4 : 48);          // (the big scenes: fewer, the check stays quick)
    for (size_t f = 0; f < faces; ++f) {
        const NearTri &t = b.tris[(f * 7919u) % b.tris.size()];
        for (int q = 0; q < 3; ++q) P.push_back(t.a[q]);
        for (int q = 0; q < 3; ++q) P.push_back(t.b[q]);
        for (int q = 0; q < 3; ++q) P.push_back(t.c[q]);
        for (int q = 0; q < 3; ++q) P.push_back((t.a[q] + t.b[q]) * 0.5f);
        for (int q = 0; q < 3; ++q) P.push_back((t.b[q] + t.c[q]) * 0.5f);
        for (int q = 0; q < 3; ++q) P.push_back((t.a[q] + t.b[q] + t.c[q]) / 3.0f);
    }
    for (int i = 0; i < 8; ++i)
        for (int q = 0; q < 3; ++q) P.push_back(c[q] + ((i >> q) & 1 ? 1e4f : -1e4f) * ext);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (const float bad : {nan, inf, -inf})
        for (int q = 0; q < 3; ++q) {
            float p[3] = {c[0], c[1], c[2]};
            p[q] = bad;
            P.insert(P.end(), p, p + 3);
        }
    return P;
}

static void check_scene(const char *what, const HostScene &hs, const int n_random, Tally &tally, const uint32_t seed) {
    const Bounds b = make_bounds(hs);
    if (b.tris.empty()) { CHECK(false, "%s references no face", what); return; }
    const uint64_t walked0 = tally.walked, all0 = tally.all;
    std::mt19937 rng(seed);
    const std::vector<float> P = make_points(b, rng, n_random);
    const size_t n = P.size() / 3;
    const float inf = std::numeric_limits<float>::infinity();
    // the unbounded answers first: their median and the first point's own distance give the finite radii
    std::vector<NearBest> open(n);
    std::vector<float> dist;
    for (size_t i = 0; i < n; ++i) {
        open[i] = brute(b, &P[i * 3], inf);
        if (open[i].face != kNearNoFace && std::isfinite(open[i].d2)) dist.push_back(std::sqrt(open[i].d2));
    }
    std::sort(dist.begin(), dist.end());
    const float median = dist.empty() ? 1.0f : dist[dist.size() / 2], own = std::sqrt(open[0].d2);
    const float radii[] = {inf, 0.0f, median, std::nextafter(own, 0.0f), own, std::nextafter(own, inf)};
    for (const float r : radii) {
        const float r2 = r * r;
        uint64_t none = 0, some = 0;
        for (size_t i = 0; i < n; ++i) {
            const float *p = &P[i * 3];
            NearWalkStats st{0, 0, false};
            const NearBest got = near_walk(b.nodes.data(), b.tris.data(), b.chunks.data(), b.chunk0.data(), b.extent, p[0], p[1], p[2], r2, &st);
            const NearBest want = r == inf ? open[i] : brute(b, p, r2);
            CHECK(same(got, want), "%s r %g point %zu (%g %g %g): walk face %d d2 %a, brute force face %d d2 %a", what, r, i, p[0], p[1], p[2],
                  static_cast<int>(got.face), got.d2, static_cast<int>(want.face), want.d2);
            if (want.face == kNearNoFace) {
                ++none;
                CHECK(want.d2 == inf && bits(want.q[0]) == bits(p[0]) && bits(want.q[1]) == bits(p[1]) && bits(want.q[2]) == bits(p[2]), "no candidate: +inf and P itself");
            } else {
                ++some;
                CHECK(want.d2 <= r2, "a candidate lies within the radius");
            }
            CHECK(!st.overflow, "%s: the walk's stack overflowed", what);
            tally.walked += st.tris; tally.all += b.tris.size();
        }
        tally.points += n; tally.none += none; tally.some += some;
    }
    // the rule on its own: no leaf box may be pruned against the least computed d2 of the leaf's own faces, nor against a d2 one ulp above
    for (size_t i = 0; i < n; ++i) {
        const float *p = &P[i * 3];
        const float sigma = near_sigma(b.extent, p[0], p[1], p[2]);
        for (const NearNode &nd : b.nodes) {
            if (!near_is_leaf(nd) || near_leaf_count(nd) == 0u) continue;
            float least = inf;
            int at_least = 0;
            for (uint32_t k = 0; k < near_leaf_count(nd); ++k) {
                const NearClosest c = near_point_triangle(p[0], p[1], p[2], b.tris[nd.first + k]);
                ++tally.regions[c.region];
                if (c.d2 < least) { least = c.d2; at_least = 1; } else if (c.d2 == least) ++at_least;
            }
            if (at_least > 1) ++tally.ties;
            CHECK(!near_pruned(near_box_bound2(nd.lo, nd.hi, p[0], p[1], p[2], sigma), least), "%s: a leaf box was pruned against its own nearest face (point %zu)", what, i);
        }
    }
    std::printf("  %-34s nodes %6zu refs %7zu lost %4d over-full %5d unreachable %5d points %5zu stepped %5.1f %%\n", what, b.nodes.size(), b.tris.size(), b.lost,
                b.over_full, b.unreachable, n, 100.0 * static_cast<double>(tally.walked - walked0) / static_cast<double>(tally.all - all0));
}

// a seeded soup as an OBJ file: m triangles with centres in [-1, 1]^3 and edges of about 0.15; slivers: the second edge almost along the first
static std::string write_soup(const uint32_t seed, const int m, const bool sliver) {
    char path[] = "/tmp/distance_check_XXXXXX.obj";
    const int fd = mkstemps(path, 4);
    if (fd < 0) { std::perror("mkstemps"); std::exit(2); }
    FILE *f = fdopen(fd, "w");
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> U(-1.0, 1.0), K(0.3, 3.0);
    std::normal_distribution<double> N(0.0, 0.15), tiny(0.0, 1e-6);
    for (int i = 0; i < m; ++i) {
        double c[3], e0[3], e1[3];
        const double k = K(rng);
        for (int q = 0; q < 3; ++q) { c[q] = U(rng); e0[q] = N(rng); e1[q] = sliver ? e0[q] * k + tiny(rng) : N(rng); }
        std::fprintf(f, "v %.9g %.9g %.9g\nv %.9g %.9g %.9g\nv %.9g %.9g %.9g\n", c[0], c[1], c[2], c[0] + e0[0], c[1] + e0[1], c[2] + e0[2], c[0] + e1[0],
                     c[1] + e1[1], c[2] + e1[2]);
    }
    // a face of a repeated vertex, a face that repeats another, and zero-area faces of three DISTINCT collinear vertices (the third on the
    // segment of the first two, beyond it, and almost on it): these have finite distances and are candidates like any other face
    std::fprintf(f, "v 0.1 0.2 0.3\nv 0.5 0.4 0.1\nv 0.3 0.3 0.2\nv 0.9 0.6 -0.1\nv 0.30000001 0.3 0.2\n");
    std::fprintf(f, "f 1 1 2\nf 4 5 6\nf %d %d %d\nf %d %d %d\nf %d %d %d\n", 3 * m + 1, 3 * m + 2, 3 * m + 3, 3 * m + 1, 3 * m + 2, 3 * m + 4, 3 * m + 1, 3 * m + 2,
                 3 * m + 5);
    for (int i = 0; i < m; ++i) std::fprintf(f, "f %d %d %d\n", 3 * i + 1, 3 * i + 2, 3 * i + 3);
    std::fclose(f);
    return path;
}

static bool load(HostScene &hs, const std::string &path, const int cap, const int depth) {
    std::string err;
    if (!hs.load_obj(path, &err)) { std::printf("FAILED to load %s: %s\n", path.c_str(), err.c_str()); ++g_failed; return false; }
    hs.build_octree(cap, depth);
    hs.flatten();
    return true;
}

static void at_scales(const char *name, HostScene &hs, const int n_random, Tally &tally, const uint32_t seed) {
    for (const int e : {0, -20, 20}) {
        const float s = std::ldexp(1.0f, e);
        const float model[12] = {s, 0, 0, 0, 0, s, 0, 0, 0, 0, s, 0};
        hs.set_model(model, true);
        char what[96];
        std::snprintf(what, sizeof what, "%s x 2^%d", name, e);
        check_scene(what, hs, n_random, tally, seed + static_cast<uint32_t>(e + 32));
    }
}

static void check_routine() {
    // the seven regions of a plain triangle, points on a vertex, an edge midpoint and the centroid, and what degenerate triangles give
    const float A[3] = {0, 0, 0}, B[3] = {1, 0, 0}, C[3] = {0, 1, 0};
    const struct { float p[3]; int region; float q[3], d2; } cases[] = {
        {{-1, -1, 0}, 0, {0, 0, 0}, 2}, {{2, -0.5f, 0}, 1, {1, 0, 0}, 1.25f}, {{0.5f, -1, 0}, 2, {0.5f, 0, 0}, 1}, {{-0.5f, 2, 0}, 3, {0, 1, 0}, 1.25f},
        {{-1, 0.5f, 0}, 4, {0, 0.5f, 0}, 1}, {{1, 1, 0}, 5, {0.5f, 0.5f, 0}, 0.5f}, {{0.25f, 0.25f, 2}, 6, {0.25f, 0.25f, 0}, 4},
        {{0, 0, 0}, 0, {0, 0, 0}, 0}, {{1, 0, 0}, 1, {1, 0, 0}, 0}, {{0, 1, 0}, 3, {0, 1, 0}, 0}, {{0.5f, 0, 0}, 2, {0.5f, 0, 0}, 0},
    };
    for (const auto &c : cases) {
        const NearClosest r = near_point_triangle(c.p[0], c.p[1], c.p[2], A[0], A[1], A[2], B[0], B[1], B[2], C[0], C[1], C[2]);
        CHECK(r.region == c.region && r.qx == c.q[0] && r.qy == c.q[1] && r.qz == c.q[2] && r.d2 == c.d2, "point (%g %g %g): region %d Q (%g %g %g) d2 %g", c.p[0],
              c.p[1], c.p[2], r.region, r.qx, r.qy, r.qz, r.d2);
    }
    // a triangle of one repeated vertex: every point is in region A; a NaN point: no test holds, the face formula gives NaN
    const NearClosest one = near_point_triangle(3, 4, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0);
    CHECK(one.region == 0 && one.d2 == 13.0f, "repeated vertex: region %d d2 %g", one.region, one.d2);
    const NearClosest bad = near_point_triangle(std::numeric_limits<float>::quiet_NaN(), 0, 0, A[0], A[1], A[2], B[0], B[1], B[2], C[0], C[1], C[2]);
    CHECK(bad.region == 6 && std::isnan(bad.d2), "NaN point: region %d d2 %g", bad.region, bad.d2);
    NearBest b = near_none(1, 2, 3);
    near_take(b, bad, 0u, std::numeric_limits<float>::infinity());
    CHECK(b.face == kNearNoFace, "a NaN d2 is never a candidate");
}

static void check_arguments() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const auto at = [](const uint64_t a) { return reinterpret_cast<const void *>(static_cast<uintptr_t>(a)); };
    const int32_t big = INT32_MAX;
    const uint64_t in = 1ull << 40, v1 = static_cast<uint64_t>(big) * 4u, v3 = v1 * 3u;
    CHECK(near_out3(static_cast<uint64_t>(big) - 1u) == 6442450938ull, "the last point's first float, in 64 bits");
    CHECK(near_args(big, at(in), inf, at(in + v3), at(in + v3 + v1), at(in + v3 + 2 * v1)) == nullptr, "n = INT32_MAX, back to back");
    CHECK(near_args(big, at(in), inf, at(in + v3 - 1), nullptr, nullptr) != nullptr, "face shares the input's last byte");
    CHECK(near_args(big, at(in), inf, nullptr, nullptr, at(in - v3 + 1)) != nullptr, "point's last byte is the input's first");
    CHECK(near_args(big, at(in), inf, at(in + v3), at(in + v3 + v1 - 1), nullptr) != nullptr, "two outputs share a byte");
    CHECK(near_args(big, at(in), inf, nullptr, nullptr, nullptr) != nullptr, "all outputs null");
    CHECK(near_args(4, nullptr, inf, at(64), nullptr, nullptr) != nullptr, "null input");
    CHECK(near_args(-1, at(in), inf, at(64), nullptr, nullptr) != nullptr, "negative n");
    CHECK(near_args(4, at(in), nan, at(64), nullptr, nullptr) != nullptr && near_args(4, at(in), -1.0f, at(64), nullptr, nullptr) != nullptr, "NaN and negative radii");
    CHECK(near_args(0, nullptr, 0.0f, nullptr, nullptr, nullptr) == nullptr && near_args(0, nullptr, nan, nullptr, nullptr, nullptr) != nullptr, "n == 0 still checks the radius");
    CHECK(near_args(4, at(in), 0.0f, nullptr, at(64), nullptr) == nullptr && near_args(4, at(in), inf, nullptr, nullptr, at(64)) == nullptr, "one output is enough");
    // a bound that overflows, a limit that overflows, non-finite points: not pruned
    const float lo[3] = {-1, -1, -1}, hi[3] = {1, 1, 1};
    CHECK(!near_pruned(near_box_bound2(lo, hi, 3e38f, 3e38f, 3e38f, near_sigma(1.0f, 3e38f, 3e38f, 3e38f)), inf), "overflowing bound against +inf");
    CHECK(!near_pruned(near_box_bound2(lo, hi, nan, 0, 0, near_sigma(1.0f, nan, 0, 0)), 0.0f), "NaN point");
    CHECK(!near_pruned(near_box_bound2(lo, hi, inf, 0, 0, near_sigma(1.0f, inf, 0, 0)), 0.0f), "infinite point");
    CHECK(near_pruned(near_box_bound2(lo, hi, 3, 0, 0, near_sigma(1.0f, 3, 0, 0)), 1.0f) && !near_pruned(near_box_bound2(lo, hi, 3, 0, 0, near_sigma(1.0f, 3, 0, 0)), 4.0f), "a plain box");
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: distance_check <directory of the shipped scenes>\n"); return 2; }
    check_routine();
    check_arguments();
    Tally tally;
    const std::string dir = argv[1];
    {
        HostScene cube, dodge, capped;
        if (load(cube, dir + "/cube.obj", 1000, 15)) at_scales("cube.obj", cube, 400, tally, 1);
        if (load(dodge, dir + "/dodgeColorTest.obj", 1000, 15)) at_scales("dodgeColorTest.obj", dodge, 8, tally, 2);
        if (load(capped, dir + "/dodgeColorTest.obj", 16, 3)) {
            const Bounds b = make_bounds(capped);
            CHECK(b.over_full > 0 && b.lost > 0, "dodgeColorTest at 16 / 3 must hold over-full leaves and a lost node");
            check_scene("dodgeColorTest.obj cap 16 depth 3", capped, 8, tally, 3);
        }
    }
    const struct { uint32_t seed; int m; bool sliver; int cap, depth; } soups[] = {
        {11, 12, false, 1000, 15}, {12, 64, false, 1000, 15}, {13, 65, false, 1000, 15}, {8, 800, false, 250, 15}, {9, 600, true, 100, 15},
    };
    for (const auto &s : soups) {
        const std::string path = write_soup(s.seed, s.m, s.sliver);
        HostScene hs;
        char name[64];
        std::snprintf(name, sizeof name, "%s %d (seed %u)", s.sliver ? "slivers" : "soup", s.m, s.seed);
        if (load(hs, path, s.cap, s.depth)) at_scales(name, hs, 256, tally, s.seed);
        unlink(path.c_str());
    }
    // depth-capped trees: over-full leaves and a lost node above (dodgeColorTest at 16 / 3); lost nodes and unreachable faces here, in the first
    // seeded soup that shows both
    bool found = false;
    for (uint32_t seed = 30; seed < 46 && !found; ++seed) {
        const std::string path = write_soup(seed, 300, false);
        HostScene hs;
        if (load(hs, path, 16, 5)) {
            const Bounds b = make_bounds(hs);
            if (b.lost > 0 && b.unreachable > 0) {
                found = true;
                char name[64];
                std::snprintf(name, sizeof name, "capped soup 300 (seed %u) 16 / 5", seed);
                at_scales(name, hs, 64, tally, seed);
            }
        }
        unlink(path.c_str());
    }
    CHECK(found, "no seed gave a capped tree with lost nodes and unreachable faces");
    CHECK(tally.none > 0 && tally.some > 0, "radii with and without candidates");
    for (int r = 0; r < 7; ++r) CHECK(tally.regions[r] > 0, "region %d was never reached", r);
    CHECK(tally.ties > 0, "no leaf held a tie");
    std::printf("points x radii %" PRIu64 " (none %" PRIu64 ", some %" PRIu64 "); triangles stepped %" PRIu64 " of %" PRIu64 " (%.2f %%); regions", tally.points, tally.none,
                tally.some, tally.walked, tally.all, 100.0 * static_cast<double>(tally.walked) / static_cast<double>(tally.all));
    for (int r = 0; r < 7; ++r) std::printf(" %" PRIu64, tally.regions[r]);
    std::printf("; leaves with ties %" PRIu64 "\n", tally.ties);
    if (g_failed) { std::printf("%d checks FAILED\n", g_failed); return 1; }
    std::printf("all checks held\n");
    return 0;
}
