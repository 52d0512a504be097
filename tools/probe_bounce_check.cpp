// Stand-alone host check of the bounced-light part of rt_probe_layout.hpp (the streamed per-lane blend that k_gather_bounce and
// k_probes_bounce run at every hit, the clamp and the argument rule of the calls), meant for a sanitizer build on the CPU:
//   g++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iraytracer-in-cpp_amd/csrc tools/probe_bounce_check.cpp -o probe_bounce_check
// (make -C raytracer-in-cpp_amd/csrc probe_bounce_check builds and runs it).  Exit status 0: every check held.
// The streamed blend must equal probe_lookup / probe_lookup_visible bit for bit: on random grids with every subset of single-layer axes, for
// all 256 visibility bytes, with NaN, +-inf and negative coefficients, at points inside, outside and on the planes of the grid.
// With an argument, it also writes a fixture for tests/test_probe_bounce_api.py there: raw little-endian records of one small case
// (header of 16 int32: magic, dims[3], points, then origin[3] and step[3] as float bits; coefficients; per point 6 floats P N, one uint32 of
// visibility bits, one uint32 mode, 3 floats kd, 3 floats R before, 3 floats R after probe_bounce_add of probe_bounce_lookup).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_probe_layout.hpp"

using namespace rtamd;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// equal in every bit; two NaNs count as equal whatever their sign and payload: which of two NaN operands an addition hands on is the
// compiler's choice of operand order, on the host and on the device, and no definition of this library reads a NaN's payload
static bool same(const float a, const float b) { return std::memcmp(&a, &b, sizeof a) == 0 || (std::isnan(a) && std::isnan(b)); }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(rng_state >> 33);
}
static float unit() { return static_cast<float>(rnd() & 0xffffff) / 16777216.0f; }                // [0, 1)
static float signed_unit() { return unit() * 2.0f - 1.0f; }

struct Volume {
    ProbeGrid G;
    std::vector<float> coeff;
};
// `single`: bit q set = axis q has one layer.  special: NaN, +-inf and large negative coefficients among the values
static Volume volume(const int single, const bool special) {
    Volume v;
    for (int q = 0; q < 3; ++q) {
        v.G.dims[q] = ((single >> q) & 1) ? 1 : 2 + static_cast<int32_t>(rnd() % 3u);
        v.G.origin[q] = signed_unit() * 3.0f;
        v.G.step[q] = 0.125f + unit() * 2.0f;
    }
    CHECK(probe_grid_bad(v.G) == nullptr);
    v.coeff.resize(static_cast<size_t>(probe_cells(v.G)) * kProbeCoeffs);
    for (float &c : v.coeff) {
        c = signed_unit() * 4.0f;
        if (special) {
            const uint32_t r = rnd() % 23u;
            if (r == 0u) c = std::numeric_limits<float>::quiet_NaN();
            else if (r == 1u) c = std::numeric_limits<float>::infinity();
            else if (r == 2u) c = -std::numeric_limits<float>::infinity();
            else if (r == 3u) c = -1.0e30f;
            else if (r == 4u) c = -0.0f;
        }
    }
    return v;
}
// a point in, round or on a plane of the grid; now and then a NaN coordinate
static void point(const ProbeGrid &G, const int kind, float P[3]) {
    for (int q = 0; q < 3; ++q) {
        const float span = G.step[q] * static_cast<float>(G.dims[q] - 1);
        P[q] = G.origin[q] - 0.3f * (span + 1.0f) + unit() * 1.6f * (span + 1.0f);
        if (kind == 1) P[q] = probe_position(G, q, static_cast<int32_t>(rnd() % static_cast<uint32_t>(G.dims[q])));       // on a plane: weights 0 and 1
        if (kind == 2 && q == static_cast<int>(rnd() % 3u)) P[q] = std::numeric_limits<float>::quiet_NaN();
    }
}
static void normal(const int kind, float N[3]) {
    for (int q = 0; q < 3; ++q) N[q] = signed_unit();
    if (kind == 3) { N[0] = 0.0f; N[1] = -0.0f; N[2] = 0.0f; }                    // no point
}

static void check_streamed_blend() {
    int cases = 0, divided = 0, nonfinite = 0;
    for (int single = 0; single < 8; ++single)
        for (int rep = 0; rep < 6; ++rep) {
            const Volume v = volume(single, rep >= 3);
            for (int pt = 0; pt < 12; ++pt) {
                float P[3], N[3];
                point(v.G, pt % 4 == 1 ? 1 : (pt == 6 ? 2 : 0), P);
                normal(pt == 7 ? 3 : 0, N);
                float want[3], got[3];
                probe_lookup(v.G, v.coeff.data(), P[0], P[1], P[2], N[0], N[1], N[2], want);
                probe_bounce_lookup(v.G, v.coeff.data(), P[0], P[1], P[2], N[0], N[1], N[2], false, 0xa5u, got);
                for (int c = 0; c < 3; ++c) CHECK(same(want[c], got[c]));
                for (uint32_t vis = 0; vis < 256u; ++vis) {
                    (void)probe_lookup_visible(v.G, v.coeff.data(), P[0], P[1], P[2], N[0], N[1], N[2], vis, want);
                    probe_bounce_lookup(v.G, v.coeff.data(), P[0], P[1], P[2], N[0], N[1], N[2], true, vis, got);
                    for (int c = 0; c < 3; ++c) {
                        CHECK(same(want[c], got[c]));
                        if (!std::isfinite(want[c])) ++nonfinite;
                    }
                    ++cases;
                }
                // how often case B divides: the fixture must reach it
                const ProbeAxis ax = probe_axis(P[0], v.G.origin[0], v.G.step[0], v.G.dims[0]), ay = probe_axis(P[1], v.G.origin[1], v.G.step[1], v.G.dims[1]),
                                az = probe_axis(P[2], v.G.origin[2], v.G.step[2], v.G.dims[2]);
                for (uint32_t vis = 0; vis < 256u; ++vis)
                    if (probe_visible_use(probe_read_mask(v.G), vis, probe_positive_mask(ax, ay, az)).divide) ++divided;
                // the segment's far end: the position of the probe the blend reads for that corner
                for (int b = 0; b < 8; ++b) {
                    float cx, cy, cz;
                    probe_corner_position(v.G, P[0], P[1], P[2], b, cx, cy, cz);
                    CHECK(same(cx, probe_position(v.G, 0, ax.i0 + (b & 1))) && same(cy, probe_position(v.G, 1, ay.i0 + ((b >> 1) & 1))) &&
                          same(cz, probe_position(v.G, 2, az.i0 + (b >> 2))));
                    if ((probe_read_mask(v.G) >> b) & 1u)
                        CHECK(ax.i0 + (b & 1) < v.G.dims[0] && ay.i0 + ((b >> 1) & 1) < v.G.dims[1] && az.i0 + (b >> 2) < v.G.dims[2]);
                }
            }
        }
    std::printf("streamed blend: %d lookups equal probe_lookup_visible in every bit (%d of them case B, %d non-finite channels)\n", cases, divided, nonfinite);
    CHECK(cases == 8 * 6 * 12 * 256 && divided > cases / 8 && nonfinite > 1000);
}

static void check_clamp() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    CHECK(same(probe_bounce_add(0.0f, 0.5f, 0.0f), 0.0f) && same(probe_bounce_add(0.0f, 0.5f, -0.0f), 0.0f));
    CHECK(same(probe_bounce_add(0.25f, 0.5f, -3.0f), 0.25f) && same(probe_bounce_add(0.25f, 0.5f, nan), 0.25f) && same(probe_bounce_add(0.25f, 0.5f, -inf), 0.25f));
    CHECK(same(probe_bounce_add(0.25f, 0.5f, 3.0f), 1.75f) && same(probe_bounce_add(0.25f, 0.5f, inf), inf));
    CHECK(same(probe_bounce_add(1.0f, 0.1f, 0.3f), 1.0f + 0.1f * 0.3f));
}

static void check_arguments() {
    ProbeGrid G{{0, 0, 0}, {1, 1, 1}, {2, 2, 2}};
    std::vector<float> arena(27 + 8 * 27 + 27), out(64 * 27);           // (a probe's worth of room on either side of the source)
    float *const srcp = arena.data() + 27;
    const size_t bytes = out.size() * sizeof(float);
    CHECK(probe_source_args(&G, srcp, 64, out.data(), bytes) == nullptr);
    CHECK(probe_source_args(nullptr, srcp, 64, out.data(), bytes) != nullptr && probe_source_args(nullptr, srcp, 0, out.data(), 0) != nullptr);
    CHECK(probe_source_args(&G, nullptr, 64, out.data(), bytes) != nullptr && probe_source_args(&G, nullptr, 0, nullptr, 0) == nullptr);
    ProbeGrid bad = G;
    bad.dims[1] = 0;
    CHECK(probe_source_args(&bad, srcp, 64, out.data(), bytes) != nullptr && probe_source_args(&bad, srcp, 0, out.data(), 0) != nullptr);
    bad = G;
    bad.step[2] = std::numeric_limits<float>::quiet_NaN();
    CHECK(probe_source_args(&bad, srcp, 64, out.data(), bytes) != nullptr);
    // an output that shares the last byte / the first byte of the source, and one that ends where the source begins
    const char *s0 = reinterpret_cast<const char *>(srcp);
    CHECK(probe_source_args(&G, srcp, 1, s0 + 8 * 27 * 4 - 1, 108) != nullptr && probe_source_args(&G, srcp, 1, s0 - 107, 108) != nullptr);
    CHECK(probe_source_args(&G, srcp, 1, s0 + 8 * 27 * 4, 108) == nullptr && probe_source_args(&G, srcp, 1, s0 - 108, 108) == nullptr);
    CHECK(probe_source_args(&G, srcp, 64, srcp, bytes) != nullptr);
}

static void put(std::FILE *f, const void *p, const size_t bytes) { CHECK(std::fwrite(p, 1, bytes, f) == bytes); }

static void write_fixture(const char *path) {
    std::FILE *f = std::fopen(path, "wb");
    CHECK(f != nullptr);
    if (!f) return;
    rng_state = 77u;
    const int32_t points = 600;
    for (int single : {0, 2, 5}) {
        const Volume v = volume(single, single == 5);
        int32_t head[16] = {0x42504c42, v.G.dims[0], v.G.dims[1], v.G.dims[2], points};
        std::memcpy(head + 5, v.G.origin, 12);
        std::memcpy(head + 8, v.G.step, 12);
        put(f, head, sizeof head);
        put(f, v.coeff.data(), v.coeff.size() * sizeof(float));
        for (int32_t i = 0; i < points; ++i) {
            float rec[6], kd[3], R[3], after[3], I[3];
            point(v.G, i % 5 == 1 ? 1 : (i % 37 == 5 ? 2 : 0), rec);
            normal(i % 41 == 7 ? 3 : 0, rec + 3);
            const uint32_t vis = rnd() & 0xffu, mode = static_cast<uint32_t>(i & 1);
            for (int c = 0; c < 3; ++c) { kd[c] = unit(); R[c] = unit() * 2.0f; }
            probe_bounce_lookup(v.G, v.coeff.data(), rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], mode != 0u, vis, I);
            for (int c = 0; c < 3; ++c) after[c] = probe_bounce_add(R[c], kd[c], I[c]);
            put(f, rec, sizeof rec); put(f, &vis, 4); put(f, &mode, 4); put(f, kd, 12); put(f, R, 12); put(f, after, 12);
        }
    }
    CHECK(std::fclose(f) == 0);
}

int main(int argc, char **argv) {
    check_streamed_blend();
    check_clamp();
    check_arguments();
    if (argc > 1) write_fixture(argv[1]);
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all checks held\n");
    return 0;
}
