// Stand-alone host check of rt_probe_layout.hpp (the task map and the carried sums of k_probes, the table offsets, the probe grid, the
// lookup arithmetic and the argument rules of the light-probe calls), meant for a sanitizer build on the CPU:
//   g++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iraytracer-in-cpp_amd/csrc tools/probe_layout_check.cpp -o probe_layout_check
// (make -C raytracer-in-cpp_amd/csrc probe_check builds and runs it).  Exit status 0: every check held.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "rt_probe_layout.hpp"

using namespace rtamd;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// The sums of a unit as the kernel takes them.  Every lane stages what it holds -- here the pair (probe, direction) -- in an array of 64
// entries per round; the task lanes of every pass read their probe's range of it; one array of 27 entries carries the running values of
// the one probe that goes on into the next round.  A "running value" here is the list of directions added so far, so that the order
// shows.  Every read must stay inside its array (the vectors' at() and the sanitizer see to that), every sum must end up as the
// directions 0 .. K - 1 of its probe in this order, be stored exactly once, and a carried value must be the one written one round before
// for the same (probe, sum).
static void sums(const int32_t m) {
    const AoLayout L = ao_layout(m);
    std::vector<int32_t> stored(static_cast<size_t>(L.group) * kProbeCoeffs, 0);
    struct Running { int32_t p, jc, next; };
    std::vector<Running> carry(kProbeCoeffs, Running{-1, -1, -1});
    for (int32_t round = 0; round < L.rounds; ++round) {
        std::vector<int32_t> staged_p(64), staged_k(64);
        for (int32_t lane = 0; lane < 64; ++lane) {
            const AoSlot s = ao_slot(1 << 20, L, 0, round, lane);
            staged_p[lane] = s.p; staged_k[lane] = s.k;
        }
        const ProbeSpan span = probe_span(L, round);
        CHECK(span.first == staged_p.at(0) && span.first + span.count - 1 == staged_p.at(63) && span.count >= 1);
        const int32_t passes = probe_passes(span);
        CHECK(passes * 64 >= kProbeCoeffs * span.count && (passes - 1) * 64 < kProbeCoeffs * span.count);
        std::vector<Running> keep(64, Running{-1, -1, -1});           // per lane: at most one value goes on
        std::vector<int32_t> seen(static_cast<size_t>(span.count) * kProbeCoeffs, 0);
        for (int32_t pass = 0; pass < passes; ++pass)
            for (int32_t lane = 0; lane < 64; ++lane) {
                const ProbeTask t = probe_task(span, pass, lane);
                if (!t.live) continue;
                CHECK(t.p >= span.first && t.p < span.first + span.count && t.p < L.group && t.jc >= 0 && t.jc < kProbeCoeffs);
                ++seen.at(static_cast<size_t>(t.p - span.first) * kProbeCoeffs + t.jc);
                int32_t next = 0;
                if (probe_carried_in(L, t.p, round)) {
                    const Running &c = carry.at(t.jc);
                    CHECK(c.p == t.p && c.jc == t.jc);
                    next = c.next;
                }
                const GatherRange r = gather_range(L, t.p, round);
                CHECK(r.count >= 1 && r.first >= 0 && r.first + r.count <= 64 && r.k0 == next);
                for (int32_t q = r.first; q < r.first + r.count; ++q) {
                    CHECK(staged_p.at(q) == t.p && staged_k.at(q) == next);
                    CHECK((r.k0 + (q - r.first)) * kProbeBasis + t.jc / 3 < L.K * kProbeBasis);         // the weight read
                    ++next;
                }
                if (probe_finished(L, t.p, round)) {
                    CHECK(next == L.K);
                    ++stored.at(static_cast<size_t>(t.p) * kProbeCoeffs + t.jc);
                } else {
                    CHECK(t.p == span.first + span.count - 1 && next < L.K && keep.at(lane).p < 0);
                    keep.at(lane) = Running{t.p, t.jc, next};
                }
            }
        for (const int32_t s : seen) CHECK(s == 1);
        for (const Running &k : keep)
            if (k.p >= 0) carry.at(k.jc) = k;
    }
    for (const int32_t s : stored) CHECK(s == 1);
    if (L.rounds == 1)
        for (int32_t p = 0; p < L.group; ++p) CHECK(!probe_carried_in(L, p, 0) && probe_finished(L, p, 0));
}

static bool same(const float a, const float b) { return a == b && std::signbit(a) == std::signbit(b); }

int main() {
    for (int32_t m = 1; m <= kAoMaxGrid; ++m) sums(m);
    // the tables: back to back, the weights behind the directions
    CHECK(probe_dir_offset(1) == 0u && probe_dir_offset(2) == 3u && probe_weight_offset(1) == kAoDirEntries * 3u && probe_weight_offset(2) == kAoDirEntries * 3u + 9u);
    CHECK(probe_dir_offset(16) + 256u * 3u == kAoDirEntries * 3u && probe_weight_offset(16) + 256u * 9u == kProbeTableFloats);
    CHECK(kProbeTableFloats * sizeof(float) == 71808u);
    CHECK(probe_out(0x7fffffffull) == 0x7fffffffull * 27ull);
    // the basis and the bands
    float Y[kProbeBasis];
    probe_sh9(0.0f, 0.0f, 1.0f, Y);
    CHECK(Y[0] == kShC0 && Y[1] == 0.0f && Y[2] == kShC1 && Y[3] == 0.0f && Y[4] == 0.0f && Y[5] == 0.0f && Y[6] == kShC3 * 2.0f && Y[7] == 0.0f && Y[8] == 0.0f);
    CHECK(probe_direct_band(0) == 3.14159274f && probe_direct_band(1) == 2.09439510f && probe_direct_band(3) == 2.09439510f && probe_direct_band(4) == 0.785398163f &&
          probe_direct_band(8) == 0.785398163f);
    // the grid rule
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    ProbeGrid G{{0.0f, 1.0f, 2.0f}, {1.0f, 0.5f, 2.0f}, {2, 3, 1}};
    CHECK(probe_grid_bad(G) == nullptr && probe_cells(G) == 6);
    for (int q = 0; q < 3; ++q) {
        ProbeGrid B = G;
        B.dims[q] = 0; CHECK(probe_grid_bad(B) != nullptr);
        B = G; B.step[q] = 0.0f; CHECK(probe_grid_bad(B) != nullptr);
        B.step[q] = -1.0f; CHECK(probe_grid_bad(B) != nullptr);
        B.step[q] = inf; CHECK(probe_grid_bad(B) != nullptr);
        B.step[q] = nan; CHECK(probe_grid_bad(B) != nullptr);
    }
    ProbeGrid big = G;
    big.dims[0] = 256; big.dims[1] = 256; big.dims[2] = 256; CHECK(probe_grid_bad(big) == nullptr);
    big.dims[2] = 257; CHECK(probe_grid_bad(big) != nullptr);
    big.dims[0] = big.dims[1] = big.dims[2] = 0x7fffffff; CHECK(probe_grid_bad(big) != nullptr);          // (no overflow on the way)
    CHECK(probe_index(G, 1, 2, 0) == 5 && probe_position(G, 1, 2) == 2.0f && probe_position(G, 2, 0) == 2.0f);
    // one axis: on a probe, between two, outside, NaN, a single layer
    ProbeAxis a = probe_axis(1.0f, 1.0f, 0.5f, 3);
    CHECK(a.i0 == 0 && a.w0 == 1.0f && a.w1 == 0.0f);
    a = probe_axis(1.75f, 1.0f, 0.5f, 3); CHECK(a.i0 == 1 && a.w0 == 0.5f && a.w1 == 0.5f);
    a = probe_axis(2.0f, 1.0f, 0.5f, 3); CHECK(a.i0 == 1 && a.w0 == 0.0f && a.w1 == 1.0f);             // the last probe: the far corner of the last cell
    a = probe_axis(9.0f, 1.0f, 0.5f, 3); CHECK(a.i0 == 1 && a.w0 == 0.0f && a.w1 == 1.0f);
    a = probe_axis(inf, 1.0f, 0.5f, 3); CHECK(a.i0 == 1 && a.w1 == 1.0f);
    a = probe_axis(-9.0f, 1.0f, 0.5f, 3); CHECK(a.i0 == 0 && a.w0 == 1.0f && same(a.w1, 0.0f));
    a = probe_axis(nan, 1.0f, 0.5f, 3); CHECK(a.i0 == 0 && a.w0 == 1.0f && same(a.w1, 0.0f));
    a = probe_axis(7.0f, 2.0f, 2.0f, 1); CHECK(a.i0 == 0 && a.w0 == 1.0f && same(a.w1, 0.0f));
    // the lookup on the 2 x 3 x 1 grid: coefficient jc of probe i is i * 100 + jc; a vector, so that a read outside it shows
    std::vector<float> C(static_cast<size_t>(probe_cells(G)) * kProbeCoeffs);
    for (size_t i = 0; i < C.size(); ++i) C[i] = static_cast<float>((i / kProbeCoeffs) * 100 + i % kProbeCoeffs);
    const auto eval = [&](const std::vector<float> &B, const float nx, const float ny, const float nz, const int c) {
        float y[kProbeBasis], o = 0.0f;
        probe_sh9(nx, ny, nz, y);
        for (int j = 0; j < kProbeBasis; ++j) o = o + B[static_cast<size_t>(j) * 3 + c] * y[j];
        return o;
    };
    float out[3];
    for (int32_t iy = 0; iy < 3; ++iy)
        for (int32_t ix = 0; ix < 2; ++ix) {                 // on a probe, at any z: that probe's coefficients
            probe_lookup(G, C.data(), probe_position(G, 0, ix), probe_position(G, 1, iy), -77.0f, 0.6f, 0.0f, 0.8f, out);
            const size_t i = static_cast<size_t>(probe_index(G, ix, iy, 0));
            const std::vector<float> B(C.begin() + i * kProbeCoeffs, C.begin() + (i + 1) * kProbeCoeffs);
            for (int c = 0; c < 3; ++c) CHECK(out[c] == eval(B, 0.6f, 0.0f, 0.8f, c));
        }
    probe_lookup(G, C.data(), 0.5f, 1.25f, 0.0f, 0.0f, 1.0f, 0.0f, out);              // the middle of cell (0, 0): a quarter of each corner
    {
        std::vector<float> B(kProbeCoeffs);
        for (int jc = 0; jc < kProbeCoeffs; ++jc) B[jc] = (0.0f + jc) * 0.25f + (100.0f + jc) * 0.25f + (200.0f + jc) * 0.25f + (300.0f + jc) * 0.25f;
        for (int c = 0; c < 3; ++c) CHECK(std::fabs(out[c] - eval(B, 0.0f, 1.0f, 0.0f, c)) <= 1e-3f);
    }
    probe_lookup(G, C.data(), nan, nan, nan, 0.0f, 0.0f, 1.0f, out);                    // NaN coordinates: cell 0, probe 0
    {
        const std::vector<float> B(C.begin(), C.begin() + kProbeCoeffs);
        for (int c = 0; c < 3; ++c) CHECK(out[c] == eval(B, 0.0f, 0.0f, 1.0f, c));
    }
    out[0] = out[1] = out[2] = 5.0f;
    probe_lookup(G, nullptr, 0.5f, 1.25f, 0.0f, 0.0f, -0.0f, 0.0f, out);                // no point: nothing is read
    CHECK(same(out[0], 0.0f) && same(out[1], 0.0f) && same(out[2], 0.0f));
    // the argument rules
    float p[64], cf[27 * 8], o[64], nrm[64];
    CHECK(probe_args(4, p, 3, cf) == nullptr && probe_args(0, nullptr, 3, nullptr) == nullptr);
    CHECK(probe_args(-1, p, 3, cf) != nullptr && probe_args(4, p, 0, cf) != nullptr && probe_args(4, p, 17, cf) != nullptr && probe_args(0, nullptr, 0, nullptr) != nullptr);
    CHECK(probe_args(4, p, 1, cf) == nullptr && probe_args(4, p, 16, cf) == nullptr);
    CHECK(probe_args(4, nullptr, 3, cf) != nullptr && probe_args(4, p, 3, nullptr) != nullptr);
    CHECK(probe_args(2, cf + 53, 3, cf) != nullptr && probe_args(2, cf + 54, 3, cf) == nullptr);          // the last float of the output / directly behind it
    CHECK(probe_args(4, p, 3, p + 11) != nullptr && probe_args(4, p, 3, p + 12) == nullptr);
    CHECK(probe_lookup_args(&G, cf, 4, p, nrm, o) == nullptr && probe_lookup_args(&G, nullptr, 0, nullptr, nullptr, nullptr) == nullptr);
    CHECK(probe_lookup_args(nullptr, cf, 4, p, nrm, o) != nullptr && probe_lookup_args(&G, cf, -1, p, nrm, o) != nullptr);
    ProbeGrid B = G;
    B.dims[1] = 0;
    CHECK(probe_lookup_args(&B, cf, 4, p, nrm, o) != nullptr && probe_lookup_args(&B, nullptr, 0, nullptr, nullptr, nullptr) != nullptr);
    CHECK(probe_lookup_args(&G, nullptr, 4, p, nrm, o) != nullptr && probe_lookup_args(&G, cf, 4, nullptr, nrm, o) != nullptr &&
          probe_lookup_args(&G, cf, 4, p, nullptr, o) != nullptr && probe_lookup_args(&G, cf, 4, p, nrm, nullptr) != nullptr);
    CHECK(probe_lookup_args(&G, cf, 4, p, nrm, p) != nullptr && probe_lookup_args(&G, cf, 4, p, nrm, nrm + 11) != nullptr && probe_lookup_args(&G, cf, 4, p, nrm, nrm + 12) == nullptr);
    CHECK(probe_lookup_args(&G, cf, 4, p, nrm, cf + 6 * 27 - 1) != nullptr && probe_lookup_args(&G, cf, 4, p, nrm, cf + 6 * 27) == nullptr);   // coeff counts as an input of 6 probes
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("rt_probe_layout.hpp: all checks held\n");
    return 0;
}
