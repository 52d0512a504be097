// rt_probe_layout.hpp -- the arithmetic of the light-probe queries (rt_light_probes_device, rt_probe_irradiance_device; DESIGN.md §5, Light
// probes) that the host, k_probes and k_probe_lookup share.  k_probes takes k_gather's mapping whole (rt_ao_layout.hpp: AoLayout, ao_units,
// ao_next, ao_xyz, ao_grid; rt_gather_layout.hpp: gather_range); what it adds is here: which probes have lanes in a round, the map from a
// task lane to the (probe, coefficient, channel) whose sum it takes, when a sum is carried into or out of a round, the offsets of the two
// tables, the float32 basis, the probe grid with its lookup (the blend and the evaluation, as the kernel runs them) and the argument rules of
// the calls.  Header-only and free of HIP, so that tools/probe_layout_check.cpp can run it under a sanitizer.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rt_ao_layout.hpp"
#include "rt_gather_layout.hpp"

namespace rtamd {

constexpr int32_t kProbeCoeffs = 27, kProbeBasis = 9;       // RT_PROBE_COEFFS; coefficient j, channel c of a probe is float j * 3 + c
constexpr int32_t kProbeMaxCells = 1 << 24;                 // probes of a grid

// The device tables, one float array: the directions of m = 1 .. 16 back to back (xyz per entry), then their weights (9 per entry).
constexpr uint32_t kProbeTableFloats = kAoDirEntries * 3u + kAoDirEntries * 9u;
RT_QUERY_HD uint32_t probe_dir_offset(const int32_t m) { return ao_dir_offset(m) * 3u; }                                // first float
RT_QUERY_HD uint32_t probe_weight_offset(const int32_t m) { return kAoDirEntries * 3u + ao_dir_offset(m) * 9u; }        // first float

// ---- the 27 sums of a probe as lane tasks ----------------------------------------------------------------------------------------------
// Lane l of round r holds ray e = r * 64 + l of the unit, e = p * K + k: the probes with a lane in round r are consecutive, p = first ..
// first + count - 1.  Of these only the first can have begun in an earlier round and only the last can go on into the next one, so one
// probe's 27 running values are all that a wave carries from a round to the next.
struct ProbeSpan {
    int32_t first, count;
};
RT_QUERY_HD ProbeSpan probe_span(const AoLayout &L, const int32_t round) {
    const int32_t lo = (round * 64) / L.K, hi = (round * 64 + 63) / L.K;
    return ProbeSpan{lo, hi - lo + 1};
}
// The tasks of a round are (probe of the span, jc = j * 3 + c), 27 * count of them, numbered probe-major and taken 64 at a time: lane `lane`
// of pass `pass` takes task pass * 64 + lane.
RT_QUERY_HD int32_t probe_passes(const ProbeSpan &s) { return (kProbeCoeffs * s.count + 63) / 64; }
struct ProbeTask {
    int32_t p, jc;        // the probe's place in the unit, the sum
    bool live;            // the lane has a task in this pass
};
RT_QUERY_HD ProbeTask probe_task(const ProbeSpan &s, const int32_t pass, const int32_t lane) {
    const int32_t t = pass * 64 + lane, q = t / kProbeCoeffs;
    return ProbeTask{s.first + q, t - q * kProbeCoeffs, t < kProbeCoeffs * s.count};
}
// the sum of probe p begins with the carried value in round `round` (else with +0.0f) / is complete at the end of it (else it is carried on)
RT_QUERY_HD bool probe_carried_in(const AoLayout &L, const int32_t p, const int32_t round) { return p * L.K < round * 64; }
RT_QUERY_HD bool probe_finished(const AoLayout &L, const int32_t p, const int32_t round) { return (p + 1) * L.K <= (round + 1) * 64; }
// first float of probe i in a float[n * 27] array
RT_QUERY_HD size_t probe_out(const uint64_t i) { return static_cast<size_t>(i) * static_cast<size_t>(kProbeCoeffs); }

// ---- the float32 basis (rt_sh9): every operation on its own, in the order of the header --------------------------------------------------
constexpr float kShC0 = 0.282094792f, kShC1 = 0.488602512f, kShC2 = 1.092548431f, kShC3 = 0.315391565f, kShC4 = 0.546274215f;
RT_QUERY_HD float probe_sh9_at(const int32_t j, const float x, const float y, const float z) {
    switch (j) {
    case 0: return kShC0;
    case 1: return kShC1 * y;
    case 2: return kShC1 * z;
    case 3: return kShC1 * x;
    case 4: return kShC2 * (x * y);
    case 5: return kShC2 * (y * z);
    case 6: return kShC3 * ((3.0f * (z * z)) - 1.0f);
    case 7: return kShC2 * (x * z);
    default: return kShC4 * ((x * x) - (y * y));
    }
}
RT_QUERY_HD void probe_sh9(const float x, const float y, const float z, float out[kProbeBasis]) {
    for (int32_t j = 0; j < kProbeBasis; ++j) out[j] = probe_sh9_at(j, x, y, z);
}
// b_j of the direct term: pi, 2 pi / 3, pi / 4 per band
RT_QUERY_HD float probe_direct_band(const int32_t j) { return j == 0 ? 3.14159274f : (j < 4 ? 2.09439510f : 0.785398163f); }

// ---- the probe grid and its lookup -------------------------------------------------------------------------------------------------------
struct ProbeGrid {            // rt_probe_grid, member for member
    float origin[3], step[3];
    int32_t dims[3];
};
// 0: valid; else the rule that failed
inline const char *probe_grid_bad(const ProbeGrid &G) {
    int64_t cells = 1;
    for (int q = 0; q < 3; ++q) {
        if (G.dims[q] < 1) return "every dimension of the grid must be >= 1";
        if (!(G.step[q] > 0.0f) || G.step[q] > 3.402823466e+38f) return "every step of the grid must be finite and > 0";
        cells *= G.dims[q];
        if (cells > kProbeMaxCells) return "the grid has more than 2^24 probes";
    }
    return nullptr;
}
RT_QUERY_HD int64_t probe_cells(const ProbeGrid &G) { return static_cast<int64_t>(G.dims[0]) * G.dims[1] * G.dims[2]; }       // of a valid grid
RT_QUERY_HD int32_t probe_index(const ProbeGrid &G, const int32_t ix, const int32_t iy, const int32_t iz) { return (iz * G.dims[1] + iy) * G.dims[0] + ix; }
RT_QUERY_HD float probe_position(const ProbeGrid &G, const int32_t q, const int32_t i) { return G.origin[q] + static_cast<float>(i) * G.step[q]; }

// one axis of the cell of a point: the near corner and the two weights
struct ProbeAxis {
    int32_t i0;
    float w0, w1;
};
RT_QUERY_HD ProbeAxis probe_axis(const float p, const float origin, const float step, const int32_t dim) {
    float g = (p - origin) / step;
    g = (0.0f < g) ? g : 0.0f;                               // smax(0.0f, g): NaN and -0 give +0
    const float top = static_cast<float>(dim - 1);
    if (g > top) g = top;
    int32_t i0 = static_cast<int32_t>(g);
    const int32_t cap = dim - 2 > 0 ? dim - 2 : 0;
    if (i0 > cap) i0 = cap;
    const float f = g - static_cast<float>(i0);
    return ProbeAxis{i0, 1.0f - f, f};
}
// Steps 1 to 5 of the header: the blend of the (at most) 8 probes round P and its evaluation at N.  coeff: the probes of G, 27 floats each.
RT_QUERY_HD void probe_lookup(const ProbeGrid &G, const float *coeff, const float px, const float py, const float pz, const float nx, const float ny,
                              const float nz, float out[3]) {
    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
    if ((nx == 0.0f) & (ny == 0.0f) & (nz == 0.0f)) return;                                 // (+-0 both compare equal to 0)
    const ProbeAxis ax = probe_axis(px, G.origin[0], G.step[0], G.dims[0]), ay = probe_axis(py, G.origin[1], G.step[1], G.dims[1]),
                    az = probe_axis(pz, G.origin[2], G.step[2], G.dims[2]);
    float B[kProbeCoeffs];
    for (int32_t jc = 0; jc < kProbeCoeffs; ++jc) B[jc] = 0.0f;
    for (int32_t dz = 0; dz < (G.dims[2] == 1 ? 1 : 2); ++dz)
        for (int32_t dy = 0; dy < (G.dims[1] == 1 ? 1 : 2); ++dy)
            for (int32_t dx = 0; dx < (G.dims[0] == 1 ? 1 : 2); ++dx) {
                const float w = ((dz ? az.w1 : az.w0) * (dy ? ay.w1 : ay.w0)) * (dx ? ax.w1 : ax.w0);
                const float *C = coeff + static_cast<size_t>(probe_index(G, ax.i0 + dx, ay.i0 + dy, az.i0 + dz)) * static_cast<size_t>(kProbeCoeffs);
                for (int32_t jc = 0; jc < kProbeCoeffs; ++jc) B[jc] = B[jc] + w * C[jc];
            }
    for (int32_t j = 0; j < kProbeBasis; ++j) {
        const float y = probe_sh9_at(j, nx, ny, nz);
        for (int32_t c = 0; c < 3; ++c) out[c] = out[c] + B[j * 3 + c] * y;
    }
}

// ---- the argument rules.  0: valid; else the rule that failed, as a text for rt_last_error ------------------------------------------------
inline const char *probe_args(const int32_t n, const void *position, const int32_t m, const void *coeff) {
    if (n < 0) return "n is negative";
    if (!ao_grid_ok(m)) return "the grid size m must be in 1 .. 16";
    if (n == 0) return nullptr;
    if (!position || !coeff) return "a pointer is null";
    const size_t pts = static_cast<size_t>(n);
    if (query_any_overlap({{coeff, pts * kProbeCoeffs * sizeof(float)}}, {{position, pts * 3 * sizeof(float)}})) return "the output overlaps the input";
    return nullptr;
}
inline const char *probe_lookup_args(const ProbeGrid *G, const void *coeff, const int32_t n, const void *point, const void *normal, const void *rgb) {
    if (!G) return "grid is null";
    if (const char *bad = probe_grid_bad(*G)) return bad;
    if (n < 0) return "n is negative";
    if (n == 0) return nullptr;
    if (!coeff || !point || !normal || !rgb) return "a pointer is null";
    const size_t v3 = static_cast<size_t>(n) * 3 * sizeof(float);
    if (query_any_overlap({{rgb, v3}}, {{point, v3}, {normal, v3}, {coeff, static_cast<size_t>(probe_cells(*G)) * kProbeCoeffs * sizeof(float)}}))
        return "the output overlaps an input";
    return nullptr;
}

}  // namespace rtamd
