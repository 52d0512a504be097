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

// ---- the visible lookup (rt_probe_irradiance_visible_device, k_probe_lookup_visible; DESIGN.md §5, Leak-free probe lookup) ---------------
// corner b = 4 dz + 2 dy + dx of a cell; bit b of the read mask: the corner is read (its index does not repeat because dims_q == 1)
RT_QUERY_HD uint32_t probe_read_mask(const ProbeGrid &G) {
    uint32_t m = 0xffu;
    if (G.dims[0] == 1) m &= 0x55u;
    if (G.dims[1] == 1) m &= 0x33u;
    if (G.dims[2] == 1) m &= 0x0fu;
    return m;
}
RT_QUERY_HD float probe_corner_weight(const ProbeAxis &ax, const ProbeAxis &ay, const ProbeAxis &az, const int32_t b) {
    return (((b & 4) ? az.w1 : az.w0) * ((b & 2) ? ay.w1 : ay.w0)) * ((b & 1) ? ax.w1 : ax.w0);
}
// Steps 5 and 6 of the header, the choice: which corners the blend adds and whether it divides by their weight.  read: the corners read;
// vis: those judged visible; positive: those of weight > 0.  Case A (every read corner visible, or none USED): all read corners, no
// division -- the plain lookup.  Case B: the USED corners, then the division by W.
struct ProbeUse {
    uint32_t use;
    bool divide;
};
RT_QUERY_HD ProbeUse probe_visible_use(const uint32_t read, const uint32_t vis, const uint32_t positive) {
    const uint32_t seen = vis & read, used = seen & positive;
    if (seen == read || used == 0u) return ProbeUse{read, false};
    return ProbeUse{used, true};
}
// Steps 1 to 6 of the header given the eight visibility bits `vis` (bit b: corner b is visible; bits of corners not read are ignored):
// the blend over the corners probe_visible_use names, evaluated at N.  Returns the mask byte.  k_probe_lookup_visible runs the same steps
// from the same parts (probe_axis, probe_read_mask, probe_corner_weight, probe_visible_use, probe_sh9_at), one sum per lane task.
RT_QUERY_HD uint32_t probe_lookup_visible(const ProbeGrid &G, const float *coeff, const float px, const float py, const float pz, const float nx,
                                          const float ny, const float nz, const uint32_t vis, float out[3]) {
    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
    if ((nx == 0.0f) & (ny == 0.0f) & (nz == 0.0f)) return 0u;
    const ProbeAxis ax = probe_axis(px, G.origin[0], G.step[0], G.dims[0]), ay = probe_axis(py, G.origin[1], G.step[1], G.dims[1]),
                    az = probe_axis(pz, G.origin[2], G.step[2], G.dims[2]);
    const uint32_t read = probe_read_mask(G);
    float w[8];
    uint32_t positive = 0u;
    for (int32_t b = 0; b < 8; ++b) {
        w[b] = probe_corner_weight(ax, ay, az, b);
        if (w[b] > 0.0f) positive |= 1u << b;
    }
    const ProbeUse u = probe_visible_use(read, vis, positive);
    float B[kProbeCoeffs], W = 0.0f;
    for (int32_t jc = 0; jc < kProbeCoeffs; ++jc) B[jc] = 0.0f;
    for (int32_t b = 0; b < 8; ++b) {
        if (!((u.use >> b) & 1u)) continue;
        const float *C = coeff + static_cast<size_t>(probe_index(G, ax.i0 + (b & 1), ay.i0 + ((b >> 1) & 1), az.i0 + (b >> 2))) * static_cast<size_t>(kProbeCoeffs);
        W = W + w[b];
        for (int32_t jc = 0; jc < kProbeCoeffs; ++jc) B[jc] = B[jc] + w[b] * C[jc];
    }
    for (int32_t j = 0; j < kProbeBasis; ++j) {
        const float y = probe_sh9_at(j, nx, ny, nz);
        for (int32_t c = 0; c < 3; ++c) out[c] = out[c] + B[j * 3 + c] * y;
    }
    if (u.divide)
        for (int32_t c = 0; c < 3; ++c) out[c] = out[c] / W;
    return vis & read;
}

// The kernel's mapping.  A wave unit is 8 consecutive points; lane l walks the segment of point l >> 3 of the unit, corner l & 7, so one
// ballot holds the unit's 64 answers and byte p of it is the mask of point p.  The 8 x 27 blended coefficients are lane tasks numbered
// point-major (t = p * 27 + jc) and taken 64 at a time, 4 passes; task t stores its sum at float t of the wave's staging slice: the 32
// lanes of a half-wave store 32 consecutive floats, one per bank.  The 8 x 3 evaluations are tasks of the lanes (p, corner c < 3), which
// hold their point's normal already: lane p * 8 + c reads floats p * 27 + j * 3 + c, and within a half-wave (4 points) 27 p + c takes 12
// distinct values modulo 32, so these reads meet in no bank either.
constexpr int32_t kPvPoints = 8, kPvTasks = kPvPoints * kProbeCoeffs, kPvPasses = (kPvTasks + 63) / 64, kPvStageFloats = kPvTasks + 128;
RT_QUERY_HD int32_t pv_lane_point(const int32_t lane) { return lane >> 3; }
RT_QUERY_HD int32_t pv_lane_corner(const int32_t lane) { return lane & 7; }
RT_QUERY_HD uint64_t pv_units(const int32_t n) { return n <= 0 ? 0u : (static_cast<uint64_t>(n) + kPvPoints - 1u) / kPvPoints; }
RT_QUERY_HD ProbeTask pv_task(const int32_t pass, const int32_t lane) {
    const int32_t t = pass * 64 + lane, p = t / kProbeCoeffs;
    return ProbeTask{p, t - p * kProbeCoeffs, t < kPvTasks};
}
RT_QUERY_HD int32_t pv_stage(const int32_t p, const int32_t jc) { return p * kProbeCoeffs + jc; }
// behind the sums: the weight and the probe index of the corner that lane `lane` walked (lane-linear: a wave's stores meet in no bank; the
// tasks of a half-wave belong to at most 3 points, so their reads of corner k of their point are broadcasts of at most 3 words)
RT_QUERY_HD int32_t pv_stage_weight(const int32_t lane) { return kPvTasks + lane; }
RT_QUERY_HD int32_t pv_stage_cell(const int32_t lane) { return kPvTasks + 64 + lane; }
// the lane that evaluates channel c of point p, and whether a lane is such a task (its channel is its corner)
RT_QUERY_HD int32_t pv_final_lane(const int32_t p, const int32_t c) { return p * 8 + c; }
RT_QUERY_HD bool pv_final(const int32_t lane) { return pv_lane_corner(lane) < 3; }
// grid of k_probe_lookup_visible: ao_grid's rule over units of one round
RT_QUERY_HD int32_t pv_grid(const int32_t n, const int32_t cus) { return ao_grid(pv_units(n), cus, 1); }

// ---- bounced light (rt_light_probes_bounce_device, rt_indirect_diffuse_bounce_device; DESIGN.md §5, Bounced light) ---------------------------
// The lookup of a source volume at a hit, ONE LANE = ONE LOOKUP, without the 27 blended values of probe_lookup in registers: the blend is
// streamed per (j, c) -- B[j][c] over the corners in order, then out_c = out_c + B[j][c] * Y[j] -- so a lane holds three accumulators, one
// running B, the eight weights and the index of the near corner.  Every B[j][c], every out_c and W take their additions in the order of
// probe_lookup / probe_lookup_visible, so the result is theirs bit for bit (tools/probe_bounce_check.cpp).  use: the corners the blend adds
// (a subset of the read corners: a corner that is not read has no index); divide: case B of the leak-free lookup.
// (probe_corner_weight's expression under a name of the bounce kernels' own: a second device caller of that function changes how it is
// inlined into k_probe_lookup_visible, whose instruction stream is to stay as it is)
RT_QUERY_HD float probe_bounce_weight(const ProbeAxis &ax, const ProbeAxis &ay, const ProbeAxis &az, const int32_t b) {
    return (((b & 4) ? az.w1 : az.w0) * ((b & 2) ? ay.w1 : ay.w0)) * ((b & 1) ? ax.w1 : ax.w0);
}
RT_QUERY_HD void probe_blend_streamed(const ProbeGrid &G, const float *coeff, const ProbeAxis &ax, const ProbeAxis &ay, const ProbeAxis &az, const uint32_t use,
                                      const bool divide, const float nx, const float ny, const float nz, float out[3]) {
    float w[8], W = 0.0f;
    for (int32_t b = 0; b < 8; ++b) {
        w[b] = probe_bounce_weight(ax, ay, az, b);
        if ((use >> b) & 1u) W = W + w[b];
    }
    const size_t base = static_cast<size_t>(probe_index(G, ax.i0, ay.i0, az.i0)) * static_cast<size_t>(kProbeCoeffs);
    const size_t sx = static_cast<size_t>(kProbeCoeffs), sy = sx * static_cast<size_t>(G.dims[0]), sz = sy * static_cast<size_t>(G.dims[1]);
    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
    for (int32_t j = 0; j < kProbeBasis; ++j) {
        const float y = probe_sh9_at(j, nx, ny, nz);
        for (int32_t c = 0; c < 3; ++c) {
            float B = 0.0f;
            for (int32_t b = 0; b < 8; ++b)
                if ((use >> b) & 1u)
                    B = B + w[b] * coeff[base + ((b & 1) ? sx : 0u) + ((b & 2) ? sy : 0u) + ((b & 4) ? sz : 0u) + static_cast<size_t>(j * 3 + c)];
            out[c] = out[c] + B * y;
        }
    }
    if (divide)
        for (int32_t c = 0; c < 3; ++c) out[c] = out[c] / W;
}
// the corners of weight > 0 of a cell, as bits
RT_QUERY_HD uint32_t probe_positive_mask(const ProbeAxis &ax, const ProbeAxis &ay, const ProbeAxis &az) {
    uint32_t positive = 0u;
    for (int32_t b = 0; b < 8; ++b)
        if (probe_bounce_weight(ax, ay, az, b) > 0.0f) positive |= 1u << b;
    return positive;
}
// I of the "bounced light" section: the source looked up at H with the turned face normal N.  visible == false: steps 1 to 5 of the plain
// lookup.  visible == true: steps 1 to 6 of the leak-free lookup given the eight answers `vis` (bits of corners not read are ignored).
RT_QUERY_HD void probe_bounce_lookup(const ProbeGrid &G, const float *coeff, const float hx, const float hy, const float hz, const float nx, const float ny,
                                     const float nz, const bool visible, const uint32_t vis, float out[3]) {
    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
    if ((nx == 0.0f) & (ny == 0.0f) & (nz == 0.0f)) return;                                 // no point
    const ProbeAxis ax = probe_axis(hx, G.origin[0], G.step[0], G.dims[0]), ay = probe_axis(hy, G.origin[1], G.step[1], G.dims[1]),
                    az = probe_axis(hz, G.origin[2], G.step[2], G.dims[2]);
    const uint32_t read = probe_read_mask(G);
    ProbeUse u{read, false};
    if (visible) u = probe_visible_use(read, vis, probe_positive_mask(ax, ay, az));
    probe_blend_streamed(G, coeff, ax, ay, az, u.use, u.divide, nx, ny, nz, out);
}
// b_c = smax(0.0f, I_c) (NaN and -0 give +0), then R_c = R_c + kd_c * b_c: one product, then the addition
RT_QUERY_HD float probe_bounce_add(const float R, const float kd, const float I) { return R + kd * ((0.0f < I) ? I : 0.0f); }
// the position of corner b of the cell of H, the far end of the segment that asks whether H sees that probe
RT_QUERY_HD void probe_corner_position(const ProbeGrid &G, const float hx, const float hy, const float hz, const int32_t b, float &cx, float &cy, float &cz) {
    cx = probe_position(G, 0, probe_axis(hx, G.origin[0], G.step[0], G.dims[0]).i0 + (b & 1));
    cy = probe_position(G, 1, probe_axis(hy, G.origin[1], G.step[1], G.dims[1]).i0 + ((b >> 1) & 1));
    cz = probe_position(G, 2, probe_axis(hz, G.origin[2], G.step[2], G.dims[2]).i0 + (b >> 2));
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
// (mask may be null; the two outputs must not share a byte with an input or with each other)
inline const char *probe_visible_args(const ProbeGrid *G, const void *coeff, const int32_t n, const void *point, const void *normal, const void *rgb,
                                      const void *mask) {
    if (const char *bad = probe_lookup_args(G, coeff, n, point, normal, rgb)) return bad;
    if (n == 0 || !mask) return nullptr;
    const size_t pts = static_cast<size_t>(n), v3 = pts * 3 * sizeof(float);
    if (query_any_overlap({{mask, pts}}, {{point, v3}, {normal, v3}, {coeff, static_cast<size_t>(probe_cells(*G)) * kProbeCoeffs * sizeof(float)}, {rgb, v3}}))
        return "the mask overlaps an input or the other output";
    return nullptr;
}

// the source of the bounce calls, checked behind the parent's own rule: a bad grid is refused whatever n is; out: the call's output
inline const char *probe_source_args(const ProbeGrid *src, const void *src_coeff, const int32_t n, const void *out, const size_t out_bytes) {
    if (!src) return "the source grid is null";
    if (const char *bad = probe_grid_bad(*src)) return bad;
    if (n == 0) return nullptr;
    if (!src_coeff) return "the source coefficients are null";
    if (query_any_overlap({{out, out_bytes}}, {{src_coeff, static_cast<size_t>(probe_cells(*src)) * kProbeCoeffs * sizeof(float)}}))
        return "the output overlaps the source";
    return nullptr;
}

}  // namespace rtamd
