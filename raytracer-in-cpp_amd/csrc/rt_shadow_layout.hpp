// rt_shadow_layout.hpp -- the arithmetic of the soft-shadow query (rt_soft_shadows_device; DESIGN.md §5, Soft shadows) that the host and
// k_soft_shadows share: the wave layout of rt_ao_layout.hpp (AoLayout, ao_units, ao_slot, ao_next, ao_point_lanes, ao_xyz) for a GENERAL number
// of segments per point K = n_lights * usteps * vsteps in 1 .. 25,600, how a lane's segment k becomes (light, grid row, grid column) and how
// that triple moves from one round to the next without a division, the grid, the per-point jitter and the argument rules of the calls.
// Header-only and free of HIP, so that tools/shadow_layout_check.cpp can run it under a sanitizer.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rt_ao_layout.hpp"

namespace rtamd {

constexpr int32_t kShadowMaxLights = 25, kShadowMaxSamples = 1024;      // RT_MAX_LIGHTS, RT_MAX_SAMPLES
constexpr int32_t kShadowMaxK = kShadowMaxLights * kShadowMaxSamples;   // 25,600: a count fits uint16_t
constexpr int32_t kShadowPoint = 0, kShadowArea = 1, kShadowSphere = 2; // RT_LIGHT_POINT, RT_LIGHT_AREA, RT_LIGHT_SPHERE

// The wave layout of K segments per point: g = gcd(K, 64), a unit of 64 / g points walked in K / g rounds (AoLayout's rule, for any K >= 1).
RT_QUERY_HD AoLayout shadow_wave_layout(const int32_t K) {
    int32_t g = 64;
    while (K % g != 0) g >>= 1;                            // gcd(K, 64)
    return AoLayout{K, 64 / g, K / g, 64 / K, 64 % K};
}

// Segment k of a point is sample s = k % N of light l = k / N, N = usteps * vsteps, and sample s is cell (i, j) = (s / vsteps, s % vsteps) of
// the light's grid: k = (l * usteps + i) * vsteps + j, a number of three digits in the mixed radix (n_lights, usteps, vsteps).  From one round
// to the next k grows by 64 % K modulo K (ao_next), so the digits grow by the digits (dl, di, dj) of 64 % K with carries, and the carry out of
// the top digit is ao_next's step to the next point: no division after the first round.  A point light is a 1 x 1 grid.
struct ShadowLayout {
    AoLayout A;
    int32_t n_lights, usteps, vsteps;
    int32_t dl, di, dj;      // 64 % K = (dl * usteps + di) * vsteps + dj
};
RT_QUERY_HD ShadowLayout shadow_layout(const int32_t n_lights, const int32_t usteps, const int32_t vsteps) {
    const int32_t N = usteps * vsteps;
    const AoLayout A = shadow_wave_layout(n_lights * N);
    const int32_t dl = A.r64 / N, ds = A.r64 - dl * N, di = ds / vsteps;
    return ShadowLayout{A, n_lights, usteps, vsteps, dl, di, ds - di * vsteps};
}
// (l, i, j) of segment k: three divisions, for a lane's first round only
struct ShadowCell {
    int32_t l, i, j;
};
RT_QUERY_HD ShadowCell shadow_cell(const ShadowLayout &L, const int32_t k) {
    const int32_t N = L.usteps * L.vsteps, l = k / N, s = k - l * N, i = s / L.vsteps;
    return ShadowCell{l, i, s - i * L.vsteps};
}
// a lane's point place p and cell in the next round: what ao_next does to (p, k), on the digits of k
RT_QUERY_HD void shadow_next(const ShadowLayout &L, int32_t &p, ShadowCell &c) {
    p += L.A.q64;
    c.j += L.dj;
    if (c.j >= L.vsteps) { c.j -= L.vsteps; ++c.i; }
    c.i += L.di;
    if (c.i >= L.usteps) { c.i -= L.usteps; ++c.l; }
    c.l += L.dl;
    if (c.l >= L.n_lights) { c.l -= L.n_lights; ++p; }
}
// grid of k_soft_shadows: ao_grid's rule (RT_WAVES = 4 units per block, a cap that grows with the rounds of a unit up to 4 times)
RT_QUERY_HD int32_t shadow_grid(const uint64_t units, const int32_t cus, const int32_t rounds) { return ao_grid(units, cus, rounds); }
// segments of a call, for the figures a caller reports (n * K leaves 32 bits)
RT_QUERY_HD uint64_t shadow_segments(const int32_t n, const int32_t K) { return n <= 0 || K <= 0 ? 0u : static_cast<uint64_t>(n) * static_cast<uint64_t>(K); }

// The per-point jitter of rt_shadow_jitter: g = the mixing of ao_hash once more over ao_hash(seed, i) ^ 0xB5297A4D; fu = (g >> 16) * 2^-16,
// fv = (g & 0xFFFF) * 2^-16, both exact and in [0, 1).
RT_QUERY_HD uint32_t shadow_hash(const uint32_t seed, const uint32_t i) {
    uint32_t g = ao_hash(seed, i) ^ 0xB5297A4Du;
    g ^= g >> 15; g *= 0x2C1B3C6Du; g ^= g >> 12; g *= 0x297A2D39u; g ^= g >> 15;
    return g;
}
RT_QUERY_HD void shadow_jitter(const uint32_t seed, const uint32_t i, float &fu, float &fv) {
    const uint32_t g = shadow_hash(seed, i);
    fu = static_cast<float>(g >> 16) * 1.52587890625e-05f;            // 2^-16
    fv = static_cast<float>(g & 0xFFFFu) * 1.52587890625e-05f;
}

// The argument rules.  0: valid; else the rule that failed, as a text for rt_last_error.
// the lights, as check_lights (rt_capi.cpp) checks a point or area light; sphere mode is the caller's to refuse beforehand
inline const char *shadow_light_args(const int32_t n_lights, const int32_t mode, const int32_t usteps, const int32_t vsteps) {
    if (n_lights < 1 || n_lights > kShadowMaxLights) return "n_lights must be in 1..25";
    if (mode != kShadowPoint && mode != kShadowArea && mode != kShadowSphere) return "mode must be point, area or sphere";
    if (mode == kShadowArea && (usteps < 1 || vsteps < 1 || static_cast<int64_t>(usteps) * vsteps > kShadowMaxSamples)) return "usteps*vsteps must be in 1..1024";
    return nullptr;
}
// (an offset is tested as !(f >= 0 && f < 1) so that NaN fails)
inline const char *shadow_args(const int32_t n, const void *point, const void *normal, const bool has_params, const int32_t per_point, const float fu,
                               const float fv, const void *visible, const void *share) {
    if (!has_params) return "the parameters are null";
    if (n < 0) return "n is negative";
    if (per_point == 0 && (!(fu >= 0.0f && fu < 1.0f) || !(fv >= 0.0f && fv < 1.0f))) return "fu and fv must be in [0, 1)";
    if (n == 0) return nullptr;
    if (!point) return "point is null";
    if (!visible && !share) return "visible and share are both null";
    const size_t in = static_cast<size_t>(n) * 3 * sizeof(float);
    if (query_any_overlap({{visible, static_cast<size_t>(n) * 2}, {share, static_cast<size_t>(n) * 4}}, {{point, in}, {normal, in}})) return "an output overlaps an input";
    return nullptr;
}

}  // namespace rtamd
