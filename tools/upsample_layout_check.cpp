// Stand-alone host check of rt_upsample_layout.hpp (the low size, the tap and nearest-pixel arithmetic, the scales and the argument rules of
// the guided upsample), meant for a sanitizer build on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iraytracer-in-cpp_amd/csrc tools/upsample_layout_check.cpp -o upsample_layout_check
// (make -C raytracer-in-cpp_amd/csrc upsample_check builds and runs it).  Exit status 0: every check held.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "rt_upsample_layout.hpp"

using namespace rtamd;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static uint32_t bits(const float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// one axis of `n` high pixels at factor s, coordinates [v0, v1): the taps and the nearest pixel of every coordinate, in 64-bit arithmetic
static void axis_holds(const int32_t n, const int32_t s, const int32_t v0, const int32_t v1) {
    const int32_t e = up_low_extent(n, s);
    CHECK(static_cast<int64_t>(e) * s >= n && (static_cast<int64_t>(e) - 1) * s < n);                     // e = ceil(n / s)
    for (int64_t v = v0; v < v1; ++v) {
        const UpTap T = up_tap(static_cast<int32_t>(v), s);
        CHECK(T.f >= 0 && T.f < s && static_cast<int64_t>(T.i0) * s + T.f == v);
        CHECK(T.i0 >= 0 && T.i0 < e);                                                                     // the first tap is always inside
        CHECK(up_tap_inside(T.i0, 0, e) && up_tap_coord(T.i0, 0, e) == T.i0);
        const bool in1 = static_cast<int64_t>(T.i0) + 1 < e;
        CHECK(up_tap_inside(T.i0, 1, e) == in1 && up_tap_coord(T.i0, 1, e) == (in1 ? T.i0 + 1 : T.i0));
        CHECK((static_cast<int64_t>(T.i0) + 1) * s < n ? in1 : true);                                     // a low pixel that lies on a high one exists
        const int32_t nr = up_nearest(static_cast<int32_t>(v), s, e);
        CHECK(nr >= 0 && nr < e && (nr == T.i0 || nr == T.i0 + 1));
        const int64_t d = v - static_cast<int64_t>(nr) * s;                                               // distance to the nearest, in high pixels
        CHECK(nr == e - 1 ? d >= -(s / 2) : (d < 0 ? -2 * d <= s : 2 * d < s));                           // a tie goes up
        if (T.f == 0) CHECK(nr == T.i0);                                                                  // on a low pixel: that pixel
    }
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    // the factor and the low size: sizes 1, s - 1, s, s + 1 and around a multiple, for every factor
    CHECK(!up_factor_ok(1) && !up_factor_ok(0) && !up_factor_ok(-2) && !up_factor_ok(9) && !up_factor_ok(INT32_MAX) && !up_factor_ok(INT32_MIN));
    for (int32_t s = 2; s <= kUpMaxFactor; ++s) {
        CHECK(up_factor_ok(s));
        CHECK(up_low_extent(0, s) == 0 && up_low_extent(1, s) == 1 && up_low_extent(s - 1, s) == 1 && up_low_extent(s, s) == 1 && up_low_extent(s + 1, s) == 2);
        CHECK(up_low_extent(7 * s, s) == 7 && up_low_extent(7 * s + 1, s) == 8 && up_low_extent(7 * s - 1, s) == 7);
        CHECK(up_low_extent(INT32_MAX, s) == static_cast<int32_t>((static_cast<int64_t>(INT32_MAX) + s - 1) / s));
        for (const int32_t n : {1, s - 1, s, s + 1, 2 * s, 2 * s + 1, 64, 65, 127, 131}) axis_holds(n, s, 0, n);
        // a width near INT32_MAX: the first and the last coordinates (2v + s is formed in 64 bits)
        for (const int32_t n : {INT32_MAX, INT32_MAX - 1, INT32_MAX - s, INT32_MAX - s + 1}) {
            axis_holds(n, s, 0, 70);
            axis_holds(n, s, n - 70, n);
        }
        int32_t w = -7, r = -7;
        CHECK(up_low_size(1, 1, s, &w, &r) && w == 1 && r == 1);
        CHECK(up_low_size(s + 1, s - 1, s, &w, &r) && w == 2 && r == 1);
        CHECK(up_low_size(1920, 1080, s, &w, &r) && w == (1920 + s - 1) / s && r == (1080 + s - 1) / s);
        CHECK(up_low_size(INT32_MAX, 0, s, &w, &r) && w == up_low_extent(INT32_MAX, s) && r == 0);
        w = r = -7;
        CHECK(!up_low_size(0, 4, s, &w, &r) && !up_low_size(-1, 4, s, &w, &r) && !up_low_size(4, -1, s, &w, &r) && w == -7 && r == -7);
    }
    {
        int32_t w = -7, r = -7;
        CHECK(!up_low_size(4, 4, 1, &w, &r) && !up_low_size(4, 4, 9, &w, &r) && !up_low_size(4, 4, 0, &w, &r) && !up_low_size(4, 4, -2, &w, &r) && w == -7 && r == -7);
    }
    // the pins' coordinates: width 4, s 2 and width 5, s 3
    CHECK(up_tap(3, 2).i0 == 1 && up_tap(3, 2).f == 1 && !up_tap_inside(1, 1, 2) && up_nearest(3, 2, 2) == 1 && up_nearest(1, 2, 2) == 1 && up_nearest(0, 2, 2) == 0);
    CHECK(up_tap(4, 3).i0 == 1 && up_tap(4, 3).f == 1 && up_nearest(1, 3, 2) == 0 && up_nearest(2, 3, 2) == 1 && up_nearest(4, 3, 2) == 1);

    // the scales: squared once; the depth scale times the factor; +inf stays +inf; a tiny sigma underflows to 0
    for (int32_t s = 2; s <= kUpMaxFactor; ++s) {
        const UpScales S = up_scales(0.75f, 0.0625f, 3.0f, s);
        const float sz = 0.0625f * static_cast<float>(s);
        CHECK(bits(S.sn2) == bits(0.5625f) && bits(S.sz2) == bits(sz * sz) && bits(S.sa2) == bits(9.0f));
        const UpScales I = up_scales(inf, inf, inf, s);
        CHECK(I.sn2 == inf && I.sz2 == inf && I.sa2 == inf);
        const UpScales Z = up_scales(1e-30f, 1e-30f, 1e-30f, s);
        CHECK(Z.sn2 == 0.0f && Z.sz2 == 0.0f && Z.sa2 == 0.0f);
    }
    CHECK(bits(up_scales(1.0f, 0.1f, 1.0f, 3).sz2) == bits((0.1f * 3.0f) * (0.1f * 3.0f)));
    CHECK(bits(up_scales(0.5f, 0.125f, 0.25f, 2).sz2) == bits(0.0625f));

    // the argument rules (pointers are only compared, never followed)
    alignas(16) static float arena[4096];
    alignas(16) static uint8_t marena[256];
    const int32_t w = 5, r = 3;                          // high 5 x 3 = 15 pixels: out 60 / 180 bytes, miss 15, high buffers 480; low 3 x 2 at s = 2: 24 / 72 and 192
    float *low = arena, *gl = arena + 64, *gh = arena + 256, *out = arena + 512;
    uint8_t *miss = marena;
    int32_t s2 = 2;
    float sg[3] = {0.5f, 0.0625f, inf};
    bool uns = true;
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out, miss, true, &uns) == nullptr && !uns);
    CHECK(up_args(low, 3, gl, gh, w, r, &s2, sg, out, miss, true, &uns) == nullptr);
    CHECK(up_args(low, 3, gl, gh, w, r, &s2, sg, out, nullptr, true, &uns) == nullptr);                 // the mask is optional
    CHECK(up_args(low, 3, gl, gh, w, r, &s2, sg, out, nullptr, false, &uns) == nullptr && up_args(low, 3, gl, gh, w, r, &s2, sg, out, miss, false, &uns) == nullptr);
    // every required pointer
    CHECK(up_args(nullptr, 1, gl, gh, w, r, &s2, sg, out, miss, true, &uns) && !uns);
    CHECK(up_args(low, 1, nullptr, gh, w, r, &s2, sg, out, miss, true, &uns) && up_args(low, 1, gl, nullptr, w, r, &s2, sg, out, miss, true, &uns));
    CHECK(up_args(low, 1, gl, gh, w, r, nullptr, sg, out, miss, true, &uns) && up_args(low, 1, gl, gh, w, r, &s2, nullptr, out, miss, true, &uns));
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, nullptr, miss, true, &uns) && up_args(low, 1, gl, gh, w, r, &s2, sg, nullptr, miss, false, &uns));
    // channels, width, rows, factor, sigmas
    for (const int32_t ch : {0, 2, 4, -1}) CHECK(up_args(low, ch, gl, gh, w, r, &s2, sg, out, miss, true, &uns) && !uns);
    CHECK(up_args(low, 1, gl, gh, 0, r, &s2, sg, out, miss, true, &uns) && up_args(low, 1, gl, gh, -3, r, &s2, sg, out, miss, true, &uns));
    CHECK(up_args(low, 1, gl, gh, w, -1, &s2, sg, out, miss, true, &uns) && !uns);
    CHECK(up_args(low, 1, gl, gh, w, 0, &s2, sg, out, miss, true, &uns) == nullptr);
    for (const int32_t bad : {1, 0, -1, 9, INT32_MAX, INT32_MIN}) { int32_t b = bad; CHECK(up_args(low, 1, gl, gh, w, r, &b, sg, out, miss, true, &uns) && !uns); }
    for (const int32_t good : {2, 3, 8}) { int32_t g = good; CHECK(up_args(low, 1, gl, gh, w, r, &g, sg, out, miss, true, &uns) == nullptr); }
    for (int k = 0; k < 3; ++k)
        for (const float bad : {0.0f, -0.0f, -1.0f, nan, -inf}) {
            float b[3] = {1.0f, 1.0f, 1.0f};
            b[k] = bad;
            CHECK(up_args(low, 1, gl, gh, w, r, &s2, b, out, miss, true, &uns) && !uns);
            CHECK(up_args(low, 1, gl, gh, w, r, &s2, b, out, miss, false, &uns) && !uns);
        }
    // the size: RT_ERR_UNSUPPORTED, in both forms; an empty image of any width is fine
    CHECK(up_args(low, 1, gl, gh, INT32_MAX, 2, &s2, sg, out, miss, true, &uns) && uns);
    CHECK(up_args(low, 3, gl, gh, 46341, 46341, &s2, sg, out, miss, false, &uns) && uns);
    CHECK(up_args(low, 1, gl, gh, INT32_MAX, 1, &s2, sg, out, nullptr, false, &uns) == nullptr && !uns);
    CHECK(up_args(low, 1, gl, gh, INT32_MAX, 0, &s2, sg, out, miss, true, &uns) == nullptr && !uns);
    // alignment of out and of both geometry buffers (the device form only); the low image and the mask have no alignment rule
    for (int k = 1; k < 4; ++k) {
        CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out + k, miss, true, &uns) && !uns);
        CHECK(up_args(low, 1, gl + k, gh, w, r, &s2, sg, out, miss, true, &uns) && up_args(low, 1, gl, gh + k, w, r, &s2, sg, out, miss, true, &uns));
        CHECK(up_args(low, 1, gl + k, gh + k, w, r, &s2, sg, out + k, miss, false, &uns) == nullptr);
        CHECK(up_args(low + k, 1, gl, gh, w, r, &s2, sg, out, miss + k, true, &uns) == nullptr);
    }
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out + 4, miss, true, &uns) == nullptr);
    // each overlap pair, by one byte at either end, and the neighbouring placement that shares none
    const uint64_t img1 = dn_image_bytes(w, r, 1), lb1 = dn_image_bytes(3, 2, 1), glb = dn_gbuffer_bytes(3, 2), ghb = dn_gbuffer_bytes(w, r);
    CHECK(img1 == 60 && lb1 == 24 && glb == 192 && ghb == 480 && up_miss_bytes(w, r) == 15);
    uint8_t *fb = reinterpret_cast<uint8_t *>(arena);                                                      // byte addresses inside the float arena
    auto at = [&](float *p) { return reinterpret_cast<uint8_t *>(p); };
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(out), true, &uns) && !uns);                       // out + k: the mask inside the output
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(out) + 59, true, &uns) && up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(out) + 60, true, &uns) == nullptr);
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(out) - 14, true, &uns) && up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(out) - 15, true, &uns) == nullptr);
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, low, miss, true, &uns));                                  // out == low
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, low + 4, miss, true, &uns) && up_args(low, 1, gl, gh, w, r, &s2, sg, low + 8, miss, true, &uns) == nullptr);   // 16 < 24 <= 32
    CHECK(up_args(low + 12, 1, gl, gh, w, r, &s2, sg, low, miss, true, &uns) && up_args(low + 15, 1, gl, gh, w, r, &s2, sg, low, miss, true, &uns) == nullptr);   // low inside out
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, gl, miss, true, &uns) && up_args(low, 1, gl, gh, w, r, &s2, sg, gl + 44, miss, true, &uns));                   // 176 < 192
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, gl + 48, miss, true, &uns) == nullptr);
    CHECK(up_args(low, 1, gl + 12, gh, w, r, &s2, sg, gl, miss, true, &uns) && up_args(low, 1, gl + 16, gh, w, r, &s2, sg, gl, miss, true, &uns) == nullptr);   // 48 < 60 <= 64
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, gh, miss, true, &uns) && up_args(low, 1, gl, gh, w, r, &s2, sg, gh + 116, miss, true, &uns));                  // 464 < 480
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, gh + 120, miss, true, &uns) == nullptr);
    CHECK(up_args(low, 1, gl, gh + 12, w, r, &s2, sg, gh, miss, true, &uns) && up_args(low, 1, gl, gh + 16, w, r, &s2, sg, gh, miss, true, &uns) == nullptr);
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(low), true, &uns) && up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(low) + 23, true, &uns));           // miss + k: the mask against each input
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(low) + 24, true, &uns) == nullptr);
    CHECK(up_args(low + 4, 1, gl, gh, w, r, &s2, sg, out, at(low) + 2, true, &uns) && up_args(low + 4, 1, gl, gh, w, r, &s2, sg, out, at(low) + 1, true, &uns) == nullptr);
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(gl), true, &uns) && up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(gl) + 191, true, &uns));
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(gl) + 192, true, &uns) == nullptr && up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(gl) - 15, true, &uns) == nullptr);
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(gl) - 14, true, &uns));
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(gh), true, &uns) && up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(gh) + 479, true, &uns));
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(gh) + 480, true, &uns) == nullptr && up_args(low, 1, gl, gh, w, r, &s2, sg, out, at(gh) - 14, true, &uns));
    CHECK(fb == at(low));
    // the inputs may share bytes with each other (they are only read): the low buffers as the high ones
    CHECK(up_args(low, 1, gh, gh, w, r, &s2, sg, out, miss, true, &uns) == nullptr);
    // the host form has no overlap rule; an empty image overlaps nothing
    CHECK(up_args(low, 1, gl, gh, w, r, &s2, sg, low, at(low), false, &uns) == nullptr);
    CHECK(up_args(low, 1, low, low, w, 0, &s2, sg, low, at(low), true, &uns) == nullptr);

    std::printf(failures ? "upsample_layout_check: %d FAILED\n" : "upsample_layout_check: all checks held\n", failures);
    return failures ? 1 : 0;
}
