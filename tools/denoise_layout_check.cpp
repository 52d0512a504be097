// Stand-alone host check of rt_denoise_layout.hpp (the scratch layout, the tile / pixel / tap arithmetic, the per-iteration scales and the
// argument rules of the denoiser), meant for a sanitizer build on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iraytracer-in-cpp_amd/csrc tools/denoise_layout_check.cpp -o denoise_layout_check
// (make -C raytracer-in-cpp_amd/csrc denoise_check builds and runs it).  Exit status 0: every check held.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_denoise_layout.hpp"

using namespace rtamd;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static uint32_t bits(const float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// the parts of the scratch: in order, 16-byte aligned, disjoint, large enough, and their sum is the total
static void layout_holds(const int32_t w, const int32_t r, const int32_t ch) {
    const DnLayout L = dn_layout(w, r, ch);
    const uint64_t px = dn_pixels(w, r), work = px * (ch == 3 ? 16u : 4u);
    CHECK(L.work_pixel_bytes == (ch == 3 ? 16u : 4u));
    CHECK(L.guide0 == 0 && L.guide1 == px * 16u && L.work0 == px * 32u);
    CHECK(L.work1 >= L.work0 + work && L.work1 - (L.work0 + work) < 16u);
    CHECK(L.bytes >= L.work1 + work && L.bytes - (L.work1 + work) < 16u);
    for (const uint64_t off : {L.guide0, L.guide1, L.work0, L.work1, L.bytes}) CHECK(off % 16u == 0);
    CHECK(dn_scratch_bytes(w, r, ch) == L.bytes);
    CHECK(L.bytes == px * 32u + 2u * dn_align16(work));
}

// tiles [t0, t1) of a width x rows image: a live lane holds a pixel of its tile inside the image, its offsets stay inside every part of the
// scratch and inside the caller's image, and the coordinate of every tap at every step is inside the image whether the tap is or not
static void covers(const int32_t w, const int32_t r, const uint32_t t0, const uint32_t t1) {
    const DnTiles T = dn_tiles(w, r);
    CHECK(static_cast<uint64_t>(T.tiles_x) * T.tiles_y == T.tiles && t1 <= T.tiles);
    const uint64_t px = dn_pixels(w, r);
    for (uint32_t t = t0; t < t1; ++t)
        for (int32_t wave = 0; wave < kDnTileH; ++wave)
            for (int32_t lane = 0; lane < kDnTileW; lane += (lane == 0 || lane >= 62 ? 1 : 61)) {
                const DnLane L = dn_lane(T, w, r, t, wave, lane);
                const uint64_t x = static_cast<uint64_t>(t % T.tiles_x) * kDnTileW + static_cast<uint64_t>(lane);
                const uint64_t y = static_cast<uint64_t>(t / T.tiles_x) * kDnTileH + static_cast<uint64_t>(wave);
                CHECK(L.live == (x < static_cast<uint64_t>(w) && y < static_cast<uint64_t>(r)));
                if (!L.live) continue;
                CHECK(static_cast<uint64_t>(L.x) == x && static_cast<uint64_t>(L.y) == y);
                const uint64_t p = dn_pixel(w, L.x, L.y);
                CHECK(p < px && p == y * static_cast<uint64_t>(w) + x);
                for (int32_t k = 0; k < kDnMaxIterations; ++k)
                    for (int32_t d = -2; d <= 2; ++d) {
                        const int32_t off = (1 << k) * d;
                        const int32_t qx = dn_tap_coord(L.x, off, w), qy = dn_tap_coord(L.y, off, r);
                        CHECK(qx >= 0 && qx < w && qy >= 0 && qy < r);
                        CHECK(dn_tap_inside(L.x, off, w) == (static_cast<int64_t>(L.x) + off >= 0 && static_cast<int64_t>(L.x) + off < w));
                        CHECK(dn_tap_inside(L.x, off, w) ? qx == L.x + off : qx == L.x);
                        CHECK(dn_tap_inside(L.y, off, r) ? qy == L.y + off : qy == L.y);
                        CHECK(dn_pixel(w, qx, qy) < px);
                    }
            }
    if (px <= (1u << 20) && t0 == 0 && t1 == T.tiles) {         // small images: every pixel is held exactly once
        std::vector<uint8_t> seen(static_cast<size_t>(px), 0);
        for (uint32_t t = 0; t < T.tiles; ++t)
            for (int32_t wave = 0; wave < kDnTileH; ++wave)
                for (int32_t lane = 0; lane < kDnTileW; ++lane) {
                    const DnLane L = dn_lane(T, w, r, t, wave, lane);
                    if (!L.live) continue;
                    uint8_t &cell = seen[static_cast<size_t>(dn_pixel(w, L.x, L.y))];
                    CHECK(cell == 0);
                    cell = 1;
                }
        for (const uint8_t c : seen) CHECK(c == 1);
    }
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    // small images: width 1, rows 1, odd widths, a multiple of the tile and not, wider than one wave's run
    for (const int32_t w : {1, 2, 3, 37, 48, 63, 64, 65, 70, 129})
        for (const int32_t r : {1, 2, 3, 4, 5, 21, 32}) {
            const DnTiles T = dn_tiles(w, r);
            CHECK(T.tiles_x == static_cast<uint32_t>((w + 63) / 64) && T.tiles_y == static_cast<uint32_t>((r + 3) / 4));
            covers(w, r, 0, T.tiles);
            for (const int32_t ch : {1, 3}) layout_holds(w, r, ch);
        }
    CHECK(dn_tiles(5, 0).tiles == 0 && dn_layout(5, 0, 3).bytes == 0);
    CHECK(dn_layout(3, 2, 1).bytes == 6 * 32 + 2 * 32 && dn_layout(3, 2, 3).bytes == 6 * 64 && dn_layout(1, 1, 1).bytes == 64);
    CHECK(dn_layout(1920, 1080, 3).bytes == 1920ull * 1080 * 64 && dn_layout(1920, 1080, 1).bytes == 1920ull * 1080 * 40);

    // images at the INT32_MAX pixel limit: first and last tiles
    const struct { int32_t w, r; } big[] = {{1, INT32_MAX}, {INT32_MAX, 1}, {46341, 46340}, {65535, 32768}, {3, 715827882}, {715827882, 3}};
    for (const auto &s : big) {
        CHECK(dn_shape_ok(s.w, s.r) && dn_size_ok(s.w, s.r));
        const DnTiles T = dn_tiles(s.w, s.r);
        CHECK(static_cast<uint64_t>(T.tiles_x) * T.tiles_y <= UINT32_MAX);
        CHECK(static_cast<uint64_t>(T.tiles) + 8u * 1024u <= UINT32_MAX);          // (the kernel's tile += gridDim.x cannot wrap)
        covers(s.w, s.r, 0, T.tiles < 3 ? T.tiles : 3);
        covers(s.w, s.r, T.tiles < 3 ? 0 : T.tiles - 3, T.tiles);
        for (const int32_t ch : {1, 3}) {
            layout_holds(s.w, s.r, ch);
            CHECK(dn_image_bytes(s.w, s.r, ch) == static_cast<uint64_t>(s.w) * s.r * ch * 4u);
        }
        CHECK(dn_gbuffer_bytes(s.w, s.r) == static_cast<uint64_t>(s.w) * s.r * 32u);
        CHECK(dn_grid(T.tiles, 256) == (T.tiles >= 2048 ? 2048 : static_cast<int32_t>(T.tiles)));
    }
    CHECK(dn_layout(INT32_MAX, 1, 3).bytes > (1ull << 36));
    CHECK(!dn_size_ok(46341, 46341) && !dn_size_ok(INT32_MAX, 2) && !dn_size_ok(2, INT32_MAX) && !dn_size_ok(INT32_MAX, INT32_MAX));
    CHECK(dn_size_ok(INT32_MAX, 0) && dn_size_ok(1, 0));
    CHECK(dn_guide_grid(0, 256) == 0 && dn_guide_grid(1, 256) == 1 && dn_guide_grid(256, 256) == 1 && dn_guide_grid(257, 256) == 2);
    CHECK(dn_guide_grid(INT32_MAX, 256) == 2048 && dn_guide_grid(2048ull * 256u, 256) == 2048 && dn_guide_grid(2047ull * 256u + 1u, 256) == 2048);
    CHECK(dn_grid(0, 256) == 0 && dn_grid(1, 256) == 1 && dn_grid(2047, 256) == 2047 && dn_grid(UINT32_MAX, 256) == 2048);

    // rt_denoise_scratch_bytes: 0 for invalid arguments
    CHECK(dn_scratch_bytes(0, 4, 3) == 0 && dn_scratch_bytes(-1, 4, 3) == 0 && dn_scratch_bytes(4, -1, 3) == 0 && dn_scratch_bytes(4, 4, 2) == 0);
    CHECK(dn_scratch_bytes(4, 4, 0) == 0 && dn_scratch_bytes(4, 4, 4) == 0 && dn_scratch_bytes(INT32_MAX, 2, 1) == 0 && dn_scratch_bytes(4, 0, 1) == 0);
    CHECK(dn_scratch_bytes(4, 4, 3) == 16 * 64 && dn_scratch_bytes(4, 4, 1) == 16 * 40);

    // the scales: exact powers of two, squared once; +inf stays +inf; a tiny sigma underflows to 0
    for (int32_t k = 0; k < kDnMaxIterations; ++k) {
        const DnScales S = dn_scales(0.5f, 0.75f, 0.0625f, 3.0f, k);
        const float sc = std::ldexp(0.5f, -k), sz = std::ldexp(0.0625f, k);
        CHECK(bits(S.sc2) == bits(sc * sc) && bits(S.sn2) == bits(0.5625f) && bits(S.sz2) == bits(sz * sz) && bits(S.sa2) == bits(9.0f));
        const DnScales I = dn_scales(inf, inf, inf, inf, k);
        CHECK(I.sc2 == inf && I.sn2 == inf && I.sz2 == inf && I.sa2 == inf);
        const DnScales Z = dn_scales(1e-30f, 1e-30f, 1e-30f, 1e-30f, k);
        CHECK(Z.sc2 == 0.0f && Z.sn2 == 0.0f && Z.sz2 == 0.0f && Z.sa2 == 0.0f);
    }
    CHECK(bits(dn_scales(0.1f, 1.0f, 0.1f, 1.0f, 7).sc2) == bits((0.1f * 0.0078125f) * (0.1f * 0.0078125f)));
    CHECK(bits(dn_scales(0.1f, 1.0f, 0.1f, 1.0f, 7).sz2) == bits((0.1f * 128.0f) * (0.1f * 128.0f)));

    // the argument rules (pointers are only compared, never followed)
    alignas(16) static float arena[4096];
    const int32_t w = 5, r = 3;                                  // 15 pixels: image 60 / 180 bytes, gbuffer 480, scratch 15 * 32 + 2 * 64 (1 ch)
    float *in = arena, *gb = arena + 64, *out = arena + 256, *scr = arena + 512;
    int32_t it = 5;
    float sg[4] = {0.5f, 0.5f, 0.0625f, inf};
    bool uns = true;
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, scr, out, true, &uns) == nullptr && !uns);
    CHECK(dn_args(in, 3, gb, w, r, &it, sg, scr, out, true, &uns) == nullptr);
    CHECK(dn_args(in, 3, gb, w, r, &it, sg, nullptr, out, false, &uns) == nullptr);
    CHECK(dn_args(nullptr, 1, gb, w, r, &it, sg, scr, out, true, &uns) && dn_args(in, 1, nullptr, w, r, &it, sg, scr, out, true, &uns));
    CHECK(dn_args(in, 1, gb, w, r, nullptr, sg, scr, out, true, &uns) && dn_args(in, 1, gb, w, r, &it, nullptr, scr, out, true, &uns));
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, nullptr, out, true, &uns) && dn_args(in, 1, gb, w, r, &it, sg, scr, nullptr, true, &uns));
    for (const int32_t ch : {0, 2, 4, -1}) CHECK(dn_args(in, ch, gb, w, r, &it, sg, scr, out, true, &uns) && !uns);
    CHECK(dn_args(in, 1, gb, 0, r, &it, sg, scr, out, true, &uns) && dn_args(in, 1, gb, -3, r, &it, sg, scr, out, true, &uns));
    CHECK(dn_args(in, 1, gb, w, -1, &it, sg, scr, out, true, &uns) && !uns);
    CHECK(dn_args(in, 1, gb, w, 0, &it, sg, scr, out, true, &uns) == nullptr);
    for (const int32_t bad : {0, -1, 9, INT32_MAX, INT32_MIN}) { int32_t b = bad; CHECK(dn_args(in, 1, gb, w, r, &b, sg, scr, out, true, &uns) && !uns); }
    for (const int32_t good : {1, 8}) { int32_t g = good; CHECK(dn_args(in, 1, gb, w, r, &g, sg, scr, out, true, &uns) == nullptr); }
    for (int k = 0; k < 4; ++k)
        for (const float bad : {0.0f, -0.0f, -1.0f, nan, -inf}) {
            float s2[4] = {1.0f, 1.0f, 1.0f, 1.0f};
            s2[k] = bad;
            CHECK(dn_args(in, 1, gb, w, r, &it, s2, scr, out, true, &uns) && !uns);
            CHECK(dn_args(in, 1, gb, w, r, &it, s2, nullptr, out, false, &uns) && !uns);
        }
    CHECK(dn_args(in, 1, gb, INT32_MAX, 2, &it, sg, scr, out, true, &uns) && uns);
    CHECK(dn_args(in, 3, gb, 46341, 46341, &it, sg, nullptr, out, false, &uns) && uns);
    CHECK(dn_args(in, 1, gb, INT32_MAX, 0, &it, sg, scr, out, true, &uns) == nullptr && !uns);
    // alignment of out and scratch (the device form only)
    for (int k = 1; k < 4; ++k) {
        CHECK(dn_args(in, 1, gb, w, r, &it, sg, scr, out + k, true, &uns) && dn_args(in, 1, gb, w, r, &it, sg, scr + k, out, true, &uns));
        CHECK(dn_args(in, 1, gb, w, r, &it, sg, nullptr, out + k, false, &uns) == nullptr);
    }
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, scr, out + 4, true, &uns) == nullptr);
    // each overlap pair, by one byte at either end, and the neighbouring placement that shares none
    const uint64_t img1 = dn_image_bytes(w, r, 1), gbb = dn_gbuffer_bytes(w, r), sb = dn_layout(w, r, 1).bytes;
    CHECK(img1 == 60 && gbb == 480 && sb == 15 * 32 + 2 * 64);
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, scr, in, true, &uns) && !uns);                                     // out == in
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, scr, in + 12, true, &uns));                                          // out starts inside in (48 < 60)
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, scr, in + 16, true, &uns) == nullptr);                               // 64 >= 60: apart
    CHECK(dn_args(in + 12, 1, gb, w, r, &it, sg, scr, in, true, &uns));                                          // in starts inside out
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, scr, gb, true, &uns) && dn_args(in, 1, gb, w, r, &it, sg, scr, gb + 116, true, &uns));
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, scr, gb + 120, true, &uns) == nullptr);
    CHECK(dn_args(in, 1, gb + 12, w, r, &it, sg, scr, gb, true, &uns));                                          // out's last bytes inside gb
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, out, out, true, &uns) && dn_args(in, 1, gb, w, r, &it, sg, scr, scr + 148, true, &uns));
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, scr, scr + 152, true, &uns) == nullptr);
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, out + 12, out, true, &uns));                                         // scratch starts inside out
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, in, out, true, &uns) && dn_args(in + 148, 1, gb, w, r, &it, sg, in, out, true, &uns));
    CHECK(dn_args(in + 152, 1, gb + 256, w, r, &it, sg, in, out + 256, true, &uns) == nullptr);
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, gb, out, true, &uns) && dn_args(in, 1, gb + 148, w, r, &it, sg, gb, out, true, &uns));
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, gb + 116, out, true, &uns));
    // the host form has no overlap rule; an empty image overlaps nothing
    CHECK(dn_args(in, 1, gb, w, r, &it, sg, nullptr, in, false, &uns) == nullptr);
    CHECK(dn_args(in, 1, in, w, 0, &it, sg, in, in, true, &uns) == nullptr);
    CHECK(query_ranges_overlap(in, 4, in + 1, 4) == false && query_ranges_overlap(in, 5, in + 1, 4) && query_ranges_overlap(in + 1, 4, in, 5) && !query_ranges_overlap(in, 0, in, 4));

    std::printf(failures ? "denoise_layout_check: %d FAILED\n" : "denoise_layout_check: all checks held\n", failures);
    return failures ? 1 : 0;
}
