// rt_upsample.hip -- the kernel of the guided upsample (rt_upsample_device; include/rt_mi355x.h, "upsampling", is the definition; DESIGN.md
// §5, Upsampling, the mapping).  A translation unit of its own: the operator reads a low image, its geometry buffers and the geometry
// buffers of the high frame and needs none of the tracer.
//   k_upsample<CH, MISS>     one launch: lane = high pixel, a wave owns a 64 x 1 run of a row, a workgroup the 64 x 4 tile (the denoiser's
//                            tiles, lanes and grid).  The high guide is one pair of 16-byte loads per lane; the four low taps of a lane are
//                            shared with its s - 1 neighbours along the row and with s - 1 rows, so they come from cache; their guides
//                            are recomputed per tap (28 divisions) rather than stored.  No LDS, no atomics, no scratch.
// All arithmetic is float32, every operation rounded on its own (-ffp-contract=off, correctly rounded division), in the header's order.
#include <hip/hip_runtime.h>

#include "rt_launch.hpp"
#include "rt_upsample_layout.hpp"

namespace rtamd {
namespace {

constexpr int kUpThreads = kDnTileH * 64;

// the guide of a pixel from its eight floats {alpha, depth, N[3], A[3]}: covered exactly when alpha > 0.0f, then every value over alpha
struct UpGuide {
    float z, n[3], a[3];
};
__device__ __forceinline__ UpGuide up_guide(const float4 &g0, const float4 &g1) {
    const float a = g0.x;
    return UpGuide{g0.y / a, {g0.z / a, g0.w / a, g1.x / a}, {g1.y / a, g1.z / a, g1.w / a}};
}
__device__ __forceinline__ float up_dist3(const float *p, const float *q) {
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}
// u = 1.0f - d2 / s2; the tap lives on while u > 0.0f (a NaN ends it) and then takes the factor u * u
__device__ __forceinline__ void up_guide_factor(const float d2, const float s2, float &w, bool &ok) {
    const float u = 1.0f - d2 / s2;
    ok = ok && (u > 0.0f);
    w = w * (u * u);
}

// gl, gh: the geometry buffers as pairs of float4 per pixel (the caller's pointers are 16-byte aligned); low: the caller's packed image
template <int CH, bool MISS>
__global__ __launch_bounds__(kUpThreads) void k_upsample(const float *__restrict__ low, const float4 *__restrict__ gl, const float4 *__restrict__ gh,
                                                         float *__restrict__ out, uint8_t *__restrict__ miss, const int32_t width, const int32_t rows,
                                                         const int32_t w, const int32_t r, const int32_t s, const UpScales S, const DnTiles T) {
    const int32_t lane = static_cast<int32_t>(threadIdx.x & 63u), wave = static_cast<int32_t>(threadIdx.x >> 6);
    const float fs = static_cast<float>(s);
    for (uint32_t tile = blockIdx.x; tile < T.tiles; tile += gridDim.x) {
        const DnLane L = dn_lane(T, width, rows, tile, wave, lane);
        if (!L.live) continue;
        const uint64_t p = dn_pixel(width, L.x, L.y);
        const float4 p0 = gh[p * 2u], p1 = gh[p * 2u + 1u];
        const bool pc = p0.x > 0.0f;
        const UpTap X = up_tap(L.x, s), Y = up_tap(L.y, s);
        const float bx[2] = {static_cast<float>(s - X.f) / fs, static_cast<float>(X.f) / fs};
        const float by[2] = {static_cast<float>(s - Y.f) / fs, static_cast<float>(Y.f) / fs};
        UpGuide P{};
        if (pc) P = up_guide(p0, p1);
        float sumw = 0.0f, sum[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) sum[c] = 0.0f;
#pragma unroll
        for (int ey = 0; ey < 2; ++ey) {
#pragma unroll
            for (int ex = 0; ex < 2; ++ex) {
                const float h = bx[ex] * by[ey];
                // the loads of the four taps are unconditional, so that they are in flight together: the coordinate of a tap outside the
                // low image is the first tap's, inside it whatever `ok` says
                const uint64_t q = dn_pixel(w, up_tap_coord(X.i0, ex, w), up_tap_coord(Y.i0, ey, r));
                const float4 q0 = gl[q * 2u], q1 = gl[q * 2u + 1u];
                float lq[CH];
#pragma unroll
                for (int c = 0; c < CH; ++c) lq[c] = low[q * static_cast<uint64_t>(CH) + static_cast<uint64_t>(c)];
                bool ok = up_tap_inside(X.i0, ex, w) && up_tap_inside(Y.i0, ey, r) && h != 0.0f && (q0.x > 0.0f) == pc;
                float wt = h;
                if (ok && pc) {
                    const UpGuide Q = up_guide(q0, q1);
                    up_guide_factor(up_dist3(P.n, Q.n), S.sn2, wt, ok);
                    { const float d = P.z - Q.z; up_guide_factor(d * d, S.sz2, wt, ok); }
                    up_guide_factor(up_dist3(P.a, Q.a), S.sa2, wt, ok);
                }
                if (ok) {
                    sumw = sumw + wt;
#pragma unroll
                    for (int c = 0; c < CH; ++c) sum[c] = sum[c] + wt * lq[c];
                }
            }
        }
        float *o = out + p * static_cast<uint64_t>(CH);
        const bool hit = sumw > 0.0f;
        if (hit) {
#pragma unroll
            for (int c = 0; c < CH; ++c) o[c] = sum[c] / sumw;
        } else {                                                                                // no tap is left: the nearest low pixel, bit for bit
            const uint64_t n = dn_pixel(w, up_nearest(L.x, s, w), up_nearest(L.y, s, r));
#pragma unroll
            for (int c = 0; c < CH; ++c) o[c] = low[n * static_cast<uint64_t>(CH) + static_cast<uint64_t>(c)];
        }
        if constexpr (MISS) miss[p] = hit ? uint8_t{0} : uint8_t{1};
    }
}

template <int CH>
void launch_upsample_as(const int grid, hipStream_t st, const float *low, const float *gb_low, const float *gb_high, float *out, uint8_t *miss,
                        const int32_t width, const int32_t rows, const int32_t w, const int32_t r, const int32_t s, const UpScales &S, const DnTiles &T) {
    const float4 *gl = reinterpret_cast<const float4 *>(gb_low), *gh = reinterpret_cast<const float4 *>(gb_high);
    if (miss) k_upsample<CH, true><<<grid, kUpThreads, 0, st>>>(low, gl, gh, out, miss, width, rows, w, r, s, S, T);
    else k_upsample<CH, false><<<grid, kUpThreads, 0, st>>>(low, gl, gh, out, nullptr, width, rows, w, r, s, S, T);
}

}  // namespace

void launch_upsample(const int grid, hipStream_t st, const int channels, const float *low, const float *gb_low, const float *gb_high, float *out,
                     uint8_t *miss, const int32_t width, const int32_t rows, const int32_t s, const UpScales &S) {
    const DnTiles T = dn_tiles(width, rows);
    const int32_t w = up_low_extent(width, s), r = up_low_extent(rows, s);
    if (channels == 3) launch_upsample_as<3>(grid, st, low, gb_low, gb_high, out, miss, width, rows, w, r, s, S, T);
    else launch_upsample_as<1>(grid, st, low, gb_low, gb_high, out, miss, width, rows, w, r, s, S, T);
}

}  // namespace rtamd
