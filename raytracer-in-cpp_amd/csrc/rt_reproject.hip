// rt_reproject.hip -- the kernel of the temporal reprojection (rt_reproject_device; include/rt_mi355x.h, "temporal reprojection", is the
// definition; DESIGN.md §5, Temporal reprojection, the mapping).  A translation unit of its own: the operator reads the current image, the
// accumulated image of the previous frame with its lengths and the geometry buffers of both frames, and needs none of the tracer.
//   k_reproject<CH>          one launch: lane = output pixel, a wave owns a 64 x 1 run of a row, a workgroup the 64 x 4 tile (the denoiser's
//                            tiles, lanes and grid).  The current guide is one pair of 16-byte loads per lane; the four history taps are a
//                            gather at data-dependent coordinates: guide, image and length of all four are loaded unconditionally at
//                            clamped coordinates, so that they are in flight together, and `ok` decides.  No LDS, no atomics, no scratch.
// All arithmetic is float32, every operation rounded on its own (-ffp-contract=off, correctly rounded division), in the header's order.
#include <hip/hip_runtime.h>

#include "rt_launch.hpp"
#include "rt_reproject_layout.hpp"

namespace rtamd {
namespace {

constexpr int kRpThreads = kDnTileH * 64;

// the guide of a pixel from its eight floats {alpha, depth, N[3], A[3]}: covered exactly when alpha > 0.0f, then every value over alpha
struct RpGuide {
    float z, n[3], a[3];
};
__device__ __forceinline__ RpGuide rp_guide(const float4 &g0, const float4 &g1) {
    const float a = g0.x;
    return RpGuide{g0.y / a, {g0.z / a, g0.w / a, g1.x / a}, {g1.y / a, g1.z / a, g1.w / a}};
}
__device__ __forceinline__ float rp_dist3(const float *p, const float *q) {
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}
// u = 1.0f - d2 / s2; the tap lives on while u > 0.0f (a NaN ends it) and then takes the factor u * u
__device__ __forceinline__ void rp_guide_factor(const float d2, const float s2, float &w, bool &ok) {
    const float u = 1.0f - d2 / s2;
    ok = ok && (u > 0.0f);
    w = w * (u * u);
}

// gc, gh: the geometry buffers as pairs of float4 per pixel (the caller's pointers are 16-byte aligned); cur, hist: the caller's packed images
template <int CH>
__global__ __launch_bounds__(kRpThreads) void k_reproject(const float *__restrict__ cur, const float4 *__restrict__ gc, const float *__restrict__ hist,
                                                          const float4 *__restrict__ gh, const uint8_t *__restrict__ len_hist, float *__restrict__ out,
                                                          uint8_t *__restrict__ len_out, const int32_t width, const int32_t rows, const RpMap M,
                                                          const RpScales S, const int32_t max_history, const DnTiles T) {
    const int32_t lane = static_cast<int32_t>(threadIdx.x & 63u), wave = static_cast<int32_t>(threadIdx.x >> 6);
    for (uint32_t tile = blockIdx.x; tile < T.tiles; tile += gridDim.x) {
        const DnLane L = dn_lane(T, width, rows, tile, wave, lane);
        if (!L.live) continue;
        const uint64_t p = dn_pixel(width, L.x, L.y);
        const float4 p0 = gc[p * 2u], p1 = gc[p * 2u + 1u];
        float c[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) c[k] = cur[p * static_cast<uint64_t>(CH) + static_cast<uint64_t>(k)];
        RpGuide P{};
        bool look = p0.x > 0.0f;                                                              // covered ...
        if (look) P = rp_guide(p0, p1);
        look = look && P.z > 0.0f;                                                            // ... with a depth to reproject ...
        RpPos R{0.0f, 0.0f, 0.0f, false};
        if (look) R = rp_project(M, static_cast<float>(L.x), static_cast<float>(L.y), P.z);
        look = look && R.ok && rp_inside(R.x, width) && rp_inside(R.y, rows);                 // ... to a place in front of and inside the previous frame
        float sumw = 0.0f, sum[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) sum[k] = 0.0f;
        int32_t nmin = 255;
        if (look) {
            const RpTap X = rp_tap(R.x), Y = rp_tap(R.y);
            const float bx[2] = {1.0f - X.f, X.f}, by[2] = {1.0f - Y.f, Y.f};
#pragma unroll
            for (int ey = 0; ey < 2; ++ey) {
#pragma unroll
                for (int ex = 0; ex < 2; ++ex) {
                    const float h = bx[ex] * by[ey];
                    // the loads of the four taps are unconditional, so that they are in flight together: the coordinate of a tap outside the
                    // image is clamped into it, inside it whatever `ok` says
                    const uint64_t q = dn_pixel(width, rp_tap_coord(X.i0, ex, width), rp_tap_coord(Y.i0, ey, rows));
                    const float4 q0 = gh[q * 2u], q1 = gh[q * 2u + 1u];
                    const int32_t lq = static_cast<int32_t>(len_hist[q]);
                    float hq[CH];
#pragma unroll
                    for (int k = 0; k < CH; ++k) hq[k] = hist[q * static_cast<uint64_t>(CH) + static_cast<uint64_t>(k)];
                    bool ok = rp_tap_inside(X.i0, ex, width) && rp_tap_inside(Y.i0, ey, rows) && h != 0.0f && lq != 0 && q0.x > 0.0f;
                    float wt = h;
                    if (ok) {
                        const RpGuide Q = rp_guide(q0, q1);
                        rp_guide_factor(rp_dist3(P.n, Q.n), S.sn2, wt, ok);
                        { const float d = R.zr - Q.z; rp_guide_factor(d * d, S.sz2, wt, ok); }
                        rp_guide_factor(rp_dist3(P.a, Q.a), S.sa2, wt, ok);
                    }
                    if (ok) {
                        sumw = sumw + wt;
#pragma unroll
                        for (int k = 0; k < CH; ++k) sum[k] = sum[k] + wt * hq[k];
                        nmin = lq < nmin ? lq : nmin;
                    }
                }
            }
        }
        float *o = out + p * static_cast<uint64_t>(CH);
        if (sumw > 0.0f) {
            const int32_t n = nmin + 1 < max_history ? nmin + 1 : max_history;
            const float fn = static_cast<float>(n);
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const float H = sum[k] / sumw;
                o[k] = H + (c[k] - H) / fn;
            }
            len_out[p] = static_cast<uint8_t>(n);
        } else {                                                                              // no history: the current frame, bit for bit
#pragma unroll
            for (int k = 0; k < CH; ++k) o[k] = c[k];
            len_out[p] = uint8_t{1};
        }
    }
}

}  // namespace

void launch_reproject(const int grid, hipStream_t st, const int channels, const float *cur, const float *gb_cur, const float *hist, const float *gb_hist,
                      const uint8_t *len_hist, float *out, uint8_t *len_out, const int32_t width, const int32_t rows, const RpMap &M, const RpScales &S,
                      const int32_t max_history) {
    const DnTiles T = dn_tiles(width, rows);
    const float4 *gc = reinterpret_cast<const float4 *>(gb_cur), *gh = reinterpret_cast<const float4 *>(gb_hist);
    if (channels == 3) k_reproject<3><<<grid, kRpThreads, 0, st>>>(cur, gc, hist, gh, len_hist, out, len_out, width, rows, M, S, max_history, T);
    else k_reproject<1><<<grid, kRpThreads, 0, st>>>(cur, gc, hist, gh, len_hist, out, len_out, width, rows, M, S, max_history, T);
}

}  // namespace rtamd
