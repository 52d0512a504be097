// rt_denoise.hip -- the kernels of the edge-avoiding denoiser (rt_denoise_device; include/rt_mi355x.h, "denoising", is the definition;
// DESIGN.md §5, Denoising, the mapping).  A translation unit of its own: the filter reads an image and the geometry buffers of the same
// frame and needs none of the tracer.
//   k_denoise_guide<CH>      one launch: the two float4 guide records of every pixel, and for three channels the RGBx working image
//   k_atrous<CH, LAST>       one launch per iteration: lane = pixel, a wave owns a 64 x 1 run of a row, a workgroup the 64 x 4 tile; every
//                            tap is the same row segment shifted by step * dx, so every tap load is coalesced without LDS
//   k_atrous_lds<CH, LAST, STEP>  the same iteration with the tile, its halo of 2 * STEP pixels and both guide records staged in LDS: measured
//                            and rejected (Denoising), so only an A/B build with -DRT_DENOISE_STAGED_STEPS=mask holds it
// All arithmetic is float32, every operation rounded on its own (-ffp-contract=off, correctly rounded division), in the header's order.
#include <hip/hip_runtime.h>

#include "rt_denoise_layout.hpp"
#include "rt_launch.hpp"

namespace rtamd {
namespace {

constexpr int kDnThreads = kDnTileH * 64;
constexpr float kDnH[3] = {0.375f, 0.25f, 0.0625f};

// a pixel of a working image: float4 RGBx for three channels, one float for one
template <int CH> struct DnWork;
template <> struct DnWork<3> { using type = float4; };
template <> struct DnWork<1> { using type = float; };

template <int CH> struct DnPixel {
    float c[CH];
};
__device__ __forceinline__ DnPixel<3> dn_unpack(const float4 v) { return DnPixel<3>{{v.x, v.y, v.z}}; }
__device__ __forceinline__ DnPixel<1> dn_unpack(const float v) { return DnPixel<1>{{v}}; }

// the output of an iteration: the caller's packed image (LAST) or a working image
template <int CH, bool LAST>
__device__ __forceinline__ void dn_store(void *dst, const uint64_t p, const DnPixel<CH> &v) {
    if constexpr (LAST) {
        float *o = static_cast<float *>(dst) + p * static_cast<uint64_t>(CH);
#pragma unroll
        for (int c = 0; c < CH; ++c) o[c] = v.c[c];
    } else if constexpr (CH == 3) {
        static_cast<float4 *>(dst)[p] = make_float4(v.c[0], v.c[1], v.c[2], 0.0f);
    } else {
        static_cast<float *>(dst)[p] = v.c[0];
    }
}

template <int CH> struct DnSums {
    float w, c[CH];
};

// u = 1.0f - d2 / s2; the tap lives on while u > 0.0f (a NaN ends it) and then takes the factor u * u
__device__ __forceinline__ void dn_guide_factor(const float d2, const float s2, float &w, bool &ok) {
    const float u = 1.0f - d2 / s2;
    ok = ok && (u > 0.0f);
    w = w * (u * u);
}
__device__ __forceinline__ float dn_dist3(const float ax, const float ay, const float az, const float bx, const float by, const float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// One tap that is not the centre: pixel p (image ip, records pa, pb) against pixel q, `ok` = q exists.  The four guides in the order
// colour, normal, depth, albedo; a tap that a guide stops, or whose pixel is missing or not covered, leaves the sums as they are.
template <int CH>
__device__ __forceinline__ void dn_tap(DnSums<CH> &A, const float h, const DnPixel<CH> &ip, const float4 &pa, const float4 &pb, const DnPixel<CH> &iq,
                                       const float4 &qa, const float4 &qb, bool ok, const DnScales &S) {
    ok = ok && (qb.w > 0.0f);
    float w = h, d2;
    if constexpr (CH == 3) d2 = dn_dist3(ip.c[0], ip.c[1], ip.c[2], iq.c[0], iq.c[1], iq.c[2]);
    else { const float d = ip.c[0] - iq.c[0]; d2 = d * d; }
    dn_guide_factor(d2, S.sc2, w, ok);
    dn_guide_factor(dn_dist3(pa.x, pa.y, pa.z, qa.x, qa.y, qa.z), S.sn2, w, ok);
    { const float d = pa.w - qa.w; dn_guide_factor(d * d, S.sz2, w, ok); }
    dn_guide_factor(dn_dist3(pb.x, pb.y, pb.z, qb.x, qb.y, qb.z), S.sa2, w, ok);
    const float sw = A.w + w;
    A.w = ok ? sw : A.w;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const float sc = A.c[c] + w * iq.c[c];
        A.c[c] = ok ? sc : A.c[c];
    }
}
template <int CH>
__device__ __forceinline__ void dn_centre(DnSums<CH> &A, const DnPixel<CH> &ip) {
    constexpr float h = kDnH[0] * kDnH[0];
    A.w = A.w + h;
#pragma unroll
    for (int c = 0; c < CH; ++c) A.c[c] = A.c[c] + h * ip.c[c];
}
template <int CH>
__device__ __forceinline__ DnPixel<CH> dn_result(const DnSums<CH> &A) {
    DnPixel<CH> r;
#pragma unroll
    for (int c = 0; c < CH; ++c) r.c[c] = A.c[c] / A.w;
    return r;
}

// gb: the caller's geometry buffers, eight floats per pixel {alpha, depth, N[3], A[3]} (read as floats: the caller's pointer has no alignment rule)
template <int CH>
__global__ __launch_bounds__(kDnThreads) void k_denoise_guide(const float *__restrict__ in, const float *__restrict__ gb, float4 *__restrict__ g0,
                                                              float4 *__restrict__ g1, float4 *__restrict__ work0, const uint64_t pixels) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kDnThreads;
    for (uint64_t p = static_cast<uint64_t>(blockIdx.x) * kDnThreads + threadIdx.x; p < pixels; p += stride) {
        const float *g = gb + p * static_cast<uint64_t>(kDnGbChannels);
        const float a = g[0];
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;
        if (a > 0.0f) {
            r0 = make_float4(g[2] / a, g[3] / a, g[4] / a, g[1] / a);
            r1 = make_float4(g[5] / a, g[6] / a, g[7] / a, 1.0f);
        }
        g0[p] = r0;
        g1[p] = r1;
        if constexpr (CH == 3) work0[p] = make_float4(in[p * 3u], in[p * 3u + 1u], in[p * 3u + 2u], 0.0f);
    }
}

template <int CH, bool LAST>
__global__ __launch_bounds__(kDnThreads) void k_atrous(const typename DnWork<CH>::type *__restrict__ src, const float4 *__restrict__ g0,
                                                       const float4 *__restrict__ g1, void *__restrict__ dst, const int32_t width, const int32_t rows,
                                                       const int32_t step, const DnScales S, const DnTiles T) {
    const int32_t lane = static_cast<int32_t>(threadIdx.x & 63u), wave = static_cast<int32_t>(threadIdx.x >> 6);
    for (uint32_t tile = blockIdx.x; tile < T.tiles; tile += gridDim.x) {
        const DnLane L = dn_lane(T, width, rows, tile, wave, lane);
        if (!L.live) continue;
        const uint64_t p = dn_pixel(width, L.x, L.y);
        const DnPixel<CH> ip = dn_unpack(src[p]);
        const float4 pb = g1[p];
        if (!(pb.w > 0.0f)) { dn_store<CH, LAST>(dst, p, ip); continue; }          // not covered: I_{k+1}(p) = I_k(p)
        const float4 pa = g0[p];
        DnSums<CH> A{};
        // one row of five taps at a time: its 15 loads are in flight together, the next row's are not hoisted above it (unrolling both
        // loops put all 72 loads first: 255 VGPRs, one wave per SIMD)
#pragma unroll 1
        for (int dy = -2; dy <= 2; ++dy) {
            const bool in_y = dn_tap_inside(L.y, step * dy, rows);
            const int32_t qy = dn_tap_coord(L.y, step * dy, rows);
            const float hy = dy == 0 ? kDnH[0] : (dy == 1 || dy == -1 ? kDnH[1] : kDnH[2]);
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                if (dx == 0 && dy == 0) { dn_centre(A, ip); continue; }
                const bool in = in_y && dn_tap_inside(L.x, step * dx, width);
                const uint64_t q = dn_pixel(width, dn_tap_coord(L.x, step * dx, width), qy);      // (inside the image whatever `in` says)
                dn_tap(A, kDnH[dx < 0 ? -dx : dx] * hy, ip, pa, pb, dn_unpack(src[q]), g0[q], g1[q], in, S);
            }
        }
        dn_store<CH, LAST>(dst, p, dn_result(A));
    }
}

#ifdef RT_DENOISE_STAGED_STEPS
// The staged variant: the 64 x 4 tile with a halo of 2 * STEP pixels on every side -- working image and both guide records -- goes to LDS
// first (a pixel outside the image as "not covered"), then every tap is an LDS read at a compile-time offset.
template <int CH, bool LAST, int STEP>
__global__ __launch_bounds__(kDnThreads) void k_atrous_lds(const typename DnWork<CH>::type *__restrict__ src, const float4 *__restrict__ g0,
                                                           const float4 *__restrict__ g1, void *__restrict__ dst, const int32_t width, const int32_t rows,
                                                           const DnScales S, const DnTiles T) {
    using Work = typename DnWork<CH>::type;
    constexpr int HALO = 2 * STEP, RW = kDnTileW + 2 * HALO, RH = kDnTileH + 2 * HALO, CELLS = RW * RH;
    __shared__ float4 s_g0[CELLS], s_g1[CELLS];
    __shared__ Work s_img[CELLS];
    const int32_t lane = static_cast<int32_t>(threadIdx.x & 63u), wave = static_cast<int32_t>(threadIdx.x >> 6);
    for (uint32_t tile = blockIdx.x; tile < T.tiles; tile += gridDim.x) {
        const int64_t x0 = static_cast<int64_t>(tile % T.tiles_x) * kDnTileW - HALO, y0 = static_cast<int64_t>(tile / T.tiles_x) * kDnTileH - HALO;
        __syncthreads();                                   // the reads of the previous tile are done
        for (int i = static_cast<int>(threadIdx.x); i < CELLS; i += kDnThreads) {
            const int64_t gx = x0 + i % RW, gy = y0 + i / RW;
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
            Work v{};
            if (gx >= 0 && gx < width && gy >= 0 && gy < rows) {
                const uint64_t q = static_cast<uint64_t>(gy) * static_cast<uint64_t>(width) + static_cast<uint64_t>(gx);
                a = g0[q]; b = g1[q]; v = src[q];
            }
            s_g0[i] = a; s_g1[i] = b; s_img[i] = v;
        }
        __syncthreads();
        const DnLane L = dn_lane(T, width, rows, tile, wave, lane);
        if (L.live) {
            const uint64_t p = dn_pixel(width, L.x, L.y);
            const int c = (wave + HALO) * RW + lane + HALO;
            const DnPixel<CH> ip = dn_unpack(s_img[c]);
            const float4 pb = s_g1[c];
            if (!(pb.w > 0.0f)) {
                dn_store<CH, LAST>(dst, p, ip);
            } else {
                const float4 pa = s_g0[c];
                DnSums<CH> A{};
#pragma unroll
                for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
                    for (int dx = -2; dx <= 2; ++dx) {
                        if (dx == 0 && dy == 0) { dn_centre(A, ip); continue; }
                        const int q = c + STEP * dy * RW + STEP * dx;
                        const float h = kDnH[dx < 0 ? -dx : dx] * kDnH[dy < 0 ? -dy : dy];
                        dn_tap(A, h, ip, pa, pb, dn_unpack(s_img[q]), s_g0[q], s_g1[q], true, S);
                    }
                }
                dn_store<CH, LAST>(dst, p, dn_result(A));
            }
        }
    }
}

#endif

template <int CH, bool LAST>
void launch_atrous_as(const int grid, hipStream_t st, const bool staged, const void *src, const float4 *g0, const float4 *g1, void *dst, const int32_t width,
                      const int32_t rows, const int32_t step, const DnScales &S, const DnTiles &T) {
    const auto *s = static_cast<const typename DnWork<CH>::type *>(src);
#ifdef RT_DENOISE_STAGED_STEPS
    if (staged && step == 1) { k_atrous_lds<CH, LAST, 1><<<grid, kDnThreads, 0, st>>>(s, g0, g1, dst, width, rows, S, T); return; }
    if (staged && step == 2) { k_atrous_lds<CH, LAST, 2><<<grid, kDnThreads, 0, st>>>(s, g0, g1, dst, width, rows, S, T); return; }
#endif
    k_atrous<CH, LAST><<<grid, kDnThreads, 0, st>>>(s, g0, g1, dst, width, rows, step, S, T);
}

}  // namespace

// the steps whose tile plus halo (both guide records and the working image, 48 bytes per pixel) fit the 64 KB a workgroup may declare
bool denoise_staged_fits(const int32_t step) {
#ifdef RT_DENOISE_STAGED_STEPS
    return step == 1 || step == 2;
#else
    (void)step;
    return false;
#endif
}

void launch_denoise_guide(const int grid, hipStream_t st, const int channels, const float *in, const float *gbuffer, float4 *g0, float4 *g1, float4 *work0,
                          const uint64_t pixels) {
    if (channels == 3) k_denoise_guide<3><<<grid, kDnThreads, 0, st>>>(in, gbuffer, g0, g1, work0, pixels);
    else k_denoise_guide<1><<<grid, kDnThreads, 0, st>>>(in, gbuffer, g0, g1, work0, pixels);
}

void launch_atrous(const int grid, hipStream_t st, const int channels, const bool last, const bool staged, const void *src, const float4 *g0, const float4 *g1,
                   void *dst, const int32_t width, const int32_t rows, const int32_t step, const DnScales &S) {
    const DnTiles T = dn_tiles(width, rows);
    if (channels == 3) {
        if (last) launch_atrous_as<3, true>(grid, st, staged, src, g0, g1, dst, width, rows, step, S, T);
        else launch_atrous_as<3, false>(grid, st, staged, src, g0, g1, dst, width, rows, step, S, T);
    } else {
        if (last) launch_atrous_as<1, true>(grid, st, staged, src, g0, g1, dst, width, rows, step, S, T);
        else launch_atrous_as<1, false>(grid, st, staged, src, g0, g1, dst, width, rows, step, S, T);
    }
}

}  // namespace rtamd
