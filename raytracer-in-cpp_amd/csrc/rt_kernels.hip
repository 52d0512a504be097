// rt_kernels.hip -- hand-written HIP kernels (gfx950 / CDNA4) for the primary/shadow ray-trace path.
//
// Execution model (designed for 64-wide wavefronts + the scalar unit, not a port of a lane-per-ray CPU loop):
//   * PACKET TRAVERSAL.  One wavefront owns 64 coherent rays (an 8x8 pixel tile, 64 compacted bounce rays, or the
//     N area-light samples of one hit point).  The octree walk is WAVE-UNIFORM: node ids and per-node lane masks
//     live in a small per-wave LDS stack, node boxes and leaf triangle records are fetched with scalar loads
//     (s_load_dwordx8/x16 through the scalar cache -- no VGPR gather, no per-lane addressing), and each lane only
//     runs the arithmetic for its own ray under an exec mask.  `__ballot` decides whether any lane still needs a
//     child / a leaf.  This reproduces BoxTree::intersect's result exactly (src/boxTree.cpp:150-173: a lane's
//     candidate set = faces of every non-empty leaf whose whole ancestor chain its ray's box tests accept) while
//     touching each node/triangle once per wave instead of once per ray.
//   * PERSISTENT WAVES.  Every kernel is launched with a fixed grid sized to its residency (CUs x blocks/CU from
//     the occupancy query); waves pull CHUNKS of units from a sharded device-side queue (8 XCD-keyed heads on separate
//     cache lines, interleaved chunk ownership, next index prefetched, stealing when drained).  Measured on the way here: a
//     single atomic head caps a kernel at ~88 units/us; static striding leaves waves idle 58 % of the time.  Work sizes that depend on earlier kernels (lit
//     hits, bounce rays) are read from device memory, so a whole frame is a fixed launch sequence with no host
//     round trip and can be captured in a hipGraph.
//   * Shadow samples are a SEPARATE kernel (k_shadow) so rocprof attributes traversal time to
//     closest-hit (k_trace) vs area-light shadow rays (k_shadow) separately.
//   * Ray compaction between bounces uses wave-wide ballot + mbcnt prefix and one atomicAdd per wave.
//
// Numerics: compiled with -ffp-contract=off and correctly rounded fp32 divide/sqrt; every expression keeps the
// reference's operation order (Eigen 3.3.7: a.dot(b) = a0*b0 + (a1*b1 + a2*b2)), std::min/std::max are spelt as
// the ternaries libstdc++ uses, so integer results (face ids, 8-bit pixels) are bit-exact and float RGB differs
// from the CPU path nowhere: powf is glibc's published algorithm evaluated bit for bit (pow_shininess).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "rt_ao_layout.hpp"
#include "rt_shadow_layout.hpp"
#include "rt_gather_layout.hpp"
#include "rt_probe_layout.hpp"
#include "rt_distance_layout.hpp"
#include "rt_hits_layout.hpp"
#include "rt_device.hpp"
#include "rt_gbuffer_layout.hpp"
#include "rt_launch.hpp"

namespace rtamd {

#define RT_WAVES 4          // waves per workgroup (256 threads)
#define RT_STACK 128        // >= 7*16 + 8: DFS stack bound for MAX_DEPTH 15 octrees (checked on upload)

// ---- libstdc++ std::min / std::max (NaN behaviour is part of the reference's slab test) -----------------------
__device__ __forceinline__ float smin(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float smax(float a, float b) { return (a < b) ? b : a; }
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return ax * bx + (ay * by + az * bz);
}
__device__ __forceinline__ void normalize3(float &x, float &y, float &z) {
    const float q = x * x + (y * y + z * z);
    if (q > 0.0f) {
        const float s = sqrtf(q);
        x = x / s; y = y / s; z = z / s;
    }
}

// The expected side of a wave-uniform test of the sample loop: the compiler then lays the common side out as the fall-through, so a headline
// sample takes no taken branch to a block that only branches back ("The sample loop: table and layout").  RT_SELDOM is the
// same statement at 0.97 instead of certainty: block frequencies also weigh the register allocator's spill choices, and with a certain
// hint on pow_shininess's general-path test k_shade<true, false, false> and <true, true, false> come out with 12 and 8 bytes of scratch
// per lane more than without; at 0.97 (and 0.9) the layout is the same and no variant's scratch grows.
// (make ab AB_FLAGS=-DRT_NO_HOT_LAYOUT: the compiler's own layout, for the A/B.)
#ifdef RT_NO_HOT_LAYOUT
#define RT_LIKELY(x) (x)
#define RT_UNLIKELY(x) (x)
#define RT_SELDOM(x) (x)
#else
#define RT_LIKELY(x) __builtin_expect(static_cast<bool>(x), true)
#define RT_UNLIKELY(x) __builtin_expect(static_cast<bool>(x), false)
#define RT_SELDOM(x) __builtin_expect_with_probability(static_cast<bool>(x), false, 0.97)
#endif

// Eigen's normalized() (Dot.h:124-134: v / sqrt(squaredNorm) when that is > 0) with the work the three IEEE divisions share done once.
// hipcc expands a correctly rounded x / s into  d = div_scale(s), n = div_scale(x), r = rcp(d), e = fma(-d, r, 1), r = fma(e, r, r),
// q = n r, q = fma(fma(-d, q, n), r, q), div_fmas(fma(-d, q, n), r, q), div_fixup  -- 11 instructions, of which the reciprocal and its
// refinement depend on the divisor alone.  div_scale leaves both operands as they are and div_fmas / div_fixup pass the quotient through
// whenever divisor and quotient are far from the ends of the exponent range, so for 2^-40 <= s <= 2^40 and 2^-60 <= |x| (<= s) the plain
// FMA chain below IS that sequence, bit for bit, and the three quotients share r: 18 instead of 33 instructions.  Anything else -- a zero
// or tiny component (the sign of a zero quotient comes from div_fixup), a huge or non-finite norm -- takes the three full divisions; the
// test is wave-uniform, so the common case has no divergent branch.  (k_shade runs two of these per sample.)
__device__ __forceinline__ void normalize3_fast(const float q, float &x, float &y, float &z) {
    // the correctly rounded square root as hipcc expands sqrtf -- v_sqrt_f32 (1 ulp), then the neighbour whose residual says so -- without the
    // scaling of denormal arguments and the 0 / inf pass-through, neither of which this range can need: 9 instead of 16 instructions
    float s = __builtin_amdgcn_sqrtf(q);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u), sp = __uint_as_float(__float_as_uint(s) + 1u);
    const float rm = __builtin_fmaf(-sm, s, q), rp = __builtin_fmaf(-sp, s, q);
    s = rp > 0.0f ? sp : (rm <= 0.0f ? sm : s);
    float r = __builtin_amdgcn_rcpf(s);
    const float e = __builtin_fmaf(-s, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
    float qx = x * r, qy = y * r, qz = z * r;
    qx = __builtin_fmaf(__builtin_fmaf(-s, qx, x), r, qx);
    qy = __builtin_fmaf(__builtin_fmaf(-s, qy, y), r, qy);
    qz = __builtin_fmaf(__builtin_fmaf(-s, qz, z), r, qz);
    x = __builtin_fmaf(__builtin_fmaf(-s, qx, x), r, qx);
    y = __builtin_fmaf(__builtin_fmaf(-s, qy, y), r, qy);
    z = __builtin_fmaf(__builtin_fmaf(-s, qz, z), r, qz);
}
__device__ __forceinline__ void normalize3_shared(float &x, float &y, float &z) {
    const float q = x * x + (y * y + z * z);
    const bool ok = (q >= 0x1p-80f) && (q <= 0x1p80f) && (fminf(fminf(fabsf(x), fabsf(y)), fabsf(z)) >= 0x1p-60f);     // NaN: false
    if (RT_LIKELY(__ballot(!ok) == 0ull)) {
        normalize3_fast(q, x, y, z);
    } else if (q > 0.0f) {
        const float s = sqrtf(q);
        x = x / s; y = y / s; z = z / s;
    }
}
// The form whose q = x*x + (y*y + z*z) comes from the caller: k_shade's row loop builds it from parts that the samples of a light grid share
// (shade_samples_rows).  TESTED: the caller has evaluated the range test for every sample of its loop up front (light_dirs_in_range) and it
// passed in every active lane, so the fast body runs without the test.  The fast body is one definition, normalize3_fast.  (The test and
// the two lines of the slow side are written out in both forms: with the three-argument form calling this one the compiler commutes the
// operands of two s_or_b64 in k_deep, k_phong_probe and the k_shade variants without the table -- the same instructions, but their listings
// would no longer be the parent's, which tools/isa_diff.py holds them to.)
template <bool TESTED>
__device__ __forceinline__ void normalize3_shared(const float q, float &x, float &y, float &z) {
    if constexpr (TESTED) {
        normalize3_fast(q, x, y, z);
    } else {
        const bool ok = (q >= 0x1p-80f) && (q <= 0x1p80f) && (fminf(fminf(fabsf(x), fabsf(y)), fabsf(z)) >= 0x1p-60f);     // NaN: false
        if (RT_LIKELY(__ballot(!ok) == 0ull)) {
            normalize3_fast(q, x, y, z);
        } else if (q > 0.0f) {
            const float s = sqrtf(q);
            x = x / s; y = y / s; z = z / s;
        }
    }
}

__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
}

// BoundingBox::boxIntersect (src/boundingBox.cpp:48-83) with dir = dest - origin already formed by the caller.
__device__ __forceinline__ bool box_hit(const float *__restrict__ b, float ox, float oy, float oz, float dx, float dy, float dz) {
    const float tx0 = (b[0] - ox) / dx, tx1 = (b[3] - ox) / dx;
    const float ty0 = (b[1] - oy) / dy, ty1 = (b[4] - oy) / dy;
    const float tz0 = (b[2] - oz) / dz, tz1 = (b[5] - oz) / dz;
    const float tin = smax(smax(smin(tx0, tx1), smin(ty0, ty1)), smin(tz0, tz1));
    const float tout = smin(smin(smax(tx0, tx1), smax(ty0, ty1)), smax(tz0, tz1));
    return !((tin > tout) || (tout < 0));
}

// The node and leaf-triangle arrays reach the kernels as separate `const T *__restrict__` parameters (noalias +
// readonly): only then can the compiler prove that no store in the kernel clobbers them and select the
// wave-uniform loads as s_load_dwordx8/x16 (scalar cache, SGPR destination) instead of 64-lane global_loads.

// Dynamic work distribution without a single hot atomic (one queue head saturates at ~88 dequeues/us on MI355X;
// plain static striding left waves resident only ~42 % of the kernel on the dodge scene).
//   * units are handed out in CHUNKS of `chunk` consecutive units (chunk ~ units / (6 x waves), computed in-kernel
//     because the unit count itself is produced on the device), so a wave performs only ~6 atomics per launch;
//   * chunk c belongs to queue head c % 8; a workgroup uses head blockIdx % 8 -- blocks b and b+8 share an XCD, so
//     each head is hit from one XCD's L2 -- and the interleaving keeps all 8 heads equally loaded, so stealing
//     (next head, checked with a plain load first) only happens in the last few chunks;
//   * the next chunk index is fetched BEFORE the current chunk is processed: the atomic's latency hides behind work.
// Approximate-then-verify form of the slab test.  The six quotients are first formed with ONE v_rcp_f32 per axis
// (relative error of x * rcp(d) vs the correctly rounded x / d: <= ~2.4e-7).  If the resulting tin/tout are separated --
// and tout is away from zero -- by more than 1e-6 * sum|t_i| (4x that bound; a perturbation of max/min compositions never
// exceeds the largest perturbation of their inputs), the reference's decision `!((tin > tout) || (tout < 0))` is already
// determined and no IEEE division is needed.  Anything closer, and anything non-finite (zero direction components make
// inf/NaN terms whose handling depends on std::min/std::max argument order), takes the exact path.  ~30 VALU instead of
// ~100 per box test; the decision is bit-identical by construction (checked by the counter-equality tests).
__device__ __forceinline__ bool box_hit_verified(const float *__restrict__ b, float ox, float oy, float oz, float dx, float dy, float dz,
                                                 float rx, float ry, float rz) {
    const float ax0 = (b[0] - ox) * rx, ax1 = (b[3] - ox) * rx;
    const float ay0 = (b[1] - oy) * ry, ay1 = (b[4] - oy) * ry;
    const float az0 = (b[2] - oz) * rz, az1 = (b[5] - oz) * rz;
    const float tin = fmaxf(fmaxf(fminf(ax0, ax1), fminf(ay0, ay1)), fminf(az0, az1));
    const float tout = fminf(fminf(fmaxf(ax0, ax1), fmaxf(ay0, ay1)), fmaxf(az0, az1));
    const float mag = ((fabsf(ax0) + fabsf(ax1)) + (fabsf(ay0) + fabsf(ay1))) + (fabsf(az0) + fabsf(az1));
    const float e = 1e-6f * mag;
    const bool finite = mag < 3.0e38f;                       // false for inf and NaN
    const bool sure_hit = finite && (tout - tin > e) && (tout > e);
    const bool sure_miss = finite && ((tin - tout > e) || (tout < -e));
    if (sure_hit) return true;
    if (sure_miss) return false;
    return box_hit(b, ox, oy, oz, dx, dy, dz);
}

// A ray as the walks take it.  The two constructors are the only places that form these expressions.
struct WalkRay {
    float ox, oy, oz;        // origin
    float dx, dy, dz;        // triangle-test direction
    float bx, by, bz;        // box-test direction (dest - origin)
    float brx, bry, brz;     // v_rcp_f32 of it (approximate)
};
// traceRay: boxIntersect(origin, origin + direction) -- the box-test direction is (o + d) - o, not d (flyscene.cpp:655)
__device__ __forceinline__ WalkRay trace_ray(const float ox, const float oy, const float oz, const float dx, const float dy, const float dz) {
    const float bx = (ox + dx) - ox, by = (oy + dy) - oy, bz = (oz + dz) - oz;
    return WalkRay{ox, oy, oz, dx, dy, dz, bx, by, bz, __builtin_amdgcn_rcpf(bx), __builtin_amdgcn_rcpf(by), __builtin_amdgcn_rcpf(bz)};
}
// the segment lightStrikes tests (flyscene.cpp:912-954): origin = light point or sample, direction = hitPoint - origin for both tests
__device__ __forceinline__ WalkRay segment_ray(const float fx, const float fy, const float fz, const float tx, const float ty, const float tz) {
    const float dx = tx - fx, dy = ty - fy, dz = tz - fz;
    return WalkRay{fx, fy, fz, dx, dy, dz, dx, dy, dz, __builtin_amdgcn_rcpf(dx), __builtin_amdgcn_rcpf(dy), __builtin_amdgcn_rcpf(dz)};
}
// the ray against the root's own box (BoundingBox::boxIntersect, exact)
__device__ __forceinline__ bool root_hit(const DNode &root, const WalkRay &r) {
    return box_hit_verified(root.bmin, r.ox, r.oy, r.oz, r.bx, r.by, r.bz, r.brx, r.bry, r.brz);
}
// what a closest-hit walk returns; found(): the face is one of the scene's
struct Hit { float t; int face; };
__device__ __forceinline__ bool found(const int face, const uint32_t n_faces) { return face >= 0 && static_cast<uint32_t>(face) < n_faces; }
// walk<ANY = true> returns `occluded`, walk<ANY = false> the closest hit
template <bool ANY>
__device__ __forceinline__ auto walk_result(const float best_t, const int best_f, const bool occluded) {
    if constexpr (ANY) return occluded;
    else return Hit{best_t, best_f};
}
// bits [0, n) of a lane mask
__device__ __forceinline__ unsigned long long low_mask(const uint32_t n) { return n >= 64u ? ~0ull : ((1ull << n) - 1ull); }

struct ShardedQueue {
    uint32_t *ctr;
    uint32_t total, chunk, nchunks, shard, tries, fetched, cur, cur_end;
    uint32_t local;          // 0: strided chunks, interleaved heads (balance first); else: chunks of `local` CONSECUTIVE units and head x
                             // owns the x-th eighth of the unit range (locality first: scenes that do not fit the 4 MB L2 of an XCD)
    int lane;
    __device__ __forceinline__ uint32_t chunks_of(uint32_t s) const {         // index range of head s (some ids may fall past nchunks)
        if (local) { const uint32_t per = (nchunks + RT_QUEUE_SHARDS - 1u) / RT_QUEUE_SHARDS; return per; }
        const uint32_t groups = (nchunks + 31u) / 32u;
        return (groups / RT_QUEUE_SHARDS + ((groups % RT_QUEUE_SHARDS) > s ? 1u : 0u)) * 32u;
    }
    __device__ __forceinline__ uint32_t grab() {
        uint32_t v = 0;
        if (lane == 0) v = atomicAdd(&ctr[shard * 16u], 1u);
        return v;
    }
    // static variant (no atomics at all): wave w owns units w, w + W, w + 2W, ...  Best when units are cheap and
    // uniform (primary tiles: measured 0.25 ms static vs 0.39 ms dynamic on the cube frame).
    __device__ __forceinline__ void init_static(uint32_t total_units, uint32_t total_waves, uint32_t wave_id, int ln) {
        local = 0u;
        ctr = nullptr; total = 0u; lane = ln; chunk = 1u; nchunks = total_waves; shard = 0; tries = 0; fetched = 0;
        cur = wave_id; cur_end = total_units;
    }
    __device__ __forceinline__ void init(uint32_t *heads, uint32_t total_units, uint32_t total_waves, uint32_t home, int ln, uint32_t local_chunk = 0u, uint32_t div = 6u) {
        ctr = heads; total = total_units; lane = ln; local = local_chunk;
        chunk = total_units / (total_waves * div);
        if (chunk < 1u) chunk = 1u;
        if (local) chunk = local;
        nchunks = (total_units + chunk - 1u) / chunk;          // chunk c = { c + j * nchunks }   (local: { c * chunk + j })
        shard = home % RT_QUEUE_SHARDS; tries = 0; cur = 0; cur_end = 0;
        fetched = total ? grab() : 0u;
    }
    __device__ __forceinline__ bool next(uint32_t &unit) {
        // a chunk is NOT a run of consecutive units: chunk c owns units c, c + nchunks, c + 2*nchunks, ...  Expensive
        // units cluster (neighbouring hit points cross the same 979-triangle leaves); consecutive membership made
        // single chunks 5x heavier than average and doubled the kernel's tail.
        if (cur < cur_end) { unit = cur; cur += local ? 1u : nchunks; return true; }
        if (total == 0u) return false;
        for (;;) {
            const uint32_t idx = uniform_u32(fetched);
            if (idx < chunks_of(shard)) {
                // head `shard` owns GROUPS of 32 consecutive chunk ids, groups dealt round-robin over the 8 heads: inside a
                // group the waves of one XCD work on neighbouring hit points (same leaves -> that XCD's 4 MB L2) while the
                // fine interleave keeps the heads equally loaded (fully contiguous ownership measured +17 % on dodge,
                // chunk-granular interleave +5 % on the 1M-triangle scene)
                const uint32_t c = local ? shard * chunks_of(shard) + idx : ((idx / 32u) * RT_QUEUE_SHARDS + shard) * 32u + (idx % 32u);
                fetched = grab();                     // prefetch the following chunk index
                if (c >= nchunks) { cur = 0; cur_end = 0; continue; }     // id past the end of the last partial group
                if (local) {
                    unit = c * chunk;
                    cur = unit + 1u;
                    cur_end = unit + chunk < total ? unit + chunk : total;
                    return true;
                }
                unit = c;
                cur = c + nchunks;
                cur_end = total;
                return true;
            }
            for (;;) {
                if (++tries >= RT_QUEUE_SHARDS) return false;
                shard = (shard + 1u) % RT_QUEUE_SHARDS;
                const uint32_t seen = uniform_u32(__hip_atomic_load(&ctr[shard * 16u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if (seen < chunks_of(shard)) break;
            }
            fetched = grab();
        }
    }
};

struct WaveStack {
    uint32_t *node;
    unsigned long long *mask;
    uint4 *stage;            // per-wave LDS staging buffer: RT_STAGE_TRIS leaf-triangle records (80 B each)
};
#define RT_STAGE_TRIS 64
#ifndef RT_LDS_NODES
#define RT_LDS_NODES 256        // DNodes of the top of the tree kept in LDS by k_shadow (16 KB per block)
#endif
#define RT_SCALAR_LEAF_MAX 16   // leaves up to this size are walked with scalar loads straight from the scalar cache

// Wave-uniform octree walk for 64 rays.
//   ANY   = false: closest hit (flyscene.cpp:675-683): min t over candidates with t > 1e-5, ties to the lowest
//                  face id.  No t-ordered pruning: the reference tests every triangle of every intersected leaf,
//                  and because its tree loses/misfiles triangles a pruned walk would not be equivalent.
//   ANY   = true : lightStrikes (flyscene.cpp:912-954): visible iff min t >= 0.98, i.e. occluded iff SOME candidate
//                  (not illum 9) has 1e-5 < t < 0.98 -- so a lane may stop at its first occluder (exact).
//   COUNT = true : no early-out; counts boxIntersect calls / leaf face references with the reference's semantics
//                  (every pushed node is box-tested again when popped, boxTree.cpp:158,164).
// ---- explicit scalar load of a wave-uniform TriRec ----------------------------------------------------------------
// hipcc only selects s_load for a uniform global load when it can prove the memory unclobbered, which depends on code
// shape (it fell back to 64-lane global_loads in the flat kernels, and split the record into three dependent waits
// elsewhere).  The records are read-only for the kernel's lifetime, so the load is spelt out: s_load_dwordx16 +
// s_load_dwordx4 + ONE s_waitcnt inside a single asm statement (no output is visible before its wait; an asynchronous
// issue/wait split was tried and is unsafe: the compiler may copy the destination SGPRs before the data lands).
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ TriRec tri_load_uniform(const TriRec *p) {
    u32x16 lo;
    u32x4 hi;
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx4 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(lo), "=&s"(hi) : "s"(p) : "memory");
    TriRec t;
    t.ax = __uint_as_float(lo[0]); t.ay = __uint_as_float(lo[1]); t.az = __uint_as_float(lo[2]);
    t.e0x = __uint_as_float(lo[3]); t.e0y = __uint_as_float(lo[4]); t.e0z = __uint_as_float(lo[5]);
    t.e1x = __uint_as_float(lo[6]); t.e1y = __uint_as_float(lo[7]); t.e1z = __uint_as_float(lo[8]);
    t.nx = __uint_as_float(lo[9]); t.ny = __uint_as_float(lo[10]); t.nz = __uint_as_float(lo[11]);
    t.nA = __uint_as_float(lo[12]); t.d00 = __uint_as_float(lo[13]); t.d01 = __uint_as_float(lo[14]); t.d11 = __uint_as_float(lo[15]);
    t.inv_denom = __uint_as_float(hi[0]); t.face = hi[1]; t.flags = hi[2]; t.pad = 0u;
    return t;
}

// Plane culling for shadow units.  All 64 segments of a k_shadow unit end at the same point h (the shaded hit) and start
// at light samples inside the box [slo, shi].  Flyscene::rayTriangleIntersection (flyscene.cpp:787-819) accepts a triangle
// only for 0.00001 < t, and lightStrikes (flyscene.cpp:874-899) only counts t < 0.98, with
//      t = num / dn,   num = n.A - s.n,   dn = (h - s).n          (float, Eigen order)
// so a triangle is irrelevant for EVERY segment of the unit when interval arithmetic over the sample box proves
//   (A) num and dn have opposite signs (t <= 0: the plane lies behind the light sample), or
//   (B) |num| >= 0.981 |dn| (|t| >= 0.98: the plane is not crossed before the hit point -- this covers the face h lies on).
// Only signs and magnitudes of the reference's own two dot products are used, each bounded with a margin M = 2e-5 x the
// operand magnitudes (>= 20x the worst-case float rounding of the reference's evaluation and of the interval arithmetic),
// so the decision never depends on how accurate t is; a NaN anywhere makes every comparison false (= keep).
struct SegPacket {
    bool on;
    bool prepared;                 // the sample box is the one the lanes' LanePlane.sn_lo/sn_hi were prepared for
    float hx, hy, hz;              // common end point
    float slx, sly, slz, shx, shy, shz;   // box of the start points (exact extreme samples)
    float m0;                      // 2e-5 * (|slo|_1 + |shi|_1 + |h|_1)
};
__device__ __forceinline__ SegPacket seg_off() { return SegPacket{false, false, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }

__device__ __forceinline__ bool plane_rules_out(const SegPacket &g, const float nx, const float ny, const float nz, const float nA) {
    const float ax = nx * g.slx, bx = nx * g.shx, ay = ny * g.sly, by = ny * g.shy, az = nz * g.slz, bz = nz * g.shz;
    const float sn_lo = fminf(ax, bx) + (fminf(ay, by) + fminf(az, bz));
    const float sn_hi = fmaxf(ax, bx) + (fmaxf(ay, by) + fmaxf(az, bz));
    const float num_lo = nA - sn_hi, num_hi = nA - sn_lo;
    const float cx = nx * (g.hx - g.shx), dx = nx * (g.hx - g.slx), cy = ny * (g.hy - g.shy), dy = ny * (g.hy - g.sly),
                cz = nz * (g.hz - g.shz), dz = nz * (g.hz - g.slz);
    const float dn_lo = fminf(cx, dx) + (fminf(cy, dy) + fminf(cz, dz));
    const float dn_hi = fmaxf(cx, dx) + (fmaxf(cy, dy) + fmaxf(cz, dz));
    const float M = g.m0 + 2e-5f * fabsf(nA);
    const bool sane = (fabsf(nx) + fabsf(ny) + fabsf(nz) <= 4.0f) && (fabsf(nA) <= 1e30f);
    const bool opposite = (num_lo > M && dn_hi < -M) || (num_hi < -M && dn_lo > M);
    const float min_abs_num = fmaxf(num_lo, -num_hi);              // <= 0 when the interval straddles zero
    const float max_abs_dn = fmaxf(fabsf(dn_lo), fabsf(dn_hi));
    const bool beyond = (min_abs_num - M) >= 0.981f * (max_abs_dn + M);
    return sane && (num_lo <= num_hi) && (dn_lo <= dn_hi) && (opposite || beyond);
}

// The same decision when the sample box is the one the lane prepared its plane for before the unit loop (scene light 0): the
// interval of s.n over the box (sn_lo, sn_hi) is a per-triangle constant, and (h - s).n = h.n - s.n turns the second interval
// into one dot product.  ~20 VALU instructions instead of ~45 per unit.
struct LanePlane { float nx, ny, nz, nA, sn_lo, sn_hi; };
__device__ __forceinline__ void plane_prepare(LanePlane &pl, const float slx, const float sly, const float slz, const float shx, const float shy, const float shz) {
    const float ax = pl.nx * slx, bx = pl.nx * shx, ay = pl.ny * sly, by = pl.ny * shy, az = pl.nz * slz, bz = pl.nz * shz;
    pl.sn_lo = fminf(ax, bx) + (fminf(ay, by) + fminf(az, bz));
    pl.sn_hi = fmaxf(ax, bx) + (fmaxf(ay, by) + fmaxf(az, bz));
}
__device__ __forceinline__ bool plane_rules_out_prepared(const SegPacket &g, const LanePlane &pl) {
    const float num_lo = pl.nA - pl.sn_hi, num_hi = pl.nA - pl.sn_lo;
    const float hn = pl.nx * g.hx + (pl.ny * g.hy + pl.nz * g.hz);
    const float dn_lo = hn - pl.sn_hi, dn_hi = hn - pl.sn_lo;
    const float M = g.m0 + 2e-5f * fabsf(pl.nA);
    const bool sane = (fabsf(pl.nx) + fabsf(pl.ny) + fabsf(pl.nz) <= 4.0f) && (fabsf(pl.nA) <= 1e30f);
    const bool opposite = (num_lo > M && dn_hi < -M) || (num_hi < -M && dn_lo > M);
    const float min_abs_num = fmaxf(num_lo, -num_hi);
    const float max_abs_dn = fmaxf(fabsf(dn_lo), fabsf(dn_hi));
    const bool beyond = (min_abs_num - M) >= 0.981f * (max_abs_dn + M);
    return sane && (num_lo <= num_hi) && (dn_lo <= dn_hi) && (opposite || beyond);
}

// How a packet walk starts and when it gives work away.
struct WalkCtl {
    bool resume;                      // leaf task: process chunks [c_begin, c_end) of leaf `start_node` for `start_mask`, nothing else
    uint32_t start_node;
    unsigned long long start_mask;
    uint32_t c_begin, c_end;
    uint32_t budget;                  // 0 = process every leaf inline; otherwise leaves whose estimated cost exceeds it become tasks
    uint32_t unit;                    // unit id stored in the emitted tasks
    ContTask *tasks;                  // output queue (capacity task_cap) and its counter
    uint32_t *task_count;
    uint32_t target;                  // estimated cost of one task piece
    uint32_t task_cap;
    SegPacket seg;                    // shadow units: plane culling (off for every other kind of packet)
    unsigned long long skip;          // flat scenes: triangles of the root leaf that no ray of the unit can hit (bit = position in the leaf)
    const float4 *cone;               // per-wave LDS record of the packet's cone (common origin, box of the ray targets): the lane = triangle test of the leaves; nullptr = none
    bool cone_box;                    // counted hits lie before the targets (t < 0.98: light-centre segments): the AABB of hull(origin, targets) bounds them too
};
// (defined with the shaft code below)
__device__ __forceinline__ bool tri_outside_cone(const float4 *rec, const TriRec &tr, const float m, const bool use_box);
#ifndef RT_TRI_SHAFT_MIN
#define RT_TRI_SHAFT_MIN 8            // live rays on a chunk from which the per-triangle test (~3 triangle steps) is run
#endif
#ifndef RT_RAYMODE_EXTRA
#define RT_RAYMODE_EXTRA 8u          // scalar loads of the survivors' records
#endif
__device__ __forceinline__ WalkCtl walk_plain() {
    WalkCtl w{};
    w.target = 1u; w.seg = seg_off();
    return w;
}

__device__ __forceinline__ TriRec tri_from_regs(const u32x16 &lo, const u32x4 &hi) {
    TriRec t;
    t.ax = __uint_as_float(lo[0]); t.ay = __uint_as_float(lo[1]); t.az = __uint_as_float(lo[2]);
    t.e0x = __uint_as_float(lo[3]); t.e0y = __uint_as_float(lo[4]); t.e0z = __uint_as_float(lo[5]);
    t.e1x = __uint_as_float(lo[6]); t.e1y = __uint_as_float(lo[7]); t.e1z = __uint_as_float(lo[8]);
    t.nx = __uint_as_float(lo[9]); t.ny = __uint_as_float(lo[10]); t.nz = __uint_as_float(lo[11]);
    t.nA = __uint_as_float(lo[12]); t.d00 = __uint_as_float(lo[13]); t.d01 = __uint_as_float(lo[14]); t.d11 = __uint_as_float(lo[15]);
    t.inv_denom = __uint_as_float(hi[0]); t.face = hi[1]; t.flags = hi[2]; t.pad = 0u;
    return t;
}
// two consecutive records (p[0], p[1]) with ONE wait: the caller tests both in straight-line code, which puts two
// independent division/dot-product chains in flight per wave
__device__ __forceinline__ void tri_load_uniform2(const TriRec *p, TriRec &a, TriRec &b) {
    u32x16 lo0, lo1;
    u32x4 hi0, hi1;
    asm volatile("s_load_dwordx16 %0, %4, 0x0\n\ts_load_dwordx4 %1, %4, 0x40\n\ts_load_dwordx16 %2, %4, 0x50\n\ts_load_dwordx4 %3, %4, 0x90\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(lo0), "=&s"(hi0), "=&s"(lo1), "=&s"(hi1) : "s"(p) : "memory");
    a = tri_from_regs(lo0, hi0);
    b = tri_from_regs(lo1, hi1);
}

// same, for two records that are not neighbours
__device__ __forceinline__ const TriRec *uniform_ptr(const TriRec *p) {
    // (folds away when the compiler already knows the value is wave-uniform; under SGPR pressure it may have parked the pointer in a VGPR)
    return reinterpret_cast<const TriRec *>(uniform_u64(reinterpret_cast<unsigned long long>(p)));
}
__device__ __forceinline__ void tri_load_uniform_pair(const TriRec *pa_, const TriRec *pb_, TriRec &a, TriRec &b) {
    const TriRec *pa = uniform_ptr(pa_), *pb = uniform_ptr(pb_);
    u32x16 lo0, lo1;
    u32x4 hi0, hi1;
    asm volatile("s_load_dwordx16 %0, %4, 0x0\n\ts_load_dwordx4 %1, %4, 0x40\n\ts_load_dwordx16 %2, %5, 0x0\n\ts_load_dwordx4 %3, %5, 0x40\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(lo0), "=&s"(hi0), "=&s"(lo1), "=&s"(hi1) : "s"(pa), "s"(pb) : "memory");
    a = tri_from_regs(lo0, hi0);
    b = tri_from_regs(lo1, hi1);
}

__device__ __forceinline__ float lane_f(float v, int src_lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}

// Counting build (-DRT_WORK_COUNTERS, `make work`): the shipped kernels + wave-level step counters, one atomic per counted step by lane 0
// (slow, never timed).  The indices are the WORK_* names of rt_device.hpp; k_set_prof points the launches that follow at their region.
#ifdef RT_WORK_COUNTERS
__device__ unsigned long long *g_prof = nullptr;
__device__ uint32_t g_prof_base = 0u;       // step counters of the launch in flight go to prof[g_prof_base + idx]: 0 = trace kernels, RT_WORK_SHADOW = shadow kernels
#define RT_PROF_ADD(lane, idx, val) do { const unsigned long long pv_ = static_cast<unsigned long long>(val); if ((lane) == 0 && g_prof) atomicAdd(&g_prof[g_prof_base + (idx)], pv_); } while (0)
#else
#define RT_PROF_ADD(lane, idx, val) do { } while (0)
#endif

// Per-leaf choice between the two lane mappings (wave-uniform): issue-cost estimates in VALU instructions.
#define RT_COST_RAY_MODE 45u      // per triangle, lanes = rays (all 64 lanes step through every triangle)
#define RT_COST_TRI_MODE 58u      // per (active ray, 64-triangle chunk), lanes = triangles
#define RT_COST_CHUNK_TEST 30u    // per chunk: conservative bound test for all 64 rays at once

// One leaf of a packet walk: every triangle of the leaf is a candidate for the rays in `live` (BoxTree::intersect inserts all faces of an
// intersected leaf, boxTree.cpp:158-160).  Shared by the stack walk (packet_walk) and the shaft-culled breadth-first walk of the shadow units.
struct RayLane {
    float ox, oy, oz;        // origin
    float dx, dy, dz;        // triangle-test direction
    float idx, idy, idz;     // v_rcp_f32 of the box-test direction (conservative tests only)
    float slab_pad;
};
// The conservative box tests (content boxes of nodes, chunk boxes of big leaves) only ever SKIP work, so approximate
// arithmetic is fine: they use the v_rcp_f32 reciprocals of the box-test direction that the ray already holds (it is the
// triangle-test direction up to one rounding).  A zero component gives inf: an origin inside that slab yields (-inf, +inf) = no
// constraint, one outside yields tin = +inf = miss (both correct for a line parallel to the slab), 0 * inf = NaN keeps the box.
__device__ __forceinline__ RayLane make_ray_lane(const WalkRay &r, const float extent) {
    return RayLane{r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, r.brx, r.bry, r.brz, 4e-4f * (fabsf(r.ox) + fabsf(r.oy) + fabsf(r.oz) + extent)};
}
template <bool ANY, bool COUNT, bool STAGED = true>
__device__ __forceinline__ void leaf_visit(const DNode &nd, const uint32_t ni, const TriRec *__restrict__ tris, const ChunkBound *__restrict__ chunks,
                                           const uint32_t *__restrict__ leaf_chunk0, const WaveStack stk, const int lane, const WalkCtl &wc,
                                           const RayLane &R, unsigned long long live, bool mine,
                                           float &best_t, int &best_f, bool &occluded, uint32_t &cnt_ref, uint32_t &cnt_sig) {
    const float ox = R.ox, oy = R.oy, oz = R.oz, dx = R.dx, dy = R.dy, dz = R.dz;
    const float idx_ = R.idx, idy_ = R.idy, idz_ = R.idz, slab_pad = R.slab_pad;
    const uint32_t cnt = nd.count_flags & 0x7fffffffu;
    if (COUNT && mine) { cnt_ref += cnt; cnt_sig += ni * 2654435761u; }      // cnt_sig: signature of the ray's set of intersected leaves (rt_tree_probe)
    const TriRec *__restrict__ T = tris + nd.first;
    const uint32_t nchunk = (cnt + 63u) >> 6;
    // lanes=triangles estimate: one bound test per chunk + live rays x the share of chunks a ray cannot skip
    // STAGED = false (kernels without the LDS staging buffer): leaves too large for the scalar-load walk always take lanes = triangles
    const bool tri_mode = (!STAGED && cnt > RT_SCALAR_LEAF_MAX) ||
                          nchunk * RT_COST_CHUNK_TEST + static_cast<uint32_t>(__popcll(live)) * ((nchunk + 2u) / 3u) * RT_COST_TRI_MODE
                          < cnt * RT_COST_RAY_MODE;
    const uint32_t est = tri_mode ? nchunk * RT_COST_CHUNK_TEST + static_cast<uint32_t>(__popcll(live)) * ((nchunk + 2u) / 3u) * RT_COST_TRI_MODE
                                  : cnt * RT_COST_RAY_MODE;
    uint32_t cb = 0u, ce = nchunk;                       // chunk range processed here
    if (wc.resume) {
        cb = wc.c_begin; ce = wc.c_end < nchunk ? wc.c_end : nchunk;
    } else if (wc.budget != 0u && est > wc.budget) {
        // hand the leaf away as ~target-instruction pieces (whole chunks); one atomic reserves the slots
        uint32_t ntask = (est + wc.target - 1u) / wc.target;
        if (ntask > nchunk) ntask = nchunk;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(wc.task_count, ntask);
        base = uniform_u32(base);
        // The counter only ever grows (the consumer clamps it to the capacity): pieces that fall past the end of the
        // queue are simply processed here.  (Giving a failed reservation back with an atomicSub is unsound: a later
        // reservation can land inside the window and end up beyond the final count.)
        const uint32_t fit = base >= wc.task_cap ? 0u : (ntask < wc.task_cap - base ? ntask : wc.task_cap - base);
        for (uint32_t i = static_cast<uint32_t>(lane); i < fit; i += 64u) {
            ContTask t;
            t.unit = wc.unit; t.node = ni; t.mask = live;
            t.c_begin = static_cast<uint32_t>(static_cast<unsigned long long>(nchunk) * i / ntask);
            t.c_end = static_cast<uint32_t>(static_cast<unsigned long long>(nchunk) * (i + 1u) / ntask);
            t.pad0 = t.pad1 = 0u;
            wc.tasks[base + i] = t;
        }
        if (fit == ntask) return;
        cb = static_cast<uint32_t>(static_cast<unsigned long long>(nchunk) * fit / ntask);       // the rest of the leaf, inline
    }
    RT_PROF_ADD(lane, tri_mode ? WORK_LEAVES_LANES_TRIANGLES : WORK_LEAVES_LANES_RAYS, 1);
    if (tri_mode) {
        RT_PROF_ADD(lane, WORK_LEAF_LIVE_RAYS, __popcll(live));
        // ---- lanes = triangles.  Each lane keeps ONE leaf triangle in registers (coalesced 80-B records, next
        // chunk prefetched); the active rays are broadcast one at a time with v_readlane and every lane tests
        // its triangle against that ray.  A ballot reports the hits: exact early-out per ray for shadow rays,
        // and a scalar pick of the (t, face) minimum for closest hit.  No per-triangle memory round trip.
        unsigned long long occ_new = 0ull;
        const ChunkBound *__restrict__ cbounds = chunks + nd.pad[0];      // first chunk bound of the leaf (rt_scene_image.cpp: DNode.pad[0])
        // per-ray quantities of the conservative chunk test (approximate arithmetic is fine: they only ever SKIP
        // work); computed per leaf visit so that scenes that never take this mode (the cube) pay nothing
        const uint32_t t_end = ce * 64u < cnt ? ce * 64u : cnt;
        TriRec tr = T[cb * 64u + static_cast<uint32_t>(lane) < cnt ? cb * 64u + static_cast<uint32_t>(lane) : 0u];
        for (uint32_t c0 = cb * 64u; c0 < t_end; c0 += 64u) {
            const uint32_t n = cnt - c0 < 64u ? cnt - c0 : 64u;
            const bool has = static_cast<uint32_t>(lane) < n && !(ANY && (tr.flags & 1u));
            // conservative chunk test (lanes = rays): a live ray skips the chunk when no point of its line that a hit could
            // count at lies in the chunk's inflated box (rt_scene_image.cpp, build_chunk_bounds, has the error analysis)
            unsigned long long todo = live;
            const ChunkBound bd = cbounds[c0 >> 6];
            {
                if (bd.never < 1.5f) {
                    RT_PROF_ADD(lane, WORK_CHUNK_TESTS_STACK_WALK, 1);
                    const float t0x = (bd.lo[0] - slab_pad - ox) * idx_, t1x = (bd.hi[0] + slab_pad - ox) * idx_;
                    const float t0y = (bd.lo[1] - slab_pad - oy) * idy_, t1y = (bd.hi[1] + slab_pad - oy) * idy_;
                    const float t0z = (bd.lo[2] - slab_pad - oz) * idz_, t1z = (bd.hi[2] + slab_pad - oz) * idz_;
                    const float tin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
                    const float tout = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
                    // the line misses the box, or only meets it where no hit can count: behind the origin (t <= 0.00001 is
                    // never accepted), and beyond 0.98 for a shadow ray / beyond the current closest hit otherwise
                    // (t of an accepted hit lies in [tin, tout] up to ~1e-6 relative: its point is inside the padded box)
                    const bool miss = (tin > tout) || (tout < -1e-3f) ||
                                      (ANY ? (tin > 0.981f) : (tin > best_t + 1e-3f * (1.0f + fabsf(best_t))));
                    const unsigned long long culled = __ballot(miss) & live;
                    todo = live & ~culled;
                    RT_PROF_ADD(lane, WORK_RAY_CHUNK_PAIRS_CULLED, __popcll(culled));
                }
            }
            // lane = triangle cone test (packets with a common origin: primary tiles, light-centre segments): the triangles of the chunk that
            // ANY ray of the packet can hit (tri_outside_cone); few survivors and many rays -> lanes = rays over the survivors
            bool has_c = has;
            if (!COUNT && wc.cone != nullptr && static_cast<uint32_t>(__popcll(todo)) >= RT_TRI_SHAFT_MIN && bd.never < 1.5f) {
                __builtin_amdgcn_wave_barrier();
                has_c = has && !tri_outside_cone(wc.cone, tr, bd.infl * 1.0625f, wc.cone_box);
                unsigned long long tmask = __ballot(has_c);
                RT_PROF_ADD(lane, WORK_TRI_SHAFT_TESTS, 1); RT_PROF_ADD(lane, WORK_TRI_SHAFT_SURVIVORS, __popcll(tmask)); RT_PROF_ADD(lane, WORK_TRI_SHAFT_RAYS, __popcll(todo)); RT_PROF_ADD(lane, WORK_TRI_SHAFT_EMPTY_CHUNKS, tmask == 0ull ? 1 : 0);
                if (tmask == 0ull) {
                    todo = 0ull;
                } else if (static_cast<uint32_t>(__popcll(tmask)) * (RT_COST_RAY_MODE + RT_RAYMODE_EXTRA) < static_cast<uint32_t>(__popcll(todo)) * RT_COST_TRI_MODE) {
                    const bool my = ((todo >> lane) & 1ull) != 0ull;
                    bool occ_r = false;
                    const TriRec *__restrict__ Tc = T + c0;
                    auto ray_lane = [&](const TriRec &ta) {
                        // Flyscene::rayTriangleIntersection, flyscene.cpp:787-819 (lanes = rays)
                        const float dn = dot3(dx, dy, dz, ta.nx, ta.ny, ta.nz);
                        const float t = (ta.nA - dot3(ox, oy, oz, ta.nx, ta.ny, ta.nz)) / dn;
                        const float v2x = (ox + t * dx) - ta.ax, v2y = (oy + t * dy) - ta.ay, v2z = (oz + t * dz) - ta.az;
                        const float d02 = dot3(ta.e0x, ta.e0y, ta.e0z, v2x, v2y, v2z);
                        const float d12 = dot3(ta.e1x, ta.e1y, ta.e1z, v2x, v2y, v2z);
                        const float u = (ta.d11 * d02 - ta.d01 * d12) * ta.inv_denom;
                        const float v = (ta.d00 * d12 - ta.d01 * d02) * ta.inv_denom;
                        const bool ok = my && !(ANY && (ta.flags & 1u)) && (dn != 0) && (u >= 0) && (v >= 0) && (u + v < 1) && (t > 0.00001f);
                        if (ANY) {
                            occ_r = occ_r || (ok && t < 0.98f);
                        } else {
                            const bool better = ok && (t < best_t || (t == best_t && static_cast<int>(ta.face) < best_f));
                            best_t = better ? t : best_t;
                            best_f = better ? static_cast<int>(ta.face) : best_f;
                        }
                    };
                    while (tmask != 0ull) {
                        const uint32_t j0 = static_cast<uint32_t>(__builtin_ctzll(tmask));
                        tmask &= tmask - 1ull;
                        const bool two = tmask != 0ull;
                        const uint32_t j1 = two ? static_cast<uint32_t>(__builtin_ctzll(tmask)) : j0;
                        if (two) tmask &= tmask - 1ull;
                        RT_PROF_ADD(lane, WORK_TRI_STEPS_LANES_RAYS, two ? 2 : 1);
                        TriRec ta, tb;
                        tri_load_uniform_pair(Tc + j0, Tc + j1, ta, tb);
                        ray_lane(ta);
                        ray_lane(tb);                 // (j1 == j0 for an odd tail: the same triangle twice changes nothing)
                        if (ANY && __ballot(my && !occ_r) == 0ull) break;
                    }
                    if (ANY) {
                        const unsigned long long ob = __ballot(occ_r);
                        occ_new |= ob;
                        live &= ~ob;
                    }
                    todo = 0ull;
                }
            }
            // step 3 (lanes = triangles): full test of the surviving rays, two rays per step for ILP (two independent
            // division chains in flight)
            while (todo != 0ull) {
                const int r0 = static_cast<int>(__builtin_ctzll(todo));
                todo &= todo - 1ull;
                const bool two = todo != 0ull;
                const int r1 = two ? static_cast<int>(__builtin_ctzll(todo)) : r0;
                if (two) todo &= todo - 1ull;
                RT_PROF_ADD(lane, WORK_TRI_STEPS_LANES_TRIANGLES, two ? 2 : 1); RT_PROF_ADD(lane, WORK_TRI_USEFUL_LANES_TRIANGLES, (two ? 2 : 1) * __popcll(__ballot(has_c)));
                // Flyscene::rayTriangleIntersection, flyscene.cpp:787-819 (same operations as the ray-lane form)
                float tq[2]; bool inq[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int r = q == 0 ? r0 : r1;
                    const float rdx = lane_f(dx, r), rdy = lane_f(dy, r), rdz = lane_f(dz, r);
                    const float rox = lane_f(ox, r), roy = lane_f(oy, r), roz = lane_f(oz, r);
                    const float dn = dot3(rdx, rdy, rdz, tr.nx, tr.ny, tr.nz);
                    const float t = (tr.nA - dot3(rox, roy, roz, tr.nx, tr.ny, tr.nz)) / dn;
                    const float v2x = (rox + t * rdx) - tr.ax, v2y = (roy + t * rdy) - tr.ay, v2z = (roz + t * rdz) - tr.az;
                    const float d02 = dot3(tr.e0x, tr.e0y, tr.e0z, v2x, v2y, v2z);
                    const float d12 = dot3(tr.e1x, tr.e1y, tr.e1z, v2x, v2y, v2z);
                    const float u = (tr.d11 * d02 - tr.d01 * d12) * tr.inv_denom;
                    const float v = (tr.d00 * d12 - tr.d01 * d02) * tr.inv_denom;
                    tq[q] = t;
                    inq[q] = has_c && (dn != 0) && (u >= 0) && (v >= 0) && (u + v < 1) && (t > 0.00001f);
                }
                if (!two) inq[1] = false;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int r = q == 0 ? r0 : r1;
                    if (ANY) {
                        if (__ballot(inq[q] && tq[q] < 0.98f) != 0ull) {
                            occ_new |= 1ull << r;
                            if (!COUNT) live &= ~(1ull << r);
                        }
                    } else {
                        unsigned long long hm = __ballot(inq[q]);
                        if (hm != 0ull) {
                            float bt = lane_f(best_t, r);
                            int bf = __builtin_amdgcn_readlane(best_f, r);
                            do {
                                const int l = static_cast<int>(__builtin_ctzll(hm));
                                hm &= hm - 1ull;
                                const float tl = lane_f(tq[q], l);
                                const int fl = __builtin_amdgcn_readlane(static_cast<int>(tr.face), l);
                                if (tl < bt || (tl == bt && fl < bf)) { bt = tl; bf = fl; }
                            } while (hm != 0ull);
                            if (lane == r) { best_t = bt; best_f = bf; }
                        }
                    }
                }
            }
            if (ANY && !COUNT && live == 0ull) break;
            { const uint32_t nx = c0 + 64u + static_cast<uint32_t>(lane); if (c0 + 64u < t_end) tr = T[nx < cnt ? nx : 0u]; }
        }
        if (ANY) occluded = occluded || (((occ_new >> lane) & 1ull) != 0ull);
    } else {
        // ---- lanes = rays: every lane steps through the leaf's triangles for its own ray.
        // Small leaves: the records are wave-uniform scalar loads (s_load_dwordx16 + x4, scalar cache).
        // Larger leaves: 64-triangle chunks are staged into this wave's LDS buffer with coalesced 16-byte
        // loads (ONE memory round trip per chunk instead of one per triangle), then read back as LDS
        // broadcasts (all lanes the same address), software-pipelined one record ahead.
        auto test_lane = [&](const TriRec &tr) {
            // Flyscene::rayTriangleIntersection, flyscene.cpp:787-819 (straight-line form, see flat_walk)
            const float dn = dot3(dx, dy, dz, tr.nx, tr.ny, tr.nz);
            const float t = (tr.nA - dot3(ox, oy, oz, tr.nx, tr.ny, tr.nz)) / dn;
            const float v2x = (ox + t * dx) - tr.ax, v2y = (oy + t * dy) - tr.ay, v2z = (oz + t * dz) - tr.az;
            const float d02 = dot3(tr.e0x, tr.e0y, tr.e0z, v2x, v2y, v2z);
            const float d12 = dot3(tr.e1x, tr.e1y, tr.e1z, v2x, v2y, v2z);
            const float u = (tr.d11 * d02 - tr.d01 * d12) * tr.inv_denom;
            const float v = (tr.d00 * d12 - tr.d01 * d02) * tr.inv_denom;
            const bool ok = mine && !(ANY && (tr.flags & 1u)) && (dn != 0) && (u >= 0) && (v >= 0) && (u + v < 1) && (t > 0.00001f);
            if (ANY) {
                occluded = occluded || (ok && t < 0.98f);
            } else {
                const bool better = ok && (t < best_t || (t == best_t && static_cast<int>(tr.face) < best_f));
                best_t = better ? t : best_t;
                best_f = better ? static_cast<int>(tr.face) : best_f;
            }
        };
        if (cnt <= RT_SCALAR_LEAF_MAX) {
            uint32_t k = 0;
            for (; k + 1u < cnt; k += 2u) {
                TriRec ta, tb;
                tri_load_uniform2(T + k, ta, tb);
                RT_PROF_ADD(lane, WORK_TRI_STEPS_LANES_RAYS, 2); RT_PROF_ADD(lane, WORK_TRI_USEFUL_LANES_RAYS, 2 * __popcll(__ballot(mine)));
                test_lane(ta);
                test_lane(tb);
            }
            if (k < cnt) {
                RT_PROF_ADD(lane, WORK_TRI_STEPS_LANES_RAYS, 1); RT_PROF_ADD(lane, WORK_TRI_USEFUL_LANES_RAYS, __popcll(__ballot(mine)));
                test_lane(tri_load_uniform(T + k));
            }
        } else if (STAGED) {
            const uint32_t r_end = ce * 64u < cnt ? ce * 64u : cnt;
            for (uint32_t c0 = cb * 64u; c0 < r_end; c0 += RT_STAGE_TRIS) {
                const uint32_t n = cnt - c0 < RT_STAGE_TRIS ? cnt - c0 : RT_STAGE_TRIS;
                const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(T + c0);
                __builtin_amdgcn_wave_barrier();
                for (uint32_t q = static_cast<uint32_t>(lane); q < n * 5u; q += 64u) stk.stage[q] = src[q];
                __builtin_amdgcn_wave_barrier();
                const TriRec *staged = reinterpret_cast<const TriRec *>(stk.stage);
                uint32_t k = 0;
                for (; k + 1u < n; k += 2u) {       // two records per step: two independent chains in flight
                    const TriRec ta = staged[k], tb = staged[k + 1u];
                    RT_PROF_ADD(lane, WORK_TRI_STEPS_LANES_RAYS, 2); RT_PROF_ADD(lane, WORK_TRI_USEFUL_LANES_RAYS, 2 * __popcll(__ballot(mine)));
                    test_lane(ta);
                    test_lane(tb);
                }
                if (k < n) {
                    RT_PROF_ADD(lane, WORK_TRI_STEPS_LANES_RAYS, 1); RT_PROF_ADD(lane, WORK_TRI_USEFUL_LANES_RAYS, __popcll(__ballot(mine)));
                    test_lane(staged[k]);
                }
                if (ANY && !COUNT) {
                    mine = mine && !occluded;
                    if (__ballot(mine) == 0ull) break;
                }
            }
        }
    }
}

template <bool ANY, bool COUNT, bool STAGED = true>
__device__ __forceinline__ auto packet_walk(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                            const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                            const float extent, const WaveStack stk, const int lane, const WalkCtl wc, bool in_root, const WalkRay &ray,
                                            uint32_t &cnt_box, uint32_t &cnt_ref, uint32_t &cnt_sig) {
    const RayLane R = make_ray_lane(ray, extent);
    const float ox = R.ox, oy = R.oy, oz = R.oz, idx_ = R.idx, idy_ = R.idy, idz_ = R.idz, slab_pad = R.slab_pad;
    float best_t = 3.402823466e+38f;
    int best_f = -1;
    bool occluded = false;
    int sp = 0;
    {
        unsigned long long m0 = __ballot(in_root);
        if (wc.resume) m0 &= wc.start_mask;
        if (m0 == 0ull) return walk_result<ANY>(best_t, best_f, occluded);
        if (COUNT && in_root && !wc.resume) cnt_box += 1;      // BoxTree::intersect re-tests the root it was just given
        stk.node[0] = wc.resume ? wc.start_node : 0u;
        stk.mask[0] = m0;
        sp = 1;
    }
    while (sp > 0) {
        --sp;
        __builtin_amdgcn_wave_barrier();
        const uint32_t ni = uniform_u32(stk.node[sp]);
        const unsigned long long m = uniform_u64(stk.mask[sp]);
        bool mine = ((m >> lane) & 1ull) != 0ull;
        if (ANY && !COUNT) mine = mine && !occluded;
        unsigned long long live = __ballot(mine);          // rays that still need this node
        if (live == 0ull) continue;
        const DNode nd = nodes[ni];
        const uint32_t cnt = nd.count_flags & 0x7fffffffu;
        if (nd.count_flags & RT_NODE_LEAF) {
            leaf_visit<ANY, COUNT, STAGED>(nd, ni, tris, chunks, leaf_chunk0, stk, lane, wc, R, live, mine, best_t, best_f, occluded, cnt_ref, cnt_sig);
        } else {
            for (uint32_t c = 0; c < cnt; ++c) {
                const uint32_t ci = nd.first + c;
                const DNode ch = nodes[ci];
                bool h = mine;
                if (!COUNT && ch.pad[1] == 0u) {         // pad[1]: a never-cullable chunk below -> the content box only bounds the rest
                    // content test first (it is the cheaper one and rules out most children): no countable point of the line
                    // inside the subtree's content box -> nothing below can be hit, whatever the reference's box test says
                    const float t0x = (ch.clo[0] - slab_pad - ox) * idx_, t1x = (ch.chi[0] + slab_pad - ox) * idx_;
                    const float t0y = (ch.clo[1] - slab_pad - oy) * idy_, t1y = (ch.chi[1] + slab_pad - oy) * idy_;
                    const float t0z = (ch.clo[2] - slab_pad - oz) * idz_, t1z = (ch.chi[2] + slab_pad - oz) * idz_;
                    const float tin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
                    const float tout = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
                    const bool miss = (tin > tout) || (tout < -1e-3f) ||
                                      (ANY ? (tin > 0.981f) : (tin > best_t + 1e-3f * (1.0f + fabsf(best_t))));
                    RT_PROF_ADD(lane, WORK_RAY_NODE_PAIRS_CONTENT_CULLED, __popcll(__ballot(h && miss)));
                    h = h && !miss;
                    if (__ballot(h) == 0ull) continue;
                }
                h = h && box_hit_verified(ch.bmin, ox, oy, oz, ray.bx, ray.by, ray.bz, ray.brx, ray.bry, ray.brz);   // BoundingBox::boxIntersect, exact
                RT_PROF_ADD(lane, WORK_BOX_STEPS_STACK_WALK, 1); RT_PROF_ADD(lane, WORK_BOX_USEFUL_STACK_WALK, __popcll(__ballot(mine)));
                if (COUNT && mine) cnt_box += h ? 2u : 1u;
                const unsigned long long hm = __ballot(h);
                if (hm != 0ull) {
                    stk.node[sp] = ci;           // same value from every lane
                    stk.mask[sp] = hm;
                    ++sp;
                }
            }
        }
    }
    return walk_result<ANY>(best_t, best_f, occluded);
}

// Flat scenes (the root is itself a small leaf -- cube.obj: 1 node, 12 triangles): no stack, no LDS, no mode choice;
// every ray that passes the root test steps through the same wave-uniform triangle list (scalar loads).
// Lane k of the wave keeps the plane (n, n.A) of root triangle k for the whole kernel (k_shadow): one plane_rules_out per
// unit then tells which of the root's triangles any of the unit's 64 segments can still be blocked by.

template <bool ANY, bool COUNT>
__device__ __forceinline__ auto flat_walk(const DNode &root, const TriRec *__restrict__ tris, bool in_root, const SegPacket &seg, const unsigned long long skip, const LanePlane &pl,
                                          const WalkRay &ray, uint32_t &cnt_box, uint32_t &cnt_ref) {
    const float ox = ray.ox, oy = ray.oy, oz = ray.oz, dx = ray.dx, dy = ray.dy, dz = ray.dz;
    float best_t = 3.402823466e+38f;
    int best_f = -1;
    bool occluded = false;
    if (__ballot(in_root) == 0ull) return walk_result<ANY>(best_t, best_f, occluded);
    const uint32_t cnt = root.count_flags & 0x7fffffffu;
    if (COUNT && in_root) { cnt_box += 1; cnt_ref += cnt; }
    const TriRec *__restrict__ T = tris + root.first;
    bool mine = in_root;
    auto test_one = [&](const TriRec &tr) {
        // Flyscene::rayTriangleIntersection, flyscene.cpp:787-819 -- straight-line form: every lane evaluates the same
        // operations (a zero d.n just produces inf/NaN that the final predicate rejects, exactly like the reference's early
        // `return -72`), which removes the exec-mask juggling of nested branches.
        const float dn = dot3(dx, dy, dz, tr.nx, tr.ny, tr.nz);
        const float t = (tr.nA - dot3(ox, oy, oz, tr.nx, tr.ny, tr.nz)) / dn;
        const float v2x = (ox + t * dx) - tr.ax, v2y = (oy + t * dy) - tr.ay, v2z = (oz + t * dz) - tr.az;
        const float d02 = dot3(tr.e0x, tr.e0y, tr.e0z, v2x, v2y, v2z);
        const float d12 = dot3(tr.e1x, tr.e1y, tr.e1z, v2x, v2y, v2z);
        const float u = (tr.d11 * d02 - tr.d01 * d12) * tr.inv_denom;
        const float v = (tr.d00 * d12 - tr.d01 * d02) * tr.inv_denom;
        const bool ok = mine && !(ANY && (tr.flags & 1u)) && (dn != 0) && (u >= 0) && (v >= 0) && (u + v < 1) && (t > 0.00001f);
        if (ANY) {
            occluded = occluded || (ok && t < 0.98f);
        } else {
            const bool better = ok && (t < best_t || (t == best_t && static_cast<int>(tr.face) < best_f));
            best_t = better ? t : best_t;
            best_f = better ? static_cast<int>(tr.face) : best_f;
        }
    };
    if (ANY && !COUNT && seg.on) {
        // shadow unit: only the triangles whose plane is crossed between a light sample and the hit point
        unsigned long long keep = low_mask(cnt) & ~skip;
        keep &= ~__ballot(seg.prepared ? plane_rules_out_prepared(seg, pl) : plane_rules_out(seg, pl.nx, pl.ny, pl.nz, pl.nA));
        RT_PROF_ADD(threadIdx.x & 63, WORK_LEAVES_LANES_RAYS, 1); RT_PROF_ADD(threadIdx.x & 63, WORK_TRI_USEFUL_LANES_RAYS, __popcll(keep));
        while (keep != 0ull) {
            const uint32_t k0 = static_cast<uint32_t>(__builtin_ctzll(keep));
            keep &= keep - 1ull;
            if (keep != 0ull) {
                const uint32_t k1 = static_cast<uint32_t>(__builtin_ctzll(keep));
                keep &= keep - 1ull;
                TriRec ta, tb;
                tri_load_uniform_pair(T + k0, T + k1, ta, tb);
                RT_PROF_ADD(threadIdx.x & 63, WORK_TRI_STEPS_LANES_RAYS, 2);
                test_one(ta);
                test_one(tb);
            } else {
                RT_PROF_ADD(threadIdx.x & 63, WORK_TRI_STEPS_LANES_RAYS, 1);
                test_one(tri_load_uniform(T + k0));
            }
            mine = mine && !occluded;
            if (__ballot(mine) == 0ull) break;
        }
        return walk_result<ANY>(best_t, best_f, occluded);
    }
    uint32_t k = 0;
    RT_PROF_ADD(threadIdx.x & 63, WORK_LEAVES_LANES_RAYS, 1);
    for (; k + 1u < cnt; k += 2u) {          // two records per step: two independent chains in flight
        TriRec ta, tb;
        tri_load_uniform2(T + k, ta, tb);
        RT_PROF_ADD(threadIdx.x & 63, WORK_TRI_STEPS_LANES_RAYS, 2);
        test_one(ta);
        test_one(tb);
        if (ANY && !COUNT && (k & 6u) == 6u) {
            mine = mine && !occluded;
            if (__ballot(mine) == 0ull) return walk_result<ANY>(best_t, best_f, occluded);
        }
    }
    if (k < cnt) { RT_PROF_ADD(threadIdx.x & 63, WORK_TRI_STEPS_LANES_RAYS, 1); test_one(tri_load_uniform(T + k)); }
    return walk_result<ANY>(best_t, best_f, occluded);
}

template <bool ANY, bool COUNT, bool FLAT, bool STAGED = true>
__device__ __forceinline__ auto walk(const DNode &root, const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                     const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                     const float extent, const WaveStack stk, const int lane, const WalkCtl wc, const LanePlane &pl, bool in_root,
                                     const WalkRay &ray, uint32_t &cnt_box, uint32_t &cnt_ref) {
    uint32_t sig_unused = 0u;
    if constexpr (FLAT) return flat_walk<ANY, COUNT>(root, tris, in_root, wc.seg, wc.skip, pl, ray, cnt_box, cnt_ref);
    else return packet_walk<ANY, COUNT, STAGED>(nodes, tris, chunks, leaf_chunk0, extent, stk, lane, wc, in_root, ray, cnt_box, cnt_ref, sig_unused);
}

// The rays of one (hit, light) unit of a FLAT scene after its triangle cull, lane = sample: for the segment lightStrikes tests (`ray` =
// segment_ray(sample, hit)), the root box test and the walk over the triangles the cull kept.  true = the sample is blocked.
// k_shadow<.., FLAT> runs it for its units, k_shade<.., FOLD> for the hits k_beam left pending, k_deep for every sample of its hits (no cull: an
// empty packet): one body, so they cannot drift apart.
template <bool COUNT>
__device__ __forceinline__ bool flat_unit_occluded(const DNode &root, const TriRec *__restrict__ tris, const SegPacket &seg, const unsigned long long skip,
                                                   const LanePlane &pl, const bool valid, const WalkRay &ray, uint32_t &cnt_box, uint32_t &cnt_ref) {
    return flat_walk<true, COUNT>(root, tris, valid && root_hit(root, ray), seg, skip, pl, ray, cnt_box, cnt_ref);
}

// ======================================================================================================
// SHAFT WALK -- the traversal of a shadow unit (k_shadow_shaft: one (hit, light) pair -- or one 64-sample pass of it -- per wave).
//
// All 64 segments of the unit end at the shaded hit point h and start inside the box S of the unit's light samples: they lie in the
// SHAFT hull(S, h).  A counted hit (0.00001 < t < 0.98) has its computed point inside the inflated chunk box it belongs to
// (rt_scene_image.cpp, build_chunk_bounds) and on its segment up to rounding, so a node whose CONTENT box (padded like the per-ray
// content test) does not meet the shaft cannot contribute to any ray of the unit -- whatever the reference's own box tests say.
// And a node whose OWN box (padded) misses every point a ray of the unit can reach -- the shaft and the FAR cone behind h, the
// rays continue beyond the hit point: boxIntersect has no upper bound -- fails the reference's boxIntersect for every ray of the
// unit by a margin far above the rounding of its float slab test, so no ray enters the subtree.
//
// The shaft test runs with LANE = (CHILD, TEST): the 8 children of an inner node x 8 separating tests (six tangent planes through
// h -- two per axis-aligned projection; the x-z and y-z pairs are the side faces of the pyramid over an axis-aligned light
// rectangle -- plus the near and the far bounding box) take ONE wave step; each lane keeps its test's coefficients in registers for
// the whole unit.  Only the surviving children are tested per ray (lane = ray) with the reference's exact boxIntersect; their
// records are broadcast with v_readlane from the lanes that loaded them (no second memory round trip).  The top of the tree is
// read from LDS (the first RT_LDS_NODES DNodes of the breadth-first array), the rest from global memory.  Leaves found by the
// walk are processed afterwards, chunk bounds again with lane = (chunk, test).
// The candidate set of every ray is unchanged: leaves are still entered only through the per-ray exact tests of the whole
// ancestor chain (BoxTree::intersect, boxTree.cpp:150-173).
// ======================================================================================================
#ifndef RT_SHAFT_TRUNC
#define RT_SHAFT_TRUNC 0.0185f        // the tip of the shaft that holds no counted point (t > 0.9815; 0: keep it)
#endif
struct ShaftLanes {
    float r[8];          // this lane's test (lane & 7): planes 0-5 (ax+, ax-, ay+, ay-, az+, az-, c, 2*margin); 6: near box (lo, hi); 7: far box
    float pad;           // padding of the tested boxes (>= the per-ray slab_pad of every segment of the unit); wave-uniform
    bool node_ok;        // the node-box test is valid: no ray of the unit has a zero / non-finite direction component (0/0 = NaN makes
                         // the reference's min/max chain ACCEPT whatever the geometry says)
};

// lane & 7 = test index.  The tangent lines from h to the rectangle S are computed in the projection the lane's plane belongs to:
// planes 0,1 (x,z), 2,3 (y,z), 4,5 (x,y); a line a*u + b*v + c = 0 through h with S on its non-positive side, given as the plane
// (ax, ay, az, c) with the third coefficient zero and split into positive / negative parts, so that
//      min over the corners of a box = ax+ * lx + ax- * hx + ay+ * ly + ay- * hy + az+ * lz + az- * hz + c      (max: lo <-> hi)
__device__ __forceinline__ ShaftLanes make_shaft_lanes(const int lane, const float hx, const float hy, const float hz, const float slx, const float sly,
                                                       const float slz, const float shx, const float shy, const float shz, const float extent,
                                                       const float trunc = 0.0f) {
    ShaftLanes SL;
    const int tk = lane & 7, proj = tk >> 1;
    const bool q1 = (tk & 1) != 0;
    const float big = fmaxf(fmaxf(fabsf(slx), fabsf(shx)), fmaxf(fabsf(sly), fabsf(shy))) + fmaxf(fabsf(slz), fabsf(shz));
    const float scale = extent + big + (fabsf(hx) + fabsf(hy) + fabsf(hz));
    // per-ray slab_pad = 4e-4 * (|o|_1 + extent) with o inside S
    SL.pad = 4e-4f * ((fmaxf(fabsf(slx), fabsf(shx)) + fmaxf(fabsf(sly), fabsf(shy)) + fmaxf(fabsf(slz), fabsf(shz))) + extent) * 1.001f;
    SL.node_ok = true;
    const float hu = proj == 1 ? hy : hx, hv = proj == 2 ? hy : hz;
    const float u0 = proj == 1 ? sly : slx, u1 = proj == 1 ? shy : shx;
    const float v0 = proj == 2 ? sly : slz, v1 = proj == 2 ? shy : shz;
    const bool ul = hu < u0, ur = hu > u1, vl = hv < v0, vr = hv > v1;
    const bool su0 = !(ul || ur), sv0 = !(vl || vr);
    const float near_u = ul ? u0 : u1, far_u = ul ? u1 : u0, near_v = vl ? v0 : v1, far_v = vl ? v1 : v0;
    // the two tangent corners of the rectangle seen from h (q = 0 / 1)
    const float cu = q1 ? (su0 ? u1 : (sv0 ? near_u : far_u)) : (su0 ? u0 : near_u);
    const float cv = q1 ? (sv0 ? v1 : near_v) : (sv0 ? v0 : (su0 ? near_v : far_v));
    const float mu = 0.5f * (u0 + u1) - hu, mv = 0.5f * (v0 + v1) - hv;        // rectangle centre relative to h
    const float nu = -(cv - hv), nv = cu - hu;
    const float fm = nu * mu + nv * mv;
    const float mag = fabsf(nu) + fabsf(nv);
    // usable: h outside the rectangle and the centre strictly on one side (a degenerate rectangle in line with h has no tangent)
    const bool ok = !(su0 && sv0) && (fabsf(fm) > 1e-5f * mag * scale);
    const float sgn = fm > 0.0f ? -1.0f : 1.0f;
    const float a = ok ? sgn * nu : 0.0f, b = ok ? sgn * nv : 0.0f;
    const float margin = 2e-5f * mag * scale;                                   // >> the rounding of the plane evaluations
    const float c = ok ? -(a * hu + b * hv) - margin : -1.0f;                   // unusable: never separates (value -1, far margin 3e38)
    const float ax = proj == 1 ? 0.0f : a, ay = proj == 0 ? 0.0f : (proj == 1 ? a : b), az = proj == 2 ? 0.0f : b;
    SL.r[0] = fmaxf(ax, 0.0f); SL.r[1] = fminf(ax, 0.0f); SL.r[2] = fmaxf(ay, 0.0f); SL.r[3] = fminf(ay, 0.0f);
    SL.r[4] = fmaxf(az, 0.0f); SL.r[5] = fminf(az, 0.0f); SL.r[6] = c; SL.r[7] = ok ? 2.0f * margin : 3e38f;
    if (tk == 6) {          // near box: AABB of hull(S, h)
        SL.r[0] = fminf(slx, hx); SL.r[1] = fminf(sly, hy); SL.r[2] = fminf(slz, hz);
        SL.r[3] = fmaxf(shx, hx); SL.r[4] = fmaxf(shy, hy); SL.r[5] = fmaxf(shz, hz);
        if (trunc > 0.0f) {
            // ... without its TIP: where h lies beyond S along an axis (h_k < sl_k), a point p of a segment s -> h with p_k < h_k + trunc (sl_k - h_k)
            // has t > 1 - trunc = 0.9815 on that segment -- lightStrikes counts t < 0.98 only.  The box then bounds every COUNTED point (content
            // boxes, chunk bounds, the triangles' vertex boxes); it says nothing about where the rays run, so own boxes are not tested against it
            // (shaft_lane_test: near_box = false).  m: far above the rounding of a computed point o + t d (~1e-7 |o|).
            const float m = 1e-5f * scale;
            SL.r[0] += hx < slx ? fmaxf(trunc * (slx - hx) - m, 0.0f) : 0.0f; SL.r[3] -= hx > shx ? fmaxf(trunc * (hx - shx) - m, 0.0f) : 0.0f;
            SL.r[1] += hy < sly ? fmaxf(trunc * (sly - hy) - m, 0.0f) : 0.0f; SL.r[4] -= hy > shy ? fmaxf(trunc * (hy - shy) - m, 0.0f) : 0.0f;
            SL.r[2] += hz < slz ? fmaxf(trunc * (slz - hz) - m, 0.0f) : 0.0f; SL.r[5] -= hz > shz ? fmaxf(trunc * (hz - shz) - m, 0.0f) : 0.0f;
        }
    }
    if (tk == 7) {          // far box: AABB of the far cone { h + tau * (h - s) : s in S, tau >= 0 }
        SL.r[0] = hx >= shx ? hx : -3e38f; SL.r[1] = hy >= shy ? hy : -3e38f; SL.r[2] = hz >= shz ? hz : -3e38f;
        SL.r[3] = hx <= slx ? hx : 3e38f; SL.r[4] = hy <= sly ? hy : 3e38f; SL.r[5] = hz <= slz ? hz : 3e38f;
    }
    return SL;
}

// this lane's test on a padded box: near = the box is outside the near shaft by this test, far = outside the far cone by this test.
// NaN anywhere compares false = keep.
__device__ __forceinline__ void shaft_lane_test(const ShaftLanes &SL, const int tk, const float lx, const float ly, const float lz, const float hx, const float hy,
                                                const float hz, bool &near_out, bool &far_out, const bool near_box = true) {
    const float mn = __builtin_fmaf(SL.r[0], lx, __builtin_fmaf(SL.r[1], hx, __builtin_fmaf(SL.r[2], ly, __builtin_fmaf(SL.r[3], hy,
                     __builtin_fmaf(SL.r[4], lz, __builtin_fmaf(SL.r[5], hz, SL.r[6]))))));
    const float mx = __builtin_fmaf(SL.r[0], hx, __builtin_fmaf(SL.r[1], lx, __builtin_fmaf(SL.r[2], hy, __builtin_fmaf(SL.r[3], ly,
                     __builtin_fmaf(SL.r[4], hz, __builtin_fmaf(SL.r[5], lz, SL.r[6]))))));
    const bool box_out = (lx > SL.r[3]) || (hx < SL.r[0]) || (ly > SL.r[4]) || (hy < SL.r[1]) || (lz > SL.r[5]) || (hz < SL.r[2]);
    near_out = tk < 6 ? (mn > 0.0f) : (tk == 6 && near_box && box_out);
    far_out = tk < 6 ? (mx + SL.r[7] < 0.0f) : (tk == 7 && box_out);
}
// byte j of a 64-bit ballot, for lane j < 8: does any of the 8 tests of child / chunk j say "outside"?
__device__ __forceinline__ bool ballot_byte_any(const unsigned long long b, const int lane) {
    return ((b >> ((lane & 7) * 8)) & 0xffull) != 0ull;
}

// The lanes' coefficients are parked in LDS between uses (8 records of 8 floats per wave, written by lanes 0-7 once per unit): they are
// needed once per group and once per 8 chunk bounds, and eight registers held across the whole walk were eight registers spilled.
struct ShaftCtl { float pad; bool node_ok; };
__device__ __forceinline__ void shaft_lanes_store(float4 *lds, const int lane, const ShaftLanes &SL) {
    if (lane < 8) { lds[2 * lane] = make_float4(SL.r[0], SL.r[1], SL.r[2], SL.r[3]); lds[2 * lane + 1] = make_float4(SL.r[4], SL.r[5], SL.r[6], SL.r[7]); }
}
__device__ __forceinline__ ShaftLanes shaft_lanes_load(const float4 *lds, const int tk, const ShaftCtl &SC) {
    const float4 a = lds[2 * tk], b = lds[2 * tk + 1];
    ShaftLanes SL;
    SL.r[0] = a.x; SL.r[1] = a.y; SL.r[2] = a.z; SL.r[3] = a.w; SL.r[4] = b.x; SL.r[5] = b.y; SL.r[6] = b.z; SL.r[7] = b.w;
    SL.pad = SC.pad; SL.node_ok = SC.node_ok;
    return SL;
}

// ---- lane = triangle: one 64-triangle chunk against the unit's shaft --------------------------------------------------------------
// A counted hit of triangle T (0.00001 < t < 0.98 and the barycentric test of rayTriangleIntersection passed IN FLOAT) has its computed
// point within ChunkBound::infl (per axis) of T itself (rt_scene_image.cpp: build_chunk_bounds -- the chunk box is the union of exactly these
// neighbourhoods), and that point lies on its segment up to rounding, i.e. inside hull(S, h).  So T cannot be hit by ANY ray of the unit
// when the three boxes [v - m, v + m] around its vertices (m = 1.0625 * infl: B and C are re-derived as A + edge, one rounding each)
// lie strictly outside one of the shaft's tangent planes (their convex hull contains T's neighbourhood) or outside the near box; the
// planes carry the same margins as in the node / chunk tests.  Independently, plane_rules_out (round 1, flat scenes) proves from the
// reference's own two dot products that t <= 0 or |t| >= 0.98 for every sample of S: this is what removes the face h lies on and its
// coplanar neighbours, which no geometric test can separate from h.
// The unit's planes are kept as a per-wave LDS record (written once per unit by the lanes that own them) so that the test costs no
// register for the rest of the walk: 11 broadcast ds_read_b128.
#define RT_SHAFT_TRI_REC 11           // float4 per wave: 6 planes (a_u, a_v, c, |a_u| + |a_v|), near box lo / hi, (h, m0), S lo, S hi
__device__ __forceinline__ void shaft_tri_store(float4 *rec, const int lane, const ShaftLanes &SL, const float hx, const float hy, const float hz,
                                                const float slx, const float sly, const float slz, const float shx, const float shy, const float shz) {
    const int proj = (lane & 7) >> 1;
    const float ax = SL.r[0] + SL.r[1], ay = SL.r[2] + SL.r[3], az = SL.r[4] + SL.r[5];        // (one addend is zero: exact)
    const float au = proj == 1 ? ay : ax, av = proj == 2 ? ay : az;
    if (lane < 6) rec[lane] = make_float4(au, av, SL.r[6], fabsf(au) + fabsf(av));
    if (lane == 6) { rec[6] = make_float4(SL.r[0], SL.r[1], SL.r[2], 0.f); rec[7] = make_float4(SL.r[3], SL.r[4], SL.r[5], 0.f); }
    if (lane == 7) {
        const float m0 = 2e-5f * ((fabsf(slx) + fabsf(shx)) + (fabsf(sly) + fabsf(shy)) + (fabsf(slz) + fabsf(shz)) + (fabsf(hx) + fabsf(hy) + fabsf(hz)));
        rec[8] = make_float4(hx, hy, hz, m0); rec[9] = make_float4(slx, sly, slz, 0.f); rec[10] = make_float4(shx, shy, shz, 0.f);
    }
}
__device__ __forceinline__ bool tri_outside_shaft(const float4 *rec, const TriRec &tr, const float m) {
    const float bx = tr.ax + tr.e1x, by = tr.ay + tr.e1y, bz = tr.az + tr.e1z;
    const float cx = tr.ax + tr.e0x, cy = tr.ay + tr.e0y, cz = tr.az + tr.e0z;
    bool out = false;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const float4 pl = rec[p];
        const int proj = p >> 1;
        const float ua = proj == 1 ? tr.ay : tr.ax, ub = proj == 1 ? by : bx, uc = proj == 1 ? cy : cx;
        const float va = proj == 2 ? tr.ay : tr.az, vb = proj == 2 ? by : bz, vc = proj == 2 ? cy : cz;
        const float fa = __builtin_fmaf(pl.x, ua, pl.y * va), fb = __builtin_fmaf(pl.x, ub, pl.y * vb), fc = __builtin_fmaf(pl.x, uc, pl.y * vc);
        out = out || (fminf(fminf(fa, fb), fc) + (pl.z - m * pl.w) > 0.0f);
    }
    const float4 lo = rec[6], hi = rec[7];
    out = out || (fminf(fminf(tr.ax, bx), cx) - m > hi.x) || (fmaxf(fmaxf(tr.ax, bx), cx) + m < lo.x)
              || (fminf(fminf(tr.ay, by), cy) - m > hi.y) || (fmaxf(fmaxf(tr.ay, by), cy) + m < lo.y)
              || (fminf(fminf(tr.az, bz), cz) - m > hi.z) || (fmaxf(fmaxf(tr.az, bz), cz) + m < lo.z);
    const float4 h = rec[8], s0 = rec[9], s1 = rec[10];
    const SegPacket g{true, false, h.x, h.y, h.z, s0.x, s0.y, s0.z, s1.x, s1.y, s1.z, h.w};
    return out || plane_rules_out(g, tr.nx, tr.ny, tr.nz, tr.nA);
}

// The same test for a packet whose rays share their ORIGIN o (a primary tile: the camera centre; light-centre segments: the light) and
// run through targets inside a box: every point a ray can reach (any t >= 0) lies in the cone from o through that box, all of it on the
// non-positive side of the six tangent planes through o -- so a triangle whose vertex boxes are strictly outside one plane is missed by
// every ray, whatever t.  The near box (AABB of hull(o, targets)) only bounds hits BEFORE the targets: use_box is set for the
// light-centre segments (counted hits have t < 0.98) and not for closest-hit rays.  The record is the one shaft_tri_store writes with
// h := o and S := the target box.
__device__ __forceinline__ bool tri_outside_cone(const float4 *rec, const TriRec &tr, const float m, const bool use_box) {
    const float bx = tr.ax + tr.e1x, by = tr.ay + tr.e1y, bz = tr.az + tr.e1z;
    const float cx = tr.ax + tr.e0x, cy = tr.ay + tr.e0y, cz = tr.az + tr.e0z;
    bool out = false;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const float4 pl = rec[p];
        const int proj = p >> 1;
        const float ua = proj == 1 ? tr.ay : tr.ax, ub = proj == 1 ? by : bx, uc = proj == 1 ? cy : cx;
        const float va = proj == 2 ? tr.ay : tr.az, vb = proj == 2 ? by : bz, vc = proj == 2 ? cy : cz;
        const float fa = __builtin_fmaf(pl.x, ua, pl.y * va), fb = __builtin_fmaf(pl.x, ub, pl.y * vb), fc = __builtin_fmaf(pl.x, uc, pl.y * vc);
        out = out || (fminf(fminf(fa, fb), fc) + (pl.z - m * pl.w) > 0.0f);
    }
    if (use_box) {
        const float4 lo = rec[6], hi = rec[7];
        out = out || (fminf(fminf(tr.ax, bx), cx) - m > hi.x) || (fmaxf(fmaxf(tr.ax, bx), cx) + m < lo.x)
                  || (fminf(fminf(tr.ay, by), cy) - m > hi.y) || (fmaxf(fmaxf(tr.ay, by), cy) + m < lo.y)
                  || (fminf(fminf(tr.az, bz), cz) - m > hi.z) || (fmaxf(fmaxf(tr.az, bz), cz) + m < lo.z);
    }
    return out;
}

#define RT_LEAF_SLOTS 16
#define RT_COST_TRI_STEP 58u

struct ShaftLds {
    const DNode *nodes;            // LDS copy of the first n_lds nodes (the top of the breadth-first array)
    uint32_t n_lds;
    uint32_t *lnode;               // per-wave leaf list (RT_LEAF_SLOTS)
    unsigned long long *lmask;
    float4 *tri;                   // per-wave shaft record of the lane = triangle test (RT_SHAFT_TRI_REC)
    float4 *shaft;                 // per-wave copy of the lanes' coefficients (16 float4: ShaftLanes::r of test tk at [2 tk], [2 tk + 1])
};

// One leaf of the shaft walk.  Chunk bounds are shaft-tested 8 at a time (lane = (chunk, test)); what survives goes through the per-ray
// chunk test (lane = ray) and the triangle tests (lane = triangle).
// where a shaft walk hands big leaves to (the leaf-task queue of the k_shadow<.., CONT> launch that follows): budget 0 = never
struct ShaftTasks {
    ContTask *tasks;
    uint32_t *count;
    uint32_t cap, budget, target, unit;
};

template <bool TASKS>
__device__ __forceinline__ void shaft_leaf(const uint32_t ni, const uint32_t first, const uint32_t cnt, const uint32_t chunk0, const TriRec *__restrict__ tris,
                                           const ChunkBound *__restrict__ chunks, const int lane, const RayLane &R, const ShaftCtl &SC, const ShaftTasks &TQ,
                                           const ShaftLds &sl, const uint32_t c_begin, const uint32_t c_end, unsigned long long live, bool &occluded) {
    const float4 *__restrict__ srec = sl.tri;
    const float ox = R.ox, oy = R.oy, oz = R.oz, dx = R.dx, dy = R.dy, dz = R.dz;
    const TriRec *__restrict__ T = tris + first;
    bool mine = ((live >> lane) & 1ull) != 0ull;
    auto test_lane = [&](const TriRec &tr) {
        // Flyscene::rayTriangleIntersection, flyscene.cpp:787-819 (lanes = rays)
        const float dn = dot3(dx, dy, dz, tr.nx, tr.ny, tr.nz);
        const float t = (tr.nA - dot3(ox, oy, oz, tr.nx, tr.ny, tr.nz)) / dn;
        const float v2x = (ox + t * dx) - tr.ax, v2y = (oy + t * dy) - tr.ay, v2z = (oz + t * dz) - tr.az;
        const float d02 = dot3(tr.e0x, tr.e0y, tr.e0z, v2x, v2y, v2z);
        const float d12 = dot3(tr.e1x, tr.e1y, tr.e1z, v2x, v2y, v2z);
        const float u = (tr.d11 * d02 - tr.d01 * d12) * tr.inv_denom;
        const float v = (tr.d00 * d12 - tr.d01 * d02) * tr.inv_denom;
        const bool ok = mine && !(tr.flags & 1u) && (dn != 0) && (u >= 0) && (v >= 0) && (u + v < 1) && (t > 0.00001f);
        occluded = occluded || (ok && t < 0.98f);
    };
    if (c_begin == 0u && cnt <= RT_SCALAR_LEAF_MAX && static_cast<uint32_t>(__popcll(live)) * RT_COST_TRI_STEP > cnt * RT_COST_RAY_MODE) {
        // small leaf, many rays: every lane steps through the wave-uniform records (scalar loads)
        uint32_t k = 0;
        for (; k + 1u < cnt; k += 2u) {
            TriRec ta, tb;
            tri_load_uniform2(T + k, ta, tb);
            test_lane(ta);
            test_lane(tb);
        }
        if (k < cnt) test_lane(tri_load_uniform(T + k));
        return;
    }
    const uint32_t nchunk_all = (cnt + 63u) >> 6;
    const uint32_t nchunk = c_end < nchunk_all ? c_end : nchunk_all;                  // chunks [c_begin, nchunk) are processed here
    const ChunkBound *__restrict__ cbounds = chunks + chunk0;
    const int tk = lane & 7, tc = lane >> 3;
    unsigned long long occ_new = 0ull;
    uint32_t c_first = c_begin;
    // A big leaf with many live rays is not ground through by this wave (one unit crossing a 979-triangle leaf with 64 rays is ~60k
    // instructions: the tail of the whole launch): it becomes chunk-range tasks for the leaf-task launch, which merges its occluded
    // bits into `vis` with atomicAnd.  Estimate as leaf_visit: a third of the chunks survive the per-ray test.
    if (TASKS && TQ.budget != 0u) {
        const uint32_t est = nchunk * RT_COST_CHUNK_TEST + static_cast<uint32_t>(__popcll(live)) * ((nchunk + 2u) / 3u) * RT_COST_TRI_STEP;
        if (est > TQ.budget) {
            uint32_t ntask = (est + TQ.target - 1u) / TQ.target;
            if (ntask > nchunk) ntask = nchunk;
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(TQ.count, ntask);
            base = uniform_u32(base);
            // the counter only grows (the consumer clamps it): pieces past the end of the queue are processed here
            const uint32_t fit = base >= TQ.cap ? 0u : (ntask < TQ.cap - base ? ntask : TQ.cap - base);
            for (uint32_t i = static_cast<uint32_t>(lane); i < fit; i += 64u) {
                ContTask t;
                t.unit = TQ.unit; t.node = ni; t.mask = live;
                t.c_begin = static_cast<uint32_t>(static_cast<unsigned long long>(nchunk) * i / ntask);
                t.c_end = static_cast<uint32_t>(static_cast<unsigned long long>(nchunk) * (i + 1u) / ntask);
                t.pad0 = t.pad1 = 0u;
                TQ.tasks[base + i] = t;
            }
            if (fit == ntask) return;
            c_first = static_cast<uint32_t>(static_cast<unsigned long long>(nchunk) * fit / ntask);     // (queue full) the rest of the leaf, inline
        }
    }
    for (uint32_t cb0 = c_first & ~7u; cb0 < nchunk && live != 0ull; cb0 += 8u) {
        const uint32_t myc = cb0 + static_cast<uint32_t>(tc);
        const ChunkBound bd = cbounds[myc < nchunk ? myc : cb0];
        bool near_out, far_out;
        __builtin_amdgcn_wave_barrier();
        const ShaftLanes SL = shaft_lanes_load(sl.shaft, tk, SC);
        shaft_lane_test(SL, tk, bd.lo[0] - SL.pad, bd.lo[1] - SL.pad, bd.lo[2] - SL.pad, bd.hi[0] + SL.pad, bd.hi[1] + SL.pad, bd.hi[2] + SL.pad, near_out, far_out);
        const unsigned long long b_out = __ballot(near_out && bd.never < 1.5f);
        const uint32_t nhere = nchunk - cb0 < 8u ? nchunk - cb0 : 8u;
        unsigned long long cm = __ballot(static_cast<uint32_t>(lane) < nhere && cb0 + static_cast<uint32_t>(lane) >= c_first && !ballot_byte_any(b_out, lane));      // bit j: chunk cb0 + j survives
        RT_PROF_ADD(lane, WORK_LEAF_CHUNK_BATCHES, 1); RT_PROF_ADD(lane, WORK_LEAF_CHUNKS_IN_BATCHES, nhere); RT_PROF_ADD(lane, WORK_CHUNKS_TESTED_PER_RAY, __popcll(cm));
        // next chunk of `cm` that some live ray cannot skip (per-ray conservative test, lanes = rays), or -1
        auto find_next = [&](unsigned long long &todo_out) -> int {
            while (cm != 0ull) {
                const int j = static_cast<int>(__builtin_ctzll(cm));
                cm &= cm - 1ull;
                unsigned long long todo = live;
                if (lane_f(bd.never, 8 * j) < 1.5f) {
                    const float l0 = lane_f(bd.lo[0], 8 * j), l1 = lane_f(bd.lo[1], 8 * j), l2 = lane_f(bd.lo[2], 8 * j);
                    const float h0 = lane_f(bd.hi[0], 8 * j), h1 = lane_f(bd.hi[1], 8 * j), h2 = lane_f(bd.hi[2], 8 * j);
                    const float t0x = (l0 - R.slab_pad - ox) * R.idx, t1x = (h0 + R.slab_pad - ox) * R.idx;
                    const float t0y = (l1 - R.slab_pad - oy) * R.idy, t1y = (h1 + R.slab_pad - oy) * R.idy;
                    const float t0z = (l2 - R.slab_pad - oz) * R.idz, t1z = (h2 + R.slab_pad - oz) * R.idz;
                    const float tin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
                    const float tout = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
                    bool miss = (tin > tout) || (tout < -1e-3f) || (tin > 0.981f);
#ifndef RT_NO_SLAB
                    // ... and the chunk's slab (ChunkBound::sn): f(t) = sn . (o + t d) over the part of the line inside the box and the counted range;
                    // a counted point has f in [slo, shi].  m: far above the rounding of the two dot products (~4e-7 (|o| + |d|) |sn|_1)
                    const float n0 = lane_f(bd.sn[0], 8 * j), n1 = lane_f(bd.sn[1], 8 * j), n2 = lane_f(bd.sn[2], 8 * j);
                    const float fa = __builtin_fmaf(n0, ox, __builtin_fmaf(n1, oy, n2 * oz)), fb = __builtin_fmaf(n0, dx, __builtin_fmaf(n1, dy, n2 * dz));
                    const float f0 = __builtin_fmaf(fmaxf(tin, -1e-3f), fb, fa), f1 = __builtin_fmaf(fminf(tout, 0.981f), fb, fa);
                    const float m = 0.04f * R.slab_pad;
                    miss = miss || (fmaxf(f0, f1) + m < lane_f(bd.slo, 8 * j)) || (fminf(f0, f1) - m > lane_f(bd.shi, 8 * j));
#endif
                    todo = live & ~__ballot(miss);
                }
                if (todo != 0ull) { RT_PROF_ADD(lane, WORK_CHUNKS_WITH_WORK, 1); todo_out = todo; return j; }
            }
            return -1;
        };
        auto load_chunk = [&](const int j) -> TriRec {
            const uint32_t k = (cb0 + static_cast<uint32_t>(j)) * 64u + static_cast<uint32_t>(lane);
            return T[k < cnt ? k : 0u];
        };
        unsigned long long todo_cur = 0ull, todo_nxt = 0ull;
        int cur = find_next(todo_cur);
        if (cur < 0) continue;
        TriRec tr = load_chunk(cur);
        while (cur >= 0) {
            const uint32_t c0 = (cb0 + static_cast<uint32_t>(cur)) * 64u;
            const uint32_t n = cnt - c0 < 64u ? cnt - c0 : 64u;
            bool hast = static_cast<uint32_t>(lane) < n && !(tr.flags & 1u);
            unsigned long long todo = todo_cur & live;
            const uint32_t m_rays = static_cast<uint32_t>(__popcll(todo));
            unsigned long long tmask = ~0ull;
            // (a chunk that is never culled as a whole still carries the inflation of its well-conditioned triangles -- 0: it has none --; the
            //  ill-conditioned ones, TriRec::flags bit 1, are kept whatever the test says: dodge's collinear slivers sit one or two to a chunk and
            //  used to cost 64 rays x 64 triangles wherever a unit entered their leaf)
            if (m_rays >= RT_TRI_SHAFT_MIN && (lane_f(bd.never, 8 * cur) < 1.5f || lane_f(bd.infl, 8 * cur) > 0.0f)) {
                // lane = triangle: which triangles of the chunk can be hit by ANY ray of the unit
                __builtin_amdgcn_wave_barrier();
                hast = hast && ((tr.flags & 2u) != 0u || !tri_outside_shaft(srec, tr, lane_f(bd.infl, 8 * cur) * 1.0625f));
                tmask = __ballot(hast);
                RT_PROF_ADD(lane, WORK_TRI_SHAFT_TESTS, 1); RT_PROF_ADD(lane, WORK_TRI_SHAFT_SURVIVORS, __popcll(tmask)); RT_PROF_ADD(lane, WORK_TRI_SHAFT_RAYS, m_rays); RT_PROF_ADD(lane, WORK_TRI_SHAFT_EMPTY_CHUNKS, tmask == 0ull ? 1 : 0);
            }
            if (tmask == 0ull) {
                todo = 0ull;
            } else if (tmask != ~0ull && static_cast<uint32_t>(__popcll(tmask)) * (RT_COST_RAY_MODE + RT_RAYMODE_EXTRA) < m_rays * RT_COST_TRI_STEP) {
                // few triangles left, many rays: lanes = rays step through the survivors (wave-uniform records, scalar loads)
                const bool my = ((todo >> lane) & 1ull) != 0ull;
                bool occ_r = false;
                const TriRec *__restrict__ Tc = T + c0;
                auto hit_lane = [&](const TriRec &ta) -> bool {
                    // Flyscene::rayTriangleIntersection, flyscene.cpp:787-819 (lanes = rays)
                    const float dn = dot3(dx, dy, dz, ta.nx, ta.ny, ta.nz);
                    const float t = (ta.nA - dot3(ox, oy, oz, ta.nx, ta.ny, ta.nz)) / dn;
                    const float v2x = (ox + t * dx) - ta.ax, v2y = (oy + t * dy) - ta.ay, v2z = (oz + t * dz) - ta.az;
                    const float d02 = dot3(ta.e0x, ta.e0y, ta.e0z, v2x, v2y, v2z);
                    const float d12 = dot3(ta.e1x, ta.e1y, ta.e1z, v2x, v2y, v2z);
                    const float u = (ta.d11 * d02 - ta.d01 * d12) * ta.inv_denom;
                    const float v = (ta.d00 * d12 - ta.d01 * d02) * ta.inv_denom;
                    return my && (dn != 0) && (u >= 0) && (v >= 0) && (u + v < 1) && (t > 0.00001f) && (t < 0.98f);
                };
                while (tmask != 0ull) {
                    const uint32_t j0 = static_cast<uint32_t>(__builtin_ctzll(tmask));
                    tmask &= tmask - 1ull;
                    const bool two = tmask != 0ull;
                    const uint32_t j1 = two ? static_cast<uint32_t>(__builtin_ctzll(tmask)) : j0;
                    if (two) tmask &= tmask - 1ull;
                    RT_PROF_ADD(lane, WORK_TRI_STEPS_LANES_RAYS, two ? 2 : 1);
                    TriRec ta, tb;
                    tri_load_uniform_pair(Tc + j0, Tc + j1, ta, tb);
                    const bool ha = hit_lane(ta), hb = hit_lane(tb);
                    occ_r = occ_r || ha || hb;
                    if (__ballot(my && !occ_r) == 0ull) break;
                }
                const unsigned long long ob = __ballot(occ_r);
                occ_new |= ob; live &= ~ob;
                todo = 0ull;
            }
            while (todo != 0ull) {
                const int r0 = static_cast<int>(__builtin_ctzll(todo));
                todo &= todo - 1ull;
                const bool two = todo != 0ull;
                const int r1 = two ? static_cast<int>(__builtin_ctzll(todo)) : r0;
                if (two) todo &= todo - 1ull;
                float tq[2]; bool inq[2];
                RT_PROF_ADD(lane, WORK_TRI_STEPS_LANES_TRIANGLES, two ? 2 : 1);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    // Flyscene::rayTriangleIntersection, flyscene.cpp:787-819 (lanes = triangles, the ray broadcast)
                    const int r = q == 0 ? r0 : r1;
                    const float rdx = lane_f(dx, r), rdy = lane_f(dy, r), rdz = lane_f(dz, r);
                    const float rox = lane_f(ox, r), roy = lane_f(oy, r), roz = lane_f(oz, r);
                    const float dn = dot3(rdx, rdy, rdz, tr.nx, tr.ny, tr.nz);
                    const float t = (tr.nA - dot3(rox, roy, roz, tr.nx, tr.ny, tr.nz)) / dn;
                    const float v2x = (rox + t * rdx) - tr.ax, v2y = (roy + t * rdy) - tr.ay, v2z = (roz + t * rdz) - tr.az;
                    const float d02 = dot3(tr.e0x, tr.e0y, tr.e0z, v2x, v2y, v2z);
                    const float d12 = dot3(tr.e1x, tr.e1y, tr.e1z, v2x, v2y, v2z);
                    const float u = (tr.d11 * d02 - tr.d01 * d12) * tr.inv_denom;
                    const float v = (tr.d00 * d12 - tr.d01 * d02) * tr.inv_denom;
                    tq[q] = t;
                    inq[q] = hast && (dn != 0) && (u >= 0) && (v >= 0) && (u + v < 1) && (t > 0.00001f);
                }
                if (!two) inq[1] = false;
                if (__ballot(inq[0] && tq[0] < 0.98f) != 0ull) { occ_new |= 1ull << r0; live &= ~(1ull << r0); }
                if (__ballot(inq[1] && tq[1] < 0.98f) != 0ull) { occ_new |= 1ull << r1; live &= ~(1ull << r1); }
            }
            if (live == 0ull) break;
            // (the next chunk's records used to be requested before this one was worked on: twenty registers for one hidden round trip.
            // Without them the kernel fits 80 registers -- six waves per SIMD cover the latency better: cfg4 -6 %, dodge -3 %)
            cur = find_next(todo_nxt); todo_cur = todo_nxt;
            if (cur >= 0) tr = load_chunk(cur);
        }
    }
    occluded = occluded || (((occ_new >> lane) & 1ull) != 0ull);
}


__device__ __forceinline__ DNode node_from_lane(const DNode &mine, const int j) {
    DNode o;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o.bmin[k] = lane_f(mine.bmin[k], j); o.bmax[k] = lane_f(mine.bmax[k], j);
        o.clo[k] = lane_f(mine.clo[k], j); o.chi[k] = lane_f(mine.chi[k], j);
    }
    o.first = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(mine.first), j));
    o.count_flags = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(mine.count_flags), j));
    o.pad[0] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(mine.pad[0]), j));
    o.pad[1] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(mine.pad[1]), j));
    return o;
}

template <bool TASKS>
__device__ __forceinline__ void shaft_walk(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris, const ChunkBound *__restrict__ chunks,
                                           const WaveStack stk, const ShaftLds sl, const int lane, const DNode &root, const bool in_root,
                                           const RayLane &R, const ShaftCtl &SC, const ShaftTasks &TQ, bool &occluded) {
    const float ox = R.ox, oy = R.oy, oz = R.oz;
    const unsigned long long m0 = __ballot(in_root);
    if (m0 == 0ull) return;
    const int tk = lane & 7, tc = lane >> 3;
    int sp = 0, nleaf = 0;
    if (root.count_flags & RT_NODE_LEAF) {
        if (lane == 0) { sl.lnode[0] = 0u; sl.lmask[0] = m0; }
        nleaf = 1;
    } else {
        // stack entry = one GROUP: the children [first, first + cnt) of an inner node whose box the rays in `mask` hit
        if (lane == 0) { stk.node[0] = root.first | ((root.count_flags & 0xfu) << 28); stk.mask[0] = m0; }
        sp = 1;
    }
    while (sp > 0 || nleaf > 0) {
        if (sp == 0 || nleaf > RT_LEAF_SLOTS - 8) {
            // the leaves found so far (ONE inlined copy of the leaf code: all of them are processed here)
            for (int k = 0; k < nleaf; ++k) {
                __builtin_amdgcn_wave_barrier();
                const uint32_t li = uniform_u32(sl.lnode[k]);
                unsigned long long lm = uniform_u64(sl.lmask[k]);
                lm &= ~__ballot(occluded);
                if (lm == 0ull) continue;
                uint32_t lf, lc, l0;
                if (li < sl.n_lds) { lf = sl.nodes[li].first; lc = sl.nodes[li].count_flags; l0 = sl.nodes[li].pad[0]; }
                else { lf = nodes[li].first; lc = nodes[li].count_flags; l0 = nodes[li].pad[0]; }
                shaft_leaf<TASKS>(li, uniform_u32(lf), uniform_u32(lc) & 0x7fffffffu, uniform_u32(l0), tris, chunks, lane, R, SC, TQ, sl, 0u, 0xffffffffu, lm, occluded);
            }
            nleaf = 0;
            continue;
        }
        --sp;
        __builtin_amdgcn_wave_barrier();
        const uint32_t ent = uniform_u32(stk.node[sp]);
        unsigned long long gm = uniform_u64(stk.mask[sp]);
        gm &= ~__ballot(occluded);
        if (gm == 0ull) continue;
        const uint32_t base = ent & 0x0fffffffu, gcnt = ent >> 28;
        // lane = (child tc, test tk): the child's record, then this lane's separating test on its content box and on its own box
        const uint32_t ci = base + (static_cast<uint32_t>(tc) < gcnt ? static_cast<uint32_t>(tc) : 0u);
        DNode ch;
        const bool resident = base + gcnt <= sl.n_lds;
        if (resident) ch = sl.nodes[ci];
        else ch = nodes[ci];
        bool c_near, c_far, n_near, n_far;
        const ShaftLanes SL = shaft_lanes_load(sl.shaft, tk, SC);
        shaft_lane_test(SL, tk, ch.clo[0] - SL.pad, ch.clo[1] - SL.pad, ch.clo[2] - SL.pad, ch.chi[0] + SL.pad, ch.chi[1] + SL.pad, ch.chi[2] + SL.pad, c_near, c_far);
        shaft_lane_test(SL, tk, ch.bmin[0] - SL.pad, ch.bmin[1] - SL.pad, ch.bmin[2] - SL.pad, ch.bmax[0] + SL.pad, ch.bmax[1] + SL.pad, ch.bmax[2] + SL.pad, n_near, n_far, false);
        const unsigned long long b_c = __ballot(c_near && ch.pad[1] == 0u), b_nn = __ballot(n_near), b_nf = __ballot(n_far);
        const bool culled = (SL.node_ok && ballot_byte_any(b_nn, lane) && ballot_byte_any(b_nf, lane)) || ballot_byte_any(b_c, lane);
        unsigned long long surv = __ballot(static_cast<uint32_t>(lane) < gcnt && !culled);       // bit j: child j survives
        RT_PROF_ADD(lane, WORK_SHAFT_GROUPS, 1); RT_PROF_ADD(lane, WORK_SHAFT_GROUP_CHILDREN, gcnt); RT_PROF_ADD(lane, WORK_NODES_TESTED_PER_RAY, __popcll(surv));
        while (surv != 0ull) {
            const int j = static_cast<int>(__builtin_ctzll(surv));
            surv &= surv - 1ull;
            // the survivor's record as wave-uniform values: an LDS broadcast read where the group sits in the LDS copy of the top of the
            // tree (4 ds_read_b128), else 16 v_readlane from the lane that loaded it (cfg4: -2.5 % on k_shadow_shaft).  Measured and
            // rejected here: skipping the per-ray content test on inner nodes (+8 % on cfg4), prefetching the next unit's item with a
            // scalar load (+4 %: 16 more live SGPRs -> spills) or through one VGPR with the queue looking one unit ahead (+6 %: the
            // other waves of the SIMD already cover that latency), the records of non-resident groups through an LDS slot instead of
            // v_readlane (+1.5 % on cfg4), 2x / 4x / 8x larger k_stage grids (0 %), two survivors per step as independent chains (round 3:
            // +3 % dodge, +7 % cfg4 -- the second record's registers are spilled), the survivors in descending order (0.0 %: the any-hit walk
            // does not care which child comes first).
            const DNode nd = resident ? sl.nodes[base + static_cast<uint32_t>(j)] : node_from_lane(ch, 8 * j);
            bool h = ((gm >> lane) & 1ull) != 0ull && !occluded;
            RT_PROF_ADD(lane, WORK_NODE_TEST_LIVE_RAYS, __popcll(__ballot(h)));
            if (nd.pad[1] == 0u) {   // per-ray content test (as packet_walk): no countable point of the segment inside the subtree's content box
                const float t0x = (nd.clo[0] - R.slab_pad - ox) * R.idx, t1x = (nd.chi[0] + R.slab_pad - ox) * R.idx;
                const float t0y = (nd.clo[1] - R.slab_pad - oy) * R.idy, t1y = (nd.chi[1] + R.slab_pad - oy) * R.idy;
                const float t0z = (nd.clo[2] - R.slab_pad - oz) * R.idz, t1z = (nd.chi[2] + R.slab_pad - oz) * R.idz;
                const float tin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
                const float tout = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
                const bool miss = (tin > tout) || (tout < -1e-3f) || (tin > 0.981f);
                h = h && !miss;
                if (__ballot(h) == 0ull) continue;
            }
            // (R comes from a segment_ray: its box-test direction IS its triangle-test direction, so R.d and R.id belong together here)
            h = h && box_hit_verified(nd.bmin, ox, oy, oz, R.dx, R.dy, R.dz, R.idx, R.idy, R.idz);     // BoundingBox::boxIntersect, exact
            const unsigned long long hm = __ballot(h);
            if (hm == 0ull) continue;
            RT_PROF_ADD(lane, WORK_NODES_HIT, 1); RT_PROF_ADD(lane, WORK_NODE_HIT_RAYS, __popcll(hm));
            const uint32_t cj = base + static_cast<uint32_t>(j);
            if (nd.count_flags & RT_NODE_LEAF) {
                if ((nd.count_flags & 0x7fffffffu) == 0u) continue;
                // (a group adds at most 8 leaves and the list is emptied when it reaches RT_LEAF_SLOTS - 8 entries before the next group)
                if (lane == 0) { sl.lnode[nleaf] = cj; sl.lmask[nleaf] = hm; }
                ++nleaf;
            } else {
                if ((nd.count_flags & 0xfu) == 0u) continue;              // a "lost" node: no children
                if (lane == 0) { stk.node[sp] = nd.first | ((nd.count_flags & 0xfu) << 28); stk.mask[sp] = hm; }
                ++sp;
            }
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
// one wave's count into counter `st` of the block's shard of Control::stat (the caller keeps its lane-0 condition and its `if (count)`)
__device__ __forceinline__ void stat_add(Control *ctl, const int st, const uint32_t count) {
    atomicAdd(&ctl->stat[blockIdx.x & (RT_STAT_SHARDS - 1)][st], static_cast<unsigned long long>(count));
}

// ---- sharded compaction lists (rt_device.hpp, RT_LIST_SHARDS) ----
// Lane s (< RT_LIST_SHARDS) of a ShardMap holds shard s: its element count and where its work units start in the dense
// numbering [0, total) of the consumer's work (tiles of 64 elements, or shadow units).
struct ShardMap {
    uint32_t start, next, cnt;   // per lane
    uint32_t total;              // uniform
};
__device__ __forceinline__ ShardMap shard_map(const uint32_t *counters, const int lane, const uint32_t cap, const uint32_t mult, const uint32_t gran) {
    uint32_t c = lane < RT_LIST_SHARDS ? counters[lane * 16] : 0u;
    if (c > cap) c = cap;
    const uint32_t w = static_cast<uint32_t>((static_cast<unsigned long long>(c) * mult + gran - 1u) / gran);
    uint32_t incl = w;
    for (int d = 1; d < RT_LIST_SHARDS; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    ShardMap m;
    m.cnt = c;
    m.start = incl - w;
    m.next = lane < RT_LIST_SHARDS ? incl : 0xffffffffu;
    m.total = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), RT_LIST_SHARDS - 1));
    return m;
}
// dense work number w (wave-uniform, < total) -> shard, work number inside the shard, the shard's element count
__device__ __forceinline__ void shard_find(const ShardMap &m, const uint32_t w, uint32_t &shard, uint32_t &local, uint32_t &cnt) {
    shard = static_cast<uint32_t>(__popcll(__ballot(m.next <= w)));
    if (shard >= RT_LIST_SHARDS) shard = RT_LIST_SHARDS - 1;     // never taken for w < total
    local = w - static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(m.start), static_cast<int>(shard)));
    cnt = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(m.cnt), static_cast<int>(shard)));
}
// one returning atomic per wave on the counter of the list shard picked by the producing tile / group number
__device__ __forceinline__ uint32_t shard_reserve(uint32_t *counters, uint32_t *overflow, const uint32_t producer, const uint32_t n, const uint32_t cap,
                                                  const int lane, bool &fits) {
    const uint32_t sh = producer & (RT_LIST_SHARDS - 1u);
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&counters[sh * 16u], n);
    base = uniform_u32(base);
    fits = base + n <= cap;       // always true: the capacity is derived from the tile count (rt_capi.cpp, list_cap)
    if (!fits && lane == 0) atomicOr(overflow, 1u);      // ... and if it ever is not, the frame is reported as failed, not silently short
    return sh * cap + base;
}

// adaptive pass 2 (DFrame::tiles): dense primary tile number k -> the k-th entry of k_flag's list: the tile and its lane mask
__device__ __forceinline__ void flag_tile(const DFrame &F, const ShardMap &m, const uint32_t k, uint32_t &tile, unsigned long long &lanes) {
    uint32_t sh, loc, cnt;
    shard_find(m, k, sh, loc, cnt);
    const FlagTile ft = F.tiles[sh * F.tile_cap + loc];
    tile = uniform_u32(ft.tile);
    lanes = uniform_u64(ft.mask);
}
// frame row of local row lr: the shard's stripe arithmetic, or adaptive pass 1's row table (DFrame::rows).  The term lanes of a partial
// last tile row ask for rows past the last local row; only invalid lanes use those.
__device__ __forceinline__ int frame_row(const DFrame &F, const int lr) {
    if (F.rows != nullptr) return F.rows[lr < F.local_rows ? lr : F.local_rows - 1];
    return F.row0 + ((lr / F.stripe) * F.nranks + F.rank) * F.stripe + (lr % F.stripe);
}

// arealight::getPointLights / createSpherePoint (arealight.hpp:15-25, flyscene.cpp:956-972): sample s of light p
// N > 64 samples: a k_shadow pass holds 64 of them.  When both grid sides are multiples of 8 a pass is an 8x8 BLOCK of the grid
// (pass p = block (p / (vsteps/8), p % (vsteps/8)), lane l = cell (l / 8, l % 8) of it) instead of 64 consecutive samples (a
// 4 x 16 strip of a 16 x 16 light): the 64 segments of a unit form a tighter bundle (-6 % on cfg4's k_shadow).  The visibility
// word of pass p keeps bit l for lane l, so k_shade looks sample (i, j) up in word (i/8)*(vsteps/8) + j/8, bit (i%8)*8 + j%8.
__device__ __forceinline__ bool sample_blocks(const DLights &L) {
    return L.mode == RT_LIGHT_AREA && L.n_samples > 64 && (L.usteps & 7) == 0 && (L.vsteps & 7) == 0;
}

// The sample grid of one light: sample (i, j) = ((i + 0.5) * cx, (j + 0.5) * cy, z).  cx and cy each hold a float division, so a
// caller that needs several samples of the same light (k_shadow: the lane's sample + the two corners of the sample box) builds
// the grid once; (i, j) = (s / vsteps, s % vsteps) are passed as the floats i + 0.5 and j + 0.5, which the callers keep out of
// their hot loops (an integer division by a run-time value costs ~25 VALU instructions).
struct LightGrid { float cx, cy, z, px, py; bool point; };
__device__ __forceinline__ LightGrid light_grid(const DLights &L, const float px, const float py, const float pz) {
    LightGrid g;
    g.point = L.mode == RT_LIGHT_POINT;
    g.px = px; g.py = py;
    const float ux = px + L.len_x * 1.0f;     // uvec = corner + lengthX * (1,0,0)
    const float uz = pz + L.len_x * 0.0f;
    const float vy = py + L.len_y * 1.0f;     // vvec = corner + lengthY * (0,1,0)
    g.cx = ux / static_cast<float>(L.usteps);
    g.cy = vy / static_cast<float>(L.vsteps);
    g.z = g.point ? pz : uz;
    return g;
}
__device__ __forceinline__ void grid_sample(const LightGrid &g, const float fi, const float fj, float &sx, float &sy, float &sz) {
    sx = g.point ? g.px : fi * g.cx;
    sy = g.point ? g.py : fj * g.cy;
    sz = g.z;
}
__device__ __forceinline__ void light_sample_ij(const DLights &L, const float px, const float py, const float pz, const float fi, const float fj,
                                                float &sx, float &sy, float &sz) {
    grid_sample(light_grid(L, px, py, pz), fi, fj, sx, sy, sz);
}
// RT_LIGHT_SPHERE (createSpherePoint's third branch, flyscene.cpp:974-995): sample s of a light at p = offsets[s] + p, its samples lie in
// p + obox (float addition is monotone, so the box of the offsets bounds the samples exactly)
__device__ __forceinline__ void sphere_sample(const DLights &L, const uint32_t s, const float px, const float py, const float pz, float &sx, float &sy, float &sz) {
    const uint32_t k = s < static_cast<uint32_t>(L.n_samples) ? s : 0u;
    sx = L.offsets[k * 3u] + px; sy = L.offsets[k * 3u + 1u] + py; sz = L.offsets[k * 3u + 2u] + pz;
}
__device__ __forceinline__ void sphere_box(const DLights &L, const float px, const float py, const float pz, float &x0, float &y0, float &z0, float &x1, float &y1,
                                           float &z1) {
    x0 = L.obox[0] + px; y0 = L.obox[1] + py; z0 = L.obox[2] + pz; x1 = L.obox[3] + px; y1 = L.obox[4] + py; z1 = L.obox[5] + pz;
}
// the box of a light's samples between grid corners (i0, j0) and (i1, j1): the samples are monotone in each grid index, so the two corners give
// the exact extremes (min / max per axis is the caller's); a sphere light's box is its offsets' box
__device__ __forceinline__ void light_sample_box(const DLights &L, const LightGrid &g, const float px, const float py, const float pz, const float i0, const float j0,
                                                 const float i1, const float j1, float &x0, float &y0, float &z0, float &x1, float &y1, float &z1) {
    grid_sample(g, i0, j0, x0, y0, z0);
    grid_sample(g, i1, j1, x1, y1, z1);
    if (L.mode == RT_LIGHT_SPHERE) sphere_box(L, px, py, pz, x0, y0, z0, x1, y1, z1);
}
// the light a hit is lit by: scene light l, or the light its ray carries (lmode: a mirror bounce)
__device__ __forceinline__ void light_point(const DLights &L, const int l, const uint32_t lmode, const float lx, const float ly, const float lz, float &px, float &py,
                                            float &pz) {
    px = lmode ? lx : L.pos[l][0]; py = lmode ? ly : L.pos[l][1]; pz = lmode ? lz : L.pos[l][2];
}
// the hit point of a shade item, as every shadow kernel forms it (flyscene.cpp:695)
__device__ __forceinline__ void hit_point(const ShadeItem &it, float &hx, float &hy, float &hz) {
    hx = it.ox + it.t * it.dx; hy = it.oy + it.t * it.dy; hz = it.oz + it.t * it.dz;
}
// the plane-rule packet of a (hit, light) unit: the hit h and the two extreme samples of the light
__device__ __forceinline__ SegPacket seg_packet(const float hx, const float hy, const float hz, const float x0, const float y0, const float z0, const float x1,
                                                const float y1, const float z1) {
    SegPacket g;
    g.on = true; g.prepared = false;
    g.hx = hx; g.hy = hy; g.hz = hz;
    g.slx = fminf(x0, x1); g.shx = fmaxf(x0, x1);
    g.sly = fminf(y0, y1); g.shy = fmaxf(y0, y1);
    g.slz = fminf(z0, z1); g.shz = fmaxf(z0, z1);
    g.m0 = 2e-5f * ((fabsf(x0) + fabsf(x1)) + (fabsf(y0) + fabsf(y1)) + (fabsf(z0) + fabsf(z1)) + (fabsf(hx) + fabsf(hy) + fabsf(hz)));
    return g;
}
__device__ __forceinline__ void light_sample(const DLights &L, const float px, const float py, const float pz, const int s,
                                             float &sx, float &sy, float &sz) {
    const int i = s / L.vsteps, j = s - i * L.vsteps;
    light_sample_ij(L, px, py, pz, static_cast<float>(i) + 0.5f, static_cast<float>(j) + 0.5f, sx, sy, sz);
}

// Supersampling (rt_set_supersampling, DESIGN.md §5, Supersampling): internal column / row v of the sub-sample frame is sub-sample v % n of pixel v / n, at
// the raster coordinate (float)(v / n) + o[v % n].  n = 1 keeps (float)v.  Only the 16 term lanes of a tile evaluate it.  (o[] is read with
// an index from the kernel argument: a select chain over its four SGPR values kept three hoisted VGPR copies live across the tile loop.)
// Passes (rt_set_passes, DESIGN.md §5, Multi-pass accumulation): the frames of a pass p > 0 run the PASS instantiations of the primary kernels.
// There columns read the first half of o[] and rows the second (the halves differ from pass 1 on), n = 1 takes the table too --
// (float)v + o[0] -- and lens_ray / shutter_time XOR the pass key into their scramble.  Pass 0 keeps the instantiations it always had: every
// extra per-lane term in this function costs them a VGPR (and k_stage<true, false, 1> an occupancy step at 96), so it is compiled out there.
template <bool PASS = false>
__device__ __forceinline__ float raster_coord(const DFrame &F, const int v, const bool col) {
    if (PASS) {
        if (F.ss == 1) return static_cast<float>(v) + (col ? F.sso[0] : F.sso[RT_MAX_SUPERSAMPLING]);
        const int i = static_cast<int>(__umulhi(static_cast<uint32_t>(v), F.ss_mul)), s = v - i * F.ss;
        return static_cast<float>(i) + F.sso[s + (col ? 0 : RT_MAX_SUPERSAMPLING)];
    }
    if (F.ss == 1) return static_cast<float>(v);
    const int i = static_cast<int>(__umulhi(static_cast<uint32_t>(v), F.ss_mul)), s = v - i * F.ss;     // v / n (v < 2^31)
    return static_cast<float>(i) + F.sso[s];
}

// Camera::screenToWorld (camera.hpp:155-173): raster -> [-1,1] in double, cast, perspective scale, inverse view.  One definition for
// the fused k_trace, the staged k_stage and the probe kernel (rt_primary_points).
// the same point for the (sub-sample) pixel (x0 + (lane & 7), y0 + (lane >> 3)) of an 8 x 8 tile, with the tile's sixteen double divisions done ONCE: lane c < 8
// evaluates the column term of x0 + c, lane 8 + r the row term of row ys[r] (the caller passes each lane ITS candidate: the row of lane 8 + r is
// the y of the lanes r * 8 .. r * 8 + 7), every lane then fetches its two terms.  Same double operations on the same operands as screen_point --
// 2 divisions per lane become 1 (a double division is ~30 half-rate instructions: a third of what a sky tile costs).
template <bool PASS = false>
__device__ __forceinline__ void screen_point_tile(const DCam &cam, const DFrame &F, const int lane, const int x0, const int y_of_row_lane, float &sx, float &sy,
                                                  float &sz) {
    const bool col = lane < 8;
    const float f = raster_coord<PASS>(F, col ? x0 + lane : y_of_row_lane, col);
    const double q = 2.0 * static_cast<double>(f - (col ? cam.vp[0] : cam.vp[1])) / static_cast<double>(col ? cam.vp[2] : cam.vp[3]);
    const float term = col ? static_cast<float>(q - 1.0) : static_cast<float>(1.0 - q);
    float n0 = __shfl(term, lane & 7, 64);
    float n1 = __shfl(term, 8 + (lane >> 3), 64);
    const float n2 = -1.0f;
    n0 = n0 * cam.k0;
    n1 = n1 * cam.k1;
    const float *m = cam.inv_view;
    sx = ((m[0] * n0 + m[1] * n1) + m[2] * n2) + m[3] * 1.0f;
    sy = ((m[4] * n0 + m[5] * n1) + m[6] * n2) + m[7] * 1.0f;
    sz = ((m[8] * n0 + m[9] * n1) + m[10] * n2) + m[11] * 1.0f;
}
// the per-lane form: the point of the raster coordinates (fi, fj) -- a pixel's own (screen_point) or a sub-sample's (k_gbuffer, whose lanes
// hold the same sub-sample of 64 neighbouring pixels: no eight contiguous internal columns for screen_point_tile to share)
__device__ __forceinline__ void screen_point_at(const DCam &cam, const float fi, const float fj, float &sx, float &sy, float &sz) {
    float n0 = static_cast<float>(2.0 * static_cast<double>(fi - cam.vp[0]) / static_cast<double>(cam.vp[2]) - 1.0);
    float n1 = static_cast<float>(1.0 - 2.0 * static_cast<double>(fj - cam.vp[1]) / static_cast<double>(cam.vp[3]));
    const float n2 = -1.0f;
    n0 = n0 * cam.k0;
    n1 = n1 * cam.k1;
    const float *m = cam.inv_view;
    sx = ((m[0] * n0 + m[1] * n1) + m[2] * n2) + m[3] * 1.0f;
    sy = ((m[4] * n0 + m[5] * n1) + m[6] * n2) + m[7] * 1.0f;
    sz = ((m[8] * n0 + m[9] * n1) + m[10] * n2) + m[11] * 1.0f;
}
__device__ __forceinline__ void screen_point(const DCam &cam, const int x, const int y, float &sx, float &sy, float &sz) {
    screen_point_at(cam, static_cast<float>(x), static_cast<float>(y), sx, sy, sz);
}

// The per-pixel scramble of the lens and the shutter (rt_set_lens, rt_set_shutter in include/rt_mi355x.h define it).
__device__ __forceinline__ uint32_t mix32(uint32_t h) {
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    return h;
}
// internal column x / frame row y of the sub-sample frame -> output pixel (i, j), sub-sample (sx, sy) = (x % n, y % n); n = 1: the pixel itself
__device__ __forceinline__ void pixel_of(const DFrame &F, const int x, const int y, uint32_t &i, uint32_t &j, uint32_t &sx, uint32_t &sy) {
    const uint32_t n = static_cast<uint32_t>(F.ss);
    i = static_cast<uint32_t>(x); j = static_cast<uint32_t>(y); sx = 0u; sy = 0u;
    if (n > 1u) {
        i = __umulhi(static_cast<uint32_t>(x), F.ss_mul); j = __umulhi(static_cast<uint32_t>(y), F.ss_mul);
        sx = static_cast<uint32_t>(x) - i * n; sy = static_cast<uint32_t>(y) - j * n;
    }
}
// h of output pixel (i, j), of this pass where PASS (rt_set_passes)
template <bool PASS>
__device__ __forceinline__ uint32_t pixel_scramble(const DFrame &F, const uint32_t i, const uint32_t j) {
    uint32_t h = (i * 0x9E3779B1u) ^ (j * 0x85EBCA6Bu);
    if (PASS) h ^= F.pass_key;
    return mix32(h);
}

// Thin lens (rt_set_lens in include/rt_mi355x.h defines every step; DESIGN.md §5, Depth of field): the primary ray of internal column x /
// frame row y of the sub-sample frame, whose screen point is (sx, sy, sz), starts at a point of the lens and runs through the point of the
// focus plane on the pinhole ray.  Only the LENS instantiations of the primary kernels call it (DFrame::lens != null), so the pinhole
// instantiations keep their uniform origin.  The table index is rot * n*n + k with rot < 64 and k clamped below n*n: inside the table
// whatever x and y a lane past the frame edge carries.
template <bool PASS = false>
__device__ __forceinline__ void lens_ray(const DCam &cam, const DFrame &F, const int x, const int y, const float sx, const float sy, const float sz,
                                         float &ox, float &oy, float &oz, float &dx, float &dy, float &dz) {
    const float cx = cam.center[0], cy = cam.center[1], cz = cam.center[2];
    const float vx = sx - cx, vy = sy - cy, vz = sz - cz;                                   // 1. the pinhole direction
    const float px = cx + F.lens_focus * vx, py = cy + F.lens_focus * vy, pz = cz + F.lens_focus * vz;   // 2. the focus point
    const uint32_t n = static_cast<uint32_t>(F.ss), nn = n * n;
    uint32_t i, j, sx_, sy_;
    pixel_of(F, x, y, i, j, sx_, sy_);
    const uint32_t sub = sy_ * n + sx_;
    const uint32_t h = pixel_scramble<PASS>(F, i, j);                                         // 3. the per-pixel scramble
    uint32_t k = 0u;
    if (n > 1u) {
        const uint32_t v = sub + ((h >> 8) & 0xFFFFu);
        k = v - __umulhi(v, F.lens_mul) * nn;                                                 // v % (n*n)
        k = k < nn ? k : nn - 1u;
    }
    const float2 t = F.lens[(h >> 26) * nn + k];
    const float a = F.lens_aperture * t.x, b = F.lens_aperture * t.y;                         // 4. the lens point
    const float *m = cam.inv_view;
    ox = (cx + a * m[0]) + b * m[1]; oy = (cy + a * m[4]) + b * m[5]; oz = (cz + a * m[8]) + b * m[9];
    dx = px - ox; dy = py - oy; dz = pz - oz;                                                 // 5. direction = focus point - origin (UNNORMALISED)
}

// Camera motion blur (rt_set_shutter in include/rt_mi355x.h defines every step; DESIGN.md §5, Motion blur).  Only the SHUTTER
// instantiations of the primary kernels call these: there the CAMERA is a per-lane quantity.
// shutter_time: the time t in [0, 1) of internal column x / frame row y of the sub-sample frame -- the lens's per-pixel scramble h, mixed
// once more into g, picks the pixel's cyclic shift of the n*n time slots and the jitter u inside the slot.  Pure arithmetic on x and y:
// a lane past the frame edge gets some t in [0, 1) and reads nothing with it.
template <bool PASS = false>
__device__ __forceinline__ float shutter_time(const DFrame &F, const int x, const int y) {
    const uint32_t n = static_cast<uint32_t>(F.ss), nn = n * n;
    uint32_t i, j, sx_, sy_;
    pixel_of(F, x, y, i, j, sx_, sy_);
    const uint32_t sub = sx_ * n + sy_;                                                       // the transpose of the lens's
    const uint32_t g = mix32(pixel_scramble<PASS>(F, i, j) ^ 0x68E31DA4u);
    uint32_t slot = 0u;
    if (n > 1u) {
        const uint32_t v = sub + (g & 0xFFFFu);
        slot = v - __umulhi(v, F.lens_mul) * nn;                                              // v % (n*n)
    }
    const float u = static_cast<float>(g >> 16) * 1.52587890625e-05f;                         // 2^-16: exact
    return (static_cast<float>(slot) + u) / static_cast<float>(nn);                           // exact sum, one correctly rounded division
}
// shutter_camera: K(t), each of the 15 pose values q_open + t * d (multiply, then add), or q_open itself where d == 0 (so that a still
// shutter is the open camera bit for bit, negative zeros included).  vp, k0, k1 are open's and stay wave-uniform.
__device__ __forceinline__ DCam shutter_camera(const DCam &open, const DShutter &sh, const float t) {
    DCam k = open;
#pragma unroll
    for (int q = 0; q < 3; ++q) k.center[q] = sh.d[q] == 0.0f ? open.center[q] : open.center[q] + t * sh.d[q];
#pragma unroll
    for (int q = 0; q < 12; ++q) k.inv_view[q] = sh.d[3 + q] == 0.0f ? open.inv_view[q] : open.inv_view[q] + t * sh.d[3 + q];
    return k;
}
// the primary ray of a SHUTTER tile: the lane's own camera first, then the screen point and the pinhole or (F.lens != null, a wave-uniform
// branch: both cases have a per-lane origin) the thin-lens ray of that camera, by the functions every other frame uses.  y_r is the row
// term lane's frame row as for screen_point_tile.
template <bool PASS = false>
__device__ __forceinline__ void shutter_ray(const DCam &open, const DShutter &sh, const DFrame &F, const int lane, const int x, const int x0, const int y_r,
                                            float &ox, float &oy, float &oz, float &dx, float &dy, float &dz) {
    const int y = __shfl(y_r, 8 + (lane >> 3), 64);
    const DCam k = shutter_camera(open, sh, shutter_time<PASS>(F, x, y));
    float sx, sy, sz;
    screen_point_tile<PASS>(k, F, lane, x0, y_r, sx, sy, sz);
    if (F.lens != nullptr) lens_ray<PASS>(k, F, x, y, sx, sy, sz, ox, oy, oz, dx, dy, dz);
    else {
        ox = k.center[0]; oy = k.center[1]; oz = k.center[2];
        dx = sx - ox; dy = sy - oy; dz = sz - oz;
    }
}

// what a primary pixel whose ray finds nothing records (the trace kernels) and what k_resolve folds for a pixel that was never traced
__device__ __forceinline__ float4 background_record() { return make_float4(1.f, 1.f, 1.f, __uint_as_float(KIND_CONST)); }
// what a hit that no light centre sees records
__device__ __forceinline__ float4 shadow_record() { return make_float4(0.f, 0.f, 0.f, __uint_as_float(KIND_CONST)); }

// Primary culling (DFrame::cull, DESIGN.md §5, Primary culling): DCamBlock::rect in frame PIXELS, [x0, x1) x [y0, y1).  The host proves that
// no primary ray of a pixel outside it passes the root-box test, so such a pixel is a culled pixel with the background colour before its
// ray exists.  All of it is wave-uniform scalar work.
struct CullRect { int x0, y0, x1, y1; };
// The camera block of the frame, from the source its CamArg names (rt_device.hpp): device memory under a captured graph, the kernel argument
// itself in an eager launch sequence.  The branch is wave-uniform and both sides are scalar loads.  (Member by member, and never through the
// address of ca.val: a pointer that may be either source sends the argument through scratch.  The empty asm behind the loads from device
// memory keeps them together in their branch: without it the compiler hoists the argument's loads and branches once per dword of the block --
// k_trace<true, false, true> then spills 361 SGPRs instead of 100.)
#define RT_CAM_LOADS_STAY() asm volatile("" ::: "memory")
__device__ __forceinline__ DCam cam_of(const CamArg &ca) {
    DCam cam;
    if (ca.ptr != nullptr) { cam = ca.ptr->cam; RT_CAM_LOADS_STAY(); }
    else cam = ca.val.cam;
    return cam;
}
__device__ __forceinline__ DShutter shutter_of(const CamArg &ca) {
    DShutter sh;
    if (ca.ptr != nullptr) { sh = ca.ptr->sh; RT_CAM_LOADS_STAY(); }
    else sh = ca.val.sh;
    return sh;
}
__device__ __forceinline__ CullRect cull_rect(const CamArg &ca) {
    int r0, r1, r2, r3;
    if (ca.ptr != nullptr) { r0 = ca.ptr->rect[0]; r1 = ca.ptr->rect[1]; r2 = ca.ptr->rect[2]; r3 = ca.ptr->rect[3]; RT_CAM_LOADS_STAY(); }
    else { r0 = ca.val.rect[0]; r1 = ca.val.rect[1]; r2 = ca.val.rect[2]; r3 = ca.val.rect[3]; }
    return CullRect{r0 * 8, r1 * 8, r2 * 8, r3 * 8};
}
// every pixel of local tile (tx, ty) lies outside the rectangle.  (The frame rows of a tile's local rows increase with the local row, so the
// first and the last valid one bound them; a tile of a striped shard that straddles the rectangle without a row inside is merely kept.)
__device__ __forceinline__ bool tile_outside(const DFrame &F, const CullRect &R, const int tx, const int ty) {
    const int lr0 = ty * 8, lr1 = lr0 + 7 < F.local_rows ? lr0 + 7 : F.local_rows - 1;
    return tx * 8 >= R.x1 || tx * 8 + 8 <= R.x0 || frame_row(F, lr0) >= R.y1 || frame_row(F, lr1) < R.y0;
}

// The ray of a lane of a tile, for the fused k_trace and the staged k_stage.  pre: the ray takes part in the walk -- a primary ray passed
// the root-box pre-test of raytraceScene's loop (flyscene.cpp:576), a listed ray is there.
struct TileRay {
    bool valid, pre;
    uint32_t pix, lmode;
    float ox, oy, oz, dx, dy, dz, lx, ly, lz;
};
// the root-box pre-test of raytraceScene's loop on the primary ray (o, d) (flyscene.cpp:576)
__device__ __forceinline__ bool root_pre_test(const DNode &root, const float ox, const float oy, const float oz, const float dx, const float dy, const float dz) {
    return box_hit_verified(root.bmin, ox, oy, oz, dx, dy, dz, __builtin_amdgcn_rcpf(dx), __builtin_amdgcn_rcpf(dy), __builtin_amdgcn_rcpf(dz));
}
// the primary half: lane = pixel (lane & 7, lane >> 3) of frame tile pt; a lane outside the mask `lanes` is invalid like one past the frame edge
template <bool LENS, bool SHUTTER, bool PASS>
__device__ __forceinline__ TileRay primary_ray(const uint32_t pt, const unsigned long long lanes, const int lane, const DFrame &F, const DCam &cam,
                                               const DShutter &shut, const DNode &root) {
    TileRay r;
    r.lx = r.ly = r.lz = 0.f; r.lmode = 0u;
    const int tx = static_cast<int>(pt % static_cast<uint32_t>(F.tiles_x)), ty = static_cast<int>(pt / static_cast<uint32_t>(F.tiles_x));
    const int x = tx * 8 + (lane & 7), lr = ty * 8 + (lane >> 3);
    r.valid = (x < F.width) && (lr < F.local_rows) && ((lanes >> lane) & 1ull) != 0ull;
    r.pix = static_cast<uint32_t>(lr) * static_cast<uint32_t>(F.width) + static_cast<uint32_t>(x);
    float sx, sy, sz;
    {   // (lane 8 + r evaluates the row term of tile row r: the frame row of local row ty * 8 + r)
        const int lr_r = ty * 8 + ((lane - 8) & 7);
        const int y_r = frame_row(F, lr_r);
        if (SHUTTER) shutter_ray<PASS>(cam, shut, F, lane, x, tx * 8, y_r, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
        else screen_point_tile<PASS>(cam, F, lane, tx * 8, y_r, sx, sy, sz);
        if (LENS) lens_ray<PASS>(cam, F, x, __shfl(y_r, 8 + (lane >> 3), 64), sx, sy, sz, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
    }
    if (!LENS && !SHUTTER) {
        r.ox = cam.center[0]; r.oy = cam.center[1]; r.oz = cam.center[2];
        r.dx = sx - r.ox; r.dy = sy - r.oy; r.dz = sz - r.oz;          // direction = screen - origin (UNNORMALISED), flyscene.cpp:619
    }
    r.pre = r.valid && root_pre_test(root, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
    return r;
}
// the listed half: lane = ray `lane` of dense group `group` of the sharded ray list (rmap: its shard map)
__device__ __forceinline__ TileRay listed_ray(const uint32_t group, const int lane, const DFrame &F, const RayItem *__restrict__ rays_in, const ShardMap &rmap) {
    TileRay r;
    uint32_t sh, tj, n_in;
    shard_find(rmap, group, sh, tj, n_in);
    const uint32_t k = tj * 64u + static_cast<uint32_t>(lane);
    r.valid = k < n_in;
    const RayItem it = rays_in[r.valid ? sh * F.ray_cap + k : 0u];
    r.ox = it.ox; r.oy = it.oy; r.oz = it.oz; r.dx = it.dx; r.dy = it.dy; r.dz = it.dz;
    r.lx = it.lx; r.ly = it.ly; r.lz = it.lz; r.lmode = it.lmode; r.pix = it.pix;
    r.pre = r.valid;
    return r;
}
// dense tile number -> ray: a primary launch maps it through k_flag's list first (adaptive pass 2; rmap is that list's map there)
template <bool PRIMARY, bool LENS, bool SHUTTER, bool PASS>
__device__ __forceinline__ TileRay tile_ray(const uint32_t tile, const int lane, const DFrame &F, const DCam &cam, const DShutter &shut, const DNode &root,
                                            const RayItem *__restrict__ rays_in, const ShardMap &rmap) {
    if (PRIMARY) {
        uint32_t pt = tile;
        unsigned long long lanes = ~0ull;
        if (F.tiles != nullptr) flag_tile(F, rmap, tile, pt, lanes);
        return primary_ray<LENS, SHUTTER, PASS>(pt, lanes, lane, F, cam, shut, root);
    }
    return listed_ray(tile, lane, F, rays_in, rmap);
}

// The finish of a tile, once its closest hits and their light-centre visibility are known: the BACKGROUND / SHADOW record, the hit outputs,
// and the compaction of the lit hits into the shade list (wave ballot + prefix, one atomic per wave).
__device__ __forceinline__ void finish_tile(const TileRay &r, const bool hit, const bool lit, const int best_f, const float best_t, const uint32_t tile,
                                            const int level, const int lane, const DFrame &F, ShadeItem *__restrict__ items, Control *__restrict__ ctl,
                                            float4 *__restrict__ rec, int32_t *__restrict__ out_hit, float *__restrict__ out_t) {
    if (r.valid) {
        if (!hit) rec[r.pix] = background_record();                // BACKGROUND
        else if (!lit) rec[r.pix] = shadow_record();               // SHADOW
        if (out_hit) out_hit[r.pix] = hit ? best_f : -1;
        if (out_t) out_t[r.pix] = hit ? best_t : -1.0f;
    }
    const unsigned long long lm = __ballot(lit);
    if (lm != 0ull) {
        bool fits;
        const uint32_t base = shard_reserve(ctl->n_items[level], &ctl->overflow, tile, static_cast<uint32_t>(__popcll(lm)), F.item_cap, lane, fits);
        if (lit && fits) {
            ShadeItem o;
            o.ox = r.ox; o.oy = r.oy; o.oz = r.oz; o.dx = r.dx; o.dy = r.dy; o.dz = r.dz;
            o.lx = r.lx; o.ly = r.ly; o.lz = r.lz; o.lmode = r.lmode; o.pix = r.pix; o.face = best_f; o.t = best_t;
            o.pad0 = o.pad1 = o.pad2 = 0u;
            items[base + lanes_below(lm)] = o;
        }
    }
}
// per-wave counters of a trace kernel -> control block.  c_outside: pixels no wave counted (k_trace's cull window), added once by the caller's pick
template <bool PRIMARY, bool COUNT>
__device__ __forceinline__ void flush_trace_counters(Control *__restrict__ ctl, const int lane, const int level, uint32_t c_rays, uint32_t c_cull,
                                                     uint32_t c_centre, uint32_t c_box, uint32_t c_ref, const uint32_t c_outside) {
    c_rays = wave_sum(c_rays); c_cull = wave_sum(c_cull); c_centre = wave_sum(c_centre);
    c_cull += c_outside;
    if (COUNT) { c_box = wave_sum(c_box); c_ref = wave_sum(c_ref); }
    if (lane == 0) {
        if (c_rays) stat_add(ctl, (PRIMARY || level == 0) ? ST_RAYS_PRIMARY : ST_RAYS_BOUNCE, c_rays);
        if (c_cull) stat_add(ctl, ST_PIXELS_CULLED, c_cull);
        if (c_centre) stat_add(ctl, ST_RAYS_CENTRE, c_centre);
        if (COUNT) {
            if (c_box) stat_add(ctl, ST_BOX_TESTS, c_box);
            if (c_ref) stat_add(ctl, ST_LEAF_TRI_REFS, c_ref);
        }
    }
}

// lightStrikes(hitPoint, lights): one segment per light CENTRE (flyscene.cpp:700) for the lanes with a hit at h -- true: some centre sees it.
// The fused k_trace runs it over its tree or root leaf; k_deep over the root leaf (FLAT: nothing of the tree arguments is read).
template <bool COUNT, bool FLAT>
__device__ __forceinline__ bool centre_lit(const DNode &root, const DNode *__restrict__ nodes, const TriRec *__restrict__ tris, const ChunkBound *__restrict__ chunks,
                                           const uint32_t *__restrict__ leaf_chunk0, const float extent, const WaveStack stk, const int lane, const DLights &L,
                                           const bool hit, const float hx, const float hy, const float hz, const uint32_t lmode, const float lx, const float ly,
                                           const float lz, uint32_t &c_centre, uint32_t &c_box, uint32_t &c_ref) {
    bool lit = false;
    const int nl_lane = lmode ? 1 : L.n_lights;
    const int nl_wave = (__ballot(hit && lmode == 0u) != 0ull) ? L.n_lights : 1;
    if (__ballot(hit) != 0ull) {
        for (int l = 0; l < nl_wave; ++l) {
            const bool act = hit && (l < nl_lane);
            float px, py, pz;
            light_point(L, l, lmode, lx, ly, lz, px, py, pz);
            c_centre += act ? 1u : 0u;
            if (COUNT && act) c_box += 1;
            const WalkRay ray = segment_ray(px, py, pz, hx, hy, hz);
            const bool occ = walk<true, COUNT, FLAT>(root, nodes, tris, chunks, leaf_chunk0, extent, stk, lane, walk_plain(), LanePlane{}, act && root_hit(root, ray), ray,
                                                     c_box, c_ref);
            lit = lit || (act && !occ);
        }
    }
    return lit;
}
// traceRay's closest hit over the root leaf of a flat scene (flyscene.cpp:655-691), exactly as k_trace<.., FLAT> runs it: k_shade's bounce rays, k_deep
__device__ __forceinline__ Hit flat_closest_hit(const DNode &root, const TriRec *__restrict__ tris, const bool active, const float ox, const float oy, const float oz,
                                                const float dx, const float dy, const float dz) {
    const WalkRay ray = trace_ray(ox, oy, oz, dx, dy, dz);
    uint32_t cu0 = 0, cu1 = 0;
    return flat_walk<false, false>(root, tris, active && root_hit(root, ray), seg_off(), 0ull, LanePlane{}, ray, cu0, cu1);
}

// ======================================================================================================
// K1: closest hit + light-centre visibility.  PRIMARY: fused primary-ray generation (Camera::screenToWorld)
// and root-AABB cull of raytraceScene's serial loop (flyscene.cpp:573-598); otherwise reads compacted rays.
// ======================================================================================================
template <bool PRIMARY, bool COUNT, bool FLAT, bool LENS = false, bool SHUTTER = false, bool PASS = false>
__global__ __launch_bounds__(RT_WAVES * 64) void k_trace(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                          const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                          const DScene S, const CamArg camarg, const DLights L, const DFrame F,
                                                          const int level, const int ctr_slot,
                                                          const RayItem *__restrict__ rays_in, ShadeItem *__restrict__ items,
                                                          Control *__restrict__ ctl, float4 *__restrict__ rec,
                                                          int32_t *__restrict__ out_hit, float *__restrict__ out_t) {
    __shared__ uint4 s_stage[FLAT ? 1 : RT_WAVES * RT_STAGE_TRIS * 5];        // flat scenes need neither staging buffer nor stack
    __shared__ unsigned long long s_mask[FLAT ? 1 : RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[FLAT ? 1 : RT_WAVES * RT_STACK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + (FLAT ? 0 : wave * RT_STACK), s_mask + (FLAT ? 0 : wave * RT_STACK), s_stage + (FLAT ? 0 : wave * RT_STAGE_TRIS * 5)};
    ShardMap rmap{0u, 0u, 0u, 0u};
    if (!PRIMARY) rmap = shard_map(ctl->n_rays[level], lane, 0xffffffffu, 1u, 64u);
    else if (F.tiles != nullptr) rmap = shard_map(ctl->n_flag, lane, F.tile_cap, 1u, 1u);          // adaptive pass 2: k_flag's tiles
    uint32_t ntiles = (!PRIMARY || F.tiles != nullptr) ? rmap.total : static_cast<uint32_t>(F.tiles_x) * static_cast<uint32_t>(F.tiles_y);
    if (!PRIMARY && ntiles == 0u) return;         // an empty bounce level: every wave leaves ahead of the root node (no counter to flush, no queue head taken)
    const DNode root = nodes[0];
    // the camera: device memory under a captured hipGraph (a replay uploads a new one), the kernel argument itself in an eager sequence
    DCam cam;
    if (PRIMARY) cam = cam_of(camarg);
    DShutter shut;                   // SHUTTER: cam is the camera at shutter open, shut the way to the one at shutter close
    if (PRIMARY && SHUTTER) shut = shutter_of(camarg);
    // primary culling: the pinhole one-ray frames only (the host leaves F.cull 0 for every other frame, whose instantiations compile this out)
    constexpr bool CULL = PRIMARY && !COUNT && !LENS && !SHUTTER && !PASS;
    const bool cull = CULL && F.cull != 0;
    CullRect crect{0, 0, 0, 0};
    // window: one shard holds the rows row0 + lr and nobody asks for hit ids, so the queue runs over the tiles that hold a pixel of the rectangle
    // -- tiles [wx0, wx0 + ww) x [wy0, ..) of the shard -- and the pixels of all the others are counted here, once
    bool window = false;
    uint32_t wx0 = 0, wy0 = 0, ww = 1, c_outside = 0;
    if (cull) {
        crect = cull_rect(camarg);
        if (F.nranks == 1 && out_hit == nullptr && out_t == nullptr) {
            window = true;
            const int lx0 = crect.x0 < F.width ? crect.x0 : F.width, lx1 = crect.x1 < F.width ? crect.x1 : F.width;
            int ly0 = crect.y0 - F.row0, ly1 = crect.y1 - F.row0;
            ly0 = ly0 < 0 ? 0 : (ly0 < F.local_rows ? ly0 : F.local_rows);
            ly1 = ly1 < 0 ? 0 : (ly1 < F.local_rows ? ly1 : F.local_rows);
            ntiles = 0u; c_outside = F.npix;
            if (lx0 < lx1 && ly0 < ly1) {
                const int wx1 = (lx1 + 7) / 8, wy1 = (ly1 + 7) / 8;
                wx0 = static_cast<uint32_t>(lx0 / 8); wy0 = static_cast<uint32_t>(ly0 / 8);
                ww = static_cast<uint32_t>(wx1) - wx0;
                ntiles = ww * (static_cast<uint32_t>(wy1) - wy0);
                const int px1 = wx1 * 8 < F.width ? wx1 * 8 : F.width, py1 = wy1 * 8 < F.local_rows ? wy1 * 8 : F.local_rows;
                c_outside = F.npix - static_cast<uint32_t>(px1 - static_cast<int>(wx0) * 8) * static_cast<uint32_t>(py1 - static_cast<int>(wy0) * 8);
            }
        }
    }

    uint32_t c_rays = 0, c_cull = 0, c_centre = 0, c_box = 0, c_ref = 0;
    ShardedQueue q;
    if (F.dyn_trace) q.init(ctl->queue[ctr_slot], ntiles, gridDim.x * RT_WAVES, blockIdx.x, lane);
    else q.init_static(ntiles, gridDim.x * RT_WAVES, uniform_u32(blockIdx.x * RT_WAVES + static_cast<uint32_t>(wave)), lane);
    for (uint32_t tile = 0; q.next(tile);) {
        RT_PROF_ADD(lane, WORK_UNITS, 1);
        TileRay r;
        if (PRIMARY) {
            uint32_t pt = tile;
            unsigned long long lanes = ~0ull;
            if (F.tiles != nullptr) flag_tile(F, rmap, tile, pt, lanes);       // (a lane outside the mask is invalid like one past the frame edge)
            if (window) pt = (wy0 + tile / ww) * static_cast<uint32_t>(F.tiles_x) + wx0 + tile % ww;       // the tile-th tile of the window
            if (cull && !window) {
                const int tx = static_cast<int>(pt % static_cast<uint32_t>(F.tiles_x)), ty = static_cast<int>(pt / static_cast<uint32_t>(F.tiles_x));
                if (tile_outside(F, crect, tx, ty)) {
                    // no ray, no box test, no record: its pixels are culled pixels (k_resolve stores their colour)
                    const int x = tx * 8 + (lane & 7), lr = ty * 8 + (lane >> 3);
                    const bool valid = (x < F.width) && (lr < F.local_rows) && ((lanes >> lane) & 1ull) != 0ull;
                    const uint32_t pix = static_cast<uint32_t>(lr) * static_cast<uint32_t>(F.width) + static_cast<uint32_t>(x);
                    c_cull += valid ? 1u : 0u;
                    if (valid && out_hit) out_hit[pix] = -1;
                    if (valid && out_t) out_t[pix] = -1.0f;
                    continue;
                }
            }
            r = primary_ray<LENS, SHUTTER, PASS>(pt, lanes, lane, F, cam, shut, root);
            c_cull += (r.valid && !r.pre) ? 1u : 0u;
        } else {
            r = listed_ray(tile, lane, F, rays_in, rmap);
        }
        bool in_root = r.pre;
        c_rays += in_root ? 1u : 0u;
        const WalkRay ray = trace_ray(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
        if (COUNT && in_root) c_box += 1;
        in_root = in_root && root_hit(root, ray);

        const Hit best = walk<false, COUNT, FLAT>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, in_root, ray, c_box, c_ref);
        const bool hit = r.valid && found(best.face, S.n_faces);
        const float hx = r.ox + best.t * r.dx, hy = r.oy + best.t * r.dy, hz = r.oz + best.t * r.dz;   // flyscene.cpp:695
        const bool lit = centre_lit<COUNT, FLAT>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, L, hit, hx, hy, hz, r.lmode, r.lx, r.ly, r.lz,
                                                 c_centre, c_box, c_ref);

        finish_tile(r, hit, lit, best.face, best.t, tile, level, lane, F, items, ctl, rec, out_hit, out_t);
    }
    // (CULL: the pixels of the tiles the window left out)
    flush_trace_counters<PRIMARY, COUNT>(ctl, lane, level, c_rays, c_cull, c_centre, c_box, c_ref, (CULL && blockIdx.x == 0 && wave == 0) ? c_outside : 0u);
}

// ======================================================================================================
// K1 for TREE scenes, split in three so that every traversal can hand work away (measured on dodgeColorTest: ONE 8x8 tile
// cost 2.45 M cycles -- the whole fused kernel -- while the average wave had 0.18 M cycles of work):
//   STAGE 0  closest hit        -> best[tile*64+lane] = (t bits << 32 | face), merged by continuations with atomicMin
//                                  (minimum t, ties to the lowest face id: exactly the reference's strict '<' over the
//                                  ascending std::set, flyscene.cpp:675-683)
//   STAGE 1  light-centre rays  -> lit[tile*lslots+l] = lane mask of visible centres, continuations clear bits (atomicAnd)
//   STAGE 2  finish             -> BACKGROUND / SHADOW records, out_hit/out_t, compaction of lit hits
// The fused k_trace above remains the path of flat scenes (cube.obj).
// ======================================================================================================

#define RT_NO_HIT_KEY 0xffffffffffffffffull

template <bool PRIMARY, bool COUNT, int STAGE, bool CONT, bool LENS = false, bool SHUTTER = false, bool PASS = false>
__global__ __launch_bounds__(RT_WAVES * 64) void k_stage(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                          const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                          const DScene S, const CamArg camarg, const DLights L, const DFrame F,
                                                          const int level, const int lslots,
                                                          const RayItem *__restrict__ rays_in, ShadeItem *__restrict__ items,
                                                          Control *__restrict__ ctl, float4 *__restrict__ rec,
                                                          int32_t *__restrict__ out_hit, float *__restrict__ out_t,
                                                          unsigned long long *best, unsigned long long *lit, const TaskQueues Q) {
    constexpr bool CONE = CONT && STAGE < 2 && !COUNT;
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    __shared__ float4 s_cone[CONE ? RT_WAVES * RT_SHAFT_TRI_REC : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, s_stage + wave * RT_STAGE_TRIS * 5};
    float4 *const cone_rec = s_cone + (CONE ? wave * RT_SHAFT_TRI_REC : 0);
    ShardMap rmap{0u, 0u, 0u, 0u};
    if (!PRIMARY) rmap = shard_map(ctl->n_rays[level], lane, 0xffffffffu, 1u, 64u);
    else if (F.tiles != nullptr) rmap = shard_map(ctl->n_flag, lane, F.tile_cap, 1u, 1u);          // adaptive pass 2: k_flag's tiles
    // (units, ray slots and lit words are numbered by the dense tile number; tile_ray maps it to the listed tile)
    const uint32_t ntiles = (!PRIMARY || F.tiles != nullptr) ? rmap.total : static_cast<uint32_t>(F.tiles_x) * static_cast<uint32_t>(F.tiles_y);

    uint32_t n_units = STAGE == 1 ? ntiles * static_cast<uint32_t>(lslots) : ntiles;
    ShardMap tmap{0u, 0u, 0u, 0u};
    if (CONT) {
        tmap = shard_map(ctl->n_task_tr[level][Q.q_in & 1u], lane, Q.cap / RT_LIST_SHARDS, 1u, 1u);      // producers clamp to the per-shard capacity too
        n_units = tmap.total;
    }
    if (n_units == 0u) return;                    // an empty bounce level / no leaf tasks: leave before any set-up (every wave takes this branch)
    const DNode root = nodes[0];
    DCam cam;
    if (PRIMARY) cam = cam_of(camarg);
    DShutter shut;                   // SHUTTER: cam is the camera at shutter open, shut the way to the one at shutter close
    if (PRIMARY && SHUTTER) shut = shutter_of(camarg);
    // primary culling (see k_trace): every stage skips the tiles outside the rectangle -- the units keep their dense numbers, so a skipped
    // tile's ray slots and lit words are simply never written nor read.  (The leaf tasks of a CONT launch come from tiles that were walked.)
    constexpr bool CULL = PRIMARY && !COUNT && !CONT && !LENS && !SHUTTER && !PASS;
    const bool cull = CULL && F.cull != 0;
    CullRect crect{0, 0, 0, 0};
    if (cull) crect = cull_rect(camarg);

    uint32_t c_rays = 0, c_cull = 0, c_centre = 0, c_box = 0, c_ref = 0;
    ShardedQueue q;
    q.init_static(n_units, gridDim.x * RT_WAVES, uniform_u32(blockIdx.x * RT_WAVES + static_cast<uint32_t>(wave)), lane);
    for (uint32_t work = 0; q.next(work);) {
        uint32_t unit = work;
        WalkCtl wc = walk_plain();
        RT_PROF_ADD(lane, WORK_UNITS, 1);
        if (CONT) {
            uint32_t tsh, tloc, tn;
            shard_find(tmap, work, tsh, tloc, tn);
            const ContTask task = Q.tasks_in[tsh * (Q.cap / RT_LIST_SHARDS) + tloc];
            unit = uniform_u32(task.unit);
            wc.resume = true;
            wc.start_node = uniform_u32(task.node);
            wc.start_mask = uniform_u64(task.mask);
            wc.c_begin = uniform_u32(task.c_begin);
            wc.c_end = uniform_u32(task.c_end);
        }
        if (STAGE < 2 && Q.tasks_out != nullptr && Q.budget != 0u) {
            const uint32_t tsh = blockIdx.x & (RT_LIST_SHARDS - 1u), tcap = Q.cap / RT_LIST_SHARDS;      // sharded task queue (Control::n_task_tr)
            wc.budget = Q.budget; wc.unit = unit; wc.tasks = Q.tasks_out + tsh * tcap; wc.task_count = &ctl->n_task_tr[level][Q.q_out & 1u][tsh * 16u]; wc.task_cap = tcap;
            wc.target = Q.target ? Q.target : Q.budget;
        }
        const uint32_t tile = STAGE == 1 ? unit / static_cast<uint32_t>(lslots) : unit;
        const int l = STAGE == 1 ? static_cast<int>(unit - tile * static_cast<uint32_t>(lslots)) : 0;
        if (cull) {
            const int tx = static_cast<int>(tile % static_cast<uint32_t>(F.tiles_x)), ty = static_cast<int>(tile / static_cast<uint32_t>(F.tiles_x));
            if (tile_outside(F, crect, tx, ty)) {
                // no ray, no box test, no record: its pixels are culled pixels (k_resolve stores their colour)
                const int x = tx * 8 + (lane & 7), lr = ty * 8 + (lane >> 3);
                const bool valid = (x < F.width) && (lr < F.local_rows);
                if (STAGE == 0) c_cull += valid ? 1u : 0u;
                if (STAGE == 2 && valid) {
                    const uint32_t pix = static_cast<uint32_t>(lr) * static_cast<uint32_t>(F.width) + static_cast<uint32_t>(x);
                    if (out_hit) out_hit[pix] = -1;
                    if (out_t) out_t[pix] = -1.0f;
                }
                continue;
            }
        }
        const TileRay r = tile_ray<PRIMARY, LENS, SHUTTER, PASS>(tile, lane, F, cam, shut, root, rays_in, rmap);
        const size_t ray_slot = static_cast<size_t>(tile) * 64u + static_cast<size_t>(lane);
        // the packet's cone for the lane = triangle test of its leaves (leaf_visit): common origin (ax, ay, az), box of the targets of the
        // lanes in `on` (exact wave min / max).  Only the leaf-task launches build it: there every unit is a run of 64-triangle chunks of a big
        // leaf (cfg4: closest-hit tasks 0.92 -> 0.68 ms, light-centre tasks 0.55 -> 0.48 ms), while on the walking launches the ~200
        // instructions per tile cost more than the few big leaves they keep inline return (dodge: +7 us on both)
        auto set_cone = [&](const bool on, const float ax, const float ay, const float az, const float tx, const float ty, const float tz, const bool box) {
            float lx = on ? tx : 3e38f, ly = on ? ty : 3e38f, lz = on ? tz : 3e38f, hx_ = on ? tx : -3e38f, hy_ = on ? ty : -3e38f, hz_ = on ? tz : -3e38f;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lx = fminf(lx, __shfl_xor(lx, o, 64)); ly = fminf(ly, __shfl_xor(ly, o, 64)); lz = fminf(lz, __shfl_xor(lz, o, 64));
                hx_ = fmaxf(hx_, __shfl_xor(hx_, o, 64)); hy_ = fmaxf(hy_, __shfl_xor(hy_, o, 64)); hz_ = fmaxf(hz_, __shfl_xor(hz_, o, 64));
            }
            const ShaftLanes SLc = make_shaft_lanes(lane, ax, ay, az, lx, ly, lz, hx_, hy_, hz_, S.extent);
            __builtin_amdgcn_wave_barrier();
            shaft_tri_store(cone_rec, lane, SLc, ax, ay, az, lx, ly, lz, hx_, hy_, hz_);
            __builtin_amdgcn_wave_barrier();
            wc.cone = cone_rec; wc.cone_box = box;
        };

        if (STAGE == 0) {
            // ---- closest hit (flyscene.cpp:655-691)
            bool in_root = r.pre;
            const WalkRay ray = trace_ray(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
            if (!CONT) {
                c_cull += (PRIMARY && r.valid && !r.pre) ? 1u : 0u;
                c_rays += in_root ? 1u : 0u;
                if (COUNT && in_root) c_box += 1;
                in_root = in_root && root_hit(root, ray);
            }
            // (pinhole primary tiles: every ray starts at the camera centre and runs through its screen point o + d.  A LENS tile has 64
            // origins: it builds no cone -- wc.cone stays null, the leaves are tested ray by ray as for bounce rays -- DESIGN.md §5, Depth of field.
            // A SHUTTER tile has 64 cameras, so 64 origins too whenever the camera translates: the same state -- DESIGN.md §5, Motion blur)
            if (CONT && PRIMARY && !LENS && !SHUTTER && !COUNT && __ballot(in_root) != 0ull) set_cone(r.pre, r.ox, r.oy, r.oz, r.ox + r.dx, r.oy + r.dy, r.oz + r.dz, false);
            const Hit h = walk<false, COUNT, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, wc, LanePlane{}, in_root, ray, c_box, c_ref);
            const bool got = found(h.face, S.n_faces);
            const unsigned long long key = got ? ((static_cast<unsigned long long>(__float_as_uint(h.t)) << 32) | static_cast<uint32_t>(h.face))
                                               : RT_NO_HIT_KEY;
            if (CONT) { if (got) atomicMin(&best[ray_slot], key); }
            else best[ray_slot] = key;
        } else {
            const unsigned long long key = best[ray_slot];
            const bool hit = r.valid && key != RT_NO_HIT_KEY;
            const float best_t = __uint_as_float(static_cast<uint32_t>(key >> 32));
            const int best_f = static_cast<int>(static_cast<uint32_t>(key));
            const float hx = r.ox + best_t * r.dx, hy = r.oy + best_t * r.dy, hz = r.oz + best_t * r.dz;   // flyscene.cpp:695
            const int nl_lane = r.lmode ? 1 : L.n_lights;
            if (STAGE == 1) {
                // ---- lightStrikes(hitPoint, lights): the segment to light CENTRE l (flyscene.cpp:700)
                bool act = hit && (l < nl_lane);
                const unsigned long long lit_index = static_cast<unsigned long long>(tile) * static_cast<unsigned long long>(lslots) + static_cast<unsigned long long>(l);
                if (CONT) act = act && (((lit[lit_index] >> lane) & 1ull) != 0ull);     // still believed visible
                if (__ballot(act) == 0ull) {
                    if (!CONT && lane == 0) lit[lit_index] = 0ull;
                    continue;
                }
                float px, py, pz;
                light_point(L, l, r.lmode, r.lx, r.ly, r.lz, px, py, pz);
                const WalkRay ray = segment_ray(px, py, pz, hx, hy, hz);
                bool sroot = act;
                if (!CONT) {
                    c_centre += act ? 1u : 0u;
                    if (COUNT && act) c_box += 1;
                    sroot = act && root_hit(root, ray);
                }
                // (every segment starts at the light: one cone per (tile, light) unless the lanes carry lights of their own)
                if (CONT && !COUNT && __ballot(act && r.lmode != 0u) == 0ull && __ballot(sroot) != 0ull) set_cone(act, L.pos[l][0], L.pos[l][1], L.pos[l][2], hx, hy, hz, true);
                const bool occ = walk<true, COUNT, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, wc, LanePlane{}, sroot, ray, c_box, c_ref);
                if (CONT) {
                    const unsigned long long om = __ballot(act && occ);
                    if (lane == 0 && om != 0ull) atomicAnd(&lit[lit_index], ~om);
                } else {
                    const unsigned long long vm = __ballot(act && !occ);
                    if (lane == 0) lit[lit_index] = vm;
                }
            } else {
                // ---- finish: classification, outputs, compaction of lit hits (wave ballot + prefix, one atomic per wave)
                bool is_lit = false;
                for (int k = 0; k < lslots; ++k) {
                    const unsigned long long w = lit[static_cast<unsigned long long>(tile) * static_cast<unsigned long long>(lslots) + static_cast<unsigned long long>(k)];
                    is_lit = is_lit || (hit && k < nl_lane && ((w >> lane) & 1ull) != 0ull);
                }
                finish_tile(r, hit, is_lit, best_f, best_t, tile, level, lane, F, items, ctl, rec, out_hit, out_t);
            }
        }
    }
    flush_trace_counters<PRIMARY, COUNT>(ctl, lane, level, c_rays, c_cull, c_centre, c_box, c_ref, 0u);
}

// ======================================================================================================
// K2: area-light sample shadow rays (phongShade's lightStrikes(hitPoint, samples), flyscene.cpp:834-836).
// One wave = the N samples of one (hit, light) pair (N = 64), several pairs per wave (N < 64) or
// ceil(N/64) wave passes per pair (N > 64).  Output: one visibility bit per sample.
// ======================================================================================================
// Leaf tasks (tree scenes): leaves whose estimated cost exceeds `budget` are not processed by the walking wave but written
// to `tasks_out` as chunk-range pieces; k_shadow<.., CONT=true> processes them on whichever wave is free and merges the
// occluded bits into `vis` with atomicAnd.  (A first version handed over whole sub-trees once a unit was over budget: the
// pieces were still 979-triangle leaves and the passes ran back to back -- no gain.)

// 97 VGPRs would cost the tree variants their fifth wave per SIMD; asked for 5, the allocator finds them without spilling
#ifndef RT_SHADOW_WPE
#define RT_SHADOW_WPE 5
#endif
template <bool COUNT, bool FLAT, bool CONT>
__global__ __launch_bounds__(RT_WAVES * 64) __attribute__((amdgpu_waves_per_eu(FLAT ? 6 : RT_SHADOW_WPE, 8))) void k_shadow(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                          const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                           const DScene S, const DLights L, const int level, const int ctr_slot,
                                                           const int lslots, const uint32_t item_cap, const ShadeItem *__restrict__ items,
                                                           Control *__restrict__ ctl, unsigned long long *vis, const TaskQueues Q, const uint32_t *__restrict__ sidx) {
    __shared__ uint4 s_stage[1];                                              // k_shadow never stages leaves in LDS (leaf_visit<.., STAGED = false>)
    __shared__ float4 s_fv[(FLAT && !COUNT) ? 64 * 3 : 1];                    // flat scenes: the vertices A, B, C of the root leaf's triangles
    __shared__ unsigned long long s_mask[FLAT ? 1 : RT_WAVES * RT_STACK];     // flat scenes need no stack
    __shared__ uint32_t s_node[FLAT ? 1 : RT_WAVES * RT_STACK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + (FLAT ? 0 : wave * RT_STACK), s_mask + (FLAT ? 0 : wave * RT_STACK), s_stage};
    const uint32_t N = static_cast<uint32_t>(L.n_samples);
    const uint32_t G = N <= 64u ? 64u / N : 1u;              // (hit,light) pairs per wave
    const uint32_t P = (N + 63u) / 64u;                       // 64-sample passes (= mask words) per pair
    // units of list shard s: ceil(cnt_s * lslots / G) (N <= 64) or cnt_s * lslots * P (N > 64), numbered shard after shard
    // (after k_beam: the units are the hits of its compacted survivor list)
    const uint32_t *__restrict__ item_counts = sidx != nullptr ? ctl->n_sitems[level] : ctl->n_items[level];
    const ShardMap imap = N <= 64u ? shard_map(item_counts, lane, item_cap, static_cast<uint32_t>(lslots), G)
                                   : shard_map(item_counts, lane, item_cap, static_cast<uint32_t>(lslots) * P, 1u);
    const unsigned long long units = imap.total;
    if (!CONT && units == 0ull) return;           // an empty bounce level: leave before any set-up (every wave takes this branch)
    const DNode root = nodes[0];
    const uint32_t slot = N <= 64u ? static_cast<uint32_t>(lane) / N : 0u;
    const uint32_t s_in = N <= 64u ? static_cast<uint32_t>(lane) - slot * N : static_cast<uint32_t>(lane);
    const unsigned long long low = low_mask(N);
    // sample grid coordinates of this lane: fixed for the whole kernel when a unit holds all N <= 64 samples
    const uint32_t vst = static_cast<uint32_t>(L.vsteps > 0 ? L.vsteps : 1);
    const float fi_lane = static_cast<float>(s_in / vst) + 0.5f, fj_lane = static_cast<float>(s_in % vst) + 0.5f;
    const float fi_last = static_cast<float>(L.usteps - 1) + 0.5f, fj_last = static_cast<float>(L.vsteps - 1) + 0.5f;
    const bool blocks = sample_blocks(L);

    LanePlane plane{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (FLAT && static_cast<uint32_t>(lane) < (root.count_flags & 0x7fffffffu)) {
        const TriRec *tp = tris + root.first + lane;
        plane = LanePlane{tp->nx, tp->ny, tp->nz, tp->nA, 0.f, 0.f};
    }
    // Flat scenes, one (hit, light) pair per wave: besides the plane rule, the geometric shaft test of the tree scenes, here with
    // lane = (triangle, test) -- 8 triangles x (6 tangent planes + near box) per wave step, ceil(count / 8) steps per unit; the vertices
    // come from LDS (unit-invariant), the margin from the leaf's chunk bound.  cube.obj at 1080p/64: 6.8 -> 0.011 triangle tests per
    // unit (99.8 % of the units keep no triangle at all and leave before a single ray is set up).
    float flat_m = -1.0f;
    if (FLAT && !COUNT) {
        const uint32_t fcnt = root.count_flags & 0x7fffffffu;
        for (uint32_t i = threadIdx.x; i < fcnt && i < 64u; i += blockDim.x) {
            const TriRec t = tris[root.first + i];
            s_fv[3u * i] = make_float4(t.ax, t.ay, t.az, 0.f);
            s_fv[3u * i + 1u] = make_float4(t.ax + t.e1x, t.ay + t.e1y, t.az + t.e1z, 0.f);
            s_fv[3u * i + 2u] = make_float4(t.ax + t.e0x, t.ay + t.e0y, t.az + t.e0z, 0.f);
        }
        __syncthreads();
        const ChunkBound cb0 = chunks[root.pad[0]];
        if (cb0.never < 1.5f && fcnt <= 64u) flat_m = cb0.infl * 1.0625f;
    }
    // (tried on octree leaves too: 25 % fewer ray-mode triangle tests on dodgeColorTest.obj but no whole 64-triangle chunk is ever
    // skipped, and the per-leaf plane pass plus its registers cost more than they saved: 2.31 ms vs 1.93 ms)
    const bool plane_cull = FLAT && !COUNT && G == 1u && S.plane_cull != 0;
    // the lane's sample and the sample box of scene light 0 (see the unit loop)
    const bool scene_light0 = lslots == 1 && N <= 64u;
    float pre_sx = 0.f, pre_sy = 0.f, pre_sz = 0.f, pre_x0 = 0.f, pre_x1 = 0.f, pre_y0 = 0.f, pre_y1 = 0.f, pre_z0 = 0.f, pre_z1 = 0.f;
    if (scene_light0) {
        const LightGrid lg = light_grid(L, L.pos[0][0], L.pos[0][1], L.pos[0][2]);
        grid_sample(lg, fi_lane, fj_lane, pre_sx, pre_sy, pre_sz);
        if (L.mode == RT_LIGHT_SPHERE) sphere_sample(L, s_in, L.pos[0][0], L.pos[0][1], L.pos[0][2], pre_sx, pre_sy, pre_sz);
        light_sample_box(L, lg, L.pos[0][0], L.pos[0][1], L.pos[0][2], 0.5f, 0.5f, fi_last, fj_last, pre_x0, pre_y0, pre_z0, pre_x1, pre_y1, pre_z1);
        if (FLAT) plane_prepare(plane, fminf(pre_x0, pre_x1), fminf(pre_y0, pre_y1), fminf(pre_z0, pre_z1), fmaxf(pre_x0, pre_x1), fmaxf(pre_y0, pre_y1),
                                fmaxf(pre_z0, pre_z1));
    }

    uint32_t c_rays = 0, c_box = 0, c_ref = 0, c_walked = 0;
    ShardedQueue q;
    uint32_t n_work = 0;
    ShardMap tmap{0u, 0u, 0u, 0u};
    if (CONT) {
        tmap = shard_map(ctl->n_task_sh[level], lane, Q.cap / RT_LIST_SHARDS, 1u, 1u);     // producers clamp to the per-shard capacity too
        n_work = tmap.total;
        q.init_static(n_work, gridDim.x * RT_WAVES, uniform_u32(blockIdx.x * RT_WAVES + static_cast<uint32_t>(wave)), lane);
    } else {
        // N > 64: the passes of one (hit, light) pair are consecutive units and walk the same part of the tree -- hand them out two
        // at a time (4K / 256 samples / 1 M triangles: k_shadow 40 -> 32 ms); otherwise balance first (neighbouring heavy units
        // pile up: dodge 1.03 -> 1.9 ms with chunks of 8)
        // (a launch with only a few units per wave -- what k_beam leaves of a flat scene -- would spend its time on the queue heads: one
        // returning atomic per unit and 88 of them per microsecond and head; such a launch is dealt out statically)
        if (FLAT && units < 16ull * gridDim.x * RT_WAVES)
            q.init_static(static_cast<uint32_t>(units), gridDim.x * RT_WAVES, uniform_u32(blockIdx.x * RT_WAVES + static_cast<uint32_t>(wave)), lane);
        else
            q.init(ctl->queue[ctr_slot], static_cast<uint32_t>(units), gridDim.x * RT_WAVES, blockIdx.x, lane,
                   S.queue_local >= 0 ? static_cast<uint32_t>(S.queue_local) : (P > 1u ? 2u : 0u));
    }
    for (uint32_t work = 0; q.next(work);) {
        uint32_t unit = work;
        WalkCtl wc = walk_plain();
        RT_PROF_ADD(lane, WORK_UNITS, 1);
        if (CONT) {
            uint32_t tsh, tloc, tn;
            shard_find(tmap, work, tsh, tloc, tn);
            const ContTask task = Q.tasks_in[tsh * (Q.cap / RT_LIST_SHARDS) + tloc];
            unit = uniform_u32(task.unit);
            wc.resume = true;
            wc.start_node = uniform_u32(task.node);
            wc.start_mask = uniform_u64(task.mask);
            wc.c_begin = uniform_u32(task.c_begin);
            wc.c_end = uniform_u32(task.c_end);
        }
        // leaf tasks only pay when the launch has few units per wave (dodge at 1080p: 41, +5 %); with thousands of units per
        // wave the dynamic queue balances on its own and the second pass is pure overhead (cfg4: 3,600 per wave, 58 vs 46 ms)
        if (!FLAT && Q.tasks_out != nullptr && Q.budget != 0u && units < 256ull * gridDim.x * RT_WAVES) {
            const uint32_t tsh = blockIdx.x & (RT_LIST_SHARDS - 1u), tcap = Q.cap / RT_LIST_SHARDS;      // sharded task queue (Control::n_task_sh)
            wc.budget = Q.budget; wc.unit = unit; wc.tasks = Q.tasks_out + tsh * tcap; wc.task_count = &ctl->n_task_sh[level][tsh * 16u]; wc.task_cap = tcap;
            wc.target = Q.target ? Q.target : Q.budget;
        }
        uint32_t g, s, pass = 0;
        bool valid, slot_ok = false;
        uint32_t sh, lu, n_sh;
        shard_find(imap, unit, sh, lu, n_sh);
        const uint32_t groups = n_sh * static_cast<uint32_t>(lslots);     // (hit, light) pairs of this list shard
        if (N <= 64u) {
            g = lu * G + slot; s = s_in;
            valid = (slot < G) && (g < groups);
            slot_ok = valid;
        } else {
            g = lu / P; pass = lu - g * P; s = pass * 64u + s_in;
            if (blocks) {
                const uint32_t bpr = vst >> 3, bi = pass / bpr, bj = pass - bi * bpr;
                s = (bi * 8u + (s_in >> 3)) * vst + bj * 8u + (s_in & 7u);
            }
            valid = s < N;
        }
        uint32_t item_i = valid ? (lslots == 1 ? g : g / static_cast<uint32_t>(lslots)) : 0u;
        int l = valid ? static_cast<int>(g - item_i * static_cast<uint32_t>(lslots)) : 0;
        uint32_t item_at;
        ShadeItem it;
        if (G == 1u) {
            // one pair per wave: g is the same in every lane, and so is the item -- a wave-uniform index (scalar load).  Every lane, also
            // one past the last sample, then carries the unit's h and light: the triangle lanes of the culling tests rely on that.
            const uint32_t gu = uniform_u32(g);
            item_i = lslots == 1 ? gu : gu / static_cast<uint32_t>(lslots);
            l = static_cast<int>(gu - item_i * static_cast<uint32_t>(lslots));
            item_at = uniform_u32(sh * item_cap + item_i);
            if (sidx != nullptr) item_at = uniform_u32(sidx[item_at]);           // k_beam's survivors: position in the list -> item storage index
            it = items[item_at];
        } else {
            item_at = sh * item_cap + item_i;
            if (sidx != nullptr) item_at = sidx[item_at];
            it = items[item_at];
        }
        g = item_at * static_cast<uint32_t>(lslots) + static_cast<uint32_t>(l);     // (item storage index) * lslots + light: the vis slot
        const int nl = it.lmode ? 1 : L.n_lights;
        valid = valid && (l < nl);
        float hx, hy, hz, px, py, pz;
        hit_point(it, hx, hy, hz);
        light_point(L, l, it.lmode, it.lx, it.ly, it.lz, px, py, pz);
        // Everything that depends on the light alone was computed before the loop for scene light 0; it applies when every lane's
        // item sees the scene lights (level-0 items always do) and there is one of them.
        const bool own_light = scene_light0 ? (__ballot(valid && it.lmode != 0u) != 0ull) : true;
        float sx = pre_sx, sy = pre_sy, sz = pre_sz;
        float x0 = pre_x0, x1 = pre_x1, y0 = pre_y0, y1 = pre_y1, z0 = pre_z0, z1 = pre_z1;
        if (own_light) {
            const LightGrid lg = light_grid(L, px, py, pz);
            if (N <= 64u) grid_sample(lg, fi_lane, fj_lane, sx, sy, sz);
            else grid_sample(lg, static_cast<float>(s / vst) + 0.5f, static_cast<float>(s % vst) + 0.5f, sx, sy, sz);
            if (L.mode == RT_LIGHT_SPHERE) sphere_sample(L, s, px, py, pz, sx, sy, sz);
            light_sample_box(L, lg, px, py, pz, 0.5f, 0.5f, fi_last, fj_last, x0, y0, z0, x1, y1, z1);       // box of this light's sample positions
        }
        const unsigned long long vis_index = N <= 64u ? static_cast<unsigned long long>(g) : static_cast<unsigned long long>(g) * P + pass;
        // the unit's visibility word from the lane mask m of its samples (N <= 64: the first lane of each slot holds its pair's bits):
        // stored, or (and_out, the leaf tasks) its set bits cleared from the word another launch stored
        auto vis_word = [&](const unsigned long long m, const bool and_out) {
            const unsigned long long word = N <= 64u ? (m >> (slot * N)) & low : m;
            if ((N <= 64u ? (s_in == 0u && slot_ok) : lane == 0) && !(and_out && word == 0ull)) {
                if (and_out) atomicAnd(&vis[vis_index], ~word);
                else vis[vis_index] = word;
            }
        };
        if (plane_cull) {
            wc.seg = seg_packet(hx, hy, hz, x0, y0, z0, x1, y1, z1);
            wc.seg.prepared = !own_light;
        }
        if (FLAT && !COUNT && plane_cull && flat_m >= 0.0f) {
            // Which triangles of the (flat) scene can ANY ray of the unit hit?  Known before a single ray is set up: the geometric shaft
            // test (lane = (triangle, test)) and the plane rule (lane = triangle) only need h and the box of the samples.
            const ShaftLanes SLf = make_shaft_lanes(lane, wc.seg.hx, wc.seg.hy, wc.seg.hz, wc.seg.slx, wc.seg.sly, wc.seg.slz, wc.seg.shx, wc.seg.shy, wc.seg.shz, S.extent);
            const int tk = lane & 7;
            const float pax = SLf.r[0] + SLf.r[1], pay = SLf.r[2] + SLf.r[3], paz = SLf.r[4] + SLf.r[5];          // (one addend is zero: exact)
            const float pcm = SLf.r[6] - flat_m * ((fabsf(pax) + fabsf(pay)) + fabsf(paz));
            const uint32_t fcnt = root.count_flags & 0x7fffffffu;
            unsigned long long skip = 0ull;
            for (uint32_t t0 = 0u; t0 < fcnt; t0 += 8u) {
                const uint32_t t = t0 + (static_cast<uint32_t>(lane) >> 3);
                const bool tv = t < fcnt;
                const float4 A = s_fv[3u * (tv ? t : 0u)], B = s_fv[3u * (tv ? t : 0u) + 1u], C = s_fv[3u * (tv ? t : 0u) + 2u];
                const float fa = __builtin_fmaf(pax, A.x, __builtin_fmaf(pay, A.y, paz * A.z));
                const float fb = __builtin_fmaf(pax, B.x, __builtin_fmaf(pay, B.y, paz * B.z));
                const float fc = __builtin_fmaf(pax, C.x, __builtin_fmaf(pay, C.y, paz * C.z));
                const bool p_out = fminf(fminf(fa, fb), fc) + pcm > 0.0f;
                const bool b_out = (fminf(fminf(A.x, B.x), C.x) - flat_m > SLf.r[3]) || (fmaxf(fmaxf(A.x, B.x), C.x) + flat_m < SLf.r[0])
                                || (fminf(fminf(A.y, B.y), C.y) - flat_m > SLf.r[4]) || (fmaxf(fmaxf(A.y, B.y), C.y) + flat_m < SLf.r[1])
                                || (fminf(fminf(A.z, B.z), C.z) - flat_m > SLf.r[5]) || (fmaxf(fmaxf(A.z, B.z), C.z) + flat_m < SLf.r[2]);
                const unsigned long long bo = __ballot(tv && (tk < 6 ? p_out : (tk == 6 && b_out)));
                const unsigned long long m8 = __ballot(lane < 8 && ballot_byte_any(bo, lane)) & 0xffull;
                skip |= m8 << t0;
            }
            skip |= __ballot(wc.seg.prepared ? plane_rules_out_prepared(wc.seg, plane) : plane_rules_out(wc.seg, plane.nx, plane.ny, plane.nz, plane.nA));
            wc.skip = skip;
            RT_PROF_ADD(lane, WORK_TRI_SHAFT_TESTS, 1); RT_PROF_ADD(lane, WORK_TRI_SHAFT_SURVIVORS, __popcll(skip & low_mask(fcnt)));
            if ((low_mask(fcnt) & ~skip) == 0ull) {
                // nothing in the scene can block any ray of this unit: every sample is visible, whatever the root test of its ray says
                c_rays += valid ? 1u : 0u;
                vis_word(__ballot(valid), false);
                continue;
            }
        }
        bool occ = false;
        const WalkRay ray = segment_ray(sx, sy, sz, hx, hy, hz);
        if (FLAT && !CONT) {
            c_rays += valid ? 1u : 0u;
            c_walked += valid ? 1u : 0u;                        // segments actually formed (units the culling devices left before this line formed none)
            if (COUNT && valid) c_box += 1;
            occ = flat_unit_occluded<COUNT>(root, tris, wc.seg, wc.skip, plane, valid, ray, c_box, c_ref);
        } else {
            bool sroot;
            if (CONT) {
                // the root test was passed when the task was emitted (the mask only holds lanes that reached `node`); rays
                // another piece of this unit already found occluded are dropped
                const unsigned long long seen = valid ? vis[vis_index] : 0ull;
                sroot = valid && (((seen >> s_in) & 1ull) != 0ull);
            } else {
                c_rays += valid ? 1u : 0u;
                c_walked += valid ? 1u : 0u;
                if (COUNT && valid) c_box += 1;
                sroot = valid && root_hit(root, ray);
            }
            occ = walk<true, COUNT, FLAT, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, wc, plane, sroot, ray, c_box, c_ref);
        }
        if (CONT) vis_word(__ballot(valid && occ), true);
        else vis_word(__ballot(valid && !occ), false);
    }
    c_rays = wave_sum(c_rays); c_walked = wave_sum(c_walked);
    if (COUNT) { c_box = wave_sum(c_box); c_ref = wave_sum(c_ref); }
    if (lane == 0) {
        if (c_rays) stat_add(ctl, ST_RAYS_SAMPLE, c_rays);
        if (c_walked) stat_add(ctl, ST_SAMPLE_WALKED, c_walked);
        if (COUNT) {
            if (c_box) stat_add(ctl, ST_BOX_TESTS_SHADOW, c_box);
            if (c_ref) stat_add(ctl, ST_LEAF_TRI_REFS_SHADOW, c_ref);
        }
    }
}

// ======================================================================================================
// K2 on TREE scenes with one (hit, light) pair -- or one 64-sample pass of it -- per wave (N >= 33 samples): the shaft walk.
// Same units, same queue and same output words as k_shadow<false, false, false>.
// ======================================================================================================
#ifndef RT_SHAFT_WPE
#define RT_SHAFT_WPE 6
#endif
template <bool CONT, bool TASKS>
__global__ __launch_bounds__(RT_WAVES * 64) __attribute__((amdgpu_waves_per_eu(RT_SHAFT_WPE, 8)))
void k_shadow_shaft(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris, const ChunkBound *__restrict__ chunks,
                    const DScene S, const DLights L, const int level, const int ctr_slot, const int lslots, const uint32_t item_cap,
                    const ShadeItem *__restrict__ items, Control *__restrict__ ctl, unsigned long long *__restrict__ vis, const TaskQueues Q,
                    const uint32_t *__restrict__ sidx) {
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    __shared__ uint4 s_top[CONT ? 1 : RT_LDS_NODES * 4];           // the top of the octree: first RT_LDS_NODES DNodes (breadth-first order)
    __shared__ unsigned long long s_lmask[RT_WAVES * RT_LEAF_SLOTS];
    __shared__ uint32_t s_lnode[RT_WAVES * RT_LEAF_SLOTS];
    __shared__ float4 s_tri[RT_WAVES * RT_SHAFT_TRI_REC];
    __shared__ float4 s_shaft[RT_WAVES * 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, nullptr};
    const uint32_t n_lds = CONT ? 0u : (S.n_nodes < RT_LDS_NODES ? S.n_nodes : RT_LDS_NODES);
    ShaftLds sl{reinterpret_cast<const DNode *>(s_top), n_lds, s_lnode + wave * RT_LEAF_SLOTS, s_lmask + wave * RT_LEAF_SLOTS, s_tri + wave * RT_SHAFT_TRI_REC, s_shaft + wave * 16};
    const uint32_t N = static_cast<uint32_t>(L.n_samples);
    const uint32_t P = (N + 63u) / 64u;                       // 64-sample passes (= mask words) per pair
    const ShardMap imap = shard_map(sidx != nullptr ? ctl->n_sitems[level] : ctl->n_items[level], lane, item_cap, static_cast<uint32_t>(lslots) * P, 1u);
    const uint32_t units = imap.total;
    if (units == 0u) return;                      // an empty bounce level: leave before the LDS copy (every wave of the block takes this branch)
    if (!CONT) {
        const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(nodes);
        for (uint32_t i = threadIdx.x; i < n_lds * 4u; i += blockDim.x) s_top[i] = src[i];
        __syncthreads();
    }
    const uint32_t vst = static_cast<uint32_t>(L.vsteps > 0 ? L.vsteps : 1);
    const bool blocks = sample_blocks(L);
    const float fi_last = static_cast<float>(L.usteps - 1) + 0.5f, fj_last = static_cast<float>(L.vsteps - 1) + 0.5f;
    // Everything that depends on the light alone is evaluated once for scene light 0 (one light, item sees the scene lights: every
    // level-0 item); the lane's grid coordinates inside a pass are lane constants; the two run-time divisions of a unit (pair / pass,
    // block row / column) go through a float reciprocal with an exact correction step instead of the ~30-instruction integer division.
    const LightGrid lg0 = light_grid(L, L.pos[0][0], L.pos[0][1], L.pos[0][2]);
    const uint32_t bpr = blocks ? (vst >> 3) : 1u;
    const float inv_P = 1.0f / static_cast<float>(P), inv_bpr = 1.0f / static_cast<float>(bpr), inv_ls = 1.0f / static_cast<float>(lslots);
    // (a power-of-two divisor -- 256 samples: 4 passes, 2 blocks per row -- is a shift)
    const int sh_P = (P & (P - 1u)) == 0u ? __builtin_ctz(P) : -1, sh_bpr = (bpr & (bpr - 1u)) == 0u ? __builtin_ctz(bpr) : -1;
    const int sh_ls = (static_cast<uint32_t>(lslots) & (static_cast<uint32_t>(lslots) - 1u)) == 0u ? __builtin_ctz(static_cast<uint32_t>(lslots)) : -1;
    auto udiv = [](const uint32_t n, const uint32_t d, const float inv, const int sh) -> uint32_t {
        if (sh >= 0) return n >> sh;
        // float(n) * inv is off by about q * 2^-23 (q = n / d): one correction step each way is exact while q < 2^23; beyond that
        // (a per-shard unit count of a very large frame with many lights and a non-power-of-two pass count) the integer division
        // itself decides -- never a wrong (item, light, pass)
        uint32_t qv = static_cast<uint32_t>(static_cast<float>(n) * inv);
        if (qv * d > n) qv -= 1u;
        if (n - qv * d >= d) qv += 1u;
        if (qv * d > n || n - qv * d >= d) qv = n / d;
        return qv;
    };
    const float fi_lane = blocks ? static_cast<float>(static_cast<uint32_t>(lane) >> 3) : static_cast<float>(static_cast<uint32_t>(lane) / vst);
    const float fj_lane = blocks ? static_cast<float>(static_cast<uint32_t>(lane) & 7u) : static_cast<float>(static_cast<uint32_t>(lane) % vst);
    uint32_t c_rays = 0;
    ShardedQueue q;
    ShardMap tmap{0u, 0u, 0u, 0u};
    if (CONT) {
        // the leaf-task launch: work = the chunk-range tasks the walking launch emitted (sharded queue, Control::n_task_sh)
        tmap = shard_map(ctl->n_task_sh[level], lane, Q.cap / RT_LIST_SHARDS, 1u, 1u);
        q.init_static(tmap.total, gridDim.x * RT_WAVES, uniform_u32(blockIdx.x * RT_WAVES + static_cast<uint32_t>(wave)), lane);
    } else {
        q.init(ctl->queue[ctr_slot], units, gridDim.x * RT_WAVES, blockIdx.x, lane, S.queue_local >= 0 ? static_cast<uint32_t>(S.queue_local) : (P > 1u ? 2u : 0u),
               static_cast<uint32_t>(S.queue_div));
    }
    for (uint32_t work = 0; q.next(work);) {
        RT_PROF_ADD(lane, WORK_UNITS, 1);
        uint32_t unit = work;
        uint32_t t_node = 0u, t_cb = 0u, t_ce = 0u;
        unsigned long long t_mask = 0ull;
        if (CONT) {
            uint32_t tsh, tloc, tn;
            shard_find(tmap, work, tsh, tloc, tn);
            const ContTask task = Q.tasks_in[tsh * (Q.cap / RT_LIST_SHARDS) + tloc];
            unit = uniform_u32(task.unit); t_node = uniform_u32(task.node); t_mask = uniform_u64(task.mask);
            t_cb = uniform_u32(task.c_begin); t_ce = uniform_u32(task.c_end);
        }
        uint32_t sh, lu, n_sh;
        shard_find(imap, unit, sh, lu, n_sh);
        const uint32_t g = P == 1u ? lu : udiv(lu, P, inv_P, sh_P), pass = lu - g * P;                       // (hit, light) pair of the list shard, pass of it
        const uint32_t item_i = lslots == 1 ? g : udiv(g, static_cast<uint32_t>(lslots), inv_ls, sh_ls);
        const int l = static_cast<int>(g - item_i * static_cast<uint32_t>(lslots));
        uint32_t item_at = uniform_u32(sh * item_cap + item_i);
        if (sidx != nullptr) item_at = uniform_u32(sidx[item_at]);            // k_beam's survivors: position in the list -> item storage index
        if (!CONT && Q.pair_done != nullptr) {
            // several lights behind k_pair_beam: the beam of this (hit, light) pair found it unblocked and wrote its words (accounted for there)
            const size_t di = static_cast<size_t>(item_at) * static_cast<size_t>(lslots) + static_cast<size_t>(l);
            const uint32_t dw = reinterpret_cast<const uint32_t *>(Q.pair_done)[di >> 2];          // wave-uniform: a scalar load
            if (((dw >> (8u * static_cast<uint32_t>(di & 3u))) & 0xffu) != 0u) continue;
        }
        const ShadeItem it = items[item_at];                                  // wave-uniform: a scalar load
        uint32_t s = pass * 64u + static_cast<uint32_t>(lane);
        float fi = fi_lane + 0.5f, fj = fj_lane + 0.5f;                       // the lane's sample (i + 0.5, j + 0.5) -- P == 1: s = lane
        float b_i0 = 0.5f, b_j0 = 0.5f, b_i1 = fi_last, b_j1 = fj_last;      // grid corners of the unit's samples (the whole light unless in blocks)
        if (blocks) {
            const uint32_t bi = udiv(pass, bpr, inv_bpr, sh_bpr), bj = pass - bi * bpr;
            s = (bi * 8u + (static_cast<uint32_t>(lane) >> 3)) * vst + bj * 8u + (static_cast<uint32_t>(lane) & 7u);
            b_i0 = static_cast<float>(bi * 8u) + 0.5f; b_j0 = static_cast<float>(bj * 8u) + 0.5f;
            b_i1 = static_cast<float>(bi * 8u + 7u) + 0.5f; b_j1 = static_cast<float>(bj * 8u + 7u) + 0.5f;
            fi = (static_cast<float>(bi * 8u) + fi_lane) + 0.5f; fj = (static_cast<float>(bj * 8u) + fj_lane) + 0.5f;     // exact small integers
        } else if (P > 1u) {
            fi = static_cast<float>(s / vst) + 0.5f; fj = static_cast<float>(s % vst) + 0.5f;
        }
        const int nl = it.lmode ? 1 : L.n_lights;
        const bool valid = s < N && l < nl;
        float hx, hy, hz;
        hit_point(it, hx, hy, hz);
        LightGrid lg = lg0;
        if (it.lmode != 0u || l != 0) {
            float px, py, pz;
            light_point(L, l, it.lmode, it.lx, it.ly, it.lz, px, py, pz);
            lg = light_grid(L, px, py, pz);
        }
        float sx, sy, sz, x0, y0, z0, x1, y1, z1;
        grid_sample(lg, fi, fj, sx, sy, sz);
        // (light_sample_box by hand: with the sphere light's sample and box behind two tests instead of this one, k_shadow_shaft<false, false>
        // takes 80 instead of 68 bytes of scratch and spills 19 instead of 16 VGPRs)
        grid_sample(lg, b_i0, b_j0, x0, y0, z0);             // the samples are monotone in each grid index: two corners give the exact box
        grid_sample(lg, b_i1, b_j1, x1, y1, z1);
        if (L.mode == RT_LIGHT_SPHERE) {
            float px, py, pz;
            light_point(L, l, it.lmode, it.lx, it.ly, it.lz, px, py, pz);
            sphere_sample(L, s, px, py, pz, sx, sy, sz);
            sphere_box(L, px, py, pz, x0, y0, z0, x1, y1, z1);
        }
        const WalkRay ray = segment_ray(sx, sy, sz, hx, hy, hz);
        const unsigned long long vis_index = (static_cast<unsigned long long>(item_at) * static_cast<unsigned long long>(lslots) + static_cast<unsigned long long>(l)) * P + pass;
        if (!CONT) c_rays += static_cast<uint32_t>(__popcll(__ballot(valid)));      // wave-uniform: a scalar register, not a lane counter held (and spilled) across the walk
        ShaftLanes SL = make_shaft_lanes(lane, hx, hy, hz, fminf(x0, x1), fminf(y0, y1), fminf(z0, z1), fmaxf(x0, x1), fmaxf(y0, y1), fmaxf(z0, z1), S.extent, RT_SHAFT_TRUNC);
        __builtin_amdgcn_wave_barrier();
        shaft_tri_store(sl.tri, lane, SL, hx, hy, hz, fminf(x0, x1), fminf(y0, y1), fminf(z0, z1), fmaxf(x0, x1), fmaxf(y0, y1), fmaxf(z0, z1));
        shaft_lanes_store(sl.shaft, lane, SL);
        __builtin_amdgcn_wave_barrier();
        ShaftCtl SC{SL.pad, true};
        SC.node_ok = __ballot(valid && !(fabsf(ray.dx) > 0.0f && fabsf(ray.dy) > 0.0f && fabsf(ray.dz) > 0.0f && fabsf(ray.dx) + fabsf(ray.dy) + fabsf(ray.dz) < 3e38f)) == 0ull;
        const RayLane R = make_ray_lane(ray, S.extent);
        bool occ = false;
        // leaf tasks only pay when the launch has few units per wave (k_shadow has the numbers)
        const bool tasks_on = TASKS && Q.tasks_out != nullptr && Q.budget != 0u && units < 256u * gridDim.x * RT_WAVES;
        const uint32_t tsh = blockIdx.x & (RT_LIST_SHARDS - 1u), tcap = Q.cap / RT_LIST_SHARDS;          // sharded task queue (Control::n_task_sh)
        if (CONT) {
            // one chunk range of one big leaf for the rays that reached it; rays another piece already found occluded are dropped
            const ShaftTasks TQ{nullptr, nullptr, 0u, 0u, 0u, unit};
            const unsigned long long live = t_mask & uniform_u64(vis[vis_index]);
            if (live != 0ull) {
                const DNode leaf = nodes[t_node];
                shaft_leaf<false>(t_node, uniform_u32(leaf.first), uniform_u32(leaf.count_flags) & 0x7fffffffu, uniform_u32(leaf.pad[0]), tris, chunks, lane, R, SC, TQ,
                           sl, t_cb, t_ce, live, occ);
            }
            const unsigned long long om = __ballot(valid && occ);
            if (lane == 0 && om != 0ull) atomicAnd(&vis[vis_index], ~om);
        } else {
            // (the root record comes from the LDS copy of the top of the tree at each use: held in 16 scalar registers for the kernel's lifetime it was
            //  spilled and restored around every unit -- dodge 1.079 -> 1.052 ms, cfg4 26.8 -> 26.2 ms.  Parking the shard map and the lane constants in
            //  LDS as well cut the spilled VGPRs from 14 to 10 and LOST 1.5 %: the unit prologue waits for every extra LDS read)
            const DNode rootl = sl.nodes[0];
            const bool sroot = valid && root_hit(rootl, ray);
            const ShaftTasks TQ{Q.tasks_out + tsh * tcap, &ctl->n_task_sh[level][tsh * 16u], tcap, tasks_on ? Q.budget : 0u, Q.target ? Q.target : Q.budget, unit};
            shaft_walk<TASKS>(nodes, tris, chunks, stk, sl, lane, rootl, sroot, R, SC, TQ, occ);
            const unsigned long long vm = __ballot(valid && !occ);
            if (lane == 0) vis[vis_index] = vm;
        }
    }
    if (lane == 0 && c_rays) {
        stat_add(ctl, ST_RAYS_SAMPLE, c_rays);
        stat_add(ctl, ST_SAMPLE_WALKED, c_rays);     // the shaft walk forms every segment of its units
    }
}

// ======================================================================================================
// K1.5 BEAM TEST -- one wave per tile of 64 consecutive lit hits (a k_shade tile: neighbouring pixels of a primary tile, neighbouring
// bounce rays), before any sample shadow ray is formed.
//
// The sample segments of every hit of the tile to scene light l lie in the BEAM hull(S, H): S the box of the light's samples, H the box
// of the tile's hit points.  With h_c the centre of H and e its half extent, hull(S, h') is contained in hull(S, h_c) + [-e, e] for
// every h' in H (the same parameter on the two segments s -> h' and s -> h_c gives points that differ by at most e per axis), so a box or
// triangle neighbourhood GROWN by e that lies outside the shaft of (S, h_c) is outside the shaft of every hit of the tile.  The shaft
// tests of the unit walk are therefore reused as they are: the lanes' coefficients are built for h_c and then relaxed by e
// (shaft_inflate).  The tree is walked by content box only (a counted hit lies in the content box of every ancestor of its leaf and in
// its chunk box, whatever the reference's own box tests say), chunk bounds, then triangle by triangle; the plane rules take the
// interval of h.n over H (plane_rules_out_box).  If NO triangle of the scene survives, every sample of every hit of the tile sees the
// light: the visibility words are written here and the hits never become shadow units.  One surviving triangle, an uncullable chunk or a
// hit with a light list of its own (mirror bounce) and the items go to the shadow kernels through the compacted index list `sidx`.
// ======================================================================================================
// the decision of plane_rules_out for EVERY (s, h), s in the sample box, h in [hlo, hhi]; m0 as there, over both boxes
__device__ __forceinline__ bool plane_rules_out_box(const float slx, const float sly, const float slz, const float shx, const float shy, const float shz,
                                                    const float hlx, const float hly, const float hlz, const float hhx, const float hhy, const float hhz,
                                                    const float m0, const float nx, const float ny, const float nz, const float nA) {
    const float ax = nx * slx, bx = nx * shx, ay = ny * sly, by = ny * shy, az = nz * slz, bz = nz * shz;
    const float sn_lo = fminf(ax, bx) + (fminf(ay, by) + fminf(az, bz));
    const float sn_hi = fmaxf(ax, bx) + (fmaxf(ay, by) + fmaxf(az, bz));
    const float cx = nx * hlx, dx = nx * hhx, cy = ny * hly, dy = ny * hhy, cz = nz * hlz, dz = nz * hhz;
    const float hn_lo = fminf(cx, dx) + (fminf(cy, dy) + fminf(cz, dz));
    const float hn_hi = fmaxf(cx, dx) + (fmaxf(cy, dy) + fmaxf(cz, dz));
    const float num_lo = nA - sn_hi, num_hi = nA - sn_lo;                 // num = n.A - s.n
    const float dn_lo = hn_lo - sn_hi, dn_hi = hn_hi - sn_lo;             // dn = (h - s).n, s and h independent
    const float M = m0 + 2e-5f * fabsf(nA);
    const bool sane = (fabsf(nx) + fabsf(ny) + fabsf(nz) <= 4.0f) && (fabsf(nA) <= 1e30f);
    const bool opposite = (num_lo > M && dn_hi < -M) || (num_hi < -M && dn_lo > M);
    const float min_abs_num = fmaxf(num_lo, -num_hi);              // <= 0 when the interval straddles zero
    const float max_abs_dn = fmaxf(fabsf(dn_lo), fabsf(dn_hi));
    const bool beyond = (min_abs_num - M) >= 0.981f * (max_abs_dn + M);
    // the same s in both: dn = num + e with e = h.n - n.A, so |e| <= 0.018 |num| puts t = num / dn into [0.982, 1.019] -- not counted
    // (lightStrikes wants t < 0.98).  This is the face the hits lie on and its near-coplanar neighbours, at any light orientation.
    const float e_max = fmaxf(fabsf(hn_lo - nA), fabsf(hn_hi - nA));
    const float a_min = min_abs_num - M;
    const bool near_plane = (a_min > 0.0f) && (e_max + 2.0f * M <= 0.018f * a_min);
    return sane && (num_lo <= num_hi) && (dn_lo <= dn_hi) && (hn_lo <= hn_hi) && (opposite || beyond || near_plane);
}
// relaxes this lane's test by the half extent e of the apex box (see above): a plane value over a box grown by e is lower by
// sum |a_k| e_k; the near box grows by e.  The far tests are not used by beams.
__device__ __forceinline__ void shaft_inflate(ShaftLanes &SL, const int tk, const float ex, const float ey, const float ez) {
    if (tk < 6) {
        const float ax = SL.r[0] + SL.r[1], ay = SL.r[2] + SL.r[3], az = SL.r[4] + SL.r[5];
        SL.r[6] = SL.r[6] - ((fabsf(ax) * ex + fabsf(ay) * ey) + fabsf(az) * ez) * 1.0001f;
    } else if (tk == 6) {
        SL.r[0] -= ex; SL.r[1] -= ey; SL.r[2] -= ez; SL.r[3] += ex; SL.r[4] += ey; SL.r[5] += ez;
    }
}
// ---- lane-local shaft of ONE hit: every lane builds the six tangent planes of its own (S, h) -- the construction of make_shaft_lanes with
// the projection and the tangent as compile-time constants -- and tests wave-uniform boxes against them.  Used by k_beam for the few
// leaves that hold a chunk which may never be culled: can a ray from the light's samples to this hit, or its continuation behind the hit
// (boxIntersect has no upper bound), enter the leaf's own box?  If not, the reference never looks at that leaf for this hit.
struct ItemPlane { float a, b, c, far_margin; };     // a*u + b*v + c over the projection (u, v); unusable: never separates
template <int PROJ, bool Q1>
__device__ __forceinline__ ItemPlane item_plane(const float hx, const float hy, const float hz, const float slx, const float sly, const float slz,
                                                const float shx, const float shy, const float shz, const float scale) {
    const float hu = PROJ == 1 ? hy : hx, hv = PROJ == 2 ? hy : hz;
    const float u0 = PROJ == 1 ? sly : slx, u1 = PROJ == 1 ? shy : shx;
    const float v0 = PROJ == 2 ? sly : slz, v1 = PROJ == 2 ? shy : shz;
    const bool ul = hu < u0, ur = hu > u1, vl = hv < v0, vr = hv > v1;
    const bool su0 = !(ul || ur), sv0 = !(vl || vr);
    const float near_u = ul ? u0 : u1, far_u = ul ? u1 : u0, near_v = vl ? v0 : v1, far_v = vl ? v1 : v0;
    const float cu = Q1 ? (su0 ? u1 : (sv0 ? near_u : far_u)) : (su0 ? u0 : near_u);
    const float cv = Q1 ? (sv0 ? v1 : near_v) : (sv0 ? v0 : (su0 ? near_v : far_v));
    const float mu = 0.5f * (u0 + u1) - hu, mv = 0.5f * (v0 + v1) - hv;
    const float nu = -(cv - hv), nv = cu - hu;
    const float fm = nu * mu + nv * mv;
    const float mag = fabsf(nu) + fabsf(nv);
    const bool ok = !(su0 && sv0) && (fabsf(fm) > 1e-5f * mag * scale);
    const float sgn = fm > 0.0f ? -1.0f : 1.0f;
    const float margin = 2e-5f * mag * scale;
    ItemPlane p;
    p.a = ok ? sgn * nu : 0.0f; p.b = ok ? sgn * nv : 0.0f;
    p.c = ok ? -(p.a * hu + p.b * hv) - margin : -1.0f;
    p.far_margin = ok ? 2.0f * margin : 3e38f;
    return p;
}
// box [lo, hi] (already padded) against one plane: near = outside the shaft by this plane, far = outside the far cone by it
template <int PROJ>
__device__ __forceinline__ void item_plane_test(const ItemPlane &p, const float lx, const float ly, const float lz, const float hx, const float hy, const float hz,
                                                bool &near_out, bool &far_out) {
    const float ul = PROJ == 1 ? ly : lx, uh = PROJ == 1 ? hy : hx, vl = PROJ == 2 ? ly : lz, vh = PROJ == 2 ? hy : hz;
    const float ap = fmaxf(p.a, 0.0f), an = fminf(p.a, 0.0f), bp = fmaxf(p.b, 0.0f), bn = fminf(p.b, 0.0f);
    const float mn = __builtin_fmaf(ap, ul, __builtin_fmaf(an, uh, __builtin_fmaf(bp, vl, __builtin_fmaf(bn, vh, p.c))));
    const float mx = __builtin_fmaf(ap, uh, __builtin_fmaf(an, ul, __builtin_fmaf(bp, vh, __builtin_fmaf(bn, vl, p.c))));
    near_out = near_out || (mn > 0.0f);
    far_out = far_out || (mx + p.far_margin < 0.0f);
}

#ifndef RT_BEAM_BUDGET
#define RT_BEAM_BUDGET 1024               // group steps + chunk bound batches + chunks tested triangle by triangle, per beam
#endif
#ifndef RT_PAIR_WPE
#define RT_PAIR_WPE 6
#endif
#define RT_BEAM_REC 13                 // float4 per wave: shaft_tri_store's 11 (planes, near box, (h_c, m0), S lo, S hi) + H lo, H hi

// lane = triangle: can ANY segment of the beam hit this triangle with a counted t?  (planes and near box from the relaxed record)
__device__ __forceinline__ bool tri_outside_beam(const float4 *rec, const TriRec &tr, const float m) {
    if (tri_outside_cone(rec, tr, m, true)) return true;
    const float4 hm = rec[8], s0 = rec[9], s1 = rec[10], h0 = rec[11], h1 = rec[12];
    return plane_rules_out_box(s0.x, s0.y, s0.z, s1.x, s1.y, s1.z, h0.x, h0.y, h0.z, h1.x, h1.y, h1.z, hm.w, tr.nx, tr.ny, tr.nz, tr.nA);
}

// one leaf against the beam: true = some triangle may be hit (or a chunk that may never be culled is in the way)
__device__ __forceinline__ bool beam_leaf(const uint32_t first, const uint32_t cnt, const uint32_t chunk0, const TriRec *__restrict__ tris,
                                          const ChunkBound *__restrict__ chunks, const int lane, const float4 *shaft, const float4 *rec, const ShaftCtl &SC,
                                          const bool per_item, int &budget) {
    const TriRec *__restrict__ T = tris + first;
    const ChunkBound *__restrict__ cbounds = chunks + chunk0;
    const uint32_t nchunk = (cnt + 63u) >> 6;
    const int tk = lane & 7, tc = lane >> 3;
    for (uint32_t cb0 = 0u; cb0 < nchunk; cb0 += 8u) {
        const uint32_t myc = cb0 + static_cast<uint32_t>(tc);
        const ChunkBound bd = cbounds[myc < nchunk ? myc : cb0];
        const ShaftLanes SL = shaft_lanes_load(shaft, tk, SC);
        bool near_out, far_out;
        shaft_lane_test(SL, tk, bd.lo[0], bd.lo[1], bd.lo[2], bd.hi[0], bd.hi[1], bd.hi[2], near_out, far_out);
        const unsigned long long b_out = __ballot(near_out && bd.never < 1.5f);
        const uint32_t nhere = nchunk - cb0 < 8u ? nchunk - cb0 : 8u;
        unsigned long long cm = __ballot(static_cast<uint32_t>(lane) < nhere && !ballot_byte_any(b_out, lane));      // bit j: chunk cb0 + j is in the beam
        // a chunk that may never be culled: its leaf is tested per hit afterwards (S.bad_leaves) -- or, without that list, it blocks the beam
        const unsigned long long nv = __ballot(static_cast<uint32_t>(lane) < nhere && ((cm >> lane) & 1ull) != 0ull && __shfl(bd.never, 8 * (lane & 7), 64) >= 1.5f);
        if (nv != 0ull && !per_item) return true;
        cm &= ~nv;
        budget -= 1 + static_cast<int>(__popcll(cm));
        RT_PROF_ADD(lane, WORK_BEAM_CHUNK_BATCHES, 1); RT_PROF_ADD(lane, WORK_BEAM_CHUNKS_TESTED_BY_TRIANGLE, __popcll(cm)); if (cb0 == 0u) RT_PROF_ADD(lane, WORK_BEAM_LEAF_VISITS, 1);
        if (budget < 0) return true;                                       // too much work for one wave: let the shadow units decide
        while (cm != 0ull) {
            const int j = static_cast<int>(__builtin_ctzll(cm));
            cm &= cm - 1ull;
            const uint32_t c0 = (cb0 + static_cast<uint32_t>(j)) * 64u;
            const uint32_t k = c0 + static_cast<uint32_t>(lane);
            const TriRec tr = T[k < cnt ? k : 0u];
            const bool hast = k < cnt && !(tr.flags & 1u);                        // (illum 9 faces never occlude: lightStrikes skips them)
            if (__ballot(hast && !tri_outside_beam(rec, tr, lane_f(bd.infl, 8 * j) * 1.0625f)) != 0ull) return true;
        }
    }
    return false;
}

// no sample segment of light (px, py, pz) to the hit h has a zero direction component (0/0 = NaN makes the reference's min/max chain accept any box)
__device__ __forceinline__ bool beam_dirs_ok(const DLights &L, const LightGrid &lg, const uint32_t N, const float px, const float py, const float pz,
                                             const float hx, const float hy, const float hz) {
    bool dirs_ok = fabsf(hx) + fabsf(hy) + fabsf(hz) < 1e30f;
    if (L.mode == RT_LIGHT_SPHERE) {
        for (uint32_t k = 0u; k < N; ++k) {
            float sx, sy, sz;
            sphere_sample(L, k, px, py, pz, sx, sy, sz);
            dirs_ok = dirs_ok && (hx - sx != 0.0f) && (hy - sy != 0.0f) && (hz - sz != 0.0f);
        }
    } else {
        float sx, sy, sz;
        for (int i = 0; i < L.usteps; ++i) { grid_sample(lg, static_cast<float>(i) + 0.5f, 0.5f, sx, sy, sz); dirs_ok = dirs_ok && (hx - sx != 0.0f); }
        for (int j = 0; j < L.vsteps; ++j) { grid_sample(lg, 0.5f, static_cast<float>(j) + 0.5f, sx, sy, sz); dirs_ok = dirs_ok && (hy - sy != 0.0f); }
        dirs_ok = dirs_ok && (hz - sz != 0.0f);
    }
    return dirs_ok;
}

// the same for a wave-uniform hit, the samples spread over the lanes
__device__ __forceinline__ bool beam_dirs_ok_wave(const DLights &L, const LightGrid &lg, const uint32_t N, const float px, const float py, const float pz,
                                                  const float hx, const float hy, const float hz, const int lane) {
    bool bad = !(fabsf(hx) + fabsf(hy) + fabsf(hz) < 1e30f);
    if (L.mode == RT_LIGHT_SPHERE) {
        for (uint32_t k = static_cast<uint32_t>(lane); k < N; k += 64u) {
            float sx, sy, sz;
            sphere_sample(L, k, px, py, pz, sx, sy, sz);
            bad = bad || !((hx - sx != 0.0f) && (hy - sy != 0.0f) && (hz - sz != 0.0f));
        }
    } else {
        float sx, sy, sz;
        for (int i = lane; i < L.usteps; i += 64) { grid_sample(lg, static_cast<float>(i) + 0.5f, 0.5f, sx, sy, sz); bad = bad || !(hx - sx != 0.0f); }
        for (int j = lane; j < L.vsteps; j += 64) { grid_sample(lg, 0.5f, static_cast<float>(j) + 0.5f, sx, sy, sz); bad = bad || !(hy - sy != 0.0f); }
        grid_sample(lg, 0.5f, 0.5f, sx, sy, sz);
        bad = bad || !(hz - sz != 0.0f);
    }
    return __ballot(bad) == 0ull;
}

struct BeamCtx {
    const DNode *nodes; const TriRec *tris; const ChunkBound *chunks;
    uint32_t *stack; float4 *rec; float4 *shaft;           // per-wave LDS
    uint32_t *yield; bool brake, per_item, blocks;
    uint32_t N, P, item_cap; int lslots, level;
    float fi_last, fj_last;
    const DNode *lds_nodes; uint32_t n_lds;                // the top of the tree in LDS (k_pair_beam), or (nullptr, 0)
};
// The walk of one beam: groups of children by content box (and, for a beam with ONE hit, by own box against the shaft and the far cone behind the
// hit: a child outside both is entered by no sample ray -- shaft_walk's rule, with its condition `far_ok`: no ray with a zero / non-finite
// direction component), leaves chunk by chunk, triangle by triangle.  true = something may block a segment of the beam (or the budget ran out).
__device__ __forceinline__ bool beam_walk(const BeamCtx &B, const DScene &S, const DNode &root, const int lane, const ShaftCtl &SC, const bool far_ok, int &budget) {
    const DNode *__restrict__ nodes = B.nodes; const TriRec *__restrict__ tris = B.tris; const ChunkBound *__restrict__ chunks = B.chunks;
    uint32_t *const stack = B.stack; float4 *const rec = B.rec; float4 *const shaft = B.shaft;
    const bool per_item = B.per_item;
    const int tk = lane & 7, tc = lane >> 3;
    bool blocked = false;
    int sp = 0;
    if (root.count_flags & RT_NODE_LEAF) {
        blocked = (root.count_flags & 0x7fffffffu) != 0u &&
                  beam_leaf(uniform_u32(root.first), uniform_u32(root.count_flags) & 0x7fffffffu, uniform_u32(root.pad[0]), tris, chunks, lane, shaft, rec, SC, per_item, budget);
    } else if ((root.count_flags & 0xfu) != 0u) {
        if (lane == 0) stack[0] = root.first | ((root.count_flags & 0xfu) << 28);
        sp = 1;
    }
    while (sp > 0 && !blocked) {
        --sp;
        __builtin_amdgcn_wave_barrier();
        const uint32_t ent = uniform_u32(stack[sp]);
        const uint32_t base = ent & 0x0fffffffu, gcnt = ent >> 28;
        const uint32_t ci = base + (static_cast<uint32_t>(tc) < gcnt ? static_cast<uint32_t>(tc) : 0u);
        DNode ch;
        if (base + gcnt <= B.n_lds) ch = B.lds_nodes[ci];
        else ch = nodes[ci];
        const ShaftLanes SLg = shaft_lanes_load(shaft, tk, SC);
        bool c_near, c_far;
        shaft_lane_test(SLg, tk, ch.clo[0] - SC.pad, ch.clo[1] - SC.pad, ch.clo[2] - SC.pad, ch.chi[0] + SC.pad, ch.chi[1] + SC.pad, ch.chi[2] + SC.pad, c_near, c_far);
        // (per_item: the content box bounds the cullable chunks below; the others are tested per hit afterwards)
        const unsigned long long b_c = __ballot(c_near && (ch.pad[1] == 0u || per_item));
        bool culled = ballot_byte_any(b_c, lane);
        if (far_ok) {
            bool n_near, n_far;
            shaft_lane_test(SLg, tk, ch.bmin[0] - SC.pad, ch.bmin[1] - SC.pad, ch.bmin[2] - SC.pad, ch.bmax[0] + SC.pad, ch.bmax[1] + SC.pad, ch.bmax[2] + SC.pad, n_near, n_far, false);
            const unsigned long long b_nn = __ballot(n_near), b_nf = __ballot(n_far);
            culled = culled || (ballot_byte_any(b_nn, lane) && ballot_byte_any(b_nf, lane));
        }
        unsigned long long surv = __ballot(static_cast<uint32_t>(lane) < gcnt && !culled);
        if (--budget < 0) blocked = true;
        RT_PROF_ADD(lane, WORK_BEAM_GROUP_STEPS, 1); RT_PROF_ADD(lane, WORK_BEAM_CHILDREN_IN_SHAFT, __popcll(surv));
        while (surv != 0ull && !blocked) {
            const int j = static_cast<int>(__builtin_ctzll(surv));
            surv &= surv - 1ull;
            const uint32_t cf = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(ch.count_flags), 8 * j));
            const uint32_t ff = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(ch.first), 8 * j));
            if (cf & RT_NODE_LEAF) {
                const uint32_t lc = cf & 0x7fffffffu;
                if (lc != 0u) blocked = beam_leaf(ff, lc, static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(ch.pad[0]), 8 * j)), tris, chunks, lane, shaft, rec, SC, per_item, budget);
            } else if ((cf & 0xfu) != 0u) {
                if (lane == 0) stack[sp] = ff | ((cf & 0xfu) << 28);
                ++sp;
            }
        }
    }
    return blocked;
}

// k_shadow<.., FLAT>'s unit cull, transposed: lane = HIT, a loop over the root leaf's triangles (vertices A, B, C in `fv`, planes (n, n.A) in
// `fn`, both staged in LDS as k_shadow stages s_fv).  The same tests with the same arithmetic: the tangent planes of make_shaft_lanes (tk =
// 0..5) and its near box (tk = 6) against the vertex boxes [v - m, v + m] (m = flat_m; < 0: no geometric test), then the plane rule on the
// unit's segment packet.  Bit t set: no segment from the light's sample box to h can be blocked by triangle t.
__device__ __forceinline__ unsigned long long flat_hit_cull(const float4 *fv, const float4 *fn, const uint32_t fcnt, const float flat_m, const float extent,
                                                            const SegPacket &seg) {
    float pax[6], pay[6], paz[6], pcm[6];
#pragma unroll
    for (int tk = 0; tk < 6; ++tk) {
        const ShaftLanes SLf = make_shaft_lanes(tk, seg.hx, seg.hy, seg.hz, seg.slx, seg.sly, seg.slz, seg.shx, seg.shy, seg.shz, extent);
        pax[tk] = SLf.r[0] + SLf.r[1]; pay[tk] = SLf.r[2] + SLf.r[3]; paz[tk] = SLf.r[4] + SLf.r[5];          // (one addend is zero: exact)
        pcm[tk] = SLf.r[6] - flat_m * ((fabsf(pax[tk]) + fabsf(pay[tk])) + fabsf(paz[tk]));
    }
    const ShaftLanes SLb = make_shaft_lanes(6, seg.hx, seg.hy, seg.hz, seg.slx, seg.sly, seg.slz, seg.shx, seg.shy, seg.shz, extent);
    unsigned long long skip = 0ull;
    for (uint32_t t = 0u; t < fcnt; ++t) {
        const float4 A = fv[3u * t], B = fv[3u * t + 1u], C = fv[3u * t + 2u];
        bool out = false;
        if (flat_m >= 0.0f) {
#pragma unroll
            for (int tk = 0; tk < 6; ++tk) {
                const float fa = __builtin_fmaf(pax[tk], A.x, __builtin_fmaf(pay[tk], A.y, paz[tk] * A.z));
                const float fb = __builtin_fmaf(pax[tk], B.x, __builtin_fmaf(pay[tk], B.y, paz[tk] * B.z));
                const float fc = __builtin_fmaf(pax[tk], C.x, __builtin_fmaf(pay[tk], C.y, paz[tk] * C.z));
                out = out || (fminf(fminf(fa, fb), fc) + pcm[tk] > 0.0f);
            }
            out = out || (fminf(fminf(A.x, B.x), C.x) - flat_m > SLb.r[3]) || (fmaxf(fmaxf(A.x, B.x), C.x) + flat_m < SLb.r[0])
                      || (fminf(fminf(A.y, B.y), C.y) - flat_m > SLb.r[4]) || (fmaxf(fmaxf(A.y, B.y), C.y) + flat_m < SLb.r[1])
                      || (fminf(fminf(A.z, B.z), C.z) - flat_m > SLb.r[5]) || (fmaxf(fmaxf(A.z, B.z), C.z) + flat_m < SLb.r[2]);
        }
        const float4 n = fn[t];
        out = out || plane_rules_out(seg, n.x, n.y, n.z, n.w);
        skip |= out ? (1ull << t) : 0ull;
    }
    return skip;
}

// (Measured and rejected: running this inside the flat k_trace on the tile's own hits -- no k_beam launch, no second pass over the items.
// The kernel grows from ~90 to 145 VGPRs, its primary launch from 57 to 84 us, and the frame stays at 0.40 ms.)
// One tile of lit hits (lane = hit: `have`, its item storage index, hit point and light mode) through the beam test: writes the visibility
// words of the hits nothing can block, accounts their sample rays, and returns the others (`list`: appends them to the survivor list too).
__device__ __forceinline__ bool beam_tile(const BeamCtx &B, const DScene &S, const DLights &L, const DNode &root, Control *__restrict__ ctl,
                                          unsigned long long *__restrict__ vis, uint32_t *__restrict__ sidx, const int lane, const uint32_t tile,
                                          const bool have, const uint32_t idx, const float hx, const float hy, const float hz, const uint32_t lmode, uint32_t &c_rays,
                                          const bool list = true) {
    float4 *const rec = B.rec; float4 *const shaft = B.shaft; uint32_t *const yield = B.yield;
    const bool brake = B.brake, per_item = B.per_item, blocks = B.blocks;
    const uint32_t N = B.N, P = B.P, item_cap = B.item_cap;
    const int lslots = B.lslots, level = B.level;
    const float fi_last = B.fi_last, fj_last = B.fj_last;
    const int tk = lane & 7;
    const bool scene = have && lmode == 0u;              // sees the scene lights (a mirror bounce carries a light list of its own)
    bool survive = have && !scene;
    const unsigned long long sm0 = __ballot(scene);
    bool give_up = false;
    if (brake) {
        const uint32_t y_t = uniform_u32(__hip_atomic_load(&yield[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const uint32_t y_u = uniform_u32(__hip_atomic_load(&yield[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        give_up = y_t >= 16u && y_u * 4u < y_t;
    }
    if (give_up) survive = have;
    if (sm0 != 0ull && !give_up) {
        // H: exact wave min / max of the hit points
        float lx = scene ? hx : 3e38f, ly = scene ? hy : 3e38f, lz = scene ? hz : 3e38f;
        float ux = scene ? hx : -3e38f, uy = scene ? hy : -3e38f, uz = scene ? hz : -3e38f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lx = fminf(lx, __shfl_xor(lx, o, 64)); ly = fminf(ly, __shfl_xor(ly, o, 64)); lz = fminf(lz, __shfl_xor(lz, o, 64));
            ux = fmaxf(ux, __shfl_xor(ux, o, 64)); uy = fmaxf(uy, __shfl_xor(uy, o, 64)); uz = fmaxf(uz, __shfl_xor(uz, o, 64));
        }
        const float cx = 0.5f * (lx + ux), cy = 0.5f * (ly + uy), cz = 0.5f * (lz + uz);
        // half extent around the ROUNDED centre, rounded up
        const float ex = fmaxf(ux - cx, cx - lx) * 1.0001f + 1e-7f * S.extent, ey = fmaxf(uy - cy, cy - ly) * 1.0001f + 1e-7f * S.extent,
                    ez = fmaxf(uz - cz, cz - lz) * 1.0001f + 1e-7f * S.extent;
        for (int l = 0; l < L.n_lights; ++l) {
            float x0, y0, z0, x1, y1, z1;
            const float px = L.pos[l][0], py = L.pos[l][1], pz = L.pos[l][2];
            const LightGrid lg = light_grid(L, px, py, pz);
            light_sample_box(L, lg, px, py, pz, 0.5f, 0.5f, fi_last, fj_last, x0, y0, z0, x1, y1, z1);
            const float slx = fminf(x0, x1), sly = fminf(y0, y1), slz = fminf(z0, z1), shx = fmaxf(x0, x1), shy = fmaxf(y0, y1), shz = fmaxf(z0, z1);
            ShaftLanes SL = make_shaft_lanes(lane, cx, cy, cz, slx, sly, slz, shx, shy, shz, S.extent);
            shaft_inflate(SL, tk, ex, ey, ez);
            const ShaftCtl SC{SL.pad, false};
            __builtin_amdgcn_wave_barrier();
            shaft_tri_store(rec, lane, SL, cx, cy, cz, slx, sly, slz, shx, shy, shz);
            shaft_lanes_store(shaft, lane, SL);
            if (lane == 8) {
                const float m0 = 2e-5f * (((fabsf(slx) + fabsf(shx)) + (fabsf(sly) + fabsf(shy)) + (fabsf(slz) + fabsf(shz))) +
                                          ((fabsf(lx) + fabsf(ux)) + (fabsf(ly) + fabsf(uy)) + (fabsf(lz) + fabsf(uz))));
                rec[8] = make_float4(cx, cy, cz, m0); rec[11] = make_float4(lx, ly, lz, 0.f); rec[12] = make_float4(ux, uy, uz, 0.f);
            }
            __builtin_amdgcn_wave_barrier();
            int budget = S.beam_budget;
            const bool blocked = beam_walk(B, S, root, lane, SC, false, budget);
            RT_PROF_ADD(lane, WORK_BEAMS_TESTED, 1); RT_PROF_ADD(lane, WORK_BEAMS_UNBLOCKED, blocked ? 0 : 1); RT_PROF_ADD(lane, WORK_BEAM_STEPS_OF_UNBLOCKED, blocked ? 0 : S.beam_budget - budget); RT_PROF_ADD(lane, WORK_BEAMS_OVER_BUDGET, budget < 0 ? 1 : 0);
            if (brake && lane == 0) { atomicAdd(&yield[0], 1u); if (!blocked) atomicAdd(&yield[1], 1u); }
            // the leaves with a chunk that may never be culled (degenerate triangles whose computed barycentrics are noise): can a ray to
            // THIS hit -- or its continuation behind the hit -- enter the leaf's own box?  Lane-local shaft of (S, h): if the padded box is
            // outside the near shaft by one plane AND outside the far cone by one, the reference's boxIntersect fails for every
            // sample ray of the hit by a margin far above its rounding, so that leaf is never looked at for it.  (Not valid with a zero
            // direction component: 0/0 = NaN makes the reference's min/max chain accept -- such hits stay with the shadow units.)
            bool reach = false;
            if (!blocked && per_item && S.n_bad_leaves != 0u) {
                const bool dirs_ok = beam_dirs_ok(L, lg, N, px, py, pz, hx, hy, hz);
                const float big = fmaxf(fmaxf(fabsf(slx), fabsf(shx)), fmaxf(fabsf(sly), fabsf(shy))) + fmaxf(fabsf(slz), fabsf(shz));
                const float scale = S.extent + big + (fabsf(hx) + fabsf(hy) + fabsf(hz));
                const float pad = 4e-4f * ((fmaxf(fabsf(slx), fabsf(shx)) + fmaxf(fabsf(sly), fabsf(shy)) + fmaxf(fabsf(slz), fabsf(shz))) + S.extent) * 1.001f;
                const ItemPlane p0 = item_plane<0, false>(hx, hy, hz, slx, sly, slz, shx, shy, shz, scale), p1 = item_plane<0, true>(hx, hy, hz, slx, sly, slz, shx, shy, shz, scale);
                const ItemPlane p2 = item_plane<1, false>(hx, hy, hz, slx, sly, slz, shx, shy, shz, scale), p3 = item_plane<1, true>(hx, hy, hz, slx, sly, slz, shx, shy, shz, scale);
                const ItemPlane p4 = item_plane<2, false>(hx, hy, hz, slx, sly, slz, shx, shy, shz, scale), p5 = item_plane<2, true>(hx, hy, hz, slx, sly, slz, shx, shy, shz, scale);
                // near box: AABB of hull(S, h); far box: AABB of the far cone { h + tau (h - s) }
                const float nlx = fminf(slx, hx), nly = fminf(sly, hy), nlz = fminf(slz, hz), nhx = fmaxf(shx, hx), nhy = fmaxf(shy, hy), nhz = fmaxf(shz, hz);
                const float flx = hx >= shx ? hx : -3e38f, fly = hy >= shy ? hy : -3e38f, flz = hz >= shz ? hz : -3e38f;
                const float fhx = hx <= slx ? hx : 3e38f, fhy = hy <= sly ? hy : 3e38f, fhz = hz <= slz ? hz : 3e38f;
                for (uint32_t b = 0u; b < S.n_bad_leaves; ++b) {
                    const float *bb = S.bad_leaves + 6u * b;
                    const float lx_ = bb[0] - pad, ly_ = bb[1] - pad, lz_ = bb[2] - pad, hx_ = bb[3] + pad, hy_ = bb[4] + pad, hz_ = bb[5] + pad;
                    bool near_out = (lx_ > nhx) || (hx_ < nlx) || (ly_ > nhy) || (hy_ < nly) || (lz_ > nhz) || (hz_ < nlz);
                    bool far_out = (lx_ > fhx) || (hx_ < flx) || (ly_ > fhy) || (hy_ < fly) || (lz_ > fhz) || (hz_ < flz);
                    item_plane_test<0>(p0, lx_, ly_, lz_, hx_, hy_, hz_, near_out, far_out); item_plane_test<0>(p1, lx_, ly_, lz_, hx_, hy_, hz_, near_out, far_out);
                    item_plane_test<1>(p2, lx_, ly_, lz_, hx_, hy_, hz_, near_out, far_out); item_plane_test<1>(p3, lx_, ly_, lz_, hx_, hy_, hz_, near_out, far_out);
                    item_plane_test<2>(p4, lx_, ly_, lz_, hx_, hy_, hz_, near_out, far_out); item_plane_test<2>(p5, lx_, ly_, lz_, hx_, hy_, hz_, near_out, far_out);
                    reach = reach || !(dirs_ok && near_out && far_out);
                }
                RT_PROF_ADD(lane, WORK_BEAM_BAD_LEAF_CHECKS, __popcll(__ballot(scene))); RT_PROF_ADD(lane, WORK_BEAM_BAD_LEAF_REACHED, __popcll(__ballot(scene && reach)));
            }
            if (blocked) {
                survive = survive || scene;
            } else if (scene && reach) {
                survive = true;
            } else if (scene) {
                // nothing can block any sample segment of these hits to light l: all N samples visible
                const unsigned long long slot0 = (static_cast<unsigned long long>(idx) * static_cast<unsigned long long>(lslots) + static_cast<unsigned long long>(l)) * P;
                for (uint32_t p = 0u; p < P; ++p) {
                    const uint32_t left = N - p * 64u;
                    vis[slot0 + p] = (blocks || left >= 64u) ? ~0ull : ((1ull << left) - 1ull);
                }
            }
        }
    }
    // hits that need no shadow unit at all: their sample rays are accounted for here (the shadow kernels count the others)
    c_rays += (have && !survive) ? N * static_cast<uint32_t>(L.n_lights) : 0u;
    const unsigned long long sm = __ballot(survive);
    if (list && sm != 0ull) {
        bool fits;
        const uint32_t at = shard_reserve(ctl->n_sitems[level], &ctl->overflow, tile, static_cast<uint32_t>(__popcll(sm)), item_cap, lane, fits);
        if (survive && fits) sidx[at + lanes_below(sm)] = idx;
    }
    return survive;
}

// `pend` != nullptr (flat scenes, one visibility word per (hit, light), the k_shadow launch folded away): the hits the tile test cannot clear go
// through flat_hit_cull, lane = hit, light after light.  A (hit, light) pair with every triangle ruled out gets its all-visible word here; any
// other pair gets its triangle SKIP MASK in its visibility word and its bit in the tile's pending word pend[tile * lslots + light], written for
// every tile: k_shade<.., FOLD> walks the pending pairs' sample segments in place and overwrites the skip masks with the visibility.
__global__ __launch_bounds__(RT_WAVES * 64) void k_beam(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris, const ChunkBound *__restrict__ chunks,
                                                        const DScene S, const DLights L, const int level, const int lslots, const uint32_t item_cap,
                                                        const ShadeItem *__restrict__ items, Control *__restrict__ ctl, unsigned long long *__restrict__ vis,
                                                        uint32_t *__restrict__ sidx, unsigned long long *__restrict__ pend, float2 *__restrict__ ltab) {
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    __shared__ float4 s_rec[RT_WAVES * RT_BEAM_REC];
    __shared__ float4 s_shaft[RT_WAVES * 16];
    __shared__ float4 s_fv[64 * 3];                  // fold: the vertices A, B, C of the root leaf's triangles (as k_shadow's s_fv) ...
    __shared__ float4 s_fn[64];                      // ... and their planes (n, n.A)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *const stack = s_node + wave * RT_STACK;
    float4 *const rec = s_rec + wave * RT_BEAM_REC;
    float4 *const shaft = s_shaft + wave * 16;
    const ShardMap imap = shard_map(ctl->n_items[level], lane, item_cap, 1u, 64u);        // tiles of 64 items, shard after shard
    const uint32_t ntiles = imap.total;
    if (ntiles == 0u) return;
    const uint32_t N = static_cast<uint32_t>(L.n_samples);
    const uint32_t P = (N + 63u) / 64u;
    const bool blocks = sample_blocks(L);
    const DNode root = nodes[0];
    const float fi_last = static_cast<float>(L.usteps - 1) + 0.5f, fj_last = static_cast<float>(L.vsteps - 1) + 0.5f;
    const bool per_item = S.n_bad_leaves != 0xffffffffu;
    const bool brake = (root.count_flags & RT_NODE_LEAF) == 0u;      // (a flat scene is one leaf: always cheap to test, nothing to watch)
    uint32_t c_rays = 0;
    const uint32_t wave_id = uniform_u32(blockIdx.x * RT_WAVES + static_cast<uint32_t>(wave)), wave_count = gridDim.x * RT_WAVES;
    // The test only pays where most beams come out unblocked (a convex object, a car body under a light: 85-95 %); under grazing light over
    // a height field 9 in 10 beams meet a triangle, after a long walk.  The launch watches its own yield: every wave reports (tested,
    // unblocked) after each beam into one of 16 counter pairs, and once a pair holds 16 beams with fewer than a quarter unblocked the waves
    // that report to it pass their remaining tiles on untested.  The results do not depend on it -- an untested tile simply goes to the shadow kernels.
    uint32_t *const yield = ctl->beam_yield[level] + (blockIdx.x & (RT_LIST_SHARDS - 1u)) * 16u;      // this workgroup's shard (one returning or
                                                                                                      // non-returning atomic word takes ~88 updates per microsecond)
    const BeamCtx B{nodes, tris, chunks, stack, rec, shaft, yield, brake, per_item, blocks, N, P, item_cap, lslots, level, fi_last, fj_last, nullptr, 0u};
    const bool fold = pend != nullptr;
    const uint32_t fcnt = root.count_flags & 0x7fffffffu;
    float flat_m = -1.0f;
    if (fold) {
#ifndef RT_NO_SAMPLE_TABLE
        // the light-sample table of k_shade<.., FOLD> ("The sample loop: table and layout"): entry [l * RT_LIGHT_TAB_STRIDE + s]
        // = (x, y) of sample s of the scene's light l, by the very operations shade_samples runs per (hit, sample) -- light_grid on the
        // light's position, grid_sample on (s / vsteps + 0.5, s % vsteps + 0.5).  One wave, lane = sample; written by every launch, so no
        // frame and no graph replay reads the table of other lights.
        if (blockIdx.x == 0u && wave == 0 && static_cast<uint32_t>(lane) < N && N <= RT_LIGHT_TAB_STRIDE) {
            const uint32_t vst = static_cast<uint32_t>(L.vsteps > 0 ? L.vsteps : 1);
            const float fi = static_cast<float>(static_cast<uint32_t>(lane) / vst) + 0.5f, fj = static_cast<float>(static_cast<uint32_t>(lane) % vst) + 0.5f;
            for (int l = 0; l < L.n_lights && l < RT_MAX_LIGHTS; ++l) {
                float sx, sy, sz;
                grid_sample(light_grid(L, L.pos[l][0], L.pos[l][1], L.pos[l][2]), fi, fj, sx, sy, sz);
                ltab[static_cast<uint32_t>(l) * RT_LIGHT_TAB_STRIDE + static_cast<uint32_t>(lane)] = make_float2(sx, sy);
            }
        }
#endif
        for (uint32_t i = threadIdx.x; i < fcnt && i < 64u; i += blockDim.x) {
            const TriRec t = tris[root.first + i];
            s_fv[3u * i] = make_float4(t.ax, t.ay, t.az, 0.f);
            s_fv[3u * i + 1u] = make_float4(t.ax + t.e1x, t.ay + t.e1y, t.az + t.e1z, 0.f);
            s_fv[3u * i + 2u] = make_float4(t.ax + t.e0x, t.ay + t.e0y, t.az + t.e0z, 0.f);
            s_fn[i] = make_float4(t.nx, t.ny, t.nz, t.nA);
        }
        __syncthreads();
        const ChunkBound cb0 = chunks[root.pad[0]];
        if (cb0.never < 1.5f && fcnt <= 64u) flat_m = cb0.infl * 1.0625f;
    }
    const unsigned long long low = low_mask(N), fmask = low_mask(fcnt);
    for (uint32_t tile = wave_id; tile < ntiles; tile += wave_count) {
        uint32_t sh, tj, n_sh;
        shard_find(imap, tile, sh, tj, n_sh);
        const bool have = tj * 64u + static_cast<uint32_t>(lane) < n_sh;
        const uint32_t idx = sh * item_cap + tj * 64u + static_cast<uint32_t>(lane);     // item storage index (also keys vis)
        const ShadeItem it = items[have ? idx : sh * item_cap];
        float hx, hy, hz;
        hit_point(it, hx, hy, hz);
        const bool survive = beam_tile(B, S, L, root, ctl, vis, sidx, lane, tile, have, idx, hx, hy, hz, it.lmode, c_rays, !fold);
        if (!fold) continue;
        const int nl = it.lmode ? 1 : L.n_lights;
        for (int l = 0; l < lslots; ++l) {
            const bool act = survive && l < nl;
            bool pending = false;
            if (__ballot(act) != 0ull) {
                // the unit k_shadow would run for (hit, l): h, the box of the light's samples, the plane-rule packet
                float px, py, pz, x0, y0, z0, x1, y1, z1;
                light_point(L, l, it.lmode, it.lx, it.ly, it.lz, px, py, pz);
                const LightGrid lg = light_grid(L, px, py, pz);
                grid_sample(lg, 0.5f, 0.5f, x0, y0, z0);             // (the folded path serves grid lights only)
                grid_sample(lg, fi_last, fj_last, x1, y1, z1);
                const SegPacket seg = seg_packet(hx, hy, hz, x0, y0, z0, x1, y1, z1);
                const unsigned long long skip = flat_hit_cull(s_fv, s_fn, fcnt, flat_m, S.extent, seg);
                const bool clear = (fmask & ~skip) == 0ull;          // nothing in the scene can block any sample segment of the pair
                if (act) vis[static_cast<unsigned long long>(idx) * static_cast<unsigned long long>(lslots) + static_cast<unsigned long long>(l)] = clear ? low : skip;
                c_rays += (act && clear) ? N : 0u;
                pending = act && !clear;
            }
            const unsigned long long pw = __ballot(pending);
            if (lane == 0) pend[static_cast<size_t>(tile) * static_cast<size_t>(lslots) + static_cast<size_t>(l)] = pw;
        }
    }
    c_rays = wave_sum(c_rays);
    if (lane == 0 && c_rays) stat_add(ctl, ST_RAYS_SAMPLE, c_rays);
}

// The beam test at the granularity of ONE lit hit -- tree scenes with more than 64 samples per light, in front of k_shadow_shaft.
// A (hit, light) pair is 2 to 16 shadow units there (one per 64-sample pass), each of which builds its own shaft and walks the top of the tree
// on its own; where nothing at all lies between the hit and the light -- nine units in ten under the 16 x 16 light of the 4K height field, and
// they were half of that kernel's time -- ONE walk with the shaft of the whole light decides all passes at once: the visibility words are
// written here and the pair never becomes a unit.  The apex of the shaft is the hit itself, so (unlike a 64-hit tile, whose apex is a box)
//   * the shaft is the exact hull of the hit and the light's samples plus the rounding margins: the surface around the hit does not block it
//     (the hit's own face and its near-coplanar neighbours are ruled out by plane_rules_out_box's t > 0.981 rule);
//   * the far cone behind the hit is known, so a child whose OWN box lies outside the shaft and outside the far cone is skipped exactly as
//     shaft_walk skips it -- in the reference's over-inclusive tree (clasifyFace tests normalised vectors) the content boxes alone cull
//     almost nothing: 7.5 of 8 children survived per group, 360 steps per beam; with the own-box rule 2.7 of 8 and 11 steps (dodge).
// One wave = one hit at a time, taken from the item list as k_shadow_shaft takes its units (wave-uniform: the item is a scalar load, the hit
// lives in SGPRs): lane = (child, test) in the walk, lane = chunk / triangle in the leaves, lane = leaf in the check against the leaves that
// hold a chunk which may never be culled, lane = pass when the visibility words are written.  A beam is a chain of dependent loads like a
// shadow unit (~2 groups, ~4 leaves with their chunk bounds and triangles), so what counts is how many run at once: everything per hit is
// scalar, the kernel fits the register budget of 6 waves per SIMD.  Hits that may be blocked go to the survivor list of their OWN list
// shard (its capacity holds every item of the shard), 16 at a time through a per-wave LDS buffer.
// The brake is k_beam's: a shard's waves stop testing once it has seen 256 beams with fewer than a quarter unblocked (counters updated
// every 16 beams per wave).
#define RT_PAIR_BUF 16
__global__ __launch_bounds__(RT_WAVES * 64) __attribute__((amdgpu_waves_per_eu(RT_PAIR_WPE, 8)))
void k_pair_beam(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris, const ChunkBound *__restrict__ chunks,
                 const DScene S, const DLights L, const int level, const int lslots, const uint32_t item_cap,
                 const ShadeItem *__restrict__ items, Control *__restrict__ ctl, unsigned long long *__restrict__ vis,
                 uint32_t *__restrict__ sidx, uint8_t *__restrict__ done) {
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    __shared__ float4 s_rec[RT_WAVES * RT_BEAM_REC];
    __shared__ float4 s_shaft[RT_WAVES * 16];
    __shared__ uint4 s_top[RT_LDS_NODES * 4];           // the top of the octree, as in k_shadow_shaft
    __shared__ float s_bad[32 * 6];                     // boxes of the leaves with a chunk that may never be culled (at most 32: rt_scene_image.cpp)
    __shared__ uint32_t s_buf[RT_WAVES * RT_PAIR_BUF];  // survivors waiting for their list reservation
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *const stack = s_node + wave * RT_STACK;
    float4 *const rec = s_rec + wave * RT_BEAM_REC;
    float4 *const shaft = s_shaft + wave * 16;
    uint32_t *const buf = s_buf + wave * RT_PAIR_BUF;
    const ShardMap imap = shard_map(ctl->n_items[level], lane, item_cap, 1u, 1u);
    const uint32_t n_items = imap.total;
    if (n_items == 0u) return;
    const uint32_t n_lds = S.n_nodes < RT_LDS_NODES ? S.n_nodes : RT_LDS_NODES;
    const bool per_item = S.n_bad_leaves != 0xffffffffu;
    const uint32_t n_bad = per_item ? S.n_bad_leaves : 0u;
    {
        const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(nodes);
        for (uint32_t i = threadIdx.x; i < n_lds * 4u; i += blockDim.x) s_top[i] = src[i];
        if (threadIdx.x < n_bad * 6u) s_bad[threadIdx.x] = S.bad_leaves[threadIdx.x];
        __syncthreads();
    }
    const uint32_t N = static_cast<uint32_t>(L.n_samples);
    const uint32_t P = (N + 63u) / 64u;
    const bool blocks = sample_blocks(L);
    const float fi_last = static_cast<float>(L.usteps - 1) + 0.5f, fj_last = static_cast<float>(L.vsteps - 1) + 0.5f;
    uint32_t c_rays = 0;
    const uint32_t wave_id = uniform_u32(blockIdx.x * RT_WAVES + static_cast<uint32_t>(wave)), wave_count = gridDim.x * RT_WAVES;
    uint32_t *const yield = ctl->beam_yield[level] + (blockIdx.x & (RT_LIST_SHARDS - 1u)) * 16u;
    const BeamCtx B{nodes, tris, chunks, stack, rec, shaft, yield, false, per_item, blocks, N, P, item_cap, lslots, level, fi_last, fj_last,
                    reinterpret_cast<const DNode *>(s_top), n_lds};
    const int tk = lane & 7;
    uint32_t n_buf = 0u, buf_shard = 0u;            // survivors in the buffer, all of list shard buf_shard
    uint32_t n_tested = 0u, n_unblocked = 0u, since = 0u;
    bool give_up = false;
    auto flush = [&]() {
        if (n_buf == 0u) return;
        uint32_t base = 0u;
        if (lane == 0) base = atomicAdd(&ctl->n_sitems[level][buf_shard * 16u], n_buf);
        base = uniform_u32(base);
        __builtin_amdgcn_wave_barrier();
        if (static_cast<uint32_t>(lane) < n_buf) {
            if (base + n_buf <= item_cap) sidx[buf_shard * item_cap + base + static_cast<uint32_t>(lane)] = buf[lane];
            else if (lane == 0) atomicOr(&ctl->overflow, 1u);           // (never: the shard's survivors are a subset of its items)
        }
        __builtin_amdgcn_wave_barrier();
        n_buf = 0u;
    };
    for (uint32_t w = wave_id; w < n_items; w += wave_count) {
        uint32_t sh, li, n_sh;
        shard_find(imap, w, sh, li, n_sh);
        const uint32_t idx = uniform_u32(sh * item_cap + li);               // item storage index (also keys vis)
        const ShadeItem it = items[idx];                                    // wave-uniform: a scalar load
        float ax, ay, az;                                                   // the hit
        hit_point(it, ax, ay, az);
        bool survive = it.lmode != 0u || give_up;          // (a mirror bounce carries a light list of its own: straight to the shadow units)
        // Several lights (`done`): a hit blocked from one light is still decided for the others -- every (hit, light) pair gets a byte, 1 = its
        // words are written, and k_shadow_shaft skips the units of such pairs; the sample rays of a decided pair are accounted for here.
        // One light: the first blocked light ends the hit's beams (it becomes a survivor, the unit kernel does all of it).
        uint32_t n_decided = 0u;
        if (done != nullptr && survive && lane < L.n_lights) done[static_cast<size_t>(idx) * static_cast<size_t>(lslots) + static_cast<uint32_t>(lane)] = 0;
        const bool skip_all = survive;
        for (int l = 0; l < L.n_lights && !skip_all && (done != nullptr || !survive); ++l) {
            float x0, y0, z0, x1, y1, z1;
            const float px = L.pos[l][0], py = L.pos[l][1], pz = L.pos[l][2];
            const LightGrid lg = light_grid(L, px, py, pz);
            light_sample_box(L, lg, px, py, pz, 0.5f, 0.5f, fi_last, fj_last, x0, y0, z0, x1, y1, z1);
            const float slx = fminf(x0, x1), sly = fminf(y0, y1), slz = fminf(z0, z1), shx = fmaxf(x0, x1), shy = fmaxf(y0, y1), shz = fmaxf(z0, z1);
            const float e = 1e-7f * S.extent;
            ShaftLanes SL = make_shaft_lanes(lane, ax, ay, az, slx, sly, slz, shx, shy, shz, S.extent, RT_SHAFT_TRUNC);
            shaft_inflate(SL, tk, e, e, e);
            const ShaftCtl SC{SL.pad, false};
            __builtin_amdgcn_wave_barrier();
            shaft_tri_store(rec, lane, SL, ax, ay, az, slx, sly, slz, shx, shy, shz);
            shaft_lanes_store(shaft, lane, SL);
            if (lane == 8) {
                const float m0 = 2e-5f * (((fabsf(slx) + fabsf(shx)) + (fabsf(sly) + fabsf(shy)) + (fabsf(slz) + fabsf(shz))) +
                                          ((fabsf(ax) + fabsf(ax)) + (fabsf(ay) + fabsf(ay)) + (fabsf(az) + fabsf(az))));
                rec[8] = make_float4(ax, ay, az, m0); rec[11] = make_float4(ax, ay, az, 0.f); rec[12] = make_float4(ax, ay, az, 0.f);
            }
            __builtin_amdgcn_wave_barrier();
            const bool dirs_ok = beam_dirs_ok_wave(L, lg, N, px, py, pz, ax, ay, az, lane);
            int budget = S.beam_budget;
            const DNode root = B.lds_nodes[0];
            bool blocked = beam_walk(B, S, root, lane, SC, dirs_ok, budget);
            RT_PROF_ADD(lane, WORK_BEAMS_TESTED, 1); RT_PROF_ADD(lane, WORK_BEAMS_UNBLOCKED, blocked ? 0 : 1); RT_PROF_ADD(lane, WORK_BEAM_STEPS_OF_UNBLOCKED, blocked ? 0 : S.beam_budget - budget); RT_PROF_ADD(lane, WORK_BEAMS_OVER_BUDGET, budget < 0 ? 1 : 0);
            n_tested += 1u; n_unblocked += blocked ? 0u : 1u;
            // the leaves with a chunk that may never be culled (beam_tile has the argument): lane = leaf
            if (!blocked && n_bad != 0u) {
                const float big = fmaxf(fmaxf(fabsf(slx), fabsf(shx)), fmaxf(fabsf(sly), fabsf(shy))) + fmaxf(fabsf(slz), fabsf(shz));
                const float scale = S.extent + big + (fabsf(ax) + fabsf(ay) + fabsf(az));
                const float pad = 4e-4f * ((fmaxf(fabsf(slx), fabsf(shx)) + fmaxf(fabsf(sly), fabsf(shy)) + fmaxf(fabsf(slz), fabsf(shz))) + S.extent) * 1.001f;
                const ItemPlane p0 = item_plane<0, false>(ax, ay, az, slx, sly, slz, shx, shy, shz, scale), p1 = item_plane<0, true>(ax, ay, az, slx, sly, slz, shx, shy, shz, scale);
                const ItemPlane p2 = item_plane<1, false>(ax, ay, az, slx, sly, slz, shx, shy, shz, scale), p3 = item_plane<1, true>(ax, ay, az, slx, sly, slz, shx, shy, shz, scale);
                const ItemPlane p4 = item_plane<2, false>(ax, ay, az, slx, sly, slz, shx, shy, shz, scale), p5 = item_plane<2, true>(ax, ay, az, slx, sly, slz, shx, shy, shz, scale);
                const float nlx = fminf(slx, ax), nly = fminf(sly, ay), nlz = fminf(slz, az), nhx = fmaxf(shx, ax), nhy = fmaxf(shy, ay), nhz = fmaxf(shz, az);
                const float flx = ax >= shx ? ax : -3e38f, fly = ay >= shy ? ay : -3e38f, flz = az >= shz ? az : -3e38f;
                const float fhx = ax <= slx ? ax : 3e38f, fhy = ay <= sly ? ay : 3e38f, fhz = az <= slz ? az : 3e38f;
                const float *bb = s_bad + 6u * (static_cast<uint32_t>(lane) < n_bad ? static_cast<uint32_t>(lane) : 0u);
                const float lx_ = bb[0] - pad, ly_ = bb[1] - pad, lz_ = bb[2] - pad, hx_ = bb[3] + pad, hy_ = bb[4] + pad, hz_ = bb[5] + pad;
                bool near_out = (lx_ > nhx) || (hx_ < nlx) || (ly_ > nhy) || (hy_ < nly) || (lz_ > nhz) || (hz_ < nlz);
                bool far_out = (lx_ > fhx) || (hx_ < flx) || (ly_ > fhy) || (hy_ < fly) || (lz_ > fhz) || (hz_ < flz);
                item_plane_test<0>(p0, lx_, ly_, lz_, hx_, hy_, hz_, near_out, far_out); item_plane_test<0>(p1, lx_, ly_, lz_, hx_, hy_, hz_, near_out, far_out);
                item_plane_test<1>(p2, lx_, ly_, lz_, hx_, hy_, hz_, near_out, far_out); item_plane_test<1>(p3, lx_, ly_, lz_, hx_, hy_, hz_, near_out, far_out);
                item_plane_test<2>(p4, lx_, ly_, lz_, hx_, hy_, hz_, near_out, far_out); item_plane_test<2>(p5, lx_, ly_, lz_, hx_, hy_, hz_, near_out, far_out);
                blocked = __ballot(static_cast<uint32_t>(lane) < n_bad && !(dirs_ok && near_out && far_out)) != 0ull;
                RT_PROF_ADD(lane, WORK_BEAM_BAD_LEAF_CHECKS, 1); RT_PROF_ADD(lane, WORK_BEAM_BAD_LEAF_REACHED, blocked ? 1 : 0);
            }
            if (done != nullptr && lane == 0) done[static_cast<size_t>(idx) * static_cast<size_t>(lslots) + static_cast<uint32_t>(l)] = blocked ? 0 : 1;
            n_decided += blocked ? 0u : 1u;
            if (blocked) {
                survive = true;              // (one light: the words of lights already written stay, the unit kernel rewrites the same values)
            } else if (static_cast<uint32_t>(lane) < P) {
                // nothing can block any sample segment of this hit to light l: all N samples visible (lane = pass)
                const uint32_t left = N - static_cast<uint32_t>(lane) * 64u;
                vis[(static_cast<unsigned long long>(idx) * static_cast<unsigned long long>(lslots) + static_cast<unsigned long long>(l)) * P + static_cast<uint32_t>(lane)] =
                    (blocks || left >= 64u) ? ~0ull : ((1ull << left) - 1ull);
            }
        }
        if (survive) {
            if (n_buf != 0u && buf_shard != sh) flush();
            buf_shard = sh;
            if (lane == 0) buf[n_buf] = idx;
            if (++n_buf == RT_PAIR_BUF) flush();
            if (done != nullptr) c_rays += N * n_decided;            // (the units of the decided pairs will be skipped)
        } else {
            c_rays += N * static_cast<uint32_t>(L.n_lights);        // sample rays that never become a shadow unit are accounted for here (wave-uniform)
        }
        if (++since == 16u && !give_up) {
            since = 0u;
            uint32_t a = 0u, b = 0u;
            if (lane == 0) { a = atomicAdd(&yield[0], n_tested) + n_tested; b = atomicAdd(&yield[1], n_unblocked) + n_unblocked; }
            a = uniform_u32(a); b = uniform_u32(b);
            n_tested = 0u; n_unblocked = 0u;
            give_up = a >= 256u && b * 4u < a;
        }
    }
    flush();
    if (lane == 0 && c_rays) stat_add(ctl, ST_RAYS_SAMPLE, c_rays);
}

// ======================================================================================================
// K3: Phong shading of lit hits + material dispatch + bounce-ray emission with wave-level compaction.
// phongShade flyscene.cpp:822-859, getInterpolatedNormal :864-888, fresnel :890-910, traceRay dispatch :712-760.
// ======================================================================================================
// powf(cosphi, Ns) of phongShade (flyscene.cpp:852).  The reference calls libm's powf: glibc 2.35's e_powf.c (the ARM "optimized
// routines" algorithm: log2 through a 16-entry table + degree-5 polynomial, exp2 through a 32-entry table + degree-3 polynomial, all
// in double) in the build the x86-64 ifunc selects on FMA+AVX2 CPUs.  That published algorithm is evaluated here with the same
// tables, the same operation order and fused multiply-adds at the same places, so the result is the libm result BIT FOR BIT and
// the float accumulators of the frame equal the CPU path's exactly (the tests compare with tolerance 0).
__device__ const double POWF_LOG2_INVC[16] = {0x1.661ec79f8f3bep+0, 0x1.571ed4aaf883dp+0, 0x1.49539f0f010bp+0, 0x1.3c995b0b80385p+0, 0x1.30d190c8864a5p+0,
                                              0x1.25e227b0b8eap+0, 0x1.1bb4a4a1a343fp+0, 0x1.12358f08ae5bap+0, 0x1.0953f419900a7p+0, 0x1p+0,
                                              0x1.e608cfd9a47acp-1, 0x1.ca4b31f026aap-1, 0x1.b2036576afce6p-1, 0x1.9c2d163a1aa2dp-1, 0x1.886e6037841edp-1,
                                              0x1.767dcf5534862p-1};
__device__ const double POWF_LOG2_LOGC[16] = {-0x1.efec65b963019p-2, -0x1.b0b6832d4fca4p-2, -0x1.7418b0a1fb77bp-2, -0x1.39de91a6dcf7bp-2, -0x1.01d9bf3f2b631p-2,
                                              -0x1.97c1d1b3b7afp-3, -0x1.2f9e393af3c9fp-3, -0x1.960cbbf788d5cp-4, -0x1.a6f9db6475fcep-5, 0x0p+0,
                                              0x1.338ca9f24f53dp-4, 0x1.476a9543891bap-3, 0x1.e840b4ac4e4d2p-3, 0x1.40645f0c6651cp-2, 0x1.88e9c2c1b9ff8p-2,
                                              0x1.ce0a44eb17bccp-2};
__device__ const unsigned long long POWF_EXP2_TAB[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull, 0x3fef72b83c7d517bull, 0x3fef54873168b9aaull,
    0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull, 0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
    0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull, 0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull,
    0x3feea11473eb0187ull, 0x3feea589994cce13ull, 0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
    0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull, 0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full,
    0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};

#define RT_POW_TAB 64
// The tables live in LDS for the kernel (64 x 8 B: INVC[16] | LOGC[16] | EXP2_TAB[32]): a lookup is a ds_read_b64, not a global load on the
// critical path of every sample.
// The three polynomial coefficients that are ADDENDS of a v_fmac_f64 (its destination is the addend, so it is copied per sample whatever
// holds it): left to the compiler they sit in six VGPRs across the whole tile loop, which the all-visible copy of the sample loop pays for in
// scratch ("The sample loop's rare cases").  Set from literals next to their use they hold no register between samples: the
// copy per sample becomes two s_mov_b32 + two v_mov_b32 instead of one v_mov_b64.  The value is the same double, bit for bit.
// (make ab AB_FLAGS=-DRT_POW_ADDEND_VGPR: the compiler's own placement, for the A/B.)
template <uint32_t LO, uint32_t HI>
__device__ __forceinline__ double literal_double() {
    uint32_t lo, hi;
    asm("s_mov_b32 %0, %1" : "=s"(lo) : "n"(static_cast<int32_t>(LO)));
    asm("s_mov_b32 %0, %1" : "=s"(hi) : "n"(static_cast<int32_t>(HI)));
    return __longlong_as_double(static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo));
}
#ifdef RT_POW_ADDEND_VGPR
#define RT_ADDEND(x, lo, hi) (x)
#else
#define RT_ADDEND(x, lo, hi) literal_double<lo, hi>()
#endif
// e_powf.c's log2_inline on the bits of a positive normal float: the table step, then the degree-5 polynomial in double
__device__ __forceinline__ double powf_log2_inline(const uint32_t ix, const double *__restrict__ tab) {
    const uint32_t tmp = ix - 0x3f330000u;
    const uint32_t i = (tmp >> 19) & 15u;
    const uint32_t top = tmp & 0xff800000u;
    const int k = static_cast<int>(top) >> 23;
    const double z = static_cast<double>(__uint_as_float(ix - top));
    const double r = __builtin_fma(z, tab[i], -1.0);
    const double y0 = tab[16u + i] + static_cast<double>(k);
    const double r2 = r * r;
    const double yy = __builtin_fma(0x1.27616c9496e0bp-2, r, RT_ADDEND(-0x1.71969a075c67ap-2, 0xa075c67au, 0xbfd71969u));
    const double p = __builtin_fma(0x1.ec70a6ca7baddp-2, r, RT_ADDEND(-0x1.7154748bef6c8p-1, 0x48bef6c8u, 0xbfe71547u));
    const double r4 = r2 * r2;
    double q = __builtin_fma(0x1.71547652ab82bp+0, r, y0);
    q = __builtin_fma(p, r2, q);
    return __builtin_fma(yy, r4, q);
}
// e_powf.c's exp2_inline (sign_bias = 0: the base is never negative here), rounded to float
__device__ __forceinline__ float powf_exp2_inline(const double ylogx, const double *__restrict__ tab) {
    const double shift = 0x1.8p+47;
    double kd = ylogx + shift;
    const unsigned long long ki = static_cast<unsigned long long>(__double_as_longlong(kd));
    kd -= shift;
    const double rr = ylogx - kd;
    const unsigned long long t = static_cast<unsigned long long>(__double_as_longlong(tab[32u + static_cast<uint32_t>(ki & 31ull)])) + (ki << 47);
    const double sc = __longlong_as_double(static_cast<long long>(t));
    const double zz = __builtin_fma(0x1.c6af84b912394p-5, rr, RT_ADDEND(0x1.ebfce50fac4f3p-3, 0x50fac4f3u, 0x3fcebfceu));
    const double rr2 = rr * rr;
    double yv = __builtin_fma(0x1.62e42ff0c52d6p-1, rr, 1.0);
    yv = __builtin_fma(zz, rr2, yv);
    yv = yv * sc;
    return static_cast<float>(yv);
}
// e_powf.c's range test, (asuint64(ylogx) >> 47 & 0xffff) >= asuint64(126.0) >> 47, as one compare: the 16 bits are the exponent and the top
// five mantissa bits, 126.0 has no mantissa bit below those, and the bit pattern of a finite non-negative double grows with its value, so the
// test is |ylogx| >= 126 for every finite value; +-inf and NaN (exponent 0x7ff: above 0x80bf) pass it, and `!(|v| < 126)` is true for them too.
__device__ __forceinline__ bool powf_big(const double ylogx) { return !(__builtin_fabs(ylogx) < 126.0); }
// wave-uniform "some active lane": the predicate's lane mask as the compare leaves it (HIP's __ballot goes through a 0 / 1 select and a
// second compare: two more vector instructions per test, and pow_shininess runs three per sample)
__device__ __forceinline__ bool any_lane(const bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
// |y * log2(x)| >= 126: __math_oflowf / __math_uflowf / __math_may_uflowf, else the ordinary value (also for -149 <= y log2 x <= -126)
__device__ __forceinline__ float powf_range(const float res, const double ylogx, const bool big) {
    const bool r_of = big && (ylogx > 0x1.fffffffd1d571p+6);
    const bool r_uf = big && !r_of && (ylogx <= -150.0);
    const bool r_mu = big && !r_of && !r_uf && (ylogx < -149.0);
    return r_of ? __uint_as_float(0x7f800000u) : (r_uf ? 0.0f : (r_mu ? __uint_as_float(1u) : res));
}
// the GENERAL path: every case e_powf.c answers without arithmetic resolved with selects behind one wave-uniform test, then log2, exp2 and the
// range answers
__device__ __forceinline__ float pow_shininess_general(const float x, const float y_in, const double *__restrict__ tab) {
    const uint32_t ix0 = __float_as_uint(x);
    const float y = y_in;
    const uint32_t iy = __float_as_uint(y);
    const bool y_special = (2u * iy - 1u) >= (2u * 0x7f800000u - 1u);                 // y is 0, inf or NaN
    const bool special = !(ix0 - 0x00800000u < 0x7f800000u - 0x00800000u) || y_special;
    const bool zero_common = (ix0 == 0u) && !y_special && (iy >> 31) == 0u;            // pow(+0, y), y > 0 finite: +0
    uint32_t ix = zero_common ? 0x3f800000u : ix0;
    bool use_spec = false;
    float spec = 0.0f;
    if (any_lane(special && !zero_common)) {
        // e_powf.c's cases without arithmetic, first match wins (x >= 0 or NaN here: cosphi = max(0, .)), then subnormal x
        // (y is the same for every sample of a hit: left alone, its tests below are hoisted out of the caller's sample loop and held there in
        //  five SGPR pairs that this rare block alone reads -- the empty asm keeps them in here)
        uint32_t iy = __float_as_uint(y_in);
        asm volatile("" : "+v"(iy));
        const float y = __uint_as_float(iy);
        const bool odd = special && !zero_common;
        const bool c1 = 2u * iy == 0u;                                                  // pow(x, +-0) = 1
        const bool c2 = x == 1.0f;
        const bool c3 = (x != x) || (y != y);                                           // NaN
        const bool c4 = 2u * iy == 2u * 0x7f800000u;                                    // y = +-inf
        const bool c5 = 2u * ix0 == 0u;                                                 // pow(+-0, y)
        const bool c6 = ix0 == 0x7f800000u;                                             // pow(+inf, y)
        const bool c7 = (ix0 >> 31) != 0u;                                              // negative x: not reachable from phongShade
        const bool yneg = (iy >> 31) != 0u;
        const bool small = 2u * ix0 < 2u * 0x3f800000u;                                // |x| < 1
        const float inf = __uint_as_float(0x7f800000u);
        const float v4 = (small == yneg) ? inf : 0.0f;
        const float v5 = yneg ? inf : 0.0f;
        const float v6 = yneg ? 0.0f : x;
        spec = c1 ? 1.0f : (c2 ? 1.0f : (c3 ? x + y : (c4 ? v4 : (c5 ? v5 : (c6 ? v6 : __uint_as_float(0x7fc00000u))))));
        use_spec = odd && (c1 || c2 || c3 || c4 || c5 || c6 || c7);
        // subnormal x: normalise as e_powf.c does
        uint32_t isub = __float_as_uint(x * 0x1p23f);
        isub &= 0x7fffffffu;
        isub -= 23u << 23;
        ix = use_spec ? 0x3f800000u : ((odd && !use_spec) ? isub : ix);
    }
    const double ylogx = static_cast<double>(y) * powf_log2_inline(ix, tab);
    float res = powf_range(powf_exp2_inline(ylogx, tab), ylogx, powf_big(ylogx));
    res = use_spec ? spec : res;
    return zero_common ? 0.0f : res;
}
// Wave-uniform tests sort the work by how often it is needed ("The sample loop's rare cases").  The LEAN path runs when every
// active lane has a positive finite non-zero y and an x that is +0 or a positive normal -- every sample of the headline.  x = +0 is e_powf.c's
// zero case (the answer is +0: one select; a wave whose lanes are ALL there returns at once, without the double-precision path); the others run
// log2 and exp2, and the three range answers only if some lane's |y log2 x| >= 126.  Anything else in some lane takes the general path.  log2
// and exp2 are the same instructions on both (the helpers above), so a lane's answer does not depend on the path its wave took.  Each test
// feeds one branch and nothing else: that is what lets the compiler branch on the compare's own lane mask.  No divergent branch anywhere.
// (The straight translation -- nine early returns -- cost k_shade ~40 exec-mask branches and three dependent global loads per two
// samples: cube k_shade 0.236 ms.)
__device__ __forceinline__ float pow_shininess(const float x, const float y, const double *__restrict__ tab) {
    const uint32_t ix0 = __float_as_uint(x);
    const uint32_t iy = __float_as_uint(y);
    const bool y_plain = (2u * iy - 1u) < (2u * 0x7f800000u - 1u) && (iy >> 31) == 0u;     // not 0, inf or NaN, and positive
    // (y is the same for every sample of a hit, so y_plain reaches the sample loop as a hoisted lane mask; folded into the VALUE that is
    //  tested, the wave-uniform test stays two compares of this block -- a mask combined with the hoisted one costs a select and a compare more)
    const uint32_t t = y_plain ? ix0 : 0xffffffffu;
    const bool x_zero = t == 0u;
    if (RT_SELDOM(any_lane(!x_zero && !(t - 0x00800000u < 0x7f800000u - 0x00800000u)))) return pow_shininess_general(x, y, tab);
    if (!any_lane(!x_zero)) return 0.0f;                                               // pow(+0, y), y > 0 finite: +0 in every lane
    const double ylogx = static_cast<double>(y) * powf_log2_inline(x_zero ? 0x3f800000u : ix0, tab);
    const bool big = powf_big(ylogx);
    float res = powf_exp2_inline(ylogx, tab);
    if (RT_UNLIKELY(any_lane(big))) res = powf_range(res, ylogx, big);
    return x_zero ? 0.0f : res;
}

__device__ __forceinline__ float fresnel_term(float ix, float iy, float iz, float nx, float ny, float nz, float ior) {
    float cosi = dot3(ix, iy, iz, nx, ny, nz);
    float etai = 1, etat = ior;
    if (cosi > 0) { const float tmp = etai; etai = etat; etat = tmp; }
    const float sint = etai / etat * sqrtf(smax(0.f, 1 - cosi * cosi));
    if (sint >= 1) return 1;
    const float cost = sqrtf(smax(0.f, 1 - sint * sint));
    cosi = fabsf(cosi);
    const float Rs = ((etat * cosi) - (etai * cost)) / ((etat * cosi) + (etai * cost));
    const float Rp = ((etai * cosi) - (etat * cost)) / ((etai * cosi) + (etat * cost));
    return (Rs * Rs + Rp * Rp) / 2;
}

// waves per SIMD: 3 (149 VGPRs) -> 4 (128) was -7 % on the 576k-item cube frame in round 1; 4 -> 5 (96 VGPRs, 20 B of scratch) is another -4 % now that
// the sample loop is leaner (round 3, same-box A/B: k_shade 0.192 -> 0.185 ms).  (The powf coefficients stay literals: kept in LDS they are
// hoisted into 24 VGPRs, which is +1 % at four waves and 112 B of scratch at five.)
#ifndef RT_SHADE_WPE
#define RT_SHADE_WPE 5
#endif
#define RT_SHADE_ATTR __attribute__((amdgpu_waves_per_eu(RT_SHADE_WPE, 8)))
// The two parts of k_shade's table loop by rows and columns ("The sample loop: rows and columns"), each with its A/B switch:
// make ab AB_FLAGS=-DRT_NO_SHADE_ROWS compiles the row loop out (the hoisted test then serves the loop by samples), -DRT_NO_HOISTED_TEST the
// range test in front of the loop (the row loop then tests per sample).
#ifdef RT_NO_SHADE_ROWS
constexpr bool RT_SHADE_ROWS = false;
#else
constexpr bool RT_SHADE_ROWS = true;
#endif
#ifdef RT_NO_HOISTED_TEST
constexpr bool RT_HOISTED_TEST = false;
#else
constexpr bool RT_HOISTED_TEST = true;
#endif
// ---- phongShade / getInterpolatedNormal / the material dispatch of traceRay, shared by k_shade (visibility words from the shadow kernels) and
// k_deep (the deep bounce levels of flat scenes, visibility computed in place).  Every function keeps the reference's operation order.
struct ShadeHit {
    float hx, hy, hz;            // hitPoint = origin + t * direction (flyscene.cpp:695)
    float nx, ny, nz;            // (modelMatrix * interpolated normal).normalized()
    float ex, ey, ez;            // eyeToHitPoint
    float fnx, fny, fnz;         // face normal
    rt_material mat;
};
__device__ __forceinline__ ShadeHit shade_hit(const DScene &S, const int face, const float ox, const float oy, const float oz, const float dx, const float dy,
                                              const float dz, const float t) {
    ShadeHit H;
    const float hx = ox + t * dx, hy = oy + t * dy, hz = oz + t * dz;
    const float *tv = S.tri_verts + static_cast<size_t>(face) * 9;
    const float Ax = tv[0], Ay = tv[1], Az = tv[2], Bx = tv[3], By = tv[4], Bz = tv[5], Cx = tv[6], Cy = tv[7], Cz = tv[8];
    const uint32_t ia = S.tri_vid[face * 3], ib = S.tri_vid[face * 3 + 1], ic = S.tri_vid[face * 3 + 2];
    const float *nA = S.vert_normal + static_cast<size_t>(ia) * 3, *nB = S.vert_normal + static_cast<size_t>(ib) * 3,
                *nC = S.vert_normal + static_cast<size_t>(ic) * 3;
    H.mat = S.mats[S.mat_id[face]];
    H.fnx = S.face_normal[face * 3]; H.fny = S.face_normal[face * 3 + 1]; H.fnz = S.face_normal[face * 3 + 2];
    // getInterpolatedNormal (flyscene.cpp:864-888)
    const float v0x = Bx - Ax, v0y = By - Ay, v0z = Bz - Az;
    const float v1x = Cx - Ax, v1y = Cy - Ay, v1z = Cz - Az;
    const float v2x = hx - Ax, v2y = hy - Ay, v2z = hz - Az;
    const float d00 = dot3(v0x, v0y, v0z, v0x, v0y, v0z), d01 = dot3(v0x, v0y, v0z, v1x, v1y, v1z);
    const float d11 = dot3(v1x, v1y, v1z, v1x, v1y, v1z);
    const float d20 = dot3(v2x, v2y, v2z, v0x, v0y, v0z), d21 = dot3(v2x, v2y, v2z, v1x, v1y, v1z);
    const float denom = d00 * d11 - d01 * d01;
    const float bv = (d11 * d20 - d01 * d21) / denom;
    const float bw = (d00 * d21 - d01 * d20) / denom;
    const float bu = 1.0f - bv - bw;
    const float inx = (bu * nA[0] + bv * nB[0]) + bw * nC[0];
    const float iny = (bu * nA[1] + bv * nB[1]) + bw * nC[1];
    const float inz = (bu * nA[2] + bv * nB[2]) + bw * nC[2];
    // mesh.getModelMatrix() * n: Affine * Vector3f adds the translation (flyscene.cpp:829)
    const float *M = S.model;
    float nx = ((M[0] * inx + M[1] * iny) + M[2] * inz) + M[3] * 1.0f;
    float ny = ((M[4] * inx + M[5] * iny) + M[6] * inz) + M[7] * 1.0f;
    float nz = ((M[8] * inx + M[9] * iny) + M[10] * inz) + M[11] * 1.0f;
    normalize3(nx, ny, nz);
    // eyeToHitPoint = (-1 * (hitPoint - origin)).normalized(): invariant over samples
    float ex = -1.0f * (hx - ox), ey = -1.0f * (hy - oy), ez = -1.0f * (hz - oz);
    normalize3(ex, ey, ez);
    H.hx = hx; H.hy = hy; H.hz = hz; H.nx = nx; H.ny = ny; H.nz = nz; H.ex = ex; H.ey = ey; H.ez = ez;
    return H;
}
// the diffuse + specular term of ONE light sample at (sx, sy, sz) (flyscene.cpp:838-853), colour x material factors passed in.
// ldn = lightDirection . normal, cosphi and pw = powf(cosphi, Ns) are handed back for the probe (k_phong_probe); the shading kernels drop them.
// (this form: from the light vector (ldx, ldy, ldz) = sample - hitPoint.  NORM 0: q, its squared length, is formed here; 1: the caller formed it as
//  normalize3_shared does; 2: and light_dirs_in_range passed for the wave, TESTED there)
template <int NORM>
__device__ __forceinline__ void phong_sample_dir(const ShadeHit &H, const float q, float ldx, float ldy, float ldz, const float lkd0, const float lkd1, const float lkd2,
                                                 const float lks0, const float lks1, const float lks2, const double *__restrict__ tab, float &tr_, float &tg_, float &tb_,
                                                 float &ldn, float &cosphi, float &pw) {
    if constexpr (NORM == 0) normalize3_shared(ldx, ldy, ldz);
    else normalize3_shared<NORM == 2>(q, ldx, ldy, ldz);
    ldn = dot3(ldx, ldy, ldz, H.nx, H.ny, H.nz);
    const float costheta = smax(0.0f, ldn);
    const float two = 2 * ldn;
    float rx = ldx - two * H.nx, ry = ldy - two * H.ny, rz = ldz - two * H.nz;
    normalize3_shared(rx, ry, rz);
    cosphi = smax(0.0f, dot3(H.ex, H.ey, H.ez, -1.0f * rx, -1.0f * ry, -1.0f * rz));
    // (the eye on the far side of the reflected ray for EVERY hit of the wave -- powf(+0, Ns) = +0 without the double-precision path -- is
    //  the first exit of pow_shininess's lean path)
    pw = pow_shininess(cosphi, H.mat.shininess, tab);
    tr_ = lkd0 * costheta + lks0 * pw; tg_ = lkd1 * costheta + lks1 * pw; tb_ = lkd2 * costheta + lks2 * pw;
}
__device__ __forceinline__ void phong_sample(const ShadeHit &H, const float sx, const float sy, const float sz, const float lkd0, const float lkd1, const float lkd2,
                                             const float lks0, const float lks1, const float lks2, const double *__restrict__ tab, float &tr_, float &tg_, float &tb_,
                                             float &ldn, float &cosphi, float &pw) {
    const float ldx = sx - H.hx, ldy = sy - H.hy, ldz = sz - H.hz;
    phong_sample_dir<0>(H, 0.0f, ldx, ldy, ldz, lkd0, lkd1, lkd2, lks0, lks1, lks2, tab, tr_, tg_, tb_, ldn, cosphi, pw);
}
__device__ __forceinline__ void phong_sample(const ShadeHit &H, const float sx, const float sy, const float sz, const float lkd0, const float lkd1, const float lkd2,
                                             const float lks0, const float lks1, const float lks2, const double *__restrict__ tab, float &tr_, float &tg_, float &tb_) {
    float ldn, cosphi, pw;
    phong_sample(H, sx, sy, sz, lkd0, lkd1, lkd2, lks0, lks1, lks2, tab, tr_, tg_, tb_, ldn, cosphi, pw);
}
// material dispatch of traceRay (flyscene.cpp:712-760); a hit at level == max_depth is plain Phong (extension).  Returns the blend kind; for
// kinds other than KIND_CONST `child` is the spawned ray (origin, pix filled by the caller); illum 5 stores its Fresnel factor.
__device__ __forceinline__ uint32_t material_dispatch(const ShadeHit &H, const bool may_spawn, const float dx, const float dy, const float dz, const float lx, const float ly,
                                                      const float lz, const uint32_t lmode, RayItem &child, float *__restrict__ fres_pix) {
    const int imodel = H.mat.illum;
    uint32_t kind = KIND_CONST;
    if (may_spawn) {
        if (imodel == 9) {
            kind = KIND_PASS;
            child.dx = dx; child.dy = dy; child.dz = dz;
            child.lx = lx; child.ly = ly; child.lz = lz; child.lmode = lmode;
        } else if (imodel == 6) {
            kind = KIND_REFRACT;
            const float c1 = fabsf(dot3(dx, dy, dz, H.fnx, H.fny, H.fnz));
            const float inv = 1 / H.mat.optical_density;
            const double p1 = static_cast<double>(inv) * static_cast<double>(inv);     // pow((1/Ni), 2)
            const double p2 = static_cast<double>(c1) * static_cast<double>(c1);       // pow(c1, 2)
            const float c2 = static_cast<float>(sqrt(1 - p1 * (1 - p2)));
            const float k = inv * c1 - c2;
            child.dx = inv * dx + k * H.fnx; child.dy = inv * dy + k * H.fny; child.dz = inv * dz + k * H.fnz;
            child.lx = lx; child.ly = ly; child.lz = lz; child.lmode = lmode;
        } else if (imodel > 2 && imodel < 6) {
            kind = imodel == 5 ? KIND_FRESNEL : KIND_MIRROR;
            const float two = 2 * dot3(dx, dy, dz, H.fnx, H.fny, H.fnz);
            child.dx = dx - two * H.fnx; child.dy = dy - two * H.fny; child.dz = dz - two * H.fnz;
            child.lx = H.hx; child.ly = H.hy; child.lz = H.hz; child.lmode = 1u;             // reflectedLights = {hitPoint}
            if (imodel == 5) *fres_pix = fresnel_term(child.dx, child.dy, child.dz, H.fnx, H.fny, H.fnz, H.mat.optical_density);
        }
    }
    return kind;
}
__device__ __forceinline__ void pow_tables_to_lds(double *s_pow) {
    if (threadIdx.x < RT_POW_TAB) {
        const uint32_t ti = threadIdx.x;
        s_pow[ti] = ti < 16u ? POWF_LOG2_INVC[ti] : (ti < 32u ? POWF_LOG2_LOGC[ti - 16u] : __longlong_as_double(static_cast<long long>(POWF_EXP2_TAB[ti - 32u])));
    }
    __syncthreads();
}

// The sample loop of phongShade for one (hit, light): sum = the number of visible samples, (cr, cg, cb) = the sum of their terms.
// The per-sample term is evaluated for EVERY sample and added as `visible ? term : +0` in sample order -- identical to skipping invisible
// samples (x + 0 == x for the non-negative accumulators) but branch-free.  ALLVIS (SIMPLE lights only): the caller has seen the full mask in
// every active lane's word, so `visible` is a compile-time true: no bit extraction, no selects, and sum = N (the loop would add N ones,
// N <= 64: exact).  One body for both, so the variants cannot drift apart.
// (unrolled by two at five waves per SIMD: 0.185 against 0.1865 ms -- noise; by two or four at four waves: +5 %.  The loop is not waiting on
//  its own dependency chains: what it lacks is issue slots -- FP64 at half rate, v_sqrt / v_rcp at quarter rate)
// TABLE (k_shade<SIMPLE, .., FOLD> only, tiles whose hits are all lit by the scene's lights): the position of sample s comes from k_beam's
// light-sample table instead of grid_sample -- lt points at the light's slot, the address is wave-uniform, so the pair is a scalar load into
// two SGPRs that feed the two subtractions directly.  Sample s + 1 is loaded before the arithmetic of sample s (the index stops at N - 1:
// the last iteration reads its own entry again, never the next slot) and is waited for with the powf tables' LDS reads.
// TESTED (TABLE only; the build without the row loop, -DRT_NO_SHADE_ROWS): light_dirs_in_range passed for the wave.
template <bool SIMPLE, bool ALLVIS, bool TABLE = false, bool TESTED = false>
__device__ __forceinline__ void shade_samples(const ShadeHit &H, const DLights &L, const LightGrid &lg, const unsigned long long *__restrict__ vw,
                                              unsigned long long word, const uint32_t N, const float px, const float py, const float pz, const float lkd0,
                                              const float lkd1, const float lkd2, const float lks0, const float lks1, const float lks2,
                                              const double *__restrict__ s_pow, float &sum, float &cr, float &cg, float &cb,
                                              const float2 *__restrict__ lt = nullptr) {
    static_assert(SIMPLE || !ALLVIS, "the all-visible variant is for one-word lights");
    static_assert(SIMPLE || !TABLE, "the table holds one-word lights");
    static_assert(TABLE || !TESTED, "the hoisted test reads the table");
    float2 ahead = make_float2(0.f, 0.f);
    if (TABLE) ahead = lt[0];
    uint32_t si = 0, sj = 0;                       // s = si * vsteps + sj, kept as counters: no division per sample
    const uint32_t vst = static_cast<uint32_t>(L.vsteps > 0 ? L.vsteps : 1);
    const bool blocks = !SIMPLE && sample_blocks(L);
    const uint32_t bpr = vst >> 3;
    for (uint32_t s = 0; s < N; ++s) {
        uint32_t bit = s & 63u;
        if (!SIMPLE) {
            if (blocks) {
                if ((sj & 7u) == 0u) word = vw[(si >> 3) * bpr + (sj >> 3)];       // a new block every 8 samples of a grid row
                bit = ((si & 7u) << 3) | (sj & 7u);
            } else if (bit == 0u) {
                word = vw[s >> 6];
            }
        }
        const bool visible = ALLVIS || ((word >> bit) & 1ull) != 0ull;
        if (!ALLVIS) sum += visible ? 1.0f : 0.0f;
        float sx, sy, sz;
        if (TABLE) {
            sx = ahead.x; sy = ahead.y; sz = lg.z;
            ahead = lt[s + 1u < N ? s + 1u : s];
        } else {
            grid_sample(lg, static_cast<float>(si) + 0.5f, static_cast<float>(sj) + 0.5f, sx, sy, sz);
            if (!SIMPLE && L.mode == RT_LIGHT_SPHERE) sphere_sample(L, s, px, py, pz, sx, sy, sz);
            if (++sj == vst) { sj = 0; ++si; }
        }
        float tr_, tg_, tb_;
        if (TESTED) {
            const float ldx = sx - H.hx, ldy = sy - H.hy, ldz = sz - H.hz;
            float ldn, cosphi, pw;
            phong_sample_dir<2>(H, ldx * ldx + (ldy * ldy + ldz * ldz), ldx, ldy, ldz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, tr_, tg_, tb_, ldn, cosphi, pw);
        } else {
            phong_sample(H, sx, sy, sz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, tr_, tg_, tb_);
        }
        cr = cr + (visible ? tr_ : 0.0f);
        cg = cg + (visible ? tg_ : 0.0f);
        cb = cb + (visible ? tb_ : 0.0f);
    }
    if (ALLVIS) sum = static_cast<float>(N);
}

// Rows and columns of the light grid ("The sample loop: rows and columns").  grid_sample gives sample s = i * vsteps + j the
// position (fi * cx, fj * cy, z): x belongs to the row, y to the column, z to the light, and a SIMPLE light has N = usteps * vsteps samples
// (a point light: one row, one column), so the table holds usteps distinct x -- entry [i * vsteps].x -- and vsteps distinct y, entry [j].y.
//
// light_dirs_in_range: the range test in front of normalize3_shared's fast body for the light vector of EVERY sample of one (hit, light),
// from the usteps + vsteps + 1 components.  With x_i = sx_i - hx, y_j = sy_j - hy, z = sz - hz the loop's q is
//     q_ij = fl(fl(x_i x_i) + fl(fl(y_j y_j) + fl(z z)))
// fl(x x) does not decrease as |x| grows and fl(a + b) does not decrease as a or b grows (rounding is monotone), so the smallest q_ij is this
// expression at the smallest |x_i| and the smallest |y_j| and the largest is it at the two largest: both are values the loop itself computes
// for some sample.  The smallest |component| over all samples is min(min |x_i|, min |y_j|, |z|).  The three clauses on these values are
// therefore exactly "the per-sample test passes in this lane for every sample", not a bound.  The extremes of |x_i| and |y_j| are taken on
// the bit patterns with the sign cleared (ordered as the values are, and any NaN above every number): a NaN among the x_i is then the
// largest pattern, makes the largest q a NaN and fails `q <= 2^80` as it fails the sample's own test; a NaN z does so through fl(z z).
// Nothing here needs the x_i to be ordered in i.  The entries are read in groups of eight scalar loads (the index of a group's surplus
// members is entry 0's: a repeated member changes no extreme) so their latencies overlap.  Returns the wave-uniform answer over the
// active lanes.
__device__ __forceinline__ bool light_dirs_in_range(const ShadeHit &H, const DLights &L, const float sz, const float2 *__restrict__ lt) {
    const uint32_t ust = static_cast<uint32_t>(L.usteps > 0 ? L.usteps : 1), vst = static_cast<uint32_t>(L.vsteps > 0 ? L.vsteps : 1);
    uint32_t xlo = 0x7fffffffu, xhi = 0u, ylo = 0x7fffffffu, yhi = 0u;
    for (uint32_t k0 = 0; k0 < ust; k0 += 8u) {
        float sx[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) sx[k] = lt[k0 + k < ust ? (k0 + k) * vst : 0u].x;
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const uint32_t a = __float_as_uint(sx[k] - H.hx) & 0x7fffffffu;
            xlo = a < xlo ? a : xlo; xhi = a > xhi ? a : xhi;
        }
    }
    for (uint32_t k0 = 0; k0 < vst; k0 += 8u) {
        float sy[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) sy[k] = lt[k0 + k < vst ? k0 + k : 0u].y;
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const uint32_t a = __float_as_uint(sy[k] - H.hy) & 0x7fffffffu;
            ylo = a < ylo ? a : ylo; yhi = a > yhi ? a : yhi;
        }
    }
    const float z = sz - H.hz, zz = z * z;
    const float x0 = __uint_as_float(xlo), x1 = __uint_as_float(xhi), y0 = __uint_as_float(ylo), y1 = __uint_as_float(yhi);
    const float qlo = x0 * x0 + (y0 * y0 + zz), qhi = x1 * x1 + (y1 * y1 + zz);
    const bool ok = (qlo >= 0x1p-80f) && (qhi <= 0x1p80f) && (fminf(fminf(x0, y0), fabsf(z)) >= 0x1p-60f);     // NaN: false (through qhi)
    return __ballot(!ok) == 0ull;
}

// The table loop by rows: per row i  x_i = sx_i - hx and x_i x_i once, per sample  q = x_i x_i + (y_j y_j + z z)  -- the operations of
// normalize3_shared's q in their order, so every q is the float the loop by samples produces (no contraction in this build) -- and the
// components x_i, y_j, z go to the shared body of phong_sample.  The y of the next sample and the x of the next row are loaded ahead, as
// the table loop loads its pairs.  TESTED: light_dirs_in_range passed for the wave, the light vector is normalised without its test.
template <bool ALLVIS, bool TESTED>
__device__ __forceinline__ void shade_samples_rows(const ShadeHit &H, const DLights &L, const LightGrid &lg, const unsigned long long word, const uint32_t N,
                                                   const float lkd0, const float lkd1, const float lkd2, const float lks0, const float lks1, const float lks2,
                                                   const double *__restrict__ s_pow, float &sum, float &cr, float &cg, float &cb, const float2 *__restrict__ lt) {
    const uint32_t vst = static_cast<uint32_t>(L.vsteps > 0 ? L.vsteps : 1);
    const float ldz = lg.z - H.hz, zz = ldz * ldz;
    float ahead_x = lt[0].x, ahead_y = lt[0].y;
    for (uint32_t s0 = 0; s0 < N; s0 += vst) {
        const float ldx = ahead_x - H.hx, xx = ldx * ldx;
        ahead_x = lt[s0 + vst < N ? s0 + vst : s0].x;
        for (uint32_t j = 0; j < vst; ++j) {
            const bool visible = ALLVIS || ((word >> ((s0 + j) & 63u)) & 1ull) != 0ull;
            if (!ALLVIS) sum += visible ? 1.0f : 0.0f;
            const float ldy = ahead_y - H.hy;
            ahead_y = lt[j + 1u < vst ? j + 1u : 0u].y;          // (the last of a row loads the next row's first)
            float tr_, tg_, tb_, ldn, cosphi, pw;
            phong_sample_dir<TESTED ? 2 : 1>(H, xx + (ldy * ldy + zz), ldx, ldy, ldz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, tr_, tg_, tb_, ldn, cosphi, pw);
            cr = cr + (visible ? tr_ : 0.0f);
            cg = cg + (visible ? tg_ : 0.0f);
            cb = cb + (visible ? tb_ : 0.0f);
        }
    }
    if (ALLVIS) sum = static_cast<float>(N);
}

// SIMPLE: the light is a point or a grid of at most 64 samples (one visibility word per (hit, light), sample s = bit s, no 8 x 8 blocks, no
// sphere offsets) -- the reference's own 5 x 5 and the 8 x 8 headline.  The sample loop then carries no word / block / mode branches.
// FLAT: the scene is one root leaf.  A spawned child ray is then tested against that leaf right here (the closest-hit walk k_trace would run for
// it at the next level: ~45 instructions per triangle for the whole tile); a child that hits nothing gets its BACKGROUND record now and never
// becomes a ray -- on a convex mirror object (cube.obj) that is every child: level 1 stays empty, its 576k-ray k_trace launch (24 us) is gone.
// Children that do hit something go through the wide kernels as before (their walk is repeated there: the exception, not the rule).
// FOLD (SIMPLE lights of flat scenes, no k_shadow launch in front): k_beam left the (hit, light) pairs it could not decide PENDING -- a bit per
// hit in pend[tile * lslots + light], the triangle skip mask in the pair's visibility word.  Before the hits are shaded, the wave takes the
// pending pairs of its tile one at a time, lane = sample, through flat_unit_occluded (k_shadow's unit body), and stores the visibility word.
template <bool SIMPLE, bool FLAT, bool FOLD>
__global__ __launch_bounds__(256) RT_SHADE_ATTR void k_shade(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris, const DScene S, const DLights L, const DFrame F,
                                               const int level, const int ctr_slot,
                                               const int lslots, const ShadeItem *__restrict__ items, Control *__restrict__ ctl,
                                               unsigned long long *vis, float4 *__restrict__ rec,
                                               float *__restrict__ fres, RayItem *__restrict__ rays_out, const unsigned long long *__restrict__ pend,
                                               const float2 *__restrict__ ltab) {
#ifdef RT_NO_SAMPLE_TABLE
    constexpr bool TABLE = false;
#else
    constexpr bool TABLE = SIMPLE && FOLD;     // k_beam wrote the light-sample table in front of this launch
#endif
    __shared__ double s_pow[RT_POW_TAB];       // powf tables: INVC[16] | LOGC[16] | EXP2_TAB[32] (bit patterns)
    const int lane = threadIdx.x & 63;
    const ShardMap imap = shard_map(ctl->n_items[level], lane, F.item_cap, 1u, 64u);      // groups of 64 items, shard after shard
    const uint32_t ntiles = imap.total;
    if (ntiles == 0u) return;                  // an empty level: every wave of every block leaves here, ahead of the tables and their barrier
    pow_tables_to_lds(s_pow);
    const uint32_t N = static_cast<uint32_t>(L.n_samples);
    const uint32_t P = (N + 63u) / 64u;
    uint32_t c_shaded = 0, c_resolved = 0, c_sample = 0;      // per WAVE (scalar registers): every count below is a popcount of a lane mask
    const uint32_t wave_id = uniform_u32(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t wave_count = gridDim.x * 4u;
    DNode root;
    if (FLAT || FOLD) root = nodes[0];
    if (FOLD) {
        // first the pending pairs of all of this wave's tiles (their own loop: nothing of the shading below is live across the walks)
        for (uint32_t tile = wave_id; tile < ntiles; tile += wave_count) {
            uint32_t sh, tj, n_sh;
            shard_find(imap, tile, sh, tj, n_sh);
            const uint32_t at = sh * F.item_cap + tj * 64u + static_cast<uint32_t>(lane);
            bool loaded = false;
            float hx = 0.f, hy = 0.f, hz = 0.f, lx = 0.f, ly = 0.f, lz = 0.f;
            uint32_t lmode = 0u;
            for (int l = 0; l < lslots; ++l) {
                unsigned long long pw = uniform_u64(pend[static_cast<size_t>(tile) * static_cast<size_t>(lslots) + static_cast<size_t>(l)]);
                if (pw == 0ull) continue;
                // the tile's hits and the pending skip masks, one vector load each: the pairs below then read them with v_readlane
                // (no memory round trip between one pair's walk and the next)
                const bool mine = ((pw >> lane) & 1ull) != 0ull;
                if (!loaded) {
                    const ShadeItem it = items[tj * 64u + static_cast<uint32_t>(lane) < n_sh ? at : sh * F.item_cap];
                    hit_point(it, hx, hy, hz);
                    lx = it.lx; ly = it.ly; lz = it.lz; lmode = it.lmode;
                    loaded = true;
                }
                const unsigned long long slot_l = static_cast<unsigned long long>(at) * static_cast<unsigned long long>(lslots) + static_cast<unsigned long long>(l);
                const unsigned long long skip_l = mine ? vis[slot_l] : 0ull;
                const uint32_t vst = static_cast<uint32_t>(L.vsteps > 0 ? L.vsteps : 1);
                const float fi = static_cast<float>(static_cast<uint32_t>(lane) / vst) + 0.5f, fj = static_cast<float>(static_cast<uint32_t>(lane) % vst) + 0.5f;
                const bool s_ok = static_cast<uint32_t>(lane) < N;
                while (pw != 0ull) {
                    const int j = static_cast<int>(__builtin_ctzll(pw));
                    pw &= pw - 1ull;
                    const uint32_t lm = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(lmode), j));
                    const float px = lm ? lane_f(lx, j) : L.pos[l][0], py = lm ? lane_f(ly, j) : L.pos[l][1], pz = lm ? lane_f(lz, j) : L.pos[l][2];
                    const unsigned long long skip = (static_cast<unsigned long long>(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(skip_l >> 32), j))) << 32) |
                                                    static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(skip_l & 0xffffffffull), j));
                    float sx, sy, sz;
                    grid_sample(light_grid(L, px, py, pz), fi, fj, sx, sy, sz);
                    // the skip mask already holds the plane rule of the pair: the walk gets a plane that rules nothing out (|n.A| > 1e30)
                    SegPacket seg = seg_off();
                    seg.on = true;
                    uint32_t cu0 = 0, cu1 = 0;
                    const bool occ = flat_unit_occluded<false>(root, tris, seg, skip, LanePlane{0.f, 0.f, 0.f, 3e38f, 0.f, 0.f}, s_ok,
                                                               segment_ray(sx, sy, sz, lane_f(hx, j), lane_f(hy, j), lane_f(hz, j)), cu0, cu1);
                    const unsigned long long vm = __ballot(s_ok && !occ);
                    if (lane == j) vis[slot_l] = vm;        // (read back by this same lane when it is shaded)
                    c_sample += static_cast<uint32_t>(__popcll(__ballot(s_ok)));
                }
            }
        }
    }
    for (uint32_t tile = wave_id; tile < ntiles; tile += wave_count) {
        uint32_t sh, tj, n_sh;
        shard_find(imap, tile, sh, tj, n_sh);
        const bool valid = tj * 64u + static_cast<uint32_t>(lane) < n_sh;
        const uint32_t idx = sh * F.item_cap + tj * 64u + static_cast<uint32_t>(lane);     // item storage index (also keys vis)
        const ShadeItem it = items[valid ? idx : sh * F.item_cap];
        bool spawn = false;
        RayItem child;
        child.pad = 0u;
        c_shaded += static_cast<uint32_t>(__popcll(__ballot(valid)));
        if (valid) {
            const ShadeHit H = shade_hit(S, it.face, it.ox, it.oy, it.oz, it.dx, it.dy, it.dz, it.t);
            float fr = 0.f, fg = 0.f, fb = 0.f;
            const int nl = it.lmode ? 1 : L.n_lights;
            // TABLE: no hit of the tile carries a light of its own (every level-0 tile; behind a mirror bounce the hits do) -- one wave-uniform
            // test per tile; then the lights are the scene's in every lane, and the sample positions come from the table
            const bool scene_lights = TABLE && __ballot(it.lmode != 0u) == 0ull;
            for (int l = 0; l < nl; ++l) {
                // (light_point by hand: through the helper every k_shade stream moves, <true, true, true> spills 79 instead of 74 SGPRs and the cube
                // frame misses its bound, 0.2466 ms against the parent's 0.2436 -- profiles/walk_rays_ab.json, session 1)
                const float px = it.lmode ? it.lx : L.pos[l][0], py = it.lmode ? it.ly : L.pos[l][1], pz = it.lmode ? it.lz : L.pos[l][2];
                const unsigned long long *vw = vis + (static_cast<unsigned long long>(idx) * static_cast<unsigned long long>(lslots) + static_cast<unsigned long long>(l)) * P;
                float sum = 0.f, cr = 0.f, cg = 0.f, cb = 0.f;
                const float lkd0 = L.color[0] * H.mat.kd[0], lkd1 = L.color[1] * H.mat.kd[1], lkd2 = L.color[2] * H.mat.kd[2];
                const float lks0 = L.color[0] * H.mat.ks[0], lks1 = L.color[1] * H.mat.ks[1], lks2 = L.color[2] * H.mat.ks[2];
                const LightGrid lg = light_grid(L, px, py, pz);
                const unsigned long long word = SIMPLE ? vw[0] : 0ull;
                // SIMPLE lights: k_beam proves nearly every (hit, light) pair of the headline unblocked, so the word is usually the full mask
                // in every valid lane of the tile -- one wave-uniform test, then the loop without the visibility bit (same body, ALLVIS)
                const unsigned long long full = low_mask(N);
                if constexpr (TABLE) {
                    const bool all_visible = __ballot(word != full) == 0ull;
                    if (scene_lights) {
                        const float2 *__restrict__ lt = ltab + uniform_u32(static_cast<uint32_t>(l)) * RT_LIGHT_TAB_STRIDE;
                        // the light vectors' range test once per (tile, light); a tile where it fails in any lane keeps the loop by samples
                        const bool in_range = RT_HOISTED_TEST && light_dirs_in_range(H, L, lg.z, lt);
                        if (RT_HOISTED_TEST && RT_LIKELY(in_range)) {
                            if (RT_SHADE_ROWS) {
                                if (__builtin_expect(all_visible, 1))
                                    shade_samples_rows<true, true>(H, L, lg, word, N, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb, lt);
                                else
                                    shade_samples_rows<false, true>(H, L, lg, word, N, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb, lt);
                            } else if (__builtin_expect(all_visible, 1)) {
                                shade_samples<true, true, true, true>(H, L, lg, vw, word, N, px, py, pz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb, lt);
                            } else {
                                shade_samples<true, false, true, true>(H, L, lg, vw, word, N, px, py, pz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb, lt);
                            }
                        } else if (RT_SHADE_ROWS && !RT_HOISTED_TEST) {
                            if (__builtin_expect(all_visible, 1))
                                shade_samples_rows<true, false>(H, L, lg, word, N, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb, lt);
                            else
                                shade_samples_rows<false, false>(H, L, lg, word, N, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb, lt);
                        } else if (__builtin_expect(all_visible, 1)) {
                            shade_samples<true, true, true>(H, L, lg, vw, word, N, px, py, pz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb, lt);
                        } else {
                            shade_samples<true, false, true>(H, L, lg, vw, word, N, px, py, pz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb, lt);
                        }
                    } else if (all_visible) {
                        shade_samples<true, true>(H, L, lg, vw, word, N, px, py, pz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb);
                    } else {
                        shade_samples<true, false>(H, L, lg, vw, word, N, px, py, pz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb);
                    }
                } else if constexpr (SIMPLE) {
                    if (__builtin_expect(__ballot(word != full) == 0ull, 1))
                        shade_samples<true, true>(H, L, lg, vw, word, N, px, py, pz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb);
                    else
                        shade_samples<true, false>(H, L, lg, vw, word, N, px, py, pz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb);
                } else {
                    shade_samples<false, false>(H, L, lg, vw, word, N, px, py, pz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, sum, cr, cg, cb);
                }
                const float a = sum / static_cast<float>(N), b = 1.3f / static_cast<float>(N);
                fr = fr + (cr * a) * b;
                fg = fg + (cg * a) * b;
                fb = fb + (cb * a) * b;
            }
            const uint32_t kind = material_dispatch(H, level < F.max_depth, it.dx, it.dy, it.dz, it.lx, it.ly, it.lz, it.lmode, child, &fres[it.pix]);
            rec[it.pix] = make_float4(fr, fg, fb, __uint_as_float(kind));
            if (kind != KIND_CONST) {
                spawn = true;
                child.ox = H.hx; child.oy = H.hy; child.oz = H.hz; child.pix = it.pix;
            }
        }
        if (FLAT && __ballot(spawn) != 0ull) {
            // traceRay of the child, closest hit only (flyscene.cpp:655-691), exactly as k_trace runs it; no hit -> BACKGROUND at the next level
            const bool hit = found(flat_closest_hit(root, tris, spawn, child.ox, child.oy, child.oz, child.dx, child.dy, child.dz).face, S.n_faces);
            c_resolved += static_cast<uint32_t>(__popcll(__ballot(spawn && !hit)));                                            // bounce rays that were traced here
            if (spawn && !hit) {
                rec[static_cast<size_t>(F.npix) + child.pix] = background_record();          // BACKGROUND (level + 1)
                spawn = false;
            }
        }
        const unsigned long long sm = __ballot(spawn);
        if (sm != 0ull) {
            bool fits;
            const uint32_t base = shard_reserve(ctl->n_rays[level + 1], &ctl->overflow, tile, static_cast<uint32_t>(__popcll(sm)), F.ray_cap, lane, fits);
            if (spawn && fits) rays_out[base + lanes_below(sm)] = child;
        }
    }
    if (lane == 0 && c_shaded) stat_add(ctl, ST_SHADED_HITS, c_shaded);
    if (FOLD) {          // the pending pairs' sample rays: counted (and formed) here
        if (lane == 0 && c_sample) {
            stat_add(ctl, ST_RAYS_SAMPLE, c_sample);
            stat_add(ctl, ST_SAMPLE_WALKED, c_sample);
        }
    }
    if (FLAT) {
        if (lane == 0 && c_resolved) stat_add(ctl, ST_RAYS_BOUNCE, c_resolved);
    }
}

// ======================================================================================================
// K3b: the DEEP bounce levels of flat scenes (levels 2 .. max_depth), one launch.
// A bounce level costs four launches (trace, beam, shadow, shade) whether anything reaches it or not: on a convex mirror object -- cube.obj, the
// headline -- levels 2 .. 4 are empty and their 12 launches were 40 us of a 0.36 ms frame.  A pixel's chain of bounces depends on nothing but
// itself, so here a wave takes 64 level-2 rays and carries them through ALL remaining levels on its own: closest hit and light-centre
// visibility over the root leaf (flat_walk, as k_trace), then phongShade with the visibility of every light sample computed in place
// (lane = hit, one flat_walk over the root leaf per sample: the segment lightStrikes would test), material dispatch, next level.  Nothing is
// compacted and nothing is culled: every decision is the reference's own test on the ray itself, and the per-sample arithmetic is the code
// k_shade runs (shade_hit / phong_sample / material_dispatch).  An empty level 2 is one launch that reads one counter.  Flat scenes only (a
// root leaf of <= 64 triangles: a sample costs <= 64 triangle tests); tree scenes and levels 0 / 1 keep the wide kernels.
// ======================================================================================================
__global__ __launch_bounds__(256) RT_SHADE_ATTR void k_deep(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris, const DScene S, const DLights L, const DFrame F,
                                                            const int level0, const RayItem *__restrict__ rays_in, Control *__restrict__ ctl,
                                                            float4 *__restrict__ rec0, float *__restrict__ fres0) {
    __shared__ double s_pow[RT_POW_TAB];
    const int lane = threadIdx.x & 63;
    const ShardMap rmap = shard_map(ctl->n_rays[level0], lane, 0xffffffffu, 1u, 64u);
    const uint32_t ntiles = rmap.total;
    if (ntiles == 0u) return;                     // nothing reaches the deep levels: every wave leaves here
    pow_tables_to_lds(s_pow);
    const DNode root = nodes[0];
    const uint32_t N = static_cast<uint32_t>(L.n_samples);
    const uint32_t vst = static_cast<uint32_t>(L.vsteps > 0 ? L.vsteps : 1);
    uint32_t c_rays = 0, c_centre = 0, c_sample = 0, c_shaded = 0, c_unused0 = 0, c_unused1 = 0;
    const uint32_t wave_id = uniform_u32(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t wave_count = gridDim.x * 4u;
    for (uint32_t tile = wave_id; tile < ntiles; tile += wave_count) {
        uint32_t sh, tj, n_in;
        shard_find(rmap, tile, sh, tj, n_in);
        const uint32_t k = tj * 64u + static_cast<uint32_t>(lane);
        bool alive = k < n_in;
        const RayItem it0 = rays_in[alive ? sh * F.ray_cap + k : 0u];
        float ox = it0.ox, oy = it0.oy, oz = it0.oz, dx = it0.dx, dy = it0.dy, dz = it0.dz, lx = it0.lx, ly = it0.ly, lz = it0.lz;
        uint32_t lmode = it0.lmode;
        const uint32_t pix = it0.pix;
        for (int level = level0; level <= F.max_depth && __ballot(alive) != 0ull; ++level) {
            float4 *__restrict__ rec = rec0 + static_cast<size_t>(level - level0) * F.npix;
            float *__restrict__ fres = fres0 + static_cast<size_t>(level - level0) * F.npix;
            // ---- traceRay: closest hit (flyscene.cpp:655-691), as k_trace
            c_rays += alive ? 1u : 0u;
            const Hit best = flat_closest_hit(root, tris, alive, ox, oy, oz, dx, dy, dz);
            const float best_t = best.t;
            const int best_f = best.face;
            const bool hit = alive && found(best_f, S.n_faces);
            const float hx = ox + best_t * dx, hy = oy + best_t * dy, hz = oz + best_t * dz;   // flyscene.cpp:695
            // ---- lightStrikes(hitPoint, lights): one segment per light centre (flyscene.cpp:700)
            const int nl_lane = lmode ? 1 : L.n_lights;
            const bool lit = centre_lit<false, true>(root, nodes, tris, nullptr, nullptr, S.extent, WaveStack{nullptr, nullptr, nullptr}, lane, L, hit, hx, hy, hz, lmode, lx, ly, lz,
                                                     c_centre, c_unused0, c_unused1);
            if (alive) {
                if (!hit) rec[pix] = background_record();          // BACKGROUND
                else if (!lit) rec[pix] = shadow_record();         // SHADOW
            }
            alive = lit;
            if (__ballot(lit) == 0ull) break;
            // ---- phongShade (flyscene.cpp:822-859): the lanes that hold a lit hit; every sample's lightStrikes segment is walked in place
            c_shaded += lit ? 1u : 0u;
            const int face = lit ? best_f : 0;
            const ShadeHit H = shade_hit(S, face, ox, oy, oz, dx, dy, dz, lit ? best_t : 0.0f);      // (lanes without a lit hit: finite stand-in values, never stored)
            float fr = 0.f, fg = 0.f, fb = 0.f;
            const int nl_shade = (__ballot(lit && lmode == 0u) != 0ull) ? L.n_lights : 1;
            const float lkd0 = L.color[0] * H.mat.kd[0], lkd1 = L.color[1] * H.mat.kd[1], lkd2 = L.color[2] * H.mat.kd[2];
            const float lks0 = L.color[0] * H.mat.ks[0], lks1 = L.color[1] * H.mat.ks[1], lks2 = L.color[2] * H.mat.ks[2];
            for (int l = 0; l < nl_shade; ++l) {
                const bool act = lit && (l < nl_lane);
                float px, py, pz;
                light_point(L, l, lmode, lx, ly, lz, px, py, pz);
                const LightGrid lg = light_grid(L, px, py, pz);
                float sum = 0.f, cr = 0.f, cg = 0.f, cb = 0.f;
                uint32_t si = 0, sj = 0;
                for (uint32_t s = 0; s < N; ++s) {
                    float sx, sy, sz;
                    grid_sample(lg, static_cast<float>(si) + 0.5f, static_cast<float>(sj) + 0.5f, sx, sy, sz);
                    if (L.mode == RT_LIGHT_SPHERE) sphere_sample(L, s, px, py, pz, sx, sy, sz);
                    if (++sj == vst) { sj = 0; ++si; }
                    // lightStrikes(hitPoint, {sample}): origin = sample, direction = hitPoint - sample (flyscene.cpp:912-954), as k_shadow forms it
                    c_sample += act ? 1u : 0u;
                    const bool occ = flat_unit_occluded<false>(root, tris, seg_off(), 0ull, LanePlane{}, act, segment_ray(sx, sy, sz, H.hx, H.hy, H.hz), c_unused0, c_unused1);
                    const bool visible = act && !occ;
                    sum += visible ? 1.0f : 0.0f;
                    float tr_, tg_, tb_;
                    phong_sample(H, sx, sy, sz, lkd0, lkd1, lkd2, lks0, lks1, lks2, s_pow, tr_, tg_, tb_);
                    cr = cr + (visible ? tr_ : 0.0f);
                    cg = cg + (visible ? tg_ : 0.0f);
                    cb = cb + (visible ? tb_ : 0.0f);
                }
                const float a = sum / static_cast<float>(N), b = 1.3f / static_cast<float>(N);
                fr = act ? fr + (cr * a) * b : fr;
                fg = act ? fg + (cg * a) * b : fg;
                fb = act ? fb + (cb * a) * b : fb;
            }
            RayItem child;
            child.pad = 0u;
            uint32_t kind = KIND_CONST;
            if (lit) {
                kind = material_dispatch(H, level < F.max_depth, dx, dy, dz, lx, ly, lz, lmode, child, &fres[pix]);
                rec[pix] = make_float4(fr, fg, fb, __uint_as_float(kind));
            }
            alive = lit && kind != KIND_CONST;
            if (alive) {       // the child ray of this lane: origin = hitPoint
                ox = H.hx; oy = H.hy; oz = H.hz; dx = child.dx; dy = child.dy; dz = child.dz;
                lx = child.lx; ly = child.ly; lz = child.lz; lmode = child.lmode;
            }
        }
    }
    c_rays = wave_sum(c_rays); c_centre = wave_sum(c_centre); c_sample = wave_sum(c_sample); c_shaded = wave_sum(c_shaded);
    if (lane == 0) {
        unsigned long long *st = ctl->stat[blockIdx.x & (RT_STAT_SHARDS - 1)];
        if (c_rays) atomicAdd(&st[ST_RAYS_BOUNCE], static_cast<unsigned long long>(c_rays));
        if (c_centre) atomicAdd(&st[ST_RAYS_CENTRE], static_cast<unsigned long long>(c_centre));
        if (c_sample) { atomicAdd(&st[ST_RAYS_SAMPLE], static_cast<unsigned long long>(c_sample)); atomicAdd(&st[ST_SAMPLE_WALKED], static_cast<unsigned long long>(c_sample)); }
        if (c_shaded) atomicAdd(&st[ST_SHADED_HITS], static_cast<unsigned long long>(c_shaded));
    }
}

// ======================================================================================================
// K4: resolve.  Folds the per-level records from the deepest level outwards -- c_k = a*phong_k + b*c_{k+1} --
// which keeps the recursion's rounding (a running throughput product would not), then quantises like
// writePPMImage (ppmIO.hpp:145): min(255, (int)(255*c)).
// ======================================================================================================
// the colour traceRay returns for the primary ray of (sub-sample) pixel `pix`: its level-record chain folded (k_resolve: SRC_ONE folds one, SRC_SS n x n)
__device__ __forceinline__ void fold_chain(const float4 *__restrict__ rec, const float *__restrict__ fres, const uint32_t npix, const int max_depth,
                                           const uint32_t pix, float &vr, float &vg, float &vb) {
    int k = 0;
    float4 r = rec[pix];
    while (__float_as_uint(r.w) != KIND_CONST && k < max_depth) {
        ++k;
        r = rec[static_cast<size_t>(k) * npix + pix];
    }
    vr = r.x; vg = r.y; vb = r.z;
    for (int j = k - 1; j >= 0; --j) {
        const float4 p = rec[static_cast<size_t>(j) * npix + pix];
        const uint32_t kind = __float_as_uint(p.w);
        float a, b;
        if (kind == KIND_PASS) { a = 0.10f; b = 0.90f; }
        else if (kind == KIND_REFRACT) { a = 0.2f; b = 0.8f; }
        else { a = 0.15f; b = 0.85f; }
        vr = a * p.x + b * vr; vg = a * p.y + b * vg; vb = a * p.z + b * vb;
        if (kind == KIND_FRESNEL) {
            const float f = fres[static_cast<size_t>(j) * npix + pix];
            vr = f * vr; vg = f * vg; vb = f * vb;
        }
    }
}
__device__ __forceinline__ void store_pixel(float *__restrict__ out_rgb, uint8_t *__restrict__ out_u8, const uint32_t pix, const float vr, const float vg,
                                            const float vb) {
    if (out_rgb) { out_rgb[pix * 3] = vr; out_rgb[pix * 3 + 1] = vg; out_rgb[pix * 3 + 2] = vb; }
    if (out_u8) {
        const float c3[3] = {vr, vg, vb};
        for (int c = 0; c < 3; ++c) {
            int q = static_cast<int>(255 * c3[c]);
            q = q < 255 ? q : 255;
            out_u8[pix * 3 + c] = static_cast<uint8_t>(q < 0 ? 0 : q);
        }
    }
}
// Supersampled resolve (n = F.ss > 1): one thread per OUTPUT pixel (lr, i); it folds the chains of its n x n sub-samples -- internal pixel
// (n*lr + sy) * F.width + n*i + sx -- and stores acc / (float)(n*n), acc = 0.0f + the sub-sample colours, sy outer, sx inner (the order
// rt_set_supersampling defines).  Read-bound: adjacent threads take adjacent output pixels, so a wave's n reads per sub-row cover one
// contiguous run of 64 n records.
__device__ __forceinline__ void resolve_ss_pixel(const DFrame &F, const float4 *__restrict__ rec, const float *__restrict__ fres, const uint32_t lr,
                                                 const uint32_t i, float &vr, float &vg, float &vb) {
    const uint32_t n = static_cast<uint32_t>(F.ss);
    const float nn = static_cast<float>(n * n);
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    for (uint32_t sy = 0; sy < n; ++sy) {
        const uint32_t row = (n * lr + sy) * static_cast<uint32_t>(F.width) + n * i;
        for (uint32_t sx = 0; sx < n; ++sx) {
            float sr, sg, sb;
            fold_chain(rec, fres, F.npix, F.max_depth, row + sx, sr, sg, sb);
            ar = ar + sr; ag = ag + sg; ab = ab + sb;
        }
    }
    vr = ar / nn; vg = ag / nn; vb = ab / nn;
}

// Multi-pass accumulation (rt_set_passes, DESIGN.md §5, Multi-pass accumulation): the resolve of one pass of a count > 1 frame.  F_p is what
// the SINK_STORE resolve of the same SRC would store; MODE says where the pass stands in its run (wave-uniform from the launch):
//   ACC_FIRST  A = 0.0f + F_p          ACC_MIDDLE  A = A + F_p          ACC_LAST  store_pixel((A + F_p) / (float)count)
// A is one float[3] per output pixel of the call; thread <-> pixel is the same map in every pass, each pass is a launch of its own on one
// stream, so the read-modify-write needs no atomics.  Every operation rounds on its own (-ffp-contract=off, correctly rounded division).
// acc_add / acc_finish are the two halves of the step with run-time `first` / `last`: the converging resolve (SINK_CONV) takes them for S1 and S2.
__device__ __forceinline__ void acc_add(const float *__restrict__ a, const bool first, const float vr, const float vg, const float vb, float &ar, float &ag,
                                        float &ab) {
    ar = 0.0f; ag = 0.0f; ab = 0.0f;
    if (!first) { ar = a[0]; ag = a[1]; ab = a[2]; }
    ar = ar + vr; ag = ag + vg; ab = ab + vb;
}
__device__ __forceinline__ void acc_finish(float *__restrict__ a, const bool last, const float count, float *__restrict__ out_rgb, uint8_t *__restrict__ out_u8,
                                           const uint32_t pix, const float ar, const float ag, const float ab) {
    if (last) store_pixel(out_rgb, out_u8, pix, ar / count, ag / count, ab / count);
    else { a[0] = ar; a[1] = ag; a[2] = ab; }
}
// where a resolve takes a pixel's colour from (SRC) and what it does with it (SINK); the ACC_* sinks are the MODE of accumulate_pixel
enum : int { SRC_ONE = 0, SRC_SS = 1, SRC_ADAPTIVE = 2 };
enum : int { SINK_STORE = 0, ACC_FIRST = 1, ACC_MIDDLE = 2, ACC_LAST = 3, SINK_CONV = 4 };
template <int MODE>
__device__ __forceinline__ void accumulate_pixel(float *__restrict__ acc, const float count, float *__restrict__ out_rgb, uint8_t *__restrict__ out_u8,
                                                 const uint32_t pix, const float vr, const float vg, const float vb) {
    float *a = acc + static_cast<size_t>(pix) * 3u;
    float ar, ag, ab;
    acc_add(a, MODE == ACC_FIRST, vr, vg, vb, ar, ag, ab);
    acc_finish(a, MODE == ACC_LAST, count, out_rgb, out_u8, pix, ar, ag, ab);
}

// ======================================================================================================
// Adaptive pass counts (rt_set_pass_tolerance, DESIGN.md §5, Adaptive pass counts).
// SINK_CONV of k_resolve below is the resolve of pass k (1-based) of such a frame.  An active pixel folds F_p as the SINK_STORE resolve of its
// SRC (SRC_ONE: n = 1, SRC_SS: n > 1) would store it, adds it to S1 (the accumulator of rt_set_passes) and its square to S2, notes k in
// `taken`, and from pass min_passes on -- but not in the last one -- evaluates the rule of the header: kf S2 - S1 S1 <= ((tol tol)(kf kf))(kf - 1)
// in all three channels (every operation rounds on its own; a NaN compares false and never converges).  The pixel stores S1 / taken exactly
// once: when it converges or in the last pass.  An inactive pixel touches nothing -- its level records are stale.  Pass 1 writes every
// field of every pixel without reading any, so no frame sees the state of the one before it.  first / last / test are wave-uniform.
// The waves of block 0 also zero the list counters Control::n_flag for k_pass_list behind this launch: every reader of the list of THIS pass
// (the primary kernels of level 0) has finished on the stream.
// ======================================================================================================
// The resolve kernel: one thread per OUTPUT pixel pix of the F.out_width x F.out_rows frame (a frame with F.ss == 1 has out_width * out_rows ==
// npix: output pixel = traced pixel).  SRC says where the pixel's colour comes from, SINK what becomes of it:
//   SRC_ONE       fold_chain of pix
//   SRC_SS        resolve_ss_pixel: the mean of the n x n sub-samples
//   SRC_ADAPTIVE  the last launch of an adaptive frame: a refined pixel is the regular n x n pixel (resolve_ss_pixel), any other copies C1
//   SINK_STORE    store_pixel            ACC_*  accumulate_pixel (rt_set_passes)            SINK_CONV  the converging resolve (above)
// Primary culling (F.cull, DESIGN.md §5, Primary culling; the plain one-ray frame only, the host leaves F.cull 0 for every other): a pixel
// outside the rectangle (DCamBlock::rect of a.cam: the camera of this frame, or the one this replay uploaded) has either no record at
// all -- its tile was never traced -- or a BACKGROUND record; it stores what that record folds to without reading it.
// ======================================================================================================
// The kernel's arguments: ResolveIo -- the argument list of the plain storing resolve -- and what the SRC and the SINK add to it, so that an
// instantiation carries only the arguments it reads (launch_resolve fills them from the host's ResolveArgs).
struct ResolveIo { const float4 *rec; const float *fres; float *out_rgb; uint8_t *out_u8; CamArg cam; };       // cam: read for `rect`, by a frame with F.cull set
struct ResolveNoSrc {};
struct ResolveNoSink {};
struct ResolveAdaptive { const uint8_t *refine; const float *c1; const int32_t *pos; };
struct ResolveAcc { float *acc; float count; };
struct ResolveConv { float *acc, *s2; uint16_t *taken; uint8_t *active; uint32_t *n_flag; int k, min_passes, count; float tol; };       // k: the 1-based pass
template <int SRC, int SINK>
struct ResolvePack : ResolveIo,
                     std::conditional_t<SRC == SRC_ADAPTIVE, ResolveAdaptive, ResolveNoSrc>,
                     std::conditional_t<SINK == SINK_CONV, ResolveConv, std::conditional_t<SINK == SINK_STORE, ResolveNoSink, ResolveAcc>> {};

template <int SRC, int SINK>
__global__ __launch_bounds__(256) void k_resolve(const DFrame F, const ResolvePack<SRC, SINK> a) {
    const uint32_t W = static_cast<uint32_t>(F.out_width);
    const uint32_t nout = SRC == SRC_ONE ? F.npix : W * static_cast<uint32_t>(F.out_rows);      // (the same number: SRC_ONE has F.ss == 1)
    const uint32_t stride = gridDim.x * blockDim.x;
    // primary culling: the rectangle, and the colour of a pixel outside it
    bool cull = false;
    CullRect R{0, 0, 0, 0};
    float br = 0.f, bgr = 0.f, bb = 0.f;
    if constexpr (SRC == SRC_ONE && SINK == SINK_STORE) {
        cull = F.cull != 0;
        if (cull) R = cull_rect(a.cam);
        const float4 bg = background_record();
        fold_chain(&bg, nullptr, 0u, 0, 0u, br, bgr, bb);
    }
    // the converging resolve: where pass k stands, the rule's right-hand side, and the list counters for the builder behind this launch
    bool first = false, last = false, test = false;
    float kf = 0.f, T = 0.f;
    if constexpr (SINK == SINK_CONV) {
        first = a.k == 1; last = a.k == a.count; test = a.k >= a.min_passes && !last;
        if (test) {
            if (blockIdx.x == 0u && threadIdx.x < RT_LIST_SHARDS) a.n_flag[threadIdx.x * 16u] = 0u;
        }
        kf = static_cast<float>(a.k);
        T = ((a.tol * a.tol) * (kf * kf)) * (kf - 1.0f);
    }
    for (uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x; pix < nout; pix += stride) {
        if constexpr (SINK == SINK_CONV) {
            bool act = true;
            if (!first) act = a.active[pix] != 0u;
            if (!act) continue;
        }
        const uint32_t lr = pix / W, i = pix - lr * W;
        float vr, vg, vb;
        if constexpr (SRC == SRC_ONE) {
            bool outside = false;
            if (cull) {
                const int x = static_cast<int>(i), y = frame_row(F, static_cast<int>(lr));
                outside = x < R.x0 || x >= R.x1 || y < R.y0 || y >= R.y1;
            }
            if (outside) { vr = br; vg = bgr; vb = bb; }
            else fold_chain(a.rec, a.fres, F.npix, F.max_depth, pix, vr, vg, vb);
        } else if constexpr (SRC == SRC_SS) {
            resolve_ss_pixel(F, a.rec, a.fres, lr, i, vr, vg, vb);
        } else if (a.refine[pix] != 0u) {
            resolve_ss_pixel(F, a.rec, a.fres, lr, i, vr, vg, vb);
        } else {
            const float *p = a.c1 + (static_cast<size_t>(a.pos[3 * lr + 1]) * W + i) * 3;
            vr = p[0]; vg = p[1]; vb = p[2];
        }
        if constexpr (SINK == SINK_STORE) {
            store_pixel(a.out_rgb, a.out_u8, pix, vr, vg, vb);
        } else if constexpr (SINK != SINK_CONV) {
            accumulate_pixel<SINK>(a.acc, a.count, a.out_rgb, a.out_u8, pix, vr, vg, vb);
        } else {
            float *s1 = a.acc + static_cast<size_t>(pix) * 3u, *s2 = a.s2 + static_cast<size_t>(pix) * 3u;
            float ar, ag, ab, sr2, sg2, sb2;
            acc_add(s1, first, vr, vg, vb, ar, ag, ab);
            const float qr = vr * vr, qg = vg * vg, qb = vb * vb;
            acc_add(s2, first, qr, qg, qb, sr2, sg2, sb2);
            bool done = last;
            if (test) {
                const float pr = kf * sr2, pg = kf * sg2, pb = kf * sb2;
                const float sr = ar * ar, sg = ag * ag, sb = ab * ab;
                const float dr = pr - sr, dg = pg - sg, db = pb - sb;
                done = dr <= T && dg <= T && db <= T;
                a.active[pix] = done ? 0u : 1u;
            } else if (first) {
                a.active[pix] = 1u;
            }
            a.taken[pix] = static_cast<uint16_t>(a.k);
            acc_finish(s1, done, kf, a.out_rgb, a.out_u8, pix, ar, ag, ab);        // (taken == k)
            if (!done) { s2[0] = sr2; s2[1] = sg2; s2[2] = sb2; }
        }
    }
}

// ======================================================================================================
// Adaptive supersampling (rt_set_supersampling_threshold, DESIGN.md §5, Adaptive supersampling).  C1 is the one-ray colour of pass 1, one
// row per frame row of the pass (the call's rows and their neighbours); pos[3 lr ..] are the C1 rows of frame rows y - 1, y, y + 1 of output
// local row lr (-1 outside the frame).  Pixel (i, lr) is refined when a 4-neighbour inside the frame differs from it by more than tau in some
// channel: fabsf of the float difference, compared in float (a NaN never refines).
// ======================================================================================================
__device__ __forceinline__ bool differs(const float *__restrict__ a, const float *__restrict__ b, const float tau) {
    return fabsf(a[0] - b[0]) > tau || fabsf(a[1] - b[1]) > tau || fabsf(a[2] - b[2]) > tau;
}
__device__ __forceinline__ bool refine_rule(const float *__restrict__ c1, const int32_t *__restrict__ pos, const uint32_t W, const uint32_t i,
                                            const uint32_t lr, const float tau) {
    const int32_t up = pos[3 * lr], mid = pos[3 * lr + 1], dn = pos[3 * lr + 2];
    const float *p = c1 + (static_cast<size_t>(mid) * W + i) * 3;
    bool r = false;
    if (i > 0u) r = r || differs(p, p - 3, tau);
    if (i + 1u < W) r = r || differs(p, p + 3, tau);
    if (up >= 0) r = r || differs(p, c1 + (static_cast<size_t>(up) * W + i) * 3, tau);
    if (dn >= 0) r = r || differs(p, c1 + (static_cast<size_t>(dn) * W + i) * 3, tau);
    return r;
}

// The list builder shared by k_flag and k_pass_list.  F is the frame of sub-samples whose primary tiles the next launch sequence takes from the
// list.  One wave per group of 16 of its 8x8 tiles that share a list shard (flag_groups); lane = sub-sample (X, Y) of the tile, which asks
// `pred` about the output pixel (X / n, Y / n) that owns it -- at n = 3 a tile straddles pixel boundaries, and the lanes of one pixel simply
// agree; at n = 1, where F.ss_mul is 0, the pixel is (X, Y) itself.  pred(i, lr, owner): owner marks the lane of sub-sample (0, 0) of the
// pixel, the one that may write per-pixel state and whose answers are counted into ST_REFINED.  A tile with a listed sub-sample goes to the
// list with the ballot of those lanes: lane j keeps the mask of tile j of the group, and ONE reservation per group places them (the order
// inside a shard is that of the reservations; the consumer does not depend on it).  Control::n_flag is zero when this starts.
template <typename Pred>
__device__ __forceinline__ void build_tile_list(const DFrame &F, FlagTile *__restrict__ list, Control *__restrict__ ctl, const Pred pred) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n = static_cast<uint32_t>(F.ss), tiles_x = static_cast<uint32_t>(F.tiles_x);
    const uint32_t ntiles = tiles_x * static_cast<uint32_t>(F.tiles_y), ngroups = flag_groups(ntiles);
    uint32_t c_listed = 0;
    for (uint32_t g = uniform_u32(blockIdx.x * RT_WAVES + static_cast<uint32_t>(wave)); g < ngroups; g += gridDim.x * RT_WAVES) {
        const uint32_t sh = g % RT_LIST_SHARDS, t0 = (g / RT_LIST_SHARDS) * (16u * RT_LIST_SHARDS) + sh;
        unsigned long long mine = 0ull;
        uint32_t my_tile = 0u;
        for (uint32_t j = 0; j < 16u; ++j) {
            const uint32_t t = t0 + j * RT_LIST_SHARDS;
            if (t >= ntiles) break;
            const uint32_t tx = t % tiles_x, ty = t / tiles_x;
            const uint32_t X = tx * 8u + static_cast<uint32_t>(lane & 7), Y = ty * 8u + static_cast<uint32_t>(lane >> 3);
            const bool valid = X < static_cast<uint32_t>(F.width) && Y < static_cast<uint32_t>(F.local_rows);
            uint32_t i = X, lr = Y;
            if (n > 1u) { i = __umulhi(X, F.ss_mul); lr = __umulhi(Y, F.ss_mul); }           // X / n, Y / n
            const bool owner = valid && X == i * n && Y == lr * n;
            bool listed = false;
            if (valid) listed = pred(i, lr, owner);
            c_listed += (listed && owner) ? 1u : 0u;
            const unsigned long long m = __ballot(listed);
            if (lane == static_cast<int>(j)) { mine = m; my_tile = t; }
        }
        const unsigned long long lm = __ballot(mine != 0ull);
        if (lm != 0ull) {
            bool fits;
            const uint32_t base = shard_reserve(ctl->n_flag, &ctl->overflow, sh, static_cast<uint32_t>(__popcll(lm)), F.tile_cap, lane, fits);
            if (mine != 0ull && fits) {
                FlagTile ft;
                ft.tile = my_tile; ft.pad = 0u; ft.mask = mine;
                list[base + lanes_below(lm)] = ft;
            }
        }
    }
    c_listed = wave_sum(c_listed);
    if (lane == 0 && c_listed) stat_add(ctl, ST_REFINED, c_listed);
}

// k_flag: F is pass 2's frame (the regular n x n frame of sub-samples).  A sub-sample is listed when the rule refines its pixel; the owner
// lane writes the pixel's refine byte, and the refined pixels are counted (build_tile_list).
struct RefinePred {
    const float *__restrict__ c1;
    const int32_t *__restrict__ pos;
    uint8_t *__restrict__ refine;
    uint32_t W;
    float tau;
    __device__ __forceinline__ bool operator()(const uint32_t i, const uint32_t lr, const bool owner) const {
        const bool ref = refine_rule(c1, pos, W, i, lr, tau);
        if (owner) refine[lr * W + i] = ref ? 1u : 0u;
        return ref;
    }
};
__global__ __launch_bounds__(RT_WAVES * 64) void k_flag(const DFrame F, const float *__restrict__ c1, const int32_t *__restrict__ pos, const float tau,
                                                       uint8_t *__restrict__ refine, FlagTile *__restrict__ list, Control *__restrict__ ctl) {
    build_tile_list(F, list, ctl, RefinePred{c1, pos, refine, static_cast<uint32_t>(F.out_width), tau});
}

// ======================================================================================================
// lightStrikes on explicit segments (rt_light_strikes): lane = segment light[i] -> hit[i]
// ======================================================================================================
__global__ __launch_bounds__(RT_WAVES * 64) void k_segments(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                          const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                             const DScene S, const int n, const float *__restrict__ hit,
                                                             const float *__restrict__ light, uint8_t *__restrict__ vis) {
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + (false ? 0 : wave * RT_STACK), s_mask + (false ? 0 : wave * RT_STACK), s_stage + (false ? 0 : wave * RT_STAGE_TRIS * 5)};
    const DNode root = nodes[0];
    const int waves_total = gridDim.x * RT_WAVES;
    for (int base = (blockIdx.x * RT_WAVES + wave) * 64; base < n; base += waves_total * 64) {
        const int i = base + lane;
        const bool valid = i < n;
        const int j = valid ? i : 0;
        const float px = light[j * 3], py = light[j * 3 + 1], pz = light[j * 3 + 2];
        const WalkRay ray = segment_ray(px, py, pz, hit[j * 3], hit[j * 3 + 1], hit[j * 3 + 2]);
        uint32_t c0 = 0, c1 = 0;
        const bool occ = walk<true, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, valid && root_hit(root, ray), ray, c0, c1);
        if (valid) vis[i] = occ ? 0 : 1;
    }
}

// ======================================================================================================
// Device ray queries (rt_closest_hits_device, rt_trace_rays_device; DESIGN.md §5, Device ray queries).  Both kernels are templates only
// so that the code object emits them where kKernelOrder names them, behind every kernel that was there before them.
// ======================================================================================================
// k_closest, the closest-hit sibling of k_segments: lane = ray (org[i], dir[i]), the level-0 closest hit of traceRay -- the root test on
// (o, o + d), then the minimum t > 1e-5, ties to the lowest face id.  face / t: either may be null; -1 / -1.0f for a miss.  It reads the
// scene alone: no control block, no list, no frame buffer.  Element indices are 64-bit (i * 3 leaves 32 bits above 715 M rays).
template <int = 0>
__global__ __launch_bounds__(RT_WAVES * 64) void k_closest(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                         const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                         const DScene S, const int n, const float *__restrict__ org,
                                                         const float *__restrict__ dir, int32_t *__restrict__ face, float *__restrict__ t) {
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, s_stage + wave * RT_STAGE_TRIS * 5};
    const DNode root = nodes[0];
    const size_t total = static_cast<size_t>(n), step = static_cast<size_t>(gridDim.x) * RT_WAVES * 64;
    for (size_t base = (static_cast<size_t>(blockIdx.x) * RT_WAVES + static_cast<size_t>(wave)) * 64; base < total; base += step) {
        const size_t i = base + static_cast<size_t>(lane);
        const bool valid = i < total;
        const size_t j = valid ? i : 0;
        const WalkRay ray = trace_ray(org[j * 3], org[j * 3 + 1], org[j * 3 + 2], dir[j * 3], dir[j * 3 + 1], dir[j * 3 + 2]);
        uint32_t c0 = 0, c1 = 0;
        const Hit best = walk<false, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, valid && root_hit(root, ray), ray, c0, c1);
        const bool hit = found(best.face, S.n_faces);
        if (valid && face) face[i] = hit ? best.face : -1;
        if (valid && t) t[i] = hit ? best.t : -1.0f;
    }
}

// k_pack_rays: lane i turns ray (org[i], dir[i]) into RayItem i of a listed-ray launch sequence, byte for byte what the host loop of
// rt_trace_rays writes (the ray sees the scene lights; pix = i, its place in the batch).  Three dword loads per array and lane at a
// twelve-byte stride: a wave's loads together cover its 768 bytes of each array fully, so nothing is staged in LDS.
template <int = 0>
__global__ __launch_bounds__(256) void k_pack_rays(const int n, const float *__restrict__ org, const float *__restrict__ dir, RayItem *__restrict__ rays) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;          // (n <= 2^24, one query chunk: 32 bits hold i * 3)
    if (i >= n) return;
    const float *__restrict__ o = org + i * 3, *__restrict__ d = dir + i * 3;
    uint4 *__restrict__ out = reinterpret_cast<uint4 *>(rays + i);
    out[0] = make_uint4(__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]), __float_as_uint(d[0]));
    out[1] = make_uint4(__float_as_uint(d[1]), __float_as_uint(d[2]), 0u, 0u);              // dy, dz, lx, ly
    out[2] = make_uint4(0u, 0u, static_cast<uint32_t>(i), 0u);                              // lz, lmode, pix, pad
}

// ======================================================================================================
// Ambient occlusion (rt_ambient_occlusion_device, rt_hit_points_device; DESIGN.md §5, Ambient occlusion).  Templates for the same reason.
// ======================================================================================================
// k_occlusion: a WAVE OWNS WHOLE POINTS and every lane of every round holds a segment (rt_ao_layout.hpp): a wave unit is 64 / gcd(K, 64)
// points, walked in K / gcd(K, 64) rounds of 64 segments; lane l of round r holds segment e = r * 64 + l of the unit, direction e % K of
// its point e / K.  ROUNDS = false: K divides 64, one round.  Each lane forms its own far end Q and the segment Q -> P as the header
// defines them (float32, one rounding per operation, in the order written there), the wave walks the segments as k_segments does, and
// lane p keeps the count of point p: the popcount, round by round, of that point's lanes in the ballot of the visible ones.  No atomics,
// no list, every output written once.  Segments of points with a zero normal and of points behind n are inactive; a round without an
// active lane skips the walk (a wave-uniform branch).  Every round loads its points afresh, so nothing of them stays in registers across a
// walk.  dirs: the table of m (K entries xyz), rot: the 64 (c, s) pairs.  It reads the scene and those tables alone.
// The segment of direction k of the point P with normal N: the frame, the rotated direction, the far end.
// (ao_direction: the rotated direction d alone, which k_gather traces as a ray)
__device__ __forceinline__ void ao_direction(const float nx, const float ny, const float nz, const float *__restrict__ dirs, const int k, const float c,
                                             const float s, float &dx, float &dy, float &dz) {
    // the frame of Duff et al.
    const float sg = __builtin_copysignf(1.0f, nz);
    const float a = -1.0f / (sg + nz);
    const float b = (nx * ny) * a;
    const float tx = 1.0f + (sg * (nx * nx)) * a, ty = sg * b, tz = -(sg * nx);
    const float bx = b, by = sg + (ny * ny) * a, bz = -ny;
    const float x = dirs[k * 3], y = dirs[k * 3 + 1], z = dirs[k * 3 + 2];
    const float xr = c * x - s * y, yr = s * x + c * y;
    dx = ((xr * tx) + (yr * bx)) + (z * nx);
    dy = ((xr * ty) + (yr * by)) + (z * ny);
    dz = ((xr * tz) + (yr * bz)) + (z * nz);
}
__device__ __forceinline__ WalkRay ao_segment(const float px, const float py, const float pz, const float nx, const float ny, const float nz,
                                              const float *__restrict__ dirs, const int k, const float c, const float s, const float radius) {
    float dx, dy, dz;
    ao_direction(nx, ny, nz, dirs, k, c, s, dx, dy, dz);
    return segment_ray(px + radius * dx, py + radius * dy, pz + radius * dz, px, py, pz);
}
template <bool ROUNDS>
__global__ __launch_bounds__(RT_WAVES * 64) void k_occlusion(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                           const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                           const DScene S, const int n, const float *__restrict__ point,
                                                           const float *__restrict__ normal, const float *__restrict__ dirs,
                                                           const float *__restrict__ rot, const int m, const float radius, const uint32_t seed,
                                                           uint16_t *__restrict__ open, float *__restrict__ ao) {
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, s_stage + wave * RT_STAGE_TRIS * 5};
    const DNode root = nodes[0];
    const AoLayout L = ao_layout(m);                       // (the launcher picks ROUNDS = L.rounds > 1)
    const int rounds = ROUNDS ? L.rounds : 1;
    const int p0 = lane / L.K, k0 = lane - p0 * L.K;
    const uint64_t units = ao_units(n, L), step = static_cast<uint64_t>(gridDim.x) * RT_WAVES;
    for (uint64_t unit = static_cast<uint64_t>(blockIdx.x) * RT_WAVES + static_cast<uint64_t>(wave); unit < units; unit += step) {
        const uint64_t first = unit * static_cast<uint64_t>(L.group);
        uint32_t count = 0u;
        bool no_point = false;
        int p = p0, k = k0;
        for (int round = 0; round < rounds; ++round) {
            const uint64_t pi = first + static_cast<uint64_t>(p);
            const bool has = pi < static_cast<uint64_t>(n);
            const size_t j = has ? ao_xyz(pi) : 0;
            // (all six loads are issued together: a short-circuit test of the normal would wait for one load after the other)
            const float px = point[j], py = point[j + 1], pz = point[j + 2];
            const float nx = normal[j], ny = normal[j + 1], nz = normal[j + 2];
            const bool zero = (nx == 0.0f) & (ny == 0.0f) & (nz == 0.0f);                  // (+-0 both compare equal to 0)
            const bool act = has & !zero;
            const uint32_t r = ao_hash(seed, static_cast<uint32_t>(pi)) >> 26;
            const WalkRay ray = ao_segment(px, py, pz, nx, ny, nz, dirs, k, rot[r * 2u], rot[r * 2u + 1u], radius);
            bool occ = false;
            if (__ballot(act) != 0ull) {
                uint32_t c0 = 0, c1 = 0;
                occ = walk<true, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, act && root_hit(root, ray), ray, c0, c1);
            }
            const unsigned long long vis = __ballot(act && !occ), zeros = __ballot(has & zero);
            const unsigned long long mine = ao_point_lanes(L, lane, round);              // (lane p counts for point p of the unit)
            count += static_cast<uint32_t>(__popcll(vis & mine));
            no_point = no_point | ((zeros & mine) != 0ull);
            if constexpr (ROUNDS) ao_next(L, p, k);
        }
        const uint64_t own = first + static_cast<uint64_t>(lane);
        if (lane < L.group && own < static_cast<uint64_t>(n)) {
            const uint32_t o = no_point ? static_cast<uint32_t>(L.K) : count;
            if (open) open[own] = static_cast<uint16_t>(o);
            if (ao) ao[own] = static_cast<float>(o) / static_cast<float>(L.K);
        }
    }
}

// k_hit_points: thread i turns closest hit (face[i], t[i]) of ray (org[i], dir[i]) into an occlusion input: P = o + t * d and the face's
// normal as uploaded, its sign bits flipped where it looks along the ray; a face id outside [0, n_faces) -- a miss -- gives six 0.0f, the
// "no point" of k_occlusion.  The id is range-checked before it indexes anything.  No LDS; element indices are 64-bit.
template <int = 0>
__global__ __launch_bounds__(256) void k_hit_points(const float *__restrict__ face_normal, const uint32_t n_faces, const int n,
                                                    const float *__restrict__ org, const float *__restrict__ dir, const int32_t *__restrict__ face,
                                                    const float *__restrict__ t, float *__restrict__ point, float *__restrict__ normal) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (i >= static_cast<size_t>(n)) return;
    const int32_t f = face[i];
    float px = 0.0f, py = 0.0f, pz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (found(f, n_faces)) {
        const float tt = t[i];
        const float dx = dir[i * 3], dy = dir[i * 3 + 1], dz = dir[i * 3 + 2];
        px = org[i * 3] + tt * dx; py = org[i * 3 + 1] + tt * dy; pz = org[i * 3 + 2] + tt * dz;
        const size_t g = static_cast<size_t>(f) * 3u;
        nx = face_normal[g]; ny = face_normal[g + 1]; nz = face_normal[g + 2];
        if ((nx * dx + ny * dy) + nz * dz > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    }
    point[i * 3] = px; point[i * 3 + 1] = py; point[i * 3 + 2] = pz;
    normal[i * 3] = nx; normal[i * 3 + 1] = ny; normal[i * 3 + 2] = nz;
}

// ======================================================================================================
// Geometry buffers as a query (rt_gbuffer_device; the RT_GBUFFER_CHANNELS section of include/rt_mi355x.h defines the eight floats; DESIGN.md
// §5, Geometry buffers as a query).  A template for the same reason.
// ======================================================================================================
// k_gbuffer: a WAVE OWNS AN 8 x 8 TILE OF OUTPUT PIXELS (rt_gbuffer_layout.hpp) and walks it once per sub-sample: three wave-uniform loops
// -- passes first .. first + count - 1, sy outer, sx inner, the definition's order -- and in each step lane (i, j) forms the ray of ITS
// sub-sample (sx, sy) of pass p, internal column i * n + sx / frame row j * n + sy, by the functions the frames use in their PASS forms (the
// PASS forms are pass 0 bit for bit with pass 0's table entry and key 0).  The 64 rays of a step are the same sub-sample of 64 neighbouring
// pixels, a coherent packet, and the hit rule is the level-0 step of k_trace: in_root = pre && root_hit, the walk of k_closest, found().
// The sub-sample index being wave-uniform, its offset is ONE scalar from the pass table (pass_tab: rt_pass_offsets of (n, p), columns
// then rows): the raster coordinate is raster_coord<true>'s (float)i + o[sx] without the per-lane split of an internal column.
// F describes the OUTPUT frame of the call (width, local_rows, the row shard: what frame_row needs) and carries the sample settings of
// the frames (ss, ss_mul, lens*, lens_mul); pass_key is set per pass here, sso is not read.  MODE 0: pinhole, 1: lens, 2: shutter (the lens
// behind it by a wave-uniform branch on F.lens, as in shutter_ray: both cases have a per-lane origin).  The camera and the shutter deltas
// are kernel arguments: the call reads the scene, the pass table and the lens table alone.  The per-lane camera of a shutter step dies
// with the step's ray; across a walk a lane keeps its pixel, the pass accumulator and the frame accumulator.  No atomics, no list: every
// output pixel is written once, as two float4.
template <int MODE>
__global__ __launch_bounds__(RT_WAVES * 64) void k_gbuffer(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                         const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                         const DScene S, const DCam cam, const DShutter shut, const DFrame F,
                                                         const float *__restrict__ pass_tab, const int first, const int count,
                                                         float4 *__restrict__ out) {
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, s_stage + wave * RT_STAGE_TRIS * 5};
    const DNode root = nodes[0];
    const int n = F.ss;
    const float nn = static_cast<float>(n * n);
    const GbTiles T = gb_tiles(F.width, F.local_rows);
    const uint32_t step = gridDim.x * RT_WAVES;             // (<= 8 blocks per CU: far below 2^32 - tiles)
    for (uint32_t tile = uniform_u32(blockIdx.x * RT_WAVES + static_cast<uint32_t>(wave)); tile < T.tiles; tile += step) {
        const GbLane px = gb_lane(T, F.width, F.local_rows, tile, lane);
        // (a lane past the frame edge computes with pixel (0, row of local row 0): its ray is formed, takes no part in the walk and stores nothing)
        const int i = px.live ? px.i : 0, j = frame_row(F, px.live ? px.lr : 0);
        const float fi = static_cast<float>(i), fj = static_cast<float>(j);
        float A[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int p = first; p < first + count; ++p) {
            const float *__restrict__ o = pass_tab + gb_pass_entry(n, p);
            DFrame Fp = F;
            Fp.pass_key = static_cast<uint32_t>(p) * 0xC2B2AE35u;
            float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int sy = 0; sy < n; ++sy) {
                const float y = fj + o[RT_MAX_SUPERSAMPLING + sy];
                for (int sx = 0; sx < n; ++sx) {
                    const float x = fi + o[sx];
                    const int xi = i * n + sx, yi = j * n + sy;        // internal column / frame row of the sub-sample frame
                    float ox, oy, oz, dx, dy, dz;
                    {
                        DCam k = cam;
                        if (MODE == 2) k = shutter_camera(cam, shut, shutter_time<true>(Fp, xi, yi));
                        float sx_, sy_, sz_;
                        screen_point_at(k, x, y, sx_, sy_, sz_);
                        if (MODE == 1 || (MODE == 2 && F.lens != nullptr)) lens_ray<true>(k, Fp, xi, yi, sx_, sy_, sz_, ox, oy, oz, dx, dy, dz);
                        else {
                            ox = k.center[0]; oy = k.center[1]; oz = k.center[2];
                            dx = sx_ - ox; dy = sy_ - oy; dz = sz_ - oz;
                        }
                    }
                    const bool pre = px.live && root_pre_test(root, ox, oy, oz, dx, dy, dz);
                    const WalkRay ray = trace_ray(ox, oy, oz, dx, dy, dz);
                    const bool in_root = pre && root_hit(root, ray);
                    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    if (__ballot(in_root) != 0ull) {                    // (a step whose 64 rays all miss the root walks nothing)
                        uint32_t c0 = 0, c1 = 0;
                        const Hit best = walk<false, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, in_root, ray, c0, c1);
                        if (px.live && found(best.face, S.n_faces)) {
                            const size_t g = static_cast<size_t>(best.face) * 3u;
                            const float *__restrict__ kd = S.mats[S.mat_id[best.face]].kd;
                            v[0] = 1.0f; v[1] = best.t;
                            v[2] = S.face_normal[g]; v[3] = S.face_normal[g + 1]; v[4] = S.face_normal[g + 2];
                            v[5] = kd[0]; v[6] = kd[1]; v[7] = kd[2];
                        }
                    }
                    if (n == 1) {
#pragma unroll
                        for (int c = 0; c < 8; ++c) a[c] = v[c];                    // (v itself: a -0.0f stays)
                    } else {
#pragma unroll
                        for (int c = 0; c < 8; ++c) a[c] = a[c] + v[c];
                    }
                }
            }
            if (n > 1) {
#pragma unroll
                for (int c = 0; c < 8; ++c) a[c] = a[c] / nn;
            }
            if (count == 1) {
#pragma unroll
                for (int c = 0; c < 8; ++c) A[c] = a[c];                            // (the pass itself)
            } else {
#pragma unroll
                for (int c = 0; c < 8; ++c) A[c] = A[c] + a[c];
            }
        }
        if (count > 1) {
            const float fc = static_cast<float>(count);
#pragma unroll
            for (int c = 0; c < 8; ++c) A[c] = A[c] / fc;
        }
        if (px.live) {
            const uint64_t q = gb_out_vec4(F.width, px.lr, px.i);
            out[q] = make_float4(A[0], A[1], A[2], A[3]);
            out[q + 1u] = make_float4(A[4], A[5], A[6], A[7]);
        }
    }
}

// ======================================================================================================
// Soft shadows as a query (rt_soft_shadows_device; the soft-shadow section of include/rt_mi355x.h is the definition; DESIGN.md §5, Soft
// shadows).  A template for the same reason.
// ======================================================================================================
// k_soft_shadows: k_occlusion's mapping (a WAVE OWNS WHOLE POINTS, every lane of every round holds a segment, lane p keeps the count of point p
// from the ballots; no atomics, no list, every output written once) for K = n_lights * usteps * vsteps segments per point
// (rt_shadow_layout.hpp).  Segment k of a point is cell (i, j) of the grid of light l, k = (l * usteps + i) * vsteps + j: the lane finds the
// three by division once, before its first round, and shadow_next carries them from round to round.  Its sample is light_grid /
// grid_sample's -- the operations of the frames -- at (float)i + fu, (float)j + fv, with (fu, fv) the call's pair or the hash of the point's
// index (shadow_jitter), and the segment sample -> point is walked as k_segments walks it.  normal == nullptr: every point is a point (a
// wave-uniform branch); else a normal of three +-0 marks "no point", as in k_occlusion.  ROUNDS = false: K divides 64, one round.  The lights
// are a kernel argument; the kernel reads the scene and its two input arrays alone.
template <bool ROUNDS>
__global__ __launch_bounds__(RT_WAVES * 64) void k_soft_shadows(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                              const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                              const DScene S, const DLights L, const int n, const float *__restrict__ point,
                                                              const float *__restrict__ normal, const int per_point, const uint32_t seed,
                                                              const float fu, const float fv, uint16_t *__restrict__ visible,
                                                              float *__restrict__ share) {
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, s_stage + wave * RT_STAGE_TRIS * 5};
    const DNode root = nodes[0];
    const ShadowLayout Y = shadow_layout(L.n_lights, L.usteps, L.vsteps);      // (the launcher picks ROUNDS = Y.A.rounds > 1)
    const int rounds = ROUNDS ? Y.A.rounds : 1;
    const int p0 = lane / Y.A.K;
    const ShadowCell c0 = shadow_cell(Y, lane - p0 * Y.A.K);
    const uint64_t units = ao_units(n, Y.A), step = static_cast<uint64_t>(gridDim.x) * RT_WAVES;
    for (uint64_t unit = static_cast<uint64_t>(blockIdx.x) * RT_WAVES + static_cast<uint64_t>(wave); unit < units; unit += step) {
        const uint64_t first = unit * static_cast<uint64_t>(Y.A.group);
        uint32_t count = 0u;
        bool no_point = false;
        int p = p0;
        ShadowCell c = c0;
        for (int round = 0; round < rounds; ++round) {
            const uint64_t pi = first + static_cast<uint64_t>(p);
            const bool has = pi < static_cast<uint64_t>(n);
            const size_t q = has ? ao_xyz(pi) : 0;
            const float px = point[q], py = point[q + 1], pz = point[q + 2];
            bool zero = false;
            if (normal != nullptr) {
                const float nx = normal[q], ny = normal[q + 1], nz = normal[q + 2];
                zero = (nx == 0.0f) & (ny == 0.0f) & (nz == 0.0f);                         // (+-0 both compare equal to 0)
            }
            const bool act = has & !zero;
            float ju = fu, jv = fv;
            if (per_point) shadow_jitter(seed, static_cast<uint32_t>(pi), ju, jv);
            float sx, sy, sz;
            grid_sample(light_grid(L, L.pos[c.l][0], L.pos[c.l][1], L.pos[c.l][2]), static_cast<float>(c.i) + ju, static_cast<float>(c.j) + jv, sx, sy, sz);
            const WalkRay ray = segment_ray(sx, sy, sz, px, py, pz);
            bool occ = false;
            if (__ballot(act) != 0ull) {
                uint32_t w0 = 0, w1 = 0;
                occ = walk<true, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, act && root_hit(root, ray), ray, w0, w1);
            }
            const unsigned long long vis = __ballot(act && !occ), zeros = __ballot(has & zero);
            const unsigned long long mine = ao_point_lanes(Y.A, lane, round);            // (lane p counts for point p of the unit)
            count += static_cast<uint32_t>(__popcll(vis & mine));
            no_point = no_point | ((zeros & mine) != 0ull);
            if constexpr (ROUNDS) shadow_next(Y, p, c);
        }
        const uint64_t own = first + static_cast<uint64_t>(lane);
        if (lane < Y.A.group && own < static_cast<uint64_t>(n)) {
            const uint32_t v = no_point ? static_cast<uint32_t>(Y.A.K) : count;
            if (visible) visible[own] = static_cast<uint16_t>(v);
            if (share) share[own] = static_cast<float>(v) / static_cast<float>(Y.A.K);
        }
    }
}

// ======================================================================================================
// One-bounce diffuse gather as a query (rt_indirect_diffuse_device; the indirect-diffuse section of include/rt_mi355x.h is the definition;
// DESIGN.md §5, Indirect diffuse).  A template for the same reason.
// ======================================================================================================
// k_gather: k_occlusion's mapping (a WAVE OWNS WHOLE POINTS, lane l of round r holds gather ray e = r * 64 + l of the unit, lane p keeps the
// result of point p; no atomics, no list, every output written once) with a RAY per lane instead of a segment: the direction is
// ao_direction's, the ray (P, d) is walked as k_closest walks it, and the lanes that hit shade their hit H by the light POSITIONS -- a
// wave-uniform loop over the lights, each one segment walk pos[l] -> H as k_segments walks it, skipped by ballot when no lane hit.  The
// face id is range-checked by found() before it indexes face_normal / mat_id (the material id was validated at upload).
// THE SUM IS IN ORDER: a point's rays sit in consecutive lanes with ascending k, and a point that straddles rounds continues in ascending
// k, so after each round every lane stores its radiance R in the wave's staging slice (3 x 64 floats of s_stage, which is free between
// walks; channel-major, so neither the stores nor the owners' loads meet in a bank) and the owner lane adds its point's lanes one by
// one, lowest first.  A float sum by ballots or by a butterfly would be a different sum.  ROUNDS = false: K divides 64, one round.  The
// lights are a kernel argument; the kernel reads the scene, the tables and its two input arrays alone.
template <bool ROUNDS>
__global__ __launch_bounds__(RT_WAVES * 64) void k_gather(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                        const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                        const DScene S, const DLights L, const int n, const float *__restrict__ point,
                                                        const float *__restrict__ normal, const float *__restrict__ dirs,
                                                        const float *__restrict__ rot, const int m, const uint32_t seed, float *__restrict__ rgb) {
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    static_assert(RT_STAGE_TRIS * 5 * sizeof(uint4) >= 3 * 64 * sizeof(float), "the staging slice of a wave holds its 64 radiances");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, s_stage + wave * RT_STAGE_TRIS * 5};
    float *const staged = reinterpret_cast<float *>(stk.stage);
    const DNode root = nodes[0];
    const AoLayout Y = ao_layout(m);                       // (the launcher picks ROUNDS = Y.rounds > 1)
    const int rounds = ROUNDS ? Y.rounds : 1;
    const int p0 = lane / Y.K, k0 = lane - p0 * Y.K;
    const uint64_t units = ao_units(n, Y), step = static_cast<uint64_t>(gridDim.x) * RT_WAVES;
    for (uint64_t unit = static_cast<uint64_t>(blockIdx.x) * RT_WAVES + static_cast<uint64_t>(wave); unit < units; unit += step) {
        const uint64_t first = unit * static_cast<uint64_t>(Y.group);
        float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f;
        int p = p0, k = k0;
        for (int round = 0; round < rounds; ++round) {
            const uint64_t pi = first + static_cast<uint64_t>(p);
            const bool has = pi < static_cast<uint64_t>(n);
            const size_t j = has ? ao_xyz(pi) : 0;
            const float px = point[j], py = point[j + 1], pz = point[j + 2];
            const float nx = normal[j], ny = normal[j + 1], nz = normal[j + 2];
            const bool zero = (nx == 0.0f) & (ny == 0.0f) & (nz == 0.0f);                  // (+-0 both compare equal to 0)
            const bool act = has & !zero;
            const uint32_t r = ao_hash(seed, static_cast<uint32_t>(pi)) >> 26;
            float dx, dy, dz;
            ao_direction(nx, ny, nz, dirs, k, rot[r * 2u], rot[r * 2u + 1u], dx, dy, dz);
            float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
            if (__ballot(act) != 0ull) {
                const WalkRay ray = trace_ray(px, py, pz, dx, dy, dz);
                uint32_t c0 = 0, c1 = 0;
                const Hit best = walk<false, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, act && root_hit(root, ray), ray, c0, c1);
                const bool hit = act && found(best.face, S.n_faces);
                if (__ballot(hit) != 0ull) {
                    const size_t f = hit ? static_cast<size_t>(best.face) : 0;             // (a lane without a hit reads face 0 and uses nothing of it)
                    const float t = hit ? best.t : 0.0f;
                    const float hx = px + t * dx, hy = py + t * dy, hz = pz + t * dz;
                    float fx = S.face_normal[f * 3u], fy = S.face_normal[f * 3u + 1u], fz = S.face_normal[f * 3u + 2u];
                    if ((fx * dx + fy * dy) + fz * dz > 0.0f) { fx = -fx; fy = -fy; fz = -fz; }
                    const rt_material *__restrict__ mat = S.mats + S.mat_id[f];
                    const float kd0 = mat->kd[0], kd1 = mat->kd[1], kd2 = mat->kd[2];
                    for (int l = 0; l < L.n_lights; ++l) {
                        const float lx = L.pos[l][0], ly = L.pos[l][1], lz = L.pos[l][2];
                        const WalkRay seg = segment_ray(lx, ly, lz, hx, hy, hz);
                        uint32_t w0 = 0, w1 = 0;
                        const bool occ = walk<true, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, hit && root_hit(root, seg), seg, w0, w1);
                        if (hit && !occ) {
                            float ldx = lx - hx, ldy = ly - hy, ldz = lz - hz;
                            normalize3(ldx, ldy, ldz);
                            const float ct = smax(0.0f, dot3(ldx, ldy, ldz, fx, fy, fz));
                            r0 = r0 + (L.color[0] * kd0) * ct; r1 = r1 + (L.color[1] * kd1) * ct; r2 = r2 + (L.color[2] * kd2) * ct;
                        }
                    }
                }
            }
            // the sum, in the definition's order: lane p adds the lanes of point p of this round, lowest first (misses and absent points add +0)
            __builtin_amdgcn_wave_barrier();
            staged[lane] = r0; staged[64 + lane] = r1; staged[128 + lane] = r2;
            __builtin_amdgcn_wave_barrier();
            const GatherRange mine = gather_range(Y, lane, round);                        // (empty for the lanes that own no point)
            for (int q = mine.first; q < mine.first + mine.count; ++q) { e0 = e0 + staged[q]; e1 = e1 + staged[64 + q]; e2 = e2 + staged[128 + q]; }
            __builtin_amdgcn_wave_barrier();
            if constexpr (ROUNDS) ao_next(Y, p, k);
        }
        const uint64_t own = first + static_cast<uint64_t>(lane);
        if (lane < Y.group && own < static_cast<uint64_t>(n)) {
            const size_t o = ao_xyz(own);
            const float fk = static_cast<float>(Y.K);
            rgb[o] = e0 / fk; rgb[o + 1] = e1 / fk; rgb[o + 2] = e2 / fk;
        }
    }
}

// ======================================================================================================
// Light probes as a query (rt_light_probes_device, rt_probe_irradiance_device; the light-probe section of include/rt_mi355x.h is the
// definition; DESIGN.md §5, Light probes).  Templates for the same reason.
// ======================================================================================================
// k_probes: k_gather's mapping (a wave owns `group` whole probes, lane l of round r holds ray e = r * 64 + l of the unit), its closest-hit
// walk and its wave-uniform light loop, over the whole sphere: the direction of ray k is table entry k as it is, the origin the probe.
// THE 27 SUMS of a probe are lane tasks (rt_probe_layout.hpp): after each round every lane stores its radiance in the wave's staging slice
// (lane-major, float lane * 3 + c: the stride 3 is odd, so the stores meet in no bank, and the three channels of one staged lane, which
// the tasks of one probe read together, lie in three banks), then the tasks of the probes that have lanes in this round -- 27 per probe,
// 64 at a time -- each add their probe's staged lanes lowest first, times W[k][j].  A round's probes are consecutive and only the last can go
// on into the next round, so what a wave carries across the walks of the next round is ONE probe's 27 running values, in s_carry (the
// staging slice belongs to the walks).  A sum that is complete takes the direct term, if asked for, and is stored: every output is written
// once, no atomics.  The direct term needs light l -> P judged by lightStrikes: lane p walks that segment for probe p ahead of the rounds
// and keeps the answers as bits of `seen`, which the task lanes fetch by a wave shuffle.  n_lights <= RT_MAX_LIGHTS = 25 bits.
template <bool ROUNDS>
__global__ __launch_bounds__(RT_WAVES * 64) void k_probes(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                        const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                        const DScene S, const DLights L, const int n, const float *__restrict__ position,
                                                        const float *__restrict__ dirs, const float *__restrict__ wts, const int m, const int direct,
                                                        float *__restrict__ coeff) {
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    __shared__ float s_carry[RT_WAVES * kProbeCoeffs];
    static_assert(RT_STAGE_TRIS * 5 * sizeof(uint4) >= 3 * 64 * sizeof(float), "the staging slice of a wave holds its 64 radiances");
    static_assert(RT_MAX_LIGHTS <= 32, "a probe's light bits fit a word");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, s_stage + wave * RT_STAGE_TRIS * 5};
    float *const staged = reinterpret_cast<float *>(stk.stage);
    float *const carry = s_carry + wave * kProbeCoeffs;
    const DNode root = nodes[0];
    const AoLayout Y = ao_layout(m);                       // (the launcher picks ROUNDS = Y.rounds > 1)
    const int rounds = ROUNDS ? Y.rounds : 1;
    const int p0 = lane / Y.K, k0 = lane - p0 * Y.K;
    const uint64_t units = ao_units(n, Y), step = static_cast<uint64_t>(gridDim.x) * RT_WAVES;
    for (uint64_t unit = static_cast<uint64_t>(blockIdx.x) * RT_WAVES + static_cast<uint64_t>(wave); unit < units; unit += step) {
        const uint64_t first = unit * static_cast<uint64_t>(Y.group);
        // the direct term's visibility: lane p judges the segments light l -> probe p, as k_segments walks them
        uint32_t seen = 0u;
        if (direct != 0) {
            const uint64_t own = first + static_cast<uint64_t>(lane);
            const bool mine = lane < Y.group && own < static_cast<uint64_t>(n);
            const size_t j = mine ? ao_xyz(own) : 0;
            const float px = position[j], py = position[j + 1], pz = position[j + 2];
            for (int l = 0; l < L.n_lights; ++l) {
                const WalkRay seg = segment_ray(L.pos[l][0], L.pos[l][1], L.pos[l][2], px, py, pz);
                uint32_t w0 = 0, w1 = 0;
                const bool occ = walk<true, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, mine && root_hit(root, seg), seg, w0, w1);
                if (mine && !occ) seen |= 1u << l;
            }
        }
        int p = p0, k = k0;
        for (int round = 0; round < rounds; ++round) {
            const uint64_t pi = first + static_cast<uint64_t>(p);
            const bool has = pi < static_cast<uint64_t>(n);
            const size_t j = has ? ao_xyz(pi) : 0;
            const float px = position[j], py = position[j + 1], pz = position[j + 2];
            const float dx = dirs[k * 3], dy = dirs[k * 3 + 1], dz = dirs[k * 3 + 2];
            float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
            {
                const WalkRay ray = trace_ray(px, py, pz, dx, dy, dz);
                uint32_t c0 = 0, c1 = 0;
                const Hit best = walk<false, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, has && root_hit(root, ray), ray, c0, c1);
                const bool hit = has && found(best.face, S.n_faces);
                if (__ballot(hit) != 0ull) {
                    const size_t f = hit ? static_cast<size_t>(best.face) : 0;             // (a lane without a hit reads face 0 and uses nothing of it)
                    const float t = hit ? best.t : 0.0f;
                    const float hx = px + t * dx, hy = py + t * dy, hz = pz + t * dz;
                    float fx = S.face_normal[f * 3u], fy = S.face_normal[f * 3u + 1u], fz = S.face_normal[f * 3u + 2u];
                    if ((fx * dx + fy * dy) + fz * dz > 0.0f) { fx = -fx; fy = -fy; fz = -fz; }
                    const rt_material *__restrict__ mat = S.mats + S.mat_id[f];
                    const float kd0 = mat->kd[0], kd1 = mat->kd[1], kd2 = mat->kd[2];
                    for (int l = 0; l < L.n_lights; ++l) {
                        const float lx = L.pos[l][0], ly = L.pos[l][1], lz = L.pos[l][2];
                        const WalkRay seg = segment_ray(lx, ly, lz, hx, hy, hz);
                        uint32_t w0 = 0, w1 = 0;
                        const bool occ = walk<true, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, hit && root_hit(root, seg), seg, w0, w1);
                        if (hit && !occ) {
                            float ldx = lx - hx, ldy = ly - hy, ldz = lz - hz;
                            normalize3(ldx, ldy, ldz);
                            const float ct = smax(0.0f, dot3(ldx, ldy, ldz, fx, fy, fz));
                            r0 = r0 + (L.color[0] * kd0) * ct; r1 = r1 + (L.color[1] * kd1) * ct; r2 = r2 + (L.color[2] * kd2) * ct;
                        }
                    }
                }
            }
            // the 27 sums of every probe with lanes in this round, in the definition's order (misses and absent probes add +0 * W)
            __builtin_amdgcn_wave_barrier();
            staged[lane * 3] = r0; staged[lane * 3 + 1] = r1; staged[lane * 3 + 2] = r2;
            __builtin_amdgcn_wave_barrier();
#ifndef RT_PROBES_NO_SUM                                   // (make ab AB_FLAGS=-DRT_PROBES_NO_SUM: the kernel without its sums, for tools/probes_timing.py)
            const ProbeSpan span = probe_span(Y, round);
            const int passes = probe_passes(span);
            float keep = 0.0f;
            int keep_jc = -1;
            for (int pass = 0; pass < passes; ++pass) {
                const ProbeTask task = probe_task(span, pass, lane);
                const uint32_t lit = static_cast<uint32_t>(__shfl(static_cast<int>(seen), task.live ? task.p : 0));      // (every lane takes part)
                if (task.live) {
                    const GatherRange mine = gather_range(Y, task.p, round);
                    const int jj = task.jc / 3, c = task.jc - jj * 3;
                    float v = (ROUNDS && probe_carried_in(Y, task.p, round)) ? carry[task.jc] : 0.0f;
                    const float *__restrict__ w = wts + mine.k0 * kProbeBasis + jj;
                    for (int q = 0; q < mine.count; ++q) v = v + staged[(mine.first + q) * 3 + c] * w[q * kProbeBasis];
                    if (!ROUNDS || probe_finished(Y, task.p, round)) {
                        const uint64_t own = first + static_cast<uint64_t>(task.p);
                        if (own < static_cast<uint64_t>(n)) {
                            if (lit != 0u) {
                                const size_t o = ao_xyz(own);
                                const float qx = position[o], qy = position[o + 1], qz = position[o + 2];
                                const float band = probe_direct_band(jj), col = L.color[c];
                                for (int l = 0; l < L.n_lights; ++l)
                                    if ((lit >> l) & 1u) {
                                        float wx = L.pos[l][0] - qx, wy = L.pos[l][1] - qy, wz = L.pos[l][2] - qz;
                                        normalize3(wx, wy, wz);
                                        v = v + col * (band * probe_sh9_at(jj, wx, wy, wz));
                                    }
                            }
                            coeff[probe_out(own) + static_cast<size_t>(task.jc)] = v;
                        }
                    } else {
                        keep = v; keep_jc = task.jc;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            if constexpr (ROUNDS) {
                if (keep_jc >= 0) carry[keep_jc] = keep;               // (behind every read of this round: one probe at most goes on)
                __builtin_amdgcn_wave_barrier();
                ao_next(Y, p, k);
            }
#else
            if (lane == 0 && has && round == rounds - 1) coeff[probe_out(pi)] = staged[0] + static_cast<float>(seen);
            __builtin_amdgcn_wave_barrier();
            if constexpr (ROUNDS) ao_next(Y, p, k);
#endif
        }
    }
}

// k_probe_lookup: lane = point, element-wise (probe_lookup of rt_probe_layout.hpp is the arithmetic, the checker's and the kernel's): the
// trilinear blend of the up to 8 probes round the point, evaluated at its normal.  It reads the grid's coefficients and its two inputs
// alone; 64-bit element indices; the rest of n by grid stride.
template <int = 0>
__global__ __launch_bounds__(256) void k_probe_lookup(const ProbeGrid G, const float *__restrict__ coeff, const int n, const float *__restrict__ point,
                                                     const float *__restrict__ normal, float *__restrict__ rgb) {
    const size_t total = static_cast<size_t>(n), step = static_cast<size_t>(gridDim.x) * 256u;
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x; i < total; i += step) {
        const size_t o = ao_xyz(i);
        float out[3];
        probe_lookup(G, coeff, point[o], point[o + 1], point[o + 2], normal[o], normal[o + 1], normal[o + 2], out);
        rgb[o] = out[0]; rgb[o + 1] = out[1]; rgb[o + 2] = out[2];
    }
}

// k_probe_lookup_visible: the lookup that asks the scene which probes a point sees (the leak-free section of include/rt_mi355x.h is the
// definition; probe_lookup_visible of rt_probe_layout.hpp is its arithmetic given the eight answers, and the mapping is described there).
// A wave owns 8 consecutive points; lane l walks the segment probe -> point of point l >> 3, corner l & 7, as k_segments walks light ->
// hit, and ONE ballot holds the 64 answers: byte p is the mask of point p.  Two more ballots (the corners read, those of weight > 0) let
// every lane decide its point's case, and a last one publishes the corners each blend takes.  The 8 x 27 blended coefficients are lane
// tasks, 64 at a time: a task reads its point's weights and probe indices, which their lanes left in the wave's staging slice (the walks are
// done with it), adds the corners in the definition's order and stores its sum in the same slice.  (A wave shuffle of the weights instead
// changed the register allocation of four k_stage variants compiled beside this kernel; the staged form leaves every other stream alone.)
// The 8 x 3 evaluations are tasks of the lanes (p, c < 3): nine terms in order, then the division in case B.  No atomics, no reduction
// across lanes; 64-bit element indices; the rest of the units by grid stride (ao_grid's rule).
template <int = 0>
__global__ __launch_bounds__(RT_WAVES * 64) void k_probe_lookup_visible(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                                      const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                                      const DScene S, const ProbeGrid G, const float *__restrict__ coeff, const int n,
                                                                      const float *__restrict__ point, const float *__restrict__ normal,
                                                                      float *__restrict__ rgb, uint8_t *__restrict__ mask) {
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    static_assert(RT_STAGE_TRIS * 5 * sizeof(uint4) >= kPvStageFloats * sizeof(float), "the staging slice of a wave holds its 216 blended coefficients");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, s_stage + wave * RT_STAGE_TRIS * 5};
    float *const staged = reinterpret_cast<float *>(stk.stage);
    int32_t *const staged_cell = reinterpret_cast<int32_t *>(stk.stage);
    const DNode root = nodes[0];
    const int pt = pv_lane_point(lane), b = pv_lane_corner(lane), own = lane & ~7;      // own: the first lane of this lane's point
    const uint32_t readable = probe_read_mask(G);
    const uint64_t units = pv_units(n), step = static_cast<uint64_t>(gridDim.x) * RT_WAVES;
    for (uint64_t unit = static_cast<uint64_t>(blockIdx.x) * RT_WAVES + static_cast<uint64_t>(wave); unit < units; unit += step) {
        const uint64_t i = unit * static_cast<uint64_t>(kPvPoints) + static_cast<uint64_t>(pt);
        const bool has = i < static_cast<uint64_t>(n);
        const size_t o = has ? ao_xyz(i) : 0;
        const float px = point[o], py = point[o + 1], pz = point[o + 2];
        const float nx = normal[o], ny = normal[o + 1], nz = normal[o + 2];
        const bool nop = (nx == 0.0f) & (ny == 0.0f) & (nz == 0.0f);
        const ProbeAxis ax = probe_axis(px, G.origin[0], G.step[0], G.dims[0]), ay = probe_axis(py, G.origin[1], G.step[1], G.dims[1]),
                        az = probe_axis(pz, G.origin[2], G.step[2], G.dims[2]);
        const float weight = probe_corner_weight(ax, ay, az, b);
        const bool read = has && !nop && ((readable >> b) & 1u) != 0u;
        const int32_t ix = ax.i0 + (b & 1), iy = ay.i0 + ((b >> 1) & 1), iz = az.i0 + (b >> 2);
        const int32_t cell = read ? probe_index(G, ix, iy, iz) : 0;               // (a corner that is not read has no index)
        // the segment probe -> point, judged as lightStrikes judges light -> hit
        const WalkRay seg = segment_ray(probe_position(G, 0, ix), probe_position(G, 1, iy), probe_position(G, 2, iz), px, py, pz);
        uint32_t w0 = 0, w1 = 0;
        const bool occ = walk<true, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, read && root_hit(root, seg), seg, w0, w1);
        const bool vis = read && !occ;
        const unsigned long long visb = __ballot(vis), readb = __ballot(read), posb = __ballot(weight > 0.0f);
        const uint32_t seen = static_cast<uint32_t>(visb >> own) & 0xffu;
        const ProbeUse u = probe_visible_use(static_cast<uint32_t>(readb >> own) & 0xffu, seen, static_cast<uint32_t>(posb >> own) & 0xffu);
        const unsigned long long useb = __ballot(((u.use >> b) & 1u) != 0u);
        if (mask != nullptr && has && b == 0) mask[i] = static_cast<uint8_t>(seen);
        // every lane's weight and probe index go to the staging slice, behind the sums: the tasks read those of their point from there
        __builtin_amdgcn_wave_barrier();
        staged[pv_stage_weight(lane)] = weight; staged_cell[pv_stage_cell(lane)] = cell;
        __builtin_amdgcn_wave_barrier();
        // W of this lane's point, the USED weights in order (every lane of the point forms it; the lanes c < 3 divide by it)
        float W = 0.0f;
        for (int k = 0; k < 8; ++k) {
            const float wk = staged[pv_stage_weight(own + k)];
            if ((u.use >> k) & 1u) W = W + wk;
        }
        // the 8 x 27 blended coefficients
#pragma unroll 1
        for (int pass = 0; pass < kPvPasses; ++pass) {
            const ProbeTask task = pv_task(pass, lane);
            const int src = task.live ? task.p * 8 : 0;
            const uint32_t use = task.live ? static_cast<uint32_t>(useb >> src) & 0xffu : 0u;
            float v = 0.0f;
            for (int k = 0; k < 8; ++k) {
                const float wk = staged[pv_stage_weight(src + k)];
                const int32_t ck = staged_cell[pv_stage_cell(src + k)];
                if ((use >> k) & 1u) v = v + wk * coeff[static_cast<size_t>(ck) * static_cast<size_t>(kProbeCoeffs) + static_cast<size_t>(task.jc)];
            }
            if (task.live) staged[pv_stage(task.p, task.jc)] = v;
        }
        __builtin_amdgcn_wave_barrier();
        // the 8 x 3 evaluations
        if (pv_final(lane) && has) {
            float s = 0.0f;
            if (!nop) {
                const float ex = normal[o], ey = normal[o + 1], ez = normal[o + 2];         // (read again: three registers fewer across the walk)
                for (int j = 0; j < kProbeBasis; ++j) s = s + staged[pv_stage(pt, j * 3 + b)] * probe_sh9_at(j, ex, ey, ez);
                if (u.divide) s = s / W;
            }
            rgb[o + static_cast<size_t>(b)] = s;
        }
        __builtin_amdgcn_wave_barrier();                   // (the next unit's walk stages over the sums)
    }
}

// ======================================================================================================
// Bounced light (rt_light_probes_bounce_device, rt_indirect_diffuse_bounce_device; the "bounced light" section of include/rt_mi355x.h is the
// definition; DESIGN.md §5, Bounced light).  k_gather and k_probes with ONE more term in the radiance of a hit: behind the last light, a
// lane that hit looks the SOURCE volume (G, src) up at its hit H with the turned face normal and adds kd * max(0, I).  The kernels are
// written out beside their parents, not as a further template parameter of them, so that the parents' instruction streams stay as they are.
// ======================================================================================================
// bounce_light: the term itself, called inside the parents' "some lane hit" branch, so a round without a hit walks and reads nothing.
// VISIBLE = false: a per-lane lookup from global memory (probe_bounce_lookup of rt_probe_layout.hpp: the streamed blend, three
// accumulators); neighbouring hits share the source's cache lines.  VISIBLE = true: ahead of it a WAVE-UNIFORM loop over the corners the
// grid reads (at most 8; the grid is a kernel argument, so the skip of a single-layer axis is a scalar branch), each ONE segment walk
// probe -> H as the light loop walks light -> H, in_root = hit && root_hit; a lane keeps its eight answers as bits of one register and
// probe_visible_use picks the corners of its blend.  A hit whose face normal is three +-0 is no point: no segment, I = 0, and the
// definition's R + kd * 0 is still formed.
template <bool VISIBLE>
__device__ __forceinline__ void bounce_light(const DNode &root, const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                             const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0, const DScene &S,
                                             const WaveStack &stk, const int lane, const ProbeGrid &G, const float *__restrict__ src, const bool hit,
                                             const float hx, const float hy, const float hz, const float fx, const float fy, const float fz,
                                             const float kd0, const float kd1, const float kd2, float &r0, float &r1, float &r2) {
    uint32_t vis = 0u;
    if constexpr (VISIBLE) {
        const bool pt = hit && !((fx == 0.0f) & (fy == 0.0f) & (fz == 0.0f));
        const uint32_t readable = probe_read_mask(G);
#pragma unroll 1
        for (int b = 0; b < 8; ++b) {
            if (((readable >> b) & 1u) == 0u) continue;
            float cx, cy, cz;
            probe_corner_position(G, hx, hy, hz, b, cx, cy, cz);
            const WalkRay seg = segment_ray(cx, cy, cz, hx, hy, hz);
            uint32_t w0 = 0, w1 = 0;
            const bool occ = walk<true, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, pt && root_hit(root, seg), seg, w0, w1);
            if (pt && !occ) vis |= 1u << b;
        }
    }
    if (hit) {
        float I[3];
        probe_bounce_lookup(G, src, hx, hy, hz, fx, fy, fz, VISIBLE, vis, I);
        r0 = probe_bounce_add(r0, kd0, I[0]); r1 = probe_bounce_add(r1, kd1, I[1]); r2 = probe_bounce_add(r2, kd2, I[2]);
    }
}

// k_gather_bounce: k_gather, line for line, with bounce_light behind the light loop.
template <bool ROUNDS, bool VISIBLE>
__global__ __launch_bounds__(RT_WAVES * 64) void k_gather_bounce(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                               const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                               const DScene S, const DLights L, const int n, const float *__restrict__ point,
                                                               const float *__restrict__ normal, const float *__restrict__ dirs,
                                                               const float *__restrict__ rot, const int m, const uint32_t seed, const ProbeGrid G,
                                                               const float *__restrict__ src, float *__restrict__ rgb) {
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    static_assert(RT_STAGE_TRIS * 5 * sizeof(uint4) >= 3 * 64 * sizeof(float), "the staging slice of a wave holds its 64 radiances");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, s_stage + wave * RT_STAGE_TRIS * 5};
    float *const staged = reinterpret_cast<float *>(stk.stage);
    const DNode root = nodes[0];
    const AoLayout Y = ao_layout(m);                       // (the launcher picks ROUNDS = Y.rounds > 1)
    const int rounds = ROUNDS ? Y.rounds : 1;
    const int p0 = lane / Y.K, k0 = lane - p0 * Y.K;
    const uint64_t units = ao_units(n, Y), step = static_cast<uint64_t>(gridDim.x) * RT_WAVES;
    for (uint64_t unit = static_cast<uint64_t>(blockIdx.x) * RT_WAVES + static_cast<uint64_t>(wave); unit < units; unit += step) {
        const uint64_t first = unit * static_cast<uint64_t>(Y.group);
        float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f;
        int p = p0, k = k0;
        for (int round = 0; round < rounds; ++round) {
            const uint64_t pi = first + static_cast<uint64_t>(p);
            const bool has = pi < static_cast<uint64_t>(n);
            const size_t j = has ? ao_xyz(pi) : 0;
            const float px = point[j], py = point[j + 1], pz = point[j + 2];
            const float nx = normal[j], ny = normal[j + 1], nz = normal[j + 2];
            const bool zero = (nx == 0.0f) & (ny == 0.0f) & (nz == 0.0f);                  // (+-0 both compare equal to 0)
            const bool act = has & !zero;
            const uint32_t r = ao_hash(seed, static_cast<uint32_t>(pi)) >> 26;
            float dx, dy, dz;
            ao_direction(nx, ny, nz, dirs, k, rot[r * 2u], rot[r * 2u + 1u], dx, dy, dz);
            float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
            if (__ballot(act) != 0ull) {
                const WalkRay ray = trace_ray(px, py, pz, dx, dy, dz);
                uint32_t c0 = 0, c1 = 0;
                const Hit best = walk<false, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, act && root_hit(root, ray), ray, c0, c1);
                const bool hit = act && found(best.face, S.n_faces);
                if (__ballot(hit) != 0ull) {
                    const size_t f = hit ? static_cast<size_t>(best.face) : 0;             // (a lane without a hit reads face 0 and uses nothing of it)
                    const float t = hit ? best.t : 0.0f;
                    const float hx = px + t * dx, hy = py + t * dy, hz = pz + t * dz;
                    float fx = S.face_normal[f * 3u], fy = S.face_normal[f * 3u + 1u], fz = S.face_normal[f * 3u + 2u];
                    if ((fx * dx + fy * dy) + fz * dz > 0.0f) { fx = -fx; fy = -fy; fz = -fz; }
                    const rt_material *__restrict__ mat = S.mats + S.mat_id[f];
                    const float kd0 = mat->kd[0], kd1 = mat->kd[1], kd2 = mat->kd[2];
                    for (int l = 0; l < L.n_lights; ++l) {
                        const float lx = L.pos[l][0], ly = L.pos[l][1], lz = L.pos[l][2];
                        const WalkRay seg = segment_ray(lx, ly, lz, hx, hy, hz);
                        uint32_t w0 = 0, w1 = 0;
                        const bool occ = walk<true, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, hit && root_hit(root, seg), seg, w0, w1);
                        if (hit && !occ) {
                            float ldx = lx - hx, ldy = ly - hy, ldz = lz - hz;
                            normalize3(ldx, ldy, ldz);
                            const float ct = smax(0.0f, dot3(ldx, ldy, ldz, fx, fy, fz));
                            r0 = r0 + (L.color[0] * kd0) * ct; r1 = r1 + (L.color[1] * kd1) * ct; r2 = r2 + (L.color[2] * kd2) * ct;
                        }
                    }
                    bounce_light<VISIBLE>(root, nodes, tris, chunks, leaf_chunk0, S, stk, lane, G, src, hit, hx, hy, hz, fx, fy, fz, kd0, kd1, kd2, r0, r1, r2);
                }
            }
            // the sum, in the definition's order: lane p adds the lanes of point p of this round, lowest first (misses and absent points add +0)
            __builtin_amdgcn_wave_barrier();
            staged[lane] = r0; staged[64 + lane] = r1; staged[128 + lane] = r2;
            __builtin_amdgcn_wave_barrier();
            const GatherRange mine = gather_range(Y, lane, round);                        // (empty for the lanes that own no point)
            for (int q = mine.first; q < mine.first + mine.count; ++q) { e0 = e0 + staged[q]; e1 = e1 + staged[64 + q]; e2 = e2 + staged[128 + q]; }
            __builtin_amdgcn_wave_barrier();
            if constexpr (ROUNDS) ao_next(Y, p, k);
        }
        const uint64_t own = first + static_cast<uint64_t>(lane);
        if (lane < Y.group && own < static_cast<uint64_t>(n)) {
            const size_t o = ao_xyz(own);
            const float fk = static_cast<float>(Y.K);
            rgb[o] = e0 / fk; rgb[o + 1] = e1 / fk; rgb[o + 2] = e2 / fk;
        }
    }
}

// k_probes_bounce: k_probes, line for line, with bounce_light behind the light loop.  The source is another array than coeff (the call
// refuses an output that shares a byte with it): an update in place would make a probe's answer depend on which waves had stored already.
template <bool ROUNDS, bool VISIBLE>
__global__ __launch_bounds__(RT_WAVES * 64) void k_probes_bounce(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                               const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                               const DScene S, const DLights L, const int n, const float *__restrict__ position,
                                                               const float *__restrict__ dirs, const float *__restrict__ wts, const int m, const int direct,
                                                               const ProbeGrid G, const float *__restrict__ src, float *__restrict__ coeff) {
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    __shared__ float s_carry[RT_WAVES * kProbeCoeffs];
    static_assert(RT_STAGE_TRIS * 5 * sizeof(uint4) >= 3 * 64 * sizeof(float), "the staging slice of a wave holds its 64 radiances");
    static_assert(RT_MAX_LIGHTS <= 32, "a probe's light bits fit a word");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, s_stage + wave * RT_STAGE_TRIS * 5};
    float *const staged = reinterpret_cast<float *>(stk.stage);
    float *const carry = s_carry + wave * kProbeCoeffs;
    const DNode root = nodes[0];
    const AoLayout Y = ao_layout(m);                       // (the launcher picks ROUNDS = Y.rounds > 1)
    const int rounds = ROUNDS ? Y.rounds : 1;
    const int p0 = lane / Y.K, k0 = lane - p0 * Y.K;
    const uint64_t units = ao_units(n, Y), step = static_cast<uint64_t>(gridDim.x) * RT_WAVES;
    for (uint64_t unit = static_cast<uint64_t>(blockIdx.x) * RT_WAVES + static_cast<uint64_t>(wave); unit < units; unit += step) {
        const uint64_t first = unit * static_cast<uint64_t>(Y.group);
        // the direct term's visibility: lane p judges the segments light l -> probe p, as k_segments walks them
        uint32_t seen = 0u;
        if (direct != 0) {
            const uint64_t own = first + static_cast<uint64_t>(lane);
            const bool mine = lane < Y.group && own < static_cast<uint64_t>(n);
            const size_t j = mine ? ao_xyz(own) : 0;
            const float px = position[j], py = position[j + 1], pz = position[j + 2];
            for (int l = 0; l < L.n_lights; ++l) {
                const WalkRay seg = segment_ray(L.pos[l][0], L.pos[l][1], L.pos[l][2], px, py, pz);
                uint32_t w0 = 0, w1 = 0;
                const bool occ = walk<true, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, mine && root_hit(root, seg), seg, w0, w1);
                if (mine && !occ) seen |= 1u << l;
            }
        }
        int p = p0, k = k0;
        for (int round = 0; round < rounds; ++round) {
            const uint64_t pi = first + static_cast<uint64_t>(p);
            const bool has = pi < static_cast<uint64_t>(n);
            const size_t j = has ? ao_xyz(pi) : 0;
            const float px = position[j], py = position[j + 1], pz = position[j + 2];
            const float dx = dirs[k * 3], dy = dirs[k * 3 + 1], dz = dirs[k * 3 + 2];
            float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
            {
                const WalkRay ray = trace_ray(px, py, pz, dx, dy, dz);
                uint32_t c0 = 0, c1 = 0;
                const Hit best = walk<false, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, has && root_hit(root, ray), ray, c0, c1);
                const bool hit = has && found(best.face, S.n_faces);
                if (__ballot(hit) != 0ull) {
                    const size_t f = hit ? static_cast<size_t>(best.face) : 0;             // (a lane without a hit reads face 0 and uses nothing of it)
                    const float t = hit ? best.t : 0.0f;
                    const float hx = px + t * dx, hy = py + t * dy, hz = pz + t * dz;
                    float fx = S.face_normal[f * 3u], fy = S.face_normal[f * 3u + 1u], fz = S.face_normal[f * 3u + 2u];
                    if ((fx * dx + fy * dy) + fz * dz > 0.0f) { fx = -fx; fy = -fy; fz = -fz; }
                    const rt_material *__restrict__ mat = S.mats + S.mat_id[f];
                    const float kd0 = mat->kd[0], kd1 = mat->kd[1], kd2 = mat->kd[2];
                    for (int l = 0; l < L.n_lights; ++l) {
                        const float lx = L.pos[l][0], ly = L.pos[l][1], lz = L.pos[l][2];
                        const WalkRay seg = segment_ray(lx, ly, lz, hx, hy, hz);
                        uint32_t w0 = 0, w1 = 0;
                        const bool occ = walk<true, false, false>(root, nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), LanePlane{}, hit && root_hit(root, seg), seg, w0, w1);
                        if (hit && !occ) {
                            float ldx = lx - hx, ldy = ly - hy, ldz = lz - hz;
                            normalize3(ldx, ldy, ldz);
                            const float ct = smax(0.0f, dot3(ldx, ldy, ldz, fx, fy, fz));
                            r0 = r0 + (L.color[0] * kd0) * ct; r1 = r1 + (L.color[1] * kd1) * ct; r2 = r2 + (L.color[2] * kd2) * ct;
                        }
                    }
                    bounce_light<VISIBLE>(root, nodes, tris, chunks, leaf_chunk0, S, stk, lane, G, src, hit, hx, hy, hz, fx, fy, fz, kd0, kd1, kd2, r0, r1, r2);
                }
            }
            // the 27 sums of every probe with lanes in this round, in the definition's order (misses and absent probes add +0 * W)
            __builtin_amdgcn_wave_barrier();
            staged[lane * 3] = r0; staged[lane * 3 + 1] = r1; staged[lane * 3 + 2] = r2;
            __builtin_amdgcn_wave_barrier();
            const ProbeSpan span = probe_span(Y, round);
            const int passes = probe_passes(span);
            float keep = 0.0f;
            int keep_jc = -1;
            for (int pass = 0; pass < passes; ++pass) {
                const ProbeTask task = probe_task(span, pass, lane);
                const uint32_t lit = static_cast<uint32_t>(__shfl(static_cast<int>(seen), task.live ? task.p : 0));      // (every lane takes part)
                if (task.live) {
                    const GatherRange mine = gather_range(Y, task.p, round);
                    const int jj = task.jc / 3, c = task.jc - jj * 3;
                    float v = (ROUNDS && probe_carried_in(Y, task.p, round)) ? carry[task.jc] : 0.0f;
                    const float *__restrict__ w = wts + mine.k0 * kProbeBasis + jj;
                    for (int q = 0; q < mine.count; ++q) v = v + staged[(mine.first + q) * 3 + c] * w[q * kProbeBasis];
                    if (!ROUNDS || probe_finished(Y, task.p, round)) {
                        const uint64_t own = first + static_cast<uint64_t>(task.p);
                        if (own < static_cast<uint64_t>(n)) {
                            if (lit != 0u) {
                                const size_t o = ao_xyz(own);
                                const float qx = position[o], qy = position[o + 1], qz = position[o + 2];
                                const float band = probe_direct_band(jj), col = L.color[c];
                                for (int l = 0; l < L.n_lights; ++l)
                                    if ((lit >> l) & 1u) {
                                        float wx = L.pos[l][0] - qx, wy = L.pos[l][1] - qy, wz = L.pos[l][2] - qz;
                                        normalize3(wx, wy, wz);
                                        v = v + col * (band * probe_sh9_at(jj, wx, wy, wz));
                                    }
                            }
                            coeff[probe_out(own) + static_cast<size_t>(task.jc)] = v;
                        }
                    } else {
                        keep = v; keep_jc = task.jc;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            if constexpr (ROUNDS) {
                if (keep_jc >= 0) carry[keep_jc] = keep;               // (behind every read of this round: one probe at most goes on)
                __builtin_amdgcn_wave_barrier();
                ao_next(Y, p, k);
            }
        }
    }
}

// ======================================================================================================
// Closest points (rt_closest_points_device; DESIGN.md §5, Closest points).  Templates for the same reason as the other query kernels.
// The query walks its OWN bounds (rt_distance_layout.hpp): NearNode, the exact vertex box of what is referenced below a node, and NearTri,
// the vertices of a leaf reference in the order of leaf_tris.  Two kernels make them once per uploaded scene, k_nearest reads them.
// ======================================================================================================
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
// wave-uniform loads of the two records, spelt out for the reason given at tri_load_uniform (both arrays are read-only while k_nearest runs)
__device__ __forceinline__ NearNode near_node_load_uniform(const NearNode *p) {
    u32x8 v;
    asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(v) : "s"(p) : "memory");
    NearNode n;
    n.lo[0] = __uint_as_float(v[0]); n.lo[1] = __uint_as_float(v[1]); n.lo[2] = __uint_as_float(v[2]); n.first = v[3];
    n.hi[0] = __uint_as_float(v[4]); n.hi[1] = __uint_as_float(v[5]); n.hi[2] = __uint_as_float(v[6]); n.count_flags = v[7];
    return n;
}
__device__ __forceinline__ NearTri near_tri_unpack(const u32x8 lo, const u32x4 hi) {
    NearTri t;
    t.a[0] = __uint_as_float(lo[0]); t.a[1] = __uint_as_float(lo[1]); t.a[2] = __uint_as_float(lo[2]);
    t.b[0] = __uint_as_float(lo[3]); t.b[1] = __uint_as_float(lo[4]); t.b[2] = __uint_as_float(lo[5]);
    t.c[0] = __uint_as_float(lo[6]); t.c[1] = __uint_as_float(lo[7]); t.c[2] = __uint_as_float(hi[0]);
    t.face = hi[1]; t.pad[0] = 0u; t.pad[1] = 0u;
    return t;
}
__device__ __forceinline__ NearTri near_tri_load_uniform(const NearTri *p) {
    u32x8 lo;
    u32x4 hi;
    asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dwordx4 %1, %2, 0x20\n\ts_waitcnt lgkmcnt(0)" : "=&s"(lo), "=&s"(hi) : "s"(p) : "memory");
    return near_tri_unpack(lo, hi);
}
// two consecutive records behind one wait
__device__ __forceinline__ void near_tri_load_uniform2(const NearTri *p, NearTri &a, NearTri &b) {
    u32x8 lo0, lo1;
    u32x4 hi0, hi1;
    asm volatile("s_load_dwordx8 %0, %4, 0x0\n\ts_load_dwordx4 %1, %4, 0x20\n\ts_load_dwordx8 %2, %4, 0x30\n\ts_load_dwordx4 %3, %4, 0x50\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(lo0), "=&s"(hi0), "=&s"(lo1), "=&s"(hi1) : "s"(p) : "memory");
    a = near_tri_unpack(lo0, hi0);
    b = near_tri_unpack(lo1, hi1);
}

// k_near_records: thread k copies the vertices of face leaf_tris[k].face into record k (the upload has checked the face ids; one that is
// out of range all the same gets NaN vertices: never a candidate).
template <int = 0>
__global__ __launch_bounds__(256) void k_near_records(const TriRec *__restrict__ leaf_tris, const float *__restrict__ tri_verts, const uint32_t n_refs,
                                                      const uint32_t n_faces, NearTri *__restrict__ out) {
    const size_t step = static_cast<size_t>(gridDim.x) * 256;
    for (size_t k = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; k < n_refs; k += step) {
        const uint32_t f = leaf_tris[k].face;
        float v[9];
        for (int q = 0; q < 9; ++q) v[q] = f < n_faces ? tri_verts[static_cast<size_t>(f) * 9 + q] : __uint_as_float(0x7fc00000u);
        uint4 *__restrict__ o = reinterpret_cast<uint4 *>(out + k);
        o[0] = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
        o[1] = make_uint4(__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7]));
        o[2] = make_uint4(__float_as_uint(v[8]), f, 0u, 0u);
    }
}

// k_near_leaf_boxes: a wave per node.  A leaf: chunk by chunk lane l takes record l of the chunk and the wave reduces the six bounds to the
// chunk's box (chunk_out[leaf_chunk0[node] + c], n_chunks of them in all); the leaf's box is their union.  An inner node: the empty box.
// first / count_flags are the node's own (the bottom-up pass on the host completes the inner boxes).
template <int = 0>
__global__ __launch_bounds__(256) void k_near_leaf_boxes(const DNode *__restrict__ nodes, const uint32_t *__restrict__ leaf_chunk0,
                                                         const NearTri *__restrict__ recs, const uint32_t n_nodes, const uint32_t n_refs,
                                                         const uint32_t n_chunks, NearNode *__restrict__ out, NearNode *__restrict__ chunk_out) {
    const int lane = threadIdx.x & 63;
    const uint32_t step = gridDim.x * 4u;
    for (uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6); j < n_nodes; j += step) {
        NearNode n;
        n.first = nodes[j].first; n.count_flags = nodes[j].count_flags;
        near_box_clear(n);
        if (near_is_leaf(n)) {
            const uint32_t cnt = near_leaf_count(n), c0 = leaf_chunk0[j];
            for (uint32_t c = 0; c < near_chunks(cnt); ++c) {
                NearNode cb;
                cb.first = n.first + c * kNearChunk; cb.count_flags = near_min_u32(cnt - c * kNearChunk, kNearChunk);
                near_box_clear(cb);
                const uint64_t r = static_cast<uint64_t>(cb.first) + static_cast<uint32_t>(lane);
                if (static_cast<uint32_t>(lane) < cb.count_flags && r < n_refs) near_box_add(cb, recs[r]);
                for (int off = 32; off > 0; off >>= 1)
                    for (int q = 0; q < 3; ++q) {
                        cb.lo[q] = near_min(cb.lo[q], __shfl_xor(cb.lo[q], off, 64));
                        cb.hi[q] = near_max(cb.hi[q], __shfl_xor(cb.hi[q], off, 64));
                    }
                if (lane == 0 && static_cast<uint64_t>(c0) + c < n_chunks) chunk_out[c0 + c] = cb;
                if (!near_empty(cb)) { near_box_add(n, cb.lo[0], cb.lo[1], cb.lo[2]); near_box_add(n, cb.hi[0], cb.hi[1], cb.hi[2]); }
            }
        }
        if (lane == 0) out[j] = n;
    }
}

// minimum of a wave's unsigned values, wave-uniform
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return uniform_u32(v);
}

// k_nearest: lane = point, the wave walks the tree together with a per-wave LDS stack of (node, lane mask).  A lane's best starts at the
// radius (r2 = max_dist * max_dist), so a small radius prunes from the root down.  An entry is tested against the lanes' bests of the
// moment when it is POPPED (they shrink while it waits).  At an inner node every child's box comes in by a uniform load, each lane forms
// its own lower bound, the child is kept for the lanes that cannot prune it, and the kept children are pushed so that the one nearest to
// the wave (the minimum of the kept lanes' bounds) is popped first: lane k < 8 holds child k's key and mask and finds its own slot by
// counting the children that go below it.  At a leaf the lanes step through the records by uniform loads, two per wait, every live lane
// against every record of a chunk; a leaf of several 64-record chunks tests each chunk's own box first and skips the chunk wave-uniformly when
// no live lane can improve in it (chunks / chunk0: those boxes, numbered as the upload numbers a leaf's chunks).  The answer is a minimum under a total order (near_better), so
// neither the order of the walk nor the make-up of the wave can change it.  Element indices are 64-bit.
template <int = 0>
__global__ __launch_bounds__(RT_WAVES * 64) void k_nearest(const NearNode *__restrict__ nodes, const NearTri *__restrict__ tris,
                                                         const NearNode *__restrict__ chunks, const uint32_t *__restrict__ chunk0, const float extent, const int n, const float *__restrict__ pin, const float r2, int32_t *__restrict__ face,
                                                         float *__restrict__ dist2, float *__restrict__ point) {
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *const stk_node = s_node + wave * RT_STACK;
    unsigned long long *const stk_mask = s_mask + wave * RT_STACK;
    const size_t total = static_cast<size_t>(n), step = static_cast<size_t>(gridDim.x) * RT_WAVES * 64;
    for (size_t base = (static_cast<size_t>(blockIdx.x) * RT_WAVES + static_cast<size_t>(wave)) * 64; base < total; base += step) {
        const size_t i = base + static_cast<size_t>(lane);
        const bool valid = i < total;
        const size_t j = valid ? i : 0;
        const float px = pin[near_out3(j)], py = pin[near_out3(j) + 1], pz = pin[near_out3(j) + 2];
        const float sigma = near_sigma(extent, px, py, pz);
        NearBest best = near_none(px, py, pz);
        int sp = 1;
        const unsigned long long all = __ballot(valid);
        if (lane == 0) { stk_node[0] = 0u; stk_mask[0] = all; }
        while (sp > 0) {
            --sp;
            const uint32_t ni = uniform_u32(stk_node[sp]);
            const unsigned long long m = uniform_u64(stk_mask[sp]);
            const NearNode nd = near_node_load_uniform(nodes + ni);
            if (near_empty(nd)) continue;
            const bool live = ((m >> lane) & 1ull) != 0ull && !near_pruned(near_box_bound2(nd.lo, nd.hi, px, py, pz, sigma), near_limit(best, r2));
            if (__ballot(live) == 0ull) continue;
            if (near_is_leaf(nd)) {
                const uint32_t cnt = near_leaf_count(nd);
                const NearTri *T = tris + nd.first;
                const NearNode *const CB = cnt > kNearChunk ? chunks + uniform_u32(chunk0[ni]) : nullptr;
                for (uint32_t c = 0; c < near_chunks(cnt); ++c) {
                    bool take = live;
                    if (CB) {            // a chunk that no live lane can improve in is skipped
                        const NearNode cb = near_node_load_uniform(CB + c);
                        take = live && !near_pruned(near_box_bound2(cb.lo, cb.hi, px, py, pz, sigma), near_limit(best, r2));
                        if (__ballot(take) == 0ull) continue;
                    }
                    const uint32_t end = near_min_u32(cnt, (c + 1u) * kNearChunk);
                    uint32_t k = c * kNearChunk;
                    for (; k + 2u <= end; k += 2u) {
                        NearTri ta, tb;
                        near_tri_load_uniform2(T + k, ta, tb);
                        const NearClosest ca = near_point_triangle(px, py, pz, ta), cb = near_point_triangle(px, py, pz, tb);
                        if (take) { near_take(best, ca, ta.face, r2); near_take(best, cb, tb.face, r2); }
                    }
                    if (k < end) {
                        const NearTri ta = near_tri_load_uniform(T + k);
                        const NearClosest ca = near_point_triangle(px, py, pz, ta);
                        if (take) near_take(best, ca, ta.face, r2);
                    }
                }
                continue;
            }
            const uint32_t kids = near_child_count(nd) < 8u ? near_child_count(nd) : 8u;
            const float limit = near_limit(best, r2);
            uint32_t my_key = 0u;
            unsigned long long my_mask = 0ull;
            for (uint32_t k = 0; k < kids; ++k) {
                const NearNode ch = near_node_load_uniform(nodes + nd.first + k);
                if (near_empty(ch)) continue;
                const float b2 = near_box_bound2(ch.lo, ch.hi, px, py, pz, sigma);
                const bool keep = live && !near_pruned(b2, limit);
                const unsigned long long km = __ballot(keep);
                if (km == 0ull) continue;
                const uint32_t key = wave_min_u32(keep ? __float_as_uint(b2) : 0xffffffffu);
                if (lane == static_cast<int>(k)) { my_key = key; my_mask = km; }
            }
            const uint32_t kept = static_cast<uint32_t>(__ballot(my_mask != 0ull));          // bit k: child k is kept (lanes 0 .. 7)
            const int add = __popc(kept);
            // An inner node pops one entry and pushes at most 8, so sp <= 7 * depth + 8 <= 113 at the depth <= 15 that rt_upload_scene
            // enforces (RT_STACK is 128).  The test below is a memory guard only: it cannot fire on an uploaded tree, and if it did the
            // children would be lost without a sign -- near_walk carries the same guard with a flag that distance_check asserts on.
            if (add == 0 || sp + add > RT_STACK) continue;
            // farthest first: child k goes above every kept child with a larger key, and above those with its own key and a lower index
            int below = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t kk = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(my_key), k));
                if (((kept >> k) & 1u) != 0u && (kk > my_key || (kk == my_key && k < lane))) ++below;
            }
            if (my_mask != 0ull) { stk_node[sp + below] = nd.first + static_cast<uint32_t>(lane); stk_mask[sp + below] = my_mask; }
            sp += add;
        }
        if (valid) {
            if (face) face[i] = best.face == kNearNoFace ? -1 : static_cast<int32_t>(best.face);
            if (dist2) dist2[i] = best.d2;
            if (point) { point[near_out3(i)] = best.q[0]; point[near_out3(i) + 1] = best.q[1]; point[near_out3(i) + 2] = best.q[2]; }
        }
    }
}

// ======================================================================================================
// Ordered ray hits (rt_ray_hits_device; DESIGN.md §5, Ordered ray hits).  The walk below is the sibling of packet_walk / leaf_visit for
// a lane that keeps a sorted list (rt_hits_layout.hpp: N = K + 1 entries in registers) instead of one best hit: the same wave stack, the
// reference's boxes through box_hit_verified, the same choice between the two leaf mappings and the same triangle statements, so a face's t
// is the same bits here, in k_closest and in either mapping.  What it leaves out is what a stream query never uses: leaf tasks, the cone
// test, the counters of the reference's steps.  The conservative tests (content boxes, chunk boxes) are bounded by the t of the list's
// LAST entry: t_max while fewer than K + 1 hits are held, the (K + 1)-th smallest from then on.  What they skip holds only hits beyond
// that entry, which change neither the K slots nor min(H, K + 1); the slack is the closest-hit walk's.
// ======================================================================================================
template <int N>
__device__ __forceinline__ bool hits_out_of_reach(const float tin, const float tout, const HitList<N> &L) {
    const float bound = L.t[N - 1];
    return (tin > tout) || (tout < -1e-3f) || (tin > bound + 1e-3f * (1.0f + fabsf(bound)));
}

template <int N>
__device__ __forceinline__ void hits_leaf_visit(const DNode &nd, const TriRec *__restrict__ tris, const ChunkBound *__restrict__ chunks,
                                                const WaveStack stk, const int lane, const RayLane &R, const float t_max,
                                                const unsigned long long live, const bool mine, HitList<N> &L) {
    const float ox = R.ox, oy = R.oy, oz = R.oz, dx = R.dx, dy = R.dy, dz = R.dz;
    const float idx_ = R.idx, idy_ = R.idy, idz_ = R.idz, slab_pad = R.slab_pad;
    const uint32_t cnt = nd.count_flags & 0x7fffffffu;
    const TriRec *__restrict__ T = tris + nd.first;
    const uint32_t nchunk = (cnt + 63u) >> 6;
    // the mode rule of leaf_visit (kernels with the staging buffer)
    const bool tri_mode = nchunk * RT_COST_CHUNK_TEST + static_cast<uint32_t>(__popcll(live)) * ((nchunk + 2u) / 3u) * RT_COST_TRI_MODE
                          < cnt * RT_COST_RAY_MODE;
    RT_PROF_ADD(lane, tri_mode ? WORK_LEAVES_LANES_TRIANGLES : WORK_LEAVES_LANES_RAYS, 1);
    if (tri_mode) {
        // ---- lanes = triangles: a lane holds one triangle of the chunk, the live rays are broadcast one at a time, and the hits of a
        // ballot go into the list of the ray's own lane
        const ChunkBound *__restrict__ cbounds = chunks + nd.pad[0];
        TriRec tr = T[static_cast<uint32_t>(lane) < cnt ? static_cast<uint32_t>(lane) : 0u];
        for (uint32_t c0 = 0u; c0 < cnt; c0 += 64u) {
            const uint32_t n = cnt - c0 < 64u ? cnt - c0 : 64u;
            const bool has = static_cast<uint32_t>(lane) < n;
            unsigned long long todo = live;
            const ChunkBound bd = cbounds[c0 >> 6];
            if (bd.never < 1.5f) {
                const float t0x = (bd.lo[0] - slab_pad - ox) * idx_, t1x = (bd.hi[0] + slab_pad - ox) * idx_;
                const float t0y = (bd.lo[1] - slab_pad - oy) * idy_, t1y = (bd.hi[1] + slab_pad - oy) * idy_;
                const float t0z = (bd.lo[2] - slab_pad - oz) * idz_, t1z = (bd.hi[2] + slab_pad - oz) * idz_;
                const float tin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
                const float tout = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
                todo = live & ~__ballot(hits_out_of_reach(tin, tout, L));
            }
            while (todo != 0ull) {
                const int r = static_cast<int>(__builtin_ctzll(todo));
                todo &= todo - 1ull;
                RT_PROF_ADD(lane, WORK_TRI_STEPS_LANES_TRIANGLES, 1);
                // Flyscene::rayTriangleIntersection, flyscene.cpp:787-819 (the statement of leaf_visit's lanes = triangles step)
                const float rdx = lane_f(dx, r), rdy = lane_f(dy, r), rdz = lane_f(dz, r);
                const float rox = lane_f(ox, r), roy = lane_f(oy, r), roz = lane_f(oz, r);
                const float dn = dot3(rdx, rdy, rdz, tr.nx, tr.ny, tr.nz);
                const float t = (tr.nA - dot3(rox, roy, roz, tr.nx, tr.ny, tr.nz)) / dn;
                const float v2x = (rox + t * rdx) - tr.ax, v2y = (roy + t * rdy) - tr.ay, v2z = (roz + t * rdz) - tr.az;
                const float d02 = dot3(tr.e0x, tr.e0y, tr.e0z, v2x, v2y, v2z);
                const float d12 = dot3(tr.e1x, tr.e1y, tr.e1z, v2x, v2y, v2z);
                const float u = (tr.d11 * d02 - tr.d01 * d12) * tr.inv_denom;
                const float v = (tr.d00 * d12 - tr.d01 * d02) * tr.inv_denom;
                // (a hit behind the ray's last entry cannot enter its list; one AT it can, by its face)
                const bool in = has && (dn != 0) && (u >= 0) && (v >= 0) && (u + v < 1) && hit_in_range(t, t_max) && (t <= lane_f(L.t[N - 1], r));
                unsigned long long hm = __ballot(in);
                while (hm != 0ull) {
                    const int l = static_cast<int>(__builtin_ctzll(hm));
                    hm &= hm - 1ull;
                    hits_insert(L, lane == r, lane_f(t, l), __builtin_amdgcn_readlane(static_cast<int>(tr.face), l));
                }
            }
            { const uint32_t nx = c0 + 64u + static_cast<uint32_t>(lane); if (c0 + 64u < cnt) tr = T[nx < cnt ? nx : 0u]; }
        }
    } else {
        // ---- lanes = rays: scalar records for small leaves, chunks staged in the wave's LDS buffer for larger ones
        auto test_lane = [&](const TriRec &tr) {
            // Flyscene::rayTriangleIntersection, flyscene.cpp:787-819 (the statement of leaf_visit's lanes = rays step)
            const float dn = dot3(dx, dy, dz, tr.nx, tr.ny, tr.nz);
            const float t = (tr.nA - dot3(ox, oy, oz, tr.nx, tr.ny, tr.nz)) / dn;
            const float v2x = (ox + t * dx) - tr.ax, v2y = (oy + t * dy) - tr.ay, v2z = (oz + t * dz) - tr.az;
            const float d02 = dot3(tr.e0x, tr.e0y, tr.e0z, v2x, v2y, v2z);
            const float d12 = dot3(tr.e1x, tr.e1y, tr.e1z, v2x, v2y, v2z);
            const float u = (tr.d11 * d02 - tr.d01 * d12) * tr.inv_denom;
            const float v = (tr.d00 * d12 - tr.d01 * d02) * tr.inv_denom;
            const bool in = mine && (dn != 0) && (u >= 0) && (v >= 0) && (u + v < 1) && hit_in_range(t, t_max) && (t <= L.t[N - 1]);
            if (__ballot(in) != 0ull) hits_insert(L, in, t, static_cast<int>(tr.face));      // (wave-uniform: most triangles are hit by no ray of the wave)
        };
        if (cnt <= RT_SCALAR_LEAF_MAX) {
            uint32_t k = 0;
            for (; k + 1u < cnt; k += 2u) {
                TriRec ta, tb;
                tri_load_uniform2(T + k, ta, tb);
                RT_PROF_ADD(lane, WORK_TRI_STEPS_LANES_RAYS, 2);
                test_lane(ta);
                test_lane(tb);
            }
            if (k < cnt) {
                RT_PROF_ADD(lane, WORK_TRI_STEPS_LANES_RAYS, 1);
                test_lane(tri_load_uniform(T + k));
            }
        } else {
            for (uint32_t c0 = 0u; c0 < cnt; c0 += RT_STAGE_TRIS) {
                const uint32_t n = cnt - c0 < RT_STAGE_TRIS ? cnt - c0 : RT_STAGE_TRIS;
                const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(T + c0);
                __builtin_amdgcn_wave_barrier();
                for (uint32_t q = static_cast<uint32_t>(lane); q < n * 5u; q += 64u) stk.stage[q] = src[q];
                __builtin_amdgcn_wave_barrier();
                const TriRec *staged = reinterpret_cast<const TriRec *>(stk.stage);
                RT_PROF_ADD(lane, WORK_TRI_STEPS_LANES_RAYS, n);
                for (uint32_t k = 0; k < n; ++k) test_lane(staged[k]);
            }
        }
    }
}

template <int N>
__device__ __forceinline__ void hits_walk(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris, const ChunkBound *__restrict__ chunks,
                                          const float extent, const WaveStack stk, const int lane, const bool in_root, const WalkRay &ray,
                                          const float t_max, HitList<N> &L) {
    const RayLane R = make_ray_lane(ray, extent);
    const float ox = R.ox, oy = R.oy, oz = R.oz, idx_ = R.idx, idy_ = R.idy, idz_ = R.idz, slab_pad = R.slab_pad;
    int sp = 0;
    {
        const unsigned long long m0 = __ballot(in_root);
        if (m0 == 0ull) return;
        stk.node[0] = 0u;
        stk.mask[0] = m0;
        sp = 1;
    }
    while (sp > 0) {
        --sp;
        __builtin_amdgcn_wave_barrier();
        const uint32_t ni = uniform_u32(stk.node[sp]);
        const unsigned long long m = uniform_u64(stk.mask[sp]);
        const bool mine = ((m >> lane) & 1ull) != 0ull;
        const unsigned long long live = m;
        if (live == 0ull) continue;
        const DNode nd = nodes[ni];
        const uint32_t cnt = nd.count_flags & 0x7fffffffu;
        if (nd.count_flags & RT_NODE_LEAF) {
            hits_leaf_visit(nd, tris, chunks, stk, lane, R, t_max, live, mine, L);
        } else {
            for (uint32_t c = 0; c < cnt; ++c) {
                const uint32_t ci = nd.first + c;
                const DNode ch = nodes[ci];
                bool h = mine;
                if (ch.pad[1] == 0u) {
                    // content test (as packet_walk): no point of the line that could still enter the list lies in the subtree's content box
                    const float t0x = (ch.clo[0] - slab_pad - ox) * idx_, t1x = (ch.chi[0] + slab_pad - ox) * idx_;
                    const float t0y = (ch.clo[1] - slab_pad - oy) * idy_, t1y = (ch.chi[1] + slab_pad - oy) * idy_;
                    const float t0z = (ch.clo[2] - slab_pad - oz) * idz_, t1z = (ch.chi[2] + slab_pad - oz) * idz_;
                    const float tin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
                    const float tout = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
                    h = h && !hits_out_of_reach(tin, tout, L);
                    if (__ballot(h) == 0ull) continue;
                }
                h = h && box_hit_verified(ch.bmin, ox, oy, oz, ray.bx, ray.by, ray.bz, ray.brx, ray.bry, ray.brz);   // BoundingBox::boxIntersect, exact
                RT_PROF_ADD(lane, WORK_BOX_STEPS_STACK_WALK, 1);
                const unsigned long long hm = __ballot(h);
                if (hm != 0ull) {
                    stk.node[sp] = ci;           // same value from every lane
                    stk.mask[sp] = hm;
                    ++sp;
                }
            }
        }
    }
}

// k_ray_hits<K>: lane = ray (org[i], dir[i]), k <= K output slots per ray.  The root test on (o, o + d) as k_closest makes it, the walk
// above with K + 1 entries, then the output rule of rt_hits_layout.hpp: face / t rows of k slots, count = min(H, k + 1); any of the three
// may be null.  It reads the scene alone.  Element indices are 64-bit.
template <int K>
__global__ __launch_bounds__(RT_WAVES * 64) void k_ray_hits(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                          const ChunkBound *__restrict__ chunks, const DScene S, const int n,
                                                          const float *__restrict__ org, const float *__restrict__ dir, const int k, const float t_max,
                                                          int32_t *__restrict__ face, float *__restrict__ t, int32_t *__restrict__ count) {
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, s_stage + wave * RT_STAGE_TRIS * 5};
    const DNode root = nodes[0];
    const size_t total = static_cast<size_t>(n), step = static_cast<size_t>(gridDim.x) * RT_WAVES * 64, slots = static_cast<size_t>(k);
    for (size_t base = (static_cast<size_t>(blockIdx.x) * RT_WAVES + static_cast<size_t>(wave)) * 64; base < total; base += step) {
        const size_t i = base + static_cast<size_t>(lane);
        const bool valid = i < total;
        const size_t j = valid ? i : 0;
        const WalkRay ray = trace_ray(org[j * 3], org[j * 3 + 1], org[j * 3 + 2], dir[j * 3], dir[j * 3 + 1], dir[j * 3 + 2]);
        HitList<K + 1> L;
        hits_clear(L, t_max);
        hits_walk(nodes, tris, chunks, S.extent, stk, lane, valid && root_hit(root, ray), ray, t_max, L);
        if (valid) hits_store(L, k, face ? face + i * slots : nullptr, t ? t + i * slots : nullptr, count ? count + i : nullptr);
    }
}

// ======================================================================================================
// Unit-parity probes (rt_box_intersect / rt_tree_probe / rt_primary_points): the PRODUCT's device functions on caller-given inputs,
// so that tests can pin them directly to outputs of the reference's own boundingBox.cpp / boxTree.cpp / camera.hpp.
// ======================================================================================================
__global__ __launch_bounds__(256) void k_box_probe(const int n, const float *__restrict__ box, const float *__restrict__ org, const float *__restrict__ dst,
                                                   uint8_t *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float b[6] = {box[i * 6], box[i * 6 + 1], box[i * 6 + 2], box[i * 6 + 3], box[i * 6 + 4], box[i * 6 + 5]};
    const float ox = org[i * 3], oy = org[i * 3 + 1], oz = org[i * 3 + 2];
    const float dx = dst[i * 3] - ox, dy = dst[i * 3 + 1] - oy, dz = dst[i * 3 + 2] - oz;        // Eigen: dir = dest - origin (boundingBox.cpp:51)
    out[i] = box_hit_verified(b, ox, oy, oz, dx, dy, dz, __builtin_amdgcn_rcpf(dx), __builtin_amdgcn_rcpf(dy), __builtin_amdgcn_rcpf(dz)) ? 1 : 0;
}

// phong_sample -- the per-sample arithmetic of k_shade / k_deep: normalize3_shared twice, pow_shininess with its tables in LDS -- one case per
// lane, whole waves (n is a multiple of 64), so that a test chooses which lanes share a wave and with it the side of every wave-uniform test.
// in[i * 20 ..]: hit point, normal (used as given), eye vector, sample position, lkd[3], lks[3], shininess, one pad;
// out[i * 6 ..]: ldn, cosphi, pw, tr, tg, tb.
__global__ __launch_bounds__(256) void k_phong_probe(const int n, const float *__restrict__ in, float *__restrict__ out) {
    __shared__ double s_pow[RT_POW_TAB];
    pow_tables_to_lds(s_pow);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;                       // (whole waves leave: n is a multiple of 64)
    const float *c = in + static_cast<size_t>(i) * 20;
    ShadeHit H;
    H.hx = c[0]; H.hy = c[1]; H.hz = c[2]; H.nx = c[3]; H.ny = c[4]; H.nz = c[5]; H.ex = c[6]; H.ey = c[7]; H.ez = c[8];
    H.fnx = 0.f; H.fny = 0.f; H.fnz = 0.f;
    H.mat = rt_material{};
    H.mat.shininess = c[18];
    float tr_, tg_, tb_, ldn, cosphi, pw;
    phong_sample(H, c[9], c[10], c[11], c[12], c[13], c[14], c[15], c[16], c[17], s_pow, tr_, tg_, tb_, ldn, cosphi, pw);
    float *o = out + static_cast<size_t>(i) * 6;
    o[0] = ldn; o[1] = cosphi; o[2] = pw; o[3] = tr_; o[4] = tg_; o[5] = tb_;
}

// BoxTree::intersect (boxTree.cpp:150-173) as the traversal kernels perform it, reference semantics (COUNT variant: no early-out, no
// culling): per ray the boxIntersect calls, the leaf face references and a signature of the set of intersected non-empty leaves
// (sum of device node index x 2654435761 mod 2^32).
__global__ __launch_bounds__(RT_WAVES * 64) void k_tree_probe(const DNode *__restrict__ nodes, const TriRec *__restrict__ tris,
                                                              const ChunkBound *__restrict__ chunks, const uint32_t *__restrict__ leaf_chunk0,
                                                              const DScene S, const int n, const float *__restrict__ org, const float *__restrict__ dst,
                                                              uint32_t *__restrict__ out_box, uint32_t *__restrict__ out_ref, uint32_t *__restrict__ out_sig) {
    __shared__ uint4 s_stage[RT_WAVES * RT_STAGE_TRIS * 5];
    __shared__ unsigned long long s_mask[RT_WAVES * RT_STACK];
    __shared__ uint32_t s_node[RT_WAVES * RT_STACK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveStack stk{s_node + wave * RT_STACK, s_mask + wave * RT_STACK, s_stage + wave * RT_STAGE_TRIS * 5};
    const DNode root = nodes[0];
    const int waves_total = gridDim.x * RT_WAVES;
    for (int base = (blockIdx.x * RT_WAVES + wave) * 64; base < n; base += waves_total * 64) {
        const int i = base + lane;
        const bool valid = i < n;
        const int j = valid ? i : 0;
        const float ox = org[j * 3], oy = org[j * 3 + 1], oz = org[j * 3 + 2];
        const WalkRay ray = segment_ray(ox, oy, oz, dst[j * 3], dst[j * 3 + 1], dst[j * 3 + 2]);
        // BoxTree::intersect tests the root itself first (the callers' own pre-test of the root is theirs, not part of intersect)
        const bool in_root = valid && root_hit(root, ray);
        uint32_t c_box = 0, c_ref = 0, c_sig = 0;
        packet_walk<true, true>(nodes, tris, chunks, leaf_chunk0, S.extent, stk, lane, walk_plain(), in_root, ray, c_box, c_ref, c_sig);
        if (valid) { out_box[i] = c_box + (in_root ? 0u : 1u); out_ref[i] = c_ref; out_sig[i] = c_sig; }
    }
}

__global__ __launch_bounds__(256) void k_primary_probe(const DCam *__restrict__ camp, const int W, const int H, float *__restrict__ out) {
    const DCam cam = *camp;
    const size_t total = static_cast<size_t>(W) * static_cast<size_t>(H);
    for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < total; p += static_cast<size_t>(gridDim.x) * blockDim.x) {
        float sx, sy, sz;
        screen_point(cam, static_cast<int>(p % static_cast<size_t>(W)), static_cast<int>(p / static_cast<size_t>(W)), sx, sy, sz);
        out[p * 3] = sx; out[p * 3 + 1] = sy; out[p * 3 + 2] = sz;
    }
}

void launch_box_probe(hipStream_t st, int n, const float *box, const float *org, const float *dst, uint8_t *out) {
    hipLaunchKernelGGL(k_box_probe, dim3((n + 255) / 256), dim3(256), 0, st, n, box, org, dst, out);
}
void launch_phong_probe(hipStream_t st, int n, const float *in, float *out) {
    hipLaunchKernelGGL(k_phong_probe, dim3((n + 255) / 256), dim3(256), 0, st, n, in, out);
}
void launch_tree_probe(int grid, hipStream_t st, const DScene &S, int n, const float *org, const float *dst, uint32_t *out_box, uint32_t *out_ref, uint32_t *out_sig) {
    hipLaunchKernelGGL(k_tree_probe, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S.leaf_chunk0, S, n, org, dst, out_box, out_ref, out_sig);
}
void launch_primary_probe(int grid, hipStream_t st, const DCam *cam, int W, int H, float *out) {
    hipLaunchKernelGGL(k_primary_probe, dim3(grid), dim3(256), 0, st, cam, W, H, out);
}

#ifdef RT_WORK_COUNTERS
__global__ void k_set_prof(Control *ctl, uint32_t base) { g_prof = ctl->prof; g_prof_base = base; }
void launch_set_prof(hipStream_t st, Control *ctl, uint32_t base) { hipLaunchKernelGGL(k_set_prof, dim3(1), dim3(1), 0, st, ctl, base); }
#else
void launch_set_prof(hipStream_t, Control *, uint32_t) {}
#endif

// k_pass_list, the sibling of k_flag (adaptive pass counts, rt_set_pass_tolerance: the banner in front of k_resolve): the primary tiles of the NEXT pass.  F is the frame of sub-samples (the output frame itself at n = 1).
// A sub-sample is listed while the output pixel that owns it is still active; the active output pixels, summed over the list passes, are
// what rt_stats::pixels needs beyond the whole-frame passes (build_tile_list counts them).  Control::n_flag is zero when this starts
// (k_resolve<.., SINK_CONV>).
struct ActivePred {
    const uint8_t *__restrict__ active;
    uint32_t W;
    __device__ __forceinline__ bool operator()(const uint32_t i, const uint32_t lr, const bool) const { return active[lr * W + i] != 0u; }
};
__global__ __launch_bounds__(RT_WAVES * 64) void k_pass_list(const DFrame F, const uint8_t *__restrict__ active, FlagTile *__restrict__ list,
                                                            Control *__restrict__ ctl) {
    build_tile_list(F, list, ctl, ActivePred{active, static_cast<uint32_t>(F.out_width)});
}

// ------------------------------------------------------------------------------------------------------
// The template kernels of the code object, in the order they are emitted: instantiations follow the non-template kernels in the order of
// their first use, and this table, ahead of every launcher, is that first use.  However the dispatch below is written, the code object holds
// these kernels in this order.  A new variant is appended HERE.
//   T = k_trace<PRIMARY, COUNT, FLAT, LENS, SHUTTER, PASS>   G = k_stage<PRIMARY, COUNT, STAGE, CONT, LENS, SHUTTER, PASS>   R = k_resolve<SRC, SINK>
// ------------------------------------------------------------------------------------------------------
#define K(...) reinterpret_cast<const void *>(&__VA_ARGS__)
#define T(...) K(k_trace<__VA_ARGS__>)
#define G(...) K(k_stage<__VA_ARGS__>)
#define R(...) K(k_resolve<__VA_ARGS__>)
[[maybe_unused]] static const void *const kKernelOrder[] = {
    // the fast variants, as query_occupancy names them
    T(true, false, true), T(false, false, true), K(k_shadow<false, true, false>), G(true, false, 0, false), G(false, false, 0, false),
    K(k_shadow<false, false, false>), K(k_shadow_shaft<false, false>), K(k_shade<true, true, true>), K(k_shade<true, false, false>),
    // k_trace: LENS (flat scenes only, as every sampling kind: see launch_trace), then pinhole
    T(true, true, true, true), T(true, false, true, true),
    T(true, true, true), T(false, true, true), T(true, true, false), T(true, false, false), T(false, true, false), T(false, false, false),
    // k_stage: LENS, then pinhole
    G(true, false, 0, true, true), G(true, false, 1, true, true), G(true, true, 0, false, true), G(true, true, 1, false, true),
    G(true, true, 2, false, true), G(true, false, 0, false, true), G(true, false, 1, false, true), G(true, false, 2, false, true),
    G(true, false, 0, true), G(true, false, 1, true), G(false, false, 0, true), G(false, false, 1, true), G(false, false, 1, false),
    G(false, false, 2, false), G(false, true, 0, false), G(false, true, 1, false), G(false, true, 2, false), G(true, false, 1, false),
    G(true, false, 2, false), G(true, true, 0, false), G(true, true, 1, false), G(true, true, 2, false),
    // k_shadow, k_shadow_shaft
    K(k_shadow<true, true, false>), K(k_shadow<true, false, false>), K(k_shadow_shaft<false, true>), K(k_shadow_shaft<true, false>),
    K(k_shadow<false, false, true>),
    // k_shade
    K(k_shade<true, false, true>), K(k_shade<true, true, false>), K(k_shade<false, true, false>), K(k_shade<false, false, false>),
    // the resolves of rt_set_passes
    R(SRC_SS, ACC_FIRST), R(SRC_SS, ACC_MIDDLE), R(SRC_SS, ACC_LAST), R(SRC_ONE, ACC_FIRST), R(SRC_ONE, ACC_MIDDLE), R(SRC_ONE, ACC_LAST),
    // SHUTTER
    T(true, true, true, false, true), T(true, false, true, false, true),
    G(true, false, 0, true, false, true), G(true, false, 1, true, false, true), G(true, true, 0, false, false, true),
    G(true, true, 1, false, false, true), G(true, true, 2, false, false, true), G(true, false, 0, false, false, true),
    G(true, false, 1, false, false, true), G(true, false, 2, false, false, true),
    // PASS: k_trace, each of shutter / lens / pinhole
    T(true, true, true, false, true, true), T(true, true, true, true, false, true), T(true, true, true, false, false, true),
    T(true, false, true, false, true, true), T(true, false, true, true, false, true), T(true, false, true, false, false, true),
    // PASS: k_stage
    G(true, false, 0, true, false, true, true), G(true, false, 0, true, true, false, true), G(true, false, 0, true, false, false, true),
    G(true, false, 1, true, false, true, true), G(true, false, 1, true, true, false, true), G(true, false, 1, true, false, false, true),
    G(true, true, 0, false, false, true, true), G(true, true, 0, false, true, false, true), G(true, true, 0, false, false, false, true),
    G(true, true, 1, false, false, true, true), G(true, true, 1, false, true, false, true), G(true, true, 1, false, false, false, true),
    G(true, true, 2, false, false, true, true), G(true, true, 2, false, true, false, true), G(true, true, 2, false, false, false, true),
    G(true, false, 0, false, false, true, true), G(true, false, 0, false, true, false, true), G(true, false, 0, false, false, false, true),
    G(true, false, 1, false, false, true, true), G(true, false, 1, false, true, false, true), G(true, false, 1, false, false, false, true),
    G(true, false, 2, false, false, true, true), G(true, false, 2, false, true, false, true), G(true, false, 2, false, false, false, true),
    // rt_set_pass_tolerance
    R(SRC_SS, SINK_CONV), R(SRC_ONE, SINK_CONV),
    // the storing resolves
    R(SRC_ONE, SINK_STORE), R(SRC_SS, SINK_STORE), R(SRC_ADAPTIVE, SINK_STORE),
    // device ray queries
    K(k_closest<>), K(k_pack_rays<>),
    // ambient occlusion
    K(k_occlusion<false>), K(k_occlusion<true>), K(k_hit_points<>),
    // geometry buffers: pinhole, lens, shutter
    K(k_gbuffer<0>), K(k_gbuffer<1>), K(k_gbuffer<2>),
};
// kKernelOrder continued.  tests/test_gbuffer_query_api.py pins the end of the table above (the geometry-buffer kernels are its last entries),
// so the kernels of later queries continue the order here, directly behind it and still ahead of every launcher: the code object emits them
// behind every kernel of the table above, in this order.  A new query kernel is appended HERE.
[[maybe_unused]] static const void *const kKernelOrderQueries[] = {
    // soft shadows
    K(k_soft_shadows<false>), K(k_soft_shadows<true>),
    // one-bounce diffuse gather
    K(k_gather<false>), K(k_gather<true>),
    // light probes
    K(k_probes<false>), K(k_probes<true>), K(k_probe_lookup<>),
    // leak-free probe lookup
    K(k_probe_lookup_visible<>),
    // closest points: the bounds, then the query
    K(k_near_records<>), K(k_near_leaf_boxes<>), K(k_nearest<>),
    // ordered ray hits: K = 1, 2, 4, 8 output slots
    K(k_ray_hits<1>), K(k_ray_hits<2>), K(k_ray_hits<4>), K(k_ray_hits<8>),
    // bounced light: the gather and the probes fed by a source volume, x ROUNDS x {plain, visible}
    K((k_gather_bounce<false, false>)), K((k_gather_bounce<true, false>)), K((k_gather_bounce<false, true>)), K((k_gather_bounce<true, true>)),
    K((k_probes_bounce<false, false>)), K((k_probes_bounce<true, false>)), K((k_probes_bounce<false, true>)), K((k_probes_bounce<true, true>)),
};
#undef R
#undef G
#undef T
#undef K

// ------------------------------------------------------------------------------------------------------
// residency: blocks per CU for each persistent kernel (fast variants), queried once per scene
// ------------------------------------------------------------------------------------------------------
void query_occupancy(bool flat, int *trace_primary, int *trace_rays, int *shadow, int *shaft_out, int *shade, int *beam) {
    int n = 0;
    auto q = [&](auto kernel, int threads, int fallback) {
        return (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, 0) == hipSuccess && n > 0) ? n : fallback;
    };
    if (flat) {
        *trace_primary = q(k_trace<true, false, true>, RT_WAVES * 64, 4);
        *trace_rays = q(k_trace<false, false, true>, RT_WAVES * 64, 4);
        *shadow = q(k_shadow<false, true, false>, RT_WAVES * 64, 4);
        *shaft_out = *shadow;
    } else {
        *trace_primary = q(k_stage<true, false, 0, false>, RT_WAVES * 64, 4);
        *trace_rays = q(k_stage<false, false, 0, false>, RT_WAVES * 64, 4);
        *shadow = q(k_shadow<false, false, false>, RT_WAVES * 64, 4);
        *shaft_out = q((k_shadow_shaft<false, false>), RT_WAVES * 64, 4);      // (its grid used to be the smaller of the two residencies: 4 of its 6 waves per SIMD)
    }
    *shade = flat ? q((k_shade<true, true, true>), 256, 2) : q((k_shade<true, false, false>), 256, 2);
    *beam = q(k_beam, RT_WAVES * 64, 4);
}

// ------------------------------------------------------------------------------------------------------
// host-callable launchers (keep <<<>>> syntax inside this translation unit)
// ------------------------------------------------------------------------------------------------------
// Run-time values -> compile-time constants: pick(f, a, b, ...) calls f(A{}, B{}, ...) where a bool became std::true_type / std::false_type
// and an int 0, 1 or anything else std::integral_constant<int, 0 / 1 / 2>.  The launchers name their kernel with these constants and guard the
// launch with `if constexpr`, so that no instantiation exists beyond those of kKernelOrder.
template <typename F>
static void pick(F &&f) { f(); }
template <typename F, typename... R>
static void pick(F &&f, int v, R... rest);
template <typename F, typename... R>
static void pick(F &&f, bool v, R... rest) {
    if (v) pick([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else pick([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
template <typename F, typename... R>
static void pick(F &&f, int v, R... rest) {
    if (v == 0) pick([&](auto... c) { f(std::integral_constant<int, 0>{}, c...); }, rest...);
    else if (v == 1) pick([&](auto... c) { f(std::integral_constant<int, 1>{}, c...); }, rest...);
    else pick([&](auto... c) { f(std::integral_constant<int, 2>{}, c...); }, rest...);
}

// The primary kernels come in three kinds -- 0 pinhole, 1 thin lens (Depth of field), 2 camera motion blur (§5, Motion blur:
// the shutter wins, the lens is a run-time branch inside it) -- and each with PASS for a pass p > 0 of rt_set_passes (§5, Multi-pass
// accumulation).  Launches of bounce or input rays look at neither.
static int primary_kind(bool primary, const DFrame &Fr) { return !primary ? 0 : Fr.shutter != 0 ? 2 : Fr.lens != nullptr ? 1 : 0; }
static bool primary_pass(bool primary, const DFrame &Fr) { return primary && Fr.pass_key != 0u; }

// flat scenes, and the fused kernel on a tree scene (the staged k_stage pipeline is the alternative).  On a tree scene the fused kernel
// exists for plain rays alone -- pinhole primary rays of a first pass, bounce and input rays -- and the host asks fused_tree_trace() once
// per launch sequence: a sampling kind (LENS, SHUTTER, PASS) costs one k_trace instantiation per counting variant, the flat one, and its
// tree frames are k_stage's whatever RT_STAGED_TRACE says.  plain_rays is the one definition of that rule, for the question and for the
// instantiations; a launch it rules out is a host bug and stops the process.
static constexpr bool plain_rays(int kind, bool pass) { return kind == 0 && !pass; }
bool fused_tree_trace(bool primary, const DFrame &Fr) { return plain_rays(primary_kind(primary, Fr), primary_pass(primary, Fr)); }
void launch_trace(bool primary, bool count, bool flat, int grid, hipStream_t st, const DScene &S, const CamArg &cam, const DLights &L, const DFrame &Fr,
                  int level, int slot, const RayItem *rays_in, ShadeItem *items, Control *ctl, float4 *rec, int32_t *out_hit, float *out_t) {
    pick([&](auto P, auto C, auto FL, auto KIND, auto PASS) {
        if constexpr (plain_rays(KIND(), PASS()) || (P() && FL()))
            hipLaunchKernelGGL((k_trace<P(), C(), FL(), KIND() == 1, KIND() == 2, PASS()>), dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks,
                               S.leaf_chunk0, S, cam, L, Fr, level, slot, rays_in, items, ctl, rec, out_hit, out_t);
        else if constexpr (P())
            std::abort();                          // a sampling kind on a tree scene: no fused kernel (fused_tree_trace says so beforehand)
    }, primary, count, flat, primary_kind(primary, Fr), primary_pass(primary, Fr));
}

void launch_stage(bool primary, bool count, int stage, bool cont, int grid, hipStream_t st, const DScene &S, const CamArg &cam, const DLights &L,
                  const DFrame &Fr, int level, int lslots, const RayItem *rays_in, ShadeItem *items, Control *ctl, float4 *rec, int32_t *out_hit,
                  float *out_t, unsigned long long *best, unsigned long long *lit, const TaskQueues &Q) {
    if (cont) { count = false; stage = stage != 0; }       // continuations exist for the two traversal stages of the fast (non-counting) variants only
    pick([&](auto P, auto C, auto STAGE, auto CONT, auto KIND, auto PASS) {
        if constexpr ((P() || (KIND() == 0 && !PASS())) && !(CONT() && (C() || STAGE() == 2)))
            hipLaunchKernelGGL((k_stage<P(), C(), STAGE(), CONT(), KIND() == 1, KIND() == 2, PASS()>), dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris,
                               S.chunks, S.leaf_chunk0, S, cam, L, Fr, level, lslots, rays_in, items, ctl, rec, out_hit, out_t, best, lit, Q);
    }, primary, count, stage, cont, primary_kind(primary, Fr), primary_pass(primary, Fr));
}

#define RT_LAUNCH_SHADOW(C, F, K) hipLaunchKernelGGL((k_shadow<C, F, K>), g, b, 0, st, S.nodes, S.leaf_tris, S.chunks, S.leaf_chunk0, S, L, level, slot, lslots, item_cap, items, ctl, vis, Q, sidx)
void launch_shadow(bool count, bool flat, int grid, hipStream_t st, const DScene &S, const DLights &L, int level, int slot, int lslots,
                   uint32_t item_cap, const ShadeItem *items, Control *ctl, unsigned long long *vis, ContTask *tasks_out, uint32_t cap, uint32_t budget, uint32_t target,
                   const uint32_t *sidx) {
    const dim3 g(grid), b(RT_WAVES * 64);
    const TaskQueues Q{nullptr, (flat || count) ? nullptr : tasks_out, 0u, 2u, cap, (flat || count) ? 0u : budget, target};
    pick([&](auto C, auto FL) { RT_LAUNCH_SHADOW(C(), FL(), false); }, count, flat);
}

void launch_shadow_shaft(int grid, hipStream_t st, const DScene &S, const DLights &L, int level, int slot, int lslots, uint32_t item_cap,
                         const ShadeItem *items, Control *ctl, unsigned long long *vis, ContTask *tasks_out, uint32_t cap, uint32_t budget, uint32_t target, const uint32_t *sidx,
                         const uint8_t *pair_done) {
    TaskQueues Q{nullptr, tasks_out, 0u, 2u, cap, budget, target};
    Q.pair_done = pair_done;
    // (the task emission costs the walking kernel 30 more spilled registers: it is compiled in only when a budget asks for it)
    if (budget != 0u && tasks_out != nullptr)
        hipLaunchKernelGGL((k_shadow_shaft<false, true>), dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S, L, level, slot, lslots, item_cap, items, ctl, vis, Q, sidx);
    else
        hipLaunchKernelGGL((k_shadow_shaft<false, false>), dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S, L, level, slot, lslots, item_cap, items, ctl, vis, Q, sidx);
}

// the leaf tasks of a shaft-walk launch: chunk ranges of big leaves, through the same leaf code (shaft_leaf)
void launch_shadow_shaft_cont(int grid, hipStream_t st, const DScene &S, const DLights &L, int level, int lslots, uint32_t item_cap, const ShadeItem *items,
                              Control *ctl, unsigned long long *vis, const ContTask *tasks_in, uint32_t cap, const uint32_t *sidx) {
    const TaskQueues Q{tasks_in, nullptr, 2u, 0u, cap, 0u};
    hipLaunchKernelGGL((k_shadow_shaft<true, false>), dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S, L, level, 0, lslots, item_cap, items, ctl, vis, Q, sidx);
}

// processes the leaf tasks of queue q_in (leaf tasks never create new tasks)
void launch_shadow_cont(int grid, hipStream_t st, const DScene &S, const DLights &L, int level, int lslots, uint32_t item_cap, const ShadeItem *items,
                        Control *ctl, unsigned long long *vis, const ContTask *tasks_in, ContTask *tasks_out, uint32_t q_in, uint32_t q_out,
                        uint32_t cap, uint32_t budget, const uint32_t *sidx) {
    const dim3 g(grid), b(RT_WAVES * 64);
    const int slot = 0;
    const TaskQueues Q{tasks_in, tasks_out, q_in, q_out, cap, tasks_out ? budget : 0u};
    RT_LAUNCH_SHADOW(false, false, true);
}

void launch_beam(int grid, hipStream_t st, const DScene &S, const DLights &L, int level, int lslots, uint32_t item_cap, const ShadeItem *items, Control *ctl,
                 unsigned long long *vis, uint32_t *sidx, unsigned long long *pend, float2 *ltab) {
    // (pend != nullptr only for SIMPLE lights -- n_samples <= RT_LIGHT_TAB_STRIDE, rt_capi.cpp's `fold` -- which is what launch_shade's
    //  FOLD instantiations, the table's readers, are picked by: the writer's N <= RT_LIGHT_TAB_STRIDE guard never drops a table they read)
    hipLaunchKernelGGL(k_beam, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S, L, level, lslots, item_cap, items, ctl, vis, sidx, pend, ltab);
}

void launch_pair_beam(int grid, hipStream_t st, const DScene &S, const DLights &L, int level, int lslots, uint32_t item_cap, const ShadeItem *items, Control *ctl,
                      unsigned long long *vis, uint32_t *sidx, uint8_t *done) {
    hipLaunchKernelGGL(k_pair_beam, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S, L, level, lslots, item_cap, items, ctl, vis, sidx, done);
}

// pend != nullptr: k_beam folded the shadow units of this level (SIMPLE lights only) -- the FOLD variants finish its pending pairs
void launch_shade(int grid, hipStream_t st, const DScene &S, const DLights &L, const DFrame &F, int level, int slot, int lslots,
                  const ShadeItem *items, Control *ctl, unsigned long long *vis, float4 *rec, float *fres, RayItem *rays_out, bool resolve_flat,
                  const unsigned long long *pend, const float2 *ltab) {
    const bool simple = L.mode != RT_LIGHT_SPHERE && L.n_samples <= 64;
    pick([&](auto SIMPLE, auto FL, auto FOLD) {
        if constexpr (SIMPLE() || !FOLD())
            hipLaunchKernelGGL((k_shade<SIMPLE(), FL(), FOLD()>), dim3(grid), dim3(256), 0, st, S.nodes, S.leaf_tris, S, L, F, level, slot, lslots, items, ctl, vis, rec, fres,
                               rays_out, pend, ltab);
    }, simple, resolve_flat, simple && pend != nullptr);
}

void launch_deep(int grid, hipStream_t st, const DScene &S, const DLights &L, const DFrame &F, int level0, const RayItem *rays_in, Control *ctl, float4 *rec0, float *fres0) {
    hipLaunchKernelGGL(k_deep, dim3(grid), dim3(256), 0, st, S.nodes, S.leaf_tris, S, L, F, level0, rays_in, ctl, rec0, fres0);
}

// the resolve of a launch sequence: the plain one-ray / n x n store, one pass of a count > 1 frame (n x n or one-ray form), pass 2 of an
// adaptive frame, or the converging resolve of a pass of an adaptive-pass frame
void launch_resolve(int grid, hipStream_t st, const DFrame &F, const ResolveArgs &a) {
    const int kind = a.s2 != nullptr ? 2 : a.count > 1 ? 1 : 0;                         // the sink: store, accumulate, converge
    const int mode = kind != 1 ? 0 : a.index == 0 ? 0 : (a.index + 1 < a.count ? 1 : 2);    // ACC_FIRST, ACC_MIDDLE, ACC_LAST
    const int src = (kind == 0 && a.refine != nullptr) ? SRC_ADAPTIVE : (F.ss > 1 ? SRC_SS : SRC_ONE);        // n x n sub-samples -> one pixel
    pick([&](auto SRC, auto KIND, auto M) {
        constexpr int SINK = KIND() == 0 ? SINK_STORE : KIND() == 1 ? ACC_FIRST + M() : SINK_CONV;
        // (a mode belongs to the accumulating sink alone, and an adaptive frame only stores)
        if constexpr ((KIND() == 1 || M() == 0) && (KIND() == 0 || SRC() != SRC_ADAPTIVE)) {
            ResolvePack<SRC(), SINK> p;
            static_cast<ResolveIo &>(p) = ResolveIo{a.rec, a.fres, a.out_rgb, a.out_u8, a.cam};
            if constexpr (SRC() == SRC_ADAPTIVE) static_cast<ResolveAdaptive &>(p) = ResolveAdaptive{a.refine, a.c1, a.pos};
            if constexpr (KIND() == 1) static_cast<ResolveAcc &>(p) = ResolveAcc{a.acc, static_cast<float>(a.count)};
            if constexpr (KIND() == 2) static_cast<ResolveConv &>(p) = ResolveConv{a.acc, a.s2, a.taken, a.active, a.n_flag, a.index + 1, a.min_passes, a.count, a.tol};
            hipLaunchKernelGGL((k_resolve<SRC(), SINK>), dim3(grid), dim3(256), 0, st, F, p);
        }
    }, src, kind, mode);
}
void launch_flag(int grid, hipStream_t st, const DFrame &F, const float *c1, const int32_t *pos, float tau, uint8_t *refine, FlagTile *list, Control *ctl) {
    hipLaunchKernelGGL(k_flag, dim3(grid), dim3(RT_WAVES * 64), 0, st, F, c1, pos, tau, refine, list, ctl);
}
void launch_pass_list(int grid, hipStream_t st, const DFrame &F, const uint8_t *active, FlagTile *list, Control *ctl) {
    hipLaunchKernelGGL(k_pass_list, dim3(grid), dim3(RT_WAVES * 64), 0, st, F, active, list, ctl);
}

void launch_segments(int grid, hipStream_t st, const DScene &S, int n, const float *hit, const float *light, uint8_t *vis) {
    hipLaunchKernelGGL(k_segments, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S.leaf_chunk0, S, n, hit, light, vis);
}
void launch_closest(int grid, hipStream_t st, const DScene &S, int n, const float *org, const float *dir, int32_t *face, float *t) {
    hipLaunchKernelGGL(k_closest<>, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S.leaf_chunk0, S, n, org, dir, face, t);
}
// n <= 2^24 (one query chunk)
void launch_pack_rays(hipStream_t st, int n, const float *org, const float *dir, RayItem *rays) {
    hipLaunchKernelGGL(k_pack_rays<>, dim3((n + 255) / 256), dim3(256), 0, st, n, org, dir, rays);
}
// dirs: the table of m; the grid is ao_grid's
void launch_occlusion(int grid, hipStream_t st, const DScene &S, int n, const float *point, const float *normal, const float *dirs, const float *rot, int m,
                      float radius, uint32_t seed, uint16_t *open, float *ao) {
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S.leaf_chunk0, S, n, point, normal, dirs, rot, m, radius,
                           seed, open, ao);
    };
    if (ao_layout(m).rounds > 1) go(k_occlusion<true>);
    else go(k_occlusion<false>);
}
// L: point or area lights (check_lights); the grid is shadow_grid's
void launch_soft_shadows(int grid, hipStream_t st, const DScene &S, const DLights &L, int n, const float *point, const float *normal, int per_point, uint32_t seed,
                         float fu, float fv, uint16_t *visible, float *share) {
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S.leaf_chunk0, S, L, n, point, normal, per_point, seed, fu,
                           fv, visible, share);
    };
    if (shadow_layout(L.n_lights, L.usteps, L.vsteps).A.rounds > 1) go(k_soft_shadows<true>);
    else go(k_soft_shadows<false>);
}
// L: n_lights, pos and color are read (check_lights); dirs / rot: the tables of launch_occlusion; the grid is ao_grid's
void launch_gather(int grid, hipStream_t st, const DScene &S, const DLights &L, int n, const float *point, const float *normal, const float *dirs, const float *rot,
                   int m, uint32_t seed, float *rgb) {
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S.leaf_chunk0, S, L, n, point, normal, dirs, rot, m, seed, rgb);
    };
    if (ao_layout(m).rounds > 1) go(k_gather<true>);
    else go(k_gather<false>);
}
// L: as launch_gather; dirs / wts: the two probe tables of m; the grid is ao_grid's
void launch_probes(int grid, hipStream_t st, const DScene &S, const DLights &L, int n, const float *position, const float *dirs, const float *wts, int m,
                   int direct, float *coeff) {
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S.leaf_chunk0, S, L, n, position, dirs, wts, m, direct, coeff);
    };
    if (ao_layout(m).rounds > 1) go(k_probes<true>);
    else go(k_probes<false>);
}
// the parents' launches with a source volume (G, src) behind the tables; visible: the leak-free lookup at the hits
void launch_gather_bounce(int grid, hipStream_t st, const DScene &S, const DLights &L, int n, const float *point, const float *normal, const float *dirs,
                          const float *rot, int m, uint32_t seed, const ProbeGrid &G, const float *src, bool visible, float *rgb) {
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S.leaf_chunk0, S, L, n, point, normal, dirs, rot, m, seed, G,
                           src, rgb);
    };
    const bool rounds = ao_layout(m).rounds > 1;
    if (visible) { if (rounds) go(k_gather_bounce<true, true>); else go(k_gather_bounce<false, true>); }
    else { if (rounds) go(k_gather_bounce<true, false>); else go(k_gather_bounce<false, false>); }
}
void launch_probes_bounce(int grid, hipStream_t st, const DScene &S, const DLights &L, int n, const float *position, const float *dirs, const float *wts, int m,
                          int direct, const ProbeGrid &G, const float *src, bool visible, float *coeff) {
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S.leaf_chunk0, S, L, n, position, dirs, wts, m, direct, G,
                           src, coeff);
    };
    const bool rounds = ao_layout(m).rounds > 1;
    if (visible) { if (rounds) go(k_probes_bounce<true, true>); else go(k_probes_bounce<false, true>); }
    else { if (rounds) go(k_probes_bounce<true, false>); else go(k_probes_bounce<false, false>); }
}
// the grid is query_grid's: a block of 256 threads per 256 points
void launch_probe_lookup(int grid, hipStream_t st, const ProbeGrid &G, const float *coeff, int n, const float *point, const float *normal, float *rgb) {
    hipLaunchKernelGGL(k_probe_lookup<>, dim3(grid), dim3(256), 0, st, G, coeff, n, point, normal, rgb);
}
// the grid is pv_grid's: a wave per 8 points; mask may be null
void launch_probe_lookup_visible(int grid, hipStream_t st, const DScene &S, const ProbeGrid &G, const float *coeff, int n, const float *point, const float *normal,
                                 float *rgb, uint8_t *mask) {
    hipLaunchKernelGGL(k_probe_lookup_visible<>, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S.leaf_chunk0, S, G, coeff, n, point, normal, rgb,
                       mask);
}
// the query's bounds: a record per leaf reference, then a box per chunk and per node (inner nodes: empty).  Room: n_refs records (one at
// the least), S.n_nodes nodes, n_chunks chunk boxes (one at the least).
void launch_near_bounds(hipStream_t st, const DScene &S, uint32_t n_refs, uint32_t n_chunks, int cus, NearTri *recs, NearNode *boxes, NearNode *chunk_boxes) {
    if (n_refs) hipLaunchKernelGGL(k_near_records<>, dim3(capped_grid(n_refs, 256u, cus)), dim3(256), 0, st, S.leaf_tris, S.tri_verts, n_refs, S.n_faces, recs);
    hipLaunchKernelGGL(k_near_leaf_boxes<>, dim3(capped_grid(S.n_nodes, 4u, cus)), dim3(256), 0, st, S.nodes, S.leaf_chunk0, recs, S.n_nodes, n_refs,
                       n_chunks, boxes, chunk_boxes);
}
// the grid is query_grid's; face, dist2, point: any may be null
// k slots run on the next instantiation of 1, 2, 4, 8 (hits_variant); a k outside 1 .. 8 launches nothing (the argument rule refused it)
void launch_ray_hits(int grid, hipStream_t st, const DScene &S, int n, const float *org, const float *dir, int k, float t_max, int32_t *face, float *t,
                     int32_t *count) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S, n, org, dir, k, t_max, face, t, count);
    };
    switch (hits_variant(k)) {
        case 1: go(k_ray_hits<1>); break;
        case 2: go(k_ray_hits<2>); break;
        case 4: go(k_ray_hits<4>); break;
        case 8: go(k_ray_hits<8>); break;
        default: break;
    }
}
void launch_nearest(int grid, hipStream_t st, const DScene &S, const NearNode *boxes, const NearTri *recs, const NearNode *chunk_boxes, int n,
                    const float *point_in, float r2, int32_t *face, float *dist2, float *point) {
    hipLaunchKernelGGL(k_nearest<>, dim3(grid), dim3(RT_WAVES * 64), 0, st, boxes, recs, chunk_boxes, S.leaf_chunk0, S.extent, n, point_in, r2, face, dist2, point);
}
void launch_hit_points(hipStream_t st, const DScene &S, int n, const float *org, const float *dir, const int32_t *face, const float *t, float *point,
                       float *normal) {
    const unsigned blocks = static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256);
    hipLaunchKernelGGL(k_hit_points<>, dim3(blocks), dim3(256), 0, st, S.face_normal, S.n_faces, n, org, dir, face, t, point, normal);
}
// F: the output frame with the sample settings (gbuffer_frame in rt_capi.cpp); the grid is gb_grid's; out is 16-byte aligned
void launch_gbuffer(int grid, hipStream_t st, const DScene &S, const DCam &cam, const DShutter &shut, const DFrame &F, const float *pass_tab, int first,
                    int count, float *out) {
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(RT_WAVES * 64), 0, st, S.nodes, S.leaf_tris, S.chunks, S.leaf_chunk0, S, cam, shut, F, pass_tab, first, count,
                           reinterpret_cast<float4 *>(out));
    };
    if (F.shutter) go(k_gbuffer<2>);
    else if (F.lens != nullptr) go(k_gbuffer<1>);
    else go(k_gbuffer<0>);
}

}  // namespace rtamd
