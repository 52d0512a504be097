// rt_device.hpp -- device-side data layout shared by the HIP kernels and the C-ABI host code.
//
// HBM layout (all arrays resident for the lifetime of the uploaded scene; 288 GB per MI355X makes the
// per-frame working buffers -- one slot per pixel per recursion level -- a non-issue):
//   nodes      rt_node[n_nodes]        32 B   breadth-first, live children contiguous, read wave-uniformly (s_load)
//   leaf_tris  TriRec[n_face_refs]     80 B   leaf-ordered, per-triangle constants of rayTriangleIntersection
//                                             hoisted (bit-identical float ops evaluated once on the host)
//   tri_verts / face_normal / tri_vid / mat_id / vert_normal / mats   shading inputs, gathered per shaded hit
//   rays[2]    RayItem[npix]           48 B   ping-pong bounce rays (level >= 1), compacted per level
//   items      ShadeItem[npix]         64 B   lit closest hits of the current level (compacted)
//   vis        u64[npix * L * words]          sample-visibility masks written by the shadow kernel
//   rec        float4[(D+1) * npix]           per pixel, per level: Phong RGB + blend kind (folded by resolve)
//   fres       float [(D+1) * npix]           Fresnel factor of illum-5 hits
#pragma once

#include <cstddef>
#include <cstdint>

#include "rt_mi355x.h"
#include "rt_scene_layout.hpp"

namespace rtamd {

struct alignas(16) RayItem {     // a bounce ray (level >= 1) or an rt_trace_rays input ray
    float ox, oy, oz, dx;
    float dy, dz, lx, ly;
    float lz;
    uint32_t lmode;              // 0: sees the scene lights; 1: sees the single light (lx,ly,lz) (flyscene.cpp:735-738)
    uint32_t pix;
    uint32_t pad;
};
static_assert(sizeof(RayItem) == 48, "RayItem must be 48 bytes");

struct alignas(16) ShadeItem {   // a lit closest hit waiting for its sample shadow rays and Phong
    float ox, oy, oz, dx;
    float dy, dz, lx, ly;
    float lz;
    uint32_t lmode;
    uint32_t pix;
    int32_t face;
    float t;
    uint32_t pad0, pad1, pad2;
};
static_assert(sizeof(ShadeItem) == 64, "ShadeItem must be 64 bytes");

// A piece of a unit's work handed to other waves: the chunks [c_begin, c_end) (64 triangles each) of leaf `node` for the
// rays in `mask` (lane mask of the unit's wave).  Big leaves are never processed inline by the walking wave: one wave
// grinding through a 979-triangle leaf for 64 rays was the critical path of whole kernels.
struct alignas(16) ContTask {
    uint32_t unit;
    uint32_t node;
    unsigned long long mask;
    uint32_t c_begin, c_end;
    uint32_t pad0, pad1;
};
static_assert(sizeof(ContTask) == 32, "ContTask must be 32 bytes");

// queues of one traversal launch: where its continuation tasks come from / go to (indices into Control::n_tasks[level])
struct TaskQueues {
    const ContTask *tasks_in;     // continuation launches only
    ContTask *tasks_out;          // nullptr: never hand work away
    uint32_t q_in, q_out;
    uint32_t cap, budget;         // queue capacity; leaves whose estimated cost (VALU instructions) exceeds `budget` are split into tasks (0 = off)
    uint32_t target = 0;          // estimated cost of one task piece (0: same as budget)
    const uint8_t *pair_done = nullptr;   // k_shadow_shaft behind k_pair_beam, several lights: byte (item, light) = 1 -- the beam has written that pair's words, skip its units
};

// blend kinds stored in rec[].w (bit pattern of a uint32)
enum : uint32_t {
    KIND_CONST = 0,      // terminal: rgb is the value (BACKGROUND, SHADOW or plain Phong)
    KIND_PASS = 1,       // illum 9:      0.10*phong + 0.90*child   (flyscene.cpp:718)
    KIND_REFRACT = 2,    // illum 6:      0.2*phong  + 0.8*child    (flyscene.cpp:754)
    KIND_MIRROR = 3,     // illum 3,4:    0.15*phong + 0.85*child   (flyscene.cpp:738)
    KIND_FRESNEL = 4     // illum 5:      fresnel * (0.15*phong + 0.85*child)  (flyscene.cpp:739-743)
};

struct DCam {
    float center[3];
    float inv_view[12];
    float vp[4];
    float k0, k1;            // aspect*scale, scale  (camera.hpp:164-166), evaluated on the host
};

// Camera motion blur (rt_set_shutter, DESIGN.md §5, Motion blur): d[q] = close - open of the 15 pose values (center[3], inv_view[12]),
// evaluated on the host.  It travels BEHIND the open camera in the same device block (DCam itself does not grow: every kernel reads it with
// scalar loads) and only the SHUTTER instantiations of the primary kernels read it.
struct DShutter {
    float d[16];             // [0, 3): center, [3, 15): inv_view, [15]: unused
};
// Primary culling (rt_set_primary_cull, DESIGN.md §5, Primary culling): the tiles [tx0, tx1) x [ty0, ty1) of the FRAME (8 x 8 pixels, frame
// rows) outside which no primary ray of this camera can meet the root box, evaluated on the host for every camera of a frame or replay.  It
// travels at the tail of the block, so a graph replay gets the rectangle of the camera it uploads.  Only frames whose DFrame::cull is set
// read it; every other block carries the whole frame.
struct DCamBlock {           // what rt_ctx::d_cam points to (a graph replay uploads the whole block) and what an eager frame's kernels get as an argument
    DCam cam;
    float pad_[3];
    DShutter sh;
    int32_t rect[4];         // tx0, ty0, tx1, ty1
};
static_assert(offsetof(DCamBlock, cam) == 0 && offsetof(DCamBlock, sh) == 96, "the shutter deltas sit 96 bytes behind the camera");
static_assert(offsetof(DCamBlock, rect) == 160 && sizeof(DCamBlock) == 176, "the cull rectangle sits behind the shutter deltas");

// How a kernel gets the camera block of its frame (the primary k_trace / k_stage instantiations, k_resolve for `rect`).  ptr != nullptr: the
// block in device memory -- a captured graph, whose replays upload a new camera in front of it.  ptr == nullptr: `val`, the block itself as
// a kernel argument -- every eager launch sequence, which needs neither the upload nor device memory.  The kernel picks one source at entry
// with a wave-uniform branch; both sides are scalar loads into the same registers.
struct CamArg {
    const DCamBlock *ptr;
    DCamBlock val;
};

struct DLights {
    float pos[RT_MAX_LIGHTS][3];
    float color[3];
    int32_t n_lights, mode, usteps, vsteps, n_samples;
    float len_x, len_y;
    const float *offsets;    // RT_LIGHT_SPHERE: n_samples * 3 sample offsets (device); sample s of a light at p = offsets[s] + p
    float obox[6];           // ... and their bounding box (min, max): p + obox bounds the samples (float addition is monotone)
};

// The light-sample table of flat scenes with a SIMPLE light (k_beam writes it, k_shade<.., FOLD> reads it): RT_MAX_LIGHTS slots of
// RT_LIGHT_TAB_STRIDE (x, y) pairs, entry [l * RT_LIGHT_TAB_STRIDE + s] = sample s of light l (a SIMPLE light has at most 64 samples; z is
// one value per light and stays with LightGrid).
#define RT_LIGHT_TAB_STRIDE 64u
#define RT_LIGHT_TAB_ENTRIES (RT_MAX_LIGHTS * RT_LIGHT_TAB_STRIDE)

// Adaptive supersampling (rt_set_supersampling_threshold): one entry of k_flag's tile list -- an 8x8 tile of the sub-sample frame that
// holds a sub-sample of a refined pixel, and the lanes (bit = lane) of those sub-samples.
struct alignas(16) FlagTile {
    uint32_t tile;
    uint32_t pad;
    unsigned long long mask;
};
static_assert(sizeof(FlagTile) == 16, "FlagTile must be 16 bytes");

// With supersampling n > 1 (rt_set_supersampling) every field down to npix describes the frame of SUB-SAMPLES: width n*W, local_rows
// n*rows, row0 n*row0, stripe n*stripe.  Internal column X is sub-sample X % n of pixel X / n, internal local row n*lr + sy is sub-row sy
// of output local row lr (Supersampling).  Only the primary-ray generator (raster_coord, lens_ray) and k_resolve look at ss / sso / out_*.
// The two pointers at the end are null for every frame but the two passes of an adaptive frame (Adaptive supersampling).
struct DFrame {              // which pixels this launch covers
    int32_t width, height;   // full frame
    int32_t local_rows;      // rows rendered by this shard
    int32_t row0, stripe, rank, nranks;
    int32_t tiles_x, tiles_y;
    uint32_t npix;           // local_rows * width
    int32_t max_depth;
    int32_t dyn_trace;       // k_trace pulls tiles from the sharded queue instead of static striding
    uint32_t item_cap, ray_cap;   // per-shard capacity of the shade-item and bounce-ray lists
    int32_t ss;              // supersampling n (1: one ray per pixel, the frame above IS the output frame)
    uint32_t ss_mul;         // ceil(2^32 / n) for n > 1: v / n == umulhi(v, ss_mul) for 0 <= v < 2^31 (no divide in the tile loop)
    // sub-sample offsets of this pass, evaluated on the host (rt_pass_offsets): [0, 4) for columns, [4, 8) for rows.  Pass 0 has
    // o[s] = (float)((2s + 1 - n) / (2.0 n)) in both halves; pass p > 0 shifts the halves by the radical inverses of p in bases 2 and 3
    float sso[2 * RT_MAX_SUPERSAMPLING];
    int32_t out_width, out_rows;       // the output frame k_resolve writes: W and the shard's rows (ss == 1: out_width * out_rows == npix)
    const int32_t *rows;               // pass 1: frame row of every local row (replaces the stripe formula); null: the formula
    const FlagTile *tiles;             // pass 2: the primary tiles are k_flag's list (count in Control::n_flag); null: every tile
    uint32_t tile_cap;                 // ... per-shard capacity of that list
    // thin lens (rt_set_lens, DESIGN.md §5, Depth of field).  null: the pinhole frame, by the pinhole instantiations of the primary kernels;
    // else T[RT_LENS_ROTATIONS][n*n] of this frame's n (device copy of rt_lens_table) and the LENS instantiations run.
    const float2 *lens;
    float lens_aperture, lens_focus;
    uint32_t lens_mul;                 // ceil(2^32 / (n*n)) for n > 1: v / (n*n) == umulhi(v, lens_mul) for v < 2^28 (lens or shutter on)
    // camera motion blur (rt_set_shutter, DESIGN.md §5, Motion blur).  0: every ray leaves the one camera *camp; 1: the SHUTTER instantiations
    // of the primary kernels run and blend a camera per lane from *camp and the DShutter behind it.  (The word fills what was padding: the
    // layout of the kernel arguments is what it was.)
    int32_t shutter;
    // multi-pass accumulation (rt_set_passes, DESIGN.md §5, Multi-pass accumulation): p * 0xC2B2AE35 of the pass p this launch belongs to, XORed
    // into the per-pixel scramble of lens_ray and shutter_time.  0 for pass 0 -- and only for pass 0 (an odd multiplier, p < 2^32) -- so
    // raster_coord also reads "pass 0" from it.  DFrame travels by value: every pass of an eager frame or of a captured graph carries its own.
    uint32_t pass_key;
    // primary culling (rt_set_primary_cull, DESIGN.md §5, Primary culling).  1: the pinhole one-ray instantiations of the primary kernels skip
    // the tiles outside DCamBlock::rect and k_resolve stores the background colour outside it without reading a record; 0: every tile is
    // traced (supersampling, lens, shutter, passes, adaptive frames, input rays, culling switched off).  (The word fills what was padding.)
    int32_t cull;
};
static_assert(sizeof(DFrame) == 160, "DFrame: 136 bytes + the row half of sso (16) + pass_key (4) + cull (4)");

#define RT_WORK_SHADOW 640
// Step counters of the counting build (-DRT_WORK_COUNTERS; RT_PROF_ADD in rt_kernels.hip): index k of a region of Control::prof.  The trace
// kernels (k_trace, k_stage and its leaf-task launch; flat scenes: also what k_shade and k_deep walk through flat_walk) add to prof[k], the shadow kernels (k_beam,
// k_pair_beam, k_shadow, k_shadow_shaft and their leaf-task launches) to prof[RT_WORK_SHADOW + k].  One wave-level step adds once (lane 0).
// bench.py and tools/work_trace.py read the counters by these values: none may move.
enum : int {
    WORK_TRI_STEPS_LANES_RAYS = 0,            // leaf_visit, flat_walk, shaft_leaf: triangle steps with lanes = rays (one per triangle, two per pair)
    WORK_TRI_USEFUL_LANES_RAYS = 1,           // leaf_visit: lanes of those steps whose ray is live; flat_walk: triangles of the root leaf kept by the unit's cull
    WORK_TRI_STEPS_LANES_TRIANGLES = 2,       // leaf_visit, shaft_leaf: (ray, 64-triangle chunk) steps with lanes = triangles
    WORK_TRI_USEFUL_LANES_TRIANGLES = 3,      // leaf_visit: lanes of those steps that hold a triangle to test
    WORK_BOX_STEPS_STACK_WALK = 4,            // packet_walk: child-box tests of the stack walk (all 64 rays at once)
    WORK_BOX_USEFUL_STACK_WALK = 5,           // packet_walk: lanes of those tests whose ray is live at the parent
    WORK_LEAVES_LANES_RAYS = 6,               // leaf_visit, flat_walk: leaf visits walked with lanes = rays
    WORK_LEAVES_LANES_TRIANGLES = 7,          // leaf_visit: leaf visits walked with lanes = triangles
    WORK_LEAF_LIVE_RAYS = 8,                  // leaf_visit: live rays summed over the lanes = triangles visits
    WORK_CHUNK_TESTS_STACK_WALK = 12,         // leaf_visit: chunk-bound tests (one per chunk, all 64 rays at once)
    WORK_UNITS = 13,                          // k_trace, k_stage, k_shadow, k_shadow_shaft: units (tiles, ray groups, shadow units, leaf tasks) taken from the queue
    WORK_RAY_CHUNK_PAIRS_CULLED = 14,         // leaf_visit: live rays that a chunk-bound test took off its chunk
    WORK_RAY_NODE_PAIRS_CONTENT_CULLED = 66,  // packet_walk: (ray, child) pairs dropped by the child's content box
    // 70-73, trace region: the lane = triangle CONE test of leaf_visit (packets with a common origin); shadow region: the lane = triangle
    // SHAFT test of shaft_leaf and, on flat scenes, the root-leaf cull of k_shadow (70 and 71 only)
    WORK_TRI_SHAFT_TESTS = 70,                // trace: chunks cone-tested; shadow: chunks shaft-tested (shaft_leaf), units whose root leaf was culled (k_shadow, flat)
    WORK_TRI_SHAFT_SURVIVORS = 71,            // trace: triangles inside the cone; shadow: triangles inside the shaft (shaft_leaf), triangles of the root leaf SKIPPED (k_shadow, flat)
    WORK_TRI_SHAFT_RAYS = 72,                 // live rays on the tested chunk (both regions)
    WORK_TRI_SHAFT_EMPTY_CHUNKS = 73,         // trace: chunks with no triangle inside the cone; shadow: with none inside the shaft
    WORK_NODE_TEST_LIVE_RAYS = 74,            // shaft_walk: live rays at the per-ray box test of a surviving child
    WORK_NODE_HIT_RAYS = 75,                  // shaft_walk: rays that hit it
    WORK_BEAMS_TESTED = 76,                   // k_beam (beam_tile: tiles of 64 hits), k_pair_beam ((hit, light) pairs)
    WORK_BEAMS_UNBLOCKED = 77,                // k_beam, k_pair_beam: beams that nothing can block
    WORK_BEAM_BAD_LEAF_CHECKS = 78,           // k_beam: hits checked against the never-culled leaves; k_pair_beam: unblocked pairs checked against them
    WORK_BEAM_BAD_LEAF_REACHED = 79,          // k_beam: hits that reach one; k_pair_beam: pairs that do
    WORK_BEAM_STEPS_OF_UNBLOCKED = 80,        // k_beam, k_pair_beam: budget spent by the unblocked beams
    WORK_BEAMS_OVER_BUDGET = 81,              // k_beam, k_pair_beam: beams that ran out of budget
    WORK_BEAM_GROUP_STEPS = 82,               // beam_walk: child groups popped
    WORK_BEAM_CHILDREN_IN_SHAFT = 83,         // beam_walk: their children that the beam's shaft does not cull
    WORK_BEAM_LEAF_VISITS = 84,               // beam_leaf: leaves visited
    WORK_BEAM_CHUNK_BATCHES = 85,             // beam_leaf: batches of up to 8 chunks
    WORK_BEAM_CHUNKS_TESTED_BY_TRIANGLE = 86, // beam_leaf: chunks of those batches tested triangle by triangle
    WORK_SHAFT_GROUPS = 88,                   // shaft_walk: child groups popped
    WORK_SHAFT_GROUP_CHILDREN = 89,           // shaft_walk: children in them
    WORK_NODES_TESTED_PER_RAY = 90,           // shaft_walk: children that survive the shaft test (each is then box-tested per ray)
    WORK_NODES_HIT = 91,                      // shaft_walk: children hit by some ray
    WORK_LEAF_CHUNK_BATCHES = 92,             // shaft_leaf: batches of up to 8 chunks
    WORK_LEAF_CHUNKS_IN_BATCHES = 93,         // shaft_leaf: chunks in them
    WORK_CHUNKS_TESTED_PER_RAY = 94,          // shaft_leaf: chunks that survive the shaft test (each is then bound-tested per ray)
    WORK_CHUNKS_WITH_WORK = 95,               // shaft_leaf: chunks left with a ray to test
};
#define RT_QUEUE_SHARDS 8
#define RT_STAT_SHARDS 64
// Compaction lists (shade items, bounce rays) are split into RT_LIST_SHARDS sub-lists, each with its own counter on its
// own 64-byte line: one returning atomicAdd per 64-pixel tile on a SINGLE counter serialises in the memory-side atomic
// unit at ~88 per us (9,000 tiles of cube.obj at 1080p = 0.1 ms, measured as the floor of k_trace and of k_shade).
// Element i of shard s lives at index s * cap + i; the producing tile/group number picks the shard (tile % RT_LIST_SHARDS),
// so the per-shard capacity is known up front.
#ifndef RT_LIST_SHARDS
#define RT_LIST_SHARDS 16
#endif
enum : int { ST_RAYS_PRIMARY = 0, ST_RAYS_BOUNCE, ST_RAYS_CENTRE, ST_RAYS_SAMPLE, ST_PIXELS_CULLED, ST_SHADED_HITS,
             ST_BOX_TESTS, ST_LEAF_TRI_REFS, ST_BOX_TESTS_SHADOW, ST_LEAF_TRI_REFS_SHADOW, ST_SAMPLE_WALKED, ST_REFINED };

// control block in device memory (zeroed once per frame by a memset node on the render stream)
struct Control {
    // work-queue heads: one set of RT_QUEUE_SHARDS counters per launch, each counter alone on a 64-byte line
    uint32_t queue[3 * (RT_MAX_DEPTH + 1) + 4][RT_QUEUE_SHARDS * 16];
    uint32_t n_items[RT_MAX_DEPTH + 1][RT_LIST_SHARDS * 16];   // lit hits per level and shard (counter s at [s * 16])
    uint32_t n_rays[RT_MAX_DEPTH + 2][RT_LIST_SHARDS * 16];    // bounce rays per level and shard (n_rays[0][0] = rt_trace_rays input count)
    // leaf tasks of the two traversal stages of the staged trace (closest hit q0 | light centre q1): RT_LIST_SHARDS sub-queues like
    // n_task_sh below, each counter on its own 64-byte line.  (ONE word per stage made the walking launches atomic-bound: dodge at 1080p
    // emits 5,878 + 3,417 tasks, one returning atomicAdd each, and one word serves ~88 of them per microsecond -- 67 and 39 us of the 80
    // and 91 us those launches took, whatever the walk itself cost.)
    uint32_t n_task_tr[RT_MAX_DEPTH + 1][2][RT_LIST_SHARDS * 16];
    // leaf tasks of the shadow kernels: RT_LIST_SHARDS sub-queues (producer block % RT_LIST_SHARDS), each counter on its own line --
    // one returning atomic per emitting leaf visit on a SINGLE word (~60k per dodge launch) ran into the ~88 per us limit
    uint32_t n_task_sh[RT_MAX_DEPTH + 1][RT_LIST_SHARDS * 16];
    uint32_t n_sitems[RT_MAX_DEPTH + 1][RT_LIST_SHARDS * 16];
    uint32_t beam_yield[RT_MAX_DEPTH + 1][RT_LIST_SHARDS * 16]; // k_beam's own brake: shard s (a line of its own) holds beams tested [16 s] / unblocked [16 s + 1] so far  // lit hits per level and shard that still need their sample shadow rays (k_beam's survivors)
    // totals, filled on the HOST by fold_stats() from the sharded counters below
    unsigned long long rays_primary, rays_bounce, rays_centre, rays_sample, pixels_culled, shaded_hits;
    unsigned long long box_tests, leaf_tri_refs;              // k_trace (closest hit + light-centre rays)
    unsigned long long box_tests_shadow, leaf_tri_refs_shadow; // k_shadow (area-light sample rays)
    unsigned long long sample_walked;                          // sample shadow segments that were actually formed (not decided by k_beam / the per-unit culling tests)
    // output pixels that the list builder of the frame listed: adaptive frames -- the pixels k_flag refined (rt_supersampling_refined reads it
    // for these frames alone); adaptive-pass frames -- the sum over the list passes of the pixels still active (k_pass_list; only
    // FrameShape::pixels reads it).  One frame is one kind, so the two never meet in one control block.
    unsigned long long refined;
    // what the kernels add to: one 128-byte line per shard, shard = blockIdx.x % RT_STAT_SHARDS.  (4096 waves adding
    // to ONE line at kernel end serialise in the memory-side atomic unit: measured 176 us for the 1080p primary k_trace
    // whose arithmetic needs < 20 us.)
    unsigned long long stat[RT_STAT_SHARDS][16];
    // adaptive frames: entries of k_flag's tile list per shard (counter s at [s * 16]).  Behind `stat`, so that the clear between the two
    // passes (kPassClearBytes: the queue and list counters of pass 1) keeps it and the counters of pass 1.  Adaptive-pass frames
    // (rt_set_pass_tolerance): k_pass_list's list for the next pass; the converging resolve of a pass zeroes it behind that pass's readers.
    uint32_t n_flag[RT_LIST_SHARDS * 16];
    // counting build (-DRT_WORK_COUNTERS) only: the WORK_* step counters above.  [0, 96): of the trace kernels; [RT_WORK_SHADOW, +96): of the
    // shadow kernels.  The words between and behind the two regions are never written (the size is what bench.py reads and the memset clears).
    unsigned long long prof[768];
    // LAST member, NOT covered by the per-frame memset (kFrameClearBytes): set by a kernel whose list reservation did not fit (never
    // expected: the capacities are derived from the tile counts).  Sticky, so that asynchronous frames (rt_render_device without stats,
    // graph replays) cannot lose it; every synchronising entry point turns it into an error and clears it.
    uint32_t overflow;
};
static const size_t kFrameClearBytes = offsetof(Control, overflow);
static const size_t kPassClearBytes = offsetof(Control, rays_primary);    // the per-level queue and list counters

// adaptive frames: k_flag group g holds the 16 tiles (g / 16) * 256 + g % 16 + 16 j of list shard g % 16 (one list reservation per group)
constexpr uint32_t flag_groups(uint32_t ntiles) { return (ntiles + 255u) / 256u * RT_LIST_SHARDS; }

inline void fold_stats(Control &h) {
    unsigned long long t[16] = {0};
    for (int sh = 0; sh < RT_STAT_SHARDS; ++sh)
        for (int k = 0; k < 16; ++k) t[k] += h.stat[sh][k];
    h.rays_primary = t[ST_RAYS_PRIMARY]; h.rays_bounce = t[ST_RAYS_BOUNCE]; h.rays_centre = t[ST_RAYS_CENTRE]; h.rays_sample = t[ST_RAYS_SAMPLE];
    h.pixels_culled = t[ST_PIXELS_CULLED]; h.shaded_hits = t[ST_SHADED_HITS];
    h.box_tests = t[ST_BOX_TESTS]; h.leaf_tri_refs = t[ST_LEAF_TRI_REFS];
    h.box_tests_shadow = t[ST_BOX_TESTS_SHADOW]; h.leaf_tri_refs_shadow = t[ST_LEAF_TRI_REFS_SHADOW];
    h.sample_walked = t[ST_SAMPLE_WALKED];
    h.refined = t[ST_REFINED];
}

// host side: what the resolve at the end of a launch sequence reads and writes (launch_resolve in rt_kernels.hip picks the
// k_resolve<SRC, SINK> instantiation and hands it the fields it reads)
struct ResolveArgs {
    const float4 *rec;
    const float *fres;
    float *out_rgb;
    uint8_t *out_u8;
    // pass 2 of an adaptive frame (refine != nullptr): k_flag's refine bytes, the one-ray colours C1 and the C1 rows of every output row
    const uint8_t *refine = nullptr;
    const float *c1 = nullptr;
    const int32_t *pos = nullptr;
    // pass `index` of a count > 1 frame (rt_set_passes): folded into the running sum `acc`, the last one stores the mean
    float *acc = nullptr;
    int index = 0, count = 1;
    // the frame's camera block (CamArg above); a frame with DFrame::cull set reads DCamBlock::rect of it
    CamArg cam{};
    // pass `index` of an adaptive-pass frame (rt_set_pass_tolerance, s2 != nullptr): the converging resolve.  `acc` is S1; S2 (float[3]), the
    // passes taken and the active byte per output pixel; the list counters (Control::n_flag) it zeroes for the list builder behind it
    float *s2 = nullptr;
    uint16_t *taken = nullptr;
    uint8_t *active = nullptr;
    uint32_t *n_flag = nullptr;
    int min_passes = 0;
    float tol = 0.0f;
};

}  // namespace rtamd
