// rt_capi.cpp -- implementation of the C ABI declared in include/rt_mi355x.h: context, scene upload,
// frame orchestration (a fixed, host-sync-free launch sequence per frame) and the host-scene wrappers.
// No CPU fallback exists here: without a HIP device every entry point that needs one fails loudly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host_scene.hpp"
#include "rt_ao_layout.hpp"
#include "rt_shadow_layout.hpp"
#include "rt_gather_layout.hpp"
#include "rt_probe_layout.hpp"
#include "rt_distance_layout.hpp"
#include "rt_hits_layout.hpp"
#include "rt_device.hpp"
#include "rt_frame_sets.hpp"
#include "rt_gbuffer_layout.hpp"
#include "rt_launch.hpp"
#include "rt_mi355x.h"
#include "rt_query_chunks.hpp"
#include "rt_scene_image.hpp"

using namespace rtamd;

struct rt_host_scene {
    HostScene hs;
};

// An owned device allocation: a pointer and its capacity in elements.  grow(n) frees and reallocates only when n exceeds the capacity (the
// contents are lost); the destructor frees.  Whoever grows a buffer that work in flight may read synchronises first.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t grow(size_t n) {
        if (n <= cap) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), n * sizeof(T));
        if (e == hipSuccess) cap = n; else p = nullptr;
        return e;
    }
    operator T *() const { return p; }
    T *operator->() const { return p; }
};

// how later frames are sampled: what the rt_set_* entry points validate and write
struct SampleSettings {
    int ss = 1;                  // supersampling n (rt_set_supersampling)
    float ss_tau = -1.0f;        // adaptive supersampling threshold (rt_set_supersampling_threshold; < 0: every pixel refined)
    float lens_aperture = 0.0f, lens_focus = 1.0f;   // thin lens (rt_set_lens; aperture 0: off)
    bool shutter_on = false;     // camera motion blur (rt_set_shutter) ...
    rt_camera shutter_close{};   // ... and the camera at shutter close
    int pass_first = 0, pass_count = 1;   // multi-pass accumulation (rt_set_passes): the frame is the mean of passes first .. first + count - 1
    float pass_tol = -1.0f;      // adaptive pass counts (rt_set_pass_tolerance): < 0 off ...
    int pass_min = 8;            // ... and the passes every pixel takes before the rule may stop it
    bool lens_on() const { return lens_aperture > 0.0f; }
    bool converge_on() const { return pass_tol >= 0.0f && pass_count > pass_min; }     // (pass_min >= 2: such a frame is a passes_on() frame)
    bool passes_on() const { return pass_first != 0 || pass_count != 1; }
    // (with the lens or the shutter on tau is ignored: the one-ray frame is sharp and cannot tell where blur will land)
    // (and with passes other than (0, 1): the rule compares one-ray frames, which a shifted or accumulated frame is not)
    bool adaptive_on() const { return ss > 1 && ss_tau >= 0.0f && !lens_on() && !shutter_on && !passes_on(); }
    // pinhole, one ray per pixel, the one pass 0: the frames whose primary kernels and resolve may cull (rt_set_primary_cull)
    bool cull_ok() const { return ss == 1 && !lens_on() && !shutter_on && !passes_on(); }
};

// The device buffers a frame reads besides the context's working set.  The context owns the set of its eager frames (rewritten or regrown by later
// calls, after a synchronise); a captured graph holds device pointers by value, so it owns a set of its own.
struct FrameTables {
    DevBuf<float> offsets;       // RT_LIGHT_SPHERE sample offsets
    DevBuf<int32_t> rows, pos;   // adaptive frames: the row tables
    DevBuf<float> acc;           // count > 1 frames (rt_set_passes): the running sum, float[3] per output pixel
    // adaptive-pass frames (rt_set_pass_tolerance): per output pixel the sum of squares S2 (float[3]), the passes taken and the active byte.
    // They grow together and `active` last: its capacity is the group's.
    DevBuf<float> s2;
    DevBuf<uint16_t> taken;
    DevBuf<uint8_t> active;
    hipError_t grow_conv(size_t pix) {
        hipError_t e = s2.grow(pix * 3);
        if (e == hipSuccess) e = taken.grow(pix);
        if (e == hipSuccess) e = active.grow(pix);
        return e;
    }
};
static constexpr double kConvBytes = 3.0 * sizeof(float) + sizeof(uint16_t) + sizeof(uint8_t);      // of those three, per output pixel

// What the statistics of a frame need of its plan (a graph and the deferred timing keep it after the frame).  The counters in the control block
// and the event sets sum over the frame's launch sequences.
struct FrameShape {
    int levels_run = 1;
    uint32_t sequences = 1;            // launch sequences: 1, the 2 passes of an adaptive frame, or the passes of rt_set_passes; a timed frame
                                       // records one set of frame_events(levels_run) events for each
    uint64_t pix_fixed = 0, pix_per_refined = 0;      // traced pixels: all of every pass, or (adaptive) pass 1's and n * n per refined pixel, or
                                                      // (adaptive passes) the whole-frame passes and n * n per pixel that a list pass still traced
    uint64_t pixels(uint64_t refined) const { return pix_fixed + pix_per_refined * refined; }
};

// One frame working set: everything the launches of a frame write and later launches of the same frame read, and the capacities.  The buffers
// grow together, to the running maximum of (pixels, levels) and of their own word counts.  A context holds two (rt_frame_sets.hpp; DESIGN.md
// §5, Frames in flight): set 0 is what every user but an overlapped frame works on -- graphs, queries, rt_render, stats, adaptive and pass
// frames -- and what captured graphs hold pointers into; set 1 exists from the first overlapped frame on.
struct FrameSet {
    size_t cap_pix = 0;
    int cap_levels = 0;
    DevBuf<RayItem> d_rays[2];
    DevBuf<ShadeItem> d_items;
    DevBuf<unsigned long long> d_vis;
    DevBuf<uint32_t> d_sidx;              // k_beam's survivors: item storage indices, 16 sub-lists like d_items
    DevBuf<uint8_t> d_done;               // k_pair_beam with several lights: one byte per (item slot, light)
    size_t cap_done = 0;                  // ... its (item slot, light) pairs (the allocation is 64 bytes longer)
    DevBuf<unsigned long long> d_best, d_lit;   // staged trace of tree scenes: closest-hit keys, centre-visibility masks
    DevBuf<float2> d_ltab;                // flat scenes, SIMPLE lights: k_beam's light-sample table (RT_LIGHT_TAB_ENTRIES pairs, allocated once: captured
                                          // graphs hold the pointer, every launch sequence rewrites the contents before it reads them)
    DevBuf<ContTask> d_tasks[2];          // continuation queues of k_shadow (tree scenes)
    DevBuf<float4> d_rec;
    DevBuf<float> d_fres;
    DevBuf<Control> d_ctl;
    void release() {
        cap_pix = 0; cap_levels = 0; cap_done = 0;
        d_rays[0].release(); d_rays[1].release(); d_items.release(); d_vis.release(); d_sidx.release(); d_done.release(); d_best.release(); d_lit.release();
        d_ltab.release(); d_tasks[0].release(); d_tasks[1].release(); d_rec.release(); d_fres.release(); d_ctl.release();
    }
};

struct rt_ctx {
    int device = 0;
    FrameSet fs[2];
    FrameSets sets;                       // which set a call gets, what it waits for and records (rt_frame_sets.hpp)
    hipStream_t fs_stream[2] = {nullptr, nullptr};   // the internal streams of the overlapped frames' launches up to the resolve, made with set 1
    hipEvent_t fs_event[4] = {};          // body_done[0], body_done[1], set_free[0], set_free[1] (FsEvent), timing disabled
    uint64_t overlapped_frames = 0;       // frames that took the overlapped route (rt_debug_overlapped_frames)
    int cus = 256;
    int occ_trace_primary = 4, occ_trace_rays = 4, occ_shadow = 4, occ_shaft = 4, occ_shade = 2, occ_beam = 4;   // resident blocks per CU
    hipStream_t stream = nullptr;
    std::string err;
    // scene
    bool has_scene = false;
    DScene S{};
    void *d_chunks = nullptr, *d_leaf_chunk0 = nullptr, *d_bad_leaves = nullptr;
    void *d_nodes = nullptr, *d_tris = nullptr, *d_tri_verts = nullptr, *d_face_normal = nullptr, *d_tri_vid = nullptr,
         *d_mat_id = nullptr, *d_vert_normal = nullptr, *d_mats = nullptr;
    bool reflective = false;     // some material spawns bounce rays (illum 3,4,5,6,9)
    bool flat = false;           // the root is a small leaf (cube.obj): specialised stack-free kernels
    float root_box[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // nodes[0].bmin / bmax as uploaded: what the primary kernels test first (primary_rect)
    bool primary_cull = true;    // rt_set_primary_cull: later pinhole one-ray frames skip the tiles outside the root box's projected rectangle
    int grid_mult = 1;
    int dyn_trace = 0;
    int staged_trace = 1;        // tree scenes: closest / centre / finish kernels with continuation tasks instead of the fused k_trace (0: an
                                 // experiment, and only for frames without lens, shutter and later passes: fused_tree_trace)
    SampleSettings smp;          // sampling of later frames
    FrameTables tab;             // offsets, row tables and running sum of the eager frames (acc: output pixels of the call)
    DevBuf<float2> d_lens;       // device copy of rt_lens_table for n = 1 .. RT_MAX_SUPERSAMPLING, back to back; made by the first lens frame, never
                                 // rewritten, freed with the context (captured graphs read it too)
    size_t mem_total = 0;        // the device's memory (hipMemGetInfo at rt_create): frames whose working set exceeds it are refused
    // frame buffers: set 0 under the names every user but the overlapped route knows them by
    size_t &cap_pix = fs[0].cap_pix;
    int &cap_levels = fs[0].cap_levels;
    DevBuf<RayItem> (&d_rays)[2] = fs[0].d_rays;
    DevBuf<ShadeItem> &d_items = fs[0].d_items;
    DevBuf<unsigned long long> &d_vis = fs[0].d_vis;
    DevBuf<uint32_t> &d_sidx = fs[0].d_sidx;
    DevBuf<uint8_t> &d_done = fs[0].d_done;
    size_t &cap_done = fs[0].cap_done;
    DevBuf<unsigned long long> &d_best = fs[0].d_best, &d_lit = fs[0].d_lit;
    DevBuf<float2> &d_ltab = fs[0].d_ltab;
    DevBuf<ContTask> (&d_tasks)[2] = fs[0].d_tasks;
    uint32_t task_cap = 1u << 21;
    uint32_t trace_budget = 500u;               // leaves above this estimated cost (VALU instructions) become tasks (0 = off); round 3 sweep after the task
                                                // counters were sharded: dodge trace 0.250 / 0.239 / 0.243 ms at 1000 / 500 / 250
    uint32_t shadow_budget = 3000u;
    bool beam_trees = false;
    uint32_t item_beam = 1;               // tree scenes, lights of more than 64 samples: the per-hit beam test (k_pair_beam) in front of k_shadow_shaft (RT_ITEM_BEAM=0: off, 2: also for one pass)
    int item_beam_blocks = 6;             // its workgroups per CU (6 waves per SIMD)
    bool deep = true;                     // flat scenes: levels 2 .. max_depth in ONE launch (k_deep); RT_NO_DEEP=1 keeps the four launches per level
    bool shadow_units = false;            // flat scenes: RT_SHADOW_UNITS=1 keeps the k_shadow launch that k_beam + k_shade otherwise fold away
    int shaft_min_samples = 33;           // tree scenes: sample counts from which a (hit, light) pair gets a wave of its own (k_shadow_shaft)
    uint32_t shaft_budget = 0u;           // the shaft walk culls per triangle: its leaves are cheap enough to stay inline (dodge 1080p: 1.31 -> 1.22 ms without tasks)
    uint32_t shaft_budget_deep = 3000u;   // ... but the bounce levels have few units and a heavy tail: their big leaves do go to a leaf-task launch (cfg4 29.2 -> 28.3 ms)
    int stage_mult = 2;                         // grid multiplier of the main k_stage launches (RT_STAGE_MULT): twice the resident grid lets
                                                // blocks of sky tiles retire early and evens out the object tiles (dodge trace 0.278 -> 0.254 ms)
    uint32_t task_target = 0u;                  // estimated cost of one leaf-task piece (0 = same as the budget); RT_TASK_TARGET, else set per scene at upload
    uint32_t trace_target = 1000u;              // ... of the trace stages: 1000 on small scenes, 4000 on big ones (cfg4 has > 130 k tasks per stage: trace 2.12 -> 1.76 ms;
                                                // dodge, 9 k tasks: 0.245 vs 0.256 ms the other way) -- by leaf references, see rt_upload_scene
    bool task_target_env = false;
    DevBuf<float4> &d_rec = fs[0].d_rec;
    DevBuf<float> &d_fres = fs[0].d_fres;
    DevBuf<Control> &d_ctl = fs[0].d_ctl;
    DevBuf<DCamBlock> d_cam;          // camera of the graph replay in flight (device memory: what a captured kernel reads), the shutter deltas behind it
    DCamBlock *h_cam_ring = nullptr;  // pinned staging ring for asynchronous camera uploads
    uint32_t cam_slot = 0;
    uint64_t frame_generation = 0;    // bumped whenever the frame buffers are reallocated (invalidates captured graphs)
    uint64_t scene_generation = 0;    // bumped by every rt_upload_scene: a captured graph holds the scene's device pointers by value
    hipEvent_t cam_events[512] = {};  // one per camera-ring slot: recorded after the slot's H2D copy, waited for before the slot is reused
    uint32_t frame_launches = 0;               // device operations (kernel launches + memsets) the launch sequences of the last frame enqueued
    int frame_wide_levels = 0;                 // levels of the last frame that ran the per-level kernel groups (the deeper ones went to k_deep)
    hipStream_t last_frame_stream = nullptr;   // stream of the most recent eager frame (it may still read `tab`)
    DevBuf<float> d_rgb;         // staging for rt_render (host output): they grow together (ensure_out)
    DevBuf<int32_t> d_hit;
    DevBuf<float> d_t;
    std::vector<hipEvent_t> events;
    // deferred timing (collect_stats == 2): events are not reused until rt_timing_collect
    size_t ev_base = 0;                       // first free event index
    std::vector<std::pair<size_t, int>> pending;   // (first event, levels_run) per frame
    hipStream_t pending_stream = nullptr;
    FrameShape pending_shape;                 // ... of the latest of them
    // adaptive frames (Adaptive supersampling): the one-ray colour C1 of pass 1, the refine bytes, k_flag's tile list ...
    DevBuf<float> d_c1;               // float[3] per pixel
    DevBuf<uint8_t> d_refine;
    DevBuf<FlagTile> d_flag;
    // ... and what the row tables of eager frames (tab.rows, tab.pos) hold: rewritten -- after a synchronise -- only when the rows change
    std::vector<int32_t> h_rowtab, h_pos;
    // rt_supersampling_refined: the count of the latest eager frame, on the host or (adaptive frames) still in the control block
    uint64_t refined = 0;
    bool refined_on_device = false;
    // rt_pass_map: the latest eager frame was an adaptive-pass frame of this many output pixels (tab.taken holds their counts)
    bool pass_map_on = false;
    size_t pass_map_pix = 0;
    // rt_set_query_chunk: rays per launch sequence of rt_trace_rays_device
    int32_t query_chunk = static_cast<int32_t>(kQueryChunkDefault);
    // rt_ambient_occlusion_device: the direction tables of m = 1 .. RT_AO_MAX_GRID and the (c, s) pairs (rt_ao_layout.hpp), made by the first
    // call that needs them, never rewritten, freed with the context
    DevBuf<float> d_ao_tab;
    // rt_light_probes_device: the probe directions of m = 1 .. RT_AO_MAX_GRID and their weights (rt_probe_layout.hpp), made by the first call,
    // never rewritten, freed with the context
    DevBuf<float> d_probe_tab;
    // rt_gbuffer_device: rt_pass_offsets of n = 1 .. RT_MAX_SUPERSAMPLING and every pass (rt_gbuffer_layout.hpp), made by the first call, never
    // rewritten, freed with the context
    DevBuf<float> d_gb_pass;
    // rt_closest_points_device: the query's own bounds of the uploaded scene (rt_distance_layout.hpp), made by the first call after an upload,
    // freed with the scene
    DevBuf<NearNode> d_near_nodes;
    DevBuf<NearTri> d_near_tris;
    DevBuf<NearNode> d_near_chunks;
    bool near_ready = false;
    uint32_t n_face_refs = 0, n_chunks = 0;         // of the uploaded scene
};

static constexpr uint32_t kCamRing = 512;   // camera uploads that may be queued before one is consumed
static const char *k_no_ctx = "rt_mi355x: null context";
static const char *k_shutter_mismatch = "shutter: the close camera's fovy, aspect and viewport must equal the open camera's (only the pose moves)";

#define HIPCHK(ctx, call)                                                                                      \
    do {                                                                                                       \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess) {                                                                                \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                    \
            return RT_ERR_HIP;                                                                                 \
        }                                                                                                      \
    } while (0)

// ---- the two frame working sets: rt_frame_sets.hpp decides, this executes (Frames in flight) -----------------------------
enum class LostStream { Tolerate, Report };
static rt_status wait_frames(rt_ctx *c, LostStream lost);
static hipStream_t fs_stream_of(const rt_ctx *c, const FsStream s, hipStream_t caller) {
    return s == FsStream::CALLER ? caller : c->fs_stream[s == FsStream::INTERNAL1 ? 1 : 0];
}
// every step but BODY and RESOLVE, which are the caller's
static rt_status fs_exec(rt_ctx *c, const FsStep &s, hipStream_t caller) {
    hipEvent_t ev = c->fs_event[static_cast<int>(s.event)];
    switch (s.op) {
    case FsStep::WAIT: HIPCHK(c, hipStreamWaitEvent(fs_stream_of(c, s.stream, caller), ev, 0)); break;
    case FsStep::RECORD: HIPCHK(c, hipEventRecord(ev, fs_stream_of(c, s.stream, caller))); break;
    case FsStep::HOST_WAIT_EVENT: HIPCHK(c, hipEventSynchronize(ev)); break;
    case FsStep::HOST_WAIT_STREAM: HIPCHK(c, hipStreamSynchronize(fs_stream_of(c, s.stream, caller))); break;
    case FsStep::HOST_WAIT_FRAMES: { const rt_status ws = wait_frames(c, LostStream::Tolerate); if (ws != RT_OK) return ws; if (caller) HIPCHK(c, hipStreamSynchronize(caller)); break; }
    default: break;
    }
    return RT_OK;
}
static rt_status fs_exec(rt_ctx *c, const FsSteps &q, hipStream_t caller) {
    for (int i = 0; i < q.n; ++i) { const rt_status s = fs_exec(c, q.step[i], caller); if (s != RT_OK) return s; }
    return RT_OK;
}
// the host waits for everything the overlapped frames have in flight (a context that never overlapped: nothing to do)
static rt_status wait_sets(rt_ctx *c) { return fs_exec(c, c->sets.host_wait(), nullptr); }
// any use of set 0 on `st` other than an overlapped frame: in front of the work, and behind it
// (a context that never overlapped asks nothing and does nothing; on a capturing stream neither happens: events recorded outside a capture
//  cannot be waited for inside it and a record inside it is no record -- whoever captures behind overlapped frames synchronises first)
static rt_status stream_capturing(rt_ctx *c, hipStream_t st, bool *capturing) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(c, hipStreamIsCapturing(st, &cap));
    *capturing = cap != hipStreamCaptureStatusNone;
    return RT_OK;
}
static rt_status set0_begin(rt_ctx *c, hipStream_t st, bool *capturing) {
    *capturing = false;
    if (!c->sets.ready()) return RT_OK;
    const rt_status s = stream_capturing(c, st, capturing);
    return s != RT_OK ? s : fs_exec(c, c->sets.before_set0_use(*capturing), st);
}
static rt_status set0_end(rt_ctx *c, hipStream_t st, bool capturing) { return fs_exec(c, c->sets.after_set0_use(capturing), st); }

// the stream of a call that takes one: the caller's, or the context's own for null
static hipStream_t stream_or_own(const rt_ctx *c, void *stream) { return stream ? static_cast<hipStream_t>(stream) : c->stream; }

// The device copies of an entry point on host pointers: in() uploads an array, out() makes room that finish() downloads into the host array
// (a null host pointer: a null device pointer and no download), room() is room alone.  finish(launch) runs `launch` -- the call's _device
// form, or a probe's launcher -- on the staged pointers, synchronises the context's stream and downloads.  The allocations are freed with
// the Staging, on every return path.  The first step that fails leaves its status in `status` and HIP's text in the context (HIPCHK), the
// steps after it do nothing and finish() returns it without launching.  (In an unnamed namespace: the library exports none of it.)
namespace {
struct Staging {
    rt_ctx *c;
    rt_status status;
    explicit Staging(rt_ctx *ctx) : c(ctx), status(use_device()) {}
    Staging(const Staging &) = delete;
    Staging &operator=(const Staging &) = delete;
    ~Staging() { for (void *p : owned) (void)hipFree(p); }
    template <typename T>
    T *room(size_t n) {
        void *p = nullptr;
        if (status == RT_OK && n != 0) status = alloc(&p, n * sizeof(T));
        return static_cast<T *>(p);
    }
    template <typename T>
    const T *in(const T *host, size_t n) {
        T *p = room<T>(n);
        if (p) status = copy(p, host, n * sizeof(T), hipMemcpyHostToDevice);
        return p;
    }
    template <typename T>
    T *out(T *host, size_t n) {
        T *p = host ? room<T>(n) : nullptr;
        if (p) downloads.push_back(Download{host, p, n * sizeof(T)});
        return p;
    }
    template <typename Launch>
    rt_status finish(Launch &&launch) {
        if (status != RT_OK || (status = launch()) != RT_OK) return status;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (const Download &d : downloads)
            if ((status = copy(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost)) != RT_OK) break;
        return status;
    }

private:
    struct Download {
        void *host;
        const void *dev;
        size_t bytes;
    };
    std::vector<void *> owned;
    std::vector<Download> downloads;
    rt_status use_device() { HIPCHK(c, hipSetDevice(c->device)); return RT_OK; }
    rt_status alloc(void **p, size_t bytes) {
        HIPCHK(c, hipMalloc(p, bytes));
        owned.push_back(*p);
        return RT_OK;
    }
    rt_status copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) { HIPCHK(c, hipMemcpy(dst, src, bytes, kind)); return RT_OK; }
};
}  // namespace

extern "C" const char *rt_version(void) { return "rt_mi355x 0.1 (gfx950)"; }

extern "C" void *rt_stream(rt_ctx *ctx) { return ctx ? static_cast<void *>(ctx->stream) : nullptr; }

extern "C" const char *rt_last_error(const rt_ctx *ctx) { return ctx ? ctx->err.c_str() : k_no_ctx; }

extern "C" void rt_destroy(rt_ctx *c);
extern "C" rt_status rt_create(rt_ctx **out, int device) {
    if (!out) return RT_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        std::fprintf(stderr, "rt_mi355x: no HIP device visible -- this library has no CPU fallback\n");
        return RT_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) return RT_ERR_NO_DEVICE;
    rt_ctx *c = new rt_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return RT_ERR_NO_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (const char *dt = std::getenv("RT_TRACE_DYNAMIC")) c->dyn_trace = std::atoi(dt) != 0;
    if (const char *sb = std::getenv("RT_SHADOW_BUDGET")) c->shadow_budget = static_cast<uint32_t>(std::atoi(sb));
    if (const char *sb = std::getenv("RT_SHAFT_BUDGET")) c->shaft_budget = c->shaft_budget_deep = static_cast<uint32_t>(std::atoi(sb));
    if (const char *sm = std::getenv("RT_SHAFT_MIN_SAMPLES")) c->shaft_min_samples = std::atoi(sm);
    if (const char *bt = std::getenv("RT_BEAM_TREES")) c->beam_trees = std::atoi(bt) != 0;
    if (const char *ib = std::getenv("RT_ITEM_BEAM")) c->item_beam = static_cast<uint32_t>(std::max(0, std::atoi(ib)));
    if (const char *ib = std::getenv("RT_ITEM_BEAM_BLOCKS")) c->item_beam_blocks = std::max(1, std::atoi(ib));
    if (std::getenv("RT_NO_DEEP")) c->deep = false;
    if (const char *su = std::getenv("RT_SHADOW_UNITS")) c->shadow_units = std::atoi(su) != 0;
    if (const char *sg = std::getenv("RT_STAGED_TRACE")) c->staged_trace = std::atoi(sg) != 0;
    if (const char *sm = std::getenv("RT_STAGE_MULT")) { const int v = std::atoi(sm); if (v >= 1 && v <= 8) c->stage_mult = v; }
    if (const char *tc = std::getenv("RT_TASK_CAP")) { const long v = std::atol(tc); if (v >= 64 && v <= (1l << 24)) c->task_cap = static_cast<uint32_t>(v); }
    if (const char *tt = std::getenv("RT_TASK_TARGET")) { c->task_target = static_cast<uint32_t>(std::atoi(tt)); c->task_target_env = true; }
    if (const char *tb = std::getenv("RT_TRACE_BUDGET")) c->trace_budget = static_cast<uint32_t>(std::atoi(tb));
    if (const char *gm = std::getenv("RT_GRID_MULT")) {          // tuning knob: grid = CUs x residency x mult
        const int m = std::atoi(gm);
        if (m > 0 && m <= 64) c->grid_mult = m;
    }
#ifdef RT_WORK_COUNTERS
    c->sets.set_on(false);       // (the counting build's step counters are read from set 0's control block: its frames stay on it)
#endif
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return RT_ERR_HIP; }
    { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess) c->mem_total = tot; }
    if (c->d_ctl.grow(1) != hipSuccess || c->d_cam.grow(1) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&c->h_cam_ring), sizeof(DCamBlock) * kCamRing, hipHostMallocDefault) != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return RT_ERR_HIP;
    }
    if (hipMemset(c->d_ctl, 0, sizeof(Control)) != hipSuccess) { rt_destroy(c); return RT_ERR_HIP; }
    *out = c;
    return RT_OK;
}

static void free_scene(rt_ctx *c) {
    void **p[] = {&c->d_bad_leaves, &c->d_chunks, &c->d_leaf_chunk0, &c->d_nodes, &c->d_tris, &c->d_tri_verts, &c->d_face_normal, &c->d_tri_vid, &c->d_mat_id, &c->d_vert_normal, &c->d_mats};
    for (void **q : p) { if (*q) (void)hipFree(*q); *q = nullptr; }
    c->d_near_nodes.release(); c->d_near_tris.release(); c->d_near_chunks.release(); c->near_ready = false;
    c->has_scene = false;
}

// (the device buffers free themselves with the context)
extern "C" void rt_destroy(rt_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)wait_sets(c);           // (the resolves of overlapped frames on the caller's streams, and the internal streams)
    free_scene(c);
    for (hipStream_t st : c->fs_stream) if (st) (void)hipStreamDestroy(st);
    for (hipEvent_t e : c->fs_event) if (e) (void)hipEventDestroy(e);
    if (c->h_cam_ring) (void)hipHostFree(c->h_cam_ring);
    for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->cam_events) if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

template <typename T>
static rt_status upload(rt_ctx *c, void **dst, const T *src, size_t n) {
    const size_t bytes = (n ? n : 1) * sizeof(T);
    HIPCHK(c, hipMalloc(dst, bytes));
    if (n) HIPCHK(c, hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
}

// host-only: builds the chunk bounds of a flattened scene (rt_scene_image.cpp) and reports {chunks, cullable chunks, leaves, max chunks per
// leaf}.  The bounds index tri_verts and face_normal by what face_refs holds; the validation in front is the upload's, whole, so a view that
// rt_upload_scene would refuse -- no materials, a bad mat_id or tri_vid entry included -- is refused here with the same status.
extern "C" rt_status rt_debug_chunk_stats(const rt_scene *sc, int32_t out[4]) {
    if (!out) return RT_ERR_INVALID;
    const SceneVerdict verdict = validate_scene(sc);
    if (verdict.status != RT_OK) return verdict.status;
    const ChunkSet k(sc, false);
    const std::vector<ChunkBound> &cbs = k.chunks;
    int cullable = 0, leaves = 0, maxc = 0;
    for (const ChunkBound &cb : cbs) cullable += cb.never < 1.5f ? 1 : 0;
    for (uint32_t i = 0; i < sc->n_nodes; ++i)
        if (sc->nodes[i].count_flags & RT_NODE_LEAF) {
            ++leaves;
            const int nc = static_cast<int>(((sc->nodes[i].count_flags & 0x7fffffffu) + 63u) / 64u);
            if (nc > maxc) maxc = nc;
        }
    out[0] = static_cast<int32_t>(cbs.size()); out[1] = cullable; out[2] = leaves; out[3] = maxc;
    return RT_OK;
}

// host-only: the chunk bounds themselves, 16 floats per chunk {lo[3], hi[3], never, infl, sn[3], slo, shi, 0, 0, 0}, the per-node index of a
// leaf's first chunk and the leaf face references in the order the chunks hold them (tests/test_host_scene.py checks the containment the
// culling rules rely on); it refuses what rt_debug_chunk_stats refuses
extern "C" rt_status rt_debug_chunk_bounds(const rt_scene *sc, float *bounds, int32_t cap_chunks, int32_t *n_chunks, uint32_t *leaf_chunk0_out, uint32_t *refs_out) {
    if (!n_chunks) return RT_ERR_INVALID;
    const SceneVerdict verdict = validate_scene(sc);
    if (verdict.status != RT_OK) return verdict.status;
    const ChunkSet k(sc, false);
    const std::vector<ChunkBound> &cbs = k.chunks;
    *n_chunks = static_cast<int32_t>(cbs.size());
    if (bounds) {
        if (cap_chunks < *n_chunks) return RT_ERR_INVALID;
        static_assert(sizeof(ChunkBound) == 16 * sizeof(float), "ChunkBound is 16 floats");
        std::memcpy(bounds, cbs.data(), cbs.size() * sizeof(ChunkBound));
    }
    if (leaf_chunk0_out) std::memcpy(leaf_chunk0_out, k.leaf_chunk0.data(), k.leaf_chunk0.size() * sizeof(uint32_t));
    if (refs_out) std::memcpy(refs_out, k.refs.data(), k.refs.size() * sizeof(uint32_t));
    return RT_OK;
}

extern "C" rt_status rt_upload_scene(rt_ctx *c, const rt_scene *sc) {
    if (!c) return RT_ERR_INVALID;
    if (!sc || !sc->nodes || sc->n_nodes == 0 || !sc->materials || sc->n_materials == 0) { c->err = "rt_upload_scene: empty scene"; return RT_ERR_INVALID; }
    if (sc->n_faces && (!sc->tri_verts || !sc->face_normal || !sc->tri_vid || !sc->mat_id || !sc->vert_normal)) { c->err = "rt_upload_scene: missing arrays"; return RT_ERR_INVALID; }
    HIPCHK(c, hipSetDevice(c->device));
    // validate indices and the depth bound of the traversal stack before anything reaches a kernel
    std::vector<int> depth(sc->n_nodes, 0);
    int max_depth = 0;
    for (uint32_t i = 0; i < sc->n_nodes; ++i) {
        const rt_node &n = sc->nodes[i];
        const uint32_t cnt = n.count_flags & 0x7fffffffu;
        if (n.count_flags & RT_NODE_LEAF) {
            if (static_cast<uint64_t>(n.first) + cnt > sc->n_face_refs) { c->err = "rt_upload_scene: leaf range outside face_refs"; return RT_ERR_INVALID; }
        } else {
            if (cnt > 8 || (cnt && (n.first <= i || static_cast<uint64_t>(n.first) + cnt > sc->n_nodes))) { c->err = "rt_upload_scene: bad child range"; return RT_ERR_INVALID; }
            for (uint32_t k = 0; k < cnt; ++k) depth[n.first + k] = depth[i] + 1;
        }
        if (depth[i] > max_depth) max_depth = depth[i];
    }
    if (max_depth > 16) { c->err = "rt_upload_scene: octree deeper than 16 levels (traversal stack bound)"; return RT_ERR_UNSUPPORTED; }
    for (uint32_t i = 0; i < sc->n_face_refs; ++i)
        if (sc->face_refs[i] >= sc->n_faces) { c->err = "rt_upload_scene: face ref out of range"; return RT_ERR_INVALID; }
    for (uint32_t f = 0; f < sc->n_faces; ++f) {
        if (sc->mat_id[f] < 0 || static_cast<uint32_t>(sc->mat_id[f]) >= sc->n_materials) { c->err = "rt_upload_scene: material id out of range"; return RT_ERR_INVALID; }
        for (int k = 0; k < 3; ++k)
            if (sc->tri_vid[f * 3 + k] >= sc->n_vert_normals) { c->err = "rt_upload_scene: vertex id outside vert_normal"; return RT_ERR_INVALID; }
    }

    // Leaf face lists are re-ordered along a Morton curve (the order inside a leaf cannot change any result: closest
    // hit is a minimum with a face-id tie-break, shadow rays are any-hit), so that every run of 64 references -- one
    // `chunk` of the lanes=triangles mode -- is spatially compact and its conservative bound is tight.
    const bool no_cull = std::getenv("RT_NO_CULL") != nullptr;
    const ChunkSet k(sc, no_cull);
    const std::vector<uint32_t> &refs = k.refs, &leaf_chunk0 = k.leaf_chunk0;
    const std::vector<ChunkBound> &cbs = k.chunks;
    const float extent = k.extent;

    // leaf-ordered triangle records: the per-triangle constants of rayTriangleIntersection (flyscene.cpp:787-811),
    // evaluated once with the same float operations the reference performs on every call
    std::vector<TriRec> recs(sc->n_face_refs);
    for (uint32_t i = 0; i < sc->n_face_refs; ++i) {
        const uint32_t f = refs[i];
        const float *v = sc->tri_verts + static_cast<size_t>(f) * 9;
        const float *n = sc->face_normal + static_cast<size_t>(f) * 3;
        TriRec &r = recs[i];
        const V3 A{v[0], v[1], v[2]}, B{v[3], v[4], v[5]}, C{v[6], v[7], v[8]}, N{n[0], n[1], n[2]};
        const V3 e0 = C - A, e1 = B - A;
        r.ax = A.x; r.ay = A.y; r.az = A.z;
        r.e0x = e0.x; r.e0y = e0.y; r.e0z = e0.z;
        r.e1x = e1.x; r.e1y = e1.y; r.e1z = e1.z;
        r.nx = N.x; r.ny = N.y; r.nz = N.z;
        r.nA = dot(N, A);
        r.d00 = dot(e0, e0); r.d01 = dot(e0, e1); r.d11 = dot(e1, e1);
        r.inv_denom = 1 / (r.d00 * r.d11 - r.d01 * r.d01);
        r.face = f;
        double edge_, binfl_;
        r.flags = (sc->materials[sc->mat_id[f]].illum == 9 ? 1u : 0u) | ((!never_hit(v, n) && tri_ill_conditioned(v, n, edge_, binfl_)) ? 2u : 0u);
        r.pad = 0u;
    }
    c->reflective = false;
    for (uint32_t m = 0; m < sc->n_materials; ++m) {
        const int il = sc->materials[m].illum;
        if (il == 9 || il == 6 || (il > 2 && il < 6)) c->reflective = true;
    }

    HIPCHK(c, hipStreamSynchronize(c->stream));      // nothing in flight may still read the old scene
    { const rt_status ws = wait_sets(c); if (ws != RT_OK) return ws; }
    free_scene(c);
    ++c->scene_generation;
    rt_status st;
    // device nodes = public nodes + content boxes, bottom-up (children always follow their parent in the array)
    std::vector<DNode> dnodes(sc->n_nodes);
    std::vector<float> bad_leaves;            // boxes of the leaves with a chunk that may never be culled (k_beam)
    for (uint32_t ii = sc->n_nodes; ii-- > 0;) {
        const rt_node &n = sc->nodes[ii];
        DNode &dn = dnodes[ii];
        std::memcpy(&dn, &n, sizeof(rt_node));
        const uint32_t cnt = n.count_flags & 0x7fffffffu;
        float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {1e30f, 1e30f, 1e30f};      // nothing inside: a far-away point
        bool any = false, open_box = false;
        auto grow = [&](const float *l, const float *h) {
            for (int k = 0; k < 3; ++k) {
                lo[k] = any ? std::fmin(lo[k], l[k]) : l[k];
                hi[k] = any ? std::fmax(hi[k], h[k]) : h[k];
            }
            any = true;
        };
        if (n.count_flags & RT_NODE_LEAF) {
            for (uint32_t k = 0; k < (cnt + 63u) / 64u; ++k) {
                const ChunkBound &cb = cbs[leaf_chunk0[ii] + k];
                if (cb.never >= 1.5f) open_box = true; else grow(cb.lo, cb.hi);
            }
            if (open_box) { for (int k = 0; k < 3; ++k) bad_leaves.push_back(n.bmin[k]); for (int k = 0; k < 3; ++k) bad_leaves.push_back(n.bmax[k]); }
        } else {
            for (uint32_t k = 0; k < cnt; ++k) {
                const DNode &ch = dnodes[n.first + k];
                if (ch.pad[1]) open_box = true;
                if (!(ch.clo[0] >= 1e30f)) grow(ch.clo, ch.chi);
            }
        }
        // The content box bounds the CULLABLE chunks below; pad[1] = 1 marks a subtree that also holds a chunk that may never be skipped
        // (a degenerate / ill-conditioned triangle inside): the walk then descends on the reference's own box test alone and the leaf's
        // cullable chunks are still skipped one by one.  (Opening the whole content box instead let 15 sliver triangles of
        // dodgeColorTest.obj -- 23 of its 437 chunks -- switch the content culling off for most of the top of the tree.)
        bool finite = true;
        for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(lo[k]) && std::isfinite(hi[k]);
        if (!finite) open_box = true;
        for (int k = 0; k < 3; ++k) {
            dn.clo[k] = finite ? lo[k] : 1e30f;
            dn.chi[k] = finite ? hi[k] : 1e30f;
        }
        dn.pad[0] = (n.count_flags & RT_NODE_LEAF) ? leaf_chunk0[ii] : 0u;
        dn.pad[1] = open_box ? 1u : 0u;
    }
    if ((st = upload(c, &c->d_nodes, dnodes.data(), dnodes.size())) != RT_OK) return st;
    if ((st = upload(c, &c->d_tris, recs.data(), recs.size())) != RT_OK) return st;
    if ((st = upload(c, &c->d_chunks, cbs.data(), cbs.size())) != RT_OK) return st;
    if ((st = upload(c, &c->d_leaf_chunk0, leaf_chunk0.data(), leaf_chunk0.size())) != RT_OK) return st;
    const size_t n_bad = bad_leaves.size() / 6;
    if (bad_leaves.empty()) bad_leaves.assign(6, 0.0f);
    if ((st = upload(c, &c->d_bad_leaves, bad_leaves.data(), bad_leaves.size())) != RT_OK) return st;
    if ((st = upload(c, &c->d_tri_verts, sc->tri_verts, static_cast<size_t>(sc->n_faces) * 9)) != RT_OK) return st;
    if ((st = upload(c, &c->d_face_normal, sc->face_normal, static_cast<size_t>(sc->n_faces) * 3)) != RT_OK) return st;
    if ((st = upload(c, &c->d_tri_vid, sc->tri_vid, static_cast<size_t>(sc->n_faces) * 3)) != RT_OK) return st;
    if ((st = upload(c, &c->d_mat_id, sc->mat_id, sc->n_faces)) != RT_OK) return st;
    if ((st = upload(c, &c->d_vert_normal, sc->vert_normal, static_cast<size_t>(sc->n_vert_normals) * 3)) != RT_OK) return st;
    if ((st = upload(c, &c->d_mats, sc->materials, sc->n_materials)) != RT_OK) return st;
    c->S.nodes = static_cast<const DNode *>(c->d_nodes);
    c->S.leaf_tris = static_cast<const TriRec *>(c->d_tris);
    c->S.chunks = static_cast<const ChunkBound *>(c->d_chunks);
    c->S.leaf_chunk0 = static_cast<const uint32_t *>(c->d_leaf_chunk0);
    c->S.bad_leaves = static_cast<const float *>(c->d_bad_leaves);
    c->S.n_bad_leaves = n_bad <= 32 ? static_cast<uint32_t>(n_bad) : 0xffffffffu;
    c->S.extent = extent;
    c->S.tri_verts = static_cast<const float *>(c->d_tri_verts);
    c->S.face_normal = static_cast<const float *>(c->d_face_normal);
    c->S.tri_vid = static_cast<const uint32_t *>(c->d_tri_vid);
    c->S.mat_id = static_cast<const int32_t *>(c->d_mat_id);
    c->S.vert_normal = static_cast<const float *>(c->d_vert_normal);
    c->S.mats = static_cast<const rt_material *>(c->d_mats);
    std::memcpy(c->S.model, sc->model, sizeof(float) * 12);
    c->S.n_nodes = sc->n_nodes;
    c->S.n_faces = sc->n_faces;
    c->n_face_refs = sc->n_face_refs; c->n_chunks = static_cast<uint32_t>(cbs.size());
    c->S.queue_local = -1;        // auto (rt_kernels.hip, k_shadow); RT_QUEUE_LOCAL=n forces chunks of n consecutive units, 0 the strided mode
    if (const char *ql = std::getenv("RT_QUEUE_LOCAL")) c->S.queue_local = std::atoi(ql);
    c->S.plane_cull = (no_cull || std::getenv("RT_NO_PLANE_CULL") != nullptr) ? 0 : 1;
    c->S.queue_div = 12;          // (units / (waves x 12) per chunk: dodge 1.125 -> 1.112 ms against 6, measured at the kernel's full residency)
    if (const char *qd = std::getenv("RT_QUEUE_DIV")) { const int v = std::atoi(qd); if (v >= 1 && v <= 4096) c->S.queue_div = v; }
    c->S.shaft = (no_cull || std::getenv("RT_NO_SHAFT") != nullptr) ? 0 : 1;
    c->S.beam = (no_cull || std::getenv("RT_NO_BEAM") != nullptr) ? 0 : 1;
    c->S.beam_budget = 1024;
    if (const char *bb = std::getenv("RT_BEAM_BUDGET")) { const int v = std::atoi(bb); if (v >= 1 && v <= (1 << 20)) c->S.beam_budget = v; }
    if (sc->n_nodes >= (1u << 28)) { c->err = "rt_upload_scene: more than 2^28 nodes"; return RT_ERR_UNSUPPORTED; }
    c->flat = (sc->nodes[0].count_flags & RT_NODE_LEAF) && (sc->nodes[0].count_flags & 0x7fffffffu) <= 64u;
    std::memcpy(c->root_box, sc->nodes[0].bmin, sizeof(float) * 3);
    std::memcpy(c->root_box + 3, sc->nodes[0].bmax, sizeof(float) * 3);
    { const uint32_t t = sc->n_face_refs / 256u; c->trace_target = t < 1000u ? 1000u : (t > 4000u ? 4000u : t); }
    query_occupancy(c->flat, &c->occ_trace_primary, &c->occ_trace_rays, &c->occ_shadow, &c->occ_shaft, &c->occ_shade, &c->occ_beam);
    // k_trace uses static tile striding: with more than ~4 blocks/CU a wave owns so few tiles (32,400 tiles at 1080p)
    // that heavy object tiles no longer average out (measured 0.26 ms at 4 blocks/CU vs 0.38 ms at 7-8)
    int trace_cap = 6;         // (round 3, RT_TRACE_OCC sweep on the cube frame: 3 / 4 / 5 / 6 / 8 blocks per CU -> trace group 76 / 80 / 76 / 68 / 78 us; round 1's cap of 4
                               // dated from the single-counter compaction lists)
    if (const char *tc = std::getenv("RT_TRACE_OCC")) { const int v = std::atoi(tc); if (v >= 1 && v <= 8) trace_cap = v; }
    if (c->occ_trace_primary > trace_cap) c->occ_trace_primary = trace_cap;
    if (c->occ_trace_rays > trace_cap) c->occ_trace_rays = trace_cap;
    c->occ_trace_primary *= c->grid_mult; c->occ_trace_rays *= c->grid_mult; c->occ_shadow *= c->grid_mult; c->occ_shaft *= c->grid_mult; c->occ_shade *= c->grid_mult;
    c->has_scene = true;
    return RT_OK;
}

extern "C" int32_t rt_local_rows(const rt_params *p) {
    if (!p || p->stripe <= 0 || p->nranks <= 0 || p->row1 < p->row0) return 0;
    int32_t n = 0;
    for (int32_t y = p->row0; y < p->row1; ++y)
        if (((y - p->row0) / p->stripe) % p->nranks == p->rank) ++n;
    return n;
}

// Waits for every frame that may still read the context's buffers: those on its own stream and those on the caller's stream of the most recent
// eager frame.  That caller's stream may have been destroyed since.  Tolerate: it has no work left then, its error is not ours, and the handle
// is dropped; Report: its error is the call's.
static rt_status wait_frames(rt_ctx *c, LostStream lost) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    { const rt_status ws = wait_sets(c); if (ws != RT_OK) return ws; }
    if (c->last_frame_stream && c->last_frame_stream != c->stream) {
        if (lost == LostStream::Report) HIPCHK(c, hipStreamSynchronize(c->last_frame_stream));
        else if (hipStreamSynchronize(c->last_frame_stream) != hipSuccess) (void)hipGetLastError();
    }
    if (lost == LostStream::Tolerate) c->last_frame_stream = nullptr;
    return RT_OK;
}

// `own` (rt_graph_create): the sphere offsets go to the caller's buffer instead of the context's -- a captured graph holds the pointer by
// value, so it must not be the buffer later calls rewrite or reallocate.
static rt_status check_lights(rt_ctx *c, const rt_lights *l, DLights *out, DevBuf<float> *own = nullptr) {
    if (!l || l->n_lights < 1 || l->n_lights > RT_MAX_LIGHTS) { c->err = "lights: n_lights must be in 1..25 (the reference overflows bool[25] beyond)"; return RT_ERR_INVALID; }
    if (l->mode != RT_LIGHT_POINT && l->mode != RT_LIGHT_AREA && l->mode != RT_LIGHT_SPHERE) { c->err = "lights: mode must be point, area or sphere"; return RT_ERR_INVALID; }
    int ns = 1;
    if (l->mode == RT_LIGHT_SPHERE) {
        if (l->n_offsets < 1 || l->n_offsets > RT_MAX_SAMPLES || !l->offsets) { c->err = "lights: sphere mode needs 1..1024 offsets"; return RT_ERR_INVALID; }
        ns = l->n_offsets;
    }
    if (l->mode == RT_LIGHT_AREA) {
        if (l->usteps < 1 || l->vsteps < 1 || static_cast<long>(l->usteps) * l->vsteps > RT_MAX_SAMPLES) { c->err = "lights: usteps*vsteps must be in 1..1024"; return RT_ERR_INVALID; }
        ns = l->usteps * l->vsteps;
    }
    std::memset(out, 0, sizeof *out);
    std::memcpy(out->pos, l->pos, sizeof out->pos);
    std::memcpy(out->color, l->color, sizeof out->color);
    out->n_lights = l->n_lights; out->mode = l->mode;
    out->usteps = l->mode == RT_LIGHT_AREA ? l->usteps : 1;
    out->vsteps = l->mode == RT_LIGHT_AREA ? l->vsteps : 1;
    out->n_samples = ns; out->len_x = l->len_x; out->len_y = l->len_y;
    out->offsets = nullptr;
    if (l->mode == RT_LIGHT_SPHERE) {
        // the offsets travel to a device buffer (synchronous copy: sphere mode is not a latency path); their box bounds the samples
        // (a frame in flight may still read the context's buffer)
        if (!own) { const rt_status ws = wait_frames(c, LostStream::Tolerate); if (ws != RT_OK) return ws; }
        DevBuf<float> &buf = own ? *own : c->tab.offsets;
        HIPCHK(c, buf.grow(static_cast<size_t>(ns) * 3));
        HIPCHK(c, hipMemcpy(buf, l->offsets, static_cast<size_t>(ns) * 3 * sizeof(float), hipMemcpyHostToDevice));
        out->offsets = buf;
        for (int k = 0; k < 3; ++k) { out->obox[k] = l->offsets[k]; out->obox[3 + k] = l->offsets[k]; }
        for (int i = 1; i < ns; ++i)
            for (int k = 0; k < 3; ++k) {
                out->obox[k] = std::fmin(out->obox[k], l->offsets[i * 3 + k]);
                out->obox[3 + k] = std::fmax(out->obox[3 + k], l->offsets[i * 3 + k]);
            }
    }
    return RT_OK;
}

// Sizes of the per-frame lists.  `tiles` bounds the dense tile/group numbering of every level: the primary 8x8 tiles, or
// ceil(n/64) + RT_LIST_SHARDS for a sharded list of n <= npix elements (each shard rounds up to whole groups of 64).  A
// list shard receives the elements of every RT_LIST_SHARDS-th tile, hence the per-shard capacity.
static size_t frame_tiles(const DFrame &F) {
    return std::max(static_cast<size_t>(F.tiles_x) * static_cast<size_t>(F.tiles_y), static_cast<size_t>(F.npix) / 64 + 1 + RT_LIST_SHARDS);
}
static uint32_t list_cap(size_t tiles) { return static_cast<uint32_t>(((tiles + RT_LIST_SHARDS - 1) / RT_LIST_SHARDS + 1) * 64); }

// the buffers only an adaptive frame has: C1 (pixels of pass 1), the refine bytes (output pixels), k_flag's tile list (entries, all shards)
struct AdaptiveSizes {
    size_t c1_pix = 0, out_pix = 0, flag_entries = 0;      // all 0: not an adaptive frame
};

// What a frame needs of the context's buffers.  acc_pix: output pixels of a count > 1 frame (rt_set_passes), 0 otherwise; conv_pix: output
// pixels of an adaptive-pass frame (rt_set_pass_tolerance: S2, taken, active), 0 otherwise.
struct WorkingSet {
    size_t npix;
    int levels;
    size_t samples_words, tiles, lslots;
    AdaptiveSizes ad;
    size_t acc_pix = 0, conv_pix = 0;
};
static WorkingSet working_set(const DLights &L, const DFrame &F) {
    return WorkingSet{F.npix, F.max_depth + 1, (static_cast<size_t>(L.n_samples) + 63) / 64, frame_tiles(F), static_cast<size_t>(L.n_lights), {}, 0, 0};
}

// device bytes of one working set at these capacities (pixels, levels, visibility / lit words, closest-hit slots; lights per item slot)
static double set_bytes(const rt_ctx *c, size_t np, int lv, size_t vw, size_t lw, size_t bs, size_t lslots) {
    return static_cast<double>(np) * (2.0 * sizeof(RayItem) + sizeof(ShadeItem) + sizeof(uint32_t) + static_cast<double>(lv) * (sizeof(float4) + sizeof(float)) +
                                      (lslots > 1 ? static_cast<double>(lslots) : 0.0)) +
           8.0 * (static_cast<double>(vw) + static_cast<double>(lw) + static_cast<double>(bs)) + 2.0 * static_cast<double>(c->task_cap) * sizeof(ContTask);
}

// (re)allocates the buffers of a set that grow together; nothing in flight may use them (the caller has waited)
static rt_status grow_set(rt_ctx *c, FrameSet &w, size_t np, int lv, size_t vw, size_t bs, size_t lw) {
    w.cap_pix = 0; w.cap_levels = 0;           // (a failure below leaves the group to be sized again)
    w.d_done.release(); w.cap_done = 0;        // (sized by cap_pix: ensure_frame, ensure_second_set)
    HIPCHK(c, w.d_rays[0].grow(np));
    HIPCHK(c, w.d_rays[1].grow(np));
    HIPCHK(c, w.d_items.grow(np));
    HIPCHK(c, w.d_vis.grow(vw));
    HIPCHK(c, w.d_sidx.grow(np));
    // staged trace: one 64-bit closest-hit key per ray slot of every 8x8 tile (tiles are padded to 64 lanes), lit masks per (tile, light)
    HIPCHK(c, w.d_best.grow(bs));
    HIPCHK(c, w.d_lit.grow(lw));
    HIPCHK(c, w.d_tasks[0].grow(c->task_cap));
    HIPCHK(c, w.d_tasks[1].grow(c->task_cap));
    HIPCHK(c, w.d_rec.grow(np * static_cast<size_t>(lv)));
    HIPCHK(c, w.d_fres.grow(np * static_cast<size_t>(lv)));
    w.cap_pix = np; w.cap_levels = lv;
    return RT_OK;
}

// acc_own: the caller (a graph) allocates the accumulator and the pass statistics itself.  The accounting below covers the context's buffers and
// those being asked for; the ones of graphs captured earlier (12 + 15 bytes per output pixel each) are not in it.
static rt_status ensure_frame(rt_ctx *c, const WorkingSet &w, bool acc_own = false) {
    const size_t lslots = w.lslots, lit_words = w.tiles * lslots, best_slots = w.tiles * 64;
    const size_t npix = std::max(w.npix, static_cast<size_t>(list_cap(w.tiles)) * RT_LIST_SHARDS);   // list storage (all shards)
    const size_t vis_words = npix * lslots * w.samples_words;
    const AdaptiveSizes &ad = w.ad;
    if (c->d_ltab.cap == 0) HIPCHK(c, c->d_ltab.grow(RT_LIGHT_TAB_ENTRIES));      // (12.5 KB, never regrown: no frame in flight reads it yet)
    const size_t cap_acc = c->tab.acc.cap / 3, cap_conv = c->tab.active.cap;
    const bool grow = npix > c->cap_pix || w.levels > c->cap_levels || vis_words > c->d_vis.cap || lit_words > c->d_lit.cap || best_slots > c->d_best.cap;
    const bool grow_ad = 3 * ad.c1_pix > c->d_c1.cap || ad.out_pix > c->d_refine.cap || ad.flag_entries > c->d_flag.cap;
    const bool grow_acc = !acc_own && (w.acc_pix > cap_acc || w.conv_pix > cap_conv);
    if (grow || grow_ad || grow_acc || (acc_own && (w.acc_pix != 0 || w.conv_pix != 0))) {
        const size_t np = std::max(npix, c->cap_pix);
        const int lv = std::max(w.levels, c->cap_levels);
        const size_t vw = std::max(vis_words, c->d_vis.cap), lw = std::max(lit_words, c->d_lit.cap), bs = std::max(best_slots, c->d_best.cap);
        const size_t a1 = std::max(3 * ad.c1_pix, c->d_c1.cap), ar = std::max(ad.out_pix, c->d_refine.cap), af = std::max(ad.flag_entries, c->d_flag.cap);
        // a frame that cannot fit is refused while the current buffers are still in place (a supersampled frame needs n*n times the
        // per-pixel buffers: 25 lights x 1024 samples at 4K with n = 4 is ~420 GB of visibility words alone)
        const double need = set_bytes(c, np, lv, vw, lw, bs, lslots) +
                            static_cast<double>(a1) * sizeof(float) + static_cast<double>(ar) + static_cast<double>(af) * sizeof(FlagTile) +
                            (static_cast<double>(acc_own ? w.acc_pix + cap_acc : std::max(w.acc_pix, cap_acc))) * 3.0 * sizeof(float) +
                            (static_cast<double>(acc_own ? w.conv_pix + cap_conv : std::max(w.conv_pix, cap_conv))) * kConvBytes;
        if (c->mem_total != 0 && need > static_cast<double>(c->mem_total)) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "frame working set %.1f GB exceeds the device's %.1f GB", need / 1e9, static_cast<double>(c->mem_total) / 1e9);
            c->err = buf;
            return RT_ERR_UNSUPPORTED;
        }
        if (grow_acc) {      // (no captured graph reads the context's accumulator: the generation stays)
            const rt_status ws = wait_frames(c, LostStream::Report);
            if (ws != RT_OK) return ws;
            HIPCHK(c, c->tab.acc.grow(w.acc_pix * 3));
            HIPCHK(c, c->tab.grow_conv(w.conv_pix));
        } else if (grow || grow_ad) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            const rt_status ws = wait_sets(c);
            if (ws != RT_OK) return ws;
        }
        if (grow_ad) {
            HIPCHK(c, c->d_c1.grow(a1));
            HIPCHK(c, c->d_refine.grow(ar));
            HIPCHK(c, c->d_flag.grow(af));
            ++c->frame_generation;
        }
        if (grow) {
            const rt_status gs = grow_set(c, c->fs[0], np, lv, vw, bs, lw);
            if (gs != RT_OK) return gs;
            ++c->frame_generation;
        }
    }
    // k_pair_beam's (item, light) bytes: only frames with several lights use them
    if (lslots > 1 && c->cap_pix * lslots > c->cap_done) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        { const rt_status ws = wait_sets(c); if (ws != RT_OK) return ws; }
        c->d_done.release(); c->cap_done = 0;
        HIPCHK(c, c->d_done.grow(c->cap_pix * lslots + 64));
        c->cap_done = c->cap_pix * lslots;
        ++c->frame_generation;
    }
    return RT_OK;
}

// The second working set, the internal streams and the events of the overlapped route: made by the first frame that takes the route and grown
// to set 0's capacities whenever those have grown (ensure_frame has just reserved set 0 for the frame).  *ok = false: the two sets do not fit
// the device together -- the second one is given up and this context takes the one-set route from now on.  Growth waits for everything in
// flight first.  Captured graphs hold set-0 pointers only: the generation stays.
static rt_status ensure_second_set(rt_ctx *c, hipStream_t caller, bool *ok) {
    const FrameSet &a = c->fs[0];
    FrameSet &b = c->fs[1];
    *ok = true;
    const bool grow = b.cap_pix < a.cap_pix || b.cap_levels < a.cap_levels || b.d_vis.cap < a.d_vis.cap || b.d_lit.cap < a.d_lit.cap || b.d_best.cap < a.d_best.cap;
    const bool grow_done = b.cap_done < a.cap_done;
    if (c->sets.ready() && !grow && !grow_done) return RT_OK;
    const double need = 2.0 * set_bytes(c, a.cap_pix, a.cap_levels, a.d_vis.cap, a.d_lit.cap, a.d_best.cap, a.cap_pix ? a.cap_done / a.cap_pix : 0) +
                        static_cast<double>(c->d_c1.cap) * sizeof(float) + static_cast<double>(c->d_refine.cap) + static_cast<double>(c->d_flag.cap) * sizeof(FlagTile) +
                        static_cast<double>(c->tab.acc.cap) * sizeof(float) + static_cast<double>(c->tab.active.cap) * kConvBytes;
    if (c->sets.ready() || c->sets.outstanding(0)) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const rt_status ws = wait_sets(c);
        if (ws != RT_OK) return ws;
    }
    if (c->mem_total != 0 && need > static_cast<double>(c->mem_total)) {
        c->fs[1].release();
        c->sets.refuse();
        *ok = false;
        return RT_OK;
    }
    for (int k = 0; k < 2; ++k)
        if (!c->fs_stream[k]) HIPCHK(c, hipStreamCreateWithFlags(&c->fs_stream[k], hipStreamNonBlocking));
    for (hipEvent_t &e : c->fs_event)
        if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (!b.d_ctl.p) {
        HIPCHK(c, b.d_ctl.grow(1));
        HIPCHK(c, hipMemset(b.d_ctl, 0, sizeof(Control)));
    }
    if (b.d_ltab.cap == 0) HIPCHK(c, b.d_ltab.grow(RT_LIGHT_TAB_ENTRIES));
    if (grow) {
        const rt_status gs = grow_set(c, b, a.cap_pix, a.cap_levels, a.d_vis.cap, a.d_best.cap, a.d_lit.cap);
        if (gs != RT_OK) return gs;
    }
    if (b.cap_done < a.cap_done) {
        b.d_done.release(); b.cap_done = 0;
        HIPCHK(c, b.d_done.grow(a.cap_done + 64));
        b.cap_done = a.cap_done;
    }
    return fs_exec(c, c->sets.first_overlap(), caller);      // (the first time only: the uses of set 0 so far left no record)
}

static hipEvent_t event_at(rt_ctx *c, size_t i) {
    while (c->events.size() <= i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        c->events.push_back(e);
    }
    return c->events[i];
}

// asynchronous camera upload through the pinned ring, in front of a graph replay (an eager frame passes its camera as a kernel argument and
// uploads nothing): a slot is only rewritten after the copy that last read it has completed
// (the whole block travels: the camera, the shutter deltas behind it -- zero when the shutter is off -- and the cull rectangle at the tail)
static rt_status upload_camera(rt_ctx *c, const DCamBlock &dc, hipStream_t st) {
    const uint32_t slot_i = c->cam_slot++ % kCamRing;
    if (c->cam_events[slot_i]) HIPCHK(c, hipEventSynchronize(c->cam_events[slot_i]));
    else HIPCHK(c, hipEventCreateWithFlags(&c->cam_events[slot_i], hipEventDisableTiming));
    DCamBlock *slot = &c->h_cam_ring[slot_i];
    *slot = dc;
    HIPCHK(c, hipMemcpyAsync(c->d_cam, slot, sizeof(DCamBlock), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(c->cam_events[slot_i], st));
    return RT_OK;
}

// events one launch sequence of a frame records when timed: start, three per level, end
static size_t frame_events(int levels_run) { return static_cast<size_t>(3 * levels_run + 2); }

// levels that run: the bounce levels can only be populated when some material reflects / refracts
static int levels_run_of(const rt_ctx *c, const DFrame &F) { return c->reflective ? F.max_depth + 1 : 1; }

// One launch sequence: what it traces, where it stands in its frame and where its results go.
struct Sequence {
    DFrame F;
    bool primary = true;       // primary rays from the camera; else n_input_rays rays in d_rays[0] (rt_trace_rays)
    bool count = false;        // the counting pass: the no-early-out traversal variants
    int timed = 0;             // 1: an event between every pair of launch groups (per-kernel breakdown; adds ~4 us per boundary)
                               // 2: the same events for timed loops, read back later (rt_timing_collect)
    uint32_t n_input_rays = 0;
    float *d_rgb = nullptr;
    uint8_t *d_u8 = nullptr;
    int32_t *d_hit = nullptr;
    float *d_t = nullptr;
    const DCamBlock *cam = nullptr;   // the frame's camera, which the kernels of every sequence of an eager frame get as an argument
                                      // (null: a captured graph, whose kernels read rt_ctx::d_cam; input rays)
    enum At {
        WHOLE,                 // the whole frame
        ADAPTIVE_1,            // the one-ray rows, resolved into C1 (d_rgb), then k_flag on the n x n frame F2
        ADAPTIVE_2,            // k_flag's tiles of the n x n frame, then k_resolve<SRC_ADAPTIVE, SINK_STORE>
        PASS                   // pass `index` of `passes` (rt_set_passes): resolved into the running sum `acc` when passes > 1
    } at = WHOLE;
    size_t ev0 = 0;            // its first event
    int set = 0;               // the working set it runs on (1: only ever an overlapped frame)
    const DFrame *F2 = nullptr;       // ADAPTIVE_1
    const int32_t *pos = nullptr;     // ADAPTIVE_1, ADAPTIVE_2: per output local row, the C1 rows of frame rows y - 1, y, y + 1 (-1 outside the frame)
    float tau = 0.0f;                 // ADAPTIVE_1
    int index = 0, passes = 1;        // PASS
    float *acc = nullptr;             // PASS, passes > 1: float[3] per output pixel
    // PASS of an adaptive-pass frame (conv != nullptr: the frame's tables): the converging resolve, and k_pass_list behind it from pass pass_min on (not the last)
    const FrameTables *conv = nullptr;
    float pass_tol = 0.0f;
    int pass_min = 0;
    bool first() const { return at == WHOLE || at == ADAPTIVE_1 || (at == PASS && index == 0); }     // the first sequence of its frame
};

static uint32_t flag_cap(const DFrame &F);

// The camera argument of a sequence's kernels (CamArg, rt_device.hpp): the block itself where the sequence has the frame's camera -- every
// eager sequence -- and the context's device block otherwise: a captured graph, whose replays upload the camera in front of it (graph_launch).
static CamArg cam_arg(const rt_ctx *c, const DCamBlock *cam) {
    CamArg a{};
    if (cam) a.val = *cam;
    else a.ptr = c->d_cam;
    return a;
}

// One launch sequence = memset(control) ; per level { trace ; shadow ; shade } ; resolve -- no host synchronisation inside and no allocation
// (the caller has reserved the working set: ensure_frame).
// The two halves are sequence_body (everything up to the resolve) and sequence_resolve (the resolve and what follows it), which SeqState
// connects: run_sequence runs both on one stream; an overlapped frame runs the body on the internal stream of its set and the resolve on the
// caller's (rt_render_device).
struct SeqState {
    DFrame F;
    CamArg cam;
    int levels_run = 1;
    bool later = false;
    size_t ev = 0;
    uint32_t nl = 0;
};

static rt_status sequence_body(rt_ctx *c, hipStream_t st, const DLights &L, const Sequence &q, SeqState *state) {
    FrameSet &w = c->fs[q.set];
    DFrame F = q.F;
    const bool primary = q.primary, count = q.count;
    const int timed = q.timed;
    int32_t *const d_hit = q.d_hit;
    float *const d_t = q.d_t;
    const int levels_run = levels_run_of(c, F);
    const int lslots = L.n_lights;
    const size_t P = (static_cast<size_t>(L.n_samples) + 63) / 64;
    F.item_cap = F.ray_cap = list_cap(frame_tiles(F));
    const bool later = !q.first();
    size_t ev = q.ev0;
    uint32_t nl = 1;             // device operations of this sequence: this memset + every kernel launch below
    if (later) {
        // (the frame's first sequence began with the frame's memset: this one clears only the per-level queue and list counters that the sequence
        //  before used, so the stat shards behind them sum over the sequences)
        if (timed) HIPCHK(c, hipEventRecord(event_at(c, ev++), st));
        HIPCHK(c, hipMemsetAsync(w.d_ctl, 0, kPassClearBytes, st));
    } else {
        HIPCHK(c, hipMemsetAsync(w.d_ctl, 0, kFrameClearBytes, st));        // everything but the sticky overflow word
    }
    launch_set_prof(st, w.d_ctl, 0u);   // no-op unless built with -DRT_WORK_COUNTERS
    if (!primary) ++nl;
    if (!primary) HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&w.d_ctl->n_rays[0][0]), static_cast<int>(q.n_input_rays), 1, st));
    const CamArg cam = cam_arg(c, q.cam);
    if (timed && !later) HIPCHK(c, hipEventRecord(event_at(c, ev++), st));
    // flat scenes: the levels from 2 on are ONE launch (k_deep); the counting pass keeps the per-level kernels (its variants count per kernel)
    const bool deep = c->flat && c->deep && !count && levels_run > 2;
    const int wide_levels = deep ? 2 : levels_run;
    const bool simple_light = L.mode != RT_LIGHT_SPHERE && L.n_samples <= 64;     // k_shade's SIMPLE lights: one visibility word per (hit, light)
    // tree scenes: the fused k_trace runs only where RT_STAGED_TRACE=0 asks for it, and only the sequences whose first rays are plain
    // (no lens, shutter or later pass: the fused tree kernel is not instantiated for those)
    const bool fused = c->flat || (!c->staged_trace && fused_tree_trace(primary, F));
    for (int level = 0; level < wide_levels; ++level) {
        float4 *rec_l = w.d_rec + static_cast<size_t>(level) * F.npix;
        float *fres_l = w.d_fres + static_cast<size_t>(level) * F.npix;
        const bool prim = primary && level == 0;
        const int tgrid = c->cus * (prim ? c->occ_trace_primary : c->occ_trace_rays);
        int32_t *hit_l = level == 0 ? d_hit : nullptr;
        float *t_l = level == 0 ? d_t : nullptr;
        if (fused) {
            ++nl, launch_trace(prim, count, c->flat, tgrid, st, c->S, cam, L, F, level, 3 * level, w.d_rays[level & 1], w.d_items, w.d_ctl, rec_l, hit_l, t_l);
        } else {
            // tree scenes: closest hit -> light-centre visibility -> finish; each traversal stage writes its big leaves as
            // chunk-range tasks that a second launch spreads over all waves
            const uint32_t B = count ? 0u : c->trace_budget, cap = c->task_cap;
            for (int stage = 0; stage < 2; ++stage) {
                const uint32_t q0 = static_cast<uint32_t>(stage);
                ++nl, launch_stage(prim, count, stage, false, tgrid * c->stage_mult, st, c->S, cam, L, F, level, lslots, w.d_rays[level & 1], w.d_items, w.d_ctl, rec_l,
                             hit_l, t_l, w.d_best, w.d_lit, TaskQueues{nullptr, B ? w.d_tasks[stage] : nullptr, 0u, q0, cap, B, c->task_target_env ? c->task_target : c->trace_target});
                if (B != 0u)
                    ++nl, launch_stage(prim, false, stage, true, tgrid, st, c->S, cam, L, F, level, lslots, w.d_rays[level & 1], w.d_items, w.d_ctl, rec_l,
                                 hit_l, t_l, w.d_best, w.d_lit, TaskQueues{w.d_tasks[stage], nullptr, q0, 0u, cap, 0u});
            }
            ++nl, launch_stage(prim, count, 2, false, tgrid, st, c->S, cam, L, F, level, lslots, w.d_rays[level & 1], w.d_items, w.d_ctl, rec_l, hit_l, t_l,
                         w.d_best, w.d_lit, TaskQueues{nullptr, nullptr, 0u, 0u, cap, 0u});
        }
        if (timed) HIPCHK(c, hipEventRecord(event_at(c, ev++), st));
        launch_set_prof(st, w.d_ctl, RT_WORK_SHADOW);
        // first the beam test of whole tiles of 64 hits (k_beam: the hits whose sample rays nothing can block get their visibility words
        // there and never become shadow units), then the survivors
        // (tree scenes: off unless RT_BEAM_TREES=1.  Measured on dodgeColorTest.obj 1080p/64: 84 % of the 3,332 tiles come out unblocked -- none
        // of their hits can reach a leaf with one of the model's degenerate triangles -- and the shadow units drop from 213k to 33k, but a beam
        // walks ~370 steps alone in its wave (k_beam 0.30 ms) and the units that remain are the expensive ones (penumbra, cluttered parts:
        // 0.60 ms of the former 0.77): 0.90 ms against 0.77.  cfg4: 9 % unblocked; the launch's own brake stops testing after 4k of 18k tiles.)
        // tree scenes with one (hit, light) pair per wave: the shaft walk (rt_kernels.hip, k_shadow_shaft), behind the per-hit beam test (k_beam_items)
        const bool shaft = !c->flat && !count && c->S.shaft != 0 && L.n_samples >= c->shaft_min_samples;
        // (one pass per pair -- 64 samples or fewer: a beam costs about 1.7 units and replaces one; dodge 1080p/64: 1.05 -> 1.50 ms.  Four passes, cfg4:
        //  nine pairs in ten are decided by their beam, k_shadow_shaft 22.6 -> 11.7 ms behind 6.5 ms of beams)
        const bool item_beam = shaft && c->S.beam != 0 && !c->beam_trees && (c->item_beam >= 2u || (c->item_beam == 1u && P > 1));
        const bool beam = !count && c->S.beam != 0 && (c->flat || c->beam_trees);
        const uint32_t *sidx = (beam || item_beam) ? w.d_sidx : nullptr;
        // flat scenes with one visibility word per (hit, light): no shadow units at all.  k_beam settles the hits its tile test cannot clear with
        // the units' triangle cull (lane = hit) and marks the rest pending per (tile, light) in d_lit (which only the staged trace of tree scenes
        // uses otherwise); k_shade walks the pending pairs' sample segments before it shades them.  k_beam stays the shadow group's launch.
        const bool fold = beam && c->flat && c->S.plane_cull != 0 && simple_light && !c->shadow_units;
        unsigned long long *pend = fold ? w.d_lit : nullptr;
        if (beam) ++nl, launch_beam(c->cus * c->occ_beam, st, c->S, L, level, lslots, F.item_cap, w.d_items, w.d_ctl, w.d_vis, w.d_sidx, pend, w.d_ltab);
        const uint8_t *pair_done = (item_beam && lslots > 1) ? w.d_done : nullptr;
        if (item_beam) ++nl, launch_pair_beam(c->cus * c->item_beam_blocks, st, c->S, L, level, lslots, F.item_cap, w.d_items, w.d_ctl, w.d_vis, w.d_sidx, lslots > 1 ? w.d_done : nullptr);
        const uint32_t shaft_b = level == 0 ? c->shaft_budget : c->shaft_budget_deep;
        if (fold) {
            // (no shadow units: k_shade<.., FOLD> finishes the pending pairs)
        } else if (shaft)
            ++nl, launch_shadow_shaft(c->cus * c->occ_shaft, st, c->S, L, level, 3 * level + 1, lslots, F.item_cap, w.d_items, w.d_ctl, w.d_vis,
                                w.d_tasks[0], c->task_cap, shaft_b, c->task_target, sidx, pair_done);
        else
            ++nl, launch_shadow(count, c->flat, c->cus * c->occ_shadow, st, c->S, L, level, 3 * level + 1, lslots, F.item_cap, w.d_items, w.d_ctl, w.d_vis,
                          w.d_tasks[0], c->task_cap, c->shadow_budget, c->task_target, sidx);
        if (shaft && shaft_b != 0u)
            ++nl, launch_shadow_shaft_cont(c->cus * c->occ_shaft, st, c->S, L, level, lslots, F.item_cap, w.d_items, w.d_ctl, w.d_vis, w.d_tasks[0], c->task_cap, sidx);
        else if (!shaft && !c->flat && !count && c->shadow_budget != 0u)      // the big leaves of the shadow units, spread over all waves
            ++nl, launch_shadow_cont(c->cus * c->occ_shadow, st, c->S, L, level, lslots, F.item_cap, w.d_items, w.d_ctl, w.d_vis, w.d_tasks[0], nullptr, 2u, 0u,
                               c->task_cap, 0u, sidx);
        if (timed) HIPCHK(c, hipEventRecord(event_at(c, ev++), st));   // after the whole shadow group (incl. continuations)
        launch_set_prof(st, w.d_ctl, 0u);
        ++nl, launch_shade(c->cus * c->occ_shade, st, c->S, L, F, level, 3 * level + 2, lslots, w.d_items, w.d_ctl, w.d_vis, rec_l, fres_l, w.d_rays[(level + 1) & 1],
                           c->flat && c->deep && !count && level + 1 < levels_run, pend, w.d_ltab);
        if (timed) HIPCHK(c, hipEventRecord(event_at(c, ev++), st));        // after k_shade (lean timing too: the shade interval is a single kernel)
    }
    if (deep) {
        ++nl, launch_deep(c->cus * c->occ_shade, st, c->S, L, F, 2, w.d_rays[0], w.d_ctl, w.d_rec + 2 * static_cast<size_t>(F.npix), w.d_fres + 2 * static_cast<size_t>(F.npix));
        // (the event layout stays three per level: the deep launch is booked as the trace interval of level 2, the other intervals are empty)
        if (timed) for (int k = 0; k < 3 * (levels_run - 2); ++k) HIPCHK(c, hipEventRecord(event_at(c, ev++), st));
    }
    c->frame_wide_levels = wide_levels;
    state->F = F; state->cam = cam; state->levels_run = levels_run; state->later = later; state->ev = ev; state->nl = nl;
    return RT_OK;
}

static rt_status sequence_resolve(rt_ctx *c, hipStream_t st, const Sequence &q, const SeqState &state) {
    FrameSet &w = c->fs[q.set];
    const DFrame &F = state.F;
    const CamArg &cam = state.cam;
    const int timed = q.timed, levels_run = state.levels_run;
    float *const d_rgb = q.d_rgb;
    size_t ev = state.ev;
    uint32_t nl = state.nl;
    DFrame Fr = F;
    Fr.max_depth = levels_run - 1;
    ResolveArgs ra{w.d_rec, w.d_fres, d_rgb, q.d_u8};
    ra.cam = cam;                       // (its rect: read only by a frame with F.cull set)
    if (q.at == Sequence::ADAPTIVE_2) { ra.refine = c->d_refine; ra.c1 = c->d_c1; ra.pos = q.pos; }
    if (q.at == Sequence::PASS && q.passes > 1) { ra.acc = q.acc; ra.index = q.index; ra.count = q.passes; }      // this pass into the running sum / the mean
    const bool conv = q.at == Sequence::PASS && q.conv != nullptr;
    if (conv) {
        ra.s2 = q.conv->s2; ra.taken = q.conv->taken; ra.active = q.conv->active; ra.n_flag = w.d_ctl->n_flag;
        ra.min_passes = q.pass_min; ra.tol = q.pass_tol;
    }
    ++nl, launch_resolve(c->cus * 8, st, Fr, ra);
    if (conv && q.index + 1 >= q.pass_min && q.index + 1 < q.passes) {      // the tiles of the next pass
        DFrame Fl = F;
        Fl.tiles = c->d_flag; Fl.tile_cap = flag_cap(F);
        ++nl, launch_pass_list(c->cus * 8, st, Fl, q.conv->active, c->d_flag, w.d_ctl);
    }
    if (q.at == Sequence::ADAPTIVE_1) ++nl, launch_flag(c->cus * 8, st, *q.F2, d_rgb, q.pos, q.tau, c->d_refine, c->d_flag, w.d_ctl);
    if (timed) HIPCHK(c, hipEventRecord(event_at(c, ev++), st));
    c->frame_launches = state.later ? c->frame_launches + nl : nl;
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

static rt_status run_sequence(rt_ctx *c, hipStream_t st, const DLights &L, const Sequence &q) {
    SeqState state;
    const rt_status s = sequence_body(c, st, L, q, &state);
    return s != RT_OK ? s : sequence_resolve(c, st, q, state);
}

static rt_status sum_frame_times(rt_ctx *c, size_t ev, int levels_run, rt_stats *out, bool lean) {
    float ms = 0.f;
    const size_t first = ev;
    for (int level = 0; level < levels_run; ++level) {
        // events: [.. trace ..] E [beam, shadow] E [shade] E [.. next trace ..]
        HIPCHK(c, hipEventElapsedTime(&ms, c->events[ev], c->events[ev + 1])); out->ms_trace += ms; ++ev;
        HIPCHK(c, hipEventElapsedTime(&ms, c->events[ev], c->events[ev + 1])); out->ms_shadow += ms; ++ev;
        HIPCHK(c, hipEventElapsedTime(&ms, c->events[ev], c->events[ev + 1])); out->ms_shade += ms; ++ev;
    }
    if (!lean) { HIPCHK(c, hipEventElapsedTime(&ms, c->events[ev], c->events[ev + 1])); out->ms_resolve += ms; }
    HIPCHK(c, hipEventElapsedTime(&ms, c->events[first], c->events[ev + 1])); out->ms_total += ms;
    const uint32_t wide = static_cast<uint32_t>(c->frame_wide_levels > 0 && c->frame_wide_levels < levels_run ? c->frame_wide_levels : levels_run);
    out->launches_trace += wide;
    out->launches_shadow += wide;
    out->launches_shade += wide;
    out->launches_total = c->frame_launches;
    return RT_OK;
}

// after a synchronise: did a kernel of the last frame fail to reserve list space?  (never expected; see list_cap)
static rt_status check_overflow(rt_ctx *c) {
    bool any = false;
    for (FrameSet &w : c->fs) {          // (the sticky word of both control blocks: an overlapped frame may have run on either set)
        if (!w.d_ctl.p) continue;
        uint32_t ov = 0;
        HIPCHK(c, hipMemcpy(&ov, &w.d_ctl->overflow, sizeof ov, hipMemcpyDeviceToHost));
        if (ov) HIPCHK(c, hipMemset(&w.d_ctl->overflow, 0, sizeof ov));
        any = any || ov != 0;
    }
    if (any) {
        c->err = "internal: a compaction list overflowed its capacity; a frame since the last synchronising call is incomplete";
        return RT_ERR_HIP;
    }
    return RT_OK;
}

// after the frames on `st`: the control block, folded into `h`, and its counters in `out`
static rt_status read_counters(rt_ctx *c, hipStream_t st, const FrameShape &shape, Control &h, rt_stats *out) {
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipMemcpy(&h, c->d_ctl, sizeof h, hipMemcpyDeviceToHost));
    { const rt_status os_ = check_overflow(c); if (os_ != RT_OK) return os_; }
    fold_stats(h);
    out->rays_primary = h.rays_primary; out->rays_bounce = h.rays_bounce; out->rays_centre = h.rays_centre; out->rays_sample = h.rays_sample; out->rays_sample_walked = h.sample_walked;
    out->pixels = shape.pixels(h.refined);
    out->pixels_culled = h.pixels_culled; out->shaded_hits = h.shaded_hits;
    return RT_OK;
}

// a sharded list counter (Control::n_items and its like: counter s at [s * 16]) summed over its shards
static uint32_t shard_sum(const uint32_t *counters) {
    uint32_t t = 0;
    for (int sh = 0; sh < RT_LIST_SHARDS; ++sh) t += counters[sh * 16];
    return t;
}

static rt_status fill_stats(rt_ctx *c, hipStream_t st, const FrameShape &shape, bool timed, rt_stats *out, bool counted) {
    Control h;
    { const rt_status rs = read_counters(c, st, shape, h, out); if (rs != RT_OK) return rs; }
    out->launches_total = c->frame_launches;
    if (std::getenv("RT_DEBUG"))
        std::fprintf(stderr, "RT_DEBUG level0: items %u tasks closest %u %u centre %u %u shadow %u %u\n", shard_sum(h.n_items[0]), shard_sum(h.n_task_tr[0][0]), 0u,
                     shard_sum(h.n_task_tr[0][1]), 0u, shard_sum(h.n_task_sh[0]), 0u);
    if (counted) {
        out->box_tests = h.box_tests + h.box_tests_shadow; out->leaf_tri_refs = h.leaf_tri_refs + h.leaf_tri_refs_shadow;
        out->box_tests_shadow = h.box_tests_shadow; out->leaf_tri_refs_shadow = h.leaf_tri_refs_shadow;
    }
    if (timed) {
        out->ms_trace = out->ms_shadow = out->ms_shade = out->ms_resolve = out->ms_total = 0.f;
        out->launches_trace = out->launches_shadow = out->launches_shade = 0;
        for (uint32_t k = 0; k < shape.sequences; ++k) {
            const rt_status s = sum_frame_times(c, c->ev_base + k * frame_events(shape.levels_run), shape.levels_run, out, false);
            if (s != RT_OK) return s;
        }
    }
    return RT_OK;
}

static rt_status make_frame(rt_ctx *c, const rt_params *p, DFrame *F) {
    if (!p || p->width <= 0 || p->height <= 0) { c->err = "params: width/height must be positive"; return RT_ERR_INVALID; }
    if (p->stripe <= 0 || p->nranks <= 0 || p->rank < 0 || p->rank >= p->nranks || p->row0 < 0 || p->row1 > p->height || p->row0 > p->row1) {
        c->err = "params: bad row shard (row0,row1,stripe,rank,nranks)";
        return RT_ERR_INVALID;
    }
    if (p->max_depth > RT_MAX_DEPTH) { c->err = "params: max_depth above RT_MAX_DEPTH"; return RT_ERR_UNSUPPORTED; }
    // supersampling: the traced frame is the frame of sub-samples -- width n*W, local rows n*rows, row0 n*row0, stripe n*stripe, same
    // rank and nranks.  Its local row n*lr + sy is then frame row n*y + sy of output local row lr (frame row y): sub-row sy of that row.
    const int32_t n = c->smp.ss;
    const int32_t rows = rt_local_rows(p);
    const int64_t n64 = n;
    if (n64 * p->width > INT32_MAX || n64 * p->height > INT32_MAX || n64 * p->stripe > INT32_MAX ||
        n64 * n64 * rows * p->width > static_cast<int64_t>(UINT32_MAX / 3u)) {
        c->err = "params: the frame of sub-samples is too large";
        return RT_ERR_UNSUPPORTED;
    }
    F->width = n * p->width; F->height = n * p->height;
    F->local_rows = n * rows;
    F->row0 = n * p->row0; F->stripe = n * p->stripe; F->rank = p->rank; F->nranks = p->nranks;
    F->tiles_x = (F->width + 7) / 8; F->tiles_y = (F->local_rows + 7) / 8;
    F->npix = static_cast<uint32_t>(F->local_rows) * static_cast<uint32_t>(F->width);
    F->max_depth = p->max_depth < 0 ? RT_MAX_DEPTH : p->max_depth;
    F->dyn_trace = c->dyn_trace;
    F->item_cap = F->ray_cap = 0;
    F->ss = n;
    F->ss_mul = n > 1 ? static_cast<uint32_t>((0x100000000ull + static_cast<uint64_t>(n) - 1u) / static_cast<uint64_t>(n)) : 0u;
    for (int s = 0; s < RT_MAX_SUPERSAMPLING; ++s) F->sso[s] = F->sso[RT_MAX_SUPERSAMPLING + s] = s < n ? static_cast<float>((2 * s + 1 - n) / (2.0 * n)) : 0.0f;
    F->pass_key = 0u;                                             // pass 0 (apply_pass sets the offsets and the key of any other)
    F->out_width = p->width; F->out_rows = rows;
    F->rows = nullptr; F->tiles = nullptr; F->tile_cap = 0u;      // (set by enqueue_frame for the two passes of an adaptive frame only)
    F->lens = nullptr; F->lens_aperture = 0.0f; F->lens_focus = 0.0f; F->lens_mul = 0u;     // (set by apply_lens when the lens is on)
    F->shutter = 0;                                                                          // (set by apply_shutter when the shutter is on)
    F->cull = 0;                                                                             // (set by plan_frame for a frame that may cull)
    return RT_OK;
}

// ---- thin lens (Depth of field) ----------------------------------------------------------------------------------------
static void concentric_disc(double u, double v, double *x, double *y) {          // Shirley-Chiu, [-1, 1]^2 -> unit disc
    if (u == 0.0 && v == 0.0) { *x = 0.0; *y = 0.0; return; }
    double r, t;
    if (std::fabs(u) > std::fabs(v)) { r = u; t = (M_PI / 4.0) * (v / u); }
    else { r = v; t = (M_PI / 2.0) - (M_PI / 4.0) * (u / v); }
    *x = r * std::cos(t); *y = r * std::sin(t);
}

extern "C" rt_status rt_lens_table(int32_t n, float *out) {
    if (n < 1 || n > RT_MAX_SUPERSAMPLING || !out) return RT_ERR_INVALID;
    const int nn = n * n;
    for (int k = 0; k < nn; ++k) {
        double x, y;
        concentric_disc(2.0 * ((k % n + 0.5) / n) - 1.0, 2.0 * ((k / n + 0.5) / n) - 1.0, &x, &y);
        for (int r = 0; r < RT_LENS_ROTATIONS; ++r) {
            const double a = (M_PI / 2.0) * r / RT_LENS_ROTATIONS;
            out[(static_cast<size_t>(r) * nn + k) * 2] = static_cast<float>(x * std::cos(a) - y * std::sin(a));
            out[(static_cast<size_t>(r) * nn + k) * 2 + 1] = static_cast<float>(x * std::sin(a) + y * std::cos(a));
        }
    }
    return RT_OK;
}

extern "C" rt_status rt_set_lens(rt_ctx *c, float aperture, float focus) {
    if (!c) return RT_ERR_INVALID;
    if (!std::isfinite(aperture) || aperture < 0.0f) { c->err = "rt_set_lens: the aperture must be finite and >= 0"; return RT_ERR_INVALID; }
    if (aperture > 0.0f && !(std::isfinite(focus) && focus > 0.0f)) { c->err = "rt_set_lens: the focus must be finite and > 0"; return RT_ERR_INVALID; }
    c->smp.lens_aperture = aperture; c->smp.lens_focus = focus;
    return RT_OK;
}

// first entry of the table of n in d_lens (the tables of 1 .. n - 1 come before it)
static size_t lens_offset(int n) { size_t o = 0; for (int m = 1; m < n; ++m) o += static_cast<size_t>(RT_LENS_ROTATIONS) * m * m; return o; }

// lens on: F gets the table of its n (uploaded once per context, before any frame or capture that reads it), the aperture and the focus
static rt_status apply_lens(rt_ctx *c, DFrame *F) {
    if (!c->smp.lens_on()) return RT_OK;
    if (!c->d_lens) {
        std::vector<float> h(lens_offset(RT_MAX_SUPERSAMPLING + 1) * 2);
        for (int n = 1; n <= RT_MAX_SUPERSAMPLING; ++n) (void)rt_lens_table(n, h.data() + lens_offset(n) * 2);
        HIPCHK(c, c->d_lens.grow(h.size() / 2));
        const hipError_t e = hipMemcpy(c->d_lens, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) { c->d_lens.release(); c->err = std::string("rt_set_lens table upload: ") + hipGetErrorString(e); return RT_ERR_HIP; }
    }
    const uint32_t nn = static_cast<uint32_t>(F->ss * F->ss);
    F->lens = c->d_lens + lens_offset(F->ss);
    F->lens_aperture = c->smp.lens_aperture; F->lens_focus = c->smp.lens_focus;
    F->lens_mul = nn > 1u ? static_cast<uint32_t>((0x100000000ull + nn - 1u) / nn) : 0u;
    return RT_OK;
}

// ---- camera motion blur (Motion blur) ---------------------------------------------------------------------------------
// The two host functions are the definition the kernels restate (shutter_time, shutter_camera in rt_kernels.hip): float32, one rounding per
// operation (this file is built with -ffp-contract=off; x86-64 evaluates float expressions in float).
static uint32_t shutter_mix(uint32_t v) { v ^= v >> 15; v *= 0x2C1B3C6Du; v ^= v >> 12; v *= 0x297A2D39u; v ^= v >> 15; return v; }

extern "C" rt_status rt_shutter_time(int32_t n, uint32_t i, uint32_t j, int32_t sx, int32_t sy, float *t) {
    if (n < 1 || n > RT_MAX_SUPERSAMPLING || sx < 0 || sx >= n || sy < 0 || sy >= n || !t) return RT_ERR_INVALID;
    const uint32_t nn = static_cast<uint32_t>(n * n);
    const uint32_t h = shutter_mix((i * 0x9E3779B1u) ^ (j * 0x85EBCA6Bu));        // the per-pixel scramble of rt_set_lens
    const uint32_t g = shutter_mix(h ^ 0x68E31DA4u);
    const uint32_t slot = (static_cast<uint32_t>(sx * n + sy) + (g & 0xFFFFu)) % nn;
    const float u = static_cast<float>(g >> 16) * 1.52587890625e-05f;             // 2^-16
    const float sum = static_cast<float>(slot) + u;
    *t = sum / static_cast<float>(nn);
    return RT_OK;
}

extern "C" rt_status rt_shutter_camera(const rt_camera *open, const rt_camera *close, float t, rt_camera *out) {
    if (!open || !close || !out) return RT_ERR_INVALID;
    rt_camera k = *open;
    for (int q = 0; q < 3; ++q) {
        const float d = close->center[q] - open->center[q];
        if (d != 0.0f) { const float td = t * d; k.center[q] = open->center[q] + td; }
    }
    for (int q = 0; q < 12; ++q) {
        const float d = close->inv_view[q] - open->inv_view[q];
        if (d != 0.0f) { const float td = t * d; k.inv_view[q] = open->inv_view[q] + td; }
    }
    *out = k;
    return RT_OK;
}

static bool shutter_pose_finite(const rt_camera *cam) {
    for (int q = 0; q < 3; ++q) if (!std::isfinite(cam->center[q])) return false;
    for (int q = 0; q < 12; ++q) if (!std::isfinite(cam->inv_view[q])) return false;
    return true;
}

extern "C" rt_status rt_set_shutter(rt_ctx *c, const rt_camera *close) {
    if (!c) return RT_ERR_INVALID;
    if (!close) { c->smp.shutter_on = false; return RT_OK; }
    if (!shutter_pose_finite(close)) { c->err = "rt_set_shutter: the close camera's center / inv_view must be finite"; return RT_ERR_INVALID; }
    c->smp.shutter_close = *close;
    c->smp.shutter_on = true;
    return RT_OK;
}

// only the pose moves during the exposure: the perspective scale and the raster terms stay wave-uniform
static bool shutter_compatible(const rt_camera *open, const rt_camera *close) {
    return std::memcmp(&open->fovy, &close->fovy, sizeof open->fovy) == 0 && std::memcmp(&open->aspect, &close->aspect, sizeof open->aspect) == 0 &&
           std::memcmp(open->viewport, close->viewport, sizeof open->viewport) == 0;
}

// shutter on: the frame runs the SHUTTER instantiations (which take v % (n*n) from lens_mul whether the lens is on or not)
static void apply_shutter(const rt_ctx *c, DFrame *F) {
    if (!c->smp.shutter_on) return;
    const uint32_t nn = static_cast<uint32_t>(F->ss * F->ss);
    F->shutter = 1;
    F->lens_mul = nn > 1u ? static_cast<uint32_t>((0x100000000ull + nn - 1u) / nn) : 0u;
}

// the deltas d = close - open of the 15 pose values, computed once here; K(t) = open + t * d per lane on the device
static void make_shutter(const rt_camera *open, const rt_camera *close, DShutter *sh) {
    for (int q = 0; q < 3; ++q) sh->d[q] = close->center[q] - open->center[q];
    for (int q = 0; q < 12; ++q) sh->d[3 + q] = close->inv_view[q] - open->inv_view[q];
    sh->d[15] = 0.0f;
}

// ---- multi-pass accumulation (Multi-pass accumulation) ----------------------------------------------------------------
// phi_b(p) in host double, in exactly the order the header gives, wrapped to the cell: e in [-0.5, 0.5), e(0) = 0
static double pass_shift(uint32_t p, uint32_t b) {
    double f = 1.0, r = 0.0;
    while (p > 0) { f = f / b; r = r + f * (p % b); p = p / b; }
    return r < 0.5 ? r : r - 1.0;
}

extern "C" rt_status rt_pass_offsets(int32_t n, int32_t p, float *ox, float *oy) {
    if (n < 1 || n > RT_MAX_SUPERSAMPLING || p < 0 || p >= RT_MAX_PASSES || !ox || !oy) return RT_ERR_INVALID;
    const double e2 = pass_shift(static_cast<uint32_t>(p), 2u), e3 = pass_shift(static_cast<uint32_t>(p), 3u);
    for (int s = 0; s < n; ++s) {
        ox[s] = static_cast<float>((2 * s + 1 - n) / (2.0 * n) + e2 / n);
        oy[s] = static_cast<float>((2 * s + 1 - n) / (2.0 * n) + e3 / n);
    }
    return RT_OK;
}

extern "C" rt_status rt_set_passes(rt_ctx *c, int32_t first, int32_t count) {
    if (!c) return RT_ERR_INVALID;
    if (first < 0 || count < 1 || static_cast<int64_t>(first) + count > RT_MAX_PASSES) {
        c->err = "rt_set_passes: first >= 0, count >= 1 and first + count <= RT_MAX_PASSES";
        return RT_ERR_INVALID;
    }
    c->smp.pass_first = first; c->smp.pass_count = count;
    return RT_OK;
}

extern "C" rt_status rt_set_pass_tolerance(rt_ctx *c, float tol, int32_t min_passes) {
    if (!c) return RT_ERR_INVALID;
    if (std::isnan(tol) || min_passes < 2 || min_passes > RT_MAX_PASSES) {
        c->err = "rt_set_pass_tolerance: tol must not be NaN and min_passes must be in 2..RT_MAX_PASSES";
        return RT_ERR_INVALID;
    }
    c->smp.pass_tol = tol; c->smp.pass_min = min_passes;
    return RT_OK;
}

// F becomes the frame of pass p: its raster offsets and the key of its scrambles (p = 0 leaves make_frame's values, bit for bit)
static void apply_pass(DFrame *F, int p) {
    float ox[RT_MAX_SUPERSAMPLING], oy[RT_MAX_SUPERSAMPLING];
    (void)rt_pass_offsets(F->ss, p, ox, oy);
    for (int s = 0; s < F->ss; ++s) { F->sso[s] = ox[s]; F->sso[RT_MAX_SUPERSAMPLING + s] = oy[s]; }
    F->pass_key = static_cast<uint32_t>(p) * 0xC2B2AE35u;
}

// ---- light jitter offsets (Light jitter: the definition; no frame uses them yet) -------------------------------------------
extern "C" rt_status rt_light_jitter_offsets(int32_t p, float *fu, float *fv) {
    if (p < 0 || p >= RT_MAX_PASSES || !fu || !fv) return RT_ERR_INVALID;
    *fu = static_cast<float>(0.5 + pass_shift(static_cast<uint32_t>(p), 5u));
    *fv = static_cast<float>(0.5 + pass_shift(static_cast<uint32_t>(p), 7u));
    return RT_OK;
}

extern "C" rt_status rt_set_supersampling(rt_ctx *c, int32_t n) {
    if (!c) return RT_ERR_INVALID;
    if (n < 1 || n > RT_MAX_SUPERSAMPLING) { c->err = "rt_set_supersampling: n must be in 1..RT_MAX_SUPERSAMPLING"; return RT_ERR_INVALID; }
    c->smp.ss = n;
    return RT_OK;
}

extern "C" rt_status rt_set_supersampling_threshold(rt_ctx *c, float threshold) {
    if (!c) return RT_ERR_INVALID;
    if (std::isnan(threshold)) { c->err = "rt_set_supersampling_threshold: the threshold is NaN"; return RT_ERR_INVALID; }
    c->smp.ss_tau = threshold;
    return RT_OK;
}

// ---- adaptive supersampling (Adaptive supersampling) ------------------------------------------------------------------
// per-shard capacity of k_flag's list: shard s receives the tiles t % RT_LIST_SHARDS == s of the n x n frame
static uint32_t flag_cap(const DFrame &F) {
    return (static_cast<uint32_t>(F.tiles_x) * static_cast<uint32_t>(F.tiles_y) + RT_LIST_SHARDS - 1u) / RT_LIST_SHARDS;
}

struct AdaptivePlan {
    DFrame F1;                      // pass 1: the one-ray frame of the call's rows and their neighbours y -+ 1 inside [0, H), in increasing order
    std::vector<int32_t> rows;      // ... its frame rows when they are not one contiguous range (else empty: F1's row0 / stripe 1 say it)
    std::vector<int32_t> pos;       // per output local row: the C1 rows of frame rows y - 1, y, y + 1 (-1 outside the frame)
    float tau;
};

static void plan_adaptive(const rt_ctx *c, const rt_params *p, const DFrame &F, AdaptivePlan *A) {
    const int32_t H = p->height;
    std::vector<int32_t> set;
    A->pos.clear();
    // the output rows come in increasing order, so each row's candidates y - 1, y, y + 1 either extend the set or are in it already
    auto index_of = [&](int32_t v) -> int32_t {
        for (size_t k = set.size(); k-- > 0 && set[k] >= v;)
            if (set[k] == v) return static_cast<int32_t>(k);
        return -1;
    };
    for (int32_t y = p->row0; y < p->row1; ++y) {
        if (((y - p->row0) / p->stripe) % p->nranks != p->rank) continue;
        for (int32_t v = y - 1; v <= y + 1; ++v)
            if (v >= 0 && v < H && (set.empty() || v > set.back())) set.push_back(v);
        A->pos.push_back(y > 0 ? index_of(y - 1) : -1);
        A->pos.push_back(index_of(y));
        A->pos.push_back(y + 1 < H ? index_of(y + 1) : -1);
    }
    const int32_t n1 = static_cast<int32_t>(set.size());
    DFrame &F1 = A->F1;
    F1 = F;
    F1.width = p->width; F1.height = H;
    F1.local_rows = n1;
    F1.row0 = set.front(); F1.stripe = 1; F1.rank = 0; F1.nranks = 1;
    F1.tiles_x = (F1.width + 7) / 8; F1.tiles_y = (n1 + 7) / 8;
    F1.npix = static_cast<uint32_t>(n1) * static_cast<uint32_t>(F1.width);
    F1.ss = 1; F1.ss_mul = 0u;
    for (int s = 0; s < 2 * RT_MAX_SUPERSAMPLING; ++s) F1.sso[s] = 0.0f;
    F1.out_width = F1.width; F1.out_rows = n1;
    F1.rows = nullptr; F1.tiles = nullptr; F1.tile_cap = 0u;
    A->rows.clear();
    if (set.back() - set.front() + 1 != n1) A->rows = set;        // (a row table: several ranks, stripes apart)
    A->tau = c->smp.ss_tau;
}

// the row tables of an adaptive frame, in the context's buffers or in a graph's own
static hipError_t upload_tables(FrameTables &t, const AdaptivePlan &A) {
    hipError_t e = t.rows.grow(A.rows.size());
    if (e == hipSuccess) e = t.pos.grow(A.pos.size());
    if (e == hipSuccess && !A.rows.empty()) e = hipMemcpy(t.rows, A.rows.data(), A.rows.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t.pos, A.pos.data(), A.pos.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    return e;
}

// the row tables of an eager adaptive frame: rewritten only when the call's rows change, after the frames that may still read them
static rt_status eager_tables(rt_ctx *c, const AdaptivePlan &A) {
    if (A.rows != c->h_rowtab || A.pos != c->h_pos) {
        const rt_status ws = wait_frames(c, LostStream::Tolerate);
        if (ws != RT_OK) return ws;
        c->h_rowtab.clear(); c->h_pos.clear();
        HIPCHK(c, upload_tables(c->tab, A));
        c->h_rowtab = A.rows; c->h_pos = A.pos;
    }
    return RT_OK;
}

// ---- the frame plan --------------------------------------------------------------------------------------------------------------------
// What one frame is, decided ONCE from the context's sample settings: its lights, its frame of sub-samples (lens and shutter applied), which
// launch sequences make it up, the working set they need and what the statistics will ask about it.  rt_render_device and rt_graph_create
// plan, reserve and enqueue; a sampling feature that adds a kind of frame adds it here (Where a sampling feature plugs in).
struct FramePlan {
    enum Kind {
        PLAIN,                 // one launch sequence
        ADAPTIVE,              // two: the one-ray frame A.F1 into C1 and k_flag, then F on k_flag's tiles (Adaptive supersampling)
        PASSES                 // pass_count: one per pass, each with its own raster offsets and scramble key (Multi-pass accumulation)
    } kind = PLAIN;
    DLights L;
    DFrame F;                  // (npix == 0: an empty shard -- nothing below is planned)
    AdaptivePlan A;            // ADAPTIVE
    int pass_first = 0, pass_count = 1;      // PASSES (count == 1 is the plain frame of pass `first`: no accumulator, the usual resolve)
    bool converge = false;                   // PASSES: an adaptive-pass frame (Adaptive pass counts) with ...
    float pass_tol = -1.0f;                  // ... this tolerance and ...
    int pass_min = 0;                        // ... this many whole-frame passes in front of the list passes
    WorkingSet ws;
    FrameShape shape;
};

// own_offsets: see check_lights
static rt_status plan_frame(rt_ctx *c, const rt_lights *lights, const rt_params *p, DevBuf<float> *own_offsets, FramePlan *plan) {
    rt_status s = check_lights(c, lights, &plan->L, own_offsets);
    if (s != RT_OK) return s;
    DFrame &F = plan->F;
    if ((s = make_frame(c, p, &F)) != RT_OK) return s;
    if (F.npix == 0) return RT_OK;
    if ((s = apply_lens(c, &F)) != RT_OK) return s;
    apply_shutter(c, &F);
    const SampleSettings &m = c->smp;
    const size_t out_pix = static_cast<size_t>(F.out_width) * static_cast<size_t>(F.out_rows);
    plan->ws = working_set(plan->L, F);
    plan->shape.levels_run = levels_run_of(c, F);
    plan->shape.pix_fixed = F.npix;
    if (m.adaptive_on()) {
        AdaptivePlan &A = plan->A;
        plan->kind = FramePlan::ADAPTIVE;
        plan_adaptive(c, p, F, &A);
        plan->ws.npix = std::max(F.npix, A.F1.npix);
        plan->ws.tiles = std::max(frame_tiles(F), frame_tiles(A.F1));
        plan->ws.ad = AdaptiveSizes{A.F1.npix, out_pix, static_cast<size_t>(flag_cap(F)) * RT_LIST_SHARDS};
        plan->shape.sequences = 2;
        plan->shape.pix_fixed = A.F1.npix;
        plan->shape.pix_per_refined = static_cast<uint64_t>(F.ss) * static_cast<uint64_t>(F.ss);
    } else if (m.passes_on()) {
        plan->kind = FramePlan::PASSES;
        plan->pass_first = m.pass_first; plan->pass_count = m.pass_count;
        // the running sum is part of the frame's working set: an oversized request is refused before anything is freed
        if (m.pass_count > 1) plan->ws.acc_pix = out_pix;
        plan->shape.sequences = static_cast<uint32_t>(m.pass_count);
        plan->shape.pix_fixed = static_cast<uint64_t>(F.npix) * static_cast<uint64_t>(m.pass_count);
        if (m.converge_on()) {
            // passes 1 .. pass_min trace the whole frame; every later one the tiles of the pixels still active, which k_pass_list counts
            plan->converge = true;
            plan->pass_tol = m.pass_tol; plan->pass_min = m.pass_min;
            plan->ws.conv_pix = out_pix;
            plan->ws.ad.flag_entries = static_cast<size_t>(flag_cap(F)) * RT_LIST_SHARDS;
            plan->shape.pix_fixed = static_cast<uint64_t>(F.npix) * static_cast<uint64_t>(m.pass_min);
            plan->shape.pix_per_refined = static_cast<uint64_t>(F.ss) * static_cast<uint64_t>(F.ss);
        }
    }
    // primary culling: the plain pinhole one-ray frame only (the camera that comes with the frame, or with a replay, brings the rectangle)
    F.cull = (c->primary_cull && plan->kind == FramePlan::PLAIN && m.cull_ok()) ? 1 : 0;
    return RT_OK;
}

// Reserves what the plan's launch sequences read and write: the working set in the context's buffers and the tables -- the context's (own ==
// nullptr, an eager frame) or the caller's own (a graph, which then also holds its own accumulator).  Every allocation and every synchronise
// of a frame happens here or in plan_frame, none in enqueue_frame (which a capture may enclose).
static rt_status reserve_frame(rt_ctx *c, const FramePlan &plan, FrameTables *own) {
    const rt_status s = ensure_frame(c, plan.ws, own != nullptr);
    if (s != RT_OK) return s;
    if (!own) return plan.kind == FramePlan::ADAPTIVE ? eager_tables(c, plan.A) : RT_OK;
    if (own->acc.grow(plan.ws.acc_pix * 3) != hipSuccess) { (void)hipGetLastError(); c->err = "rt_graph_create: the accumulator of the passes"; return RT_ERR_HIP; }
    if (own->grow_conv(plan.ws.conv_pix) != hipSuccess) { (void)hipGetLastError(); c->err = "rt_graph_create: the pass statistics"; return RT_ERR_HIP; }
    // (the graph's own row tables: later eager frames rewrite the context's)
    if (plan.kind == FramePlan::ADAPTIVE && upload_tables(*own, plan.A) != hipSuccess) { c->err = "rt_graph_create: row tables"; return RT_ERR_HIP; }
    return RT_OK;
}

// where a planned frame runs
struct FrameRun {
    hipStream_t st;
    const DCamBlock *cam;      // the frame's camera, an argument of its kernels; null inside a capture (a graph replay uploads it outside the graph)
    const FrameTables *tab;    // the tables reserve_frame filled
    float *d_rgb;
    uint8_t *d_u8;
    int32_t *d_hit;
    bool count;                // the counting pass
    int timed;
};

// Enqueues the plan's launch sequences on the one stream: no host round trip, no allocation, no synchronise and no launch beyond those of the
// sequences (capturable; a passes graph is a linear chain of nodes, no parallel branches).
//   ADAPTIVE: memset(control) ; pass 1 = the one-ray frame A.F1, resolved into C1 ; k_flag ; clear of pass 1's queue and list counters ;
//             pass 2 = the regular n x n frame F on k_flag's tiles ; k_resolve<SRC_ADAPTIVE, SINK_STORE>
//   PASSES:   every pass with its own DFrame; the resolve of each folds it into the running sum and the last one stores the mean
//             converge: passes 1 .. pass_min as above with the converging resolve; from pass_min on k_pass_list behind the resolve, and every
//             later pass runs on its tiles (Adaptive pass counts)
static rt_status enqueue_frame(rt_ctx *c, const FramePlan &plan, const FrameRun &r) {
    const size_t ev_step = frame_events(plan.shape.levels_run);
    Sequence q;
    q.F = plan.F;
    q.count = r.count; q.timed = r.timed;
    q.d_rgb = r.d_rgb; q.d_u8 = r.d_u8; q.d_hit = r.d_hit;
    q.cam = r.cam;
    q.ev0 = c->ev_base;
    if (plan.kind == FramePlan::PLAIN) return run_sequence(c, r.st, plan.L, q);
    if (plan.kind == FramePlan::ADAPTIVE) {
        const AdaptivePlan &A = plan.A;
        DFrame F2 = plan.F;
        F2.tiles = c->d_flag; F2.tile_cap = flag_cap(plan.F);
        q.F = A.F1;
        q.F.rows = A.rows.empty() ? nullptr : r.tab->rows.p;
        q.at = Sequence::ADAPTIVE_1; q.F2 = &F2; q.pos = r.tab->pos; q.tau = A.tau;
        q.d_rgb = c->d_c1; q.d_u8 = nullptr; q.d_hit = nullptr;
        const rt_status s = run_sequence(c, r.st, plan.L, q);
        if (s != RT_OK) return s;
        q.F = F2;
        q.at = Sequence::ADAPTIVE_2; q.ev0 += ev_step;
        q.d_rgb = r.d_rgb; q.d_u8 = r.d_u8;
        return run_sequence(c, r.st, plan.L, q);
    }
    q.at = Sequence::PASS; q.passes = plan.pass_count; q.acc = r.tab->acc;
    if (plan.converge) { q.conv = r.tab; q.pass_tol = plan.pass_tol; q.pass_min = plan.pass_min; }
    for (int k = 0; k < plan.pass_count; ++k) {
        q.F = plan.F;
        apply_pass(&q.F, plan.pass_first + k);
        if (plan.converge && k >= plan.pass_min) { q.F.tiles = c->d_flag; q.F.tile_cap = flag_cap(plan.F); }
        q.index = k;
        if (k > 0) q.ev0 += ev_step;
        const rt_status s = run_sequence(c, r.st, plan.L, q);
        if (s != RT_OK) return s;
    }
    return RT_OK;
}

// the refined count of the latest eager adaptive frame lives in the control block: fetch it before anything else reuses the block
static rt_status settle_refined(rt_ctx *c) {
    if (!c->refined_on_device) return RT_OK;
    { const rt_status ws = wait_frames(c, LostStream::Report); if (ws != RT_OK) return ws; }
    Control h;
    HIPCHK(c, hipMemcpy(&h, c->d_ctl, sizeof h, hipMemcpyDeviceToHost));
    fold_stats(h);
    c->refined = h.refined;
    c->refined_on_device = false;
    return RT_OK;
}

static void make_cam(const rt_camera *cam, DCam *d) {
    std::memcpy(d->center, cam->center, sizeof d->center);
    std::memcpy(d->inv_view, cam->inv_view, sizeof d->inv_view);
    std::memcpy(d->vp, cam->viewport, sizeof d->vp);
    // getPerspectiveScale / scale (camera.hpp:164-166, 263-266): host double arithmetic, as the reference
    const float persp = static_cast<float>(static_cast<double>(1.0f) / std::tan(static_cast<double>(cam->fovy / 2.0f) * (M_PI / static_cast<double>(180.0f))));
    const float scale = static_cast<float>(1.0 / static_cast<double>(persp));
    d->k0 = cam->aspect * scale;
    d->k1 = scale;
}

// what a frame uploads: the (open) camera and, shutter on, the deltas to `close` behind it
static void make_cam_block(const rt_camera *cam, const rt_camera *close, DCamBlock *b) {
    std::memset(b, 0, sizeof *b);
    make_cam(cam, &b->cam);
    if (close) make_shutter(cam, close, &b->sh);
}

// ---- primary culling (Primary culling) ---------------------------------------------------------------------------------
// The tiles (8 x 8 pixels) of a W x H frame outside which no primary ray of the camera `d` can pass the root-box test of `box` (min, max):
// [rect[0], rect[2]) x [rect[1], rect[3]), clamped to the frame; (0, 0, 0, 0) when the box is out of view.  Host double arithmetic.
//
// The primary ray of raster point (fi, fj) is c + t (s - c), t >= 0, with s = A (n0, n1, -1) + T, n0 = k0 (2 (fi - vp0) / vp2 - 1),
// n1 = k1 (1 - 2 (fj - vp1) / vp3) (screen_point in rt_kernels.hip; A, T: the 3 x 3 part and the last column of inv_view).  With
// g = A^-1 (T - c) -- zero for every camera whose centre is its view matrix's -- a point P lies on that ray exactly when q = A^-1 (P - c)
// = t (n0 + g0, n1 + g1, g2 - 1): t = q2 / (g2 - 1), n0 = q0 / t - g0, n1 = q1 / t - g1, a projective map that is continuous on t > 0.  When
// all eight corners have t > 0 the whole box has (t is affine in P), the rays that meet it are the rays through the image of the box, that
// image lies in the convex hull of the eight projected corners, and the hull lies in their bounding rectangle.  When all eight have t < 0
// no ray meets the box.  The rectangle is then grown by at least one whole tile on every side: the kernels form the ray and test the box in
// float, which moves a borderline decision by far less (the bound is evaluated below and the whole frame returned when it is not small
// against the margin).
// Returns false -- and the whole frame -- whenever that argument does not hold or was not shown to hold.
static bool primary_rect(const DCam &d, const float *box, int32_t W, int32_t H, int32_t rect[4]) {
    const int32_t TX = (W + 7) / 8, TY = (H + 7) / 8;
    rect[0] = 0; rect[1] = 0; rect[2] = TX; rect[3] = TY;
    for (int k = 0; k < 3; ++k) if (!std::isfinite(d.center[k])) return false;
    for (int k = 0; k < 12; ++k) if (!std::isfinite(d.inv_view[k])) return false;
    for (int k = 0; k < 4; ++k) if (!std::isfinite(d.vp[k])) return false;
    for (int k = 0; k < 6; ++k) if (!std::isfinite(box[k])) return false;
    if (!std::isfinite(d.k0) || !std::isfinite(d.k1) || d.k0 == 0.0f || d.k1 == 0.0f || !(d.vp[2] > 0.0f) || !(d.vp[3] > 0.0f)) return false;
    for (int a = 0; a < 3; ++a) if (!(box[a] <= box[3 + a])) return false;
    const double c[3] = {d.center[0], d.center[1], d.center[2]};
    const float *m = d.inv_view;
    const double A[3][3] = {{m[0], m[1], m[2]}, {m[4], m[5], m[6]}, {m[8], m[9], m[10]}};
    const double T[3] = {m[3], m[7], m[11]};
    double amax = 0.0, arow = 0.0, tmax_abs = 0.0, cmax = 0.0, bmax = 0.0, ext = 0.0;
    for (int i = 0; i < 3; ++i) {
        double rs = 0.0;
        for (int j = 0; j < 3; ++j) { amax = std::fmax(amax, std::fabs(A[i][j])); rs += std::fabs(A[i][j]); }
        arow = std::fmax(arow, rs);
        tmax_abs = std::fmax(tmax_abs, std::fabs(T[i]));
        cmax = std::fmax(cmax, std::fabs(c[i]));
        bmax = std::fmax(bmax, std::fmax(std::fabs(static_cast<double>(box[i])), std::fabs(static_cast<double>(box[3 + i]))));
        ext = std::fmax(ext, static_cast<double>(box[3 + i]) - static_cast<double>(box[i]));
    }
    const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    if (!(std::fabs(det) > 1e-9 * amax * amax * amax)) return false;            // (also: a zero matrix)
    double I[3][3];                                                             // A^-1
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            I[j][i] = (A[i1][j1] * A[i2][j2] - A[i1][j2] * A[i2][j1]) / det;
        }
    double irow = 0.0;
    for (int i = 0; i < 3; ++i) irow = std::fmax(irow, std::fabs(I[i][0]) + std::fabs(I[i][1]) + std::fabs(I[i][2]));
    auto apply = [&](const double v[3], double out[3]) { for (int i = 0; i < 3; ++i) out[i] = I[i][0] * v[0] + I[i][1] * v[1] + I[i][2] * v[2]; };
    const double e[3] = {T[0] - c[0], T[1] - c[1], T[2] - c[2]};
    double g[3];
    apply(e, g);
    const double gz = g[2] - 1.0;
    if (!(std::fabs(gz) > 1e-6)) return false;
    // the camera centre inside the box inflated by 1e-3 of the sizes involved, or exactly on one of its face planes (where the slab test
    // divides 0 by 0 for a ray that runs in the plane and its verdict no longer follows the geometry)
    const double infl = 1e-3 * (ext + cmax + bmax);
    bool inside = true;
    double dist2 = 0.0;                                                         // squared distance centre -> box
    for (int a = 0; a < 3; ++a) {
        if (d.center[a] == box[a] || d.center[a] == box[3 + a]) return false;
        if (c[a] < box[a] - infl || c[a] > box[3 + a] + infl) inside = false;
        const double o = c[a] < box[a] ? box[a] - c[a] : (c[a] > box[3 + a] ? c[a] - box[3 + a] : 0.0);
        dist2 += o * o;
    }
    if (inside) return false;
    const double dist = std::sqrt(dist2);
    // the eight corners.  t is affine in P: when every corner has t < 0 so has the whole box -- no ray reaches it, the rectangle is empty;
    // when the signs are mixed the box crosses the plane t = 0 and its image is unbounded: the whole frame.
    double qs[8][3];
    int behind = 0;
    for (int k = 0; k < 8; ++k) {
        const double v[3] = {static_cast<double>(box[(k & 1) ? 3 : 0]) - c[0], static_cast<double>(box[(k & 2) ? 4 : 1]) - c[1],
                             static_cast<double>(box[(k & 4) ? 5 : 2]) - c[2]};
        apply(v, qs[k]);
        const double t = qs[k][2] / gz;
        if (!std::isfinite(t)) return false;
        if (t < 0.0) ++behind;
    }
    if (behind == 8) { rect[0] = rect[1] = rect[2] = rect[3] = 0; return true; }
    double tmin = 0.0, tmax = 0.0, x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0;
    for (int k = 0; k < 8; ++k) {
        const double *q = qs[k];
        const double t = q[2] / gz;
        if (!(t > 0.0)) return false;                                          // a corner at or behind the camera
        const double n0 = q[0] / t - g[0], n1 = q[1] / t - g[1];
        const double fx = static_cast<double>(d.vp[0]) + (n0 / static_cast<double>(d.k0) + 1.0) * 0.5 * static_cast<double>(d.vp[2]);
        const double fy = static_cast<double>(d.vp[1]) + (1.0 - n1 / static_cast<double>(d.k1)) * 0.5 * static_cast<double>(d.vp[3]);
        if (!std::isfinite(fx) || !std::isfinite(fy)) return false;
        if (k == 0) { tmin = tmax = t; x0 = x1 = fx; y0 = y1 = fy; }
        tmin = std::fmin(tmin, t); tmax = std::fmax(tmax, t);
        x0 = std::fmin(x0, fx); x1 = std::fmax(x1, fx); y0 = std::fmin(y0, fy); y1 = std::fmax(y1, fy);
    }
    if (tmin < 1e-3 * tmax) return false;                                       // a corner at a depth small against the box's extent in depth
    // float rounding of the device's ray, in raster units: the direction of an on-screen ray carries an absolute error of a few ulp of the
    // terms it is summed from, A^-1 turns it into an error of (n0, n1, -1), the raster map into pixels.  And the slab test's own rounding is
    // ~1e-6 of the distances it compares: the 8-pixel margin, as an angle, must stay far above that relative to the distance to the box.
    const double k0 = std::fabs(static_cast<double>(d.k0)), k1 = std::fabs(static_cast<double>(d.k1));
    const double u0 = std::fmax(std::fabs(2.0 * (0.0 - d.vp[0]) / d.vp[2] - 1.0), std::fabs(2.0 * (static_cast<double>(W) - d.vp[0]) / d.vp[2] - 1.0));
    const double u1 = std::fmax(std::fabs(1.0 - 2.0 * (0.0 - d.vp[1]) / d.vp[3]), std::fabs(1.0 - 2.0 * (static_cast<double>(H) - d.vp[1]) / d.vp[3]));
    const double nmax = std::fmax(1.0, std::fmax(k0 * u0, k1 * u1));
    const double err_dir = 4.76837158203125e-07 * (arow * nmax + tmax_abs + cmax);             // 2^-21: 8 ulp of the largest term
    const double err_n = irow * err_dir * (1.0 + nmax);
    const double err_pix = std::fmax(err_n / k0 * 0.5 * static_cast<double>(d.vp[2]), err_n / k1 * 0.5 * static_cast<double>(d.vp[3]));
    if (!(err_pix < 1.0)) return false;
    const double margin_angle = 16.0 * std::fmin(k0 / static_cast<double>(d.vp[2]), k1 / static_cast<double>(d.vp[3])) / (1.0 + nmax);
    if (!(margin_angle * dist > 1e-4 * (cmax + bmax + dist))) return false;
    // the rectangle in tiles, one whole tile beyond the tiles of the extreme corners on every side
    auto tile_of = [](double f, int32_t n) -> int32_t {                         // floor(f / 8), clamped to [-2, n + 2]
        const double t = std::floor(f / 8.0);
        return t < -2.0 ? -2 : (t > static_cast<double>(n) + 2.0 ? n + 2 : static_cast<int32_t>(t));
    };
    int32_t tx0 = tile_of(x0, TX) - 1, tx1 = tile_of(x1, TX) + 2, ty0 = tile_of(y0, TY) - 1, ty1 = tile_of(y1, TY) + 2;
    tx0 = std::max(tx0, 0); ty0 = std::max(ty0, 0); tx1 = std::min(tx1, TX); ty1 = std::min(ty1, TY);
    if (tx0 >= tx1 || ty0 >= ty1) { rect[0] = rect[1] = rect[2] = rect[3] = 0; return true; }        // out of view
    rect[0] = tx0; rect[1] = ty0; rect[2] = tx1; rect[3] = ty1;
    return true;
}

// the rectangle a frame of plan F uploads with its camera: the culled one, or the whole frame (which nothing reads unless F.cull is set)
static void make_cull_rect(const rt_ctx *c, const DFrame &F, DCamBlock *b) {
    if (F.cull != 0) { (void)primary_rect(b->cam, c->root_box, F.width, F.height, b->rect); return; }
    b->rect[0] = 0; b->rect[1] = 0; b->rect[2] = (F.width + 7) / 8; b->rect[3] = (F.height + 7) / 8;
}

extern "C" rt_status rt_set_primary_cull(rt_ctx *c, int32_t on) {
    if (!c) return RT_ERR_INVALID;
    c->primary_cull = on != 0;
    return RT_OK;
}

extern "C" rt_status rt_debug_primary_rect(const rt_camera *cam, const float box[6], int32_t width, int32_t height, int32_t supersampling,
                                           float lens_aperture, int32_t shutter_on, int32_t pass_first, int32_t pass_count, int32_t rect[4]) {
    if (!cam || !box || !rect || width <= 0 || height <= 0) return RT_ERR_INVALID;
    SampleSettings m;
    m.ss = supersampling; m.lens_aperture = lens_aperture; m.shutter_on = shutter_on != 0; m.pass_first = pass_first; m.pass_count = pass_count;
    DCam d;
    make_cam(cam, &d);
    rect[0] = 0; rect[1] = 0; rect[2] = (width + 7) / 8; rect[3] = (height + 7) / 8;
    if (m.cull_ok()) (void)primary_rect(d, box, width, height, rect);
    return RT_OK;
}

// waits for every frame the context has enqueued (its own stream and the stream of the most recent rt_render_device call) and reports a
// work-list overflow of any of them
extern "C" rt_status rt_synchronize(rt_ctx *c) {
    if (!c) return RT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const rt_status ws = wait_frames(c, LostStream::Report);
    if (ws != RT_OK) return ws;
    return c->d_ctl ? check_overflow(c) : RT_OK;
}

extern "C" rt_status rt_render_device(rt_ctx *c, const rt_camera *cam, const rt_lights *lights, const rt_params *p,
                                      float *d_out_rgb, uint8_t *d_out_u8, int32_t *d_out_hit, void *stream, rt_stats *stats) {
    if (!c) return RT_ERR_INVALID;
    if (!c->has_scene) { c->err = "render before rt_upload_scene"; return RT_ERR_NO_SCENE; }
    if (!cam) { c->err = "camera is null"; return RT_ERR_INVALID; }
    const SampleSettings &m = c->smp;
    if (d_out_hit && m.ss > 1) { c->err = "rt_render_device: no hit ids with supersampling (n > 1)"; return RT_ERR_INVALID; }
    if (d_out_hit && m.pass_count > 1) { c->err = "rt_render_device: no hit ids with several passes (rt_set_passes count > 1)"; return RT_ERR_INVALID; }
    if (m.shutter_on && !shutter_compatible(cam, &m.shutter_close)) { c->err = k_shutter_mismatch; return RT_ERR_INVALID; }
    HIPCHK(c, hipSetDevice(c->device));
    FramePlan plan;
    rt_status s = plan_frame(c, lights, p, nullptr, &plan);
    if (s != RT_OK) return s;
    if (stats) std::memset(stats, 0, sizeof *stats);
    const DFrame &F = plan.F;
    if (F.npix == 0) { c->refined = 0; c->refined_on_device = false; c->pass_map_on = m.converge_on(); c->pass_map_pix = 0; return RT_OK; }
    // rt_pass_map: no map until this frame has been enqueued whole (every error return below leaves it off)
    c->pass_map_on = false; c->pass_map_pix = 0;
    const auto map_ready = [&]() {
        c->pass_map_on = plan.converge;
        c->pass_map_pix = static_cast<size_t>(F.out_width) * static_cast<size_t>(F.out_rows);
    };
    if ((s = reserve_frame(c, plan, nullptr)) != RT_OK) return s;
    DCamBlock dc;
    make_cam_block(cam, m.shutter_on ? &m.shutter_close : nullptr, &dc);
    make_cull_rect(c, F, &dc);
    hipStream_t st = stream_or_own(c, stream);
    FrameRun run{st, &dc, &c->tab, d_out_rgb, d_out_u8, d_out_hit, false, 0};
    c->last_frame_stream = st;
    // rt_supersampling_refined: an adaptive frame's count is read from the control block when asked for
    c->refined_on_device = plan.kind == FramePlan::ADAPTIVE;
    c->refined = F.ss == 1 ? 0u : static_cast<uint64_t>(F.out_width) * static_cast<uint64_t>(F.out_rows);
    // the overlapped route (Frames in flight): the launches up to the resolve on the internal stream of the set the overlapped
    // frame before this one did not use, k_resolve -- the only launch that writes caller memory -- on the caller's stream
    if (c->sets.on() && !c->sets.refused()) {
        FsFrame f{plan.kind == FramePlan::PLAIN, stats != nullptr, p->collect_stats != 0, d_out_hit != nullptr, plan.L.mode == RT_LIGHT_SPHERE, false, false};
        if (c->sets.admits(f) && (s = stream_capturing(c, st, &f.capturing)) != RT_OK) return s;
        if (c->sets.admits(f) && !c->sets.always()) {
            // a lone frame: the caller's stream has drained and no use of either set is still running
            f.idle = hipStreamQuery(st) == hipSuccess;
            for (int k = 0; k < 2 && f.idle; ++k)
                if (c->sets.outstanding(k)) f.idle = hipEventQuery(c->fs_event[static_cast<int>(fs_set_free(k))]) == hipSuccess;
            if (!f.idle) (void)hipGetLastError();      // (hipErrorNotReady is an answer, not an error)
        }
        bool overlap = c->sets.admits(f);
        if (overlap && (s = ensure_second_set(c, st, &overlap)) != RT_OK) return s;
        if (overlap) {
            const FsSteps steps = c->sets.overlapped_frame();
            Sequence q;
            q.F = plan.F;
            q.d_rgb = d_out_rgb; q.d_u8 = d_out_u8;
            q.cam = &dc;
            q.ev0 = c->ev_base;
            q.set = steps.set;
            SeqState state;
            for (int i = 0; i < steps.n && s == RT_OK; ++i) {
                const FsStep &step = steps.step[i];
                if (step.op == FsStep::BODY) s = sequence_body(c, fs_stream_of(c, step.stream, st), plan.L, q, &state);
                else if (step.op == FsStep::RESOLVE) s = sequence_resolve(c, fs_stream_of(c, step.stream, st), q, state);
                else s = fs_exec(c, step, st);
            }
            if (s != RT_OK) {
                // (a frame that stopped half way: nothing stays outstanding behind a wait for everything)
                (void)hipDeviceSynchronize();
                (void)c->sets.host_wait();          // (the device has drained: the steps are not executed)
                return s;
            }
            ++c->overlapped_frames;
            map_ready();
            return RT_OK;
        }
    }
    bool capturing = false;
    if ((s = set0_begin(c, st, &capturing)) != RT_OK) return s;
    if (stats && p->collect_stats == 1) {
        // counting pass: same frame with the no-early-out traversal variants (never part of a timed region)
        run.count = true;
        if ((s = enqueue_frame(c, plan, run)) != RT_OK) return s;
        if ((s = fill_stats(c, st, plan.shape, false, stats, true)) != RT_OK) return s;
        run.count = false;
    }
    if (p->collect_stats == 2) {
        // one pending event set per launch sequence
        const size_t first = c->ev_base, ev_step = frame_events(plan.shape.levels_run);
        run.timed = 2;
        if ((s = enqueue_frame(c, plan, run)) != RT_OK) return s;
        for (uint32_t k = 0; k < plan.shape.sequences; ++k) c->pending.emplace_back(first + k * ev_step, plan.shape.levels_run);
        c->ev_base = first + plan.shape.sequences * ev_step;
        c->pending_stream = st;
        c->pending_shape = plan.shape;
        map_ready();
        return set0_end(c, st, capturing);
    }
    run.timed = stats != nullptr ? 1 : 0;
    if ((s = enqueue_frame(c, plan, run)) != RT_OK) return s;
    if (stats) {
        const uint64_t bt = stats->box_tests, lr = stats->leaf_tri_refs, bts = stats->box_tests_shadow, lrs = stats->leaf_tri_refs_shadow;
        if ((s = fill_stats(c, st, plan.shape, true, stats, false)) != RT_OK) return s;
        stats->box_tests = bt; stats->leaf_tri_refs = lr; stats->box_tests_shadow = bts; stats->leaf_tri_refs_shadow = lrs;
    }
    map_ready();
    return set0_end(c, st, capturing);
}

// (frames already enqueued are not touched: the uses of set 0 that follow wait for them as they would have with the switch on)
extern "C" rt_status rt_set_frame_overlap(rt_ctx *c, int32_t on) {
    if (!c) return RT_ERR_INVALID;
#ifdef RT_WORK_COUNTERS
    (void)on;                    // (the counting build's step counters are read from set 0's control block: its frames stay on it)
#else
    c->sets.set_on(on != 0, on == 2);
#endif
    return RT_OK;
}

extern "C" rt_status rt_debug_overlapped_frames(rt_ctx *c, uint64_t *frames) {
    if (!c || !frames) return RT_ERR_INVALID;
    *frames = c->overlapped_frames;
    return RT_OK;
}

extern "C" rt_status rt_pass_map(rt_ctx *c, uint16_t *out, size_t n_pixels) {
    if (!c) return RT_ERR_INVALID;
    if (!c->pass_map_on) { c->err = "rt_pass_map: the latest frame was not an adaptive-pass frame (rt_set_pass_tolerance)"; return RT_ERR_INVALID; }
    if (n_pixels != c->pass_map_pix || (n_pixels != 0 && !out)) { c->err = "rt_pass_map: n_pixels must be the width x the local rows of the latest frame"; return RT_ERR_INVALID; }
    const rt_status s = rt_synchronize(c);
    if (s != RT_OK) return s;
    if (n_pixels) HIPCHK(c, hipMemcpy(out, c->tab.taken, n_pixels * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

// (Control::refined / ST_REFINED is read here for ADAPTIVE plans only -- refined_on_device.  A PASSES plan with `converge` uses the same slot
//  for the active pixels of its list passes, which only FrameShape::pixels reads; this function then reports what it reports for any
//  regular frame, the host value set in rt_render_device.)
extern "C" rt_status rt_supersampling_refined(rt_ctx *c, uint64_t *refined) {
    if (!c || !refined) return RT_ERR_INVALID;
    rt_status s = rt_synchronize(c);
    if (s == RT_OK) s = settle_refined(c);
    if (s != RT_OK) return s;
    *refined = c->refined;
    return RT_OK;
}

struct rt_graph {
    rt_ctx *ctx = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    FramePlan plan;                   // the frame that was captured (rt_set_* calls since do not change it)
    FrameTables tab;                  // the graph's own offsets, row tables and running sum (the kernel arguments hold these pointers)
    uint64_t generation = 0, scene_generation = 0;
    hipStream_t last_stream = nullptr;
    rt_graph() = default;
    rt_graph(const rt_graph &) = delete;
    ~rt_graph() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
};

extern "C" rt_status rt_graph_create(rt_ctx *c, const rt_lights *lights, const rt_params *p, float *d_out_rgb, uint8_t *d_out_u8,
                                     rt_graph **out) {
    if (!c || !out) return RT_ERR_INVALID;
    *out = nullptr;
    if (!c->has_scene) { c->err = "rt_graph_create before rt_upload_scene"; return RT_ERR_NO_SCENE; }
    if (!d_out_rgb && !d_out_u8) { c->err = "rt_graph_create: no output buffer"; return RT_ERR_INVALID; }
    HIPCHK(c, hipSetDevice(c->device));
    std::unique_ptr<rt_graph> g(new rt_graph());      // (every error exit below frees it and what it owns)
    g->ctx = c;
    const FramePlan &plan = g->plan;                  // (shutter: the graph keeps "on"; both cameras come with every launch)
    rt_status s = plan_frame(c, lights, p, &g->tab.offsets, &g->plan);
    if (s != RT_OK) return s;
    if (plan.F.npix == 0) { c->err = "rt_graph_create: empty shard"; return RT_ERR_INVALID; }
    // every allocation happens BEFORE the capture
    if ((s = reserve_frame(c, plan, &g->tab)) != RT_OK) return s;
    if ((s = settle_refined(c)) != RT_OK) return s;   // (the capture reuses the control block)
    if (hipStreamSynchronize(c->stream) != hipSuccess) { c->err = "rt_graph_create: hipStreamSynchronize failed"; return RT_ERR_HIP; }
    g->generation = c->frame_generation; g->scene_generation = c->scene_generation;
    if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { c->err = "hipStreamBeginCapture failed"; return RT_ERR_HIP; }
    s = enqueue_frame(c, plan, FrameRun{c->stream, nullptr, &g->tab, d_out_rgb, d_out_u8, nullptr, false, 0});
    const hipError_t e = hipStreamEndCapture(c->stream, &g->graph);
    if (s != RT_OK || e != hipSuccess || !g->graph) {
        if (s == RT_OK) { c->err = std::string("hipStreamEndCapture: ") + hipGetErrorString(e); s = RT_ERR_HIP; }
        return s;
    }
    if (hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0) != hipSuccess) { c->err = "hipGraphInstantiate failed"; return RT_ERR_HIP; }
    *out = g.release();
    return RT_OK;
}

static rt_status graph_launch(rt_graph *g, const rt_camera *cam, const rt_camera *close, void *stream) {
    rt_ctx *c = g->ctx;
    if (g->generation != c->frame_generation) { c->err = "rt_graph_launch: the frame buffers were reallocated after capture; re-create the graph"; return RT_ERR_INVALID; }
    if (g->scene_generation != c->scene_generation) { c->err = "rt_graph_launch: a scene was uploaded after capture (the graph holds the old scene's device pointers); re-create the graph"; return RT_ERR_INVALID; }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream_or_own(c, stream);
    rt_status cs = settle_refined(c);                 // (the replay reuses the control block)
    if (cs != RT_OK) return cs;
    DCamBlock dc;
    make_cam_block(cam, close, &dc);
    make_cull_rect(c, g->plan.F, &dc);                // (the rectangle of THIS camera: the captured kernels read it from the block)
    cs = upload_camera(c, dc, st);
    if (cs != RT_OK) return cs;
    bool capturing = false;
    if ((cs = set0_begin(c, st, &capturing)) != RT_OK) return cs;     // (the graph's kernels work on set 0)
    HIPCHK(c, hipGraphLaunch(g->exec, st));
    g->last_stream = st;
    return set0_end(c, st, capturing);
}

// (on a graph captured with the shutter on this is the still frame of cam: close = cam, every delta 0)
extern "C" rt_status rt_graph_launch(rt_graph *g, const rt_camera *cam, void *stream) {
    if (!g || !cam) return RT_ERR_INVALID;
    return graph_launch(g, cam, g->plan.F.shutter != 0 ? cam : nullptr, stream);
}

extern "C" rt_status rt_graph_launch_shutter(rt_graph *g, const rt_camera *open, const rt_camera *close, void *stream) {
    if (!g || !open || !close) return RT_ERR_INVALID;
    rt_ctx *c = g->ctx;
    if (g->plan.F.shutter == 0) { c->err = "rt_graph_launch_shutter: the graph was captured with the shutter off"; return RT_ERR_INVALID; }
    if (!shutter_pose_finite(close)) { c->err = "rt_graph_launch_shutter: the close camera's center / inv_view must be finite"; return RT_ERR_INVALID; }
    if (!shutter_compatible(open, close)) { c->err = k_shutter_mismatch; return RT_ERR_INVALID; }
    return graph_launch(g, open, close, stream);
}

extern "C" rt_status rt_graph_stats(rt_graph *g, rt_stats *out) {
    if (!g || !out) return RT_ERR_INVALID;
    rt_ctx *c = g->ctx;
    std::memset(out, 0, sizeof *out);
    if (g->scene_generation != c->scene_generation) { c->err = "rt_graph_stats: a scene was uploaded after capture; re-create the graph"; return RT_ERR_INVALID; }
    HIPCHK(c, hipSetDevice(c->device));
    return fill_stats(c, g->last_stream ? g->last_stream : c->stream, g->plan.shape, false, out, false);
}

extern "C" void rt_graph_destroy(rt_graph *g) {
    if (!g) return;
    (void)hipSetDevice(g->ctx->device);
    if (g->last_stream) (void)hipStreamSynchronize(g->last_stream);
    delete g;
}

extern "C" rt_status rt_timing_collect(rt_ctx *c, rt_stats *out) {
    if (!c || !out) return RT_ERR_INVALID;
    std::memset(out, 0, sizeof *out);
    if (c->pending.empty()) return RT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    Control h;
    rt_status s = read_counters(c, c->pending_stream, c->pending_shape, h, out);
    if (s != RT_OK) return s;
    for (const auto &fr : c->pending)
        if ((s = sum_frame_times(c, fr.first, fr.second, out, true)) != RT_OK) break;
    c->pending.clear();
    c->ev_base = 0;
    return s;
}

// the staging buffers of the entry points with host outputs, for n pixels or rays
static rt_status ensure_out(rt_ctx *c, size_t n) {
    if (n <= c->d_t.cap) return RT_OK;      // (the three grow together and d_t last: its capacity is the group's)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->d_rgb.grow(n * 3));
    HIPCHK(c, c->d_hit.grow(n));
    HIPCHK(c, c->d_t.grow(n));
    return RT_OK;
}

extern "C" rt_status rt_render(rt_ctx *c, const rt_camera *cam, const rt_lights *lights, const rt_params *p,
                               float *out_rgb, int32_t *out_hit, rt_stats *stats) {
    if (!c) return RT_ERR_INVALID;
    if (!out_rgb || !p) { c->err = "rt_render: null output or params"; return RT_ERR_INVALID; }
    if (out_hit && c->smp.ss > 1) { c->err = "rt_render: no hit ids with supersampling (n > 1)"; return RT_ERR_INVALID; }
    if (out_hit && c->smp.pass_count > 1) { c->err = "rt_render: no hit ids with several passes (rt_set_passes count > 1)"; return RT_ERR_INVALID; }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = static_cast<size_t>(rt_local_rows(p)) * static_cast<size_t>(p->width > 0 ? p->width : 0);
    rt_status s = ensure_out(c, npix);
    if (s != RT_OK) return s;
    s = rt_render_device(c, cam, lights, p, c->d_rgb, nullptr, out_hit ? c->d_hit : nullptr, nullptr, stats);
    if (s != RT_OK) return s;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((s = check_overflow(c)) != RT_OK) return s;
    if (npix) {
        HIPCHK(c, hipMemcpy(out_rgb, c->d_rgb, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
        if (out_hit) HIPCHK(c, hipMemcpy(out_hit, c->d_hit, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

// What rt_trace_rays and rt_trace_rays_device share: n listed rays as ONE launch sequence on `st` -- the frame of n listed rays, its working
// set (ensure_frame) and the sequence with primary = false.  `source` puts the n RayItems into d_rays[0], in order on `st`, and says where
// the results go: a host loop and a copy, or k_pack_rays.  Nothing here synchronises unless ensure_frame grows or settle_refined fetches.
struct ListedOut {
    float *rgb = nullptr;
    int32_t *face = nullptr;
    float *t = nullptr;
};
template <typename Source>
static rt_status trace_listed(rt_ctx *c, hipStream_t st, const DLights &L, int32_t max_depth, int32_t n, Source &&source) {
    DFrame F{};
    F.width = n; F.height = 1; F.local_rows = 1; F.row0 = 0; F.stripe = 1; F.rank = 0; F.nranks = 1;
    F.tiles_x = (n + 7) / 8; F.tiles_y = 1; F.npix = static_cast<uint32_t>(n);
    F.max_depth = max_depth < 0 ? RT_MAX_DEPTH : max_depth;
    F.dyn_trace = c->dyn_trace;
    F.ss = 1; F.out_width = n; F.out_rows = 1;      // (input rays: supersampling does not apply)
    rt_status s = ensure_frame(c, working_set(L, F));
    if (s != RT_OK) return s;
    ListedOut out;
    bool capturing = false;
    if ((s = set0_begin(c, st, &capturing)) != RT_OK) return s;          // (the source writes set 0's ray list)
    if ((s = source(&out)) != RT_OK) return s;
    if ((s = settle_refined(c)) != RT_OK) return s;          // (these rays reuse the control block)
    Sequence q;
    q.F = F; q.primary = false; q.n_input_rays = static_cast<uint32_t>(n);
    q.d_rgb = out.rgb; q.d_hit = out.face; q.d_t = out.t;
    if ((s = run_sequence(c, st, L, q)) != RT_OK) return s;
    return set0_end(c, st, capturing);
}

extern "C" rt_status rt_trace_rays(rt_ctx *c, const rt_lights *lights, int32_t max_depth, int32_t n, const float *origin,
                                   const float *dir, float *out_rgb, int32_t *out_face, float *out_t) {
    if (!c) return RT_ERR_INVALID;
    if (!c->has_scene) { c->err = "rt_trace_rays before rt_upload_scene"; return RT_ERR_NO_SCENE; }
    if (n < 0 || (n && (!origin || !dir || !out_rgb))) { c->err = "rt_trace_rays: bad arguments"; return RT_ERR_INVALID; }
    if (max_depth > RT_MAX_DEPTH) { c->err = "rt_trace_rays: max_depth above RT_MAX_DEPTH"; return RT_ERR_UNSUPPORTED; }
    if (n == 0) return RT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DLights L;
    rt_status s = check_lights(c, lights, &L);
    if (s != RT_OK) return s;
    const size_t need = static_cast<size_t>(n);
    std::vector<RayItem> rays;
    s = trace_listed(c, c->stream, L, max_depth, n, [&](ListedOut *out) -> rt_status {
        rays.resize(need);
        for (int32_t i = 0; i < n; ++i) {
            RayItem &r = rays[static_cast<size_t>(i)];
            r.ox = origin[i * 3]; r.oy = origin[i * 3 + 1]; r.oz = origin[i * 3 + 2];
            r.dx = dir[i * 3]; r.dy = dir[i * 3 + 1]; r.dz = dir[i * 3 + 2];
            r.lx = r.ly = r.lz = 0.f; r.lmode = 0u; r.pix = static_cast<uint32_t>(i); r.pad = 0u;
        }
        const rt_status os_ = ensure_out(c, need);
        if (os_ != RT_OK) return os_;
        HIPCHK(c, hipMemcpyAsync(c->d_rays[0], rays.data(), need * sizeof(RayItem), hipMemcpyHostToDevice, c->stream));
        *out = ListedOut{c->d_rgb, c->d_hit, c->d_t};
        return RT_OK;
    });
    if (s != RT_OK) return s;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((s = check_overflow(c)) != RT_OK) return s;
    HIPCHK(c, hipMemcpy(out_rgb, c->d_rgb, need * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out_face) HIPCHK(c, hipMemcpy(out_face, c->d_hit, need * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_t) HIPCHK(c, hipMemcpy(out_t, c->d_t, need * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" rt_status rt_light_strikes(rt_ctx *c, int32_t n, const float *hit, const float *light, uint8_t *vis) {
    if (!c) return RT_ERR_INVALID;
    if (!c->has_scene) { c->err = "rt_light_strikes before rt_upload_scene"; return RT_ERR_NO_SCENE; }
    if (n < 0 || (n && (!hit || !light || !vis))) { c->err = "rt_light_strikes: bad arguments"; return RT_ERR_INVALID; }
    if (const char *bad = query_strikes_count(n)) { c->err = std::string("rt_light_strikes: ") + bad; return RT_ERR_INVALID; }
    if (n == 0) return RT_OK;
    Staging g(c);
    const size_t nn = static_cast<size_t>(n);
    const float *d_hit = g.in(hit, nn * 3), *d_light = g.in(light, nn * 3);
    uint8_t *d_vis = g.out(vis, nn);
    return g.finish([&] { return rt_light_strikes_device(c, n, d_hit, d_light, d_vis, nullptr); });
}

// ---- device ray queries (Device ray queries): the tracer on caller-owned device rays ----------------------------------
// what every query call checks first; `bad`: the failed argument rule (rt_query_chunks.hpp) or null
static rt_status query_entry(rt_ctx *c, const char *who, const char *bad) {
    if (!c) return RT_ERR_INVALID;
    if (!c->has_scene) { c->err = std::string(who) + " before rt_upload_scene"; return RT_ERR_NO_SCENE; }
    if (bad) { c->err = std::string(who) + ": " + bad; return RT_ERR_INVALID; }
    return RT_OK;
}

extern "C" rt_status rt_closest_hits_device(rt_ctx *c, int32_t n, const float *d_origin, const float *d_dir, int32_t *d_face, float *d_t, void *stream) {
    const rt_status s = query_entry(c, "rt_closest_hits_device", query_closest_args(n, d_origin, d_dir, d_face, d_t));
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    launch_closest(query_grid(n, c->cus), stream_or_own(c, stream), c->S, n, d_origin, d_dir, d_face, d_t);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_closest_hits(rt_ctx *c, int32_t n, const float *origin, const float *dir, int32_t *face, float *t) {
    const rt_status s = query_entry(c, "rt_closest_hits", query_closest_args(n, origin, dir, face, t));
    if (s != RT_OK || n == 0) return s;
    Staging g(c);
    const size_t rays = static_cast<size_t>(n);
    const float *d_origin = g.in(origin, rays * 3), *d_dir = g.in(dir, rays * 3);
    int32_t *d_face = g.out(face, rays);
    float *d_t = g.out(t, rays);
    return g.finish([&] { return rt_closest_hits_device(c, n, d_origin, d_dir, d_face, d_t, nullptr); });
}

// ---- ordered ray hits (Ordered ray hits): one kernel on the stream, the scene alone ------------------------------------
static_assert(RT_MAX_RAY_HITS == kMaxRayHits, "rt_hits_layout.hpp restates the header's constant");

extern "C" rt_status rt_ray_hits_device(rt_ctx *c, int32_t n, const float *d_origin, const float *d_dir, int32_t k, float t_max, int32_t *d_face,
                                        float *d_t, int32_t *d_count, void *stream) {
    const rt_status s = query_entry(c, "rt_ray_hits_device", hits_args(n, d_origin, d_dir, k, t_max, d_face, d_t, d_count));
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    launch_ray_hits(query_grid(n, c->cus), stream_or_own(c, stream), c->S, n, d_origin, d_dir, k, t_max, d_face, d_t, d_count);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_ray_hits(rt_ctx *c, int32_t n, const float *origin, const float *dir, int32_t k, float t_max, int32_t *face, float *t,
                                 int32_t *count) {
    const rt_status s = query_entry(c, "rt_ray_hits", hits_args(n, origin, dir, k, t_max, face, t, count));
    if (s != RT_OK || n == 0) return s;
    Staging g(c);
    const size_t rays = static_cast<size_t>(n), slots = rays * static_cast<size_t>(k);
    const float *d_origin = g.in(origin, rays * 3), *d_dir = g.in(dir, rays * 3);
    int32_t *d_face = g.out(face, slots);
    float *d_t = g.out(t, slots);
    int32_t *d_count = g.out(count, rays);
    return g.finish([&] { return rt_ray_hits_device(c, n, d_origin, d_dir, k, t_max, d_face, d_t, d_count, nullptr); });
}

extern "C" rt_status rt_light_strikes_device(rt_ctx *c, int32_t n, const float *d_hit, const float *d_light, uint8_t *d_vis, void *stream) {
    const rt_status s = query_entry(c, "rt_light_strikes_device", query_strikes_args(n, d_hit, d_light, d_vis));
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    launch_segments(query_grid(n, c->cus), stream_or_own(c, stream), c->S, n, d_hit, d_light, d_vis);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_set_query_chunk(rt_ctx *c, int32_t rays) {
    if (!c) return RT_ERR_INVALID;
    if (!query_chunk_ok(rays)) { c->err = "rt_set_query_chunk: rays must be in 64 .. 2^24"; return RT_ERR_INVALID; }
    c->query_chunk = rays;
    return RT_OK;
}

extern "C" rt_status rt_trace_rays_device(rt_ctx *c, const rt_lights *lights, int32_t max_depth, int32_t n, const float *d_origin, const float *d_dir,
                                          float *d_out_rgb, int32_t *d_out_face, float *d_out_t, void *stream) {
    rt_status s = query_entry(c, "rt_trace_rays_device", query_trace_args(n, d_origin, d_dir, d_out_rgb, d_out_face, d_out_t));
    if (s != RT_OK) return s;
    if (max_depth > RT_MAX_DEPTH) { c->err = "rt_trace_rays_device: max_depth above RT_MAX_DEPTH"; return RT_ERR_UNSUPPORTED; }
    if (n == 0) return RT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DLights L;
    if ((s = check_lights(c, lights, &L)) != RT_OK) return s;
    if ((s = settle_refined(c)) != RT_OK) return s;          // (before anything is enqueued: the sequences reuse the control block)
    hipStream_t st = stream_or_own(c, stream);
    // one launch sequence per chunk, in order on the stream: the working set is that of one chunk whatever n is (the first is the largest)
    const size_t chunks = query_chunk_count(n, c->query_chunk);
    c->last_frame_stream = st;
    for (size_t k = 0; k < chunks; ++k) {
        const QueryChunk ch = query_chunk_at(n, c->query_chunk, k);
        s = trace_listed(c, st, L, max_depth, ch.count, [&](ListedOut *out) -> rt_status {
            launch_pack_rays(st, ch.count, d_origin + ch.first * 3, d_dir + ch.first * 3, c->d_rays[0]);
            *out = ListedOut{d_out_rgb + ch.first * 3, d_out_face ? d_out_face + ch.first : nullptr, d_out_t ? d_out_t + ch.first : nullptr};
            return RT_OK;
        });
        if (s != RT_OK) return s;
    }
    return RT_OK;
}

// ---- ambient occlusion (Ambient occlusion): the definition's host half and the two device calls ------------------------
static_assert(RT_AO_MAX_GRID == kAoMaxGrid && RT_AO_ROTATIONS == kAoRotations, "rt_ao_layout.hpp restates the header's constants");

extern "C" rt_status rt_ao_directions(int32_t m, float *out) {
    if (!ao_grid_ok(m) || !out) return RT_ERR_INVALID;
    for (int k = 0; k < m * m; ++k) {
        double a, b;
        concentric_disc(2.0 * ((k % m + 0.5) / m) - 1.0, 2.0 * ((k / m + 0.5) / m) - 1.0, &a, &b);       // the rule of rt_lens_table
        const double zz = 1.0 - a * a - b * b;
        out[k * 3] = static_cast<float>(a); out[k * 3 + 1] = static_cast<float>(b); out[k * 3 + 2] = static_cast<float>(std::sqrt(zz > 0.0 ? zz : 0.0));
    }
    return RT_OK;
}

// rotation step r of RT_AO_ROTATIONS inside one quarter turn
static void ao_rotation_cs(uint32_t r, float *c, float *s) {
    const double a = (M_PI / 2.0) * r / RT_AO_ROTATIONS;
    *c = static_cast<float>(std::cos(a)); *s = static_cast<float>(std::sin(a));
}

extern "C" rt_status rt_ao_rotation(uint32_t seed, uint32_t i, int32_t *r, float *c, float *s) {
    if (!r || !c || !s) return RT_ERR_INVALID;
    const uint32_t step = ao_hash(seed, i) >> 26;
    *r = static_cast<int32_t>(step);
    ao_rotation_cs(step, c, s);
    return RT_OK;
}

// the device tables, uploaded once per context (this allocates and copies synchronously; nothing on a stream reads them before the call
// that asked for them is enqueued)
static rt_status ensure_ao_tables(rt_ctx *c) {
    if (c->d_ao_tab) return RT_OK;
    std::vector<float> h(kAoTableFloats);
    for (int m = 1; m <= RT_AO_MAX_GRID; ++m) (void)rt_ao_directions(m, h.data() + static_cast<size_t>(ao_dir_offset(m)) * 3);
    for (uint32_t r = 0; r < RT_AO_ROTATIONS; ++r) ao_rotation_cs(r, &h[kAoDirEntries * 3u + r * 2u], &h[kAoDirEntries * 3u + r * 2u + 1u]);
    HIPCHK(c, c->d_ao_tab.grow(h.size()));
    const hipError_t e = hipMemcpy(c->d_ao_tab, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { c->d_ao_tab.release(); c->err = std::string("ambient occlusion table upload: ") + hipGetErrorString(e); return RT_ERR_HIP; }
    return RT_OK;
}

extern "C" rt_status rt_ambient_occlusion_device(rt_ctx *c, int32_t n, const float *d_point, const float *d_normal, int32_t m, float radius,
                                                 uint32_t seed, uint16_t *d_open, float *d_ao, void *stream) {
    rt_status s = query_entry(c, "rt_ambient_occlusion_device", ao_args(n, d_point, d_normal, m, radius, d_open, d_ao));
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if ((s = ensure_ao_tables(c)) != RT_OK) return s;
    const float *tab = c->d_ao_tab;
    const AoLayout lay = ao_layout(m);
    launch_occlusion(ao_grid(ao_units(n, lay), c->cus, lay.rounds), stream_or_own(c, stream), c->S, n, d_point, d_normal,
                     tab + static_cast<size_t>(ao_dir_offset(m)) * 3, tab + kAoDirEntries * 3u, m, radius, seed, d_open, d_ao);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_ambient_occlusion(rt_ctx *c, int32_t n, const float *point, const float *normal, int32_t m, float radius, uint32_t seed,
                                          uint16_t *open, float *ao) {
    const rt_status s = query_entry(c, "rt_ambient_occlusion", ao_args(n, point, normal, m, radius, open, ao));
    if (s != RT_OK || n == 0) return s;
    Staging g(c);
    const size_t pts = static_cast<size_t>(n);
    const float *d_point = g.in(point, pts * 3), *d_normal = g.in(normal, pts * 3);
    uint16_t *d_open = g.out(open, pts);
    float *d_ao = g.out(ao, pts);
    return g.finish([&] { return rt_ambient_occlusion_device(c, n, d_point, d_normal, m, radius, seed, d_open, d_ao, nullptr); });
}

// ---- closest points (Closest points) ------------------------------------------------------------------------------------
extern "C" rt_status rt_closest_point_triangle(const float p[3], const float tri[9], float q[3], float *d2) {
    if (!p || !tri || (!q && !d2)) return RT_ERR_INVALID;
    const NearClosest r = near_point_triangle(p[0], p[1], p[2], tri[0], tri[1], tri[2], tri[3], tri[4], tri[5], tri[6], tri[7], tri[8]);
    if (q) { q[0] = r.qx; q[1] = r.qy; q[2] = r.qz; }
    if (d2) *d2 = r.d2;
    return RT_OK;
}

// The query's bounds, once per uploaded scene (free_scene drops them): the records, the chunks' and the leaves' boxes by two kernels on the context's
// stream, then -- synchronously, before the call that asked for them is enqueued -- one download of the node boxes, the bottom-up pass on
// the host (children follow their parents: one sweep) and their upload.
static rt_status ensure_near_bounds(rt_ctx *c) {
    if (c->near_ready) return RT_OK;
    HIPCHK(c, c->d_near_tris.grow(c->n_face_refs ? c->n_face_refs : 1u));
    HIPCHK(c, c->d_near_nodes.grow(c->S.n_nodes));
    HIPCHK(c, c->d_near_chunks.grow(c->n_chunks ? c->n_chunks : 1u));
    launch_near_bounds(c->stream, c->S, c->n_face_refs, c->n_chunks, c->cus, c->d_near_tris, c->d_near_nodes, c->d_near_chunks);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<NearNode> h(c->S.n_nodes);
    HIPCHK(c, hipMemcpy(h.data(), c->d_near_nodes, h.size() * sizeof(NearNode), hipMemcpyDeviceToHost));
    if (!near_sweep_nodes(h.data(), c->S.n_nodes)) { c->err = "closest points: a child node does not follow its parent"; return RT_ERR_INVALID; }
    HIPCHK(c, hipMemcpy(c->d_near_nodes, h.data(), h.size() * sizeof(NearNode), hipMemcpyHostToDevice));
    c->near_ready = true;
    return RT_OK;
}

extern "C" rt_status rt_closest_points_device(rt_ctx *c, int32_t n, const float *d_point_in, float max_dist, int32_t *d_face, float *d_dist2,
                                              float *d_point, void *stream) {
    rt_status s = query_entry(c, "rt_closest_points_device", near_args(n, d_point_in, max_dist, d_face, d_dist2, d_point));
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if ((s = ensure_near_bounds(c)) != RT_OK) return s;
    launch_nearest(query_grid(n, c->cus), stream_or_own(c, stream), c->S, c->d_near_nodes, c->d_near_tris, c->d_near_chunks, n, d_point_in,
                   max_dist * max_dist, d_face, d_dist2, d_point);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_closest_points(rt_ctx *c, int32_t n, const float *point, float max_dist, int32_t *face, float *dist2, float *closest) {
    const rt_status s = query_entry(c, "rt_closest_points", near_args(n, point, max_dist, face, dist2, closest));
    if (s != RT_OK || n == 0) return s;
    Staging g(c);
    const size_t pts = static_cast<size_t>(n);
    const float *d_in = g.in(point, pts * 3);
    int32_t *d_face = g.out(face, pts);
    float *d_dist2 = g.out(dist2, pts);
    float *d_closest = g.out(closest, pts * 3);
    return g.finish([&] { return rt_closest_points_device(c, n, d_in, max_dist, d_face, d_dist2, d_closest, nullptr); });
}

extern "C" rt_status rt_hit_points_device(rt_ctx *c, int32_t n, const float *d_origin, const float *d_dir, const int32_t *d_face, const float *d_t,
                                          float *d_point, float *d_normal, void *stream) {
    const rt_status s = query_entry(c, "rt_hit_points_device", ao_hit_points_args(n, d_origin, d_dir, d_face, d_t, d_point, d_normal));
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    launch_hit_points(stream_or_own(c, stream), c->S, n, d_origin, d_dir, d_face, d_t, d_point, d_normal);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

// ---- soft shadows (Soft shadows): the definition's host half and the two calls ---------------------------------------------
static_assert(RT_MAX_LIGHTS == kShadowMaxLights && RT_MAX_SAMPLES == kShadowMaxSamples && RT_LIGHT_POINT == kShadowPoint && RT_LIGHT_AREA == kShadowArea &&
                  RT_LIGHT_SPHERE == kShadowSphere,
              "rt_shadow_layout.hpp restates the header's constants");

extern "C" void rt_default_shadow_params(rt_shadow_params *sp) {
    if (!sp) return;
    sp->per_point = 0; sp->seed = 0u; sp->fu = 0.5f; sp->fv = 0.5f;
}

extern "C" rt_status rt_shadow_jitter(uint32_t seed, uint32_t i, float *fu, float *fv) {
    if (!fu || !fv) return RT_ERR_INVALID;
    shadow_jitter(seed, i, *fu, *fv);
    return RT_OK;
}

// the host twin of light_grid / grid_sample (rt_kernels.hip): one float32 operation per line of the header's definition, in its order
extern "C" rt_status rt_light_samples(const rt_lights *l, int32_t light, float fu, float fv, float *out) {
    if (!l || !out || shadow_light_args(l->n_lights, l->mode, l->usteps, l->vsteps) != nullptr || light < 0 || light >= l->n_lights) return RT_ERR_INVALID;
    if (l->mode == RT_LIGHT_SPHERE) return RT_ERR_UNSUPPORTED;
    const float *c = l->pos[light];
    if (l->mode == RT_LIGHT_POINT) { out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; return RT_OK; }
    const float ux = c[0] + l->len_x * 1.0f, vy = c[1] + l->len_y * 1.0f;
    const float cx = ux / static_cast<float>(l->usteps), cy = vy / static_cast<float>(l->vsteps);
    const float z = c[2] + l->len_x * 0.0f;
    for (int32_t i = 0; i < l->usteps; ++i) {
        const float fi = static_cast<float>(i) + fu;
        for (int32_t j = 0; j < l->vsteps; ++j) {
            const float fj = static_cast<float>(j) + fv;
            float *s = out + (static_cast<size_t>(i) * static_cast<size_t>(l->vsteps) + static_cast<size_t>(j)) * 3;
            s[0] = fi * cx; s[1] = fj * cy; s[2] = z;
        }
    }
    return RT_OK;
}

// what both calls check, in the order the header gives: context, scene, arguments, then the lights (sphere mode before check_lights, whose
// sphere branch waits for the frames and uploads)
static rt_status shadow_entry(rt_ctx *c, const char *who, const rt_lights *l, int32_t n, const void *point, const void *normal, const rt_shadow_params *sp,
                              const void *visible, const void *share, DLights *L) {
    const rt_status s = query_entry(c, who, !l ? "lights is null"
                                               : shadow_args(n, point, normal, sp != nullptr, sp ? sp->per_point : 0, sp ? sp->fu : 0.0f, sp ? sp->fv : 0.0f, visible, share));
    if (s != RT_OK) return s;
    if (const char *bad = shadow_light_args(l->n_lights, l->mode, l->usteps, l->vsteps)) { c->err = std::string(who) + ": lights: " + bad; return RT_ERR_INVALID; }
    if (l->mode == RT_LIGHT_SPHERE) { c->err = std::string(who) + ": sphere lights are not supported (their offsets need a synchronous upload)"; return RT_ERR_UNSUPPORTED; }
    return check_lights(c, l, L);
}

extern "C" rt_status rt_soft_shadows_device(rt_ctx *c, const rt_lights *lights, int32_t n, const float *d_point, const float *d_normal,
                                            const rt_shadow_params *sp, uint16_t *d_visible, float *d_share, void *stream) {
    DLights L;
    const rt_status s = shadow_entry(c, "rt_soft_shadows_device", lights, n, d_point, d_normal, sp, d_visible, d_share, &L);
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    const AoLayout lay = shadow_layout(L.n_lights, L.usteps, L.vsteps).A;
    launch_soft_shadows(shadow_grid(ao_units(n, lay), c->cus, lay.rounds), stream_or_own(c, stream), c->S, L, n, d_point, d_normal, sp->per_point != 0 ? 1 : 0, sp->seed,
                        sp->fu, sp->fv, d_visible, d_share);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_soft_shadows(rt_ctx *c, const rt_lights *lights, int32_t n, const float *point, const float *normal, const rt_shadow_params *sp,
                                     uint16_t *visible, float *share) {
    DLights L;
    const rt_status s = shadow_entry(c, "rt_soft_shadows", lights, n, point, normal, sp, visible, share, &L);
    if (s != RT_OK || n == 0) return s;
    Staging g(c);
    const size_t pts = static_cast<size_t>(n);
    const float *d_point = g.in(point, pts * 3), *d_normal = normal ? g.in(normal, pts * 3) : nullptr;
    uint16_t *d_visible = g.out(visible, pts);
    float *d_share = g.out(share, pts);
    return g.finish([&] { return rt_soft_shadows_device(c, lights, n, d_point, d_normal, sp, d_visible, d_share, nullptr); });
}

// ---- one-bounce diffuse gather (Indirect diffuse) --------------------------------------------------------------------------
// what both calls check, in the order the header gives: context, scene, arguments, then the lights (sphere mode before check_lights, whose
// sphere branch waits for the frames and uploads)
static rt_status gather_entry(rt_ctx *c, const char *who, const rt_lights *l, int32_t n, const void *point, const void *normal, int32_t m, const void *rgb, DLights *L) {
    const rt_status s = query_entry(c, who, !l ? "lights is null" : gather_args(n, point, normal, m, rgb));
    if (s != RT_OK) return s;
    if (const char *bad = shadow_light_args(l->n_lights, l->mode, l->usteps, l->vsteps)) { c->err = std::string(who) + ": lights: " + bad; return RT_ERR_INVALID; }
    if (l->mode == RT_LIGHT_SPHERE) { c->err = std::string(who) + ": sphere lights are not supported (their offsets need a synchronous upload)"; return RT_ERR_UNSUPPORTED; }
    return check_lights(c, l, L);
}

extern "C" rt_status rt_indirect_diffuse_device(rt_ctx *c, const rt_lights *lights, int32_t n, const float *d_point, const float *d_normal, int32_t m,
                                                uint32_t seed, float *d_rgb, void *stream) {
    DLights L;
    rt_status s = gather_entry(c, "rt_indirect_diffuse_device", lights, n, d_point, d_normal, m, d_rgb, &L);
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if ((s = ensure_ao_tables(c)) != RT_OK) return s;          // (the table set of the ambient-occlusion call: one copy per context)
    const float *tab = c->d_ao_tab;
    const AoLayout lay = ao_layout(m);
    launch_gather(ao_grid(ao_units(n, lay), c->cus, lay.rounds), stream_or_own(c, stream), c->S, L, n, d_point, d_normal,
                  tab + static_cast<size_t>(ao_dir_offset(m)) * 3, tab + kAoDirEntries * 3u, m, seed, d_rgb);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_indirect_diffuse(rt_ctx *c, const rt_lights *lights, int32_t n, const float *point, const float *normal, int32_t m, uint32_t seed,
                                         float *rgb) {
    DLights L;
    const rt_status s = gather_entry(c, "rt_indirect_diffuse", lights, n, point, normal, m, rgb, &L);
    if (s != RT_OK || n == 0) return s;
    Staging g(c);
    const size_t pts = static_cast<size_t>(n);
    const float *d_point = g.in(point, pts * 3), *d_normal = g.in(normal, pts * 3);
    float *d_rgb = g.out(rgb, pts * 3);
    return g.finish([&] { return rt_indirect_diffuse_device(c, lights, n, d_point, d_normal, m, seed, d_rgb, nullptr); });
}

// ---- light probes (Light probes): the definition's host half and the four calls ---------------------------------------------
static_assert(RT_PROBE_COEFFS == kProbeCoeffs && sizeof(rt_probe_grid) == sizeof(ProbeGrid), "rt_probe_layout.hpp restates the header's constants");

extern "C" rt_status rt_probe_directions(int32_t m, float *out) {
    if (!ao_grid_ok(m) || !out) return RT_ERR_INVALID;
    for (int k = 0; k < m * m; ++k) {
        const double x = (k % m + 0.5) / m, y = (k / m + 0.5) / m;
        const double z = 1.0 - 2.0 * y, rr = 1.0 - z * z, r = std::sqrt(rr > 0.0 ? rr : 0.0), phi = 2.0 * M_PI * x;
        out[k * 3] = static_cast<float>(r * std::cos(phi)); out[k * 3 + 1] = static_cast<float>(r * std::sin(phi)); out[k * 3 + 2] = static_cast<float>(z);
    }
    return RT_OK;
}

extern "C" rt_status rt_probe_weights(int32_t m, float *out) {
    if (!ao_grid_ok(m) || !out) return RT_ERR_INVALID;
    const int K = m * m;
    std::vector<float> d(static_cast<size_t>(K) * 3);
    (void)rt_probe_directions(m, d.data());
    const double s1 = std::sqrt(3.0 / (4.0 * M_PI)), s2 = 0.5 * std::sqrt(15.0 / M_PI), s6 = 0.25 * std::sqrt(5.0 / M_PI), s8 = 0.25 * std::sqrt(15.0 / M_PI);
    const double a1 = 2.0 / 3.0, a2 = 1.0 / 4.0, solid = 4.0 * M_PI / K;
    for (int k = 0; k < K; ++k) {
        const double x = d[k * 3], y = d[k * 3 + 1], z = d[k * 3 + 2];
        const double Y[9] = {0.5 * std::sqrt(1.0 / M_PI), s1 * y, s1 * z, s1 * x, s2 * x * y, s2 * y * z, s6 * (3.0 * z * z - 1.0), s2 * x * z, s8 * (x * x - y * y)};
        const double a[9] = {1.0, a1, a1, a1, a2, a2, a2, a2, a2};
        for (int j = 0; j < 9; ++j) out[k * 9 + j] = static_cast<float>(solid * a[j] * Y[j]);
    }
    return RT_OK;
}

extern "C" rt_status rt_sh9(const float n[3], float out[9]) {
    if (!n || !out) return RT_ERR_INVALID;
    probe_sh9(n[0], n[1], n[2], out);
    return RT_OK;
}

static ProbeGrid probe_grid_of(const rt_probe_grid *g) {
    ProbeGrid G;
    for (int q = 0; q < 3; ++q) { G.origin[q] = g->origin[q]; G.step[q] = g->step[q]; G.dims[q] = g->dims[q]; }
    return G;
}

extern "C" rt_status rt_probe_grid_positions(const rt_probe_grid *grid, float *out) {
    if (!grid || !out) return RT_ERR_INVALID;
    const ProbeGrid G = probe_grid_of(grid);
    if (probe_grid_bad(G)) return RT_ERR_INVALID;
    for (int32_t iz = 0; iz < G.dims[2]; ++iz)
        for (int32_t iy = 0; iy < G.dims[1]; ++iy)
            for (int32_t ix = 0; ix < G.dims[0]; ++ix) {
                float *o = out + static_cast<size_t>(probe_index(G, ix, iy, iz)) * 3;
                o[0] = probe_position(G, 0, ix); o[1] = probe_position(G, 1, iy); o[2] = probe_position(G, 2, iz);
            }
    return RT_OK;
}

// the device tables, uploaded once per context (as ensure_ao_tables: synchronously, before the call that asked for them is enqueued)
static rt_status ensure_probe_tables(rt_ctx *c) {
    if (c->d_probe_tab) return RT_OK;
    std::vector<float> h(kProbeTableFloats);
    for (int m = 1; m <= RT_AO_MAX_GRID; ++m) {
        (void)rt_probe_directions(m, h.data() + probe_dir_offset(m));
        (void)rt_probe_weights(m, h.data() + probe_weight_offset(m));
    }
    HIPCHK(c, c->d_probe_tab.grow(h.size()));
    const hipError_t e = hipMemcpy(c->d_probe_tab, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { c->d_probe_tab.release(); c->err = std::string("light probe table upload: ") + hipGetErrorString(e); return RT_ERR_HIP; }
    return RT_OK;
}

// what both probe calls check, in the order of gather_entry
static rt_status probes_entry(rt_ctx *c, const char *who, const rt_lights *l, int32_t n, const void *position, int32_t m, const void *coeff, DLights *L) {
    const rt_status s = query_entry(c, who, !l ? "lights is null" : probe_args(n, position, m, coeff));
    if (s != RT_OK) return s;
    if (const char *bad = shadow_light_args(l->n_lights, l->mode, l->usteps, l->vsteps)) { c->err = std::string(who) + ": lights: " + bad; return RT_ERR_INVALID; }
    if (l->mode == RT_LIGHT_SPHERE) { c->err = std::string(who) + ": sphere lights are not supported (their offsets need a synchronous upload)"; return RT_ERR_UNSUPPORTED; }
    return check_lights(c, l, L);
}

extern "C" rt_status rt_light_probes_device(rt_ctx *c, const rt_lights *lights, int32_t n, const float *d_position, int32_t m, int32_t direct, float *d_coeff,
                                            void *stream) {
    DLights L;
    rt_status s = probes_entry(c, "rt_light_probes_device", lights, n, d_position, m, d_coeff, &L);
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if ((s = ensure_probe_tables(c)) != RT_OK) return s;
    const float *tab = c->d_probe_tab;
    const AoLayout lay = ao_layout(m);
    launch_probes(ao_grid(ao_units(n, lay), c->cus, lay.rounds), stream_or_own(c, stream), c->S, L, n, d_position, tab + probe_dir_offset(m),
                  tab + probe_weight_offset(m), m, direct != 0 ? 1 : 0, d_coeff);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_light_probes(rt_ctx *c, const rt_lights *lights, int32_t n, const float *position, int32_t m, int32_t direct, float *coeff) {
    DLights L;
    const rt_status s = probes_entry(c, "rt_light_probes", lights, n, position, m, coeff, &L);
    if (s != RT_OK || n == 0) return s;
    Staging g(c);
    const size_t pts = static_cast<size_t>(n);
    const float *d_position = g.in(position, pts * 3);
    float *d_coeff = g.out(coeff, pts * kProbeCoeffs);
    return g.finish([&] { return rt_light_probes_device(c, lights, n, d_position, m, direct, d_coeff, nullptr); });
}

// (no scene is needed: the lookup reads the caller's arrays alone)
static rt_status lookup_entry(rt_ctx *c, const char *who, const rt_probe_grid *grid, const void *coeff, int32_t n, const void *point, const void *normal,
                              const void *rgb, ProbeGrid *G) {
    if (!c) return RT_ERR_INVALID;
    if (grid) *G = probe_grid_of(grid);
    if (const char *bad = probe_lookup_args(grid ? G : nullptr, coeff, n, point, normal, rgb)) { c->err = std::string(who) + ": " + bad; return RT_ERR_INVALID; }
    return RT_OK;
}

extern "C" rt_status rt_probe_irradiance_device(rt_ctx *c, const rt_probe_grid *grid, const float *d_coeff, int32_t n, const float *d_point,
                                                const float *d_normal, float *d_rgb, void *stream) {
    ProbeGrid G;
    const rt_status s = lookup_entry(c, "rt_probe_irradiance_device", grid, d_coeff, n, d_point, d_normal, d_rgb, &G);
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    launch_probe_lookup(query_grid(n, c->cus), stream_or_own(c, stream), G, d_coeff, n, d_point, d_normal, d_rgb);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_probe_irradiance(rt_ctx *c, const rt_probe_grid *grid, const float *coeff, int32_t n, const float *point, const float *normal,
                                         float *rgb) {
    ProbeGrid G;
    const rt_status s = lookup_entry(c, "rt_probe_irradiance", grid, coeff, n, point, normal, rgb, &G);
    if (s != RT_OK || n == 0) return s;
    Staging g(c);
    const size_t pts = static_cast<size_t>(n);
    const float *d_coeff = g.in(coeff, static_cast<size_t>(probe_cells(G)) * kProbeCoeffs), *d_point = g.in(point, pts * 3), *d_normal = g.in(normal, pts * 3);
    float *d_rgb = g.out(rgb, pts * 3);
    return g.finish([&] { return rt_probe_irradiance_device(c, grid, d_coeff, n, d_point, d_normal, d_rgb, nullptr); });
}

// ---- the leak-free lookup (Leak-free probe lookup): this one walks segments, so it needs the scene
static rt_status visible_entry(rt_ctx *c, const char *who, const rt_probe_grid *grid, const void *coeff, int32_t n, const void *point, const void *normal,
                               const void *rgb, const void *mask, ProbeGrid *G) {
    if (!c) return RT_ERR_INVALID;
    if (grid) *G = probe_grid_of(grid);
    return query_entry(c, who, probe_visible_args(grid ? G : nullptr, coeff, n, point, normal, rgb, mask));
}

extern "C" rt_status rt_probe_irradiance_visible_device(rt_ctx *c, const rt_probe_grid *grid, const float *d_coeff, int32_t n, const float *d_point,
                                                        const float *d_normal, float *d_rgb, uint8_t *d_mask, void *stream) {
    ProbeGrid G;
    const rt_status s = visible_entry(c, "rt_probe_irradiance_visible_device", grid, d_coeff, n, d_point, d_normal, d_rgb, d_mask, &G);
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    launch_probe_lookup_visible(pv_grid(n, c->cus), stream_or_own(c, stream), c->S, G, d_coeff, n, d_point, d_normal, d_rgb, d_mask);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_probe_irradiance_visible(rt_ctx *c, const rt_probe_grid *grid, const float *coeff, int32_t n, const float *point, const float *normal,
                                                 float *rgb, uint8_t *mask) {
    ProbeGrid G;
    const rt_status s = visible_entry(c, "rt_probe_irradiance_visible", grid, coeff, n, point, normal, rgb, mask, &G);
    if (s != RT_OK || n == 0) return s;
    Staging g(c);
    const size_t pts = static_cast<size_t>(n);
    const float *d_coeff = g.in(coeff, static_cast<size_t>(probe_cells(G)) * kProbeCoeffs), *d_point = g.in(point, pts * 3), *d_normal = g.in(normal, pts * 3);
    float *d_rgb = g.out(rgb, pts * 3);
    uint8_t *d_mask = g.out(mask, pts);
    return g.finish([&] { return rt_probe_irradiance_visible_device(c, grid, d_coeff, n, d_point, d_normal, d_rgb, d_mask, nullptr); });
}

// ---- bounced light (Bounced light): the parents' calls with a source volume looked up at every hit
// the parent's checks, then the source's (probe_source_args); out_floats: the floats of the output per element
static rt_status source_entry(rt_ctx *c, const char *who, rt_status parent, const rt_probe_grid *src_grid, const void *src_coeff, int32_t n, const void *out,
                              size_t out_floats, ProbeGrid *G) {
    if (parent != RT_OK) return parent;
    if (src_grid) *G = probe_grid_of(src_grid);
    if (const char *bad = probe_source_args(src_grid ? G : nullptr, src_coeff, n, out, static_cast<size_t>(n) * out_floats * sizeof(float))) {
        c->err = std::string(who) + ": " + bad;
        return RT_ERR_INVALID;
    }
    return RT_OK;
}

extern "C" rt_status rt_light_probes_bounce_device(rt_ctx *c, const rt_lights *lights, int32_t n, const float *d_position, int32_t m, int32_t direct,
                                                   const rt_probe_grid *src_grid, const float *d_src_coeff, int32_t visible, float *d_coeff, void *stream) {
    DLights L;
    ProbeGrid G;
    const char *who = "rt_light_probes_bounce_device";
    rt_status s = source_entry(c, who, probes_entry(c, who, lights, n, d_position, m, d_coeff, &L), src_grid, d_src_coeff, n, d_coeff, kProbeCoeffs, &G);
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if ((s = ensure_probe_tables(c)) != RT_OK) return s;
    const float *tab = c->d_probe_tab;
    const AoLayout lay = ao_layout(m);
    launch_probes_bounce(ao_grid(ao_units(n, lay), c->cus, lay.rounds), stream_or_own(c, stream), c->S, L, n, d_position, tab + probe_dir_offset(m),
                         tab + probe_weight_offset(m), m, direct != 0 ? 1 : 0, G, d_src_coeff, visible != 0, d_coeff);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_light_probes_bounce(rt_ctx *c, const rt_lights *lights, int32_t n, const float *position, int32_t m, int32_t direct,
                                            const rt_probe_grid *src_grid, const float *src_coeff, int32_t visible, float *coeff) {
    DLights L;
    ProbeGrid G;
    const char *who = "rt_light_probes_bounce";
    const rt_status s = source_entry(c, who, probes_entry(c, who, lights, n, position, m, coeff, &L), src_grid, src_coeff, n, coeff, kProbeCoeffs, &G);
    if (s != RT_OK || n == 0) return s;
    Staging g(c);
    const size_t pts = static_cast<size_t>(n);
    const float *d_position = g.in(position, pts * 3), *d_src = g.in(src_coeff, static_cast<size_t>(probe_cells(G)) * kProbeCoeffs);
    float *d_coeff = g.out(coeff, pts * kProbeCoeffs);
    return g.finish([&] { return rt_light_probes_bounce_device(c, lights, n, d_position, m, direct, src_grid, d_src, visible, d_coeff, nullptr); });
}

extern "C" rt_status rt_indirect_diffuse_bounce_device(rt_ctx *c, const rt_lights *lights, int32_t n, const float *d_point, const float *d_normal, int32_t m,
                                                       uint32_t seed, const rt_probe_grid *src_grid, const float *d_src_coeff, int32_t visible, float *d_rgb,
                                                       void *stream) {
    DLights L;
    ProbeGrid G;
    const char *who = "rt_indirect_diffuse_bounce_device";
    rt_status s = source_entry(c, who, gather_entry(c, who, lights, n, d_point, d_normal, m, d_rgb, &L), src_grid, d_src_coeff, n, d_rgb, 3, &G);
    if (s != RT_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if ((s = ensure_ao_tables(c)) != RT_OK) return s;
    const float *tab = c->d_ao_tab;
    const AoLayout lay = ao_layout(m);
    launch_gather_bounce(ao_grid(ao_units(n, lay), c->cus, lay.rounds), stream_or_own(c, stream), c->S, L, n, d_point, d_normal,
                         tab + static_cast<size_t>(ao_dir_offset(m)) * 3, tab + kAoDirEntries * 3u, m, seed, G, d_src_coeff, visible != 0, d_rgb);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_indirect_diffuse_bounce(rt_ctx *c, const rt_lights *lights, int32_t n, const float *point, const float *normal, int32_t m, uint32_t seed,
                                                const rt_probe_grid *src_grid, const float *src_coeff, int32_t visible, float *rgb) {
    DLights L;
    ProbeGrid G;
    const char *who = "rt_indirect_diffuse_bounce";
    const rt_status s = source_entry(c, who, gather_entry(c, who, lights, n, point, normal, m, rgb, &L), src_grid, src_coeff, n, rgb, 3, &G);
    if (s != RT_OK || n == 0) return s;
    Staging g(c);
    const size_t pts = static_cast<size_t>(n);
    const float *d_point = g.in(point, pts * 3), *d_normal = g.in(normal, pts * 3), *d_src = g.in(src_coeff, static_cast<size_t>(probe_cells(G)) * kProbeCoeffs);
    float *d_rgb = g.out(rgb, pts * 3);
    return g.finish([&] { return rt_indirect_diffuse_bounce_device(c, lights, n, d_point, d_normal, m, seed, src_grid, d_src, visible, d_rgb, nullptr); });
}

// ---- geometry buffers as a query (Geometry buffers as a query) ----------------------------------------------------------
static_assert(RT_GBUFFER_CHANNELS == kGbChannels && RT_MAX_SUPERSAMPLING == kGbMaxSupersampling && RT_MAX_PASSES == kGbMaxPasses,
              "rt_gbuffer_layout.hpp restates the header's constants");

// the pass table, uploaded once per context (this allocates and copies synchronously; nothing on a stream reads it before the call that
// asked for it is enqueued): rt_pass_offsets itself, so that every pass has the offsets its frame has
static rt_status ensure_gb_pass_table(rt_ctx *c) {
    if (c->d_gb_pass) return RT_OK;
    std::vector<float> h(kGbPassTabFloats, 0.0f);
    for (int n = 1; n <= RT_MAX_SUPERSAMPLING; ++n)
        for (int p = 0; p < RT_MAX_PASSES; ++p) (void)rt_pass_offsets(n, p, &h[gb_pass_entry(n, p)], &h[gb_pass_entry(n, p) + RT_MAX_SUPERSAMPLING]);
    HIPCHK(c, c->d_gb_pass.grow(h.size()));
    const hipError_t e = hipMemcpy(c->d_gb_pass, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { c->d_gb_pass.release(); c->err = std::string("geometry buffer pass table upload: ") + hipGetErrorString(e); return RT_ERR_HIP; }
    return RT_OK;
}

// The checks of both calls and what the kernel takes by value, before anything is allocated or enqueued.  G.F becomes the OUTPUT frame of the
// call -- its width, rows and row shard, for the tiles and frame_row -- with the sample settings a frame on this context would have (n,
// lens, shutter; make_frame, apply_lens and apply_shutter as the frames call them).  rows == 0: nothing to do.
struct GbufferPlan {
    DFrame F;
    DCam cam;
    DShutter sh;
    int32_t rows = 0;
};
static rt_status gbuffer_plan(rt_ctx *c, const char *who, const rt_camera *cam, const rt_params *p, const char *bad, GbufferPlan *G) {
    rt_status s = query_entry(c, who, bad);
    if (s != RT_OK) return s;
    const SampleSettings &m = c->smp;
    if ((s = make_frame(c, p, &G->F)) != RT_OK) { c->err = std::string(who) + ": " + c->err; return s; }
    if (m.converge_on()) {
        c->err = std::string(who) + ": adaptive pass counts are on (rt_set_pass_tolerance): an inactive pixel forms no ray, so its buffers are not defined";
        return RT_ERR_INVALID;
    }
    if (m.shutter_on && !shutter_compatible(cam, &m.shutter_close)) { c->err = std::string(who) + ": " + k_shutter_mismatch; return RT_ERR_INVALID; }
    G->rows = rt_local_rows(p);
    if (G->rows == 0) return RT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if ((s = apply_lens(c, &G->F)) != RT_OK) return s;
    apply_shutter(c, &G->F);
    if ((s = ensure_gb_pass_table(c)) != RT_OK) return s;
    DFrame &F = G->F;
    F.width = p->width; F.height = p->height; F.local_rows = G->rows;
    F.row0 = p->row0; F.stripe = p->stripe;
    F.tiles_x = (F.width + 7) / 8; F.tiles_y = (F.local_rows + 7) / 8;
    F.npix = static_cast<uint32_t>(F.local_rows) * static_cast<uint32_t>(F.width);
    make_cam(cam, &G->cam);
    std::memset(&G->sh, 0, sizeof G->sh);
    if (m.shutter_on) make_shutter(cam, &m.shutter_close, &G->sh);
    return RT_OK;
}

// the one kernel of a planned call (rows > 0) on `st`
static rt_status gbuffer_launch(rt_ctx *c, const GbufferPlan &G, float *d_out, hipStream_t st) {
    const GbTiles T = gb_tiles(G.F.width, G.F.local_rows);
    launch_gbuffer(gb_grid(T.tiles, c->cus), st, c->S, G.cam, G.sh, G.F, c->d_gb_pass, c->smp.pass_first, c->smp.pass_count, d_out);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_gbuffer_device(rt_ctx *c, const rt_camera *cam, const rt_params *p, float *d_out, void *stream) {
    GbufferPlan G;
    const rt_status s = gbuffer_plan(c, "rt_gbuffer_device", cam, p, gb_args(cam, p, d_out), &G);
    if (s != RT_OK || G.rows == 0) return s;
    return gbuffer_launch(c, G, d_out, stream_or_own(c, stream));
}

extern "C" rt_status rt_gbuffer(rt_ctx *c, const rt_camera *cam, const rt_params *p, float *out) {
    GbufferPlan G;
    const rt_status s = gbuffer_plan(c, "rt_gbuffer", cam, p, (!cam || !p || !out) ? "a pointer is null" : nullptr, &G);
    if (s != RT_OK || G.rows == 0) return s;
    Staging g(c);
    float *d_out = g.out(out, static_cast<size_t>(gb_out_floats(G.F.width, G.rows)));
    return g.finish([&] { return gbuffer_launch(c, G, d_out, c->stream); });          // (the plan is this call's: rt_gbuffer_device would plan again)
}

// ---- denoising (Denoising): the a-trous filter of rt_denoise.hip on an image and its geometry buffers --------------------------
static_assert(RT_DENOISE_MAX_ITERATIONS == kDnMaxIterations && RT_GBUFFER_CHANNELS == kDnGbChannels, "rt_denoise_layout.hpp restates the header's constants");
static_assert(sizeof(rt_denoise_params) == 20, "rt_denoise_params is five 32-bit words");
// Which iterations k (bit k) take the LDS-staged kernel where it exists (steps 1 and 2).  Measured and rejected (Denoising):
// the product stages none; an A/B build (make ab AB_FLAGS=-DRT_DENOISE_STAGED_STEPS=3) stages them for the comparison.
#ifdef RT_DENOISE_STAGED_STEPS
constexpr uint32_t kDenoiseStagedSteps = RT_DENOISE_STAGED_STEPS;
#else
constexpr uint32_t kDenoiseStagedSteps = 0u;
#endif

extern "C" void rt_default_denoise_params(rt_denoise_params *dp) {
    if (!dp) return;
    dp->iterations = 5;
    dp->sigma_color = 1.0f; dp->sigma_normal = 0.5f; dp->sigma_depth = 0.125f; dp->sigma_albedo = 0.25f;
}

extern "C" size_t rt_denoise_scratch_bytes(int32_t width, int32_t rows, int32_t channels) { return dn_scratch_bytes(width, rows, channels); }

// what both calls check first: everything but the context is decided by rt_denoise_layout.hpp
static rt_status denoise_entry(rt_ctx *c, const char *who, const float *in, int32_t channels, const float *gbuffer, int32_t width, int32_t rows,
                               const rt_denoise_params *dp, const void *scratch, const float *out, bool device) {
    if (!c) return RT_ERR_INVALID;
    bool unsupported = false;
    const char *bad = dn_args(in, channels, gbuffer, width, rows, dp ? &dp->iterations : nullptr, dp ? &dp->sigma_color : nullptr, scratch, out, device, &unsupported);
    if (bad) { c->err = std::string(who) + ": " + bad; return unsupported ? RT_ERR_UNSUPPORTED : RT_ERR_INVALID; }
    return RT_OK;
}

extern "C" rt_status rt_denoise_device(rt_ctx *c, const float *d_in, int32_t channels, const float *d_gbuffer, int32_t width, int32_t rows,
                                       const rt_denoise_params *dp, void *d_scratch, float *d_out, void *stream) {
    const rt_status s = denoise_entry(c, "rt_denoise_device", d_in, channels, d_gbuffer, width, rows, dp, d_scratch, d_out, true);
    if (s != RT_OK || rows == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream_or_own(c, stream);
    const DnLayout lay = dn_layout(width, rows, channels);
    char *base = static_cast<char *>(d_scratch);
    float4 *g0 = reinterpret_cast<float4 *>(base + lay.guide0), *g1 = reinterpret_cast<float4 *>(base + lay.guide1);
    void *work[2] = {base + lay.work0, base + lay.work1};
    const uint64_t pixels = dn_pixels(width, rows);
    launch_denoise_guide(dn_guide_grid(pixels, c->cus), st, channels, d_in, d_gbuffer, g0, g1, static_cast<float4 *>(work[0]), pixels);
    // three channels: I_0 is the RGBx copy in work[0], iteration k writes work[(k + 1) & 1]; one channel: I_0 is d_in itself and iteration k
    // writes work[k & 1].  The last iteration writes d_out.
    const int grid = dn_grid(dn_tiles(width, rows).tiles, c->cus);
    const void *src = channels == 3 ? work[0] : static_cast<const void *>(d_in);
    for (int32_t k = 0; k < dp->iterations; ++k) {
        const bool last = k + 1 == dp->iterations;
        void *dst = last ? static_cast<void *>(d_out) : work[channels == 3 ? (k + 1) & 1 : k & 1];
        const bool staged = ((kDenoiseStagedSteps >> k) & 1u) != 0u && denoise_staged_fits(1 << k);
        launch_atrous(grid, st, channels, last, staged, src, g0, g1, dst, width, rows, 1 << k,
                      dn_scales(dp->sigma_color, dp->sigma_normal, dp->sigma_depth, dp->sigma_albedo, k));
        src = dst;
    }
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_denoise(rt_ctx *c, const float *in, int32_t channels, const float *gbuffer, int32_t width, int32_t rows,
                                const rt_denoise_params *dp, float *out) {
    const rt_status s = denoise_entry(c, "rt_denoise", in, channels, gbuffer, width, rows, dp, nullptr, out, false);
    if (s != RT_OK || rows == 0) return s;
    Staging g(c);
    const size_t img = static_cast<size_t>(dn_image_bytes(width, rows, channels)) / sizeof(float);
    const float *d_in = g.in(in, img), *d_gb = g.in(gbuffer, static_cast<size_t>(dn_gbuffer_bytes(width, rows)) / sizeof(float));
    float *d_out = g.out(out, img);
    float4 *d_scratch = g.room<float4>(dn_scratch_bytes(width, rows, channels) / sizeof(float4));
    return g.finish([&] { return rt_denoise_device(c, d_in, channels, d_gb, width, rows, dp, d_scratch, d_out, nullptr); });
}

// ---- upsampling (Upsampling): the guided upsample of rt_upsample.hip on a low image and the two sets of geometry buffers -------
static_assert(RT_UPSAMPLE_MAX_FACTOR == kUpMaxFactor, "rt_upsample_layout.hpp restates the header's constant");
static_assert(sizeof(rt_upsample_params) == 16, "rt_upsample_params is four 32-bit words");

extern "C" void rt_default_upsample_params(rt_upsample_params *up) {
    if (!up) return;
    rt_denoise_params dp;
    rt_default_denoise_params(&dp);
    up->factor = 2;
    // the denoiser's depth and albedo scales; its normal scale, 0.5f, stops the taps between the facets of a smooth surface and lost the
    // experiment of DESIGN.md §5, Upsampling, on dodgeColorTest: 2.0f stops opposite normals only and weighs the rest
    up->sigma_normal = 2.0f; up->sigma_depth = dp.sigma_depth; up->sigma_albedo = dp.sigma_albedo;
}

extern "C" rt_status rt_upsample_low_size(int32_t width, int32_t rows, int32_t factor, int32_t *w, int32_t *r) {
    return w && r && up_low_size(width, rows, factor, w, r) ? RT_OK : RT_ERR_INVALID;
}

// what both calls check first: everything but the context is decided by rt_upsample_layout.hpp
static rt_status upsample_entry(rt_ctx *c, const char *who, const float *low, int32_t channels, const float *gb_low, const float *gb_high, int32_t width,
                                int32_t rows, const rt_upsample_params *up, const float *out, const uint8_t *miss, bool device) {
    if (!c) return RT_ERR_INVALID;
    bool unsupported = false;
    const char *bad = up_args(low, channels, gb_low, gb_high, width, rows, up ? &up->factor : nullptr, up ? &up->sigma_normal : nullptr, out, miss, device,
                              &unsupported);
    if (bad) { c->err = std::string(who) + ": " + bad; return unsupported ? RT_ERR_UNSUPPORTED : RT_ERR_INVALID; }
    return RT_OK;
}

extern "C" rt_status rt_upsample_device(rt_ctx *c, const float *d_low, int32_t channels, const float *d_gb_low, const float *d_gb_high, int32_t width,
                                        int32_t rows, const rt_upsample_params *up, float *d_out, uint8_t *d_miss, void *stream) {
    const rt_status s = upsample_entry(c, "rt_upsample_device", d_low, channels, d_gb_low, d_gb_high, width, rows, up, d_out, d_miss, true);
    if (s != RT_OK || rows == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    launch_upsample(dn_grid(dn_tiles(width, rows).tiles, c->cus), stream_or_own(c, stream), channels, d_low, d_gb_low, d_gb_high, d_out, d_miss, width, rows,
                    up->factor, up_scales(up->sigma_normal, up->sigma_depth, up->sigma_albedo, up->factor));
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_upsample(rt_ctx *c, const float *low, int32_t channels, const float *gb_low, const float *gb_high, int32_t width, int32_t rows,
                                 const rt_upsample_params *up, float *out, uint8_t *miss) {
    const rt_status s = upsample_entry(c, "rt_upsample", low, channels, gb_low, gb_high, width, rows, up, out, miss, false);
    if (s != RT_OK || rows == 0) return s;
    const int32_t w = up_low_extent(width, up->factor), r = up_low_extent(rows, up->factor);
    Staging g(c);
    const float *d_low = g.in(low, static_cast<size_t>(dn_image_bytes(w, r, channels)) / sizeof(float));
    const float *d_gl = g.in(gb_low, static_cast<size_t>(dn_gbuffer_bytes(w, r)) / sizeof(float));
    const float *d_gh = g.in(gb_high, static_cast<size_t>(dn_gbuffer_bytes(width, rows)) / sizeof(float));
    float *d_out = g.out(out, static_cast<size_t>(dn_image_bytes(width, rows, channels)) / sizeof(float));
    uint8_t *d_miss = g.out(miss, static_cast<size_t>(up_miss_bytes(width, rows)));
    return g.finish([&] { return rt_upsample_device(c, d_low, channels, d_gl, d_gh, width, rows, up, d_out, d_miss, nullptr); });
}

// ---- temporal reprojection (Temporal reprojection): the kernel of rt_reproject.hip on two frames' images and geometry buffers ---
static_assert(RT_REPROJECT_MAX_HISTORY == kRpMaxHistory, "rt_reproject_layout.hpp restates the header's constant");
static_assert(sizeof(rt_reproject_params) == 16, "rt_reproject_params is four 32-bit words");

extern "C" void rt_default_reproject_params(rt_reproject_params *rp) {
    if (!rp) return;
    rt_upsample_params up;
    rt_default_upsample_params(&up);
    rp->max_history = 32;
    // the upsample's normal and albedo scales; its depth scale, 0.125f, lets history bleed across creases and lost the experiment of DESIGN.md
    // §5, Temporal reprojection, on dodgeColorTest: an eighth of it keeps the taps of the same surface and stops the rest
    rp->sigma_normal = up.sigma_normal; rp->sigma_depth = 0.015625f; rp->sigma_albedo = up.sigma_albedo;
}

extern "C" rt_status rt_reproject_map(const rt_camera *cur, const rt_camera *prev, float *m) {
    if (!cur || !prev || !m) return RT_ERR_INVALID;
    const RpCam a{cur->center, cur->inv_view, cur->fovy, cur->aspect, cur->viewport}, b{prev->center, prev->inv_view, prev->fovy, prev->aspect, prev->viewport};
    return rp_map(a, b, m) ? RT_ERR_INVALID : RT_OK;
}

// what both calls check first: everything but the context is decided by rt_reproject_layout.hpp
static rt_status reproject_entry(rt_ctx *c, const char *who, const float *cur, int32_t channels, const float *gb_cur, const float *hist, const float *gb_hist,
                                 const uint8_t *len_hist, int32_t width, int32_t rows, const float *m, const rt_reproject_params *rp, const float *out,
                                 const uint8_t *len_out, bool device) {
    if (!c) return RT_ERR_INVALID;
    bool unsupported = false;
    const char *bad = rp_args(cur, channels, gb_cur, hist, gb_hist, len_hist, width, rows, m, rp ? &rp->max_history : nullptr, rp ? &rp->sigma_normal : nullptr,
                              out, len_out, device, &unsupported);
    if (bad) { c->err = std::string(who) + ": " + bad; return unsupported ? RT_ERR_UNSUPPORTED : RT_ERR_INVALID; }
    return RT_OK;
}

extern "C" rt_status rt_reproject_device(rt_ctx *c, const float *d_cur, int32_t channels, const float *d_gb_cur, const float *d_hist, const float *d_gb_hist,
                                         const uint8_t *d_len_hist, int32_t width, int32_t rows, const float *m, const rt_reproject_params *rp, float *d_out,
                                         uint8_t *d_len_out, void *stream) {
    const rt_status s = reproject_entry(c, "rt_reproject_device", d_cur, channels, d_gb_cur, d_hist, d_gb_hist, d_len_hist, width, rows, m, rp, d_out, d_len_out, true);
    if (s != RT_OK || rows == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    RpMap M;
    std::memcpy(M.m, m, sizeof M.m);
    launch_reproject(dn_grid(dn_tiles(width, rows).tiles, c->cus), stream_or_own(c, stream), channels, d_cur, d_gb_cur, d_hist, d_gb_hist, d_len_hist, d_out,
                     d_len_out, width, rows, M, rp_scales(rp->sigma_normal, rp->sigma_depth, rp->sigma_albedo), rp->max_history);
    HIPCHK(c, hipGetLastError());
    return RT_OK;
}

extern "C" rt_status rt_reproject(rt_ctx *c, const float *cur, int32_t channels, const float *gb_cur, const float *hist, const float *gb_hist,
                                  const uint8_t *len_hist, int32_t width, int32_t rows, const float *m, const rt_reproject_params *rp, float *out,
                                  uint8_t *len_out) {
    const rt_status s = reproject_entry(c, "rt_reproject", cur, channels, gb_cur, hist, gb_hist, len_hist, width, rows, m, rp, out, len_out, false);
    if (s != RT_OK || rows == 0) return s;
    const size_t img = static_cast<size_t>(dn_image_bytes(width, rows, channels)) / sizeof(float);
    const size_t gb = static_cast<size_t>(dn_gbuffer_bytes(width, rows)) / sizeof(float), lb = static_cast<size_t>(rp_len_bytes(width, rows));
    Staging g(c);
    const float *d_cur = g.in(cur, img), *d_gc = g.in(gb_cur, gb), *d_hist = g.in(hist, img), *d_gh = g.in(gb_hist, gb);
    const uint8_t *d_lh = g.in(len_hist, lb);
    float *d_out = g.out(out, img);
    uint8_t *d_lo = g.out(len_out, lb);
    return g.finish([&] { return rt_reproject_device(c, d_cur, channels, d_gc, d_hist, d_gh, d_lh, width, rows, m, rp, d_out, d_lo, nullptr); });
}

// ---- debug ray (createDebugRay / recursiveDebugRay without the GL shapes): a host composition of the entry points above ------------
extern "C" rt_status rt_debug_ray(rt_ctx *c, const rt_camera *cam, const rt_lights *lights, float px, float py, int32_t max_levels, rt_debug_hit *out,
                                  int32_t *n_out) {
    if (!c) return RT_ERR_INVALID;
    if (!cam || !lights || !out || !n_out || max_levels < 1) { c->err = "rt_debug_ray: bad arguments"; return RT_ERR_INVALID; }
    if (!c->has_scene) { c->err = "rt_debug_ray before rt_upload_scene"; return RT_ERR_NO_SCENE; }
    *n_out = 0;
    float scr[3];
    screen_to_world(cam, px, py, scr);                                              // flyscene.cpp:439
    V3 pos{scr[0], scr[1], scr[2]};
    V3 dir = unit_fixed(pos - V3{cam->center[0], cam->center[1], cam->center[2]});   // flyscene.cpp:441
    for (int32_t n = 0; n < max_levels; ++n) {
        rt_debug_hit &r = out[n];
        std::memset(&r, 0, sizeof r);
        r.level = n; r.face = -1;
        r.pos[0] = pos.x; r.pos[1] = pos.y; r.pos[2] = pos.z; r.dir[0] = dir.x; r.dir[1] = dir.y; r.dir[2] = dir.z;
        // root box: boxIntersect(origin, origin + direction), as traceRay tests it (flyscene.cpp:655)
        const float dest[3] = {pos.x + dir.x, pos.y + dir.y, pos.z + dir.z};
        DNode root;
        HIPCHK(c, hipMemcpy(&root, c->d_nodes, sizeof root, hipMemcpyDeviceToHost));
        uint8_t in_box = 0;
        const float boxes[6] = {root.bmin[0], root.bmin[1], root.bmin[2], root.bmax[0], root.bmax[1], root.bmax[2]};
        rt_status s = rt_box_intersect(c, 1, boxes, r.pos, dest, &in_box);
        if (s != RT_OK) return s;
        int32_t face = -1; float t = -1.0f;
        s = rt_trace_rays(c, lights, 0, 1, r.pos, r.dir, r.color, &face, &t);
        if (s != RT_OK) return s;
        *n_out = n + 1;
        r.status = !in_box ? 0 : (face < 0 ? 1 : 2);
        if (face < 0) break;
        r.face = face; r.t = t;
        const V3 p0 = pos + V3{t * dir.x, t * dir.y, t * dir.z};                   // flyscene.cpp:270
        r.hit_point[0] = p0.x; r.hit_point[1] = p0.y; r.hit_point[2] = p0.z;
        float nrm[3];
        HIPCHK(c, hipMemcpy(nrm, static_cast<const float *>(c->d_face_normal) + static_cast<size_t>(face) * 3, sizeof nrm, hipMemcpyDeviceToHost));
        std::memcpy(r.normal, nrm, sizeof nrm);
        const V3 nv{nrm[0], nrm[1], nrm[2]};
        float hit[RT_MAX_LIGHTS * 3];
        const int nl = lights->n_lights < 1 ? 0 : (lights->n_lights > RT_MAX_LIGHTS ? RT_MAX_LIGHTS : lights->n_lights);
        for (int i = 0; i < nl; ++i) { hit[i * 3] = p0.x; hit[i * 3 + 1] = p0.y; hit[i * 3 + 2] = p0.z; }
        if (nl && (s = rt_light_strikes(c, nl, hit, &lights->pos[0][0], r.light_visible)) != RT_OK) return s;      // flyscene.cpp:273
        const float two = 2 * dot(dir, nv);
        const V3 refl = dir - V3{two * nv.x, two * nv.y, two * nv.z};              // flyscene.cpp:349
        r.reflected[0] = refl.x; r.reflected[1] = refl.y; r.reflected[2] = refl.z;
        pos = p0; dir = refl;
    }
    return RT_OK;
}

// ---- unit-parity probes ---------------------------------------------------------------------------------------------
extern "C" rt_status rt_box_intersect(rt_ctx *c, int32_t n, const float *boxes, const float *origin, const float *dest, uint8_t *hit) {
    if (!c) return RT_ERR_INVALID;
    if (n < 0 || (n && (!boxes || !origin || !dest || !hit))) { c->err = "rt_box_intersect: bad arguments"; return RT_ERR_INVALID; }
    if (n == 0) return RT_OK;
    Staging g(c);
    const size_t nn = static_cast<size_t>(n);
    const float *b = g.in(boxes, nn * 6), *o = g.in(origin, nn * 3), *d = g.in(dest, nn * 3);
    uint8_t *h = g.out(hit, nn);
    return g.finish([&] { launch_box_probe(c->stream, n, b, o, d, h); return RT_OK; });
}

extern "C" rt_status rt_debug_phong_samples(rt_ctx *c, int32_t n, const float *hit, const float *normal, const float *eye, const float *sample, const float *lkd,
                                            const float *lks, const float *shininess, float *out) {
    if (!c) return RT_ERR_INVALID;
    if (n < 0 || (n & 63) || (n && (!hit || !normal || !eye || !sample || !lkd || !lks || !shininess || !out))) {
        c->err = "rt_debug_phong_samples: bad arguments (n must be a multiple of 64)";
        return RT_ERR_INVALID;
    }
    if (n == 0) return RT_OK;
    const size_t nn = static_cast<size_t>(n);
    std::vector<float> packed(nn * 20, 0.0f);         // one record per case, as k_phong_probe reads it
    for (size_t i = 0; i < nn; ++i) {
        float *r = packed.data() + i * 20;
        const float *src[6] = {hit, normal, eye, sample, lkd, lks};
        for (int k = 0; k < 6; ++k) std::memcpy(r + k * 3, src[k] + i * 3, 12);
        r[18] = shininess[i];
    }
    Staging g(c);
    const float *in = g.in(packed.data(), nn * 20);
    float *o = g.out(out, nn * 6);
    return g.finish([&] { launch_phong_probe(c->stream, n, in, o); return RT_OK; });
}

extern "C" rt_status rt_tree_probe(rt_ctx *c, int32_t n, const float *origin, const float *dest, uint32_t *box_tests, uint32_t *leaf_refs, uint32_t *leaf_sig) {
    if (!c) return RT_ERR_INVALID;
    if (!c->has_scene) { c->err = "rt_tree_probe before rt_upload_scene"; return RT_ERR_NO_SCENE; }
    if (n < 0 || (n && (!origin || !dest || !box_tests || !leaf_refs || !leaf_sig))) { c->err = "rt_tree_probe: bad arguments"; return RT_ERR_INVALID; }
    if (n == 0) return RT_OK;
    if (c->flat) { c->err = "rt_tree_probe: the scene is a single leaf (no tree)"; return RT_ERR_UNSUPPORTED; }
    Staging g(c);
    const size_t nn = static_cast<size_t>(n);
    const float *o = g.in(origin, nn * 3), *d = g.in(dest, nn * 3);
    uint32_t *ob = g.out(box_tests, nn), *orf = g.out(leaf_refs, nn), *os = g.out(leaf_sig, nn);
    return g.finish([&] {
        const int blocks = (n + 255) / 256;
        launch_tree_probe(blocks < c->cus * 4 ? blocks : c->cus * 4, c->stream, c->S, n, o, d, ob, orf, os);
        return RT_OK;
    });
}

extern "C" rt_status rt_primary_points(rt_ctx *c, const rt_camera *cam, int32_t w, int32_t h, float *out) {
    if (!c) return RT_ERR_INVALID;
    if (!cam || !out || w <= 0 || h <= 0) { c->err = "rt_primary_points: bad arguments"; return RT_ERR_INVALID; }
    DCam dc;
    make_cam(cam, &dc);
    Staging g(c);
    const DCam *dcam = g.in(&dc, 1);
    float *dout = g.out(out, static_cast<size_t>(w) * static_cast<size_t>(h) * 3);
    return g.finish([&] { launch_primary_probe(c->cus * 4, c->stream, dcam, w, h, dout); return RT_OK; });
}

// executed-work counters of the last frame (counting build only: -DRT_WORK_COUNTERS, `make work`)
extern "C" rt_status rt_debug_work_counters(rt_ctx *c, uint64_t *out, int32_t n) {
    if (!c || !out || n < 0) return RT_ERR_INVALID;
#ifdef RT_WORK_COUNTERS
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t cnt = static_cast<size_t>(n) < sizeof(Control::prof) / sizeof(unsigned long long) ? static_cast<size_t>(n) : sizeof(Control::prof) / sizeof(unsigned long long);
    HIPCHK(c, hipMemcpy(out, c->d_ctl->prof, cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t i = cnt; i < static_cast<size_t>(n); ++i) out[i] = 0;
    return RT_OK;
#else
    c->err = "rt_debug_work_counters: this build carries no step counters (use librt_mi355x_work.so)";
    return RT_ERR_UNSUPPORTED;
#endif
}

// ---- host scene wrappers ------------------------------------------------------------------------------------
extern "C" rt_status rt_host_scene_load(const char *obj_path, int32_t leaf_capacity, int32_t max_depth, rt_host_scene **out) {
    if (!obj_path || !out || leaf_capacity < 1 || max_depth < 0 || max_depth > 15) return RT_ERR_INVALID;
    *out = nullptr;
    rt_host_scene *h = new rt_host_scene();
    std::string err;
    if (!h->hs.load_obj(obj_path, &err)) {
        std::fprintf(stderr, "rt_mi355x: %s\n", err.c_str());
        delete h;
        return RT_ERR_IO;
    }
    h->hs.build_octree(leaf_capacity, max_depth);
    if (h->hs.overflow) {
        std::fprintf(stderr, "rt_mi355x: the reference's octree construction does not terminate in bounded memory for this mesh at "
                             "capacity %d (more than %zu nodes / %zu face references); choose a larger capacity\n",
                     leaf_capacity, HostScene::kMaxNodes, HostScene::kMaxRefs);
        delete h;
        return RT_ERR_UNSUPPORTED;
    }
    h->hs.flatten();
    *out = h;
    return RT_OK;
}

extern "C" void rt_host_scene_free(rt_host_scene *hs) { delete hs; }

extern "C" rt_status rt_host_scene_view(const rt_host_scene *hs, rt_scene *out) {
    if (!hs || !out) return RT_ERR_INVALID;
    hs->hs.view(out);
    return RT_OK;
}

extern "C" rt_status rt_host_scene_set_model(rt_host_scene *hs, const float model[12], int32_t rebuild_tree) {
    if (!hs || !model) return RT_ERR_INVALID;
    hs->hs.set_model(model, rebuild_tree != 0);
    return hs->hs.overflow ? RT_ERR_UNSUPPORTED : RT_OK;
}

extern "C" rt_status rt_host_scene_build_gpu(rt_host_scene *hs, rt_ctx *c, int32_t leaf_capacity, int32_t max_depth) {
    if (!hs || !c || leaf_capacity < 1 || max_depth < 0 || max_depth > 15) return RT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    std::string err;
    if (!gpu_build_octree(hs->hs, leaf_capacity, max_depth, c->stream, &err)) { c->err = "rt_host_scene_build_gpu: " + err; return RT_ERR_HIP; }
    if (hs->hs.overflow) return RT_ERR_UNSUPPORTED;
    hs->hs.flatten();
    return RT_OK;
}

extern "C" rt_status rt_host_scene_info(const rt_host_scene *hs, int32_t out[8], float root_box[6]) {
    if (!hs || !out) return RT_ERR_INVALID;
    hs->hs.info(out, root_box);
    return RT_OK;
}

extern "C" void rt_default_camera(rt_camera *cam, int32_t w, int32_t h) { if (cam && w > 0 && h > 0) default_camera(cam, w, h); }
extern "C" void rt_yaw_camera(rt_camera *cam, int32_t w, int32_t h, float yaw) { if (cam && w > 0 && h > 0) yaw_camera(cam, w, h, yaw); }
extern "C" void rt_screen_to_world(const rt_camera *cam, float i, float j, float out[3]) { if (cam && out) screen_to_world(cam, i, j, out); }
extern "C" void rt_default_lights(rt_lights *l, int32_t area) { if (l) default_lights(l, area); }
extern "C" void rt_sphere_offsets(uint32_t seed, float radius, int32_t n, float *out) { if (out && n > 0) sphere_offsets(seed, radius, n, out); }

extern "C" rt_status rt_write_ppm(const char *path, const float *rgb, int32_t w, int32_t h) {
    if (!path || !rgb || w <= 0 || h <= 0) return RT_ERR_INVALID;
    return write_ppm(path, rgb, w, h) ? RT_OK : RT_ERR_IO;
}
extern "C" rt_status rt_write_pfm(const char *path, const float *rgb, int32_t w, int32_t h) {
    if (!path || !rgb || w <= 0 || h <= 0) return RT_ERR_INVALID;
    std::FILE *f = std::fopen(path, "wb");
    if (!f) return RT_ERR_IO;
    bool ok = std::fprintf(f, "PF\n%d %d\n-1.0\n", w, h) > 0;
    for (int32_t y = h - 1; ok && y >= 0; --y)
        ok = std::fwrite(rgb + static_cast<size_t>(y) * w * 3, sizeof(float), static_cast<size_t>(w) * 3, f) == static_cast<size_t>(w) * 3;
    ok = (std::fclose(f) == 0) && ok;
    return ok ? RT_OK : RT_ERR_IO;
}
extern "C" rt_status rt_write_ppm_u8(const char *path, const uint8_t *rgb, int32_t w, int32_t h) {
    if (!path || !rgb || w <= 0 || h <= 0) return RT_ERR_INVALID;
    return write_ppm_u8(path, rgb, w, h) ? RT_OK : RT_ERR_IO;
}
