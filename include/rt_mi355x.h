/*
 * rt_mi355x.h -- C ABI of the MI355X-native primary/shadow ray-trace path.
 *
 * Drop-in boundary for the reference's CPU ThreadPool render (Sh-Anand/Raytracer-in-CPP).  The reference
 * has no FFI layer; the boundary is two C++ members (citations relative to /root/reference):
 *     void            Flyscene::raytraceScene(int width = 0, int height = 0)           src/flyscene.hpp:84
 *                                                                                      src/flyscene.cpp:519-648
 *     Eigen::Vector3f Flyscene::traceRay(Vector3f& origin, Vector3f& direction, int level,
 *                                        vector<Vector3f>& lights, bool countRay)      src/flyscene.hpp:94
 *                                                                                      src/flyscene.cpp:651-771
 * called from src/main.cpp:70 (key 'T') and from the pool lambda src/flyscene.cpp:615-623.
 * Each entry point below names the reference interface it replaces.  Plain pointers and sizes only; no C++,
 * Eigen, Tucano or torch types cross this boundary.  All functions return RT_OK (0) or a negative rt_status;
 * nothing throws and nothing calls exit().  A context belongs to one HIP device; rt_render* is blocking and not
 * re-entrant per context; distinct contexts may be used from distinct threads.
 *
 * The library FAILS LOUDLY (RT_ERR_NO_DEVICE / RT_ERR_HIP) when there is no MI355X-class HIP device: there is
 * no CPU fallback in the product.
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int rt_status;
enum {
    RT_OK = 0,
    RT_ERR_INVALID = -1,      /* bad argument (NULL, W/H <= 0, L > 25, N not a square grid, ...) */
    RT_ERR_NO_DEVICE = -2,    /* no HIP device / wrong device index */
    RT_ERR_HIP = -3,          /* a HIP runtime call failed (see rt_last_error) */
    RT_ERR_IO = -4,           /* file could not be opened / written */
    RT_ERR_UNSUPPORTED = -5,  /* scene exceeds a compiled limit (tree depth, samples) */
    RT_ERR_NO_SCENE = -6      /* render before rt_upload_scene */
};

#define RT_MAX_LIGHTS 25      /* the reference's fixed bool visibleLights[25]  (flyscene.cpp:699,835) */
#define RT_MAX_SAMPLES 1024   /* per light; the reference hard-codes 5x5 = 25  (flyscene.cpp:971) */
#define RT_MAX_DEPTH 15       /* recursion levels kept per pixel (the reference is unbounded) */
#define RT_MAX_SUPERSAMPLING 4   /* n of rt_set_supersampling: at most 4 x 4 sub-samples per pixel */

/* ---- flattened scene: the device-friendly restatement of BoxTree / Tucano::Mesh / Material::Mtl ------------- */
/* replaces: class BoxTree (src/boxTree.hpp:15-62), BoundingBox (src/boundingBox.hpp:21-43),
 *           Tucano::Face (tucano/mesh.hpp:238-247), Material::Mtl (tucano/materials/mtl.hpp:16-116)             */
typedef struct rt_node {
    float    bmin[3], bmax[3];
    uint32_t first;           /* leaf: first index into face_refs; inner: index of first child node            */
    uint32_t count_flags;     /* low 31 bits: #faces (leaf) or #children (inner); bit 31 set = leaf            */
} rt_node;                    /* 32 bytes */
#define RT_NODE_LEAF 0x80000000u

typedef struct rt_material {
    float kd[3], ks[3];
    float shininess, optical_density;
    int32_t illum;
} rt_material;                /* 36 bytes */

typedef struct rt_scene {
    uint32_t n_nodes;      const rt_node  *nodes;        /* node 0 = root; children of a node are contiguous    */
    uint32_t n_face_refs;  const uint32_t *face_refs;    /* leaf face lists, concatenated                       */
    uint32_t n_faces;
    const float    *tri_verts;      /* n_faces*9  world-space A,B,C = ((model*shape)*v).head<3>()               */
    const float    *face_normal;    /* n_faces*3  Face::normal (object space, used untransformed)               */
    const uint32_t *tri_vid;        /* n_faces*3  vertex ids (index vert_normal)                                */
    const int32_t  *mat_id;         /* n_faces                                                                  */
    uint32_t n_vert_normals; const float *vert_normal;   /* *3, mesh.getNormal(vertex_id)                       */
    uint32_t n_materials;    const rt_material *materials;
    float model[12];                /* Mesh::getModelMatrix() 3x4 row-major (identity unless modifyTriangle)    */
} rt_scene;

/* replaces: Tucano::Flycamera state read by raytraceScene (flyscene.cpp:551,575; camera.hpp:115-118,155-173)    */
typedef struct rt_camera {
    float center[3];          /* flycamera.getCenter()                                                          */
    float inv_view[12];       /* getViewMatrix().inverse(), 3x4 row-major                                       */
    float fovy;               /* degrees; 60 in the reference (flyscene.cpp:46)                                 */
    float aspect;             /* width/(float)height                                                            */
    float viewport[4];        /* (0,0,W,H)                                                                      */
} rt_camera;

enum { RT_LIGHT_POINT = 0, RT_LIGHT_AREA = 1, RT_LIGHT_SPHERE = 2 };
/* replaces: Flyscene::lights, lightrep colour, the stdin switches areaLight/pointLight (flyscene.cpp:31-34,68,72)
 * and the literals of createSpherePoint/createAreaLight (flyscene.cpp:956-972, arealight.hpp:15-25)             */
typedef struct rt_lights {
    int32_t n_lights;                       /* 1..RT_MAX_LIGHTS                                                 */
    float   pos[RT_MAX_LIGHTS][3];
    float   color[3];                       /* (1,1,0)                                                          */
    int32_t mode;                           /* RT_LIGHT_POINT (1 sample) | RT_LIGHT_AREA (usteps*vsteps)        */
    int32_t usteps, vsteps;                 /* 5,5 in the reference; 8,8 / 16,16 for the 64 / 256 sample configs */
    float   len_x, len_y;                   /* 0.3, 0.15                                                        */
    /* RT_LIGHT_SPHERE: the third branch of createSpherePoint (flyscene.cpp:974-995, neither stdin switch set): sample s of a light at p
       is offsets[s] + p, offsets[s] = Vector3f(x, y, z) / 5 of that branch.  The reference draws them from an unseeded
       std::random_device for every shaded hit; here the caller fixes them per frame (rt_sphere_offsets gives the seeded restatement).  */
    int32_t      n_offsets;                 /* 1..RT_MAX_SAMPLES (25 in the reference)                          */
    const float *offsets;                   /* host, n_offsets * 3; copied by the call                           */
} rt_lights;

/* replaces: the literals inside traceRay / lightStrikes and raytraceScene's image size + thread partitioning    */
typedef struct rt_params {
    int32_t width, height;    /* full frame                                                                     */
    int32_t max_depth;        /* levels 0..max_depth are traced (a hit at level == max_depth is plain Phong);
                                 <0 = RT_MAX_DEPTH.  The reference never tests `level` (flyscene.cpp:651-771)   */
    /* row shard (multi-GPU): this call renders the rows y in [row0,row1) with ((y-row0)/stripe) % nranks == rank,
       in increasing y.  Single GPU: row0=0,row1=height,stripe=1,rank=0,nranks=1.                               */
    int32_t row0, row1, stripe, rank, nranks;
    int32_t collect_stats;    /* 0: ray counters + per-kernel times of this call (when stats != NULL; syncs)
                                 1: also run the counting (no early-out) traversal variants first and fill the
                                    algorithmic counters; costs a second frame, never set inside a timed region
                                 2: deferred timing -- record per-kernel HIP events on the launch stream, do NOT
                                    synchronise; sums are fetched later with rt_timing_collect (bench loops)   */
} rt_params;

typedef struct rt_stats {
    /* ray = one traversal query (root AABB test + tree walk)                                                    */
    uint64_t rays_primary, rays_bounce, rays_centre, rays_sample;
    uint64_t pixels, pixels_culled;       /* pixels whose primary ray misses the root box (flyscene.cpp:576-581) */
    uint64_t shaded_hits;                 /* phongShade calls                                                    */
    /* algorithmic (reference-semantics) counters, only with collect_stats: boxIntersect calls and leaf face
       references exactly as BoxTree::intersect/traceRay/lightStrikes would perform them (no early-out)         */
    uint64_t box_tests, leaf_tri_refs;                 /* whole frame (closest-hit + centre + sample rays)      */
    uint64_t box_tests_shadow, leaf_tri_refs_shadow;   /* the share of the sample-shadow kernel (k_shadow)      */
    /* per-kernel device time of the last render, milliseconds (HIP events on the render stream)                 */
    float ms_trace, ms_shadow, ms_shade, ms_resolve, ms_total;
    uint32_t launches_trace, launches_shadow, launches_shade;   /* levels that launched the group (historic name)                 */
    uint32_t launches_total;              /* device operations one frame enqueues: kernel launches + the control-block memset */
    uint64_t rays_sample_walked;          /* sample shadow segments actually FORMED and walked: rays_sample minus those whole tiles (k_beam) or whole
                                             (hit, light) units were proven unblocked for before a ray existed (0 in the counting pass)  */
} rt_stats;

typedef struct rt_ctx rt_ctx;

/* ---- context --------------------------------------------------------------------------------------------- */
rt_status   rt_create(rt_ctx **out, int device);                     /* replaces: ThreadPool pool(n) flyscene.cpp:609 */
void        rt_destroy(rt_ctx *ctx);                                 /* replaces: pool.~ThreadPool() flyscene.cpp:634 */
const char *rt_last_error(const rt_ctx *ctx);                        /* NULL-safe; static string when ctx == NULL     */
const char *rt_version(void);
void       *rt_stream(rt_ctx *ctx);                                  /* the context's own hipStream_t (what a NULL `stream` argument means)   */

/* replaces: the scene state traceRay reads through `this` (octree, mesh, materials).  Arrays are copied.          */
rt_status rt_upload_scene(rt_ctx *ctx, const rt_scene *scene);

/* replaces: Flyscene::raytraceScene's pixel loop + pool execution (flyscene.cpp:573-629).
 * out_rgb: host, [n_local_rows * W * 3] float, row-major (y,x); out_hit (optional): level-0 closest face id or -1 */
rt_status rt_render(rt_ctx *ctx, const rt_camera *cam, const rt_lights *lights, const rt_params *p,
                    float *out_rgb, int32_t *out_hit, rt_stats *stats);

/* Same, results stay in device memory (for RCCL gathers / chained launches).  d_out_rgb: device float
 * [n_local_rows*W*3]; d_out_u8 (optional): device uint8 [n_local_rows*W*3] quantised as ppmIO.hpp:145;
 * stream: hipStream_t (NULL = the context's own stream).  Asynchronous when stats == NULL.                        */
rt_status rt_render_device(rt_ctx *ctx, const rt_camera *cam, const rt_lights *lights, const rt_params *p,
                           float *d_out_rgb, uint8_t *d_out_u8, int32_t *d_out_hit, void *stream, rt_stats *stats);
/* waits for the frames rt_render_device has enqueued (the context's stream and the stream of the latest call); reports a work-list overflow */
rt_status rt_synchronize(rt_ctx *ctx);

/* Sums the per-kernel device times (ms_* = SUM over frames, launches_* = total launches) of every frame rendered
 * with collect_stats == 2 since the last call, plus the ray counters of the last frame.  Synchronises the stream.  */
rt_status rt_timing_collect(rt_ctx *ctx, rt_stats *out);

/* ---- captured frames (hipGraph) -------------------------------------------------------------------------------
 * The launch sequence of a frame has no host round trip, so it is captured once into a hipGraph and replayed per frame
 * (animation paths: BASELINE cfg5).  Lights, frame size, shard and output buffers are frozen at capture; the camera is
 * read from device memory and may change on every launch.  No reference counterpart (the reference re-runs
 * raytraceScene per key press, main.cpp:69-70).                                                                    */
typedef struct rt_graph rt_graph;
rt_status rt_graph_create(rt_ctx *ctx, const rt_lights *lights, const rt_params *p, float *d_out_rgb, uint8_t *d_out_u8,
                          rt_graph **out);
/* asynchronous: uploads `cam`, then replays the captured frame on `stream` (NULL = the context's stream)             */
rt_status rt_graph_launch(rt_graph *g, const rt_camera *cam, void *stream);
/* synchronises and returns the ray counters of the last replayed frame                                             */
rt_status rt_graph_stats(rt_graph *g, rt_stats *out);
void      rt_graph_destroy(rt_graph *g);

/* ---- multi-GPU: one process per GPU, row stripes (rt_params.stripe / rank / nranks), ONE RCCL gather over xGMI -----------------------
 * No reference counterpart (single process, std::thread pool: src/flyscene.cpp:558-629).  RCCL is bound at run time (dlopen); a
 * single-GPU user never loads it.  Typical use on every rank:
 *     rank 0: rt_comm_unique_id(id); broadcast id to the other processes out of band (MPI, a file, torch.distributed ...)
 *     rt_comm_create(&comm, device, id, nranks, rank);
 *     per frame: rt_render_gather(ctx, comm, &cam, &lights, &params, d_local_u8, block_bytes, d_gathered_u8 /-root only-/, 0, stream);
 *     root: copy d_gathered_u8 to the host, rt_stitch_rows(...), rt_write_ppm_u8("result.ppm", ...)                                    */
#define RT_COMM_ID_BYTES 128          /* sizeof(ncclUniqueId) */
typedef struct rt_comm rt_comm;
rt_status   rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]);
rt_status   rt_comm_create(rt_comm **out, int device, const uint8_t id[RT_COMM_ID_BYTES], int32_t nranks, int32_t rank);
void        rt_comm_destroy(rt_comm *comm);
const char *rt_comm_last_error(const rt_comm *comm);
/* the single exchange of a frame: `bytes` bytes from every rank to `root` (rank r's block at d_gathered + r * bytes); asynchronous on
 * `stream` (hipStream_t), no host synchronisation, capturable                                                                       */
rt_status   rt_comm_gather_rows(rt_comm *comm, const void *d_local, size_t bytes, void *d_gathered, int32_t root, void *stream);
/* rt_render_device(d_out_u8 = d_local_u8) + rt_comm_gather_rows on the same stream; local_bytes = the common block size
 * (>= rt_local_rows(p) * width * 3 on every rank)                                                                                   */
rt_status   rt_render_gather(rt_ctx *ctx, rt_comm *comm, const rt_camera *cam, const rt_lights *lights, const rt_params *p, uint8_t *d_local_u8,
                             size_t local_bytes, uint8_t *d_gathered_u8, int32_t root, void *stream);
/* root, host side: de-interleaves the gathered blocks (row0 = 0, row1 = height) into frame[height][width][3]                          */
rt_status   rt_stitch_rows(const uint8_t *gathered, size_t block_bytes, int32_t width, int32_t height, int32_t stripe, int32_t nranks, uint8_t *frame);

/* number of rows rt_render produces for p */
int32_t rt_local_rows(const rt_params *p);

/* ---- supersampling (anti-aliasing): n x n regular grid of sub-samples per pixel, box filter ---------------------------------------
 * No reference counterpart: raytraceScene traces one ray per pixel through the raster point screenToWorld(Vector2f(i, j))
 * (flyscene.cpp:573-598).  1 <= n <= RT_MAX_SUPERSAMPLING; default 1.  Needs no device; an invalid n returns RT_ERR_INVALID and keeps
 * the previous setting.
 *   Samples: sub-sample (sx, sy), 0 <= sx, sy < n, of pixel (i, j) is raytraceScene's primary ray for the raster point
 *            screenToWorld(Vector2f(x, y)), x = (float)i + o[sx], y = (float)j + o[sy] (float additions),
 *            o[s] = (float)((2*s + 1 - n) / (2.0*n)): +-0.25 for n = 2; -1/3, 0, 1/3 for n = 3; +-0.125, +-0.375 for n = 4.
 *            The pre-cull, the direction screen - centre and the rest of traceRay are unchanged.
 *   Pixel:   acc / (float)(n*n), acc = 0.0f plus the sub-sample colours in float, sy outer, sx inner (no FMA, correctly rounded
 *            division); the 8-bit output quantises that mean as writePPMImage does (ppmIO.hpp:145).  n = 1 is the one-ray frame, bit for bit.
 *   Scope:   later rt_render, rt_render_device, rt_render_gather and rt_graph_create calls on ctx (a captured graph keeps the n it was
 *            captured with).  rt_trace_rays, rt_debug_ray, rt_light_strikes and the probe entry points ignore it.
 *   With n > 1 out_hit / d_out_hit must be NULL (else RT_ERR_INVALID); rt_stats counts sub-samples (pixels = n*n*W*local_rows, the ray
 *   counters count sub-sample rays).  A frame whose working set exceeds the device's memory returns RT_ERR_UNSUPPORTED.
 * For a camera whose viewport origin is (0, 0), sub-sample (sx, sy) equals pixel (i, j) of the n = 1 frame rendered with
 * viewport[0] = -o[sx], viewport[1] = -o[sy], bit for bit ((float)i - (-o) == (float)i + o).                                            */
rt_status rt_set_supersampling(rt_ctx *ctx, int32_t n);

/* ---- adaptive supersampling: refine only the pixels on colour edges ---------------------------------------------------------------
 * No reference counterpart.  The threshold tau lives on the context like n (rt_params stays 36 bytes); default -1.  Needs no device; a
 * NULL ctx or a NaN threshold returns RT_ERR_INVALID and keeps the previous setting.
 *   tau < 0:  every pixel is refined: the regular n x n frame of rt_set_supersampling, by the same code path (no first pass).
 *   tau >= 0 (+inf included) and n > 1: the adaptive frame.  C is the float RGB of the one-ray frame of the whole W x H frame (bit for bit
 *            what rt_render returns with n = 1 for the same camera, lights and max_depth).  Pixel p is refined when some 4-neighbour q
 *            inside [0, W) x [0, H) has a channel c with fabsf(C_c(p) - C_c(q)) > tau (float32; a NaN never refines; both sides of an edge
 *            are refined).  A refined pixel is the pixel of the regular n x n frame bit for bit; any other pixel is C(p) bit for bit; the
 *            8-bit output quantises the result as for any frame.  The rule reads the whole frame: a row rendered by a shard or a row range
 *            equals that row of the single-GPU full frame (the call also traces the one-ray rows its rows' neighbours need).
 *            tau = +inf, and a 1 x 1 frame, give the n = 1 frame bit for bit.
 *   n = 1:    the threshold is ignored (the one-ray frame).
 *   Scope:   as n: later rt_render, rt_render_device, rt_render_gather and rt_graph_create calls (a graph keeps the threshold it was captured
 *            with).  out_hit / d_out_hit must still be NULL when n > 1.
 *   rt_stats of an adaptive frame: the ray counters, shaded_hits and pixels_culled sum both passes; pixels = the one-ray pixels traced
 *            (neighbour rows included) + n*n * the refined pixels; launches_total counts every device operation of the frame.          */
rt_status rt_set_supersampling_threshold(rt_ctx *ctx, float threshold);
/* synchronises, then returns the number of output pixels refined by the latest eager frame on ctx (rt_render, rt_render_device or
 * rt_render_gather): 0 for n = 1, W x local rows for tau < 0                                                                           */
rt_status rt_supersampling_refined(rt_ctx *ctx, uint64_t *refined);

/* ---- thin-lens depth of field: the n x n sub-sample rays of a pixel start at n x n points of a lens --------------------------------------
 * No reference counterpart (a pinhole camera).  aperture = the lens radius in world units, focus = the depth of the plane in focus in
 * units of the screen-plane distance (the screen plane of screenToWorld is at view depth 1: for a rigid inv_view a world distance along
 * the view axis; the default camera sits at (0, 0, 2) and the normalised model is centred at the origin, so focus = 2 focuses the model's
 * centre).  The setting lives on the context like n; default aperture 0.  Needs no device.  Invalid (RT_ERR_INVALID, the previous
 * setting is kept): a NULL ctx; an aperture that is negative, NaN or infinite; with aperture > 0 a focus that is not finite and > 0.
 *   aperture == 0: the lens is off.  Every frame is the pinhole frame bit for bit, by the pinhole code path and with its launch count,
 *            also after the lens was on.  (focus is then stored but not looked at.)
 *   aperture > 0:  sub-sample (sx, sy) of output pixel (i, j) -- i the output column, j the output row OF THE FULL FRAME, so shards
 *            agree -- is traced as follows, all arithmetic float32 without FMA in exactly this order:
 *            1. S = screenToWorld(x, y) at the sub-sample's raster point, exactly as rt_set_supersampling defines it; C = cam.center;
 *               v = S - C (the pinhole direction).
 *            2. focus point P_c = C_c + focus * v_c per component (multiply, then add).
 *            3. per-pixel scramble in uint32 arithmetic: h = (i * 0x9E3779B1) ^ (j * 0x85EBCA6B); h ^= h >> 15; h *= 0x2C1B3C6D;
 *               h ^= h >> 12; h *= 0x297A2D39; h ^= h >> 15; rotation r = h >> 26, lens point k = (sy*n + sx + ((h >> 8) & 0xFFFF)) % (n*n).
 *               h(0, 0) = 0x00000000, h(1, 0) = 0x205F0435, h(0, 1) = 0x5191C1C6, h(7, 3) = 0xAEB4B2F2, h(1919, 1079) = 0x7519E3DC.
 *            4. (a, b) = (aperture * T[r][k].x, aperture * T[r][k].y), T the table of rt_lens_table.  With U = (m[0], m[4], m[8]) and
 *               V = (m[1], m[5], m[9]), the first two columns of inv_view: origin O_c = (C_c + a * U_c) + b * V_c.
 *            5. direction D = P - O, unnormalised.  Pre-cull as raytraceScene does with the ray's own two points: boxIntersect(root, O, P);
 *               a miss is BACKGROUND and counts in pixels_culled; otherwise the colour is traceRay(O, D, level 0), unchanged from there on
 *               (its own root test on O + D, closest hit, lightStrikes, Phong with eye O, bounces).
 *            6. pixel = the same float sum (sy outer, sx inner, from 0.0f) and correctly rounded division as rt_set_supersampling;
 *               the 8-bit output as for any frame.
 *   Table:   host double precision, cast to float last.  Lens point k of an n x n grid is the Shirley-Chiu concentric-disc image of the
 *            cell centre (x, y) = ((k % n + 0.5) / n, (k / n + 0.5) / n): with u = 2x - 1, v = 2y - 1: (0, 0) if u == v == 0; if |u| > |v|:
 *            rho = u, phi = (pi/4) * (v/u); else rho = v, phi = pi/2 - (pi/4) * (u/v); the point is (rho cos phi, rho sin phi).  Rotation r
 *            turns it by (pi/2) * r / RT_LENS_ROTATIONS (the concentric grid is symmetric under quarter turns, so the 64 steps inside one
 *            quarter are 64 different patterns).  For n = 1 every entry is (0, 0): the lens needs n > 1 to blur; an n = 1 lens frame is
 *            still defined by the steps above (the pinhole frame up to the rounding of (C + focus * v) - C), not by the pinhole path.
 *            The per-pixel rotation and cyclic shift keep the 4 / 9 / 16 lens points from showing as that many ghost copies of every
 *            out-of-focus edge; the table makes them reproducible without a device sin / cos.
 *   Scope:   later rt_render, rt_render_device, rt_render_gather and rt_graph_create calls; a graph keeps the aperture and focus it was
 *            captured with and takes C, U, V from the camera of each rt_graph_launch.  rt_trace_rays, rt_debug_ray, rt_primary_points and
 *            the probe entry points ignore the lens.  out_hit follows the supersampling rule (NULL when n > 1; with n = 1 the level-0 hit
 *            of the lens ray).  rt_stats keeps its meanings.
 *   Adaptive threshold with the lens on: tau is ignored and the frame is the regular n x n lens frame (rt_supersampling_refined =
 *            W x local rows): the one-ray frame is sharp and cannot tell where blur will land.                                          */
#define RT_LENS_ROTATIONS 64
rt_status rt_set_lens(rt_ctx *ctx, float aperture, float focus);
/* host only: out[RT_LENS_ROTATIONS * n*n * 2], T[r][k] at out[(r * n*n + k) * 2 + {0, 1}]; 1 <= n <= RT_MAX_SUPERSAMPLING, out != NULL
 * (else RT_ERR_INVALID).  The device copy the frames read is made from this function.                                               */
rt_status rt_lens_table(int32_t n, float *out);

/* ---- camera motion blur: the n x n sub-sample rays of a pixel leave the camera at n x n times of an open shutter ---------------------------
 * No reference counterpart (every frame is an instantaneous exposure).  The camera passed to a render call is the camera at shutter OPEN;
 * `close`, held on the context (the struct is copied), is the camera at shutter CLOSE; each sub-sample ray is traced through the camera of
 * its own time t in [0, 1) between the two.  No extra rays: the same n x n rays integrate over pixel area, lens (if on) and time.  Only the
 * camera moves: the scene, its octree and the lights are those of the frame.  close == NULL: the shutter is off (the default) and every
 * frame is the still frame bit for bit, by the code path and with the launch count it had before, also after the shutter was on.  Needs no
 * device.  Invalid (RT_ERR_INVALID, the previous setting is kept): a NULL ctx; a close camera with a non-finite center / inv_view value.
 * All arithmetic float32, every operation rounded on its own (no FMA), in exactly this order:
 *   Time:    output pixel (i, j) -- i the output column, j the output row OF THE FULL FRAME, so shards agree -- sub-sample (sx, sy),
 *            0 <= sx, sy < n, nn = n*n.  With h the per-pixel scramble of rt_set_lens (step 3 there) and uint32 arithmetic:
 *            g = h ^ 0x68E31DA4; g ^= g >> 15; g *= 0x2C1B3C6D; g ^= g >> 12; g *= 0x297A2D39; g ^= g >> 15;
 *            slot = (sx*n + sy + (g & 0xFFFF)) % nn  (sx*n + sy: the transpose of the lens's sy*n + sx, so the time slots and the lens points
 *            of a pixel's sub-samples are not one cyclic shift of each other), u = (float)(g >> 16) * 2^-16 (exact),
 *            t = ((float)slot + u) / (float)nn  (the sum is exact; one correctly rounded division).  rt_shutter_time evaluates it.
 *            A pixel's sub-samples take every slot once (stratified in time); u jitters the strata per pixel, so a moving edge dissolves
 *            into noise rather than into nn ghost copies.  n = 1 is defined and useful: one time per pixel, t = u.
 *            g(0, 0) = 0x18FEA250, g(1, 0) = 0x83B87A41, g(0, 1) = 0x0B4F00CA, g(7, 3) = 0xE22EC469, g(1919, 1079) = 0x67E7315C.
 *   Camera:  K(t) = rt_shutter_camera(open, close, t): for each of the 15 values q of center[3] and inv_view[12], d = q_close - q_open;
 *            q(t) = q_open if d == 0, else q_open + t*d (multiply, then add).  fovy, aspect and viewport are open's.  The d == 0 rule makes
 *            K(t) = open bit for bit when close equals open, negative zeros included.  The linear blend is exact for translations and first
 *            order for rotations: the blended basis of a yaw of a few degrees is shorter than unit by under 1e-3 (a yaw of a between the
 *            two cameras shortens it by at most 1 - cos(a/2)); a caller with a large rotation splits the exposure into several frames.
 *   Ray:     lens off: S = screenToWorld of K(t) at the sub-sample's raster point exactly as rt_set_supersampling defines it,
 *            O = K(t).center, D = S - O; pre-cull boxIntersect(root, O, S), a miss is BACKGROUND and counts in pixels_culled; otherwise
 *            traceRay(O, D, level 0), unchanged.  Lens on: steps 1-5 of rt_set_lens with C, U, V and screenToWorld taken from K(t),
 *            everything else as there.  Fold and 8-bit output as for any supersampled frame.
 *   Scope:   later rt_render, rt_render_device, rt_render_gather and rt_graph_create calls.  At render time those return RT_ERR_INVALID when
 *            close's fovy, aspect or viewport differ bitwise from the open camera's (only the pose moves).  A graph captured with the
 *            shutter on keeps "on" whatever the context is set to later and takes BOTH cameras per launch from rt_graph_launch_shutter;
 *            rt_graph_launch(g, cam) on such a graph means close = cam (a still frame); rt_graph_launch_shutter on a graph captured with the
 *            shutter off is RT_ERR_INVALID.  With the shutter on the adaptive threshold is ignored as it is with the lens (the one-ray frame
 *            cannot tell where blur will land; rt_supersampling_refined = W x local rows).  out_hit follows the supersampling rule (NULL when
 *            n > 1; with n = 1 the level-0 hit of the pixel's ray).  rt_trace_rays, rt_debug_ray, rt_primary_points and the probe entry
 *            points ignore the shutter.  rt_stats keeps its meanings.                                                                    */
rt_status rt_set_shutter(rt_ctx *ctx, const rt_camera *close);
/* asynchronous: uploads both cameras, then replays a frame captured with the shutter on                                               */
rt_status rt_graph_launch_shutter(rt_graph *g, const rt_camera *open, const rt_camera *close, void *stream);
/* host only, no device: the two pieces of the definition, so that callers and tests can reproduce a frame's rays.
 * rt_shutter_time: 1 <= n <= RT_MAX_SUPERSAMPLING, 0 <= sx, sy < n, t != NULL (else RT_ERR_INVALID).  rt_shutter_camera: out may alias open. */
rt_status rt_shutter_time(int32_t n, uint32_t i, uint32_t j, int32_t sx, int32_t sy, float *t);
rt_status rt_shutter_camera(const rt_camera *open, const rt_camera *close, float t, rt_camera *out);

/* ---- multi-pass accumulation: a frame is the mean of `count` passes, each with its own sub-sample shift and its own lens / time scrambles ----
 * No reference counterpart.  One pass is one frame as the sections above define it (n x n sub-samples, lens, shutter); pass p moves the grid
 * of sub-samples by a low-discrepancy offset inside its cell and reseeds the per-pixel scrambles, so `count` passes integrate pixel area, lens
 * and time with count * n*n different rays at the working set of ONE pass.  With n = 1 that is jittered anti-aliasing: 16 passes = 16 rays per
 * pixel.  The setting lives on the context like n: frames render passes first .. first + count - 1; default (0, 1).  Needs no device.  Invalid
 * (RT_ERR_INVALID, the previous setting is kept): a NULL ctx, first < 0, count < 1, first + count > RT_MAX_PASSES.
 * PASS 0 IS THE FRAME OF THE SECTIONS ABOVE IN EVERY BIT; with (0, 1) every frame takes the code path and the launch count it had before.
 *   Raster:  phi_b(p) is the radical inverse of p in base b, in host double in exactly this order:
 *            f = 1, r = 0; while (p > 0) { f = f / b; r = r + f * (p % b); p = p / b; }  ->  r.  Wrapped to the cell: e_b(p) = phi_b(p) if
 *            phi_b(p) < 0.5, else phi_b(p) - 1, so e_b(0) = 0 and -0.5 <= e_b < 0.5.  rt_pass_offsets evaluates
 *            ox[s] = (float)((2*s + 1 - n) / (2.0*n) + e_2(p) / n),  oy[s] = (float)((2*s + 1 - n) / (2.0*n) + e_3(p) / n),  0 <= s < n.
 *            Sub-sample (sx, sy) of pixel (i, j) uses the raster point x = (float)i + ox[sx], y = (float)j + oy[sy] (float additions, also for
 *            n = 1 when p > 0); everything downstream of the raster point (screenToWorld, pre-cull, traceRay) is unchanged.  As float bits:
 *            n = 1: p = 1 ox BF000000 oy 3EAAAAAB; p = 3 ox BE800000 oy 3DE38E39; p = 255 ox BB800000 oy 3E191BBE.
 *            n = 2, p = 1: ox BF000000 00000000, oy BDAAAAAB 3ED55555.   n = 3, p = 2: ox BE800000 3DAAAAAB 3ED55555, oy BEE38E39 BDE38E39 3E638E39.
 *            n = 4, p = 5: ox BEF00000 BE600000 3D000000 3E900000, oy BEDC71C7 BE38E38E 3D8E38E4 3EA38E39.
 *            The 256 shifts (e_2, e_3) are pairwise distinct (the Halton points of bases 2 and 3).
 *   Scrambles: step 3 of rt_set_lens starts from h = (i * 0x9E3779B1) ^ (j * 0x85EBCA6B) ^ (p * 0xC2B2AE35) (uint32), then the same mixing;
 *            g of rt_set_shutter derives from that h as before.  (i, j) are full-frame coordinates, so shards and row ranges agree with the
 *            full frame.  (h, g): p = 1 pixel (0, 0): F439FA4B, F327B022; p = 1 (1, 0): A5DA958D, 92CB3388; p = 2 (7, 3): 08C48D66, E408EBEE;
 *            p = 255 (1919, 1079): 5885945E, E62BAD0C.  The lens table of n = 1 stays all zeros (the lens still needs n > 1 to blur); the
 *            shutter blurs at n = 1, because t = u changes from pass to pass.  Lights and their samples are the same in every pass.
 *   Fold:    F_p = the float RGB frame of pass p (the n x n mean as rt_set_supersampling defines it; the one-ray colour for n = 1).
 *            count == 1: the result is F_first bit for bit (no accumulator, the launches of a single frame).
 *            count > 1: per channel A = 0.0f; for p = first .. first + count - 1 in order A = A + F_p; result = A / (float)count -- every
 *            operation rounded on its own, no FMA, a correctly rounded division.  The 8-bit output quantises the result as for any frame.
 *            The sum lives in device memory and is folded by the resolve launch of each pass: a count-pass frame enqueues exactly count times
 *            the device operations of one pass, with no host round trip in between.
 *   Scope:   later rt_render, rt_render_device, rt_render_gather and rt_graph_create calls; a graph keeps the (first, count) it was captured
 *            with and replays all its passes with the camera(s) of each launch.  rt_trace_rays, rt_debug_ray, rt_primary_points and the probe
 *            entry points ignore the setting.  out_hit / d_out_hit must be NULL when n > 1 or count > 1 (else RT_ERR_INVALID); with n = 1 and
 *            count = 1 it is the level-0 hit of that pass's ray.  With (first, count) != (0, 1) the adaptive threshold is ignored, as it is
 *            with the lens (rt_supersampling_refined reports what it reports for a regular frame).
 *   rt_stats: the ray counters, shaded_hits, pixels, pixels_culled, rays_sample_walked, ms_* and launches_* sum over the passes;
 *            collect_stats = 1 counts every pass; collect_stats = 2 queues one set of timing events per pass.                                  */
#define RT_MAX_PASSES 256
rt_status rt_set_passes(rt_ctx *ctx, int32_t first, int32_t count);
/* host only: ox[n], oy[n] of pass p; 1 <= n <= RT_MAX_SUPERSAMPLING, 0 <= p < RT_MAX_PASSES, ox, oy != NULL (else RT_ERR_INVALID).  The frames
 * take their offsets from this function.                                                                                                  */
rt_status rt_pass_offsets(int32_t n, int32_t p, float *ox, float *oy);

/* ---- adaptive pass counts: a pixel of a count-pass frame stops taking passes once the standard error of its mean is within `tol` ----
 * No reference counterpart.  The setting lives on the context like n and (first, count); default tol = -1, min_passes = 8.  Needs no device.
 * Invalid (RT_ERR_INVALID, the previous setting is kept, rt_last_error names the function): a NULL ctx, a NaN tol, min_passes < 2,
 * min_passes > RT_MAX_PASSES.  +inf is a valid tolerance.
 * OFF when tol < 0 or count <= min_passes: the frame is the rt_set_passes frame in every bit, by the code path and the launch count it has
 * without this section -- also after the feature was on.
 * ON when tol >= 0 and count > min_passes.  F_p is the float RGB frame of pass p exactly as rt_set_passes defines it.  Every output pixel is
 * computed on its own; every operation is float32 and rounded on its own, no FMA.  Per pixel and channel:
 *   S1 = 0.0f, S2 = 0.0f, taken = 0, active = true
 *   for k = 1 .. count, p = first + k - 1:
 *     if active:  S1 = S1 + F_p;  q = F_p * F_p;  S2 = S2 + q;  taken = k
 *     if active and min_passes <= k < count:  kf = (float)k;  d_c = kf * S2_c - S1_c * S1_c (two products, one subtraction) per channel;
 *                 T = ((tol * tol) * (kf * kf)) * (kf - 1.0f);  the pixel becomes inactive when d_c <= T in all three channels (a NaN never does)
 *   result = S1 / (float)taken, a correctly rounded division; the 8-bit output quantises it as for any frame.
 * d_c <= T is the float form of "the squared standard error of the mean, (S2/k - (S1/k)^2) / (k - 1), is at most tol^2".  An inactive pixel forms no
 * ray in later passes.  So: a pixel that stays active to the end is the rt_set_passes pixel bit for bit; tol = +inf gives the (first,
 * min_passes) frame bit for bit; and, the rule knowing full-frame pixel identity only, shards and row ranges equal the full frame's rows.
 * LIMIT: the rule looks at one pixel at a time.  A pixel whose first min_passes samples all fall on one side of an edge stops with variance 0
 * and a wrong mean; min_passes is the guard (Adaptive pass counts, has measured figures).
 *   Scope:   as rt_set_passes: later rt_render, rt_render_device, rt_render_gather and rt_graph_create calls; a graph keeps the setting it was
 *            captured with and owns its statistics buffers as it owns its accumulator.  out_hit / d_out_hit must be NULL.  The adaptive
 *            supersampling threshold is ignored, primary culling stays off, the probe entry points ignore the setting.
 *   rt_stats: pixels = n*n * (sum of taken over the output pixels); the other counters, ms_* and launches_* sum over the passes as before
 *            (launches_total counts what is enqueued: passes behind the point where every pixel has stopped still launch, over empty lists).
 *            collect_stats = 1 reruns the frame like any other (both runs take the same decisions); collect_stats = 2 queues one event set per pass.
 * rt_pass_map synchronises, then copies `taken` of every output pixel of the latest eager frame on ctx (rt_render, rt_render_device,
 * rt_render_gather), row-major over that call's local rows.  RT_ERR_INVALID if that frame was not an adaptive-pass frame or n_pixels is not
 * width x local rows.                                                                                                                      */
rt_status rt_set_pass_tolerance(rt_ctx *ctx, float tol, int32_t min_passes);
rt_status rt_pass_map(rt_ctx *ctx, uint16_t *out, size_t n_pixels);

/* ---- geometry buffers: coverage, depth, face normal and diffuse colour of an output pixel, averaged as the colour is --------------------
 * No reference counterpart.  This section is the DEFINITION of the eight floats a frame would return next to its colour; NO FRAME FILLS THEM
 * YET: rt_gbuffer_device and rt_gbuffer below compute them in a call of their own (Geometry buffers, says what is specified,
 * what the CPU restatement shows and why the frames do not fill them).  tests/gbuffer_ref.py restates the definition in float32.
 * RT_GBUFFER_CHANNELS = 8 floats per output pixel q, at [q * 8 + c], row-major over a call's local rows:
 *   c = 0 alpha, 1 depth, 2..4 normal, 5..7 albedo.
 *   Per sub-sample: f = the level-0 closest face of the sub-sample's own ray (what out_hit holds for an n = 1 frame; -1 for a ray that is
 *            pre-culled or hits nothing), t = that hit's ray parameter: the hit point is O + t * D with the sub-sample's own O and D as the
 *            sections above define them.  Pinhole: D = S - C reaches the screen plane at view depth 1, so t is the view depth in screen-plane
 *            distances; lens and shutter rays: the t of that ray.  The sub-sample's value v is, with f >= 0,
 *            (1.0f, t, face_normal[3f .. 3f+2], materials[mat_id[f]].kd[0..2]) and otherwise eight 0.0f.  face_normal is used exactly as
 *            uploaded in rt_scene (object space, untransformed): the normal traceRay reflects about.
 *   Pass:    n = 1: G_p = v itself (a -0.0f normal component stays -0.0f).  n > 1: per channel a = 0.0f; for sy outer, sx inner: a = a + v;
 *            G_p = a / (float)(n*n) -- the order and rounding of rt_set_supersampling: float32, every operation rounded on its own, no FMA,
 *            a correctly rounded division.
 *   Frame:   count == 1: G_first, bit for bit.  count > 1: A = 0.0f; A = A + G_p for p in order; A / (float)count -- the fold of rt_set_passes.
 *   So depth, normal and albedo are COVERAGE-WEIGHTED SUMS (an empty sub-sample adds 0 to all eight): divide by alpha where the mean over
 *   the covered part of the pixel is wanted.                                                                                                */
#define RT_GBUFFER_CHANNELS 8
/* rt_gbuffer_device: the buffers of the frame a later rt_render on ctx would render with `cam` and `p`, as a query of its own.
 *   d_out: device memory on the context's device, 16-byte aligned (else RT_ERR_INVALID), rt_local_rows(p) * p->width * RT_GBUFFER_CHANNELS
 *            floats; pixel q of the call's local rows (row-major, the order of rt_render's output) at [q * 8 + c].  Exactly that many
 *            floats are written, nothing behind them.  Zero local rows: RT_OK, nothing enqueued.
 *   p:       width, height and the row shard (row0, row1, stripe, rank, nranks) mean what they mean for rt_render, and are checked as
 *            there; max_depth and collect_stats are ignored.  Sizes: the frame of sub-samples of the call's rows holds at most
 *            UINT32_MAX / 3 sub-samples and n * width, n * height fit an int32 (else RT_ERR_UNSUPPORTED, as for a frame), so pixel and
 *            tile numbers fit 32 bits; the index of a float (up to 8 * 1,431,655,765) is 64-bit throughout.
 *   Samples: the sub-samples, their rays and the passes are those of that frame: n of rt_set_supersampling, the lens of rt_set_lens, the
 *            shutter of rt_set_shutter (cam is the camera at shutter open; a close camera whose fovy, aspect or viewport differ bitwise is
 *            RT_ERR_INVALID, as for a frame), (first, count) of rt_set_passes.  The adaptive supersampling threshold is ignored: the call
 *            always takes the regular n x n frame.  With adaptive pass counts ON (rt_set_pass_tolerance: tol >= 0 and count > min_passes)
 *            the call returns RT_ERR_INVALID: an inactive pixel forms no ray, so the buffers of such a frame are not defined.
 *            rt_set_primary_cull is not looked at (it never changes a result).
 *   Hit:     f and t of a sub-sample are what the level-0 step of a frame computes for its ray: the ray passes the root-box pre-test of
 *            raytraceScene's loop and traceRay's own root test, then the closest hit of rt_closest_hits_device.
 *   A NULL context, camera, params or d_out is RT_ERR_INVALID; before rt_upload_scene the call returns RT_ERR_NO_SCENE.  Scene-only and
 *   ASYNCHRONOUS like rt_closest_hits_device: one kernel on `stream` (NULL = the context's stream), no synchronisation, none of the context's
 *   frame buffers -- the camera travels as a kernel argument, so a frame on another stream may run beside it; it is ordered by its stream
 *   only, leaves rt_supersampling_refined, rt_pass_map and every later frame as they were, and the caller orders it against
 *   rt_upload_scene.  THE ONE EXCEPTION: the first call on a context allocates the table of rt_pass_offsets (32 KB) and, with the lens on,
 *   the lens table a lens frame would make, and uploads them with a synchronous copy; they are freed by rt_destroy.
 * rt_gbuffer: the same with a host pointer (no alignment rule): it allocates, enqueues the call above on the context's stream,
 *   synchronises that stream and downloads.                                                                                              */
rt_status rt_gbuffer_device(rt_ctx *ctx, const rt_camera *cam, const rt_params *p, float *d_out, void *stream);
rt_status rt_gbuffer(rt_ctx *ctx, const rt_camera *cam, const rt_params *p, float *out);

/* ---- denoising: an edge-avoiding a-trous wavelet filter of an image, guided by the geometry buffers of the same frame --------------------
 * No reference counterpart.  This section is the DEFINITION; tests/denoise_ref.py restates it in numpy float32 (Denoising).  All
 * arithmetic is float32, every operation rounded on its own, no FMA, every division correctly rounded, in exactly the order written.
 *   Image:   width x rows pixels, row-major, channels = 1 or 3 floats per pixel at [q * channels + c]: what rt_render_device writes (3) and
 *            rt_ambient_occlusion_device's d_ao (1).  The geometry buffers hold RT_GBUFFER_CHANNELS floats per pixel, what rt_gbuffer_device
 *            writes for the same rows.  The buffer is ONE image: rows are neighbours as stored (a striped shard is the caller's business).
 *   Guide of pixel q, once per pixel: a = G[0]; q is COVERED exactly when a > 0.0f; then z = G[1] / a, N_c = G[2+c] / a, A_c = G[5+c] / a
 *            (seven divisions; a == 1.0f leaves the values as they are).  N is not normalised.
 *   Iteration k = 0 .. iterations-1 reads I_k (I_0 = the input) and writes I_{k+1}; the output is I_iterations.  step = 2^k pixels.
 *            H = {0.375f, 0.25f, 0.0625f}.  Scales: sc = sigma_color * 2^-k (one float product with the exact constant), sn = sigma_normal,
 *            sz = sigma_depth * (float)step, sa = sigma_albedo; each squared once: sc2 = sc * sc, ...
 *            A pixel p that is not covered: I_{k+1}(p) = I_k(p), bit for bit.
 *            A covered pixel p: sumw = 0.0f, sum_c = 0.0f; for dy = -2 .. 2 outer, dx = -2 .. 2 inner, q = p + step * (dx, dy):
 *              q outside [0, width) x [0, rows), or q not covered: the tap is skipped.
 *              h = H[|dx|] * H[|dy|] (exact).  The centre tap (dx == dy == 0): w = h, no guide is evaluated.
 *              Every other tap: w = h, then the guides in the order colour, normal, depth, albedo.  d2 is the squared distance of value(p) -
 *              value(q): colour ((dr*dr) + (dg*dg)) + (db*db) on I_k, or d*d for one channel; normal the same form on N; depth d*d on z;
 *              albedo the colour form on A.  u = 1.0f - d2 / s2 with that guide's squared scale; if !(u > 0.0f) -- which covers NaN -- the
 *              tap is skipped; otherwise w = w * (u * u).
 *              sumw = sumw + w; sum_c = sum_c + w * I_k(q)_c (a product, then an addition).
 *            I_{k+1}(p)_c = sum_c / sumw.  sumw >= 9/64 because of the centre tap.
 *            The weights have compact support, max(0, 1 - d2/s2)^2: across an edge a tap weighs exactly nothing.  A sigma of +inf makes
 *            d2 / inf = 0, u = 1 and leaves w as it is: that guide never stops a tap.
 *   Pin:     a 2 x 1 one-channel image {1.0f, 0.0f}, both pixels covered, every sigma +inf, one iteration -> {3F19999A, 3ECCCCCD} as bits:
 *            (9/64) / (15/64) and (3/32) / (15/64).
 * rt_denoise_params: iterations in 1 .. RT_DENOISE_MAX_ITERATIONS; each sigma > 0, +inf allowed; NaN or <= 0 is RT_ERR_INVALID.
 * rt_default_denoise_params: iterations = 5, sigma_color = 1.0f (3F800000), sigma_normal = 0.5f (3F000000), sigma_depth = 0.125f (3E000000),
 *   sigma_albedo = 0.25f (3E800000) (Denoising, has the experiment they come from).
 * rt_denoise_scratch_bytes: host only; the bytes of d_scratch a call with these arguments needs (two float4 guide records per pixel and two
 *   working images of 16 bytes per pixel for three channels, 4 for one, each part 16-byte aligned); 0 for invalid arguments.
 * rt_denoise_device: d_in, d_gbuffer, d_scratch, d_out are device pointers on the context's device; d_in and d_gbuffer are only read.
 *   RT_ERR_INVALID: a NULL context, pointer or dp; channels not 1 or 3; width < 1; rows < 0; iterations or a sigma out of range; d_out or
 *   d_scratch not 16-byte aligned; d_out or d_scratch sharing a byte with each other or with an input.  RT_ERR_UNSUPPORTED: width * rows >
 *   INT32_MAX.  rows == 0: RT_OK, nothing enqueued.  Exactly width * rows * channels floats of d_out are written, and nothing behind the
 *   rt_denoise_scratch_bytes bytes of d_scratch.  The call needs NO SCENE: it works before rt_upload_scene and never returns
 *   RT_ERR_NO_SCENE.  ASYNCHRONOUS: 1 + iterations kernels on `stream` (NULL = the context's stream), no allocation, no synchronisation,
 *   no host copy, on the first call as on every other; none of the context's buffers, so a frame on another stream may run beside it; it
 *   is ordered by its stream only and leaves rt_supersampling_refined, rt_pass_map and every later frame as they were.
 * rt_denoise: the same with host pointers (no alignment or overlap rule): it allocates the image, the buffers, the scratch and the output,
 *   uploads, enqueues the call above on the context's stream, synchronises that stream, downloads and frees.                              */
#define RT_DENOISE_MAX_ITERATIONS 8
typedef struct rt_denoise_params {
    int32_t iterations;      /* 1 .. RT_DENOISE_MAX_ITERATIONS; iteration k = 0 .. iterations-1 has step 2^k pixels */
    float   sigma_color;     /* each sigma: > 0, +inf allowed (= that guide never stops a tap); NaN, <= 0: RT_ERR_INVALID */
    float   sigma_normal, sigma_depth, sigma_albedo;
} rt_denoise_params;
size_t    rt_denoise_scratch_bytes(int32_t width, int32_t rows, int32_t channels);
rt_status rt_denoise_device(rt_ctx *ctx, const float *d_in, int32_t channels, const float *d_gbuffer, int32_t width, int32_t rows,
                            const rt_denoise_params *dp, void *d_scratch, float *d_out, void *stream);
rt_status rt_denoise(rt_ctx *ctx, const float *in, int32_t channels, const float *gbuffer, int32_t width, int32_t rows,
                     const rt_denoise_params *dp, float *out);
void      rt_default_denoise_params(rt_denoise_params *dp);

/* ---- upsampling: a joint bilateral upsample of a low-resolution image, guided by the geometry buffers of the low and the high frame --------
 * No reference counterpart.  This section is the DEFINITION; tests/upsample_ref.py restates it in numpy float32 (Upsampling).  All
 * arithmetic is float32, every operation rounded on its own, no FMA, every division correctly rounded, in exactly the order written.
 *   Images:  high: width x rows pixels; low: w x r with w = ceil(width / s), r = ceil(rows / s), factor s in 2 .. RT_UPSAMPLE_MAX_FACTOR.
 *            channels = 1 or 3 floats per pixel, packed, row-major, at [q * channels + c], in the low image and in the output.  d_gb_low and
 *            d_gb_high hold RT_GBUFFER_CHANNELS floats per pixel, what rt_gbuffer_device writes for the low and for the high frame.  Each
 *            buffer is ONE image; low row J lies on high row s*J, low column I on high column s*I (a striped shard is the caller's business).
 *   Guide of a pixel: the denoiser's.  a = G[0]; the pixel is COVERED exactly when a > 0.0f; then z = G[1] / a, N_c = G[2+c] / a,
 *            A_c = G[5+c] / a.
 *   Scales:  sn2 = sigma_normal * sigma_normal; sz = sigma_depth * (float)s, sz2 = sz * sz; sa2 = sigma_albedo * sigma_albedo.
 *   High pixel p = (x, y): I0 = x / s, fx = x - I0 * s; J0 = y / s, fy = y - J0 * s (integers).
 *            bx[0] = (float)(s - fx) / (float)s, bx[1] = (float)fx / (float)s; by[0], by[1] likewise from fy.
 *            sumw = 0.0f, sum_c = 0.0f; for ey = 0, 1 outer, ex = 0, 1 inner, low pixel q = (I0 + ex, J0 + ey):
 *              q outside [0, w) x [0, r): the tap is skipped.
 *              h = bx[ex] * by[ey]; h == 0.0f: the tap is skipped (a high pixel that lies on a low pixel looks at that pixel alone).
 *              covered(q) != covered(p): the tap is skipped (background is filled from background taps, a surface from surface taps).
 *              wt = h.  If p is covered, the guides in the order normal, depth, albedo: d2 = ((dx*dx) + (dy*dy)) + (dz*dz) of N(p) - N(q),
 *              d*d of z(p) - z(q), the first form on A(p) - A(q); u = 1.0f - d2 / s2 with that guide's squared scale; if !(u > 0.0f) --
 *              which covers NaN -- the tap is skipped; otherwise wt = wt * (u * u).
 *              sumw = sumw + wt; sum_c = sum_c + wt * L(q)_c (a product, then an addition).
 *            If sumw > 0.0f: out_c = sum_c / sumw, miss = 0.  Otherwise out_c = L(n)_c bit for bit with the nearest low pixel
 *            n = (min((2x + s) / (2s), w - 1), min((2y + s) / (2s), r - 1)) (integers), and miss = 1.  The rule is on sumw, not on the
 *            number of taps: three tiny factors can underflow a surviving tap to weight zero.  A sigma of +inf never stops a tap.
 *            So out(s*I, s*J) = (0.0f + 1.0f * L(I, J)) / 1.0f = L(I, J) bit for bit (but for -0.0f, which comes back +0.0f) wherever the two
 *            guides let that one tap live, and the nearest pixel of (s*I, s*J) is (I, J) where they do not: always where
 *            the low and the high buffers agree at that pixel, as they do for one-ray pinhole frames whose cameras differ only in the
 *            viewport size divided by s (screenToWorld maps raster i to 2 (i - vp0) / vp2 - 1, so low pixel I is high pixel s*I ray for ray
 *            whenever s divides width and rows).
 *   Pins:    one channel, alpha = 1 everywhere, equal normals and albedo, every sigma +inf unless said; outputs as bits:
 *            (A) width 4, rows 1, s 2, low {1, 0} -> 3F800000 3F000000 00000000 00000000.
 *            (B) width 5, rows 1, s 3, low {1, 0} -> 3F800000 3F2AAAAB 3EAAAAAB 00000000 00000000 (the two float thirds sum to 1).
 *            (C) width 3, rows 1, s 2, low {1, 0}, low depths {1, 1.5}, high depths {1, 1.125, 1.5}, sigma_depth 0.25
 *                -> 3F800000 3F52380F 00000000.
 *            (D) as (C) with the middle high depth 3.0 -> 3F800000 00000000 00000000, miss {0, 1, 0}: both taps stopped, nearest is low 1.
 *            (E) width 2, rows 3, s 2, low column {0.25, 0.75} -> rows {0.25, 0.25}, {0.5, 0.5}, {0.75, 0.75}.
 * rt_upsample_params: factor in 2 .. RT_UPSAMPLE_MAX_FACTOR; each sigma > 0, +inf allowed; NaN or <= 0 is RT_ERR_INVALID.
 * rt_default_upsample_params: factor = 2, sigma_normal = 2.0f (40000000), sigma_depth = 0.125f (3E000000), sigma_albedo = 0.25f (3E800000):
 *   the depth and albedo scales of rt_default_denoise_params; its normal scale, 0.5f, lost the experiment of DESIGN.md 5, Upsampling, on
 *   a facetted smooth surface, 2.0f stops exactly opposite unit normals only and weighs every other pair.
 * rt_upsample_low_size: host only; *w = ceil(width / factor), *r = ceil(rows / factor).  RT_ERR_INVALID (nothing written): a NULL w or r,
 *   width < 1, rows < 0, factor out of range.
 * rt_upsample_device: d_low, d_gb_low, d_gb_high, d_out, d_miss are device pointers on the context's device; the first three are only read.
 *   d_miss may be NULL: then no mask is written.  RT_ERR_INVALID: a NULL context, up or other pointer; channels not 1 or 3; width < 1;
 *   rows < 0; factor or a sigma out of range; d_out, d_gb_low or d_gb_high not 16-byte aligned; d_out or d_miss sharing a byte with each
 *   other or with an input.  RT_ERR_UNSUPPORTED: width * rows > INT32_MAX.  rows == 0: RT_OK, nothing enqueued.  Exactly width * rows *
 *   channels floats of d_out are written and width * rows bytes of d_miss, nothing behind them.  The call needs NO SCENE: it works before
 *   rt_upload_scene and never returns RT_ERR_NO_SCENE.  ASYNCHRONOUS: ONE kernel on `stream` (NULL = the context's stream), no scratch,
 *   no allocation, no synchronisation, no host copy, on the first call as on every other; none of the context's buffers, so a frame on
 *   another stream may run beside it; it is ordered by its stream only and leaves rt_supersampling_refined, rt_pass_map and every later
 *   frame as they were.
 * rt_upsample: the same with host pointers (no alignment or overlap rule; miss may be NULL): it allocates the images, the buffers and the
 *   mask, uploads, enqueues the call above on the context's stream, synchronises that stream, downloads and frees.                        */
#define RT_UPSAMPLE_MAX_FACTOR 8
typedef struct rt_upsample_params {
    int32_t factor;          /* 2 .. RT_UPSAMPLE_MAX_FACTOR: the low image has ceil(width / factor) x ceil(rows / factor) pixels */
    float   sigma_normal, sigma_depth, sigma_albedo;   /* each > 0, +inf allowed (= that guide never stops a tap); NaN, <= 0: RT_ERR_INVALID */
} rt_upsample_params;
void      rt_default_upsample_params(rt_upsample_params *up);
rt_status rt_upsample_low_size(int32_t width, int32_t rows, int32_t factor, int32_t *w, int32_t *r);
rt_status rt_upsample_device(rt_ctx *ctx, const float *d_low, int32_t channels, const float *d_gb_low, const float *d_gb_high,
                             int32_t width, int32_t rows, const rt_upsample_params *up, float *d_out, uint8_t *d_miss, void *stream);
rt_status rt_upsample(rt_ctx *ctx, const float *low, int32_t channels, const float *gb_low, const float *gb_high,
                      int32_t width, int32_t rows, const rt_upsample_params *up, float *out, uint8_t *miss);

/* ---- temporal reprojection: the accumulated image of the previous frame carried into the current one along a camera path ----------------------
 * No reference counterpart.  This section is the DEFINITION; tests/reproject_ref.py restates it (Temporal reprojection).  Device
 * arithmetic is float32, every operation rounded on its own, no FMA, every division correctly rounded, in exactly the order written.
 *   Images:  width x rows pixels, channels = 1 or 3 floats per pixel, packed, row-major, at [q * channels + c].  cur: the current frame's image.
 *            gb_cur, gb_hist: RT_GBUFFER_CHANNELS floats per pixel, what rt_gbuffer_device writes for the current and for the previous frame.
 *            hist: the previous frame's OUTPUT OF THIS CALL (its plain image for the first step).  len_hist: one uint8_t per pixel, the number of
 *            frames the history pixel stands for; 0 = no history here.  Outputs: out and len_out.  Each buffer is ONE image (a striped shard
 *            is the caller's business).  Only the camera may move between the frames; a lens or shutter frame's depth is not a pinhole t, so
 *            for such frames the caller gets what the map gives.
 *   Guide of a pixel: the denoiser's.  a = G[0]; the pixel is COVERED exactly when a > 0.0f; then z = G[1] / a, N_c = G[2+c] / a,
 *            A_c = G[5+c] / a.
 *   Scales:  sn2 = sigma_normal * sigma_normal, sz2 = sigma_depth * sigma_depth, sa2 = sigma_albedo * sigma_albedo.
 *   The map: rt_reproject_map(cur, prev, m) -- host only, no device -- writes m[r*4 + k], rows r = x, y, depth, columns k = E, U, V, W: the
 *            linear-fractional map that sends raster point (x, y) and ray parameter z of `cur` -- the world point P = C_cur + z * D with
 *            D = screenToWorld_cur(x, y) - C_cur, the pinhole t of the geometry buffers -- to the unique (x', y', z') of `prev` with
 *            C_prev + z' * (screenToWorld_prev(x', y') - C_prev) = P.  C is each camera's own `center` (not the translation column of inv_view).
 *            All in host DOUBLE from the float fields, every operation on its own, in this order; cast to float last.  Per camera:
 *              persp = (float)(1.0 / tan((double)(fovy / 2.0f) * (M_PI / 180.0))), scale = (float)(1.0 / (double)persp) as screen_to_world
 *              has them; sc = (double)scale, as = (double)(aspect * scale) (a float product); v0..v3 = viewport;
 *              ax = (2.0 / v2) * as, bx = ((-2.0 * v0) / v2 - 1.0) * as, ay = (-2.0 / v3) * sc, by = (1.0 + (2.0 * v1) / v3) * sc;
 *              with row r of inv_view = (m0, m1, m2, t):  B[r][0] = m0 * ax, B[r][1] = m1 * ay,
 *              B[r][2] = (((m0 * bx + m1 * by) - m2) + t) - center[r]:   D(x, y) = B (x, y, 1)^T.
 *            I = the inverse of B_prev by cofactors, as mat3_inverse forms it: cof(i, j) = B[i1][j1] * B[i2][j2] - B[i1][j2] * B[i2][j1] with
 *              i1 = (i+1) % 3, i2 = (i+2) % 3 and j1, j2 likewise; det = cof(0,0) * B[0][0] + (cof(1,0) * B[1][0] + cof(2,0) * B[2][0]);
 *              invdet = 1.0 / det; I[r][k] = cof(k, r) * invdet.
 *            d = C_cur - C_prev (each a double difference of two floats).
 *            m[r][E] = (float)(I[r][0] * d[0] + (I[r][1] * d[1] + I[r][2] * d[2]));
 *            m[r][U + k] = (float)(I[r][0] * Bc[0][k] + (I[r][1] * Bc[1][k] + I[r][2] * Bc[2][k])) for k = 0, 1, 2 (U, V, W), Bc = B_cur.
 *            EQUAL CAMERAS (every bit of every field): the identity by rule, not by arithmetic: m[x][U] = m[y][V] = m[depth][W] = 1.0f and
 *            every other entry +0.0f.
 *            RT_ERR_INVALID (m untouched): a NULL argument; a non-finite camera field; a zero viewport[2] or [3]; a singular previous
 *            inv_view (the determinant of its 3 x 3 part, or of B_prev, formed as above, is 0 or not finite); a non-finite result.
 *            As float bits, rows x, y, depth, each E U V W:
 *              a path from yaw 0.40 to yaw 0.42 at 96 x 64 (cur = rt_yaw_camera 0.42, prev = rt_yaw_camera 0.40; both centres are (0, 0, 2)):
 *                370396E1 3F8230F7 00000000 BFF84A4B
 *                366BCAA8 3C3D2C6A 3F800000 BF0F84E2
 *                33EBCAA8 39BD2C6A 00000000 3F7B83D9
 *              a path from rt_default_camera to yaw 0.05 at 1920 x 1080 (cur = rt_yaw_camera 0.05, prev = rt_default_camera):
 *                00000000 3F866801 00000000 C2BFFC34
 *                00000000 3CEC6257 3F800000 C1E3024C
 *                00000000 3860208F 00000000 3F728C31
 *   Pixel p = (x, y), xf = (float)x, yf = (float)y:
 *            1. p not covered, or !(z > 0.0f): out = cur(p) bit for bit, len_out = 1 (the background is a constant and has no depth).
 *            2. rho = 1.0f / z; for r = x, y, depth: num_r = m[r][E] * rho + ((xf * m[r][U] + yf * m[r][V]) + m[r][W]).  den = num_depth;
 *               !(den > 0.0f): no history (the point was behind the previous camera).  x' = num_x / den, y' = num_y / den, zr = z * den.
 *               Unless x' > -1.0f && x' < (float)width && y' > -1.0f && y' < (float)rows: no history.  These are float tests (a NaN fails
 *               them), made before any conversion to an integer.
 *            3. I0 = (int)floorf(x'), fx = x' - (float)I0, bx = {1.0f - fx, fx}; J0, fy, by likewise from y'.
 *            4. sumw = 0.0f, sum_c = 0.0f, nmin = 255; for ey = 0, 1 outer, ex = 0, 1 inner, history pixel q = (I0 + ex, J0 + ey).  The tap is
 *               skipped when q is outside [0, width) x [0, rows); when h = bx[ex] * by[ey] equals 0.0f; when len_hist(q) == 0; when q is not
 *               covered in gb_hist.  wt = h, then the guides in the order normal, depth, albedo: d2 = ((dx*dx) + (dy*dy)) + (dz*dz) of
 *               N(p) - N(q); d*d of d = zr - z(q); the first form on A(p) - A(q); u = 1.0f - d2 / s2 with that guide's squared scale;
 *               if !(u > 0.0f) -- which covers NaN -- the tap is skipped; otherwise wt = wt * (u * u).
 *               sumw = sumw + wt; sum_c = sum_c + wt * hist(q)_c (a product, then an addition); nmin = min(nmin, len_hist(q)).
 *            5. sumw > 0.0f: H_c = sum_c / sumw; n = min(nmin + 1, max_history); out_c = H_c + (cur_c - H_c) / (float)n (one subtraction,
 *               one division, one addition); len_out = n.  Otherwise -- and wherever "no history" is said above -- out = cur(p) bit for
 *               bit and len_out = 1.
 *            So with the identity map and equal buffers every covered pixel has the one tap of weight 1.0f (fx = fy = 0) and
 *            out = hist + (cur - hist) / n: k calls from len = 1 give the running mean over k + 1 frames up to float rounding, and len
 *            reaches max_history and stays there.  A pixel whose previous position was hidden (the depth guide), outside the frame or behind
 *            the previous camera starts again at 1.
 *   Pins:    one channel, alpha = 1 everywhere, equal normals and albedo, depth 1 unless said, every sigma +inf, max_history 255; as bits:
 *            (A) 2 x 1, identity map, hist {1, 0}, len {1, 1}, cur {0, 1} -> 3F000000 3F000000, len {2, 2}.
 *            (B) the same with m[x][W] = 0.5f, cur {0, 0}: pixel 0 blends taps 0 and 1 -> 3E800000; pixel 1 keeps tap 1 alone (tap 2 is
 *                outside) -> 00000000; len {2, 2}.
 *            (C) as (A) with history depths {1, 3}, current depths {1, 1}, sigma_depth 0.25: pixel 1 has no history -> 3F000000 3F800000,
 *                len {2, 1}.
 *            (D) as (A) with len_hist {255, 0} and max_history 4 -> 3F400000 3F800000, len {4, 1}.
 *            (E) width 1, rows 3, identity map plus m[y][W] = -1.0f, hist {1, 2, 3}, len {1, 1, 1}, cur {0, 0, 0}: row 0 looks at y' = -1,
 *                which is not > -1 -> 00000000 (len 1); rows 1, 2 -> 3F000000 3F800000 (len 2).
 * rt_reproject_params: max_history in 1 .. RT_REPROJECT_MAX_HISTORY; each sigma > 0, +inf allowed; NaN or <= 0 is RT_ERR_INVALID.
 * rt_default_reproject_params: max_history = 32, sigma_normal = 2.0f (40000000), sigma_depth = 0.015625f (3C800000), sigma_albedo = 0.25f
 *   (3E800000): the normal and albedo scales of rt_default_upsample_params; its depth scale, 0.125f, lost the experiment of DESIGN.md 5,
 *   Temporal reprojection, on dodgeColorTest (history bleeds across creases), an eighth of it won on both scenes.
 * rt_reproject_device: d_cur, d_gb_cur, d_hist, d_gb_hist, d_len_hist, d_out, d_len_out are device pointers on the context's device; the
 *   first five are only read; m (12 floats) and rp are host pointers, read before the call returns.  RT_ERR_INVALID: a NULL context,
 *   pointer, m or rp; channels not 1 or 3; width < 1; rows < 0; max_history or a sigma out of range; a non-finite entry of m; d_out,
 *   d_gb_cur or d_gb_hist not 16-byte aligned; d_out or d_len_out sharing a byte with each other or with any input (other lanes read the
 *   history's taps: the caller ping-pongs two sets of buffers).  RT_ERR_UNSUPPORTED: width * rows > INT32_MAX.  rows == 0: RT_OK, nothing
 *   enqueued.  Exactly width * rows * channels floats of d_out and width * rows bytes of d_len_out are written, nothing behind them.  The
 *   call needs NO SCENE: it works before rt_upload_scene and never returns RT_ERR_NO_SCENE.  ASYNCHRONOUS: ONE kernel on `stream` (NULL =
 *   the context's stream), no scratch, no allocation, no synchronisation, no host copy, on the first call as on every other; none of the
 *   context's buffers, so a frame on another stream may run beside it; it is ordered by its stream only and leaves
 *   rt_supersampling_refined, rt_pass_map and every later frame as they were.
 * rt_reproject: the same with host pointers (no alignment or overlap rule): it allocates the images, the buffers and the lengths, uploads,
 *   enqueues the call above on the context's stream, synchronises that stream, downloads and frees.                                         */
#define RT_REPROJECT_MAX_HISTORY 255
typedef struct rt_reproject_params {
    int32_t max_history;     /* 1 .. RT_REPROJECT_MAX_HISTORY: the length at which the running mean becomes an exponential one */
    float   sigma_normal, sigma_depth, sigma_albedo;   /* each > 0, +inf allowed (= that guide never stops a tap); NaN, <= 0: RT_ERR_INVALID */
} rt_reproject_params;
void      rt_default_reproject_params(rt_reproject_params *rp);
rt_status rt_reproject_map(const rt_camera *cur, const rt_camera *prev, float *m);
rt_status rt_reproject_device(rt_ctx *ctx, const float *d_cur, int32_t channels, const float *d_gb_cur, const float *d_hist,
                              const float *d_gb_hist, const uint8_t *d_len_hist, int32_t width, int32_t rows, const float *m,
                              const rt_reproject_params *rp, float *d_out, uint8_t *d_len_out, void *stream);
rt_status rt_reproject(rt_ctx *ctx, const float *cur, int32_t channels, const float *gb_cur, const float *hist, const float *gb_hist,
                       const uint8_t *len_hist, int32_t width, int32_t rows, const float *m, const rt_reproject_params *rp, float *out,
                       uint8_t *len_out);

/* ---- light jitter offsets: where a pass would put the area light's samples inside their grid cells ---------------------------------------
 * No reference counterpart: createSpherePoint / arealight.hpp put sample (i, j) at the centre of cell (i, j) of the usteps x vsteps grid, and so
 * does every pass of rt_set_passes ("Lights and their samples are the same in every pass"): a 5 x 5 light puts at most 26 brightness levels
 * into a penumbra however many passes are averaged.  This function is the DEFINITION of the per-pass shift that would remove the bands;
 * rt_soft_shadows_device (below) takes such a pair and puts its samples there, AND NO FRAME USES IT (Light jitter, says what is
 * specified, what the CPU restatement shows and why the frames' device side is not in).
 *   Offsets: with e_b(p) the wrapped radical inverse of rt_set_passes (the same loop, in host double):
 *            fu = (float)(0.5 + e_5(p)),  fv = (float)(0.5 + e_7(p)):  0 <= fu, fv < 1, pass 0 gives exactly (0.5f, 0.5f), and the 256 pairs
 *            are pairwise distinct (the Halton points of bases 5 and 7; bases 2 and 3 shift the raster).  As float bits (fu, fv):
 *            p = 1: 3F333333 3F249249; p = 2: 3F666666 3F492492; p = 5: 3F0A3D71 3E5B6DB7; p = 7: 3F70A3D7 3F053978; p = 255: 3F0B0F28 3F76ABA9.
 *   Samples: sample (i, j) of a light whose corner is c would have fi = (float)i + fu, fj = (float)j + fv -- each ONE float32 addition to the
 *            integer index -- and be the point (fi * cx, fj * cy, z), cx = (c.x + len_x) / (float)usteps, cy = (c.y + len_y) / (float)vsteps,
 *            z = c.z as today.  With fu = fv = 0.5f that is today's sample in every bit (tests/light_jitter_ref.py restates it).
 * host only: 0 <= p < RT_MAX_PASSES, fu, fv != NULL (else RT_ERR_INVALID).                                                                   */
rt_status rt_light_jitter_offsets(int32_t p, float *fu, float *fv);

/* Primary culling (no counterpart in the reference, which tests the root box for every pixel, flyscene.cpp:576; DESIGN.md 5, Primary
 * culling).  on != 0 (the default): a frame whose rays all leave the one camera centre through one raster point per pixel -- no
 * supersampling, lens, shutter or passes other than (0, 1) -- projects the eight corners of the root box (nodes[0] as uploaded) through its
 * camera on the host, takes the bounding rectangle of the projections, grows it by at least one 8 x 8 tile on every side and forms no
 * primary ray for the tiles outside it: their pixels are culled pixels (rt_stats.pixels_culled) of the background colour, out_hit = -1,
 * which is what the root-box test would have said.  Every output and every counter is bit for bit what on = 0 gives; only the time
 * differs.  A box wholly behind the camera leaves an empty rectangle.  The rectangle is the whole frame -- nothing is skipped -- whenever
 * some corner lies at or behind the camera while another lies in front, or very close to it against the box's depth, the camera centre lies inside (or exactly on a face plane of) the slightly inflated box, an input is not finite,
 * the view matrix is singular, or the float rounding of the device's ray is not small against the margin.  It travels with the camera: a
 * captured graph keeps the setting it was created with and every rt_graph_launch computes the rectangle of its camera.  rt_trace_rays and
 * the probe entry points are not affected.                                                                                          */
rt_status rt_set_primary_cull(rt_ctx *ctx, int32_t on);

/* Frame overlap (on by default): a frame of rt_render_device that is plain -- no adaptive supersampling, no passes other than (0, 1) -- and
 * asks for no rt_stats (stats null, collect_stats 0), no hit ids and no sphere-mode lights, on a stream that is not capturing, runs every
 * launch but its last on an internal stream of the context and on one of TWO working sets, which consecutive such frames take in turn, so
 * that the latency-bound launches of one frame run beside the shading of the frame before it.  What a caller may rely on:
 *   - with overlap on, the internal work of such a frame may start before earlier work on the caller's stream has finished;
 *   - that work reads and writes context memory only (the resident scene, the working sets; camera, lights and parameters travel by value);
 *   - the frame's outputs are written by work on the caller's stream, in call order: whatever the caller enqueues on that stream behind the
 *     call sees the frame, and the frame overwrites its outputs only after what the caller enqueued there before.
 * Every other call that uses the working set (frames that do not qualify, rt_graph_launch, rt_trace_rays*, rt_render) first waits on its
 * stream for the overlapped frames in flight; rt_synchronize, rt_upload_scene and rt_destroy wait for them on the host.  The second working
 * set is allocated by the first frame that qualifies (the frame buffers of the context double); if both sets do not fit the device's
 * memory, or with on = 0 (and always in the counting build), every frame runs on the caller's stream alone as before.  Outputs are bit for bit the same either way.
 * (On the caller's stream alone, frames of one context on DIFFERENT streams share the one working set and are the caller's to order, as they
 * always were; overlapped frames are ordered among themselves by the sets they take.)
 * on = 2 is on = 1 without one exception: with 1 a frame that finds nothing in flight to run beside (the caller's stream has drained and
 * every earlier frame has finished: a caller that waits for each frame) runs on the caller's stream alone, which costs it no hop between
 * streams, and the frame behind it overlaps; with 2 such a frame takes the overlapped route too.
 * A null context is RT_ERR_INVALID.                                                                                                       */
rt_status rt_set_frame_overlap(rt_ctx *ctx, int32_t on);
/* how many frames of this context took the overlapped route so far (a frame with nothing in flight to run beside does not: the caller's
 * stream has drained and every earlier frame has finished -- it runs on the caller's stream alone, and the frame behind it overlaps)    */
rt_status rt_debug_overlapped_frames(rt_ctx *ctx, uint64_t *frames);
/* host only, no device: rect = {tx0, ty0, tx1, ty1}, the tiles [tx0, tx1) x [ty0, ty1) of a width x height frame that a frame of `cam`
 * over a scene whose root box is box[6] (min, max) would keep with the given sample settings (rt_set_supersampling, rt_set_lens'
 * aperture, shutter on / off, rt_set_passes); the whole frame {0, 0, ceil(width / 8), ceil(height / 8)} when nothing may be culled and
 * {0, 0, 0, 0} when the box is out of view or behind the camera.                                                                                          */
rt_status rt_debug_primary_rect(const rt_camera *cam, const float box[6], int32_t width, int32_t height, int32_t supersampling,
                                float lens_aperture, int32_t shutter_on, int32_t pass_first, int32_t pass_count, int32_t rect[4]);

/* replaces: Flyscene::traceRay called directly (debug ray, flyscene.cpp:286; unit parity).  n rays, origin/dir
 * [n*3]; every ray sees the scene lights.  out_rgb [n*3]; out_face/out_t optional (level-0 closest hit).          */
rt_status rt_trace_rays(rt_ctx *ctx, const rt_lights *lights, int32_t max_depth, int32_t n,
                        const float *origin, const float *dir, float *out_rgb, int32_t *out_face, float *out_t);

/* replaces: the computational part of Flyscene::createDebugRay / recursiveDebugRay (flyscene.cpp:241-430, 433-470; the cylinders, spheres
 * and console prints are GL / GUI and out of scope).  Level 0 starts at the screen point of the pixel with dir = (screen - centre).normalized();
 * every level records the closest hit of (pos, dir), the hit point p0 = pos + t * dir, the face normal, lightStrikes(p0, lights), the colour
 * traceRay returns for that ray, and continues along reflectedDir = dir - 2 * dir.dot(n) * n from p0 (flyscene.cpp:349), until a miss or
 * max_levels records.  (The reference re-uses the PRIMARY ray's root test and candidate set at every level and keeps negative t,
 * flyscene.cpp:247-259 -- a visualiser quirk that is not reproduced: each level here traces its own ray.)                              */
typedef struct rt_debug_hit {
    int32_t level;
    int32_t status;                 /* 0: the ray misses the root box (the reference draws it red), 1: box but no triangle (blue), 2: hit (green) */
    int32_t face;                   /* closest face id, -1 without a hit                                                          */
    float   t;
    float   pos[3], dir[3];         /* the ray of this level                                                                      */
    float   hit_point[3], normal[3], reflected[3], color[3];
    uint8_t light_visible[RT_MAX_LIGHTS];
    uint8_t pad[3];
} rt_debug_hit;
rt_status rt_debug_ray(rt_ctx *ctx, const rt_camera *cam, const rt_lights *lights, float pixel_x, float pixel_y, int32_t max_levels,
                       rt_debug_hit *out, int32_t *n_out);

/* replaces: Flyscene::lightStrikes (flyscene.cpp:912-954): n segments light[i] -> hit[i]; vis[i] = 1 iff visible.  Host pointers: it
 * allocates, uploads, enqueues rt_light_strikes_device (below) on the context's stream, synchronises that stream and downloads, so it has
 * that call's limit: n <= 715,827,882 (RT_ERR_INVALID above, before anything is allocated).                            */
rt_status rt_light_strikes(rt_ctx *ctx, int32_t n, const float *hit, const float *light, uint8_t *vis);

/* ---- device ray queries: closest hit, visibility and traced colour of caller-owned rays in device memory -----------------------------
 * No reference counterpart beyond traceRay / lightStrikes themselves: these are rt_trace_rays and rt_light_strikes, and the bare closest
 * hit inside traceRay, on buffers that stay on the GPU (Device ray queries).
 * Common rules.  Every d_* argument is a device pointer on the context's device.  Origins, directions and points are float[n*3], xyz per
 * ray, as rt_trace_rays takes them; a direction is used as given (not normalised).  `stream` is a hipStream_t, NULL = the context's own
 * stream (rt_stream).  A NULL context, n < 0, a NULL required pointer or an output range that shares a byte with an input range of the same
 * call is RT_ERR_INVALID; before rt_upload_scene every call returns RT_ERR_NO_SCENE.  n == 0 returns RT_OK and enqueues nothing.  Exactly
 * n elements of every output are written, nothing behind them.  The inputs are only read.
 *
 * rt_closest_hits_device: per ray the level-0 closest hit of traceRay(origin, dir) (flyscene.cpp:655-691): the root box is tested with
 *   boxIntersect(o, o + d); of the triangles of every leaf the ray's box walk reaches, the one with the smallest t > 0.00001 wins, ties to
 *   the lowest face id.  d_face[i] = its face id, d_t[i] = its t (the hit point is o + t * d); a ray that misses the root box or every
 *   triangle gives -1 / -1.0f.  These are the values rt_trace_rays returns in out_face / out_t, bit for bit.  It needs no lights and shades
 *   nothing.  d_face or d_t may be NULL, not both.  ASYNCHRONOUS: one kernel on `stream`, no allocation, no synchronisation, and none of
 *   the context's frame buffers: it reads the uploaded scene alone.  It is therefore ordered by its stream only -- any number of these
 *   calls may run beside frames and other queries -- and the caller orders it against rt_upload_scene (which replaces what it reads).
 * rt_closest_hits: the same with host pointers: it allocates, uploads, enqueues the call above on the context's stream, synchronises that
 *   stream and downloads.
 * rt_light_strikes_device: the kernel of rt_light_strikes on device buffers: d_vis[i] = 1 iff the segment d_light[i] -> d_hit[i] is
 *   visible (lightStrikes, flyscene.cpp:912-954).  Asynchronous and scene-only like rt_closest_hits_device, the same ordering rules.
 *   n <= 715,827,882 (RT_ERR_INVALID above).
 * rt_trace_rays_device: rt_trace_rays with rays and results in device memory: d_out_rgb[n*3] = the colour traceRay returns for ray i with
 *   `lights` and `max_depth` (as rt_trace_rays: < 0 = RT_MAX_DEPTH, above RT_MAX_DEPTH = RT_ERR_UNSUPPORTED); d_out_face / d_out_t (either
 *   may be NULL) the level-0 closest hit as above.  Every value is bit for bit what rt_trace_rays returns for the same rays.
 *   The batch runs in chunks of at most rt_set_query_chunk rays, one launch sequence each, in order on `stream`, so a batch of any n
 *   needs the working set of one chunk (rt_trace_rays sizes its working set by n and returns RT_ERR_UNSUPPORTED when that exceeds the
 *   device).  The result does not depend on the chunk size.
 *   It uses the context's working set (ray lists, control block), as a frame does, so its stream rules are rt_render_device's: it becomes
 *   the context's latest frame stream, rt_synchronize waits for it and reports a work-list overflow, and calls that use the working set
 *   (frames, graph replays, rt_trace_rays, this call) on DIFFERENT streams are ordered by the caller.  ASYNCHRONOUS except where the working
 *   set has to grow (that synchronises, reallocates and invalidates captured graphs exactly as a larger frame or rt_trace_rays does), where
 *   sphere lights upload their offsets, and where the refined count of an adaptive frame still has to be fetched from the control block
 *   (rt_supersampling_refined keeps reporting that frame's count afterwards).  Errors found after some chunks were enqueued leave those
 *   chunks' results written.
 * rt_set_query_chunk: rays per chunk of later rt_trace_rays_device calls, 64 <= rays <= 16,777,216 (2^24); anything else is
 *   RT_ERR_INVALID and keeps the setting.  Default 4,194,304 (2^22): a launch sequence has a fixed cost, so larger chunks are faster
 *   (DESIGN.md 6 has the sweep) and cost memory: about 0.5 KB per ray of a chunk at RT_MAX_DEPTH with one light of up to 64 samples.  */
rt_status rt_closest_hits_device(rt_ctx *ctx, int32_t n, const float *d_origin, const float *d_dir, int32_t *d_face, float *d_t, void *stream);
rt_status rt_closest_hits(rt_ctx *ctx, int32_t n, const float *origin, const float *dir, int32_t *face, float *t);
rt_status rt_light_strikes_device(rt_ctx *ctx, int32_t n, const float *d_hit, const float *d_light, uint8_t *d_vis, void *stream);
rt_status rt_trace_rays_device(rt_ctx *ctx, const rt_lights *lights, int32_t max_depth, int32_t n, const float *d_origin, const float *d_dir,
                               float *d_out_rgb, int32_t *d_out_face, float *d_out_t, void *stream);
rt_status rt_set_query_chunk(rt_ctx *ctx, int32_t rays);

/* ---- ambient occlusion: how much of the cosine-weighted hemisphere above a point is open, from points in device memory ----------------
 * No reference counterpart beyond lightStrikes itself: per point, K = m * m segments of length `radius` are tested for visibility exactly
 * as lightStrikes tests a light sample, and the answer is the integer count of the visible ones (Ambient occlusion).  This
 * section is the DEFINITION; tests/ao_ref.py restates it in numpy float32.  All device arithmetic is float32, every operation rounded on
 * its own, no FMA, in exactly the order written.
 *   Directions: rt_ao_directions(m, out[m*m*3]), 1 <= m <= RT_AO_MAX_GRID, host only, in double: direction k belongs to the cell centre
 *            (x, y) = ((k % m + 0.5) / m, (k / m + 0.5) / m); (a, b) is its Shirley-Chiu concentric-disc image by exactly the rule of
 *            rt_lens_table (u = 2x - 1, v = 2y - 1); z = sqrt(max(0, 1 - a*a - b*b)); the entry is ((float)a, (float)b, (float)z): the
 *            cosine-weighted hemisphere about +z (Malley's method).  Cell centres never reach the rim: z >= 0.3479 even for m = 16.
 *            As float bits (x y z): m = 1, k = 0: 00000000 00000000 3F800000; m = 2, k = 0: BEB504F3 BEB504F3 3F5DB3D7;
 *            m = 3, k = 5: 3F2AAAAB 00000000 3F3ECFA6; m = 4, k = 7: 3F397530 BE46C5E5 3F2953FD; m = 16, k = 255: 3F29B4A4 3F29B4A4 3EB22B20.
 *   Rotation: rt_ao_rotation(seed, i, &r, &c, &s), host only: h = (i * 0x9E3779B1) ^ (seed * 0x85EBCA6B) in uint32, then the mixing of step
 *            3 of rt_set_lens (h ^= h >> 15; h *= 0x2C1B3C6D; h ^= h >> 12; h *= 0x297A2D39; h ^= h >> 15); r = h >> 26; in double the angle
 *            is (pi / 2) * r / RT_AO_ROTATIONS, c = (float)cos(angle), s = (float)sin(angle).  The concentric grid is symmetric under
 *            quarter turns, so the 64 steps inside one quarter turn are 64 different patterns.  i is the point's index in the call.
 *            (seed, i) -> h (r): (0, 0) 00000000 (0); (0, 1) 205F0435 (8); (7, 5) 93F76A67 (36); (0xFFFFFFFF, 0xFFFFFFFF) 1DEC3226 (7).
 *            r -> (c, s) as bits: 1: 3F7FEC43 3CC90AB0; 17: 3F6A09A7 3ECF7BCA; 63: 3CC90AB0 3F7FEC43.
 *   Point i, position P, normal N (used as given: the caller passes unit normals):
 *            No point: all three components of N are +-0: open = K, ao = 1.0f, no segment is formed.
 *            Frame (the branchless basis of Duff et al.): sg = copysignf(1.0f, Nz); a = -1.0f / (sg + Nz), a correctly rounded division;
 *            b = (Nx*Ny)*a; T = (1.0f + (sg*(Nx*Nx))*a, sg*b, -(sg*Nx)); B = (b, sg + (Ny*Ny)*a, -Ny).
 *            Direction k, (x, y, z) its table entry, (c, s) of rt_ao_rotation(seed, i): xr = c*x - s*y, yr = s*x + c*y (two products, then
 *            one subtraction or addition); per component q: d_q = ((xr*T_q) + (yr*B_q)) + (z*N_q); far end Q_q = P_q + radius*d_q.
 *            vis_k = 1 exactly when the segment Q -> P is visible as lightStrikes defines it (flyscene.cpp:912-954): the value
 *            rt_light_strikes returns for light = Q, hit = P, bit for bit.  lightStrikes ignores hits with t >= 0.98, so the last 2 % of
 *            the segment next to P cannot block it: that is the self-intersection guard, no epsilon is added.
 *            open = sum of vis_k (0 .. K) as uint16_t; ao = (float)open / (float)K, a correctly rounded division.
 * rt_ambient_occlusion_device: d_point, d_normal float[n*3]; d_open uint16_t[n], d_ao float[n]: either may be NULL, not both.  The common
 *   rules of the device ray queries above hold (device pointers, NULL context / n < 0 / NULL required pointer / an output sharing a byte
 *   with an input: RT_ERR_INVALID; RT_ERR_NO_SCENE before rt_upload_scene; n == 0: RT_OK, nothing enqueued; exactly n elements written);
 *   m outside 1 .. RT_AO_MAX_GRID or a radius that is not finite and > 0: RT_ERR_INVALID.  n * K may exceed 2^31.  Scene-only and
 *   ASYNCHRONOUS like rt_closest_hits_device: one kernel on `stream`, none of the context's frame buffers, ordered by its stream only, and
 *   the caller orders it against rt_upload_scene.  THE ONE EXCEPTION: the first call on a context allocates the direction and rotation tables
 *   (under 20 KB) and uploads them with a synchronous copy; they are freed by rt_destroy.
 * rt_ambient_occlusion: the same with host pointers: it allocates, uploads, enqueues the call above on the context's stream, synchronises
 *   that stream and downloads.
 * rt_hit_points_device: closest hits (rt_closest_hits_device's d_face, d_t, with the rays that gave them) -> occlusion inputs.  With
 *   f = d_face[i] in [0, n_faces): P_q = o_q + t*d_q (multiply, then add, as flyscene.cpp:695); N = face_normal[f] as uploaded, its three
 *   sign bits flipped when (Nx*dx + Ny*dy) + Nz*dz > 0, so that it faces the ray.  Any other f (a miss) writes six 0.0f -- a "no point".
 *   All four inputs and both outputs are required.  Scene-only and asynchronous, one kernel on `stream`, no allocation.                      */
#define RT_AO_MAX_GRID 16
#define RT_AO_ROTATIONS 64
rt_status rt_ambient_occlusion_device(rt_ctx *ctx, int32_t n, const float *d_point, const float *d_normal, int32_t m, float radius,
                                      uint32_t seed, uint16_t *d_open, float *d_ao, void *stream);
rt_status rt_ambient_occlusion(rt_ctx *ctx, int32_t n, const float *point, const float *normal, int32_t m, float radius, uint32_t seed,
                               uint16_t *open, float *ao);
rt_status rt_hit_points_device(rt_ctx *ctx, int32_t n, const float *d_origin, const float *d_dir, const int32_t *d_face, const float *d_t,
                               float *d_point, float *d_normal, void *stream);
rt_status rt_ao_directions(int32_t m, float *out);
rt_status rt_ao_rotation(uint32_t seed, uint32_t i, int32_t *r, float *c, float *s);

/* ---- soft shadows: how much of every area light a point sees, from points in device memory -------------------------------------------------
 * No reference counterpart beyond lightStrikes and the sample grid of createSpherePoint / arealight.hpp: per point, the K = n_lights * N
 * segments from every sample of every light to the point are tested for visibility exactly as lightStrikes tests them, and the answer is
 * the integer count of the visible ones (Soft shadows) -- the lit share a deferred shader, a light map or a vertex bake needs,
 * without the Phong colour, reflections and refractions a frame bakes it into.  This section is the DEFINITION; tests/shadow_ref.py restates
 * it in numpy float32.  All device arithmetic is float32, every operation rounded on its own, no FMA, in exactly the order written.
 *   Samples: rt_light_samples(l, light, fu, fv, out[N*3]), host only.  RT_LIGHT_AREA: N = usteps * vsteps; sample s = i * vsteps + j of light
 *            `light`, whose position is c = pos[light], in the order of the frames' own sample grid:
 *              cx = (c.x + len_x * 1.0f) / (float)usteps;   cy = (c.y + len_y * 1.0f) / (float)vsteps;   z = c.z + len_x * 0.0f;
 *              fi = (float)i + fu;   fj = (float)j + fv;   S = (fi * cx, fj * cy, z).
 *            With (fu, fv) = (0.5f, 0.5f) that is the sample of every frame in every bit; with rt_light_jitter_offsets(p) it is the sample
 *            that section defines (tests/light_jitter_ref.py restates both).  RT_LIGHT_POINT: N = 1, S = pos[light], fu and fv are not looked
 *            at.  RT_LIGHT_SPHERE: RT_ERR_UNSUPPORTED (its offsets need a synchronous upload, and the device call stays asynchronous).  A NULL
 *            pointer, lights that rt_render would refuse or a light index outside [0, n_lights): RT_ERR_INVALID.
 *   Per-point jitter: rt_shadow_jitter(seed, i, &fu, &fv), host only: h = the hash of rt_ao_rotation(seed, i); g = h ^ 0xB5297A4D; then the
 *            same mixing once more (g ^= g >> 15; g *= 0x2C1B3C6D; g ^= g >> 12; g *= 0x297A2D39; g ^= g >> 15); fu = (float)(g >> 16) * 2^-16,
 *            fv = (float)(g & 0xFFFF) * 2^-16: both exact, both in [0, 1).  i is the point's index in the call.
 *            (seed, i) -> g, fu, fv (floats as bits): (0, 0) 31315BDB 3E44C400 3EB7B600; (0, 1) 977B0A53 3F177B00 3D253000;
 *            (7, 5) B6706ADC 3F367000 3ED5B800; (0xFFFFFFFF, 0xFFFFFFFF) 888E5787 3F088E00 3EAF0E00; (3, 2073599) 43D51905 3E87AA00 3DC82800.
 *   Parameters: rt_shadow_params.  per_point == 0: every point uses (fu, fv), 0 <= fu, fv < 1 (anything else, NaN included, is
 *            RT_ERR_INVALID).  per_point != 0: point i uses rt_shadow_jitter(seed, i) and (fu, fv) are ignored.  A grid all points share
 *            leaves N + 1 brightness levels per light in a penumbra; a grid of the point's own turns the bands into noise that
 *            rt_denoise_device removes (DESIGN.md 6 has the figures, and the scene where it does not help).
 *   Point i, position P: segment e = l * N + s runs from sample s of light l to P; vis_e = 1 exactly when it is visible as lightStrikes
 *            defines it (flyscene.cpp:912-954): the value rt_light_strikes returns for light = S, hit = P, bit for bit.
 *            visible = sum of vis_e (0 .. K, K <= 25,600) as uint16_t; share = (float)visible / (float)K, a correctly rounded division.
 *            d_normal may be NULL: every point is a point.  Given, a normal whose three components are all +-0 means "no point" -- the six
 *            zeros rt_hit_points_device writes for a miss: visible = K, share = 1.0f, no segment is formed.  The normal is used for nothing
 *            else: no facing test, no cosine.  The centre-ray rule of traceRay (a hit none of whose light POSITIONS is visible is black,
 *            flyscene.cpp:699-712) is not part of this call; rt_light_strikes_device answers it.
 * rt_soft_shadows_device: d_point, d_normal float[n*3]; d_visible uint16_t[n], d_share float[n]: either may be NULL, not both.  The common
 *   rules of the device ray queries above hold (device pointers, NULL context / lights / sp / d_point, n < 0, an output sharing a byte with
 *   an input: RT_ERR_INVALID; RT_ERR_NO_SCENE before rt_upload_scene; n == 0: RT_OK, nothing enqueued; exactly n elements written); the
 *   lights are checked as rt_render checks them.  n * K may exceed 2^31.  Scene-only and ASYNCHRONOUS like rt_closest_hits_device: ONE kernel
 *   on `stream`, the lights travel by value as its argument, no table, no allocation and no synchronous copy on the first call or any other,
 *   none of the context's buffers: it is ordered by its stream only, runs beside frames and other queries, leaves rt_supersampling_refined,
 *   rt_pass_map and every later frame as they were, and the caller orders it against rt_upload_scene.
 * rt_soft_shadows: the same with host pointers: it allocates, uploads, enqueues the call above on the context's stream, synchronises that
 *   stream and downloads.
 * rt_default_shadow_params: {0, 0, 0.5f, 0.5f}, the samples of every frame.                                                                 */
typedef struct rt_shadow_params {
    int32_t  per_point;   /* 0: every point uses (fu, fv); != 0: point i uses rt_shadow_jitter(seed, i) and (fu, fv) are ignored */
    uint32_t seed;
    float    fu, fv;      /* 0 <= fu, fv < 1; (0.5f, 0.5f) = the samples of every frame                                        */
} rt_shadow_params;
void      rt_default_shadow_params(rt_shadow_params *sp);
rt_status rt_shadow_jitter(uint32_t seed, uint32_t i, float *fu, float *fv);
rt_status rt_light_samples(const rt_lights *l, int32_t light, float fu, float fv, float *out);
rt_status rt_soft_shadows_device(rt_ctx *ctx, const rt_lights *lights, int32_t n, const float *d_point, const float *d_normal,
                                 const rt_shadow_params *sp, uint16_t *d_visible, float *d_share, void *stream);
rt_status rt_soft_shadows(rt_ctx *ctx, const rt_lights *lights, int32_t n, const float *point, const float *normal,
                          const rt_shadow_params *sp, uint16_t *visible, float *share);

/* ---- indirect diffuse: the light that reaches a point after one diffuse bounce off the rest of the scene, from points in device memory ------
 * No reference counterpart beyond traceRay's closest hit, lightStrikes and the diffuse term of the Phong shading: per point, K = m * m
 * cosine-weighted gather rays are traced to their closest hits, each hit is lit by the light POSITIONS it sees, diffuse term only, and the
 * answer is the mean of those radiances (Indirect diffuse) -- colour bleeding, a "final gather".  This section is the
 * DEFINITION; tests/indirect_ref.py restates it in numpy float32.  All device arithmetic is float32, every operation rounded on its own, no
 * FMA, every division and square root correctly rounded, in exactly the order written.  dot3(a, b) = a0*b0 + (a1*b1 + a2*b2);
 * normalized(v) is Eigen's: q = dot3(v, v); if q > 0, s = sqrtf(q) and v / s per component; otherwise v as it is.
 *   Point i, position P, normal N (used as given), K = m * m, 1 <= m <= RT_AO_MAX_GRID:
 *            No point: all three components of N are +-0 (the six zeros rt_hit_points_device writes for a miss): out = (+0.0f, +0.0f, +0.0f),
 *            no ray is formed.
 *            Gather ray k = 0 .. K-1: its direction d is exactly the d_q of the ambient-occlusion section: the frame of Duff et al. from N,
 *            table entry k of rt_ao_directions(m), (c, s) of rt_ao_rotation(seed, i).  No radius is applied.  The ray is (origin P,
 *            direction d).
 *            Hit: (f, t) is what rt_closest_hits_device returns for that ray, bit for bit: the root test on (P, P + d), the smallest
 *            t > 0.00001, ties to the lowest face id.  The 0.00001 of traceRay is the only self-intersection guard, as it is for the
 *            reference's own bounce rays.  A miss contributes R = (0, 0, 0).
 *            Radiance of a hit: H_q = P_q + t * d_q (multiply, then add).  Nf = face_normal[f] as uploaded, its three sign bits flipped when
 *            (Nf.x*d.x + Nf.y*d.y) + Nf.z*d.z > 0 (the rule of rt_hit_points_device).  kd = materials[mat_id[f]].kd.  R_c = 0.0f; for
 *            light l = 0 .. n_lights-1 in order: vis = 1 exactly when rt_light_strikes says so for light = pos[l], hit = H (the centre
 *            segment, the one traceRay tests at flyscene.cpp:699-712; the area-light samples are not part of this call); if visible:
 *            ld = normalized(pos[l] - H); ldn = dot3(ld, Nf); ct = (0.0f < ldn) ? ldn : 0.0f (std::max(0.0f, ldn): NaN and -0 give +0);
 *            R_c = R_c + (color_c * kd_c) * ct (two products, then the addition).
 *            Point: E_c = 0.0f; for k = 0 .. K-1 in order, E_c = E_c + R_c(k); out_c = E_c / (float)K.
 *            The directions are cosine-weighted, so out is the mean radiance over the hemisphere with the cosine and 1/pi already cancelled:
 *            a Lambert surface at P sends back kd(P) * out, and the caller multiplies by its own albedo (G[5..7] / G[0] of the geometry
 *            buffers, for example).  Misses add nothing, so a convex scene gives exact zeros.
 * rt_indirect_diffuse_device: d_point, d_normal float[n*3]; d_rgb float[n*3].  The common rules of the device ray queries above hold (device
 *   pointers, NULL context / lights / pointer, n < 0, an output sharing a byte with an input: RT_ERR_INVALID; RT_ERR_NO_SCENE before
 *   rt_upload_scene; n == 0: RT_OK, nothing enqueued; exactly n * 3 floats written); m outside 1 .. RT_AO_MAX_GRID: RT_ERR_INVALID; the lights
 *   are checked as rt_render checks them, and RT_LIGHT_SPHERE is RT_ERR_UNSUPPORTED as in rt_soft_shadows_device; mode, usteps, vsteps, len_x
 *   and len_y are otherwise not looked at: only n_lights, pos and color are used.  n * K may exceed 2^31.  Scene-only and ASYNCHRONOUS like
 *   rt_closest_hits_device: ONE kernel on `stream`, the lights travel by value as its argument, none of the context's frame buffers: it is
 *   ordered by its stream only, leaves rt_supersampling_refined, rt_pass_map and every later frame as they were, and the caller orders it
 *   against rt_upload_scene.  THE ONE EXCEPTION is that of rt_ambient_occlusion_device: the first call of either kind on a context allocates
 *   and uploads the direction and rotation tables synchronously; the two calls share that one table set.
 * rt_indirect_diffuse: the same with host pointers: it allocates, uploads, enqueues the call above on the context's stream, synchronises that
 *   stream and downloads.                                                                                                                   */
rt_status rt_indirect_diffuse_device(rt_ctx *ctx, const rt_lights *lights, int32_t n, const float *d_point, const float *d_normal,
                                     int32_t m, uint32_t seed, float *d_rgb /* n*3 */, void *stream);
rt_status rt_indirect_diffuse(rt_ctx *ctx, const rt_lights *lights, int32_t n, const float *point, const float *normal,
                              int32_t m, uint32_t seed, float *rgb);

/* ---- light probes: the light arriving at points in free space as 9 spherical-harmonic coefficients per channel, and their lookup ----------
 * No reference counterpart beyond traceRay's closest hit, lightStrikes and the diffuse term of the Phong shading: an irradiance volume
 * (Light probes).  rt_light_probes_device traces and stores probes; rt_probe_irradiance_device blends the 8 probes of a regular
 * grid round a point and evaluates the blend at the point's normal, without a ray.  This section is the DEFINITION; tests/probe_ref.py
 * restates it in numpy float32.  All device arithmetic is float32, every operation rounded on its own, no FMA, every division and square
 * root correctly rounded, in exactly the order written.  dot3, normalized and smax (std::max) are those of the indirect-diffuse section.
 *   Tables (host, computed in double, stored as float), K = m * m, 1 <= m <= RT_AO_MAX_GRID:
 *     rt_probe_directions(m, out[K*3]): cell centre of direction k: x = (k % m + 0.5) / m, y = (k / m + 0.5) / m; z = 1 - 2y;
 *            r = sqrt(max(0, 1 - z*z)); phi = 2 pi x; entry k = ((float)(r cos phi), (float)(r sin phi), (float)z): the equal-area,
 *            stratified map of the unit square to the whole sphere.  No per-probe rotation and no seed: all probes share the set.
 *     rt_probe_weights(m, out[K*9]): with (x, y, z) the FLOAT entry k promoted to double and the real SH basis in double,
 *            Y0 = 0.5 sqrt(1/pi); Y1 = sqrt(3/(4pi)) y, Y2 = sqrt(3/(4pi)) z, Y3 = sqrt(3/(4pi)) x; Y4 = 0.5 sqrt(15/pi) xy,
 *            Y5 = 0.5 sqrt(15/pi) yz, Y6 = 0.25 sqrt(5/pi) (3zz - 1), Y7 = 0.5 sqrt(15/pi) xz, Y8 = 0.25 sqrt(15/pi) (xx - yy):
 *            W[k][j] = (float)((4 pi / K) * a_j * Y_j), a = 1, 2/3, 2/3, 2/3, 1/4, 1/4, 1/4, 1/4, 1/4 -- the clamped-cosine convolution
 *            divided by pi, so a stored coefficient is already "irradiance / pi", the unit of rt_indirect_diffuse_device: a Lambert surface
 *            sends back kd * out.
 *     rt_sh9(n[3], out[9]): the float32 basis, the only one the device evaluates: c0 = 0.282094792f, c1 = 0.488602512f, c2 = 1.092548431f,
 *            c3 = 0.315391565f, c4 = 0.546274215f; out = (c0, c1*y, c1*z, c1*x, c2*(x*y), c2*(y*z), c3*((3.0f*(z*z)) - 1.0f), c2*(x*z),
 *            c4*((x*x) - (y*y))).
 *     Recorded (float bits): rt_probe_directions(2): entry 0 = 24748d50 3f5db3d7 3f000000, entry 1 = a53769fc bf5db3d7 3f000000;
 *            rt_probe_weights(2): entry 0 = 3f62dfc5 3f62dfc4 3f02fc5f 247a41b0 2435bb80 3ebe3d5d bd7da728 23d1d8b6 bea4c09e;
 *            rt_probe_directions(16): entry 37 = bece9088 3f1a92a7 3f300000; rt_probe_weights(16): entry 37 = 3c62dfc5 3c1e2db5 3c341b02
 *            bbd3620f bb560c1a 3bb66021 3ad409bb bb73b807 bab15293; rt_sh9((0.6f, 0, 0.8f)) = 3e906ebb 00000000 3ec821b0 3e961944 00000000
 *            00000000 3e948fe3 3f06409b 3e4960e8.
 *   Probe i at P (rt_light_probes_device), coefficient j, channel c at d_coeff[i*27 + j*3 + c]:
 *            Ray k = 0 .. K-1: origin P, direction d_k, the table entry as it is.  Its hit (f, t) is what rt_closest_hits_device returns for
 *            that ray, bit for bit.  Its radiance R(k) is the indirect-diffuse section's "radiance of a hit", word for word (H = P + t*d, Nf
 *            flipped against d, kd of the face's material, the lights in order, the centre segment judged by lightStrikes,
 *            R_c = R_c + (color_c*kd_c)*ct); a miss gives (0, 0, 0).
 *            C[j][c] = +0.0f; for k = 0 .. K-1 in order, for every j and c: C[j][c] = C[j][c] + R_c(k) * W[k][j] (one product, then the
 *            addition).
 *            If direct != 0, after that sum, for light l = 0 .. n_lights-1 in order: the light counts if rt_light_strikes calls the segment
 *            light = pos[l], hit = P visible; w = normalized(pos[l] - P); Yw = rt_sh9(w); C[j][c] = C[j][c] + color_c * (b_j * Yw_j) with
 *            b = 3.14159274f, 2.09439510f (x3), 0.785398163f (x5): the light itself as a delta, so that out(n) approximates
 *            color * max(0, n.w), the reference's own diffuse term without falloff.  The order-2 expansion gives 1.0625 at n = w and rings
 *            to about 0.06 behind.
 *   rt_probe_grid: dims >= 1, dims[0]*dims[1]*dims[2] <= 2^24, every step finite and > 0, anything else RT_ERR_INVALID.  Probe (ix, iy, iz)
 *            has index (iz*dims[1] + iy)*dims[0] + ix and position origin_q + (float)i_q * step_q; rt_probe_grid_positions writes them (host).
 *   Point i, position P, normal N (rt_probe_irradiance_device):
 *            1. All three components of N +-0: no point; three +0.0f are written and nothing is read.
 *            2. Per axis q: g = (P_q - origin_q) / step_q; g = smax(0.0f, g) (NaN gives 0); if g > (float)(dims_q - 1) it takes that value;
 *               i0 = (int)g, lowered to max(dims_q - 2, 0) if above it; f = g - (float)i0; w0 = 1.0f - f, w1 = f.  dims_q == 1 gives i0 = 0,
 *               w0 = 1, w1 = 0, and only the near corner of that axis is read.
 *            3. Corners in the order (dz, dy, dx), dx fastest, 0 before 1; weight = (wz*wy)*wx.
 *            4. B[j][c] = +0.0f, then B[j][c] = B[j][c] + weight * C[corner][j][c], corner after corner; a corner whose index repeats
 *               because dims_q == 1 is skipped on that axis.
 *            5. Y = rt_sh9(N); out_c = +0.0f, then for j = 0 .. 8 in order out_c = out_c + B[j][c] * Y[j].
 *            The blend is plainly trilinear: no visibility weighting, so light leaks through walls thinner than a grid step
 *            (rt_probe_irradiance_visible_device, the next section, asks the scene which probes the point sees).
 * rt_light_probes_device: d_position float[n*3]; d_coeff float[n*27].  The common rules of the device ray queries above hold (device
 *   pointers, NULL context / lights / pointer, n < 0, an output sharing a byte with the input: RT_ERR_INVALID; RT_ERR_NO_SCENE before
 *   rt_upload_scene; n == 0: RT_OK, nothing enqueued; exactly n * 27 floats written); m outside 1 .. RT_AO_MAX_GRID: RT_ERR_INVALID; the lights
 *   are checked as rt_render checks them, and RT_LIGHT_SPHERE is RT_ERR_UNSUPPORTED as in rt_indirect_diffuse_device.  n * K may exceed 2^31.
 *   Scene-only and ASYNCHRONOUS: ONE kernel on `stream`, the lights travel by value as its argument, none of the context's frame buffers: it
 *   leaves rt_supersampling_refined, rt_pass_map and every later frame as they were.  THE ONE EXCEPTION: the first call on a context allocates
 *   and uploads the two probe tables synchronously (all m back to back, about 72 KB); rt_destroy frees them.
 * rt_probe_irradiance_device: d_coeff float[dims product * 27] (an input); d_point, d_normal, d_rgb float[n*3].  One element-wise kernel on
 *   `stream`; it needs no scene, no scratch and none of the context's buffers.  NULL context / grid / pointer, a bad grid, n < 0, d_rgb
 *   sharing a byte with an input: RT_ERR_INVALID; n == 0: RT_OK, nothing enqueued.
 * rt_light_probes, rt_probe_irradiance: the same with host pointers: they allocate, upload, enqueue the call above on the context's stream,
 *   synchronise that stream and download.                                                                                                   */
#define RT_PROBE_COEFFS 27
typedef struct rt_probe_grid {
    float origin[3];
    float step[3];
    int32_t dims[3];
} rt_probe_grid;
rt_status rt_probe_directions(int32_t m, float *out /* m*m*3 */);
rt_status rt_probe_weights(int32_t m, float *out /* m*m*9 */);
rt_status rt_sh9(const float n[3], float out[9]);
rt_status rt_probe_grid_positions(const rt_probe_grid *grid, float *out /* dims product * 3 */);
rt_status rt_light_probes_device(rt_ctx *ctx, const rt_lights *lights, int32_t n, const float *d_position, int32_t m, int32_t direct,
                                 float *d_coeff /* n*27 */, void *stream);
rt_status rt_light_probes(rt_ctx *ctx, const rt_lights *lights, int32_t n, const float *position, int32_t m, int32_t direct, float *coeff);
rt_status rt_probe_irradiance_device(rt_ctx *ctx, const rt_probe_grid *grid, const float *d_coeff, int32_t n, const float *d_point,
                                     const float *d_normal, float *d_rgb /* n*3 */, void *stream);
rt_status rt_probe_irradiance(rt_ctx *ctx, const rt_probe_grid *grid, const float *coeff, int32_t n, const float *point, const float *normal,
                              float *rgb);

/* ---- leak-free probe lookup: the blend of rt_probe_irradiance_device over the probes the point can SEE -------------------------------------
 * No reference counterpart beyond lightStrikes: each of the (at most) 8 probes round a point is asked, with one exact segment walk, whether
 * the point sees it, and the blend takes the visible ones alone, renormalised (Leak-free probe lookup).  This section is the
 * DEFINITION; tests/probe_visible_ref.py restates it in numpy float32.  The arithmetic rules are those of the light-probe section: float32,
 * every operation rounded on its own, no FMA, every division correctly rounded, in exactly the order written.
 *   Point i, position P, normal N:
 *            1. No point: all three components of N +-0: three +0.0f and mask 0 are written; nothing is read and no segment is formed.
 *            2. Cell: per axis q, g, i0, f, w0, w1 exactly as step 2 of rt_probe_irradiance_device.
 *            3. Corners in the order (dz, dy, dx), dx fastest, 0 before 1; corner b = 4*dz + 2*dy + dx has weight_b = (wz*wy)*wx.  A corner
 *               whose index repeats because dims_q == 1 is not read, as in the plain lookup; its mask bit stays 0.
 *            4. Visibility, for every corner that is read, a corner of weight 0 included: the probe's position is Pc_q = origin_q +
 *               (float)i_q * step_q (the floats of rt_probe_grid_positions); vis_b = 1 exactly when rt_light_strikes calls the segment
 *               light = Pc, hit = P visible: the judgement the frames' shadow segments get, with the same near-hit cut-off and the same
 *               illum 9 faces that never occlude.  Bit b of mask[i] is vis_b.
 *            5. Case A.  Call a read corner USED when it is visible and weight_b > 0.0f.  When every read corner is visible, or when no
 *               corner is USED, the output is steps 4 and 5 of rt_probe_irradiance_device over all read corners, bit for bit: in open space
 *               the two calls agree in every bit, and a point that sees none of its probes falls back to the plain blend, not to black.
 *            6. Case B, every other case: W = +0.0f, B[j][c] = +0.0f; for the USED corners in order W = W + weight_b and B[j][c] = B[j][c] +
 *               weight_b * C[corner][j][c]; Y = rt_sh9(N); s_c = +0.0f, then s_c = s_c + B[j][c] * Y[j] for j = 0 .. 8 in order;
 *               out_c = s_c / W.
 *            A NaN position takes cell 0, as in the plain lookup; its segments are whatever rt_light_strikes says of them.
 *   NOT covered: probes behind the point's tangent plane are not weighted down, and a wall ONE polygon thick still leaks: its only occluder
 *            lies at the end of the segment, where lightStrikes' near-hit cut-off ignores it.  A partition with two faces and some depth
 *            between them (above the cut-off) is held exactly.
 * rt_probe_irradiance_visible_device: d_coeff float[dims product * 27] (an input); d_point, d_normal, d_rgb float[n*3]; d_mask uint8[n] or NULL.
 *   The common rules of the device ray queries hold: device pointers; NULL context / grid / pointer other than d_mask, a bad grid, n < 0,
 *   d_rgb or d_mask sharing a byte with an input or with each other: RT_ERR_INVALID; RT_ERR_NO_SCENE before rt_upload_scene (unlike the plain
 *   lookup this call walks the scene); n == 0: RT_OK, nothing enqueued; exactly n*3 floats and, if asked for, n bytes are written.
 *   ASYNCHRONOUS: ONE kernel on `stream`, the grid travels by value as its argument; none of the context's frame buffers, no table upload: it
 *   leaves rt_supersampling_refined, rt_pass_map and every later frame as they were.
 * rt_probe_irradiance_visible: the same with host pointers: it allocates, uploads, enqueues the call above on the context's stream,
 *   synchronises that stream and downloads.                                                                                                 */
rt_status rt_probe_irradiance_visible_device(rt_ctx *ctx, const rt_probe_grid *grid, const float *d_coeff, int32_t n, const float *d_point,
                                             const float *d_normal, float *d_rgb /* n*3 */, uint8_t *d_mask /* n, may be NULL */, void *stream);
rt_status rt_probe_irradiance_visible(rt_ctx *ctx, const rt_probe_grid *grid, const float *coeff, int32_t n, const float *point, const float *normal,
                                      float *rgb, uint8_t *mask /* may be NULL */);

/* ---- bounced light: the gather and the probes with a probe volume as a further light at every hit ------------------------------------------
 * No reference counterpart.  rt_indirect_diffuse_device and rt_light_probes_device light a hit by the light positions it sees and by nothing
 * else; here a hit is lit, in addition, by the irradiance that a SOURCE volume of probes gives at the hit.  Feeding a volume back into the
 * call that computes it adds one diffuse bounce per pass (Bounced light).  This section is the DEFINITION;
 * tests/probe_bounce_ref.py restates it in numpy float32.  Arithmetic: float32, every operation rounded on its own, no FMA, every division
 * correctly rounded, in exactly the order written.
 *   Source: an rt_probe_grid and its dims product * 27 coefficients in device memory, laid out as rt_light_probes_device writes them.
 *   The "radiance of a hit" of the indirect-diffuse section gets ONE more term behind the last light, for a ray that hit:
 *            I = the source looked up at position H with the normal Nf, the turned face normal of the hit:
 *              visible == 0: steps 1 to 5 of rt_probe_irradiance_device, word for word;
 *              visible != 0: steps 1 to 6 of rt_probe_irradiance_visible_device without the mask output: one rt_light_strikes judgement per
 *              read corner, light = the probe's position Pc, hit = H, then the same case A / case B rule.
 *            A face normal of three +-0 is "no point": I = (0, 0, 0) and no segment is formed.
 *            b_c = smax(0.0f, I_c) = (0.0f < I_c) ? I_c : 0.0f: an order-2 expansion rings negative, and negative light must not feed back;
 *            NaN gives +0.
 *            R_c = R_c + kd_c * b_c (one product, then the addition), c = 0, 1, 2.
 *            A miss still contributes (0, 0, 0) and performs no lookup.
 *   Everything else -- the directions, the hits, the order of every sum, the direct term of the probes, the division by K of the gather --
 *            is the definition of the parent call, word for word.  A source of all +0.0f gives the parent's output in every bit.
 *   THE SOURCE MUST BE A VOLUME COMPUTED WITHOUT `direct`: the light loop already lights the hit by the lights themselves, exactly, and a
 *            source that holds the light deltas would count them a second time.  The calls cannot check this.
 *   Feedback: pass 0 = rt_light_probes_device(direct = 0); pass b = rt_light_probes_bounce_device(direct = 0, source = pass b - 1) over the
 *            positions of the same grid; the caller's `direct` goes into the last pass alone.  An update in place would make a probe's answer
 *            depend on which probes had been stored already, so the output may not share a byte with the source: callers keep two buffers
 *            and swap them.
 * rt_light_probes_bounce_device, rt_indirect_diffuse_bounce_device: the arguments and the rules of the parent calls hold.  RT_ERR_INVALID in
 *   addition for a NULL or bad src_grid (the rule of rt_probe_grid, whatever n is), a NULL d_src_coeff and an output that shares a byte with
 *   the dims product * 27 floats of the source.  ONE kernel on `stream`, asynchronous and scene-only; the lights and the grid travel by value
 *   as its arguments; the only synchronous step is the parent's first-call table upload; none of the context's frame buffers: they leave
 *   rt_supersampling_refined, rt_pass_map and every later frame as they were.  RT_LIGHT_SPHERE is RT_ERR_UNSUPPORTED as in the parents.
 * rt_light_probes_bounce, rt_indirect_diffuse_bounce: the same with host pointers: they allocate, upload, enqueue the call above on the
 *   context's stream, synchronise that stream and download.                                                                                */
rt_status rt_light_probes_bounce_device(rt_ctx *ctx, const rt_lights *lights, int32_t n, const float *d_position, int32_t m, int32_t direct,
                                        const rt_probe_grid *src_grid, const float *d_src_coeff, int32_t visible, float *d_coeff /* n*27 */,
                                        void *stream);
rt_status rt_light_probes_bounce(rt_ctx *ctx, const rt_lights *lights, int32_t n, const float *position, int32_t m, int32_t direct,
                                 const rt_probe_grid *src_grid, const float *src_coeff, int32_t visible, float *coeff);
rt_status rt_indirect_diffuse_bounce_device(rt_ctx *ctx, const rt_lights *lights, int32_t n, const float *d_point, const float *d_normal,
                                            int32_t m, uint32_t seed, const rt_probe_grid *src_grid, const float *d_src_coeff, int32_t visible,
                                            float *d_rgb /* n*3 */, void *stream);
rt_status rt_indirect_diffuse_bounce(rt_ctx *ctx, const rt_lights *lights, int32_t n, const float *point, const float *normal, int32_t m,
                                     uint32_t seed, const rt_probe_grid *src_grid, const float *src_coeff, int32_t visible, float *rgb);

/* ---- closest points: how far a point is from the scene, and which face is nearest ----------------------------------------------------------
 * No reference counterpart: the point query beside the ray queries (Closest points).  This section is the DEFINITION;
 * tests/closest_point_ref.py restates it in numpy float32.  Arithmetic: float32, every operation rounded on its own, no FMA, every division
 * correctly rounded, in exactly the order written; dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z.
 *   The scene of the query: the faces that at least one leaf of the uploaded tree references -- the faces a ray can ever hit.  A face the
 *            builder lost (rt_host_scene_info counts them) is not part of it.  Illum flags play no role.
 *   Point to triangle, rt_closest_point_triangle (host only): P, triangle (A, B, C) = tri[0..2], tri[3..5], tri[6..8], the world-space
 *            vertices of rt_scene.tri_verts as uploaded.  The Voronoi-region walk of Ericson, Real-Time Collision Detection, 5.1.5:
 *              ab = B - A; ac = C - A; ap = P - A; d1 = dot(ab, ap); d2 = dot(ac, ap)
 *              region A:    d1 <= 0 and d2 <= 0                          Q = A
 *              bp = P - B; d3 = dot(ab, bp); d4 = dot(ac, bp)
 *              region B:    d3 >= 0 and d4 <= d3                         Q = B
 *              vc = d1*d4 - d3*d2
 *              region AB:   vc <= 0 and d1 >= 0 and d3 <= 0              v = d1 / (d1 - d3);  Q = A + ab*v
 *              cp = P - C; d5 = dot(ab, cp); d6 = dot(ac, cp)
 *              region C:    d6 >= 0 and d5 <= d6                         Q = C
 *              vb = d5*d2 - d1*d6
 *              region AC:   vb <= 0 and d2 >= 0 and d6 <= 0              w = d2 / (d2 - d6);  Q = A + ac*w
 *              va = d3*d6 - d5*d4
 *              region BC:   va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0   w = (d4 - d3) / ((d4 - d3) + (d5 - d6));  Q = B + (C - B)*w
 *              face:        den = 1 / ((va + vb) + vc); v = vb*den; w = vc*den;  Q = (A + ab*v) + ac*w
 *            The first region whose test holds is taken (a comparison with NaN does not hold); a vertex region returns the vertex's own
 *            floats.  e = P - Q; *d2 = dot(e, e).  q or d2 may be NULL, not both; a NULL p or tri: RT_ERR_INVALID.
 *   Point i, P = d_point_in[i*3..], search radius max_dist (+inf: unbounded): r2 = max_dist*max_dist.  The candidates are the faces of the
 *            query's scene whose computed d2 <= r2 (a NaN d2 is never one).  The answer is the candidate with the smallest d2, ties to the
 *            lowest face id: d_face[i] = its id (-1: no candidate), d_dist2[i] = its d2 (+inf: none), d_point[i*3..] = its Q (P itself:
 *            none).  A minimum over a set: the result equals brute force over the referenced faces in every bit, whatever the traversal.
 * rt_closest_points_device: d_point_in, d_point float[n*3], d_face int32[n], d_dist2 float[n]; any of the three outputs may be NULL, not all.
 *   The common rules of the device ray queries hold: device pointers; NULL context / input, n < 0, an output sharing a byte with the input
 *   or with another output, max_dist NaN or negative: RT_ERR_INVALID; RT_ERR_NO_SCENE before rt_upload_scene; n == 0: RT_OK, nothing
 *   enqueued; exactly n elements of each output are written; element indices are 64-bit.  ASYNCHRONOUS: ONE kernel on `stream`, ordered by
 *   that stream alone; none of the context's frame buffers: it leaves rt_supersampling_refined, rt_pass_map and every later frame as they
 *   were.  One exception, as for the occlusion tables: the FIRST call after an rt_upload_scene builds the query's own bounds of that scene
 *   (a vertex box per node and per 64-record chunk of a leaf, a vertex record per leaf reference: 32 B per node + 32 B per chunk + 48 B per
 *   face reference of device memory) and synchronises
 *   the context's stream while it does; they are freed with the scene (the next upload, rt_destroy) and rebuilt by the next call.
 * rt_closest_points: the same with host pointers: it allocates, uploads, enqueues the call above on the context's stream, synchronises that
 *   stream and downloads.                                                                                                                   */
rt_status rt_closest_points_device(rt_ctx *ctx, int32_t n, const float *d_point_in, float max_dist, int32_t *d_face /* n, may be NULL */,
                                   float *d_dist2 /* n, may be NULL */, float *d_point /* n*3, may be NULL */, void *stream);
rt_status rt_closest_points(rt_ctx *ctx, int32_t n, const float *point, float max_dist, int32_t *face, float *dist2, float *closest);
rt_status rt_closest_point_triangle(const float p[3], const float tri[9], float q[3], float *d2);

/* ---- ordered ray hits: the first k surfaces along a ray, in order, and whether there are more -------------------------------------------
 * No reference counterpart: what lies BEHIND the closest hit (Ordered ray hits) -- depth layers, thickness, crossing parity.
 * This section is the DEFINITION; tests/ray_hits_ref.py restates it over the CPU checker.
 *   Candidates. Ray i = (o, d) = (d_origin[i*3..], d_dir[i*3..]), d used as given.  If boxIntersect(root, o, o + d) fails the ray has no hits.
 *            Otherwise the candidates are the DISTINCT faces of the leaves that BoxTree::intersect(o, o + d) reaches: exactly the candidate
 *            set of rt_closest_hits_device.  A face that several of those leaves reference counts once.
 *   Hit.     Face f is a hit with parameter x when rayTriangleIntersection(o, d, f) accepts it and x > 0.00001f and x <= t_max.  The
 *            arithmetic is that of the other ray queries: x is, bit for bit, the t that rt_closest_hits_device would report for f.
 *   Order.   The hits are sorted ascending by (x, face id).  A NaN x is never a hit.
 *   Outputs. With H the number of distinct hits: d_count[i] = min(H, k + 1), so k + 1 says "more than k"; d_face[i*k + j] and d_t[i*k + j]
 *            hold the j-th hit for j < min(H, k); the other entries of the ray's k slots are -1 / -1.0f.  So entry 0 with t_max = +inf is
 *            rt_closest_hits_device's answer in every bit, the result for k is a prefix of the result for any larger k, and nothing
 *            depends on the order in which the leaves are met.
 * rt_ray_hits_device: d_origin, d_dir float[n*3]; d_face int32[n*k], d_t float[n*k], d_count int32[n]; any of the three outputs may be
 *   NULL, not all.  1 <= k <= RT_MAX_RAY_HITS; t_max > 0, +inf = unbounded.  The common rules of the device ray queries hold: device
 *   pointers; NULL context / origin / dir, n < 0, a k out of range, a NaN or <= 0 t_max, an output range sharing a byte with an input or with
 *   another output: RT_ERR_INVALID; RT_ERR_NO_SCENE before rt_upload_scene; n == 0: RT_OK, nothing enqueued; exactly n*k, n*k and n elements
 *   are written; element indices are 64-bit.  ASYNCHRONOUS and scene-only exactly like rt_closest_hits_device: ONE kernel on `stream`
 *   (NULL = the context's stream), no allocation, no synchronisation, none of the context's frame buffers; the caller orders it against
 *   rt_upload_scene.
 * rt_ray_hits: the same with host pointers: it allocates, uploads, enqueues the call above on the context's stream, synchronises that
 *   stream and downloads.                                                                                                                   */
#define RT_MAX_RAY_HITS 8
rt_status rt_ray_hits_device(rt_ctx *ctx, int32_t n, const float *d_origin, const float *d_dir, int32_t k, float t_max,
                             int32_t *d_face /* n*k, may be NULL */, float *d_t /* n*k, may be NULL */, int32_t *d_count /* n, may be NULL */,
                             void *stream);
rt_status rt_ray_hits(rt_ctx *ctx, int32_t n, const float *origin, const float *dir, int32_t k, float t_max, int32_t *face, float *t,
                      int32_t *count);

/* ---- unit-parity entry points: the device functions of the path on caller-given inputs ------------------------------------------
 * replaces: BoundingBox::boxIntersect (src/boundingBox.cpp:48-83) -- n boxes [n*6: min, max], segments origin/dest [n*3]; hit[i] = the
 *           decision of the kernels' slab test (approximate-then-verify form, bit-identical to the reference by construction)       */
rt_status rt_box_intersect(rt_ctx *ctx, int32_t n, const float *boxes, const float *origin, const float *dest, uint8_t *hit);
/* replaces: one light sample of Flyscene::phongShade (flyscene.cpp:838-853) -- the per-sample arithmetic of the shading kernels on n
 *           caller-given cases, one per lane: case i runs in lane i % 64 of wave i / 64, so the caller decides which cases share a wave (the
 *           kernels choose their paths by wave-uniform tests).  n must be a multiple of 64.  hit, normal (used as given), eye (eyeToHitPoint),
 *           sample, lkd, lks (light colour x kd / ks) are [n*3], shininess [n]; out[i*6 ..] = {lightDirection . normal, cosphi,
 *           powf(cosphi, shininess), r, g, b} with (r, g, b) = lkd * max(0, l.n) + lks * pow                                              */
rt_status rt_debug_phong_samples(rt_ctx *ctx, int32_t n, const float *hit, const float *normal, const float *eye, const float *sample, const float *lkd,
                                 const float *lks, const float *shininess, float *out);
/* replaces: BoxTree::intersect (src/boxTree.cpp:150-173) on the uploaded tree, reference semantics (no culling, no early-out): per ray
 *           the number of boxIntersect calls, the sum of faces.size() over the intersected non-empty leaves, and a signature of that
 *           leaf set: sum over its leaves of (index into rt_scene.nodes) * 2654435761 mod 2^32                                    */
rt_status rt_tree_probe(rt_ctx *ctx, int32_t n, const float *origin, const float *dest, uint32_t *box_tests, uint32_t *leaf_refs, uint32_t *leaf_sig);
/* replaces: Camera::screenToWorld (camera.hpp:155-173) for every pixel, evaluated by the device's primary-ray generator:
 *           out[(j*W + i)*3 ..] = screenToWorld(Vector2f(i, j))                                                                   */
rt_status rt_primary_points(rt_ctx *ctx, const rt_camera *cam, int32_t width, int32_t height, float *out);

/* ---- host-side scene preparation (GL-free restatement of the Tucano loader + BoxTree builder) --------------- */
typedef struct rt_host_scene rt_host_scene;
/* replaces: MeshImporter::loadObjFile + mesh.normalizeModelMatrix() + BoxTree(mesh, capacity)
 *           (flyscene.cpp:50-56,86-93; objimporter.hpp:83-284; boxTree.cpp:11-31)                                 */
rt_status rt_host_scene_load(const char *obj_path, int32_t leaf_capacity, int32_t max_depth, rt_host_scene **out);
void      rt_host_scene_free(rt_host_scene *hs);
/* borrowed view of the flattened arrays (valid until rt_host_scene_free / rt_host_scene_set_model)               */
rt_status rt_host_scene_view(const rt_host_scene *hs, rt_scene *out);
/* replaces: Flyscene::modifyTriangle (flyscene.cpp:998-1015): sets the model matrix; rebuild != 0 also rebuilds
 * the octree (the reference leaves it stale)                                                                     */
rt_status rt_host_scene_set_model(rt_host_scene *hs, const float model[12], int32_t rebuild_tree);
/* replaces: BoxTree(mesh, capacity) / split / clasifyFace (src/boxTree.cpp:11-31,88-147,203-336) evaluated ON THE DEVICE of `ctx`
 * (level-synchronous classify + stable compaction, rt_build.hip): rebuilds the octree of the host scene's current world vertices and
 * re-flattens it.  The result equals the host build (rt_host_scene_load / _set_model(rebuild)) array for array.                   */
rt_status rt_host_scene_build_gpu(rt_host_scene *hs, rt_ctx *ctx, int32_t leaf_capacity, int32_t max_depth);
/* tree summary: nodes, non-empty leaves, face refs, largest leaf, depth, "lost" faces                             */
rt_status rt_host_scene_info(const rt_host_scene *hs, int32_t out[8], float root_box[6]);

/* diagnostic, host only: {chunks, cullable chunks, leaves, max chunks per leaf} of the lanes=triangles chunk bounds   */
rt_status rt_debug_chunk_stats(const rt_scene *scene, int32_t out[4]);
/* diagnostic, host only: the bounds themselves -- 16 floats per chunk {lo[3], hi[3], never, infl, sn[3], slo, shi, 0, 0, 0} (box, slab along
 * the chunk's mean normal) -- with the first chunk of every leaf (n_nodes words) and the leaf face references in chunk order (n_face_refs
 * words).  bounds may be NULL to query *n_chunks.                                                                                         */
rt_status rt_debug_chunk_bounds(const rt_scene *scene, float *bounds, int32_t cap_chunks, int32_t *n_chunks, uint32_t *leaf_chunk0, uint32_t *refs);

/* diagnostic: wave-level step counters of the last frame, as executed by the shipped kernels (box-test steps, shaft steps, (ray, chunk)
 * triangle steps ...; layout in DESIGN.md 6).  Only the counting build librt_mi355x_work.so (same sources, -DRT_WORK_COUNTERS) fills them;
 * the product library returns RT_ERR_UNSUPPORTED.  bench.py uses it, outside the timed region, for the executed-work roofline.          */
rt_status rt_debug_work_counters(rt_ctx *ctx, uint64_t *out, int32_t n);

/* replaces: Flycamera defaults + setPerspectiveMatrix/setViewport (flyscene.cpp:46-47, flycamera.hpp:76-86)       */
void rt_default_camera(rt_camera *cam, int32_t width, int32_t height);
/* fly-camera yaw (rotation_Y_axis) for animation paths (flycamera.hpp:166-191)                                    */
void rt_yaw_camera(rt_camera *cam, int32_t width, int32_t height, float yaw);
/* replaces: Camera::screenToWorld (camera.hpp:155-173); host evaluation, used to check the device's              */
void rt_screen_to_world(const rt_camera *cam, float i, float j, float out[3]);
/* replaces: the sphere-point loop of createSpherePoint (flyscene.cpp:976-993) with std::random_device replaced by the seed: point i
 * uses std::mt19937 gen(seed + i); std::uniform_real_distribution<> dis(0, 1) (libstdc++: generate_canonical<double, 53>), then
 * theta = 2.0f * M_PI * r, phi = acos(2.0 * r - 1.0), (x, y, z) = radius * (sin(phi) cos(theta), sin(phi) sin(theta), cos(phi)) in float,
 * out[i] = Vector3f(x, y, z) / 5.  radius = lightrep.getBoundingSphereRadius() (1.0: the unit sphere shape).  Host only.              */
void rt_sphere_offsets(uint32_t seed, float radius, int32_t n, float *out);
/* replaces: lights.push_back((-1,1,1)), lightrep colour, areaLight/pointLight stdin (flyscene.cpp:31-34,68,72)    */
void rt_default_lights(rt_lights *l, int32_t area);

/* replaces: Tucano::ImageImporter::writePPMImage (ppmIO.hpp:130-151): byte-exact ASCII P3                         */
rt_status rt_write_ppm(const char *path, const float *rgb, int32_t width, int32_t height);
rt_status rt_write_ppm_u8(const char *path, const uint8_t *rgb8, int32_t width, int32_t height);
/* binary side channel beside result.ppm (no reference counterpart): PFM "PF\nW H\n-1.0\n" + little-endian
 * float RGB rows, bottom row first as the format demands -- the un-quantised frame, 12 bytes per pixel                     */
rt_status rt_write_pfm(const char *path, const float *rgb, int32_t width, int32_t height);

#ifdef __cplusplus
}
#endif
#endif /* RT_MI355X_H */
