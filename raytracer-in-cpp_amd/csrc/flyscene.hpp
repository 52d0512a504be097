// flyscene.hpp -- host facade with the reference's scene-controller interface (src/flyscene.hpp:28-200) for the one
// path this library replaces: initialize() -> raytraceScene() -> result.ppm, plus traceRay/lightStrikes/
// createSpherePoint for single-ray use (the reference's debug ray calls traceRay, flyscene.cpp:286).
// Same member names, argument meaning and outputs; Eigen/Tucano types are replaced by a plain Vec3f because
// neither library exists outside the reference tree.  The OpenGL preview, GUI and debug-ray drawing are out of scope.
#pragma once

#include <array>
#include <string>
#include <vector>

#include "rt_mi355x.h"

namespace rtamd {

using Vec3f = std::array<float, 3>;

class Flyscene {
public:
    Flyscene() = default;
    ~Flyscene();
    Flyscene(const Flyscene &) = delete;
    Flyscene &operator=(const Flyscene &) = delete;

    // reference: prompts "Enter 0 if Point Lights or 1 if Area Lights" / "Enter 0 if spherical or 1 if point" on stdin,
    // loads resources/models/cube.obj, normalises it, builds the octree (capacity 1000) -- flyscene.cpp:29-126
    void initialize(int width, int height);
    // same without stdin: the two switches given directly.  A second initialize replaces the scene on the same device context, puts the
    // camera and the lights back to the defaults and drops the history of setTemporal (resetHistory): the first frame after it is the
    // first frame of a fresh object on that scene
    void initialize(int width, int height, bool area_light, bool point_light);

    // reference: flyscene.cpp:519-648.  0 => viewport size.  Writes ./result.ppm (ASCII P3) and prints ELAPSED TIME.  An explicit size other than
    // the viewport's re-targets the perspective (and, with setShutter, that of the close camera) for this call alone: the object's camera, what
    // getCamera() returns, is not changed, and the next raytraceScene() renders the viewport's frame again.  The same holds for gbuffer(w, h).
    void raytraceScene(int width = 0, int height = 0);

    // reference: flyscene.cpp:651-771 (countRay only drives the progress bar there; accepted and ignored here)
    Vec3f traceRay(Vec3f &origin, Vec3f &direction, int level, std::vector<Vec3f> &lights, bool countRay);
    // reference: flyscene.cpp:912-954
    bool lightStrikes(Vec3f &hitPoint, std::vector<Vec3f> &lights, bool visibleLights[]);
    // no reference member: the closest hit inside traceRay (flyscene.cpp:655-691) for a batch of rays, without lights or shading
    // (rt_closest_hits).  faces[i] / ts[i] = face id and ray parameter of ray i, -1 / -1.0f for a miss.  false: the call failed
    // (origins and dirs differ in size, no scene, a device error)
    bool closestHits(const std::vector<Vec3f> &origins, const std::vector<Vec3f> &dirs, std::vector<int> &faces, std::vector<float> &ts);
    // no reference member: ambient occlusion in terms of lightStrikes (rt_ambient_occlusion).  open[i] = how many of the m x m cosine-weighted
    // segments of length `radius` above points[i] (unit normal normals[i]; all zeros: no point, fully open) nothing blocks, 0 .. m * m.
    // false: the call failed (sizes differ, m outside 1 .. 16, a radius that is not finite and > 0, no scene, a device error)
    bool ambientOcclusion(const std::vector<Vec3f> &points, const std::vector<Vec3f> &normals, int m, float radius, unsigned seed,
                          std::vector<unsigned short> &open);
    // no reference member: the distance query beside the ray queries (rt_closest_points).  Per point the nearest face of the scene within
    // maxDist (+inf: unbounded; faces[i] = -1: none), the squared distance to it (dist2[i] = +inf: none) and the nearest point on it
    // (closest[i] = points[i]: none).  false: the call failed (a NaN or negative maxDist, no scene, a device error)
    bool closestPoints(const std::vector<Vec3f> &points, float maxDist, std::vector<int> &faces, std::vector<float> &dist2, std::vector<Vec3f> &closest);
    // no reference member: what lies behind the closest hit (rt_ray_hits).  Per ray its first k hits in order of (t, face id): faces and ts
    // hold k slots per ray (-1 / -1.0f where the ray has fewer hits), counts[i] = min(hits of ray i, k + 1), so k + 1 says "more than k";
    // hits beyond tMax (+inf: unbounded) do not count.  false: the call failed (sizes differ, k outside 1 .. 8, a NaN or <= 0 tMax, no
    // scene, a device error)
    bool rayHits(const std::vector<Vec3f> &origins, const std::vector<Vec3f> &dirs, int k, float tMax, std::vector<int> &faces, std::vector<float> &ts,
                 std::vector<int> &counts);
    // no reference member: the one-bounce diffuse gather of caller-given points (rt_indirect_diffuse) -- out[i] = the mean radiance that the
    // m x m cosine-weighted gather rays of point i bring back from their closest hits, each lit (diffuse term) by the positions of this
    // object's lights it sees; the caller multiplies by the point's own diffuse colour; a normal of three zeros gives zeros.  false: the call
    // failed (sizes differ, m outside 1 .. 16, sphere lights, no scene, a device error)
    bool indirectDiffuse(const std::vector<Vec3f> &points, const std::vector<Vec3f> &normals, int m, unsigned seed, std::vector<Vec3f> &out);
    // no reference member: an irradiance volume over the scene's root box (rt_light_probes) -- dims[0] x dims[1] x dims[2] probes whose
    // outermost ones lie on the box grown by `margin` on every side (in float: lo = min - margin, hi = max + margin, origin = lo,
    // step = (hi - lo) / (float)(dims - 1); an axis of one probe has it at (lo + hi) * 0.5f with step 1), each traced with m x m rays over the
    // sphere and lit by this object's lights; direct: the lights a probe sees are added as deltas.  grid and coeff (27 floats per probe)
    // are what probeIrradiance takes.  false: the call failed (dims below 1 or above 2^24 probes, m outside 1 .. 16, sphere lights, no scene)
    bool lightProbes(const int dims[3], int m, bool direct, float margin, rt_probe_grid &grid, std::vector<float> &coeff);
    // no reference member: lightProbes with `bounces` feedback passes behind the first (rt_light_probes_bounce) -- pass b lights every hit of
    // the probe rays by pass b - 1 of this very volume as well, one more diffuse bounce per pass; the passes swap two buffers and run without
    // the direct term, which goes into the last pass alone; visible: the passes look the volume up leak-free.  bounces == 0 is lightProbes.
    // false: the call failed (as lightProbes; bounces below 0)
    bool lightProbesBounce(const int dims[3], int m, bool direct, float margin, int bounces, bool visible, rt_probe_grid &grid, std::vector<float> &coeff);
    // no reference member: indirectDiffuse with the hits of the gather rays lit, in addition, by the probe volume (grid, coeff) looked up at
    // them (rt_indirect_diffuse_bounce) -- the final gather over a bounced volume, which must have been computed without the direct term;
    // visible: the lookup is the leak-free one.  false: the call failed (as indirectDiffuse; a bad grid, coeff of another size)
    bool indirectDiffuseBounce(const std::vector<Vec3f> &points, const std::vector<Vec3f> &normals, int m, unsigned seed, const rt_probe_grid &grid,
                               const std::vector<float> &coeff, bool visible, std::vector<Vec3f> &out);
    // no reference member: the lookup of such a volume at the frame's closest hits (rt_probe_irradiance) -- out[j * width + i] = the blend of
    // the probes round the closest hit of the pinhole ray of pixel (i, j), evaluated at the face's normal turned against the ray; zeros
    // where the ray hits nothing; the scene's camera, 0 => viewport size.  The caller multiplies by the pixel's diffuse colour.
    bool probeIrradiance(int width, int height, const rt_probe_grid &grid, const std::vector<float> &coeff, std::vector<Vec3f> &out);
    // no reference member: the same lookup over the probes each hit point can see (rt_probe_irradiance_visible): every probe round the
    // point is asked with one segment walk, the blend takes the visible ones and is renormalised, so a partition thinner than a grid step
    // no longer lets the light of the next room through; where a point sees all of its probes the two members agree in every bit
    bool probeIrradianceVisible(int width, int height, const rt_probe_grid &grid, const std::vector<float> &coeff, std::vector<Vec3f> &out);
    // no reference member: the lit share of the frame's closest hits (rt_soft_shadows) -- out[j * width + i] = the share of the samples of
    // this object's lights (point or area) that the closest hit of the pinhole ray of pixel (i, j) sees, 1.0f where the ray hits nothing; the
    // scene's camera, 0 => viewport size.  params == nullptr: rt_default_shadow_params, the samples of every frame; a per-point jitter takes the
    // pixel's raster index.  false (and an empty out): the call failed (sphere lights, parameters out of range, no scene, a device error)
    bool softShadows(int width, int height, const rt_shadow_params *params, std::vector<float> &out);
    // no reference member: the geometry buffers of the frame raytraceScene(width, height) renders (rt_gbuffer) -- RT_GBUFFER_CHANNELS floats per
    // pixel, row-major: coverage, depth, face normal, diffuse colour, averaged over the frame's sub-samples and passes with the scene's
    // camera and the sample settings set on this object (supersampling, lens, shutter, passes).  0 => viewport size.  Empty: the call failed
    // (no scene, adaptive pass counts on, a device error)
    std::vector<float> gbuffer(int width = 0, int height = 0);
    // no reference member: the edge-avoiding a-trous filter (rt_denoise) of a width x height image of `channels` (1 or 3) floats per pixel,
    // guided by the geometry buffers of the same frame (what gbuffer() returns for it); dp == nullptr: rt_default_denoise_params.
    // false: the call failed (sizes that do not fit, parameters out of range, a device error)
    bool denoise(const std::vector<float> &image, int channels, const std::vector<float> &gbuffer, int width, int height, const rt_denoise_params *dp,
                 std::vector<float> &out);
    // no reference member: the guided upsample (rt_upsample) of a low image of ceil(width / factor) x ceil(height / factor) pixels of `channels`
    // (1 or 3) floats to width x height, steered by the geometry buffers of the low and of the high frame; up == nullptr:
    // rt_default_upsample_params; miss, if given, gets one byte per pixel: 1 where no tap was left and the nearest low pixel was taken.
    // false: the call failed (sizes that do not fit, parameters out of range, a device error)
    bool upsample(const std::vector<float> &low, int channels, const std::vector<float> &gb_low, const std::vector<float> &gb_high, int width, int height,
                  const rt_upsample_params *up, std::vector<float> &out, std::vector<uint8_t> *miss = nullptr);
    // no reference member: the temporal reprojection (rt_reproject) of the accumulated image `hist` of the previous frame (lengths len_hist, one
    // byte per pixel, 0 = no history) into the current frame `cur`, both width x height pixels of `channels` (1 or 3) floats, through the
    // geometry buffers of both frames and the map m[12] of rt_reproject_map(current camera, previous camera); rp == nullptr:
    // rt_default_reproject_params.  false: the call failed (sizes that do not fit, parameters out of range, a device error)
    bool reproject(const std::vector<float> &cur, int channels, const std::vector<float> &gb_cur, const std::vector<float> &hist,
                   const std::vector<float> &gb_hist, const std::vector<uint8_t> &len_hist, int width, int height, const float m[12],
                   const rt_reproject_params *rp, std::vector<float> &out, std::vector<uint8_t> &len_out);
    // reference: flyscene.cpp:962-972 (point and area modes)
    std::vector<Vec3f> createSpherePoint(Vec3f lightPoint);
    // reference: flyscene.hpp:58-62 (adds a light at the camera centre)
    void addLight();

    // knobs the reference hard-codes (flyscene.cpp:51,86,971; boxTree.cpp:3) or does not have
    void setScenePath(const std::string &obj) { scene_path_ = obj; }
    void setAreaGrid(int usteps, int vsteps) { usteps_ = usteps; vsteps_ = vsteps; }
    // the two light switches of initialize() on their own (host only: createSpherePoint needs no scene); neither = the spherical mode, whose
    // 25 offsets are drawn here
    void setLightMode(bool area_light, bool point_light);
    void setMaxDepth(int d) { max_depth_ = d; }       // <0: the library's maximum (the reference is unbounded)
    void setOutputPath(const std::string &p) { output_path_ = p; }
    void setDevice(int d) { device_ = d; }
    // n x n sub-samples per pixel in raytraceScene (rt_set_supersampling, 1..RT_MAX_SUPERSAMPLING); 1 = the reference's one ray per pixel
    void setSupersampling(int n) { supersampling_ = n; }
    // adaptive supersampling (rt_set_supersampling_threshold): refine only pixels on colour edges; < 0 (default) = every pixel
    void setSupersamplingThreshold(float t) { supersampling_threshold_ = t; }
    // thin-lens depth of field (rt_set_lens): lens radius in world units (0 = pinhole, the default) and the depth of the plane in focus
    void setLens(float aperture, float focus) { lens_aperture_ = aperture; lens_focus_ = focus; }
    // camera motion blur (rt_set_shutter): the camera at shutter close (copied); the scene's own camera is the one at shutter open.
    // nullptr = the shutter is off, the default
    void setShutter(const rt_camera *close) { shutter_on_ = close != nullptr; if (close) shutter_close_ = *close; }
    // multi-pass accumulation (rt_set_passes(0, count), 1..RT_MAX_PASSES): the frame is the mean of `count` jittered, reseeded passes; 1 = the default
    void setPasses(int count) { passes_ = count; }
    // adaptive pass counts (rt_set_pass_tolerance): a pixel stops taking passes once it has taken min_passes (2..RT_MAX_PASSES) and the standard
    // error of its mean is at most tol in every channel; tol < 0 = every pixel takes every pass, the default
    void setPassTolerance(float tol, int min_passes = 8) { pass_tolerance_ = tol; pass_min_ = min_passes; }
    // denoising (rt_denoise): raytraceScene filters its frame, guided by the frame's geometry buffers, before it writes the image; nullptr = off,
    // the default.  (Adaptive pass counts have no geometry buffers: such a frame fails.)
    void setDenoise(const rt_denoise_params *dp) { denoise_on_ = dp != nullptr; if (dp) denoise_ = *dp; }
    // upsampling (rt_upsample): raytraceScene renders the frame at 1 / factor of the size through the low camera (the viewport size divided by
    // the factor), filters it there if setDenoise is on, and brings it to full size steered by the geometry buffers of both sizes; nullptr =
    // off, the default
    void setUpsample(const rt_upsample_params *up) { upsample_on_ = up != nullptr; if (up) upsample_ = *up; }
    // temporal reuse (rt_reproject): successive raytraceScene calls of one size keep history -- the previous camera, geometry buffers,
    // accumulated image and lengths.  Frame k after the last reset renders with rt_set_passes((k mod (RT_MAX_PASSES / count)) * count, count),
    // takes its geometry buffers, reprojects the history into it and then filters it if setDenoise is on; the stored history is the image
    // before the filter.  The first frame is itself, with every length 1.  A change of size and initialize() drop the history.  nullptr = off, the default.
    // Not together with setUpsample (such a frame fails with RT_ERR_INVALID).
    void setTemporal(const rt_reproject_params *rp) { temporal_on_ = rp != nullptr; if (rp) temporal_ = *rp; }
    void resetHistory() { hist_frames_ = 0; hist_image_.clear(); hist_gbuffer_.clear(); hist_len_.clear(); }
    const std::vector<uint8_t> &historyLengths() const { return hist_len_; }
    const rt_stats &lastStats() const { return stats_; }
    // status of the last raytraceScene() (the reference's member is void; a headless caller needs to know): RT_OK or a negative rt_status
    rt_status lastStatus() const { return last_status_; }
    const std::vector<float> &lastImage() const { return image_; }
    rt_camera *getCamera() { return &camera_; }
    std::vector<Vec3f> &getLights() { return lights_; }
    bool ok() const { return ctx_ != nullptr; }

private:
    // the camera `cam` of a width x height frame (0 => viewport size) and the sample settings of this object, set on the context; camera_ stays
    rt_status frame_settings(int &width, int &height, rt_camera &cam);
    void fill_lights(rt_lights *l, const std::vector<Vec3f> &pts) const;
    bool probeLookup(const char *who, bool visible, int width, int height, const rt_probe_grid &grid, const std::vector<float> &coeff, std::vector<Vec3f> &out);
    std::string scene_path_ = "resources/models/cube.obj";
    std::string output_path_ = "result.ppm";
    rt_ctx *ctx_ = nullptr;
    rt_host_scene *scene_ = nullptr;
    rt_camera camera_{};
    std::vector<Vec3f> lights_;
    bool areaLight = true, pointLight = false;
    int usteps_ = 5, vsteps_ = 5, max_depth_ = -1, device_ = 0, supersampling_ = 1;
    float supersampling_threshold_ = -1.0f;
    float lens_aperture_ = 0.0f, lens_focus_ = 2.0f;
    int passes_ = 1;
    float pass_tolerance_ = -1.0f;
    int pass_min_ = 8;
    bool shutter_on_ = false, denoise_on_ = false, upsample_on_ = false;
    rt_denoise_params denoise_{};
    rt_upsample_params upsample_{};
    bool temporal_on_ = false;
    rt_reproject_params temporal_{};
    int hist_frames_ = 0, hist_w_ = 0, hist_h_ = 0;       // frames since the last reset, and the size they had
    rt_camera hist_camera_{};
    std::vector<float> hist_image_, hist_gbuffer_;        // the accumulated image (before the filter) and the buffers of the previous frame
    std::vector<uint8_t> hist_len_;
    // one frame of setTemporal: render, buffers, reprojection, filter -> image_
    rt_status temporal_frame(const rt_camera &cam, const rt_lights &L, const rt_params &p);
    rt_camera shutter_close_{};
    int view_w_ = 0, view_h_ = 0;
    rt_stats stats_{};
    rt_status last_status_ = RT_OK;
    std::vector<float> image_;
    std::vector<float> sphere_offsets_;          // spherical light mode: Vector3f(x, y, z) / 5 per sample (rt_sphere_offsets)
    uint32_t sphere_seed_ = 65u;                 // "CG Raytracing Group 65" (README.MD:1)
};

}  // namespace rtamd
