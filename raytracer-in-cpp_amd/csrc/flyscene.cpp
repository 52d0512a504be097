// flyscene.cpp -- see flyscene.hpp.  Everything here goes through the C ABI of include/rt_mi355x.h.
#include "flyscene.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

namespace rtamd {

Flyscene::~Flyscene() {
    if (ctx_) rt_destroy(ctx_);
    if (scene_) rt_host_scene_free(scene_);
}

void Flyscene::initialize(int width, int height) {
    int area = 1, point = 0;
    std::cout << "Enter 0 if Point Lights or 1 if Area Lights : " << std::endl;
    std::cin >> area;
    std::cout << "Enter 0 if spherical or 1 if point : " << std::endl;
    std::cin >> point;
    initialize(width, height, area != 0, point != 0);
}

void Flyscene::setLightMode(bool area_light, bool point_light) {
    areaLight = area_light;
    pointLight = point_light;
    if (!pointLight && !areaLight) {
        // the spherical mode (flyscene.cpp:974-995): 25 points per light, drawn ONCE per initialize() from the seeded restatement of
        // the reference's loop (it re-draws them from an unseeded std::random_device at every shaded hit: not reproducible)
        sphere_offsets_.assign(25 * 3, 0.f);
        rt_sphere_offsets(sphere_seed_, 1.0f, 25, sphere_offsets_.data());
    }
}

void Flyscene::initialize(int width, int height, bool area_light, bool point_light) {
    setLightMode(area_light, point_light);
    view_w_ = width; view_h_ = height;
    resetHistory();                                    // the history of setTemporal belongs to the scene that is replaced here
    rt_default_camera(&camera_, width, height);
    lights_.clear();
    lights_.push_back({-1.0f, 1.0f, 1.0f});           // flyscene.cpp:72
    std::cout << "Seting up acceleration data structure ..." << std::endl;
    const auto t0 = std::chrono::high_resolution_clock::now();
    if (scene_) { rt_host_scene_free(scene_); scene_ = nullptr; }
    if (rt_host_scene_load(scene_path_.c_str(), 1000, 15, &scene_) != RT_OK) {
        std::cerr << "Cannot open " << scene_path_ << std::endl;
        std::exit(1);                                  // objimporter.hpp:105
    }
    const std::chrono::duration<double> el = std::chrono::high_resolution_clock::now() - t0;
    std::cout << "Seting up acceleration data structure: done!" << std::endl;
    std::cout << "ELAPSED TIME:" << el.count() << std::endl;
    if (!ctx_) {
        const rt_status s = rt_create(&ctx_, device_);
        if (s != RT_OK) {
            std::cerr << "rt_mi355x: cannot create a device context (status " << s << "); there is no CPU fallback" << std::endl;
            std::exit(1);
        }
    }
    rt_scene view;
    rt_host_scene_view(scene_, &view);
    if (rt_upload_scene(ctx_, &view) != RT_OK) {
        std::cerr << "rt_mi355x: " << rt_last_error(ctx_) << std::endl;
        std::exit(1);
    }
}

void Flyscene::fill_lights(rt_lights *l, const std::vector<Vec3f> &pts) const {
    rt_default_lights(l, (areaLight && !pointLight) ? 1 : 0);
    if (!pointLight && !areaLight) {        // createSpherePoint's third branch
        l->mode = RT_LIGHT_SPHERE;
        l->n_offsets = static_cast<int32_t>(sphere_offsets_.size() / 3);
        l->offsets = sphere_offsets_.data();
    }
    l->n_lights = static_cast<int32_t>(pts.size());
    for (size_t i = 0; i < pts.size() && i < RT_MAX_LIGHTS; ++i) std::memcpy(l->pos[i], pts[i].data(), sizeof(float) * 3);
    l->usteps = usteps_; l->vsteps = vsteps_;
}

rt_status Flyscene::frame_settings(int &width, int &height, rt_camera &cam) {
    if (width == 0 || height == 0) { width = view_w_; height = view_h_; }
    cam = camera_;
    rt_camera close = shutter_close_;
    if (width != view_w_ || height != view_h_) {
        // the reference keeps the viewport's camera; an explicit size re-targets the perspective like initialize(w,h) -- for this frame alone
        // (camera_ and shutter_close_ stay), and for the shutter's close camera too: a shutter moves the pose only
        rt_default_camera(&cam, width, height);
        std::memcpy(cam.center, camera_.center, sizeof cam.center);
        std::memcpy(cam.inv_view, camera_.inv_view, sizeof cam.inv_view);
        close = cam;
        std::memcpy(close.center, shutter_close_.center, sizeof close.center);
        std::memcpy(close.inv_view, shutter_close_.inv_view, sizeof close.inv_view);
    }
    rt_status s = rt_set_supersampling(ctx_, supersampling_);
    if (s == RT_OK) s = rt_set_supersampling_threshold(ctx_, supersampling_threshold_);
    if (s == RT_OK) s = rt_set_lens(ctx_, lens_aperture_, lens_focus_);
    if (s == RT_OK) s = rt_set_shutter(ctx_, shutter_on_ ? &close : nullptr);
    if (s == RT_OK) s = rt_set_passes(ctx_, 0, passes_);
    if (s == RT_OK) s = rt_set_pass_tolerance(ctx_, pass_tolerance_, pass_min_);
    return s;
}

void Flyscene::raytraceScene(int width, int height) {
    const auto t0 = std::chrono::high_resolution_clock::now();
    rt_camera cam;
    rt_status s = frame_settings(width, height, cam);
    rt_lights L;
    fill_lights(&L, lights_);
    rt_params p{};
    p.width = width; p.height = height; p.max_depth = max_depth_;
    p.row0 = 0; p.row1 = height; p.stripe = 1; p.rank = 0; p.nranks = 1; p.collect_stats = 0;
    image_.assign(static_cast<size_t>(width) * height * 3, 0.f);
    std::cout << "Ray tracing ..." << std::endl;
    if (s == RT_OK && temporal_on_) {           // the frame with its passes advanced, its buffers, the history reprojected into it, then the filter
        s = upsample_on_ ? RT_ERR_INVALID : temporal_frame(cam, L, p);
        last_status_ = s;
        if (s != RT_OK) {
            std::cerr << "rt_mi355x: temporal render failed: " << (upsample_on_ ? "temporal reuse together with upsampling is not supported" : rt_last_error(ctx_))
                      << std::endl;
            return;
        }
    } else if (s == RT_OK && upsample_on_) {          // the frame at 1 / factor of the size through the low camera, filtered there, then the guided upsample
        rt_camera lcam = cam;
        const float fs = static_cast<float>(upsample_.factor);
        lcam.viewport[2] = cam.viewport[2] / fs;
        lcam.viewport[3] = cam.viewport[3] / fs;
        rt_params lp = p;
        s = rt_upsample_low_size(width, height, upsample_.factor, &lp.width, &lp.height);
        if (s != RT_OK) std::cerr << "rt_mi355x: upsampling failed: the factor is outside 2 .. " << RT_UPSAMPLE_MAX_FACTOR << std::endl;
        lp.row1 = lp.height;
        const size_t lpix = s == RT_OK ? static_cast<size_t>(lp.width) * lp.height : 0;
        std::vector<float> low(lpix * 3), gl(lpix * RT_GBUFFER_CHANNELS), gh(static_cast<size_t>(width) * height * RT_GBUFFER_CHANNELS);
        if (s == RT_OK) s = rt_render(ctx_, &lcam, &L, &lp, low.data(), nullptr, &stats_);
        if (s == RT_OK) s = rt_gbuffer(ctx_, &lcam, &lp, gl.data());
        if (s == RT_OK && denoise_on_) {
            std::vector<float> out(low.size());
            s = rt_denoise(ctx_, low.data(), 3, gl.data(), lp.width, lp.height, &denoise_, out.data());
            low.swap(out);
        }
        if (s == RT_OK) s = rt_gbuffer(ctx_, &cam, &p, gh.data());
        if (s == RT_OK) s = rt_upsample(ctx_, low.data(), 3, gl.data(), gh.data(), width, height, &upsample_, image_.data(), nullptr);
        last_status_ = s;
        if (s != RT_OK) {
            std::cerr << "rt_mi355x: upsampled render failed: " << rt_last_error(ctx_) << std::endl;
            return;
        }
    } else {
        if (s == RT_OK) s = rt_render(ctx_, &cam, &L, &p, image_.data(), nullptr, &stats_);
        last_status_ = s;
        if (s != RT_OK) {
            std::cerr << "rt_mi355x: render failed: " << rt_last_error(ctx_) << std::endl;
            return;
        }
    }
    if (denoise_on_ && !upsample_on_ && !temporal_on_) {                    // the post-step: the geometry buffers of this frame, then the filter
        std::vector<float> g(static_cast<size_t>(width) * height * RT_GBUFFER_CHANNELS), out(image_.size());
        s = rt_gbuffer(ctx_, &cam, &p, g.data());
        if (s == RT_OK) s = rt_denoise(ctx_, image_.data(), 3, g.data(), width, height, &denoise_, out.data());
        last_status_ = s;
        if (s != RT_OK) {
            std::cerr << "rt_mi355x: denoising failed: " << rt_last_error(ctx_) << std::endl;
            return;
        }
        image_.swap(out);
    }
    std::cout << "Writting to restult.ppm ... " << std::endl;
    last_status_ = rt_write_ppm(output_path_.c_str(), image_.data(), width, height);
    if (last_status_ != RT_OK) { std::cerr << "rt_mi355x: cannot write " << output_path_ << std::endl; return; }
    const std::chrono::duration<double> el = std::chrono::high_resolution_clock::now() - t0;
    std::cout << "Writting to restult.ppm done!" << std::endl << std::endl << "ray tracing done! " << std::endl;
    std::cout << "ELAPSED TIME:" << el.count() << std::endl;
}

rt_status Flyscene::temporal_frame(const rt_camera &cam, const rt_lights &L, const rt_params &p) {
    const int width = p.width, height = p.height;
    if (hist_frames_ > 0 && (hist_w_ != width || hist_h_ != height)) resetHistory();
    const size_t pix = static_cast<size_t>(width) * static_cast<size_t>(height);
    const int slots = RT_MAX_PASSES / passes_ > 0 ? RT_MAX_PASSES / passes_ : 1;
    rt_status s = rt_set_passes(ctx_, (hist_frames_ % slots) * passes_, passes_);       // frame k takes its own passes, so that frames are decorrelated
    std::vector<float> g(pix * RT_GBUFFER_CHANNELS);
    if (s == RT_OK) s = rt_render(ctx_, &cam, &L, &p, image_.data(), nullptr, &stats_);
    if (s == RT_OK) s = rt_gbuffer(ctx_, &cam, &p, g.data());
    std::vector<uint8_t> len(pix, 1);
    if (s == RT_OK && hist_frames_ > 0) {
        float m[12];
        std::vector<float> out(image_.size());
        s = rt_reproject_map(&cam, &hist_camera_, m);
        if (s == RT_OK) s = rt_reproject(ctx_, image_.data(), 3, g.data(), hist_image_.data(), hist_gbuffer_.data(), hist_len_.data(), width, height, m, &temporal_,
                                         out.data(), len.data());
        if (s == RT_OK) image_.swap(out);
    }
    if (s == RT_OK) {                                                                   // the history of the next frame: the image before the filter
        hist_image_ = image_;
        hist_gbuffer_.swap(g);
        hist_len_.swap(len);
        hist_camera_ = cam;
        hist_w_ = width; hist_h_ = height;
        ++hist_frames_;
        if (denoise_on_) {
            std::vector<float> out(image_.size());
            s = rt_denoise(ctx_, image_.data(), 3, hist_gbuffer_.data(), width, height, &denoise_, out.data());
            if (s == RT_OK) image_.swap(out);
        }
    }
    const rt_status back = rt_set_passes(ctx_, 0, passes_);                             // whatever happened: later frames start at pass 0 again
    return s != RT_OK ? s : back;
}

bool Flyscene::reproject(const std::vector<float> &cur, int channels, const std::vector<float> &gb_cur, const std::vector<float> &hist,
                         const std::vector<float> &gb_hist, const std::vector<uint8_t> &len_hist, int width, int height, const float m[12],
                         const rt_reproject_params *rp, std::vector<float> &out, std::vector<uint8_t> &len_out) {
    rt_reproject_params def;
    rt_default_reproject_params(&def);
    const bool shape = (channels == 1 || channels == 3) && width >= 1 && height >= 0 && m != nullptr;
    const size_t pix = shape ? static_cast<size_t>(width) * static_cast<size_t>(height) : 0, img = pix * static_cast<size_t>(channels);
    if (!shape || cur.size() != img || hist.size() != img || gb_cur.size() != pix * RT_GBUFFER_CHANNELS || gb_hist.size() != pix * RT_GBUFFER_CHANNELS ||
        len_hist.size() != pix) {
        std::cerr << "rt_mi355x: reproject failed: the images must hold width * height * (1 or 3) floats, the buffers width * height * 8 and the lengths "
                     "width * height bytes" << std::endl;
        return false;
    }
    out.assign(img, 0.0f);
    len_out.assign(pix, 0);
    if (pix == 0) return true;
    if (rt_reproject(ctx_, cur.data(), channels, gb_cur.data(), hist.data(), gb_hist.data(), len_hist.data(), width, height, m, rp ? rp : &def, out.data(),
                     len_out.data()) != RT_OK) {
        std::cerr << "rt_mi355x: reproject failed: " << rt_last_error(ctx_) << std::endl;
        return false;
    }
    return true;
}

Vec3f Flyscene::traceRay(Vec3f &origin, Vec3f &direction, int level, std::vector<Vec3f> &lights, bool) {
    rt_lights L;
    fill_lights(&L, lights);
    Vec3f out{0.f, 0.f, 0.f};
    // `level` is never tested by the reference; here it offsets the depth budget
    int budget = max_depth_ < 0 ? -1 : (max_depth_ - level < 0 ? 0 : max_depth_ - level);
    if (rt_trace_rays(ctx_, &L, budget, 1, origin.data(), direction.data(), out.data(), nullptr, nullptr) != RT_OK)
        std::cerr << "rt_mi355x: traceRay failed: " << rt_last_error(ctx_) << std::endl;
    return out;
}

bool Flyscene::lightStrikes(Vec3f &hitPoint, std::vector<Vec3f> &lights, bool visibleLights[]) {
    const int n = static_cast<int>(lights.size());
    std::vector<float> hit(static_cast<size_t>(n) * 3), src(static_cast<size_t>(n) * 3);
    std::vector<uint8_t> vis(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        std::memcpy(&hit[i * 3], hitPoint.data(), sizeof(float) * 3);
        std::memcpy(&src[i * 3], lights[i].data(), sizeof(float) * 3);
    }
    bool any = false;
    if (rt_light_strikes(ctx_, n, hit.data(), src.data(), vis.data()) != RT_OK) {
        std::cerr << "rt_mi355x: lightStrikes failed: " << rt_last_error(ctx_) << std::endl;
        return false;
    }
    for (int i = 0; i < n; ++i) { visibleLights[i] = vis[i] != 0; any = any || visibleLights[i]; }
    return any;
}

bool Flyscene::denoise(const std::vector<float> &image, int channels, const std::vector<float> &gbuffer, int width, int height, const rt_denoise_params *dp,
                       std::vector<float> &out) {
    rt_denoise_params def;
    rt_default_denoise_params(&def);
    const bool shape = (channels == 1 || channels == 3) && width >= 1 && height >= 0;
    const size_t pix = shape ? static_cast<size_t>(width) * static_cast<size_t>(height) : 0;
    if (!shape || image.size() != pix * static_cast<size_t>(channels) || gbuffer.size() != pix * RT_GBUFFER_CHANNELS) {
        std::cerr << "rt_mi355x: denoise failed: the image must hold width * height * (1 or 3) floats and the buffers width * height * 8" << std::endl;
        return false;
    }
    out.assign(image.size(), 0.0f);
    if (pix == 0) return true;
    if (rt_denoise(ctx_, image.data(), channels, gbuffer.data(), width, height, dp ? dp : &def, out.data()) != RT_OK) {
        std::cerr << "rt_mi355x: denoise failed: " << rt_last_error(ctx_) << std::endl;
        return false;
    }
    return true;
}

bool Flyscene::upsample(const std::vector<float> &low, int channels, const std::vector<float> &gb_low, const std::vector<float> &gb_high, int width,
                        int height, const rt_upsample_params *up, std::vector<float> &out, std::vector<uint8_t> *miss) {
    rt_upsample_params def;
    rt_default_upsample_params(&def);
    if (!up) up = &def;
    int32_t w = 0, r = 0;
    const bool shape = (channels == 1 || channels == 3) && rt_upsample_low_size(width, height, up->factor, &w, &r) == RT_OK;
    const size_t pix = shape ? static_cast<size_t>(width) * static_cast<size_t>(height) : 0, lpix = static_cast<size_t>(w) * static_cast<size_t>(r);
    if (!shape || low.size() != lpix * static_cast<size_t>(channels) || gb_low.size() != lpix * RT_GBUFFER_CHANNELS || gb_high.size() != pix * RT_GBUFFER_CHANNELS) {
        std::cerr << "rt_mi355x: upsample failed: the low image must hold w * r * (1 or 3) floats with w = ceil(width / factor), r = ceil(height / factor), "
                     "the buffers w * r * 8 and width * height * 8" << std::endl;
        return false;
    }
    out.assign(pix * static_cast<size_t>(channels), 0.0f);
    if (miss) miss->assign(pix, 0);
    if (pix == 0) return true;
    if (rt_upsample(ctx_, low.data(), channels, gb_low.data(), gb_high.data(), width, height, up, out.data(), miss ? miss->data() : nullptr) != RT_OK) {
        std::cerr << "rt_mi355x: upsample failed: " << rt_last_error(ctx_) << std::endl;
        return false;
    }
    return true;
}

bool Flyscene::closestHits(const std::vector<Vec3f> &origins, const std::vector<Vec3f> &dirs, std::vector<int> &faces, std::vector<float> &ts) {
    static_assert(sizeof(Vec3f) == 3 * sizeof(float) && sizeof(int) == sizeof(int32_t), "Vec3f arrays are float[n*3], int is int32_t");
    if (origins.size() != dirs.size() || origins.size() > 0x7fffffffu) {
        std::cerr << "rt_mi355x: closestHits failed: origins and dirs must have one size below 2^31" << std::endl;
        return false;
    }
    const int n = static_cast<int>(origins.size());
    faces.assign(origins.size(), -1);
    ts.assign(origins.size(), -1.0f);
    if (n == 0) return true;
    if (rt_closest_hits(ctx_, n, origins[0].data(), dirs[0].data(), faces.data(), ts.data()) != RT_OK) {
        std::cerr << "rt_mi355x: closestHits failed: " << rt_last_error(ctx_) << std::endl;
        return false;
    }
    return true;
}

bool Flyscene::ambientOcclusion(const std::vector<Vec3f> &points, const std::vector<Vec3f> &normals, int m, float radius, unsigned seed,
                                std::vector<unsigned short> &open) {
    static_assert(sizeof(Vec3f) == 3 * sizeof(float) && sizeof(unsigned short) == sizeof(uint16_t), "Vec3f arrays are float[n*3], unsigned short is uint16_t");
    if (points.size() != normals.size() || points.size() > 0x7fffffffu) {
        std::cerr << "rt_mi355x: ambientOcclusion failed: points and normals must have one size below 2^31" << std::endl;
        return false;
    }
    const int n = static_cast<int>(points.size());
    open.assign(points.size(), 0);
    if (rt_ambient_occlusion(ctx_, n, n ? points[0].data() : nullptr, n ? normals[0].data() : nullptr, m, radius, seed, open.data(), nullptr) != RT_OK) {
        std::cerr << "rt_mi355x: ambientOcclusion failed: " << rt_last_error(ctx_) << std::endl;
        return false;
    }
    return true;
}

bool Flyscene::closestPoints(const std::vector<Vec3f> &points, float maxDist, std::vector<int> &faces, std::vector<float> &dist2, std::vector<Vec3f> &closest) {
    static_assert(sizeof(Vec3f) == 3 * sizeof(float) && sizeof(int) == sizeof(int32_t), "Vec3f arrays are float[n*3], int is int32_t");
    if (points.size() > 0x7fffffffu) {
        std::cerr << "rt_mi355x: closestPoints failed: more than 2^31 - 1 points" << std::endl;
        return false;
    }
    const int n = static_cast<int>(points.size());
    faces.assign(points.size(), -1);
    dist2.assign(points.size(), 0.0f);
    closest.assign(points.size(), Vec3f{});
    if (rt_closest_points(ctx_, n, n ? points[0].data() : nullptr, maxDist, faces.data(), dist2.data(), n ? closest[0].data() : nullptr) != RT_OK) {
        std::cerr << "rt_mi355x: closestPoints failed: " << rt_last_error(ctx_) << std::endl;
        return false;
    }
    return true;
}

bool Flyscene::rayHits(const std::vector<Vec3f> &origins, const std::vector<Vec3f> &dirs, int k, float tMax, std::vector<int> &faces, std::vector<float> &ts,
                       std::vector<int> &counts) {
    static_assert(sizeof(Vec3f) == 3 * sizeof(float) && sizeof(int) == sizeof(int32_t), "Vec3f arrays are float[n*3], int is int32_t");
    if (origins.size() != dirs.size() || origins.size() > 0x7fffffffu || k < 1 || k > RT_MAX_RAY_HITS) {
        std::cerr << "rt_mi355x: rayHits failed: origins and dirs differ in length, more than 2^31 - 1 rays, or k outside 1 .. 8" << std::endl;
        return false;
    }
    const int n = static_cast<int>(origins.size());
    faces.assign(origins.size() * static_cast<size_t>(k), -1);
    ts.assign(origins.size() * static_cast<size_t>(k), -1.0f);
    counts.assign(origins.size(), 0);
    if (rt_ray_hits(ctx_, n, n ? origins[0].data() : nullptr, n ? dirs[0].data() : nullptr, k, tMax, faces.data(), ts.data(), counts.data()) != RT_OK) {
        std::cerr << "rt_mi355x: rayHits failed: " << rt_last_error(ctx_) << std::endl;
        return false;
    }
    return true;
}

bool Flyscene::indirectDiffuse(const std::vector<Vec3f> &points, const std::vector<Vec3f> &normals, int m, unsigned seed, std::vector<Vec3f> &out) {
    static_assert(sizeof(Vec3f) == 3 * sizeof(float), "Vec3f arrays are float[n*3]");
    if (points.size() != normals.size() || points.size() > 0x7fffffffu) {
        std::cerr << "rt_mi355x: indirectDiffuse failed: points and normals must have one size below 2^31" << std::endl;
        return false;
    }
    const int n = static_cast<int>(points.size());
    rt_lights L;
    fill_lights(&L, lights_);
    out.assign(points.size(), Vec3f{0.0f, 0.0f, 0.0f});
    if (rt_indirect_diffuse(ctx_, &L, n, n ? points[0].data() : nullptr, n ? normals[0].data() : nullptr, m, seed, n ? out[0].data() : nullptr) != RT_OK) {
        std::cerr << "rt_mi355x: indirectDiffuse failed: " << rt_last_error(ctx_) << std::endl;
        return false;
    }
    return true;
}

bool Flyscene::lightProbes(const int dims[3], int m, bool direct, float margin, rt_probe_grid &grid, std::vector<float> &coeff) {
    coeff.clear();
    if (!ctx_ || !scene_) {
        std::cerr << "rt_mi355x: lightProbes failed: " << rt_last_error(ctx_) << std::endl;
        return false;
    }
    int32_t counts[8];
    float box[6];
    rt_host_scene_info(scene_, counts, box);
    for (int q = 0; q < 3; ++q) {
        const float lo = box[q] - margin, hi = box[3 + q] + margin;
        const bool one = dims[q] <= 1;
        grid.origin[q] = one ? (lo + hi) * 0.5f : lo;
        grid.step[q] = one ? 1.0f : (hi - lo) / static_cast<float>(dims[q] - 1);
        grid.dims[q] = dims[q];
    }
    // (the positions first: a bad grid fails here, before anything is sized by it)
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || static_cast<int64_t>(dims[0]) * dims[1] > (1 << 24) || static_cast<int64_t>(dims[0]) * dims[1] * dims[2] > (1 << 24)) {
        std::cerr << "rt_mi355x: lightProbes failed: dims must be >= 1 and hold at most 2^24 probes" << std::endl;
        return false;
    }
    const size_t probes = static_cast<size_t>(dims[0]) * static_cast<size_t>(dims[1]) * static_cast<size_t>(dims[2]);
    std::vector<float> pos(probes * 3);
    rt_lights L;
    fill_lights(&L, lights_);
    coeff.assign(probes * RT_PROBE_COEFFS, 0.0f);
    if (rt_probe_grid_positions(&grid, pos.data()) != RT_OK ||
        rt_light_probes(ctx_, &L, static_cast<int>(probes), pos.data(), m, direct ? 1 : 0, coeff.data()) != RT_OK) {
        std::cerr << "rt_mi355x: lightProbes failed: " << rt_last_error(ctx_) << std::endl;
        coeff.clear();
        return false;
    }
    return true;
}

bool Flyscene::lightProbesBounce(const int dims[3], int m, bool direct, float margin, int bounces, bool visible, rt_probe_grid &grid, std::vector<float> &coeff) {
    if (bounces < 0) {
        std::cerr << "rt_mi355x: lightProbesBounce failed: bounces must be >= 0" << std::endl;
        coeff.clear();
        return false;
    }
    if (!lightProbes(dims, m, direct && bounces == 0, margin, grid, coeff)) return false;
    if (bounces == 0) return true;
    const size_t probes = coeff.size() / RT_PROBE_COEFFS;
    std::vector<float> pos(probes * 3), other(coeff.size());
    rt_lights L;
    fill_lights(&L, lights_);
    bool ok = rt_probe_grid_positions(&grid, pos.data()) == RT_OK;
    for (int b = 1; ok && b <= bounces; ++b) {
        ok = rt_light_probes_bounce(ctx_, &L, static_cast<int>(probes), pos.data(), m, direct && b == bounces ? 1 : 0, &grid, coeff.data(), visible ? 1 : 0,
                                    other.data()) == RT_OK;
        coeff.swap(other);
    }
    if (!ok) {
        std::cerr << "rt_mi355x: lightProbesBounce failed: " << rt_last_error(ctx_) << std::endl;
        coeff.clear();
    }
    return ok;
}

bool Flyscene::indirectDiffuseBounce(const std::vector<Vec3f> &points, const std::vector<Vec3f> &normals, int m, unsigned seed, const rt_probe_grid &grid,
                                     const std::vector<float> &coeff, bool visible, std::vector<Vec3f> &out) {
    static_assert(sizeof(Vec3f) == 3 * sizeof(float), "Vec3f arrays are float[n*3]");
    out.clear();
    if (points.size() != normals.size() || points.size() > 0x7fffffffu) {
        std::cerr << "rt_mi355x: indirectDiffuseBounce failed: points and normals must have one size below 2^31" << std::endl;
        return false;
    }
    const bool grid_ok = grid.dims[0] >= 1 && grid.dims[1] >= 1 && grid.dims[2] >= 1 && static_cast<int64_t>(grid.dims[0]) * grid.dims[1] <= (1 << 24) &&
                         static_cast<int64_t>(grid.dims[0]) * grid.dims[1] * grid.dims[2] <= (1 << 24);
    if (!grid_ok || coeff.size() != static_cast<size_t>(grid.dims[0]) * static_cast<size_t>(grid.dims[1]) * static_cast<size_t>(grid.dims[2]) * RT_PROBE_COEFFS) {
        std::cerr << "rt_mi355x: indirectDiffuseBounce failed: coeff must hold 27 floats per probe of a valid grid" << std::endl;
        return false;
    }
    const int n = static_cast<int>(points.size());
    rt_lights L;
    fill_lights(&L, lights_);
    out.assign(points.size(), Vec3f{0.0f, 0.0f, 0.0f});
    if (rt_indirect_diffuse_bounce(ctx_, &L, n, n ? points[0].data() : nullptr, n ? normals[0].data() : nullptr, m, seed, &grid, coeff.data(), visible ? 1 : 0,
                                   n ? out[0].data() : nullptr) != RT_OK) {
        std::cerr << "rt_mi355x: indirectDiffuseBounce failed: " << rt_last_error(ctx_) << std::endl;
        out.clear();
        return false;
    }
    return true;
}

bool Flyscene::probeIrradiance(int width, int height, const rt_probe_grid &grid, const std::vector<float> &coeff, std::vector<Vec3f> &out) {
    return probeLookup("probeIrradiance", false, width, height, grid, coeff, out);
}

bool Flyscene::probeIrradianceVisible(int width, int height, const rt_probe_grid &grid, const std::vector<float> &coeff, std::vector<Vec3f> &out) {
    return probeLookup("probeIrradianceVisible", true, width, height, grid, coeff, out);
}

// both lookups: closest hits of the frame's pinhole rays -> point and normal -> rt_probe_irradiance or rt_probe_irradiance_visible
bool Flyscene::probeLookup(const char *who, bool visible, int width, int height, const rt_probe_grid &grid, const std::vector<float> &coeff,
                           std::vector<Vec3f> &out) {
    static_assert(sizeof(Vec3f) == 3 * sizeof(float), "Vec3f arrays are float[n*3]");
    if (width == 0 || height == 0) { width = view_w_; height = view_h_; }
    out.clear();
    if (!ctx_ || !scene_) {
        std::cerr << "rt_mi355x: " << who << " failed: " << rt_last_error(ctx_) << std::endl;
        return false;
    }
    if (width < 0 || height < 0 || static_cast<int64_t>(width) * height > 0x7fffffff) {
        std::cerr << "rt_mi355x: " << who << " failed: the frame must hold fewer than 2^31 pixels" << std::endl;
        return false;
    }
    const bool dims_ok = grid.dims[0] >= 1 && grid.dims[1] >= 1 && grid.dims[2] >= 1 && static_cast<int64_t>(grid.dims[0]) * grid.dims[1] <= (1 << 24) &&
                         static_cast<int64_t>(grid.dims[0]) * grid.dims[1] * grid.dims[2] <= (1 << 24);
    if (!dims_ok || coeff.size() != static_cast<size_t>(grid.dims[0]) * static_cast<size_t>(grid.dims[1]) * static_cast<size_t>(grid.dims[2]) * RT_PROBE_COEFFS) {
        std::cerr << "rt_mi355x: " << who << " failed: coeff must hold 27 floats per probe of the grid" << std::endl;
        return false;
    }
    rt_camera cam = camera_;
    if (width != view_w_ || height != view_h_) {
        rt_default_camera(&cam, width, height);
        std::memcpy(cam.center, camera_.center, sizeof cam.center);
        std::memcpy(cam.inv_view, camera_.inv_view, sizeof cam.inv_view);
    }
    const int n = width * height;
    const size_t pix = static_cast<size_t>(n);
    out.assign(pix, Vec3f{0.0f, 0.0f, 0.0f});
    if (n == 0) return true;
    // the pinhole rays of the frame, their closest hits, then point and normal by the rule of rt_hit_points_device: P = o + t * d, the face's
    // normal as uploaded with its signs flipped where it looks along the ray, six zeros for a miss
    rt_scene view;
    rt_host_scene_view(scene_, &view);
    std::vector<float> org(pix * 3), dir(pix * 3), ts(pix), nrm(pix * 3, 0.0f);
    std::vector<int32_t> faces(pix);
    rt_status s = rt_primary_points(ctx_, &cam, width, height, dir.data());
    for (size_t i = 0; s == RT_OK && i < pix; ++i)
        for (int k = 0; k < 3; ++k) { org[i * 3 + k] = cam.center[k]; dir[i * 3 + k] = dir[i * 3 + k] - cam.center[k]; }
    if (s == RT_OK) s = rt_closest_hits(ctx_, n, org.data(), dir.data(), faces.data(), ts.data());
    for (size_t i = 0; s == RT_OK && i < pix; ++i) {
        const int32_t f = faces[i];
        float *p = &org[i * 3], *nn = &nrm[i * 3];
        if (f < 0 || static_cast<uint32_t>(f) >= view.n_faces) { p[0] = p[1] = p[2] = 0.0f; continue; }
        const float *d = &dir[i * 3], *fn = view.face_normal + static_cast<size_t>(f) * 3;
        for (int k = 0; k < 3; ++k) p[k] = p[k] + ts[i] * d[k];
        const bool flip = (fn[0] * d[0] + fn[1] * d[1]) + fn[2] * d[2] > 0.0f;
        for (int k = 0; k < 3; ++k) nn[k] = flip ? -fn[k] : fn[k];
    }
    if (s == RT_OK)
        s = visible ? rt_probe_irradiance_visible(ctx_, &grid, coeff.data(), n, org.data(), nrm.data(), out[0].data(), nullptr)
                    : rt_probe_irradiance(ctx_, &grid, coeff.data(), n, org.data(), nrm.data(), out[0].data());
    if (s != RT_OK) {
        std::cerr << "rt_mi355x: " << who << " failed: " << rt_last_error(ctx_) << std::endl;
        out.clear();
        return false;
    }
    return true;
}

bool Flyscene::softShadows(int width, int height, const rt_shadow_params *params, std::vector<float> &out) {
    if (width == 0 || height == 0) { width = view_w_; height = view_h_; }
    out.clear();
    if (!ctx_) {                                            // (before initialize the viewport is 0 x 0: an empty frame must not pass for a result)
        std::cerr << "rt_mi355x: softShadows failed: " << rt_last_error(ctx_) << std::endl;
        return false;
    }
    if (width < 0 || height < 0 || static_cast<int64_t>(width) * height > 0x7fffffff) {
        std::cerr << "rt_mi355x: softShadows failed: the frame must hold fewer than 2^31 pixels" << std::endl;
        return false;
    }
    rt_camera cam = camera_;
    if (width != view_w_ || height != view_h_) {           // (an explicit size re-targets the perspective like initialize(w, h); camera_ stays)
        rt_default_camera(&cam, width, height);
        std::memcpy(cam.center, camera_.center, sizeof cam.center);
        std::memcpy(cam.inv_view, camera_.inv_view, sizeof cam.inv_view);
    }
    rt_shadow_params sp;
    rt_default_shadow_params(&sp);
    if (params) sp = *params;
    rt_lights L;
    fill_lights(&L, lights_);
    const int n = width * height;
    const size_t pix = static_cast<size_t>(n);
    out.assign(pix, 1.0f);
    if (n == 0) return true;
    // the pinhole rays of the frame, their closest hits, the hit points P = o + t * d; a normal of zeros marks a miss ("no point": share 1.0f),
    // any other normal a point (the call looks at nothing else of it)
    std::vector<float> org(pix * 3), dir(pix * 3), ts(pix), nrm(pix * 3, 0.0f);
    std::vector<int32_t> faces(pix);
    rt_status s = rt_primary_points(ctx_, &cam, width, height, dir.data());
    for (size_t i = 0; s == RT_OK && i < pix; ++i)
        for (int k = 0; k < 3; ++k) { org[i * 3 + k] = cam.center[k]; dir[i * 3 + k] = dir[i * 3 + k] - cam.center[k]; }
    if (s == RT_OK) s = rt_closest_hits(ctx_, n, org.data(), dir.data(), faces.data(), ts.data());
    for (size_t i = 0; s == RT_OK && i < pix; ++i) {
        if (faces[i] < 0) continue;
        for (int k = 0; k < 3; ++k) org[i * 3 + k] = org[i * 3 + k] + ts[i] * dir[i * 3 + k];
        nrm[i * 3 + 2] = 1.0f;
    }
    if (s == RT_OK) s = rt_soft_shadows(ctx_, &L, n, org.data(), nrm.data(), &sp, nullptr, out.data());
    if (s != RT_OK) {
        std::cerr << "rt_mi355x: softShadows failed: " << rt_last_error(ctx_) << std::endl;
        out.clear();
        return false;
    }
    return true;
}

std::vector<float> Flyscene::gbuffer(int width, int height) {
    rt_camera cam;
    rt_status s = frame_settings(width, height, cam);
    rt_params p{};
    p.width = width; p.height = height; p.max_depth = max_depth_;
    p.row0 = 0; p.row1 = height; p.stripe = 1; p.rank = 0; p.nranks = 1; p.collect_stats = 0;
    std::vector<float> out;
    if (s == RT_OK && width > 0 && height > 0) {
        out.assign(static_cast<size_t>(width) * height * RT_GBUFFER_CHANNELS, 0.f);
        s = rt_gbuffer(ctx_, &cam, &p, out.data());
    }
    if (s != RT_OK || out.empty()) {
        std::cerr << "rt_mi355x: gbuffer failed: " << rt_last_error(ctx_) << std::endl;
        out.clear();
    }
    return out;
}

std::vector<Vec3f> Flyscene::createSpherePoint(Vec3f p) {
    std::vector<Vec3f> out;
    if (pointLight) { out.push_back(p); return out; }
    if (!areaLight) {
        for (size_t i = 0; i + 2 < sphere_offsets_.size(); i += 3) out.push_back({sphere_offsets_[i] + p[0], sphere_offsets_[i + 1] + p[1], sphere_offsets_[i + 2] + p[2]});
        return out;
    }
    // createAreaLight(lightPoint, 0.3, 0.15, usteps, vsteps).getPointLights()  (flyscene.cpp:956-971, arealight.hpp:15-25)
    const float lx = static_cast<float>(0.3), ly = static_cast<float>(0.15);
    const float ux = p[0] + lx * 1.0f, uz = p[2] + lx * 0.0f, vy = p[1] + ly * 1.0f;
    for (int i = 0; i < usteps_; ++i)
        for (int j = 0; j < vsteps_; ++j)
            out.push_back({static_cast<float>(i + 0.5) * (ux / static_cast<float>(usteps_)),
                           static_cast<float>(j + 0.5) * (vy / static_cast<float>(vsteps_)), uz});
    return out;
}

void Flyscene::addLight() {
    if (lights_.size() < RT_MAX_LIGHTS) lights_.push_back({camera_.center[0], camera_.center[1], camera_.center[2]});
}

}  // namespace rtamd
