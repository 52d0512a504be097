// rt_render_main.cpp -- headless stand-in for the reference's src/main.cpp: initialize(), then the 'T' key
// (main.cpp:69-70 -> Flyscene::raytraceScene()).  Reads the same two stdin switches (flyscene.cpp:31-34).
//   usage: rt_render [--scene path.obj] [--size W H] [--samples U V] [--depth D] [--aa N] [--aa-threshold T] [--lens APERTURE FOCUS] [--shutter YAW] [--passes P] [--pass-tolerance T [MIN]] [--gbuffer PREFIX] [--denoise ITER SC SN SZ SA] [--upsample S [SN SZ SA]] [--temporal K DYAW [MAXLEN SN SZ SA]] [--probes DX DY DZ M [--probes-visible] [--probe-bounces B]] [--out result.ppm]
//   --aa N: N x N supersampling (anti-aliasing, 1..RT_MAX_SUPERSAMPLING; rt_set_supersampling)
//   --aa-threshold T: adaptive supersampling, refine only pixels on colour edges (rt_set_supersampling_threshold; T < 0 = every pixel)
//   --lens APERTURE FOCUS: thin-lens depth of field (rt_set_lens): lens radius in world units, depth of the plane in focus (2 = the model's centre)
//   --shutter YAW: camera motion blur (rt_set_shutter): the shutter opens on the default camera and closes on it yawed by YAW radians (rt_yaw_camera)
//   --passes P: multi-pass accumulation (rt_set_passes(0, P), 1..RT_MAX_PASSES): the frame is the mean of P jittered, reseeded passes
//   --pass-tolerance T [MIN]: adaptive pass counts (rt_set_pass_tolerance): a pixel stops after MIN passes (2..RT_MAX_PASSES, default 8) once the
//                             standard error of its mean is within T; prints the mean passes per pixel next to the time
//   --gbuffer PREFIX: the geometry buffers of the frame (rt_gbuffer: its camera and sample settings), three PFM files beside the image:
//                     PREFIX.geom.pfm = (alpha, depth, 0), PREFIX.normal.pfm = the face normal, PREFIX.albedo.pfm = the diffuse colour
//   --denoise ITER SC SN SZ SA: the frame is filtered before result.ppm is written (rt_denoise, guided by the frame's geometry buffers): ITER
//                     iterations (1..RT_DENOISE_MAX_ITERATIONS), then sigma_color, sigma_normal, sigma_depth, sigma_albedo (each > 0; inf = that
//                     guide never stops a tap).  Not with --pass-tolerance: an adaptive-pass frame has no geometry buffers
//   --upsample S [SN SZ SA]: the frame is rendered at ceil(W / S) x ceil(H / S) and brought to W x H with the guided upsample (rt_upsample; S in
//                     2..RT_UPSAMPLE_MAX_FACTOR), steered by the geometry buffers of both sizes; SN SZ SA: sigma_normal, sigma_depth, sigma_albedo
//                     (each > 0, inf allowed; default: rt_default_upsample_params).  --denoise then filters the low frame.  Not with --pass-tolerance
//   --temporal K DYAW [MAXLEN SN SZ SA]: K frames of a camera path, the last at the default camera and each earlier one DYAW radians less in yaw,
//                     each with its own passes, accumulated with the temporal reprojection (rt_reproject); the last accumulated frame is written.
//                     MAXLEN SN SZ SA: max_history (1..RT_REPROJECT_MAX_HISTORY), sigma_normal, sigma_depth, sigma_albedo (default:
//                     rt_default_reproject_params).  Composes with --aa, --passes and --denoise (which filters each accumulated frame; the history
//                     is the image before the filter).  Not with --pass-tolerance or --upsample
//   --probes DX DY DZ M: an irradiance volume of DX x DY x DZ light probes over the scene's root box, each traced with M x M rays
//                     (rt_light_probes, M in 1..RT_AO_MAX_GRID, the direct term included), looked up at the closest hits of the frame's camera
//                     (rt_probe_irradiance) and written as a PFM beside the image: <out>.probes.pfm
//   --probe-bounces B: with --probes, B feedback passes behind the first (rt_light_probes_bounce, B in 0..64): every pass lights the hits of
//                     the probe rays by the previous pass of the volume as well, one more diffuse bounce each; the direct term goes into the
//                     last pass; with --probes-visible the passes look the volume up leak-free, too
//   --probes-visible: with --probes, the lookup is rt_probe_irradiance_visible: each hit point blends the probes it can see, so the light of
//                     the next room does not leak through a partition thinner than a grid step
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "flyscene.hpp"

int main(int argc, char **argv) {
    int w = 1000, h = 1000;                    // WINDOW_WIDTH / WINDOW_HEIGHT, main.cpp:8-9
    rtamd::Flyscene scene;
    bool shutter = false;
    float shutter_yaw = 0.0f;
    int aa_n = 1;
    bool pass_tol_on = false;          // the frame is an adaptive-pass frame: T >= 0 and P > MIN (decided after the loop)
    float pass_tol = -1.0f;
    long pass_count = 1, pass_min = 8;
    std::string gbuffer_prefix;
    bool denoise = false;
    rt_denoise_params dn{};
    bool upsample = false;
    rt_upsample_params us{};
    bool temporal = false;
    long temporal_frames = 1;
    float temporal_dyaw = 0.0f;
    rt_reproject_params tp{};
    bool probes = false;
    bool probes_visible = false;
    int probe_bounces = -1;                          // -1: not given
    int probe_dims[3] = {1, 1, 1}, probe_m = 1;
    std::string out_path = "result.ppm";
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--scene") && i + 1 < argc) scene.setScenePath(argv[++i]);
        else if (!std::strcmp(argv[i], "--size") && i + 2 < argc) { w = std::atoi(argv[++i]); h = std::atoi(argv[++i]); }
        else if (!std::strcmp(argv[i], "--samples") && i + 2 < argc) { const int u = std::atoi(argv[++i]); scene.setAreaGrid(u, std::atoi(argv[++i])); }
        else if (!std::strcmp(argv[i], "--depth") && i + 1 < argc) scene.setMaxDepth(std::atoi(argv[++i]));
        else if (!std::strcmp(argv[i], "--aa") && i + 1 < argc) {
            const int aa = std::atoi(argv[++i]);
            if (aa < 1 || aa > RT_MAX_SUPERSAMPLING) { std::fprintf(stderr, "--aa: N must be in 1..%d\n", RT_MAX_SUPERSAMPLING); return 2; }
            scene.setSupersampling(aa);
            aa_n = aa;
        }
        else if (!std::strcmp(argv[i], "--aa-threshold") && i + 1 < argc) {
            const char *arg = argv[++i];
            char *end = nullptr;
            const float t = std::strtof(arg, &end);
            if (end == arg || *end != '\0' || std::isnan(t)) { std::fprintf(stderr, "--aa-threshold: T must be a number (not NaN)\n"); return 2; }
            scene.setSupersamplingThreshold(t);
        }
        else if (!std::strcmp(argv[i], "--lens") && i + 2 < argc) {
            float v[2];
            for (int k = 0; k < 2; ++k) {
                const char *arg = argv[++i];
                char *end = nullptr;
                v[k] = std::strtof(arg, &end);
                if (end == arg || *end != '\0' || !std::isfinite(v[k])) { std::fprintf(stderr, "--lens: APERTURE and FOCUS must be finite numbers\n"); return 2; }
            }
            if (v[0] < 0.0f || (v[0] > 0.0f && !(v[1] > 0.0f))) { std::fprintf(stderr, "--lens: APERTURE must be >= 0 and, when it is > 0, FOCUS > 0\n"); return 2; }
            scene.setLens(v[0], v[1]);
        }
        else if (!std::strcmp(argv[i], "--shutter") && i + 1 < argc) {
            const char *arg = argv[++i];
            char *end = nullptr;
            shutter_yaw = std::strtof(arg, &end);
            if (end == arg || *end != '\0' || !std::isfinite(shutter_yaw)) { std::fprintf(stderr, "--shutter: YAW must be a finite number (radians)\n"); return 2; }
            shutter = true;
        }
        else if (!std::strcmp(argv[i], "--passes") && i + 1 < argc) {
            const char *arg = argv[++i];
            char *end = nullptr;
            const long passes = std::strtol(arg, &end, 10);
            if (end == arg || *end != '\0' || passes < 1 || passes > RT_MAX_PASSES) { std::fprintf(stderr, "--passes: P must be in 1..%d\n", RT_MAX_PASSES); return 2; }
            scene.setPasses(static_cast<int>(passes));
            pass_count = passes;
        }
        else if (!std::strcmp(argv[i], "--pass-tolerance") && i + 1 < argc) {
            const char *arg = argv[++i];
            char *end = nullptr;
            const float t = std::strtof(arg, &end);
            if (end == arg || *end != '\0' || std::isnan(t)) { std::fprintf(stderr, "--pass-tolerance: T must be a number (not NaN)\n"); return 2; }
            long min_passes = 8;
            if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) {         // the optional MIN
                arg = argv[++i];
                min_passes = std::strtol(arg, &end, 10);
                if (end == arg || *end != '\0' || min_passes < 2 || min_passes > RT_MAX_PASSES) { std::fprintf(stderr, "--pass-tolerance: MIN must be in 2..%d\n", RT_MAX_PASSES); return 2; }
            }
            scene.setPassTolerance(t, static_cast<int>(min_passes));
            pass_tol = t; pass_min = min_passes;
        }
        else if (!std::strcmp(argv[i], "--gbuffer") && i + 1 < argc) gbuffer_prefix = argv[++i];
        else if (!std::strcmp(argv[i], "--denoise") && i + 5 < argc) {
            const char *arg = argv[++i];
            char *end = nullptr;
            const long it = std::strtol(arg, &end, 10);
            if (end == arg || *end != '\0' || it < 1 || it > RT_DENOISE_MAX_ITERATIONS) { std::fprintf(stderr, "--denoise: ITER must be in 1..%d\n", RT_DENOISE_MAX_ITERATIONS); return 2; }
            float v[4];
            for (int k = 0; k < 4; ++k) {
                arg = argv[++i];
                v[k] = std::strtof(arg, &end);
                if (end == arg || *end != '\0' || !(v[k] > 0.0f)) { std::fprintf(stderr, "--denoise: SC, SN, SZ and SA must be numbers > 0 (inf is allowed)\n"); return 2; }
            }
            dn.iterations = static_cast<int32_t>(it);
            dn.sigma_color = v[0]; dn.sigma_normal = v[1]; dn.sigma_depth = v[2]; dn.sigma_albedo = v[3];
            denoise = true;
        }
        else if (!std::strcmp(argv[i], "--upsample") && i + 1 < argc) {
            const char *arg = argv[++i];
            char *end = nullptr;
            const long f = std::strtol(arg, &end, 10);
            if (end == arg || *end != '\0' || f < 2 || f > RT_UPSAMPLE_MAX_FACTOR) { std::fprintf(stderr, "--upsample: S must be in 2..%d\n", RT_UPSAMPLE_MAX_FACTOR); return 2; }
            rt_default_upsample_params(&us);
            us.factor = static_cast<int32_t>(f);
            if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) {          // the three sigmas follow
                if (i + 3 >= argc) { std::fprintf(stderr, "--upsample: SN, SZ and SA come together\n"); return 2; }
                float v[3];
                for (int k = 0; k < 3; ++k) {
                    arg = argv[++i];
                    v[k] = std::strtof(arg, &end);
                    if (end == arg || *end != '\0' || !(v[k] > 0.0f)) { std::fprintf(stderr, "--upsample: SN, SZ and SA must be numbers > 0 (inf is allowed)\n"); return 2; }
                }
                us.sigma_normal = v[0]; us.sigma_depth = v[1]; us.sigma_albedo = v[2];
            }
            upsample = true;
        }
        else if (!std::strcmp(argv[i], "--temporal") && i + 2 < argc) {
            const char *arg = argv[++i];
            char *end = nullptr;
            temporal_frames = std::strtol(arg, &end, 10);
            if (end == arg || *end != '\0' || temporal_frames < 1 || temporal_frames > 4096) { std::fprintf(stderr, "--temporal: K must be in 1..4096\n"); return 2; }
            arg = argv[++i];
            temporal_dyaw = std::strtof(arg, &end);
            if (end == arg || *end != '\0' || !std::isfinite(temporal_dyaw)) { std::fprintf(stderr, "--temporal: DYAW must be a finite number (radians)\n"); return 2; }
            rt_default_reproject_params(&tp);
            if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) {          // MAXLEN and the three sigmas follow
                if (i + 4 >= argc) { std::fprintf(stderr, "--temporal: MAXLEN, SN, SZ and SA come together\n"); return 2; }
                arg = argv[++i];
                const long mh = std::strtol(arg, &end, 10);
                if (end == arg || *end != '\0' || mh < 1 || mh > RT_REPROJECT_MAX_HISTORY) { std::fprintf(stderr, "--temporal: MAXLEN must be in 1..%d\n", RT_REPROJECT_MAX_HISTORY); return 2; }
                float v[3];
                for (int k = 0; k < 3; ++k) {
                    arg = argv[++i];
                    v[k] = std::strtof(arg, &end);
                    if (end == arg || *end != '\0' || !(v[k] > 0.0f)) { std::fprintf(stderr, "--temporal: SN, SZ and SA must be numbers > 0 (inf is allowed)\n"); return 2; }
                }
                tp.max_history = static_cast<int32_t>(mh);
                tp.sigma_normal = v[0]; tp.sigma_depth = v[1]; tp.sigma_albedo = v[2];
            }
            temporal = true;
        }
        else if (!std::strcmp(argv[i], "--probes") && i + 4 < argc) {
            long v[4];
            for (int k = 0; k < 4; ++k) {
                const char *arg = argv[++i];
                char *end = nullptr;
                v[k] = std::strtol(arg, &end, 10);
                if (end == arg || *end != '\0' || v[k] < 1 || v[k] > (k < 3 ? 4096 : RT_AO_MAX_GRID)) { std::fprintf(stderr, "--probes: DX, DY and DZ must be in 1..4096 and M in 1..%d\n", RT_AO_MAX_GRID); return 2; }
            }
            if (v[0] * v[1] * v[2] > (1L << 24)) { std::fprintf(stderr, "--probes: at most 2^24 probes\n"); return 2; }
            for (int k = 0; k < 3; ++k) probe_dims[k] = static_cast<int>(v[k]);
            probe_m = static_cast<int>(v[3]);
            probes = true;
        }
        else if (!std::strcmp(argv[i], "--probes-visible")) probes_visible = true;
        else if (!std::strcmp(argv[i], "--probe-bounces") && i + 1 < argc) {
            char *end = nullptr;
            const char *arg = argv[++i];
            const long v = std::strtol(arg, &end, 10);
            if (end == arg || *end != '\0' || v < 0 || v > 64) { std::fprintf(stderr, "--probe-bounces: B must be in 0..64\n"); return 2; }
            probe_bounces = static_cast<int>(v);
        }
        else if (!std::strcmp(argv[i], "--out") && i + 1 < argc) { out_path = argv[++i]; scene.setOutputPath(out_path); }
        else { std::fprintf(stderr, "usage: %s [--scene obj] [--size W H] [--samples U V] [--depth D] [--aa N] [--aa-threshold T] [--lens APERTURE FOCUS] [--shutter YAW] [--passes P] [--pass-tolerance T [MIN]] [--gbuffer PREFIX] [--denoise ITER SC SN SZ SA] [--upsample S [SN SZ SA]] [--temporal K DYAW [MAXLEN SN SZ SA]] [--probes DX DY DZ M [--probes-visible] [--probe-bounces B]] [--out ppm]\n", argv[0]); return 2; }
    }
    if (w <= 0 || h <= 0) return 2;
    if (probes_visible && !probes) { std::fprintf(stderr, "--probes-visible needs --probes\n"); return 2; }
    if (probe_bounces >= 0 && !probes) { std::fprintf(stderr, "--probe-bounces needs --probes\n"); return 2; }
    pass_tol_on = pass_tol >= 0.0f && pass_count > pass_min;
    if (denoise && pass_tol >= 0.0f) { std::fprintf(stderr, "--denoise: not with --pass-tolerance (an adaptive-pass frame has no geometry buffers)\n"); return 2; }
    if (denoise) scene.setDenoise(&dn);
    if (upsample && pass_tol >= 0.0f) { std::fprintf(stderr, "--upsample: not with --pass-tolerance (an adaptive-pass frame has no geometry buffers)\n"); return 2; }
    if (upsample) scene.setUpsample(&us);
    if (temporal && pass_tol >= 0.0f) { std::fprintf(stderr, "--temporal: not with --pass-tolerance (an adaptive-pass frame has no geometry buffers)\n"); return 2; }
    if (temporal && upsample) { std::fprintf(stderr, "--temporal: not with --upsample\n"); return 2; }
    if (temporal) scene.setTemporal(&tp);
    if (shutter) {                             // (after the loop: --size may follow --shutter)
        rt_camera close;
        rt_yaw_camera(&close, w, h, shutter_yaw);
        scene.setShutter(&close);
    }
    scene.initialize(w, h);
    if (temporal) {                            // frames 0 .. K - 2 of the path: frame j at yaw -(float)(K - 1 - j) * DYAW; the last, below, at the default camera
        for (long j = 0; j + 1 < temporal_frames; ++j) {
            rt_yaw_camera(scene.getCamera(), w, h, -static_cast<float>(temporal_frames - 1 - j) * temporal_dyaw);
            scene.raytraceScene();
            if (scene.lastStatus() != RT_OK) return 1;
        }
        rt_default_camera(scene.getCamera(), w, h);
    }
    scene.raytraceScene();
    if (scene.lastStatus() != RT_OK) return 1;          // no result.ppm was written: say so with the exit code
    const rt_stats &st = scene.lastStats();
    std::printf("device ms: trace %.3f shadow %.3f shade %.3f resolve %.3f total %.3f", st.ms_trace, st.ms_shadow, st.ms_shade, st.ms_resolve, st.ms_total);
    // (rt_stats::pixels counts the traced sub-samples of every pass: n*n per output pixel and pass taken)
    if (pass_tol_on) std::printf("  mean passes per pixel %.2f", static_cast<double>(st.pixels) / (static_cast<double>(aa_n) * aa_n * static_cast<double>(w) * h));
    std::printf("\n");
    if (!gbuffer_prefix.empty()) {
        const std::vector<float> g = scene.gbuffer();
        if (g.empty()) return 1;
        const size_t pix = static_cast<size_t>(w) * static_cast<size_t>(h);
        std::vector<float> rgb(pix * 3);
        const struct { const char *name; int c0; bool depth_pair; } files[] = {{".geom.pfm", 0, true}, {".normal.pfm", 2, false}, {".albedo.pfm", 5, false}};
        for (const auto &f : files) {
            for (size_t q = 0; q < pix; ++q) {
                const float *v = &g[q * RT_GBUFFER_CHANNELS + static_cast<size_t>(f.c0)];
                rgb[q * 3] = v[0]; rgb[q * 3 + 1] = v[1]; rgb[q * 3 + 2] = f.depth_pair ? 0.0f : v[2];
            }
            const std::string path = gbuffer_prefix + f.name;
            if (rt_write_pfm(path.c_str(), rgb.data(), w, h) != RT_OK) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
        }
    }
    if (probes) {
        rt_probe_grid grid{};
        std::vector<float> coeff;
        std::vector<rtamd::Vec3f> img;
        if (!scene.lightProbesBounce(probe_dims, probe_m, true, 0.0f, probe_bounces > 0 ? probe_bounces : 0, probes_visible, grid, coeff) || !(probes_visible ? scene.probeIrradianceVisible(w, h, grid, coeff, img) : scene.probeIrradiance(w, h, grid, coeff, img))) return 1;
        const std::string path = out_path + ".probes.pfm";
        if (rt_write_pfm(path.c_str(), img[0].data(), w, h) != RT_OK) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
    }
    return 0;
}
