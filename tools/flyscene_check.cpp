// flyscene_check.cpp -- a user of rtamd::Flyscene (csrc/flyscene.hpp) that runs one group of calls in one process and writes every result to a
// file, for tests/test_gpu_cpp_facade.py and tests/test_cpp_facade_api.py to compare with the CPU checker, the numpy restatements and the Python
// mirror.  It includes the facade's header and the public header only.
//   usage: flyscene_check [--host] GROUP SCENE.obj INPUT OUTPUT
//   GROUP: host | trace | strikes | hits | ao | shadow | indirect | probes | probes_visible | probes_bounce | closest_points | ray_hits | lights | state | post | temporal | objects.  --host: no call of initialize (no device).
//   INPUT / OUTPUT: a sequence of arrays, each a text line "name type ndim dim0 dim1 ...\n" (type f4, i4, u1, u2 or u8, little-endian) followed by
//   the raw elements.  Exit status 0: every call returned what the group expects (the calls that must fail included).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "flyscene.hpp"

using rtamd::Flyscene;
using rtamd::Vec3f;

namespace {

struct Arr {
    std::string type;
    std::vector<long> shape;
    std::vector<unsigned char> bytes;
};

std::map<std::string, Arr> g_in;
std::ofstream g_out;
int g_fail = 0;

#define EXPECT(c)                                                                              \
    do {                                                                                       \
        if (!(c)) {                                                                            \
            std::fprintf(stderr, "flyscene_check: line %d: expected %s\n", __LINE__, #c);      \
            ++g_fail;                                                                          \
        }                                                                                      \
    } while (0)

size_t item_size(const std::string &type) { return type.size() == 2 ? static_cast<size_t>(type[1] - '0') : 0; }

bool read_arrays(const char *path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream s(line);
        std::string name;
        Arr a;
        int ndim = 0;
        s >> name >> a.type >> ndim;
        size_t n = item_size(a.type);
        if (!s || n == 0 || ndim < 0 || ndim > 8) return false;
        for (int i = 0; i < ndim; ++i) {
            long d = 0;
            s >> d;
            if (!s || d < 0) return false;
            a.shape.push_back(d);
            n *= static_cast<size_t>(d);
        }
        a.bytes.resize(n);
        if (n) f.read(reinterpret_cast<char *>(a.bytes.data()), static_cast<std::streamsize>(n));
        if (!f) return false;
        g_in[name] = a;
    }
    return true;
}

void put(const std::string &name, const char *type, const std::vector<long> &shape, const void *data) {
    size_t n = item_size(type);
    g_out << name << ' ' << type << ' ' << shape.size();
    for (long d : shape) { g_out << ' ' << d; n *= static_cast<size_t>(d); }
    g_out << '\n';
    if (n) g_out.write(static_cast<const char *>(data), static_cast<std::streamsize>(n));
}

const Arr &in(const std::string &name) {
    auto it = g_in.find(name);
    if (it == g_in.end()) { std::fprintf(stderr, "flyscene_check: the input holds no array %s\n", name.c_str()); std::exit(2); }
    return it->second;
}

template <class T> std::vector<T> in_vec(const std::string &name) {
    const Arr &a = in(name);
    std::vector<T> v(a.bytes.size() / sizeof(T));
    if (!v.empty()) std::memcpy(v.data(), a.bytes.data(), v.size() * sizeof(T));
    return v;
}

std::vector<Vec3f> in_v3(const std::string &name) { return in_vec<Vec3f>(name); }
std::string in_str(const std::string &name) { const Arr &a = in(name); return std::string(a.bytes.begin(), a.bytes.end()); }

void put_f(const std::string &name, const std::vector<float> &v, const std::vector<long> &shape) { put(name, "f4", shape, v.data()); }
void put_v3(const std::string &name, const std::vector<Vec3f> &v) { put(name, "f4", {static_cast<long>(v.size()), 3}, v.data()); }
void put_u8(const std::string &name, const std::vector<uint8_t> &v, const std::vector<long> &shape) { put(name, "u1", shape, v.data()); }
void put_flag(const std::string &name, bool b) { const uint8_t v = b ? 1 : 0; put(name, "u1", {1}, &v); }

bool exists(const std::string &path) { std::ifstream f(path); return static_cast<bool>(f); }

std::string g_ppm;        // where the frames of this run go

void frame(Flyscene &fs, const std::string &name, int w, int h, int W = 0, int H = 0) {
    fs.raytraceScene(W, H);
    EXPECT(fs.lastStatus() == RT_OK);
    EXPECT(fs.lastImage().size() == static_cast<size_t>(w) * h * 3);
    put_f(name, fs.lastImage(), {h, w, 3});
}

void buffers(Flyscene &fs, const std::string &name, int w, int h, int W = 0, int H = 0) {
    const std::vector<float> g = fs.gbuffer(W, H);
    EXPECT(g.size() == static_cast<size_t>(w) * h * RT_GBUFFER_CHANNELS);
    put_f(name, g, {h, w, RT_GBUFFER_CHANNELS});
}

void put_stats(const std::string &name, const rt_stats &s) {
    const uint64_t v[12] = {s.rays_primary, s.rays_bounce, s.rays_centre, s.rays_sample, s.pixels, s.pixels_culled, s.shaded_hits, s.rays_sample_walked,
                            s.launches_trace, s.launches_shadow, s.launches_shade, s.launches_total};
    put(name, "u8", {12}, v);
}

void yaw_camera(Flyscene &fs, int w, int h, float yaw) {
    if (yaw != 0.0f) rt_yaw_camera(fs.getCamera(), w, h, yaw);
    else rt_default_camera(fs.getCamera(), w, h);
}

const float kSentinel = 12345.0f;

// the refusals of the stand-alone denoise / upsample / reproject: a vector one element short, channels = 2, width = 0 -> false with the outputs
// as they were; on an object with a device also height = 0 -> true with empty outputs
void shape_refusals(Flyscene &fs, bool has_device) {
    const int w = 6, h = 4;
    const size_t pix = static_cast<size_t>(w) * h;
    const std::vector<float> img(pix, 0.5f), g(pix * RT_GBUFFER_CHANNELS, 1.0f), low(3 * 2, 0.5f), gl(3 * 2 * RT_GBUFFER_CHANNELS, 1.0f), none;
    const std::vector<float> img2(pix * 2, 0.5f), low2(3 * 2 * 2, 0.5f);
    const std::vector<uint8_t> len(pix, 1), no_len;
    std::vector<float> short_img(img), short_g(g), short_low(low);
    short_img.pop_back(); short_g.pop_back(); short_low.pop_back();
    std::vector<uint8_t> short_len(len);
    short_len.pop_back();
    const float m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const std::vector<float> keep{kSentinel, kSentinel};
    const std::vector<uint8_t> keep8{0xA5, 0xA5, 0xA5};
    std::vector<float> out = keep;
    std::vector<uint8_t> out8 = keep8;
    // denoise
    EXPECT(!fs.denoise(short_img, 1, g, w, h, nullptr, out) && out == keep);
    EXPECT(!fs.denoise(img, 1, short_g, w, h, nullptr, out) && out == keep);
    EXPECT(!fs.denoise(img2, 2, g, w, h, nullptr, out) && out == keep);
    EXPECT(!fs.denoise(none, 1, none, 0, h, nullptr, out) && out == keep);
    // upsample (factor 2: 6 x 4 from 3 x 2)
    EXPECT(!fs.upsample(short_low, 1, gl, g, w, h, nullptr, out, &out8) && out == keep && out8 == keep8);
    EXPECT(!fs.upsample(low, 1, gl, short_g, w, h, nullptr, out, &out8) && out == keep && out8 == keep8);
    EXPECT(!fs.upsample(low2, 2, gl, g, w, h, nullptr, out, &out8) && out == keep && out8 == keep8);
    EXPECT(!fs.upsample(none, 1, none, none, 0, h, nullptr, out, &out8) && out == keep && out8 == keep8);
    // reproject
    EXPECT(!fs.reproject(short_img, 1, g, img, g, len, w, h, m, nullptr, out, out8) && out == keep && out8 == keep8);
    EXPECT(!fs.reproject(img, 1, g, img, g, short_len, w, h, m, nullptr, out, out8) && out == keep && out8 == keep8);
    EXPECT(!fs.reproject(img2, 2, g, img2, g, len, w, h, m, nullptr, out, out8) && out == keep && out8 == keep8);
    EXPECT(!fs.reproject(none, 1, none, none, none, no_len, 0, h, m, nullptr, out, out8) && out == keep && out8 == keep8);
    if (has_device) {
        EXPECT(fs.denoise(none, 1, none, w, 0, nullptr, out) && out.empty());
        out = keep;
        EXPECT(fs.upsample(none, 1, none, none, w, 0, nullptr, out, &out8) && out.empty() && out8.empty());
        out = keep; out8 = keep8;
        EXPECT(fs.reproject(none, 1, none, none, none, no_len, w, 0, m, nullptr, out, out8) && out.empty() && out8.empty());
    }
}

// lightStrikes with canary bytes around the bool array -> the return value; vis gets the n elements as bytes.  false: a canary was written
bool strikes_guarded(Flyscene &fs, Vec3f p, std::vector<Vec3f> &lights, bool *ret, uint8_t *vis) {
    unsigned char raw[8 + RT_MAX_LIGHTS + 8];
    std::memset(raw, 0xA5, sizeof raw);
    const size_t n = lights.size();
    *ret = fs.lightStrikes(p, lights, reinterpret_cast<bool *>(raw + 8));
    if (vis) std::memcpy(vis, raw + 8, n);
    for (size_t i = 0; i < sizeof raw; ++i)
        if ((i < 8 || i >= 8 + n) && raw[i] != 0xA5) return false;
    return true;
}

void sample_grids(Flyscene &fs, const std::string &mode, Vec3f p) {
    const int grids[4][2] = {{1, 1}, {5, 5}, {3, 7}, {32, 32}};
    for (const auto &gr : grids) {
        fs.setAreaGrid(gr[0], gr[1]);
        put_v3("csp_" + mode + "_" + std::to_string(gr[0]) + "x" + std::to_string(gr[1]), fs.createSpherePoint(p));
    }
    fs.setAreaGrid(5, 5);
}

const char *kModes[3] = {"area", "point", "sphere"};
const bool kArea[3] = {true, false, false}, kPoint[3] = {false, true, false};

// ---- an object that was never initialised: every member fails cleanly
void group_host() {
    Flyscene fs;
    fs.setOutputPath(g_ppm);
    EXPECT(!fs.ok());
    Vec3f o{0.f, 0.f, 2.f}, d{0.f, 0.f, -1.f};
    std::vector<Vec3f> lights{{-1.f, 1.f, 1.f}};
    const Vec3f c = fs.traceRay(o, d, 0, lights, false);
    const Vec3f zero{0.f, 0.f, 0.f};
    EXPECT(std::memcmp(c.data(), zero.data(), sizeof zero) == 0);
    bool ret = true;
    uint8_t vis[RT_MAX_LIGHTS];
    EXPECT(strikes_guarded(fs, o, lights, &ret, vis) && !ret && vis[0] == 0xA5);
    std::vector<Vec3f> one{o}, dir{d};
    std::vector<int> faces;
    std::vector<float> ts, out{kSentinel};
    std::vector<unsigned short> open;
    EXPECT(!fs.closestHits(one, dir, faces, ts));
    EXPECT(!fs.ambientOcclusion(one, dir, 1, 0.5f, 0, open));
    EXPECT(!fs.softShadows(0, 0, nullptr, out) && out.empty());
    out.assign(1, kSentinel);
    EXPECT(!fs.softShadows(40, 24, nullptr, out) && out.empty());
    EXPECT(fs.gbuffer().empty());
    EXPECT(fs.gbuffer(40, 24).empty());
    std::remove(g_ppm.c_str());
    fs.raytraceScene();
    EXPECT(fs.lastStatus() != RT_OK && !exists(g_ppm));
    fs.raytraceScene(16, 12);
    EXPECT(fs.lastStatus() != RT_OK && !exists(g_ppm));
    rt_reproject_params rp;
    rt_default_reproject_params(&rp);
    fs.setTemporal(&rp);
    fs.raytraceScene(16, 12);
    EXPECT(fs.lastStatus() != RT_OK && !exists(g_ppm) && fs.historyLengths().empty());
    fs.setTemporal(nullptr);
    fs.resetHistory();
    const rt_stats &s = fs.lastStats();
    EXPECT(s.rays_primary == 0 && s.pixels == 0 && s.launches_total == 0);
    // the stand-alone filters need a device: valid shapes fail, refused shapes leave the outputs alone
    const std::vector<float> img(6 * 4, 0.5f), g(6 * 4 * RT_GBUFFER_CHANNELS, 1.0f), low(3 * 2, 0.5f), gl(3 * 2 * RT_GBUFFER_CHANNELS, 1.0f);
    const std::vector<uint8_t> len(6 * 4, 1);
    const float m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::vector<uint8_t> out8;
    EXPECT(!fs.denoise(img, 1, g, 6, 4, nullptr, out));
    EXPECT(!fs.upsample(low, 1, gl, g, 6, 4, nullptr, out, &out8));
    EXPECT(!fs.reproject(img, 1, g, img, g, len, 6, 4, m, nullptr, out, out8));
    shape_refusals(fs, false);
    // the sample grids are host arithmetic
    const std::vector<Vec3f> p = in_v3("p");
    for (int k = 0; k < 2; ++k) {
        fs.setLightMode(kArea[k], kPoint[k]);
        sample_grids(fs, kModes[k], p[0]);
    }
    fs.addLight();
    EXPECT(fs.getLights().size() == 1);        // (initialize gives the object its first light; before it the list is empty)
}

// ---- a. traceRay, one call per ray
void group_trace(const std::string &scene) {
    std::vector<Vec3f> o = in_v3("o"), d = in_v3("d"), three = in_v3("three");
    const long n = static_cast<long>(o.size());
    Flyscene fs;
    fs.setScenePath(scene);
    fs.setOutputPath(g_ppm);
    for (int k = 0; k < 3; ++k) {
        fs.initialize(48, 32, kArea[k], kPoint[k]);
        fs.setAreaGrid(5, 5);
        for (int md : {3, -1}) {
            fs.setMaxDepth(md);
            for (int level : {0, 1, 3, 5})
                for (int li = 0; li < 2; ++li) {
                    std::vector<Vec3f> lights = li ? three : fs.getLights();
                    std::vector<float> out(static_cast<size_t>(n) * 3);
                    for (long r = 0; r < n; ++r) {
                        const Vec3f c = fs.traceRay(o[r], d[r], level, lights, r % 2 == 0);
                        std::memcpy(&out[r * 3], c.data(), sizeof c);
                    }
                    put_f(std::string("trace_") + kModes[k] + "_" + std::to_string(md) + "_" + std::to_string(level) + (li ? "_three" : "_own"), out, {n, 3});
                }
        }
    }
}

// ---- b. lightStrikes
void group_strikes(const std::string &scene) {
    const std::vector<Vec3f> pts = in_v3("pts");
    Flyscene fs;
    fs.setScenePath(scene);
    fs.initialize(48, 32, true, false);
    for (const char *name : {"l1", "l3", "l25"}) {
        std::vector<Vec3f> lights = in_v3(name);
        const size_t n = lights.size();
        std::vector<uint8_t> vis(pts.size() * n), ret(pts.size());
        bool clean = true;
        for (size_t i = 0; i < pts.size(); ++i) {
            bool r = false;
            clean = strikes_guarded(fs, pts[i], lights, &r, &vis[i * n]) && clean;
            ret[i] = r ? 1 : 0;
        }
        EXPECT(clean);
        put_u8(std::string("vis_") + name, vis, {static_cast<long>(pts.size()), static_cast<long>(n)});
        put_u8(std::string("ret_") + name, ret, {static_cast<long>(pts.size())});
    }
    std::vector<Vec3f> none;
    bool r = true;
    EXPECT(strikes_guarded(fs, pts[0], none, &r, nullptr) && !r);
}

// ---- c. closestHits
void group_hits(const std::string &scene) {
    const std::vector<Vec3f> o = in_v3("o"), d = in_v3("d");
    Flyscene fs;
    fs.setScenePath(scene);
    fs.initialize(48, 32, true, false);
    std::vector<int> faces{7, 7};
    std::vector<float> ts{7.f};
    EXPECT(fs.closestHits(o, d, faces, ts) && faces.size() == o.size() && ts.size() == o.size());
    put("faces", "i4", {static_cast<long>(faces.size())}, faces.data());
    put_f("ts", ts, {static_cast<long>(ts.size())});
    std::vector<Vec3f> fewer(d);
    fewer.pop_back();
    EXPECT(!fs.closestHits(o, fewer, faces, ts));
    EXPECT(!fs.closestHits(fewer, d, faces, ts));
    const std::vector<Vec3f> none;
    faces.assign(2, 7); ts.assign(1, 7.f);
    EXPECT(fs.closestHits(none, none, faces, ts) && faces.empty() && ts.empty());
}

// ---- d. ambientOcclusion
void group_ao(const std::string &scene) {
    const std::vector<Vec3f> P = in_v3("P"), N = in_v3("N");
    const float radius = in_vec<float>("radius")[0];
    Flyscene fs;
    fs.setScenePath(scene);
    fs.initialize(48, 32, true, false);
    std::vector<unsigned short> open;
    for (int m : {1, 3, 16})
        for (unsigned seed : {0u, 3u}) {
            EXPECT(fs.ambientOcclusion(P, N, m, radius, seed, open) && open.size() == P.size());
            put("open_" + std::to_string(m) + "_" + std::to_string(seed), "u2", {static_cast<long>(open.size())}, open.data());
        }
    EXPECT(!fs.ambientOcclusion(P, N, 0, radius, 0, open));
    EXPECT(!fs.ambientOcclusion(P, N, 17, radius, 0, open));
    const float inf = std::numeric_limits<float>::infinity();
    for (float r : {0.0f, -1.0f, std::nanf(""), inf, -inf}) EXPECT(!fs.ambientOcclusion(P, N, 3, r, 0, open));
    std::vector<Vec3f> fewer(N);
    fewer.pop_back();
    EXPECT(!fs.ambientOcclusion(P, fewer, 3, radius, 0, open));
    EXPECT(!fs.ambientOcclusion(fewer, N, 3, radius, 0, open));
    const std::vector<Vec3f> none;
    open.assign(2, 7);
    EXPECT(fs.ambientOcclusion(none, none, 3, radius, 0, open) && open.empty());
}

// ---- e. softShadows
void group_shadow(const std::string &scene) {
    const std::vector<Vec3f> one = in_v3("one"), three = in_v3("three");
    const std::vector<float> pass5 = in_vec<float>("pass5");
    rt_shadow_params centre, offsets, jitter;
    rt_default_shadow_params(&centre);
    offsets = centre; offsets.fu = pass5[0]; offsets.fv = pass5[1];
    jitter = centre; jitter.per_point = 1; jitter.seed = 7u;
    const rt_shadow_params *params[3] = {nullptr, &offsets, &jitter};
    const char *pnames[3] = {"null", "pass5", "seed7"};
    Flyscene fs;
    fs.setScenePath(scene);
    fs.setOutputPath(g_ppm);
    fs.setMaxDepth(3);
    const struct { const char *name; bool area, point; int u, v; } modes[3] = {{"a55", true, false, 5, 5}, {"a37", true, false, 3, 7}, {"point", false, true, 5, 5}};
    for (int k = 0; k < 3; ++k) {
        if (k != 1) fs.initialize(48, 32, modes[k].area, modes[k].point);
        fs.setAreaGrid(5, 5);
        fs.getLights() = one;
        if (k == 0) frame(fs, "before", 48, 32);
        fs.setAreaGrid(modes[k].u, modes[k].v);
        for (int li = 0; li < 2; ++li) {
            fs.getLights() = li ? three : one;
            for (int big = 0; big < 2; ++big)
                for (int q = 0; q < 3; ++q) {
                    const int w = big ? 40 : 48, h = big ? 24 : 32;
                    std::vector<float> out{kSentinel};
                    EXPECT(fs.softShadows(big ? 40 : 0, big ? 24 : 0, params[q], out) && out.size() == static_cast<size_t>(w) * h);
                    put_f(std::string("shadow_") + modes[k].name + "_" + (li ? "3" : "1") + "_" + std::to_string(w) + "_" + pnames[q], out, {h, w});
                }
        }
        if (k == 1) {
            fs.setAreaGrid(5, 5);
            fs.getLights() = one;
            frame(fs, "after", 48, 32);
        }
    }
    fs.initialize(48, 32, false, false);
    std::vector<float> out{kSentinel, kSentinel};
    EXPECT(!fs.softShadows(0, 0, nullptr, out) && out.empty());
    // parameters out of range
    rt_shadow_params bad = centre;
    bad.fu = 1.0f;
    fs.initialize(48, 32, true, false);
    out.assign(2, kSentinel);
    EXPECT(!fs.softShadows(0, 0, &bad, out) && out.empty());
}

// ---- e2. indirectDiffuse: this object's lights (the inputs `one`, `two`), point mode
void group_indirect(const std::string &scene) {
    const std::vector<Vec3f> P = in_v3("P"), N = in_v3("N"), one = in_v3("one"), two = in_v3("two");
    Flyscene fs;
    fs.setScenePath(scene);
    fs.initialize(48, 32, false, true);
    std::vector<Vec3f> out{{kSentinel, kSentinel, kSentinel}};
    for (int li = 0; li < 2; ++li) {
        fs.getLights() = li ? two : one;
        for (int m : {1, 3, 16})
            for (unsigned seed : {0u, 7u}) {
                EXPECT(fs.indirectDiffuse(P, N, m, seed, out) && out.size() == P.size());
                put_v3("rgb_" + std::to_string(li + 1) + "_" + std::to_string(m) + "_" + std::to_string(seed), out);
            }
    }
    EXPECT(!fs.indirectDiffuse(P, N, 0, 0, out));
    EXPECT(!fs.indirectDiffuse(P, N, 17, 0, out));
    std::vector<Vec3f> fewer(N);
    fewer.pop_back();
    EXPECT(!fs.indirectDiffuse(P, fewer, 3, 0, out));
    EXPECT(!fs.indirectDiffuse(fewer, N, 3, 0, out));
    const std::vector<Vec3f> none;
    out.assign(2, Vec3f{kSentinel, kSentinel, kSentinel});
    EXPECT(fs.indirectDiffuse(none, none, 3, 0, out) && out.empty());
    fs.initialize(48, 32, false, false);               // sphere lights: refused
    EXPECT(!fs.indirectDiffuse(P, N, 3, 0, out));
    Flyscene bare;                                     // never initialised: fails cleanly
    EXPECT(!bare.indirectDiffuse(P, N, 3, 0, out));
}

// ---- e3. lightProbes and probeIrradiance: this object's lights (the inputs `one`, `two`), point mode
void group_probes(const std::string &scene) {
    const std::vector<Vec3f> one = in_v3("one"), two = in_v3("two");
    Flyscene fs;
    fs.setScenePath(scene);
    fs.initialize(48, 32, false, true);
    const auto put_grid = [](const std::string &name, const rt_probe_grid &g) {
        put_f(name + "_origin", {g.origin[0], g.origin[1], g.origin[2]}, {3});
        put_f(name + "_step", {g.step[0], g.step[1], g.step[2]}, {3});
        put_f(name + "_dims", {static_cast<float>(g.dims[0]), static_cast<float>(g.dims[1]), static_cast<float>(g.dims[2])}, {3});
    };
    struct Case { const char *name; int dims[3]; int m; bool direct; float margin; int lights; };
    const Case cases[] = {{"a", {3, 2, 4}, 3, false, 0.25f, 1}, {"b", {2, 2, 2}, 8, true, 0.0f, 2}, {"c", {4, 1, 3}, 16, true, 0.5f, 2}, {"d", {1, 1, 1}, 1, false, 0.0f, 1}};
    rt_probe_grid grid{};
    std::vector<float> coeff{kSentinel};
    std::vector<Vec3f> img{{kSentinel, kSentinel, kSentinel}};
    for (const Case &c : cases) {
        fs.getLights() = c.lights == 2 ? two : one;
        EXPECT(fs.lightProbes(c.dims, c.m, c.direct, c.margin, grid, coeff) && coeff.size() == static_cast<size_t>(c.dims[0]) * c.dims[1] * c.dims[2] * RT_PROBE_COEFFS);
        put_grid(std::string("grid_") + c.name, grid);
        put_f(std::string("coeff_") + c.name, coeff, {static_cast<long>(coeff.size() / RT_PROBE_COEFFS), RT_PROBE_COEFFS});
        EXPECT(fs.probeIrradiance(0, 0, grid, coeff, img) && img.size() == 48u * 32u);
        put_v3(std::string("img_") + c.name, img);
        EXPECT(fs.probeIrradiance(40, 24, grid, coeff, img) && img.size() == 40u * 24u);
        put_v3(std::string("small_") + c.name, img);
    }
    // refusals: grid sizes, m, a coefficient array of another size, sphere lights, no scene
    const int ok[3] = {2, 2, 2}, zero[3] = {2, 0, 2}, huge[3] = {4096, 4096, 2};
    rt_probe_grid g2{};
    std::vector<float> c2;
    EXPECT(!fs.lightProbes(zero, 3, false, 0.0f, g2, c2) && c2.empty());
    EXPECT(!fs.lightProbes(huge, 3, false, 0.0f, g2, c2) && c2.empty());
    EXPECT(!fs.lightProbes(ok, 0, false, 0.0f, g2, c2) && c2.empty());
    EXPECT(!fs.lightProbes(ok, 17, false, 0.0f, g2, c2) && c2.empty());
    EXPECT(fs.lightProbes(ok, 2, false, 0.0f, g2, c2) && c2.size() == 8u * RT_PROBE_COEFFS);
    std::vector<float> fewer(c2);
    fewer.pop_back();
    EXPECT(!fs.probeIrradiance(0, 0, g2, fewer, img) && img.empty());
    rt_probe_grid bad = g2;
    bad.step[1] = 0.0f;
    EXPECT(!fs.probeIrradiance(0, 0, bad, c2, img) && img.empty());
    fs.initialize(48, 32, false, false);               // sphere lights: refused
    EXPECT(!fs.lightProbes(ok, 3, false, 0.0f, g2, c2) && c2.empty());
    Flyscene bare;                                     // never initialised: fails cleanly
    EXPECT(!bare.lightProbes(ok, 3, false, 0.0f, g2, c2));
    EXPECT(!bare.probeIrradiance(0, 0, grid, coeff, img));
}

// ---- e4. probeIrradianceVisible beside probeIrradiance: this object's lights (the input `one`), point mode
void group_probes_visible(const std::string &scene) {
    const std::vector<Vec3f> one = in_v3("one");
    Flyscene fs;
    fs.setScenePath(scene);
    fs.initialize(48, 32, false, true);
    fs.getLights() = one;
    struct Case { const char *name; int dims[3]; int m; float margin; };
    const Case cases[] = {{"a", {6, 5, 5}, 3, 0.0f}, {"b", {3, 1, 4}, 2, 0.25f}, {"c", {1, 1, 1}, 1, 0.0f}};
    rt_probe_grid grid{};
    std::vector<float> coeff{kSentinel};
    std::vector<Vec3f> img{{kSentinel, kSentinel, kSentinel}};
    for (const Case &c : cases) {
        EXPECT(fs.lightProbes(c.dims, c.m, true, c.margin, grid, coeff));
        put_f(std::string("coeff_") + c.name, coeff, {static_cast<long>(coeff.size() / RT_PROBE_COEFFS), RT_PROBE_COEFFS});
        EXPECT(fs.probeIrradianceVisible(0, 0, grid, coeff, img) && img.size() == 48u * 32u);
        put_v3(std::string("visible_") + c.name, img);
        EXPECT(fs.probeIrradiance(0, 0, grid, coeff, img) && img.size() == 48u * 32u);
        put_v3(std::string("plain_") + c.name, img);
        EXPECT(fs.probeIrradianceVisible(40, 24, grid, coeff, img) && img.size() == 40u * 24u);
        put_v3(std::string("small_") + c.name, img);
    }
    // refusals: a coefficient array of another size, a bad grid, no scene
    std::vector<float> fewer(coeff);
    fewer.pop_back();
    EXPECT(!fs.probeIrradianceVisible(0, 0, grid, fewer, img) && img.empty());
    rt_probe_grid bad = grid;
    bad.step[1] = 0.0f;
    EXPECT(!fs.probeIrradianceVisible(0, 0, bad, coeff, img) && img.empty());
    Flyscene bare;                                     // never initialised: fails cleanly
    EXPECT(!bare.probeIrradianceVisible(0, 0, grid, coeff, img));
}

// ---- e4b. lightProbesBounce and indirectDiffuseBounce: this object's lights (the input `one`), point mode; the gather at the points of
// the inputs `P`, `N`
void group_probes_bounce(const std::string &scene) {
    const std::vector<Vec3f> one = in_v3("one"), P = in_v3("P"), N = in_v3("N");
    Flyscene fs;
    fs.setScenePath(scene);
    fs.initialize(48, 32, false, true);
    fs.getLights() = one;
    struct Case { const char *name; int dims[3]; int m; bool direct; float margin; int bounces; bool visible; };
    const Case cases[] = {{"a", {4, 3, 3}, 3, false, 0.0f, 2, true}, {"b", {4, 3, 3}, 3, true, 0.0f, 2, false}, {"c", {3, 1, 4}, 2, true, 0.25f, 1, true},
                          {"d", {4, 3, 3}, 3, true, 0.0f, 0, true}};
    rt_probe_grid grid{};
    std::vector<float> coeff{kSentinel};
    std::vector<Vec3f> rgb{{kSentinel, kSentinel, kSentinel}};
    for (const Case &c : cases) {
        EXPECT(fs.lightProbesBounce(c.dims, c.m, c.direct, c.margin, c.bounces, c.visible, grid, coeff));
        put_f(std::string("coeff_") + c.name, coeff, {static_cast<long>(coeff.size() / RT_PROBE_COEFFS), RT_PROBE_COEFFS});
        if (!c.direct) {                                // the final gather takes a volume without the direct term
            for (int visible = 0; visible < 2; ++visible) {
                EXPECT(fs.indirectDiffuseBounce(P, N, 3, 7u, grid, coeff, visible != 0, rgb) && rgb.size() == P.size());
                put_v3(std::string("rgb_") + c.name + "_" + std::to_string(visible), rgb);
            }
        }
    }
    // bounces == 0 is lightProbes
    std::vector<float> parent;
    rt_probe_grid pgrid{};
    EXPECT(fs.lightProbes(cases[3].dims, cases[3].m, true, 0.0f, pgrid, parent) && parent == coeff);
    // refusals: bounces below 0, a coefficient array of another size, a bad grid, sizes that differ, m out of range, no scene
    std::vector<float> out2;
    EXPECT(!fs.lightProbesBounce(cases[0].dims, 3, false, 0.0f, -1, true, pgrid, out2) && out2.empty());
    EXPECT(!fs.lightProbesBounce(cases[0].dims, 17, false, 0.0f, 1, true, pgrid, out2) && out2.empty());
    std::vector<float> fewer(coeff);
    fewer.pop_back();
    EXPECT(!fs.indirectDiffuseBounce(P, N, 3, 0, grid, fewer, true, rgb) && rgb.empty());
    rt_probe_grid bad = grid;
    bad.step[1] = 0.0f;
    EXPECT(!fs.indirectDiffuseBounce(P, N, 3, 0, bad, coeff, true, rgb) && rgb.empty());
    EXPECT(!fs.indirectDiffuseBounce(P, N, 0, 0, grid, coeff, true, rgb));
    std::vector<Vec3f> shorter(N);
    shorter.pop_back();
    EXPECT(!fs.indirectDiffuseBounce(P, shorter, 3, 0, grid, coeff, true, rgb));
    Flyscene bare;                                     // never initialised: fails cleanly
    EXPECT(!bare.lightProbesBounce(cases[0].dims, 3, false, 0.0f, 1, true, pgrid, out2));
    EXPECT(!bare.indirectDiffuseBounce(P, N, 3, 0, grid, coeff, true, rgb));
}

// ---- e5. closestPoints: the points of the input `P`, unbounded and within the radii of the input `radii`
void group_closest_points(const std::string &scene) {
    const std::vector<Vec3f> P = in_v3("P");
    const std::vector<float> radii = in_vec<float>("radii");
    Flyscene fs;
    fs.setScenePath(scene);
    fs.initialize(48, 32, true, false);
    std::vector<int> faces{7};
    std::vector<float> dist2{kSentinel};
    std::vector<Vec3f> closest{{kSentinel, kSentinel, kSentinel}};
    for (size_t k = 0; k < radii.size(); ++k) {
        EXPECT(fs.closestPoints(P, radii[k], faces, dist2, closest) && faces.size() == P.size() && dist2.size() == P.size() && closest.size() == P.size());
        put("faces_" + std::to_string(k), "i4", {static_cast<long>(faces.size())}, faces.data());
        put_f("dist2_" + std::to_string(k), dist2, {static_cast<long>(dist2.size())});
        put_v3("closest_" + std::to_string(k), closest);
    }
    // refusals: a NaN and a negative radius, no scene; no points: empty outputs
    EXPECT(!fs.closestPoints(P, std::nanf(""), faces, dist2, closest));
    EXPECT(!fs.closestPoints(P, -1.0f, faces, dist2, closest));
    const std::vector<Vec3f> none;
    EXPECT(fs.closestPoints(none, 1.0f, faces, dist2, closest) && faces.empty() && dist2.empty() && closest.empty());
    Flyscene bare;                                     // never initialised: fails cleanly
    EXPECT(!bare.closestPoints(P, 1.0f, faces, dist2, closest));
}

// ---- e6. rayHits: the rays of the inputs `O`, `D`, for every k of the input `ks`, unbounded and within the input `t_max`
void group_ray_hits(const std::string &scene) {
    const std::vector<Vec3f> O = in_v3("O"), D = in_v3("D");
    const std::vector<int> ks = in_vec<int>("ks");
    const std::vector<float> t_max = in_vec<float>("t_max");
    Flyscene fs;
    fs.setScenePath(scene);
    fs.initialize(48, 32, true, false);
    std::vector<int> faces{7}, counts{7};
    std::vector<float> ts{kSentinel};
    for (size_t i = 0; i < ks.size(); ++i) {
        for (size_t j = 0; j < t_max.size(); ++j) {
            const size_t slots = O.size() * static_cast<size_t>(ks[i]);
            EXPECT(fs.rayHits(O, D, ks[i], t_max[j], faces, ts, counts) && faces.size() == slots && ts.size() == slots && counts.size() == O.size());
            const std::string tag = std::to_string(ks[i]) + "_" + std::to_string(j);
            put("faces_" + tag, "i4", {static_cast<long>(O.size()), static_cast<long>(ks[i])}, faces.data());
            put_f("ts_" + tag, ts, {static_cast<long>(O.size()), static_cast<long>(ks[i])});
            put("counts_" + tag, "i4", {static_cast<long>(counts.size())}, counts.data());
        }
    }
    // refusals: k outside 1 .. 8, a NaN, zero and negative t_max, arrays of different lengths, no scene; no rays: empty outputs
    EXPECT(!fs.rayHits(O, D, 0, 1.0f, faces, ts, counts));
    EXPECT(!fs.rayHits(O, D, 9, 1.0f, faces, ts, counts));
    EXPECT(!fs.rayHits(O, D, 8, std::nanf(""), faces, ts, counts));
    EXPECT(!fs.rayHits(O, D, 8, 0.0f, faces, ts, counts));
    EXPECT(!fs.rayHits(O, D, 8, -1.0f, faces, ts, counts));
    const std::vector<Vec3f> none, one(1);
    EXPECT(!fs.rayHits(O, one, 8, 1.0f, faces, ts, counts));
    EXPECT(fs.rayHits(none, none, 8, 1.0f, faces, ts, counts) && faces.empty() && ts.empty() && counts.empty());
    Flyscene bare;                                     // never initialised: fails cleanly
    EXPECT(!bare.rayHits(O, D, 8, 1.0f, faces, ts, counts));
}

// ---- f, g. createSpherePoint and addLight
void group_lights(const std::string &scene) {
    const std::vector<Vec3f> p = in_v3("p");
    Flyscene fs;
    fs.setScenePath(scene);
    fs.setOutputPath(g_ppm);
    for (int k = 0; k < 3; ++k) {
        fs.initialize(16, 12, kArea[k], kPoint[k]);
        sample_grids(fs, kModes[k], p[0]);
    }
    fs.initialize(16, 12, true, false);
    fs.setAreaGrid(5, 5);
    fs.setMaxDepth(3);
    for (int i = 0; i < 30; ++i) fs.addLight();
    EXPECT(fs.getLights().size() == RT_MAX_LIGHTS);
    put_v3("lights", fs.getLights());
    frame(fs, "frame", 16, 12);
}

// ---- h. sizes and state: one process per variant (the input `shutter` is 0 or 1)
void group_state(const std::string &scene) {
    const bool shutter = in_vec<float>("shutter")[0] != 0.0f;
    const std::string v = shutter ? "shutter_" : "plain_";
    Flyscene fs;
    fs.setScenePath(scene);
    fs.setOutputPath(g_ppm);
    fs.initialize(48, 32, true, false);
    fs.setMaxDepth(3);
    if (shutter) {
        rt_camera close;
        rt_yaw_camera(&close, 48, 32, 0.05f);
        fs.setShutter(&close);
        fs.setSupersampling(2);
    }
    frame(fs, v + "0", 48, 32);
    put_stats(v + "stats0", fs.lastStats());
    frame(fs, v + "1", 40, 24, 40, 24);
    frame(fs, v + "2", 48, 32);
    buffers(fs, v + "3", 40, 24, 40, 24);
    buffers(fs, v + "4", 48, 32);
    frame(fs, v + "5", 48, 32);
}

// ---- i. the stand-alone denoise, upsample and reproject
void group_post(const std::string &scene) {
    Flyscene fs;
    fs.setScenePath(scene);
    fs.initialize(48, 32, true, false);
    const Arr &g0 = in("dn_g");
    const int h = static_cast<int>(g0.shape[0]), w = static_cast<int>(g0.shape[1]);
    const std::vector<float> tight = in_vec<float>("tight");       // sigma normal, depth, albedo
    rt_denoise_params dd, dt;
    rt_default_denoise_params(&dd);
    dt = dd; dt.iterations = 2; dt.sigma_normal = tight[0]; dt.sigma_depth = tight[1]; dt.sigma_albedo = tight[2];
    rt_upsample_params ud, u3, u3t;
    rt_default_upsample_params(&ud);
    u3 = ud; u3.factor = 3;
    u3t = u3; u3t.sigma_normal = tight[0]; u3t.sigma_depth = tight[1]; u3t.sigma_albedo = tight[2];
    rt_reproject_params rd, rt;
    rt_default_reproject_params(&rd);
    rt = rd; rt.max_history = 4; rt.sigma_normal = tight[0]; rt.sigma_depth = tight[1]; rt.sigma_albedo = tight[2];
    const std::vector<float> m = in_vec<float>("rp_m");
    for (int ch : {1, 3}) {
        const std::string c = std::to_string(ch);
        const std::vector<long> shape = ch == 3 ? std::vector<long>{h, w, 3} : std::vector<long>{h, w};
        std::vector<float> out;
        std::vector<uint8_t> miss, len;
        const std::vector<float> img = in_vec<float>("dn_img" + c), g = in_vec<float>("dn_g");
        const struct { const char *name; const rt_denoise_params *p; } dn[3] = {{"null", nullptr}, {"def", &dd}, {"tight", &dt}};
        for (const auto &q : dn) {
            EXPECT(fs.denoise(img, ch, g, w, h, q.p, out));
            put_f("dn_" + c + "_" + q.name, out, shape);
        }
        const struct { const char *name; int s; const rt_upsample_params *p; } up[4] = {{"null", ud.factor, nullptr}, {"def", ud.factor, &ud}, {"three", 3, &u3}, {"tight", 3, &u3t}};
        for (const auto &q : up) {
            const std::string s = std::to_string(q.s);
            const std::vector<float> low = in_vec<float>("up" + s + "_low" + c), gl = in_vec<float>("up" + s + "_gl"), gh = in_vec<float>("up" + s + "_gh");
            EXPECT(fs.upsample(low, ch, gl, gh, w, h, q.p, out));
            put_f("up_" + c + "_" + q.name, out, shape);
            EXPECT(fs.upsample(low, ch, gl, gh, w, h, q.p, out, &miss));
            put_f("upm_" + c + "_" + q.name, out, shape);
            put_u8("miss_" + c + "_" + q.name, miss, {h, w});
        }
        const std::vector<float> cur = in_vec<float>("rp_cur" + c), gc = in_vec<float>("rp_gc"), hist = in_vec<float>("rp_hist" + c), gh = in_vec<float>("rp_gh");
        const std::vector<uint8_t> lens = in_vec<uint8_t>("rp_len");
        const struct { const char *name; const rt_reproject_params *p; } rp[3] = {{"null", nullptr}, {"def", &rd}, {"tight", &rt}};
        for (const auto &q : rp) {
            EXPECT(fs.reproject(cur, ch, gc, hist, gh, lens, w, h, m.data(), q.p, out, len));
            put_f("rp_" + c + "_" + q.name, out, shape);
            put_u8("rplen_" + c + "_" + q.name, len, {h, w});
        }
    }
    shape_refusals(fs, true);
    // parameters out of range
    std::vector<float> out;
    rt_denoise_params bad = dd;
    bad.iterations = 0;
    EXPECT(!fs.denoise(in_vec<float>("dn_img1"), 1, in_vec<float>("dn_g"), w, h, &bad, out));
}

void temporal_settings(Flyscene &fs, const rt_reproject_params *rp) {
    fs.setAreaGrid(2, 2);
    fs.setMaxDepth(1);
    fs.setPasses(2);
    fs.setTemporal(rp);
}

void put_lengths(Flyscene &fs, const std::string &name, int w, int h) {
    EXPECT(fs.historyLengths().size() == static_cast<size_t>(w) * h);
    put_u8(name, fs.historyLengths(), {static_cast<long>(fs.historyLengths().size())});
}

// ---- j. the temporal lifecycle
void group_temporal(const std::string &scene) {
    const std::string other = in_str("scene2");
    const std::vector<float> yaws = in_vec<float>("yaws");
    rt_reproject_params rp;
    rt_default_reproject_params(&rp);
    rp.sigma_depth = in_vec<float>("sigma_depth")[0];
    {
        Flyscene fs;
        fs.setScenePath(scene);
        fs.setOutputPath(g_ppm);
        fs.initialize(48, 32, true, false);
        temporal_settings(fs, &rp);
        EXPECT(fs.historyLengths().empty());
        for (size_t k = 0; k < yaws.size(); ++k) {
            yaw_camera(fs, 48, 32, yaws[k]);
            frame(fs, "path" + std::to_string(k), 48, 32);
            put_lengths(fs, "pathlen" + std::to_string(k), 48, 32);
        }
        fs.resetHistory();
        EXPECT(fs.historyLengths().empty());
        frame(fs, "reset", 48, 32);
        put_lengths(fs, "resetlen", 48, 32);
        fs.setTemporal(nullptr);
        frame(fs, "reset_plain", 48, 32);
        fs.setTemporal(&rp);
        frame(fs, "second", 48, 32);                       // the history of `reset` is still there: lengths of 2
        put_lengths(fs, "secondlen", 48, 32);
        frame(fs, "small", 40, 24, 40, 24);                // another size drops it
        put_lengths(fs, "smalllen", 40, 24);
        frame(fs, "again0", 48, 32);
        put_lengths(fs, "again0len", 48, 32);
        frame(fs, "again1", 48, 32);
        put_lengths(fs, "again1len", 48, 32);
        fs.setScenePath(other);                            // a scene change: the first frame after it is itself
        fs.initialize(48, 32, true, false);
        frame(fs, "changed", 48, 32);
        put_lengths(fs, "changedlen", 48, 32);
        // temporal reuse together with upsampling: refused, nothing written
        rt_upsample_params up;
        rt_default_upsample_params(&up);
        fs.setUpsample(&up);
        const std::string refused = g_ppm + ".refused";
        std::remove(refused.c_str());
        fs.setOutputPath(refused);
        fs.raytraceScene();
        EXPECT(fs.lastStatus() == RT_ERR_INVALID);
        EXPECT(!exists(refused));
        put_flag("refused_written", exists(refused));
        const int32_t status = fs.lastStatus();
        put("refused_status", "i4", {1}, &status);
    }
    Flyscene fresh;
    fresh.setScenePath(other);
    fresh.setOutputPath(g_ppm);
    fresh.initialize(48, 32, true, false);
    temporal_settings(fresh, &rp);
    frame(fresh, "fresh", 48, 32);
    put_lengths(fresh, "freshlen", 48, 32);
}

std::unique_ptr<Flyscene> object_on(const std::string &scene) {
    std::unique_ptr<Flyscene> fs(new Flyscene);
    fs->setScenePath(scene);
    fs->setOutputPath(g_ppm);
    fs->initialize(48, 32, true, false);
    fs->setMaxDepth(3);
    return fs;
}

void yaw_frame(Flyscene &fs, const std::string &name, float yaw) {
    yaw_camera(fs, 48, 32, yaw);
    frame(fs, name, 48, 32);
}

// ---- k. objects
void group_objects(const std::string &scene) {
    const std::string dodge = in_str("scene2"), mixed = in_str("scene3");
    const float yaw = in_vec<float>("yaw")[0];
    {
        std::unique_ptr<Flyscene> a = object_on(scene);
        yaw_frame(*a, "alone_a0", 0.0f);
        yaw_frame(*a, "alone_a1", yaw);
    }
    {
        std::unique_ptr<Flyscene> b = object_on(dodge);
        yaw_frame(*b, "alone_b0", 0.0f);
        yaw_frame(*b, "alone_b1", yaw);
    }
    {
        std::unique_ptr<Flyscene> a = object_on(scene), b = object_on(dodge);
        yaw_frame(*a, "both_a0", 0.0f);
        yaw_frame(*b, "both_b0", 0.0f);
        yaw_frame(*a, "both_a1", yaw);
        yaw_frame(*b, "both_b1", yaw);
        a.reset();
        yaw_frame(*b, "after_b0", 0.0f);
    }
    {
        std::unique_ptr<Flyscene> c = object_on(scene);
        yaw_frame(*c, "twice_cube", 0.0f);
        c->setScenePath(mixed);
        c->initialize(48, 32, true, false);
        yaw_frame(*c, "twice_mixed", 0.0f);
        std::unique_ptr<Flyscene> d = object_on(mixed);
        yaw_frame(*d, "fresh_mixed", 0.0f);
    }
    // the reference's prompts: "1 0" area, "0 1" point, "0 0" spherical, read from stdin in this order
    const std::vector<Vec3f> p = in_v3("p");
    Flyscene e;
    e.setScenePath(scene);
    e.setOutputPath(g_ppm);
    e.setMaxDepth(3);
    for (int k = 0; k < 3; ++k) {
        e.initialize(16, 12);
        put_v3(std::string("stdin_csp_") + kModes[k], e.createSpherePoint(p[0]));
        frame(e, std::string("stdin_frame_") + kModes[k], 16, 12);
    }
}

}  // namespace

int main(int argc, char **argv) {
    bool host = false;
    int at = 1;
    if (argc > 1 && std::strcmp(argv[1], "--host") == 0) { host = true; at = 2; }
    if (argc - at != 4) {
        std::fprintf(stderr, "usage: flyscene_check [--host] GROUP SCENE.obj INPUT OUTPUT\n");
        return 2;
    }
    const std::string group = argv[at], scene = argv[at + 1];
    if (!read_arrays(argv[at + 2])) { std::fprintf(stderr, "flyscene_check: cannot read %s\n", argv[at + 2]); return 2; }
    g_out.open(argv[at + 3], std::ios::binary);
    if (!g_out) { std::fprintf(stderr, "flyscene_check: cannot write %s\n", argv[at + 3]); return 2; }
    g_ppm = std::string(argv[at + 3]) + ".ppm";
    if (host != (group == "host")) { std::fprintf(stderr, "flyscene_check: --host runs the group host, and nothing else does\n"); return 2; }
    if (group == "host") group_host();
    else if (group == "trace") group_trace(scene);
    else if (group == "strikes") group_strikes(scene);
    else if (group == "hits") group_hits(scene);
    else if (group == "ao") group_ao(scene);
    else if (group == "shadow") group_shadow(scene);
    else if (group == "indirect") group_indirect(scene);
    else if (group == "probes") group_probes(scene);
    else if (group == "probes_visible") group_probes_visible(scene);
    else if (group == "probes_bounce") group_probes_bounce(scene);
    else if (group == "closest_points") group_closest_points(scene);
    else if (group == "ray_hits") group_ray_hits(scene);
    else if (group == "lights") group_lights(scene);
    else if (group == "state") group_state(scene);
    else if (group == "post") group_post(scene);
    else if (group == "temporal") group_temporal(scene);
    else if (group == "objects") group_objects(scene);
    else { std::fprintf(stderr, "flyscene_check: no group %s\n", group.c_str()); return 2; }
    g_out.close();
    if (!g_out) { std::fprintf(stderr, "flyscene_check: writing %s failed\n", argv[at + 3]); return 2; }
    if (g_fail) std::fprintf(stderr, "flyscene_check: %d expectation(s) failed in group %s\n", g_fail, group.c_str());
    return g_fail ? 1 : 0;
}
