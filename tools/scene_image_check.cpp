// Stand-alone host check of rt_scene_image.cpp (the validation of an rt_scene view and the image of what goes to the device),
// meant for a sanitizer build on the CPU:
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iraytracer-in-cpp_amd/csrc -Iinclude
//       tools/scene_image_check.cpp raytracer-in-cpp_amd/csrc/rt_scene_image.cpp raytracer-in-cpp_amd/csrc/host_scene.cpp -o scene_image_check
// (make -C raytracer-in-cpp_amd/csrc scene_check builds and runs it).  Argument: the directory of cube.obj, toy.obj and dodgeColorTest.obj.
// It prints one FNV-1a 64-bit value per image array and scene (tests/golden/scene_image.json holds them).  Exit status 0: every check held.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_scene.hpp"
#include "rt_scene_image.hpp"

using namespace rtamd;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

template <typename T>
static unsigned long long fnv1a(const std::vector<T> &a) {
    unsigned long long h = 0xcbf29ce484222325ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(a.data());
    for (size_t i = 0; i < a.size() * sizeof(T); ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

static bool same_bits(const void *a, const void *b, size_t n) { return std::memcmp(a, b, n) == 0; }
static bool far_away(const DNode &n) { return n.clo[0] >= 1e30f; }

// the record of face f, from the arrays of the view
static TriRec record_of(const rt_scene &sc, uint32_t f) {
    const float *v = sc.tri_verts + static_cast<size_t>(f) * 9, *n = sc.face_normal + static_cast<size_t>(f) * 3;
    const V3 A{v[0], v[1], v[2]}, B{v[3], v[4], v[5]}, C{v[6], v[7], v[8]}, N{n[0], n[1], n[2]};
    const V3 e0 = C - A, e1 = B - A;
    TriRec r{};
    r.ax = A.x; r.ay = A.y; r.az = A.z; r.e0x = e0.x; r.e0y = e0.y; r.e0z = e0.z; r.e1x = e1.x; r.e1y = e1.y; r.e1z = e1.z;
    r.nx = N.x; r.ny = N.y; r.nz = N.z;
    r.nA = dot(N, A);
    r.d00 = dot(e0, e0); r.d01 = dot(e0, e1); r.d11 = dot(e1, e1);
    r.inv_denom = 1 / (r.d00 * r.d11 - r.d01 * r.d01);
    r.face = f;
    double edge, infl;
    r.flags = (sc.materials[sc.mat_id[f]].illum == 9 ? 1u : 0u) | ((!never_hit(v, n) && tri_ill_conditioned(v, n, edge, infl)) ? 2u : 0u);
    return r;
}

// TriRec::flags bit 1 by another road than tri_ill_conditioned's: kappa = d00 d11 / (d00 d11 - d01^2) is 1 / sin^2 of the angle between the
// two edges at A, here from the cross product in long double.  1: the angle is so small that the bit must be set (kappa > 1.1e4), 0: so
// wide that it must be clear (kappa < 0.9e4), -1: no verdict -- the band around 1e4, or a triangle another rule decides (non-finite,
// normal not unit, never hittable).
static long sliver_verdicts[2] = {0, 0};      // records checked against a verdict 0 / 1 (main: the scenes must bring both)
static int sliver_verdict(const float *v, const float *n) {
    for (int k = 0; k < 9; ++k) if (!std::isfinite(v[k])) return -1;
    const long double nl = std::sqrt(static_cast<long double>(n[0]) * n[0] + static_cast<long double>(n[1]) * n[1] + static_cast<long double>(n[2]) * n[2]);
    if (!(std::fabs(nl - 1.0L) < 0.5e-3L) || never_hit(v, n)) return -1;
    long double p[3], q[3];
    for (int k = 0; k < 3; ++k) { p[k] = static_cast<long double>(v[6 + k]) - v[k]; q[k] = static_cast<long double>(v[3 + k]) - v[k]; }
    const long double x[3] = {p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]};
    const long double sin2 = (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) / ((p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) * (q[0] * q[0] + q[1] * q[1] + q[2] * q[2]));
    if (!(sin2 == sin2)) return -1;
    return sin2 < 1.0L / 1.1e4L ? 1 : (sin2 > 1.0L / 0.9e4L ? 0 : -1);
}

// what node i's content box and open mark must be, top-down from the chunks (the image builds them bottom-up in one pass)
struct Content {
    float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {1e30f, 1e30f, 1e30f};
    bool any = false, open = false;
    void grow(const float *l, const float *h) {
        for (int k = 0; k < 3; ++k) { lo[k] = any ? std::fmin(lo[k], l[k]) : l[k]; hi[k] = any ? std::fmax(hi[k], h[k]) : h[k]; }
        any = true;
    }
};
static Content content_of(const rt_scene &sc, const SceneImage &img, uint32_t i, std::vector<uint32_t> *bad) {
    const rt_node &n = sc.nodes[i];
    const uint32_t cnt = n.count_flags & 0x7fffffffu;
    Content c;
    if (n.count_flags & RT_NODE_LEAF) {
        for (uint32_t k = 0; k < (cnt + 63u) / 64u; ++k) {
            const ChunkBound &cb = img.chunks[img.leaf_chunk0[i] + k];
            if (cb.never >= 1.5f) c.open = true; else c.grow(cb.lo, cb.hi);
        }
        if (c.open) bad->push_back(i);
    } else {
        for (uint32_t k = 0; k < cnt; ++k) {
            const Content ch = content_of(sc, img, n.first + k, bad);
            const DNode &dch = img.nodes[n.first + k];
            if (ch.open) c.open = true;
            if (!far_away(dch)) {
                c.grow(ch.lo, ch.hi);
                const DNode &dn = img.nodes[i];
                CHECK(!far_away(dn));
                for (int a = 0; a < 3; ++a) CHECK(dn.clo[a] <= dch.clo[a] && dn.chi[a] >= dch.chi[a]);
            }
        }
    }
    bool finite = true;
    for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(c.lo[k]) && std::isfinite(c.hi[k]);
    if (!finite) { c.open = true; for (int k = 0; k < 3; ++k) c.lo[k] = c.hi[k] = 1e30f; }
    const DNode &dn = img.nodes[i];
    CHECK(same_bits(dn.clo, c.lo, sizeof c.lo) && same_bits(dn.chi, c.hi, sizeof c.hi));
    CHECK(dn.pad[1] == (c.open ? 1u : 0u));
    CHECK(dn.pad[0] == ((n.count_flags & RT_NODE_LEAF) ? img.leaf_chunk0[i] : 0u));
    CHECK(same_bits(&dn, &n, sizeof(rt_node)));
    return c;
}

static void check_image(const rt_scene &sc, const SceneImage &img, bool no_cull) {
    CHECK(img.nodes.size() == sc.n_nodes && img.leaf_chunk0.size() == sc.n_nodes);
    CHECK(img.refs.size() == sc.n_face_refs && img.leaf_tris.size() == sc.n_face_refs);
    if (img.nodes.size() != sc.n_nodes || img.leaf_chunk0.size() != sc.n_nodes || img.refs.size() != sc.n_face_refs || img.leaf_tris.size() != sc.n_face_refs) return;
    // refs: a permutation of face_refs inside every leaf range; the chunks follow the leaves in node order
    size_t chunks = 0;
    for (uint32_t i = 0; i < sc.n_nodes; ++i) {
        const rt_node &n = sc.nodes[i];
        if (!(n.count_flags & RT_NODE_LEAF)) continue;
        const uint32_t cnt = n.count_flags & 0x7fffffffu;
        CHECK(img.leaf_chunk0[i] == chunks);
        chunks += (cnt + 63u) / 64u;
        std::vector<uint32_t> a(sc.face_refs + n.first, sc.face_refs + n.first + cnt), b(img.refs.begin() + n.first, img.refs.begin() + n.first + cnt);
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        CHECK(a == b);
    }
    CHECK(img.chunks.size() == (chunks ? chunks : 1));
    if (img.chunks.size() != (chunks ? chunks : 1)) return;
    // the triangle records: field by field, as bits
    for (uint32_t i = 0; i < sc.n_face_refs; ++i) {
        const TriRec want = record_of(sc, img.refs[i]), &got = img.leaf_tris[i];
        const float *w = &want.ax, *g = &got.ax;
        for (int k = 0; k < 17; ++k) CHECK(same_bits(w + k, g + k, sizeof(float)));
        CHECK(want.face == got.face && want.flags == got.flags && got.pad == 0u);
        const int sliver = sliver_verdict(sc.tri_verts + static_cast<size_t>(got.face) * 9, sc.face_normal + static_cast<size_t>(got.face) * 3);
        if (sliver >= 0) { CHECK(((got.flags >> 1) & 1u) == static_cast<uint32_t>(sliver)); ++sliver_verdicts[sliver]; }
    }
    // content boxes, open marks, first chunks; the bad-leaf list
    std::vector<uint32_t> bad;
    content_of(sc, img, 0, &bad);
    std::sort(bad.begin(), bad.end(), [](uint32_t a, uint32_t b) { return a > b; });      // the order of the bottom-up pass: last node first
    CHECK(img.n_bad_leaves == (bad.size() <= 32 ? bad.size() : 0xffffffffu));
    CHECK(img.bad_leaves.size() == (bad.empty() ? 6 : bad.size() * 6));
    if (img.bad_leaves.size() == bad.size() * 6)
        for (size_t b = 0; b < bad.size(); ++b)
            CHECK(same_bits(&img.bad_leaves[6 * b], sc.nodes[bad[b]].bmin, 12) && same_bits(&img.bad_leaves[6 * b + 3], sc.nodes[bad[b]].bmax, 12));
    if (bad.empty()) for (const float z : img.bad_leaves) CHECK(z == 0.0f);
    // the scalars
    float extent = 0.f;
    for (size_t i = 0; i < static_cast<size_t>(sc.n_faces) * 9; ++i) extent = std::fmax(extent, std::fabs(sc.tri_verts[i]));
    CHECK(same_bits(&extent, &img.extent, sizeof extent));
    bool reflective = false;
    for (uint32_t m = 0; m < sc.n_materials; ++m) { const int il = sc.materials[m].illum; reflective = reflective || il == 3 || il == 4 || il == 5 || il == 6 || il == 9; }
    CHECK(img.reflective == reflective);
    CHECK(img.flat == (sc.nodes[0].count_flags >= RT_NODE_LEAF && sc.nodes[0].count_flags - RT_NODE_LEAF <= 64u));
    CHECK(same_bits(img.root_box, sc.nodes[0].bmin, 12) && same_bits(img.root_box + 3, sc.nodes[0].bmax, 12));
    CHECK(img.trace_target == std::min(4000u, std::max(1000u, sc.n_face_refs / 256u)));
    if (no_cull) {
        for (const ChunkBound &cb : img.chunks) CHECK(cb.never >= 1.5f && cb.infl == 0.0f);
        for (uint32_t i = 0; i < sc.n_nodes; ++i) {
            const bool leaf_with_faces = (sc.nodes[i].count_flags & RT_NODE_LEAF) && (sc.nodes[i].count_flags & 0x7fffffffu);
            if (leaf_with_faces) CHECK(img.nodes[i].pad[1] == 1u);
            CHECK(far_away(img.nodes[i]));
        }
        if (sc.n_face_refs) CHECK(img.nodes[0].pad[1] == 1u);
    }
}

static void refused(const rt_scene &sc, rt_status status, const char *message) {
    const SceneVerdict v = validate_scene(&sc);
    if (v.status != status || !v.message || std::strcmp(v.message, message) != 0) {
        std::printf("FAILED rule \"%s\": got status %d, \"%s\"\n", message, static_cast<int>(v.status), v.message ? v.message : "(none)");
        ++failures;
    }
}

// every rule of validate_scene: each broken view is the valid view `ok` with one field changed
static void check_rules(const rt_scene &ok, const rt_scene &one_node) {
    CHECK(validate_scene(&ok).status == RT_OK && validate_scene(&ok).message == nullptr);
    CHECK(validate_scene(nullptr).status == RT_ERR_INVALID);
    rt_scene s = ok;
    s.n_nodes = 0; refused(s, RT_ERR_INVALID, "rt_upload_scene: empty scene");
    s = ok; s.nodes = nullptr; refused(s, RT_ERR_INVALID, "rt_upload_scene: empty scene");
    s = ok; s.n_materials = 0; refused(s, RT_ERR_INVALID, "rt_upload_scene: empty scene");
    s = ok; s.materials = nullptr; refused(s, RT_ERR_INVALID, "rt_upload_scene: empty scene");
    s = ok; s.tri_verts = nullptr; refused(s, RT_ERR_INVALID, "rt_upload_scene: missing arrays");
    s = ok; s.face_normal = nullptr; refused(s, RT_ERR_INVALID, "rt_upload_scene: missing arrays");
    s = ok; s.tri_vid = nullptr; refused(s, RT_ERR_INVALID, "rt_upload_scene: missing arrays");
    s = ok; s.mat_id = nullptr; refused(s, RT_ERR_INVALID, "rt_upload_scene: missing arrays");
    s = ok; s.vert_normal = nullptr; refused(s, RT_ERR_INVALID, "rt_upload_scene: missing arrays");
    // more than 2^28 nodes: refused before the one-node array behind the claim is read (the sanitizer is the witness)
    s = one_node; CHECK(s.n_nodes == 1);
    s.n_nodes = 1u << 28; refused(s, RT_ERR_UNSUPPORTED, "rt_upload_scene: more than 2^28 nodes");

    uint32_t leaf = 0, inner = 0;
    bool have_leaf = false, have_inner = false;
    for (uint32_t i = 0; i < ok.n_nodes; ++i) {
        const uint32_t cf = ok.nodes[i].count_flags;
        if ((cf & RT_NODE_LEAF) && (cf & 0x7fffffffu) && !have_leaf) { leaf = i; have_leaf = true; }
        if (!(cf & RT_NODE_LEAF) && (cf & 0x7fffffffu) && !have_inner) { inner = i; have_inner = true; }
    }
    CHECK(have_leaf && have_inner);
    if (!have_leaf || !have_inner) return;
    std::vector<rt_node> nodes(ok.nodes, ok.nodes + ok.n_nodes);
    s = ok; s.nodes = nodes.data();
    nodes[leaf].first = ok.n_face_refs; refused(s, RT_ERR_INVALID, "rt_upload_scene: leaf range outside face_refs");
    nodes[leaf] = ok.nodes[leaf];
    nodes[leaf].count_flags = RT_NODE_LEAF | (ok.n_face_refs + 1u); refused(s, RT_ERR_INVALID, "rt_upload_scene: leaf range outside face_refs");
    nodes[leaf] = ok.nodes[leaf];
    nodes[inner].first = inner; refused(s, RT_ERR_INVALID, "rt_upload_scene: bad child range");
    nodes[inner].first = ok.n_nodes; refused(s, RT_ERR_INVALID, "rt_upload_scene: bad child range");
    nodes[inner] = ok.nodes[inner];
    nodes[inner].count_flags = 9u; refused(s, RT_ERR_INVALID, "rt_upload_scene: bad child range");
    nodes[inner] = ok.nodes[inner];
    CHECK(validate_scene(&s).status == RT_OK);

    std::vector<uint32_t> refs(ok.face_refs, ok.face_refs + ok.n_face_refs);
    s = ok; s.face_refs = refs.data();
    refs.back() = ok.n_faces; refused(s, RT_ERR_INVALID, "rt_upload_scene: face ref out of range");
    std::vector<int32_t> mat(ok.mat_id, ok.mat_id + ok.n_faces);
    s = ok; s.mat_id = mat.data();
    mat.back() = static_cast<int32_t>(ok.n_materials); refused(s, RT_ERR_INVALID, "rt_upload_scene: material id out of range");
    mat.back() = -1; refused(s, RT_ERR_INVALID, "rt_upload_scene: material id out of range");
    std::vector<uint32_t> vid(ok.tri_vid, ok.tri_vid + static_cast<size_t>(ok.n_faces) * 3);
    s = ok; s.tri_vid = vid.data();
    vid.back() = ok.n_vert_normals; refused(s, RT_ERR_INVALID, "rt_upload_scene: vertex id outside vert_normal");

    // depth: a chain of 18 nodes, node i the only child of node i - 1, cut below node 16 (an inner node without children): 16 levels, valid.
    // Giving node 16 its child makes 17.
    std::vector<rt_node> chain(18, ok.nodes[0]);
    for (uint32_t i = 0; i < 18; ++i) { chain[i].first = i + 1; chain[i].count_flags = i < 16 ? 1u : 0u; }
    chain[17].first = 0; chain[17].count_flags = RT_NODE_LEAF;
    s = ok; s.nodes = chain.data(); s.n_nodes = 18;
    CHECK(validate_scene(&s).status == RT_OK);
    chain[16].count_flags = 1u; refused(s, RT_ERR_UNSUPPORTED, "rt_upload_scene: octree deeper than 16 levels (traversal stack bound)");
}

int main(int argc, char **argv) {
    if (argc != 2) { std::printf("usage: scene_image_check <directory of cube.obj, toy.obj, dodgeColorTest.obj>\n"); return 2; }
    const char *names[3] = {"cube.obj", "toy.obj", "dodgeColorTest.obj"};
    std::vector<HostScene> scenes(3);
    rt_scene views[3];
    for (int i = 0; i < 3; ++i) {
        std::string err;
        if (!scenes[i].load_obj(std::string(argv[1]) + "/" + names[i], &err)) { std::printf("FAILED to load %s: %s\n", names[i], err.c_str()); return 1; }
        scenes[i].build_octree(1000, 15);
        scenes[i].flatten();
        scenes[i].view(&views[i]);
        CHECK(validate_scene(&views[i]).status == RT_OK);
        if (validate_scene(&views[i]).status != RT_OK) continue;
        const SceneImage img(&views[i], false);
        check_image(views[i], img, false);
        check_image(views[i], SceneImage(&views[i], true), true);
        std::printf("hash %s nodes %016llx\n", names[i], fnv1a(img.nodes));
        std::printf("hash %s leaf_tris %016llx\n", names[i], fnv1a(img.leaf_tris));
        std::printf("hash %s chunks %016llx\n", names[i], fnv1a(img.chunks));
        std::printf("hash %s leaf_chunk0 %016llx\n", names[i], fnv1a(img.leaf_chunk0));
        std::printf("hash %s bad_leaves %016llx\n", names[i], fnv1a(img.bad_leaves));
        std::printf("hash %s refs %016llx\n", names[i], fnv1a(img.refs));
        std::printf("info %s nodes %zu refs %zu chunks %zu bad_leaves %u flat %d reflective %d trace_target %u\n", names[i], img.nodes.size(), img.refs.size(),
                    img.chunks.size(), img.n_bad_leaves, img.flat ? 1 : 0, img.reflective ? 1 : 0, img.trace_target);
    }
    CHECK(views[0].n_nodes == 1);                     // cube.obj: the flat scene
    CHECK(views[1].n_nodes > 1 && views[2].n_nodes > 1);
    CHECK(sliver_verdicts[0] > 0 && sliver_verdicts[1] > 0);      // (dodgeColorTest.obj has the slivers)
    if (views[0].n_nodes == 1 && views[1].n_nodes > 1) check_rules(views[1], views[0]);
    if (views[0].n_nodes == 1 && views[2].n_nodes > 1) check_rules(views[2], views[0]);
    if (failures) { std::printf("scene_image_check: %d check(s) FAILED\n", failures); return 1; }
    std::printf("scene_image_check: all checks held\n");
    return 0;
}
