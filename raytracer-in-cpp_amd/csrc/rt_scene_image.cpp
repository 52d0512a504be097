// rt_scene_image.cpp -- validation of an rt_scene view and the host arithmetic of its upload: the Morton order of the leaf face lists, the
// conservative chunk bounds every culling kernel relies on, the triangle records, the content boxes.  Host only (rt_scene_image.hpp).
#include "rt_scene_image.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include "host_scene.hpp"

namespace rtamd {

SceneVerdict validate_scene(const rt_scene *sc) {
    if (!sc || !sc->nodes || sc->n_nodes == 0 || !sc->materials || sc->n_materials == 0) return {RT_ERR_INVALID, "rt_upload_scene: empty scene"};
    if (sc->n_faces && (!sc->tri_verts || !sc->face_normal || !sc->tri_vid || !sc->mat_id || !sc->vert_normal)) return {RT_ERR_INVALID, "rt_upload_scene: missing arrays"};
    if (sc->n_nodes >= (1u << 28)) return {RT_ERR_UNSUPPORTED, "rt_upload_scene: more than 2^28 nodes"};      // (before any array is read)
    // indices and the depth bound of the traversal stack, before anything reaches a kernel
    std::vector<int> depth(sc->n_nodes, 0);
    int max_depth = 0;
    for (uint32_t i = 0; i < sc->n_nodes; ++i) {
        const rt_node &n = sc->nodes[i];
        const uint32_t cnt = n.count_flags & 0x7fffffffu;
        if (n.count_flags & RT_NODE_LEAF) {
            if (static_cast<uint64_t>(n.first) + cnt > sc->n_face_refs) return {RT_ERR_INVALID, "rt_upload_scene: leaf range outside face_refs"};
        } else {
            if (cnt > 8 || (cnt && (n.first <= i || static_cast<uint64_t>(n.first) + cnt > sc->n_nodes))) return {RT_ERR_INVALID, "rt_upload_scene: bad child range"};
            for (uint32_t k = 0; k < cnt; ++k) depth[n.first + k] = depth[i] + 1;
        }
        if (depth[i] > max_depth) max_depth = depth[i];
    }
    if (max_depth > 16) return {RT_ERR_UNSUPPORTED, "rt_upload_scene: octree deeper than 16 levels (traversal stack bound)"};
    for (uint32_t i = 0; i < sc->n_face_refs; ++i)
        if (sc->face_refs[i] >= sc->n_faces) return {RT_ERR_INVALID, "rt_upload_scene: face ref out of range"};
    for (uint32_t f = 0; f < sc->n_faces; ++f) {
        if (sc->mat_id[f] < 0 || static_cast<uint32_t>(sc->mat_id[f]) >= sc->n_materials) return {RT_ERR_INVALID, "rt_upload_scene: material id out of range"};
        for (int k = 0; k < 3; ++k)
            if (sc->tri_vid[f * 3 + k] >= sc->n_vert_normals) return {RT_ERR_INVALID, "rt_upload_scene: vertex id outside vert_normal"};
    }
    return {RT_OK, nullptr};
}

// ---------------------------------------------------------------------------------------------------------------
// Conservative chunk bounds for the lanes=triangles leaf mode.
//
// A (ray, chunk) pair may be skipped only if NO triangle of the chunk can pass Flyscene::rayTriangleIntersection as the
// reference evaluates it in float (flyscene.cpp:787-819).  That evaluation accepts a triangle when the barycentric
// coordinates of the COMPUTED point P = o + t*d (projected on the triangle's plane) pass u>=0, v>=0, u+v<1.
//   (1) P lies on the ray line up to rounding (~1e-7 * |P|), whatever the error of t.
//   (2) P is close to the triangle's plane whatever the angle between ray and plane.  With the computed num = n.A - o.n
//       (absolute error dn_ <= ~3e-7*(|A|+|o|)), den = d.n (absolute error dd_ <= ~3e-7*|d|) and t = num/den*(1+e), |e| <= 1e-7:
//           n.P - n.A = t*(den - dd_) - (num - dn_) = num*e - t*dd_ + dn_
//       so |dist(P, plane)| <= 1e-7*|num| + |t|*3e-7*|d| + 3e-7*(|A|+|o|) -- no division by den anywhere.  If |t||d| <= 4(|o|+extent)
//       this is <= ~2e-6*(|o|+extent).  If |t||d| > 4(|o|+extent), P is more than 2.3*extent away from the origin along some
//       axis, i.e. far outside every triangle, and so is its projection (P is within 3e-7*|t||d| of the plane): the true
//       barycentrics are >= ~1.3 in magnitude and their relative error (3) cannot flip a sign -- never accepted.
//   (3) With kappa = d00*d11/denom (conditioning of the reference's barycentric solve) the errors of u and v are
//       <= ~20*eps*kappa*(1+|u|+|v|), i.e. P's projection is inside the triangle grown by 1.2e-6*kappa*edge.
//   => an accepted hit implies the computed point P = o + t*d lies within  2e-6*(|o|+extent) + 1.2e-6*kappa*edge  of the
//      triangle, hence inside the chunk's inflated box, and t itself lies in the box's [t_in, t_out] of that line.
// So the chunk AABB is inflated by max(5e-6*kappa*edge) + 1e-3*max_edge + 1e-4*extent here (kappa <= 1e4 required) and the
// kernel adds 4e-4*(|o|_1+extent) per ray; a ray skips a chunk when its line misses that box or [t_in, t_out] lies outside
// the t range a hit can count in.  (An earlier version also demanded |d.n| > 0.002|d| for every triangle of the chunk, from
// a bound on dist(P, plane) that went through the RELATIVE error of d.n; the absolute form above makes that guard, and the
// per-chunk normal cone that short-cut it, unnecessary: -7 % instructions on dodgeColorTest.obj's k_shadow.)
// Chunks holding an ill-conditioned, degenerate, non-unit-normal or non-finite triangle are never cullable.
// ---------------------------------------------------------------------------------------------------------------
static uint32_t morton3(uint32_t x, uint32_t y, uint32_t z) {
    auto spread = [](uint32_t v) {
        v &= 0x3ffu; v = (v | (v << 16)) & 0x30000ffu; v = (v | (v << 8)) & 0x300f00fu;
        v = (v | (v << 4)) & 0x30c30c3u; v = (v | (v << 2)) & 0x9249249u; return v;
    };
    return spread(x) | (spread(y) << 1) | (spread(z) << 2);
}

// A triangle that rayTriangleIntersection (flyscene.cpp:787-819) can never accept, whatever the ray: a zero face normal gives
// dn = d.n = 0 for every finite direction (`dn == 0` -> rejected); a NaN normal makes t, u, v NaN (every comparison false); and when the
// float denominator d00*d11 - d01*d01 -- evaluated as the reference evaluates it -- is 0 or NaN, 1/denom is inf / NaN and u, v are each
// +-inf or NaN: u >= 0 && v >= 0 && u + v < 1 cannot hold.  Collinear triangles of real meshes are mostly of this kind; the others (a
// denominator that is one rounding error instead of zero) report hits wherever their plane is crossed and stay un-cullable.
bool never_hit(const float *v, const float *nn) {
    if (!(nn[0] == nn[0]) || !(nn[1] == nn[1]) || !(nn[2] == nn[2])) return true;
    if (nn[0] == 0.0f && nn[1] == 0.0f && nn[2] == 0.0f) {
        for (int k = 0; k < 9; ++k) if (!std::isfinite(v[k])) return false;
        return true;
    }
    const V3 A{v[0], v[1], v[2]}, B{v[3], v[4], v[5]}, C{v[6], v[7], v[8]};
    const V3 e0 = C - A, e1 = B - A;
    const float d00 = dot(e0, e0), d01 = dot(e0, e1), d11 = dot(e1, e1);
    const float inv = 1 / (d00 * d11 - d01 * d01);
    return !std::isfinite(inv);
}

// A triangle the chunk bounds cannot vouch for: non-finite, a face normal that is not unit, or a barycentric solve conditioned worse than
// kappa = d00 d11 / denom = 1e4 (edges from vertex A, as the reference sets it up).  Its computed hit points are not tied to the triangle, so
// no region bounds them: the chunk that holds it is never culled as a whole and the triangle itself never by the per-triangle shaft test
// (TriRec::flags bit 1).  Otherwise: the in-plane growth (3) of the error analysis above and the longer of its two edges.
bool tri_ill_conditioned(const float *v, const float *nn, double &edge, double &bary_infl) {
    edge = 0; bary_infl = 0;
    for (int k = 0; k < 9; ++k) if (!std::isfinite(v[k])) return true;
    const double nl = std::sqrt(double(nn[0]) * nn[0] + double(nn[1]) * nn[1] + double(nn[2]) * nn[2]);
    if (!std::isfinite(nl) || std::fabs(nl - 1.0) > 1e-3) return true;   // Face::normal is unit unless degenerate
    double e0[3], e1[3];
    for (int k = 0; k < 3; ++k) { e0[k] = double(v[6 + k]) - v[k]; e1[k] = double(v[3 + k]) - v[k]; }
    const double d00 = e0[0] * e0[0] + e0[1] * e0[1] + e0[2] * e0[2], d11 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2];
    const double d01 = e0[0] * e1[0] + e0[1] * e1[1] + e0[2] * e1[2];
    const double den = d00 * d11 - d01 * d01;
    if (!(d00 > 0) || !(d11 > 0) || !(den > 1e-4 * d00 * d11)) return true;   // kappa = d00*d11/den <= 1e4
    edge = std::sqrt(std::max(d00, d11));
    // (3): |error(u)|, |error(v)| <= ~20*eps*kappa = 1.2e-6*kappa  ->  in-plane growth 1.2e-6*kappa*edge (x4 safety)
    bary_infl = 5e-6 * (d00 * d11 / den) * edge;
    return false;
}

static void build_chunk_bounds(const rt_scene *sc, std::vector<uint32_t> &refs, std::vector<uint32_t> &leaf_chunk0,
                               std::vector<ChunkBound> &out, float extent, bool no_cull) {
    for (uint32_t ni = 0; ni < sc->n_nodes; ++ni) {
        const rt_node &nd = sc->nodes[ni];
        if (!(nd.count_flags & RT_NODE_LEAF)) continue;
        const uint32_t cnt = nd.count_flags & 0x7fffffffu;
        leaf_chunk0[ni] = static_cast<uint32_t>(out.size());
        if (cnt == 0) continue;
        uint32_t *r = refs.data() + nd.first;
        // Morton order of the centroids inside the leaf box
        float ext[3];
        for (int k = 0; k < 3; ++k) ext[k] = nd.bmax[k] - nd.bmin[k];
        std::vector<std::pair<uint32_t, uint32_t>> keyed(cnt);
        for (uint32_t i = 0; i < cnt; ++i) {
            const float *v = sc->tri_verts + static_cast<size_t>(r[i]) * 9;
            uint32_t q[3];
            for (int k = 0; k < 3; ++k) {
                const float cen = (v[k] + v[3 + k] + v[6 + k]) / 3.0f;
                float u = ext[k] > 0.f ? (cen - nd.bmin[k]) / ext[k] : 0.f;
                if (!(u > 0.f)) u = 0.f;
                if (u > 1.f) u = 1.f;
                q[k] = static_cast<uint32_t>(u * 1023.0f);
            }
            keyed[i] = {morton3(q[0], q[1], q[2]), r[i]};
        }
        std::sort(keyed.begin(), keyed.end());
        for (uint32_t i = 0; i < cnt; ++i) r[i] = keyed[i].second;
        for (uint32_t c0 = 0; c0 < cnt; c0 += 64) {
            const uint32_t n = cnt - c0 < 64 ? cnt - c0 : 64;
            ChunkBound cb{};
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, max_edge = 0, bary_infl = 0;
            bool ok = !no_cull;
            uint32_t live_tris = 0;
            double nsum[3] = {0, 0, 0}, nfirst[3] = {0, 0, 0};
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t f = r[c0 + i];
                const float *v = sc->tri_verts + static_cast<size_t>(f) * 9;
                const float *nn = sc->face_normal + static_cast<size_t>(f) * 3;
                if (never_hit(v, nn)) continue;         // cannot be hit by any ray AS THE REFERENCE COMPUTES IT: no bound needed for it
                double edge, binfl;
                if (tri_ill_conditioned(v, nn, edge, binfl)) { ok = false; continue; }      // (the well-conditioned ones still get their inflation: below)
                ++live_tris;
                for (int k = 0; k < 3; ++k) {
                    lo[k] = std::min(lo[k], double(std::min(v[k], std::min(v[3 + k], v[6 + k]))));
                    hi[k] = std::max(hi[k], double(std::max(v[k], std::max(v[3 + k], v[6 + k]))));
                }
                max_edge = std::max(max_edge, edge);
                bary_infl = std::max(bary_infl, binfl);
                // area-weighted mean normal (e1 x e0 has twice the area as its length), orientation of the chunk's first triangle
                double e0[3], e1[3];
                for (int k = 0; k < 3; ++k) { e0[k] = double(v[6 + k]) - v[k]; e1[k] = double(v[3 + k]) - v[k]; }
                const double cr[3] = {e1[1] * e0[2] - e1[2] * e0[1], e1[2] * e0[0] - e1[0] * e0[2], e1[0] * e0[1] - e1[1] * e0[0]};
                if (live_tris == 1) for (int k = 0; k < 3; ++k) nfirst[k] = cr[k];
                const double sg = (cr[0] * nfirst[0] + cr[1] * nfirst[1] + cr[2] * nfirst[2]) < 0 ? -1.0 : 1.0;
                for (int k = 0; k < 3; ++k) nsum[k] += sg * cr[k];
            }
            if (ok) {
                const double infl = bary_infl + 1e-3 * max_edge + 1e-4 * extent;
                for (int k = 0; k < 3; ++k) {
                    cb.lo[k] = std::nextafter(static_cast<float>(lo[k] - infl), -INFINITY);
                    cb.hi[k] = std::nextafter(static_cast<float>(hi[k] + infl), INFINITY);
                }
                cb.never = 0.0f;
                cb.infl = std::nextafter(static_cast<float>(infl), INFINITY);
                // the slab: any unit direction gives a valid bound (the point of an accepted hit lies within infl per axis of its triangle, a
                // convex combination of the vertices), the mean normal gives the thin one
                double nl = std::sqrt(nsum[0] * nsum[0] + nsum[1] * nsum[1] + nsum[2] * nsum[2]);
                double sn[3] = {0, 0, 1};
                if (std::isfinite(nl) && nl > 1e-30) for (int k = 0; k < 3; ++k) sn[k] = nsum[k] / nl;
                for (int k = 0; k < 3; ++k) cb.sn[k] = static_cast<float>(sn[k]);
                double slo = 1e300, shi = -1e300;
                for (uint32_t i = 0; i < n; ++i) {
                    const uint32_t f = r[c0 + i];
                    const float *v = sc->tri_verts + static_cast<size_t>(f) * 9;
                    if (never_hit(v, sc->face_normal + static_cast<size_t>(f) * 3)) continue;
                    for (int q = 0; q < 3; ++q) {
                        const double dq = double(cb.sn[0]) * v[3 * q] + double(cb.sn[1]) * v[3 * q + 1] + double(cb.sn[2]) * v[3 * q + 2];
                        slo = std::min(slo, dq); shi = std::max(shi, dq);
                    }
                }
                const double sinfl = 1.0625 * (std::fabs(double(cb.sn[0])) + std::fabs(double(cb.sn[1])) + std::fabs(double(cb.sn[2]))) * double(cb.infl);
                cb.slo = live_tris ? std::nextafter(static_cast<float>(slo - sinfl), -INFINITY) : -3e38f;
                cb.shi = live_tris ? std::nextafter(static_cast<float>(shi + sinfl), INFINITY) : 3e38f;
            }
            if (ok && live_tris == 0) { for (int k = 0; k < 3; ++k) cb.lo[k] = cb.hi[k] = 1e30f; cb.infl = 0.0f; }     // nothing hittable inside: a far-away point
            if (!ok) {
                // never culled as a whole; its well-conditioned triangles keep THEIR inflation for the per-triangle shaft test of the shadow units
                // (0: there is none -- no_cull, or every triangle of the chunk is ill-conditioned)
                const double infl = bary_infl + 1e-3 * max_edge + 1e-4 * extent;
                cb = ChunkBound{}; cb.never = 2.0f; cb.slo = -3e38f; cb.shi = 3e38f;
                cb.infl = (!no_cull && live_tris) ? std::nextafter(static_cast<float>(infl), INFINITY) : 0.0f;
            }
            out.push_back(cb);
        }
    }
    if (out.empty()) { ChunkBound cb{}; cb.never = 2.0f; cb.slo = -3e38f; cb.shi = 3e38f; out.push_back(cb); }
}

// Leaf face lists are re-ordered along a Morton curve (the order inside a leaf cannot change any result: closest
// hit is a minimum with a face-id tie-break, shadow rays are any-hit), so that every run of 64 references -- one
// `chunk` of the lanes=triangles mode -- is spatially compact and its conservative bound is tight.
ChunkSet::ChunkSet(const rt_scene *sc, bool no_cull) : refs(sc->face_refs, sc->face_refs + sc->n_face_refs), leaf_chunk0(sc->n_nodes, 0u) {
    for (size_t i = 0; i < static_cast<size_t>(sc->n_faces) * 9; ++i) extent = std::fmax(extent, std::fabs(sc->tri_verts[i]));
    build_chunk_bounds(sc, refs, leaf_chunk0, chunks, extent, no_cull);
}

SceneImage::SceneImage(const rt_scene *sc, bool no_cull) : ChunkSet(sc, no_cull), leaf_tris(sc->n_face_refs), nodes(sc->n_nodes) {
    // leaf-ordered triangle records: the per-triangle constants of rayTriangleIntersection (flyscene.cpp:787-811),
    // evaluated once with the same float operations the reference performs on every call
    for (uint32_t i = 0; i < sc->n_face_refs; ++i) {
        const uint32_t f = refs[i];
        const float *v = sc->tri_verts + static_cast<size_t>(f) * 9;
        const float *n = sc->face_normal + static_cast<size_t>(f) * 3;
        TriRec &r = leaf_tris[i];
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
    for (uint32_t m = 0; m < sc->n_materials; ++m) {
        const int il = sc->materials[m].illum;
        if (il == 9 || il == 6 || (il > 2 && il < 6)) reflective = true;
    }

    // device nodes = public nodes + content boxes, bottom-up (children always follow their parent in the array)
    for (uint32_t ii = sc->n_nodes; ii-- > 0;) {
        const rt_node &n = sc->nodes[ii];
        DNode &dn = nodes[ii];
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
                const ChunkBound &cb = chunks[leaf_chunk0[ii] + k];
                if (cb.never >= 1.5f) open_box = true; else grow(cb.lo, cb.hi);
            }
            if (open_box) { for (int k = 0; k < 3; ++k) bad_leaves.push_back(n.bmin[k]); for (int k = 0; k < 3; ++k) bad_leaves.push_back(n.bmax[k]); }
        } else {
            for (uint32_t k = 0; k < cnt; ++k) {
                const DNode &ch = nodes[n.first + k];
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
    const size_t n_bad = bad_leaves.size() / 6;
    if (bad_leaves.empty()) bad_leaves.assign(6, 0.0f);
    n_bad_leaves = n_bad <= 32 ? static_cast<uint32_t>(n_bad) : 0xffffffffu;

    flat = (sc->nodes[0].count_flags & RT_NODE_LEAF) && (sc->nodes[0].count_flags & 0x7fffffffu) <= 64u;
    std::memcpy(root_box, sc->nodes[0].bmin, sizeof(float) * 3);
    std::memcpy(root_box + 3, sc->nodes[0].bmax, sizeof(float) * 3);
    { const uint32_t t = sc->n_face_refs / 256u; trace_target = t < 1000u ? 1000u : (t > 4000u ? 4000u : t); }
}

}  // namespace rtamd
