// rt_scene_layout.hpp -- the records of an uploaded scene: what the host prepares (rt_scene_image.cpp), what rt_upload_scene copies to the
// device and what the kernels walk.  No HIP here: the host-only scene preparation and its check program include this header alone.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rt_mi355x.h"

namespace rtamd {

// Per-(leaf, triangle) record, 80 B = s_load_dwordx16 + s_load_dwordx4.  Everything here is a pure function of
// the triangle that Flyscene::rayTriangleIntersection (flyscene.cpp:787-819) recomputes on every call.
struct alignas(16) TriRec {
    float ax, ay, az;        // vertices[0]
    float e0x, e0y, e0z;     // v0 = vertices[2] - vertices[0]
    float e1x, e1y, e1z;     // v1 = vertices[1] - vertices[0]
    float nx, ny, nz;        // triangle.normal
    float nA;                // triangleNormal.dot(vertices[0])
    float d00, d01, d11;     // v0.v0, v0.v1, v1.v1
    float inv_denom;         // 1 / (d00*d11 - d01*d01)
    uint32_t face;           // face id (tie-break: lowest id wins, std::set order + strict '<')
    uint32_t flags;          // bit 0: material illum == 9 (skipped by lightStrikes, flyscene.cpp:934-936)
    uint32_t pad;
};
static_assert(sizeof(TriRec) == 80, "TriRec must be 80 bytes");

// Conservative bound of one 64-triangle chunk of a leaf.  A ray may skip the chunk only when it is provably impossible for ANY
// triangle of the chunk to pass rayTriangleIntersection AS THE REFERENCE COMPUTES IT IN FLOAT with a t the caller still counts:
// the point of an accepted hit lies inside this inflated box (rt_scene_image.cpp: build_chunk_bounds has the error analysis).
struct alignas(16) ChunkBound {
    float lo[3], hi[3];      // AABB of the chunk's triangles, inflated
    float never;             // 0: the chunk may be culled; 2: never (ill-conditioned / degenerate / non-finite triangle inside)
    float infl;              // the inflation: the point of an accepted hit lies within `infl` (per axis) of the TRIANGLE it was accepted for
    // the same bound along ONE more direction: sn . P lies in [slo, shi] for the point P of every accepted hit (sn: the chunk's mean face
    // normal; the interval is the chunk's extent along it, inflated like the box).  A patch of a smooth surface is a thin plate in a fat
    // axis-aligned box: rays that graze the surface cross the box and miss the plate.  Never-cullable chunks: sn = 0, (-3e38, 3e38).
    float sn[3], slo, shi;
    float pad_[3];
};
static_assert(sizeof(ChunkBound) == 64, "ChunkBound must be 64 bytes");

// Device copy of a node: the public rt_node (the reference's box, used for the bit-exact boxIntersect) followed by the node's
// CONTENT box -- the union of the inflated chunk boxes of every leaf below it (rt_scene_image.cpp, build_chunk_bounds), or
// (-3e38, 3e38) when some chunk below is not cullable.  A ray whose line has no countable point inside the content box
// cannot have an accepted hit anywhere in the subtree, whatever the reference's own box test says.  64 B = one
// s_load_dwordx16 per child.
struct alignas(16) DNode {
    float bmin[3], bmax[3];
    uint32_t first, count_flags;
    float clo[3], chi[3];
    uint32_t pad[2];               // pad[0]: leaves -- index of the leaf's first ChunkBound (chunks[]); pad[1]: 1 -- the subtree holds a chunk
                                   // that may never be culled (or its content box is not finite): the walk descends on the node's own box alone
};
static_assert(sizeof(DNode) == 64, "DNode must be 64 bytes");

struct DScene {
    const DNode *nodes;
    const TriRec *leaf_tris;
    const ChunkBound *chunks;          // per leaf: ceil(count/64) bounds starting at leaf_chunk0[node]
    const uint32_t *leaf_chunk0;
    float extent;                      // max |coordinate| of the scene (for the per-ray slab padding)
    const float *tri_verts;
    const float *face_normal;
    const uint32_t *tri_vid;
    const int32_t *mat_id;
    const float *vert_normal;
    const rt_material *mats;
    float model[12];
    uint32_t n_nodes, n_faces;
    int32_t queue_local;               // k_shadow queue: -1 auto, 0 strided chunks (balance first), n chunks of n consecutive units
    int32_t plane_cull;                // k_shadow: per-unit plane culling (rt_kernels.hip, SegPacket); RT_NO_PLANE_CULL=1 turns it off
    int32_t queue_div;                 // k_shadow_shaft: units are handed out in chunks of units / (waves x queue_div)
    const float *bad_leaves;           // boxes (min, max) of the leaves that hold a chunk which may never be culled (k_beam tests them per hit)
    uint32_t n_bad_leaves;             // 0xffffffff: too many for the per-hit test -- such a chunk then blocks every beam that meets it
    int32_t beam;                      // k_beam before the shadow kernels: whole tiles of 64 lit hits whose sample rays nothing can block; RT_NO_BEAM=1 turns it off
    int32_t beam_budget;               // k_beam: group steps + chunk batches + chunks a beam may spend before it leaves its hits to the shadow units (RT_BEAM_BUDGET)
    int32_t shaft;                     // k_shadow on tree scenes: shaft-culled group walk (rt_kernels.hip, shaft_walk); RT_NO_SHAFT=1 turns it off
};

}  // namespace rtamd
