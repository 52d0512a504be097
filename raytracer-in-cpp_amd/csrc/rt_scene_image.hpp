// rt_scene_image.hpp -- the host half of a scene upload: one validation of an rt_scene view and one image of what the kernels walk, built
// from a validated view.  Host arithmetic only: no HIP, no environment.  tools/scene_image_check.cpp builds and checks both under the host
// sanitizers; rt_debug_chunk_stats / rt_debug_chunk_bounds (rt_capi.cpp) validate and read the ChunkSet.  rt_upload_scene takes its chunk
// bounds from ChunkSet but still validates and makes the triangle records and content boxes itself, with the text SceneImage was moved
// from (Scene image, says why): until it reads a SceneImage, a change to either copy goes into both, and
// tests/golden/scene_image.json is what holds this one to the other.
#pragma once

#include <cstdint>
#include <vector>

#include "rt_mi355x.h"
#include "rt_scene_layout.hpp"

namespace rtamd {

// Why a view cannot be uploaded: RT_OK and a null message, or the status and text rt_upload_scene reports.  Every index the image (and a
// kernel) follows is tested here, so nothing below reads an rt_scene that has not passed.
struct SceneVerdict {
    rt_status status;
    const char *message;
};
SceneVerdict validate_scene(const rt_scene *sc);

// The chunk bounds of a validated view and what they come with.  (no_cull: every chunk is never-cullable, RT_NO_CULL)
struct ChunkSet {
    std::vector<uint32_t> refs;          // face_refs, every leaf's range in the Morton order its chunks hold (leaf_tris follows it; not uploaded)
    std::vector<uint32_t> leaf_chunk0;   // per node: index of a leaf's first chunk
    std::vector<ChunkBound> chunks;      // never empty
    float extent = 0.f;                  // max |coordinate| of the scene
    ChunkSet(const rt_scene *sc, bool no_cull);
};

// What the kernels walk, as it goes to the device, and what the context keeps beside it: the chunk set and what is built on it.
struct SceneImage : ChunkSet {
    std::vector<TriRec> leaf_tris;       // one per face reference
    std::vector<DNode> nodes;
    std::vector<float> bad_leaves;       // boxes (min, max) of the leaves with a chunk that may never be culled (k_beam), in the order the
                                         // bottom-up pass meets them: from the last node to the first; six zeros when there is none
    uint32_t n_bad_leaves = 0;           // their count, or 0xffffffff above 32 (DScene::n_bad_leaves)
    bool reflective = false;             // some material spawns bounce rays (illum 3,4,5,6,9)
    bool flat = false;                   // the root is a small leaf (cube.obj): specialised stack-free kernels
    float root_box[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // nodes[0].bmin / bmax
    uint32_t trace_target = 1000u;       // estimated cost of one leaf-task piece of the trace stages, by leaf references
    // sc: a view validate_scene has passed; no_cull: every chunk is never-cullable and every content box open (RT_NO_CULL)
    SceneImage(const rt_scene *sc, bool no_cull);
};

// the predicates the chunk bounds and TriRec::flags bit 1 are made of (rt_scene_image.cpp has the error analysis)
bool never_hit(const float *v, const float *nn);
bool tri_ill_conditioned(const float *v, const float *nn, double &edge, double &bary_infl);

}  // namespace rtamd
