// rt_launch.hpp -- the host-callable launchers of the HIP translation units (rt_kernels.hip, rt_build.hip, rt_denoise.hip, rt_upsample.hip, rt_reproject.hip), declared once for them and for
// rt_capi.cpp, which issues them.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "rt_denoise_layout.hpp"
#include "rt_device.hpp"
#include "rt_distance_layout.hpp"
#include "rt_probe_layout.hpp"
#include "rt_reproject_layout.hpp"
#include "rt_upsample_layout.hpp"

namespace rtamd {

class HostScene;

// rt_kernels.hip
void launch_trace(bool primary, bool count, bool flat, int grid, hipStream_t st, const DScene &S, const CamArg &cam, const DLights &L, const DFrame &Fr,
                  int level, int slot, const RayItem *rays_in, ShadeItem *items, Control *ctl, float4 *rec, int32_t *out_hit, float *out_t);
bool fused_tree_trace(bool primary, const DFrame &Fr);      // tree scenes: launch_trace has kernels for a launch sequence with these first rays (else launch_stage alone)
void launch_stage(bool primary, bool count, int stage, bool cont, int grid, hipStream_t st, const DScene &S, const CamArg &cam, const DLights &L,
                  const DFrame &Fr, int level, int lslots, const RayItem *rays_in, ShadeItem *items, Control *ctl, float4 *rec, int32_t *out_hit,
                  float *out_t, unsigned long long *best, unsigned long long *lit, const TaskQueues &Q);
void launch_shadow(bool count, bool flat, int grid, hipStream_t st, const DScene &S, const DLights &L, int level, int slot, int lslots,
                   uint32_t item_cap, const ShadeItem *items, Control *ctl, unsigned long long *vis, ContTask *tasks_out, uint32_t cap, uint32_t budget, uint32_t target,
                   const uint32_t *sidx);
void launch_shadow_shaft(int grid, hipStream_t st, const DScene &S, const DLights &L, int level, int slot, int lslots, uint32_t item_cap,
                         const ShadeItem *items, Control *ctl, unsigned long long *vis, ContTask *tasks_out, uint32_t cap, uint32_t budget, uint32_t target, const uint32_t *sidx,
                         const uint8_t *pair_done);
void launch_shadow_shaft_cont(int grid, hipStream_t st, const DScene &S, const DLights &L, int level, int lslots, uint32_t item_cap, const ShadeItem *items,
                              Control *ctl, unsigned long long *vis, const ContTask *tasks_in, uint32_t cap, const uint32_t *sidx);
void launch_shadow_cont(int grid, hipStream_t st, const DScene &S, const DLights &L, int level, int lslots, uint32_t item_cap, const ShadeItem *items,
                        Control *ctl, unsigned long long *vis, const ContTask *tasks_in, ContTask *tasks_out, uint32_t q_in, uint32_t q_out,
                        uint32_t cap, uint32_t budget, const uint32_t *sidx);
void launch_beam(int grid, hipStream_t st, const DScene &S, const DLights &L, int level, int lslots, uint32_t item_cap, const ShadeItem *items, Control *ctl,
                 unsigned long long *vis, uint32_t *sidx, unsigned long long *pend, float2 *ltab);
void launch_pair_beam(int grid, hipStream_t st, const DScene &S, const DLights &L, int level, int lslots, uint32_t item_cap, const ShadeItem *items, Control *ctl,
                      unsigned long long *vis, uint32_t *sidx, uint8_t *done);
void launch_shade(int grid, hipStream_t st, const DScene &S, const DLights &L, const DFrame &F, int level, int slot, int lslots,
                  const ShadeItem *items, Control *ctl, unsigned long long *vis, float4 *rec, float *fres, RayItem *rays_out, bool resolve_flat,
                  const unsigned long long *pend, const float2 *ltab);
void launch_deep(int grid, hipStream_t st, const DScene &S, const DLights &L, const DFrame &F, int level0, const RayItem *rays_in, Control *ctl, float4 *rec0, float *fres0);
void launch_resolve(int grid, hipStream_t st, const DFrame &F, const ResolveArgs &a);
void launch_flag(int grid, hipStream_t st, const DFrame &F, const float *c1, const int32_t *pos, float tau, uint8_t *refine, FlagTile *list, Control *ctl);
void launch_pass_list(int grid, hipStream_t st, const DFrame &F, const uint8_t *active, FlagTile *list, Control *ctl);
void launch_segments(int grid, hipStream_t st, const DScene &S, int n, const float *hit, const float *light, uint8_t *vis);
void launch_closest(int grid, hipStream_t st, const DScene &S, int n, const float *org, const float *dir, int32_t *face, float *t);
void launch_pack_rays(hipStream_t st, int n, const float *org, const float *dir, RayItem *rays);
void launch_occlusion(int grid, hipStream_t st, const DScene &S, int n, const float *point, const float *normal, const float *dirs, const float *rot, int m,
                      float radius, uint32_t seed, uint16_t *open, float *ao);
void launch_soft_shadows(int grid, hipStream_t st, const DScene &S, const DLights &L, int n, const float *point, const float *normal, int per_point, uint32_t seed,
                         float fu, float fv, uint16_t *visible, float *share);
void launch_gather(int grid, hipStream_t st, const DScene &S, const DLights &L, int n, const float *point, const float *normal, const float *dirs, const float *rot,
                   int m, uint32_t seed, float *rgb);
void launch_probes(int grid, hipStream_t st, const DScene &S, const DLights &L, int n, const float *position, const float *dirs, const float *wts, int m,
                   int direct, float *coeff);
void launch_gather_bounce(int grid, hipStream_t st, const DScene &S, const DLights &L, int n, const float *point, const float *normal, const float *dirs,
                          const float *rot, int m, uint32_t seed, const ProbeGrid &G, const float *src, bool visible, float *rgb);
void launch_probes_bounce(int grid, hipStream_t st, const DScene &S, const DLights &L, int n, const float *position, const float *dirs, const float *wts, int m,
                          int direct, const ProbeGrid &G, const float *src, bool visible, float *coeff);
void launch_probe_lookup(int grid, hipStream_t st, const ProbeGrid &G, const float *coeff, int n, const float *point, const float *normal, float *rgb);
void launch_probe_lookup_visible(int grid, hipStream_t st, const DScene &S, const ProbeGrid &G, const float *coeff, int n, const float *point, const float *normal,
                                 float *rgb, uint8_t *mask);
void launch_near_bounds(hipStream_t st, const DScene &S, uint32_t n_refs, uint32_t n_chunks, int cus, NearTri *recs, NearNode *boxes, NearNode *chunk_boxes);
void launch_nearest(int grid, hipStream_t st, const DScene &S, const NearNode *boxes, const NearTri *recs, const NearNode *chunk_boxes, int n,
                    const float *point_in, float r2, int32_t *face, float *dist2, float *point);
void launch_ray_hits(int grid, hipStream_t st, const DScene &S, int n, const float *org, const float *dir, int k, float t_max, int32_t *face, float *t,
                     int32_t *count);
void launch_hit_points(hipStream_t st, const DScene &S, int n, const float *org, const float *dir, const int32_t *face, const float *t, float *point,
                       float *normal);
void launch_gbuffer(int grid, hipStream_t st, const DScene &S, const DCam &cam, const DShutter &shut, const DFrame &F, const float *pass_tab, int first,
                    int count, float *out);
void launch_box_probe(hipStream_t st, int n, const float *box, const float *org, const float *dst, uint8_t *out);
void launch_phong_probe(hipStream_t st, int n, const float *in, float *out);
void launch_tree_probe(int grid, hipStream_t st, const DScene &S, int n, const float *org, const float *dst, uint32_t *out_box, uint32_t *out_ref, uint32_t *out_sig);
void launch_primary_probe(int grid, hipStream_t st, const DCam *cam, int W, int H, float *out);
void launch_set_prof(hipStream_t st, Control *ctl, uint32_t base);
void query_occupancy(bool flat, int *trace_primary, int *trace_rays, int *shadow, int *shaft, int *shade, int *beam);

// rt_build.hip
bool gpu_build_octree(HostScene &hs, int cap, int depth, hipStream_t st, std::string *err);


// rt_denoise.hip
void launch_denoise_guide(int grid, hipStream_t st, int channels, const float *in, const float *gbuffer, float4 *g0, float4 *g1, float4 *work0, uint64_t pixels);
void launch_atrous(int grid, hipStream_t st, int channels, bool last, bool staged, const void *src, const float4 *g0, const float4 *g1, void *dst,
                   int32_t width, int32_t rows, int32_t step, const DnScales &S);
bool denoise_staged_fits(int32_t step);                     // the LDS-staged variant of an iteration exists for this step

// rt_upsample.hip
void launch_upsample(int grid, hipStream_t st, int channels, const float *low, const float *gb_low, const float *gb_high, float *out, uint8_t *miss,
                     int32_t width, int32_t rows, int32_t s, const UpScales &S);

// rt_reproject.hip
void launch_reproject(int grid, hipStream_t st, int channels, const float *cur, const float *gb_cur, const float *hist, const float *gb_hist,
                      const uint8_t *len_hist, float *out, uint8_t *len_out, int32_t width, int32_t rows, const RpMap &M, const RpScales &S,
                      int32_t max_history);

}  // namespace rtamd
