#!/usr/bin/env python3
"""bench.py -- measures BASELINE.json's metric: Mrays/s (+ ms/frame) of the ray-trace path at 1920x1080, depth 4,
64-sample (8x8) area light, default scene (resources/models/cube.obj -> tests/golden/scenes/cube.obj), N GPUs.

A "step" is one whole frame: primary generation + closest hit + light-centre visibility + area-light sample
shadow rays + shading + bounces + resolve/quantise (+ the RCCL row gather when N > 1).  Inputs (flattened octree,
triangle records, materials) are resident in HBM before the timed region; output stays on the device.
`value` = rays of the whole frame (all ranks) per second, a ray being one traversal query as SURVEY.md 8(d) defines it.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--scene cube|dodge|wavy] [--width 1920 --height 1080 --grid 8 --depth 4]
                  [--dump-outputs DIR] [--full]
N > 1 is launched by torch.distributed.run (one rank per GPU, RCCL).

A plain run does what the headline needs and nothing else: scene upload, one untimed frame for the ray counters, W warm-up frames,
exactly K timed frames, one JSON line (`value`, `ms_per_step` = milliseconds of one timed frame, the configuration, the ray counts).
--dump-outputs DIR writes what the last timed frame returned to the caller: `rgb.npy` (float RGB) and `rgb_u8.npy` (the 8-bit
resolve, as float32), each [height, width, 3]; N > 1: the frame rank 0 assembled from the gathered rows, `frame_u8.npy`.  Above
64 MB in all, a fixed seeded sample of the pixels is written instead, with their indices in `pixel_index.npy`.

--full adds everything else the benchmark measures: per-kernel HIP-event times on about four of the timed frames, the executed-work
roofline, the PMC constants of profiles/, the hipGraph replay, the CPU baseline and, for N > 1, the per-rank times and the check of
the assembled frame against a plain render of the whole frame.  The headline (`value`) is the configured default scene, cube.obj --
a 1-node tree, i.e. the FLAT kernels.  The default --full invocation therefore ALSO times the two tree scenes with the same code and
reports them under `tree_scenes` with their own ms_per_step, per-kernel times, roofline and cpu_baseline: dodgeColorTest.obj at the
headline settings and BASELINE cfg4 (3840x2160, depth 8, 256 samples, ~1M-triangle synthetic mesh).

Roofline (--full).  The path is traversal / branch bound and its scenes are cache resident: the bound that limits the kernels is VALU ISSUE, not
HBM and not MFMA.  `roofline` therefore reports (all <= 1 by construction, all from THIS run unless marked `constant`):
  * achieved = modelled VALU wave-instructions of the dominant kernel (k_shadow: area-light sample shadow rays) -- the wave-level STEP
    COUNTS the shipped kernels executed for this very frame (counted by the same sources built with step counters,
    librt_mi355x_work.so, in an untimed pass) x the instruction cost of each step kind -- per SIMD per ns of the live
    launch time (HIP events on the launch stream inside the timed region); peak = the plain-FP32 issue rate measured on this chip
    (tools/micro/valu_rate.hip: 0.967 wave-instructions per SIMD per ns); `useful_frac` counts only the reference's own arithmetic
    (boxIntersect + rayTriangleIntersection evaluations), `frac` everything the kernel has to issue;
  * executed_valu: the hardware's own instruction count (SQ_INSTS_VALU, its own rocprofv3 --pmc pass, profiles/valu.json) over the live
    time -- a CONSTANT from profiles/, quoted only while profiles/valu.json carries the sha256 of the kernels source it was taken with;
  * traffic / hbm_frac: HBM bytes per launch from the TCC counters (profiles/traffic.json, same stamping) and their share of 8 TB/s;
  * reference_semantics_bytes: SURVEY 8(d)'s algorithmic-byte figure (24 B x box tests + 52 B x leaf triangle refs, every triangle of
    every intersected leaf, no early-out), counted exactly by the COUNT kernel variants.  Divided by the launch time it EXCEEDS the
    HBM peak (the culling skips most of that work exactly), so it is reported as a workload size, not as a utilisation.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

VALU_PEAK_PER_SIMD_NS = 0.967   # measured: tools/micro/valu_rate.hip (plain FP32 wave64 ops, 8 waves/SIMD); 0.5 per cycle, i.e. the chip held ~1.93 GHz in that run
N_SIMDS = 1024                  # 256 CUs x 4 SIMDs
HBM_PEAK_GBS = 8000.0           # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip-level parameters)
BOX_BYTES, TRI_REF_BYTES = 24, 52   # algorithmic bytes per box test / per leaf triangle reference
RT_WORK_SHADOW = 640            # rt_device.hpp: offset of the shadow kernels' step counters in Control::prof

# VALU wave-instructions per wave-level step: static counts of each loop body in the gfx950 listing of the shipped kernels (`make isa`;
# DESIGN.md 6).  The model lands within ~15 % of SQ_INSTS_VALU (profiles/valu.json), which is quoted beside it.
COST = {
    "tri_lanes_triangles": 68,   # one ray broadcast against the 64 triangles of a chunk: rayTriangleIntersection + 6 v_readlane + hit bookkeeping (137 per 2-ray iteration)
    "tri_lanes_rays": 45,        # one triangle against the wave's 64 rays (flat scenes: cube)
    "tri_lanes_rays_shaft": 57,  # the same step in the shaft kernel (triangles that survive the per-triangle shaft test; 114 per 2-triangle iteration)
    "node_per_ray": 90,          # a surviving child: record broadcast + content test + verified boxIntersect + masks (the IEEE-division fallback not counted)
    "box_stack_walk": 55,        # stack walk (packet_walk) child: content test + verified boxIntersect
    "shaft_group": 90,           # lane = (child, test): group pop, two separating tests, ballots, byte reduction
    "leaf_chunk_batch": 73,      # lane = (chunk, test) on 8 chunk bounds
    "chunk_per_ray": 39,         # per-ray conservative chunk test (7 v_readlane + slab test)
    "tri_shaft_test": 140,       # lane = triangle: 3 vertex boxes against 6 tangent planes + near box + the (t <= 0 or |t| >= 0.98) plane rule
    "unit_shaft": 270,           # k_shadow_shaft per unit: queue, item, sample, root test, shaft planes (make_shaft_lanes ~95), LDS records
    "unit_flat": 355,            # flat k_shadow per unit: queue, item, h, shaft planes (~85), 8 triangles x 8 tests per step (2 x ~45 on the cube), plane rule, visibility word
    "unit_stack": 200,
    "unit_trace": 260,           # trace kernels per unit (a tile of 64 rays, or a leaf task): ray generation (Camera::screenToWorld in double), root tests, records / compaction
    "pair_beam": 230,            # k_pair_beam per (hit, light): scalar item, shaft planes of the whole light, LDS records, direction check, visibility words / survivor buffer
    "beam_group": 70,            # its group step: lane = (child, test) on content and own boxes (no per-ray tests)
    "beam_chunk_batch": 60,      # 8 chunk bounds against the shaft
    "beam_tri_chunk": 120,       # one chunk triangle by triangle (lane = triangle): tangent planes, near box, the plane rules over the interval of h.n
    "beam": 700,                 # k_beam per (tile of 64 hits, light) on a flat scene: items, wave min / max, planes, one leaf (chunk test + per-triangle test)
    "shade_sample": 151,         # k_shade per (tile of 64 hits, sample): light direction + reflection normalised (2 x sqrt, the three quotients of each share one reciprocal), glibc powf in double (branch-free: range and special answers are selects)
    "shade_tile": 1100,          # k_shade per tile: items, interpolated normal, eye vector, material, record; flat scenes: the child ray against the root leaf
}


def kernels_sha():
    return hashlib.sha256(open(os.path.join(ROOT, "raytracer-in-cpp_amd", "csrc", "rt_kernels.hip"), "rb").read()).hexdigest()


def scene_of(name):
    if name == "wavy":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import scenes_gen
        import tempfile
        return ("wavy708.obj (synthetic 708x708 displaced grid + floor, 1,002,530 triangles)",
                scenes_gen.wavy_grid(os.path.join(tempfile.gettempdir(), f"rt_wavy_{os.getpid()}"), n=708))
    f = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj"}[name]
    return f, os.path.join(ROOT, "tests", "golden", "scenes", f)


def work_counters(pkg, hs, W, H, G, D):
    """one untimed frame on the counting build (same kernel sources + wave-level step counters): what the shipped kernels executed"""
    capi = pkg.capi
    path = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")
    if not os.path.exists(path):
        return None
    import numpy as np
    lib = capi.load_library(path)
    ctx = C.c_void_p()
    if lib.rt_create(C.byref(ctx), 0) != capi.RT_OK:
        return None
    try:
        capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(hs.view)), "work: rt_upload_scene")
        cam = pkg.default_camera(W, H)
        L = pkg.make_lights(area=True, usteps=G, vsteps=G)
        p = pkg.make_params(W, H, D)
        rgb = np.zeros(W * H * 3, np.float32)
        capi.check(lib, ctx, lib.rt_render(ctx, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), None, None), "work: rt_render")
        buf = (C.c_uint64 * 768)()
        capi.check(lib, ctx, lib.rt_debug_work_counters(ctx, buf, 768), "rt_debug_work_counters")
        a = [int(x) for x in buf]
    finally:
        lib.rt_destroy(ctx)
    s = a[RT_WORK_SHADOW:RT_WORK_SHADOW + 96]
    t = a[0:96]
    # Control::prof[RT_WORK_SHADOW + k]: step counters of the shadow kernels (k_beam, k_shadow, k_shadow_shaft and their leaf-task launches)
    names = {0: "tri_steps_lanes_rays", 2: "tri_steps_lanes_triangles", 4: "box_steps_stack_walk", 12: "chunk_tests_stack_walk", 13: "units",
             88: "shaft_groups", 90: "nodes_tested_per_ray", 91: "nodes_hit", 92: "leaf_chunk_batches", 94: "chunks_tested_per_ray", 95: "chunks_with_work",
             70: "tri_shaft_tests", 71: "tri_shaft_survivors", 72: "tri_shaft_rays", 73: "tri_shaft_empty_chunks", 74: "node_test_live_rays", 75: "node_hit_rays", 76: "beams_tested", 77: "beams_unblocked", 78: "beam_hits_checked_per_leaf_list", 79: "beam_hits_that_reach_a_bad_leaf", 80: "beam_steps_of_unblocked", 81: "beams_over_budget",
             82: "beam_group_steps", 83: "beam_children_in_shaft", 84: "beam_leaf_visits", 85: "beam_chunk_batches", 86: "beam_chunks_tested_by_triangle"}
    # Control::prof[k]: step counters of the trace kernels (k_trace / k_stage and the leaf-task launches of the two traversal stages).  They share
    # the leaf code (leaf_visit) with the shadow kernels but none of the shaft / beam steps, so the region has names of its own.
    trace_names = {0: "tri_steps_lanes_rays", 2: "tri_steps_lanes_triangles", 4: "box_steps_stack_walk", 6: "leaves_lanes_rays", 7: "leaves_lanes_triangles",
                   12: "chunk_tests_stack_walk", 13: "units", 14: "ray_chunk_pairs_culled", 66: "ray_node_pairs_content_culled",
                   70: "tri_cone_tests", 71: "tri_cone_survivors", 73: "tri_cone_empty_chunks"}
    return {"shadow": {v: s[k] for k, v in names.items()}, "trace": {v: t[k] for k, v in trace_names.items()}}


def trace_model(work, flat):
    """modelled VALU wave-instructions of the trace group (closest hit + light-centre visibility + finish): (useful, total)"""
    w = work["trace"]
    useful = w["tri_steps_lanes_triangles"] * COST["tri_lanes_triangles"] + w["tri_steps_lanes_rays"] * COST["tri_lanes_rays"] + w["box_steps_stack_walk"] * COST["box_stack_walk"]
    return useful, useful + w["units"] * COST["unit_trace"] + w["chunk_tests_stack_walk"] * 30 + w["tri_cone_tests"] * COST["tri_shaft_test"]


def valu_model(work, flat, shaft):
    """modelled VALU wave-instructions of the shadow kernels of the frame: (useful, total)"""
    w = work["shadow"]
    useful = w["tri_steps_lanes_triangles"] * COST["tri_lanes_triangles"] + w["tri_steps_lanes_rays"] * COST["tri_lanes_rays_shaft" if shaft and not flat else "tri_lanes_rays"]
    if flat:
        return useful, useful + w["units"] * COST["unit_flat"] + w.get("beams_tested", 0) * COST["beam"]
    if shaft:
        useful += w["nodes_tested_per_ray"] * COST["node_per_ray"]
        total = useful + w["units"] * COST["unit_shaft"] + w["shaft_groups"] * COST["shaft_group"] + w["leaf_chunk_batches"] * COST["leaf_chunk_batch"] + \
            w["chunks_tested_per_ray"] * COST["chunk_per_ray"] + w["tri_shaft_tests"] * COST["tri_shaft_test"]
        # (the leaf-task launch runs the same leaf code and reports through the same counters)
        total += w["chunk_tests_stack_walk"] * 30
        # the per-hit beam test in front of the units (lights of more than 64 samples): calibrated on cfg4, 1,051 modelled against 1,073 executed per beam
        total += w.get("beams_tested", 0) * COST["pair_beam"] + w.get("beam_group_steps", 0) * COST["beam_group"] + \
            w.get("beam_chunk_batches", 0) * COST["beam_chunk_batch"] + w.get("beam_chunks_tested_by_triangle", 0) * COST["beam_tri_chunk"]
        return useful, total
    useful += w["box_steps_stack_walk"] * COST["box_stack_walk"]
    return useful, useful + w["units"] * COST["unit_stack"] + w["chunk_tests_stack_walk"] * 30


def clock_independent(kernels, pick):
    """SQ_INSTS_VALU / (GRBM_GUI_ACTIVE / 8) / 1024 SIMDs / 0.5 wave-instructions per cycle, launch by launch (profiles/valu.json): the share of
    the VALU issue peak the launches reached WHATEVER clock the chip held (the per-ns figures above divide by a rate measured at ~1.93 GHz).
    With the second PMC pass: SQ_ACTIVE_INST_VALU / SQ_BUSY_CYCLES-style busy shares where the counters were collected."""
    sel = {k: v for k, v in kernels.items() if pick(k) and v.get("gpu_cycles")}
    if not sel:
        return {}
    insts = sum(v["valu_wave_instructions"] for v in sel.values())
    cyc = sum(v["gpu_cycles"] for v in sel.values())
    out = {"frac_clock_independent": round(insts / cyc / N_SIMDS / 0.5, 4),
           "clock_independent_source": "sum SQ_INSTS_VALU / sum (GRBM_GUI_ACTIVE / 8) / 1024 SIMDs / 0.5 per cycle over the level-0 launches of the group"}
    act = [v for v in sel.values() if v.get("active_inst_valu") and v.get("wave_cycles")]
    if act:
        # second PMC pass (tools/valu.sh): SQ_ACTIVE_INST_VALU = quad-cycles in which a wave executes a VALU instruction, SQ_WAVE_CYCLES = quad-cycles of wave
        # lifetime.  Their ratio is the share of its lifetime a wave spends executing VALU work; ACTIVE over the instruction count is the execution time per
        # instruction as the hardware counts it (1.0 = 4 cycles; half-rate FP64 work would push it up) -- counters, not estimates
        a, w, n = sum(v["active_inst_valu"] for v in act), sum(v["wave_cycles"] for v in act), sum(v["valu_wave_instructions"] for v in act)
        out["wave_lifetime_share_executing_valu"] = round(a / w, 4)
        out["valu_active_quadcycles_per_instruction"] = round(a / n, 4)
        out["valu_active_source"] = "SQ_ACTIVE_INST_VALU, SQ_WAVE_CYCLES, SQ_BUSY_CYCLES (second rocprofv3 --pmc pass of tools/valu.sh)"
    return out


def pmc_constant(fname, scene, cfg, sha):
    """an entry of profiles/valu.json / traffic.json, only while it was taken with the kernels source that is being timed"""
    try:
        j = json.load(open(os.path.join(ROOT, "profiles", fname)))
        ent = j.get(scene)
        if not ent or ent.get("config") != cfg:
            return None, "no entry for this workload"
        if ent.get("kernels_sha256") != sha:
            return None, "profiles/%s was collected with a different rt_kernels.hip (stale): not quoted" % fname
        return ent, None
    except Exception as e:       # noqa: BLE001
        return None, str(e)


DUMP_BUDGET_BYTES = 64_000_000      # --dump-outputs: all files together (4 KiB of it left for the .npy headers)


def dump_outputs(dirpath, frames):
    """--dump-outputs: each [H, W, 3] frame of `frames` as <name>.npy in float32.  Over the budget, the same fixed seeded sample of
    pixels from every frame, their flat indices (y * W + x) in pixel_index.npy (float64, exact)."""
    import numpy as np
    os.makedirs(dirpath, exist_ok=True)
    out = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in frames.items()}
    if sum(a.nbytes for a in out.values()) > DUMP_BUDGET_BYTES:
        npix = next(iter(out.values())).shape[0] * next(iter(out.values())).shape[1]
        per_pixel = sum(a.nbytes for a in out.values()) // npix + 8
        idx = np.sort(np.random.default_rng(0).choice(npix, (DUMP_BUDGET_BYTES - 4096) // per_pixel, replace=False))
        out = {k: a.reshape(npix, -1)[idx] for k, a in out.items()}
        out["pixel_index"] = idx.astype(np.float64)
    for k, a in out.items():
        np.save(os.path.join(dirpath, k + ".npy"), a)


def run_single(pkg, torch, dev, scene, W, H, G, D, S, steps, warmup, want_cpu, cpu_stride, want_graph, want_work=True, full=True, outputs=None):
    """N = 1: eager launches; returns the record of this workload.  full: per-kernel HIP events on about four of the timed steps and
    every figure beside the headline; otherwise the headline only.  `outputs` (a dict) receives the frames of the last timed step."""
    import numpy as np
    capi = pkg.capi
    scene_file, scene_path = scene_of(scene)
    hs = pkg.HostScene(scene_path, 1000, 15)
    ctx = pkg.Context(dev.index)
    ctx.upload(hs)
    lib = ctx.lib
    cam = pkg.default_camera(W, H)
    L = pkg.make_lights(area=True, usteps=G, vsteps=G)
    out_rgb = torch.zeros(H * W * 3, dtype=torch.float32, device=dev)
    out_u8 = torch.zeros(H * W * 3, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)

    def _p(collect):
        p = pkg.make_params(W, H, D, 0, H, S, 0, 1)
        p.collect_stats = collect
        return p

    def render(p, stats=None):
        st = lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(out_rgb.data_ptr()), C.c_void_p(out_u8.data_ptr()), None,
                                  C.c_void_p(stream.cuda_stream), C.byref(stats) if stats is not None else None)
        capi.check(lib, ctx.handle, st, "rt_render_device")

    # untimed: the ray counters of one frame (--full: also the algorithmic counters, from the no-early-out counting variants)
    cnt = capi.rt_stats()
    render(_p(1 if full else 0), cnt)
    torch.cuda.synchronize(dev)
    rays_frame = cnt.total_rays()
    p_timed, p_plain = _p(2 if full else 0), _p(0)
    for _ in range(warmup):
        render(p_timed)
    torch.cuda.synchronize(dev)
    if full:
        lib.rt_timing_collect(ctx.handle, C.byref(capi.rt_stats()))
    # ---- timed region: EXACTLY K steps between synchronisations
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    # --full: per-kernel HIP events on about four of the timed steps (their ~17 event records cost ~40-60 us of a 0.3 ms frame: every 4th
    # step, as until round 3, put ~3 % on the headline)
    period = 4 if steps < 16 else steps // 4
    for i in range(steps):
        render(p_timed if i % period == 0 else p_plain)
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    if outputs is not None:
        outputs["rgb"] = out_rgb.view(H, W, 3).cpu().numpy()
        outputs["rgb_u8"] = out_u8.view(H, W, 3).cpu().numpy()
    ms_step = elapsed / steps * 1e3
    value = rays_frame * steps / elapsed / 1e6
    info = hs.info()
    scene_cfg = {"workload": f"{W}x{H} depth {D} {G * G}-sample area light, {scene_file}, 1 light, row stripes of {S} over 1 GPU(s)",
                 "width": W, "height": H, "max_depth": D, "samples": G * G, "scene": scene_file, "parallelism": "rows1", "step": "eager launches",
                 "tree": {k: info[k] for k in ("nodes", "leaves", "face_refs", "max_leaf", "depth")}}
    rays = {"primary": cnt.rays_primary, "centre": cnt.rays_centre, "sample": cnt.rays_sample, "bounce": cnt.rays_bounce, "culled_pixels": cnt.pixels_culled}
    if not full:
        ctx.close()
        hs.close()
        return {"value": round(value, 2), "ms_per_step": round(ms_step, 4), "steps": steps, "warmup": warmup, "rays_per_frame": rays_frame,
                "config": scene_cfg, "rays": rays}
    tim = capi.rt_stats()
    capi.check(lib, ctx.handle, lib.rt_timing_collect(ctx.handle, C.byref(tim)), "rt_timing_collect")
    brk = capi.rt_stats()
    render(_p(0), brk)                                   # untimed: an event between every pair of launches
    torch.cuda.synchronize(dev)
    K_t = (steps + period - 1) // period
    launches = max(1, tim.launches_shadow)
    launches_per_frame = launches / K_t
    ms_shadow_frame = tim.ms_shadow / K_t
    avg_ms_shadow = tim.ms_shadow / launches
    cfg = f"{W}x{H} depth {D} {G * G} samples"
    sha = kernels_sha()
    flat = info["nodes"] == 1
    shaft = (not flat) and G * G > 32 and not os.environ.get("RT_NO_SHAFT") and not os.environ.get("RT_NO_CULL")

    # ---- executed work of this frame -> modelled VALU issue
    work = work_counters(pkg, hs, W, H, G, D) if want_work else None
    roof = {"bound": "valu", "kernel": "k_shadow (area-light sample shadow rays" + ("; shaft walk)" if shaft else ")"),
            "unit": "wave-instructions/SIMD/ns", "peak": VALU_PEAK_PER_SIMD_NS,
            "peak_source": "tools/micro/valu_rate.hip on MI355X: plain FP32 wave64 ops, 8 waves/SIMD (spec: 0.5/cycle = 1.2/ns at 2.4 GHz)"}
    if work:
        useful, total = valu_model(work, flat, shaft)
        t_ns = ms_shadow_frame * 1e6
        roof["achieved"] = round(total / t_ns / N_SIMDS, 4)
        roof["frac"] = round(total / t_ns / N_SIMDS / VALU_PEAK_PER_SIMD_NS, 4)
        roof["useful_frac"] = round(useful / t_ns / N_SIMDS / VALU_PEAK_PER_SIMD_NS, 4)
        roof["modelled_valu_wave_instructions_per_frame"] = {"useful": int(useful), "total": int(total)}
        roof["work"] = work
        roof["cost_per_step"] = COST
    else:
        roof.update({"achieved": None, "frac": None, "note": "no counting pass (--no-work-counters, or librt_mi355x_work.so missing: run __graft_entry__.build())"})
    ent, why = pmc_constant("valu.json", scene, cfg, sha)
    if ent:
        in_group = lambda k: "k_shadow" in k or "k_beam" in k or "k_pair_beam" in k          # every kernel the shadow interval of the events contains
        insts = sum(v["valu_wave_instructions"] for k, v in ent["kernels"].items() if in_group(k))
        r = insts / (ms_shadow_frame * 1e6) / N_SIMDS
        roof["executed_valu"] = {"constant": True, "wave_instructions_per_frame_level0": int(insts), "per_simd_per_ns": round(r, 4),
                                 "frac": round(r / VALU_PEAK_PER_SIMD_NS, 4), "source": ent["how"]}
        roof["executed_valu"].update(clock_independent(ent["kernels"], in_group))
    else:
        roof["executed_valu"] = {"constant": True, "frac": None, "why": why}
    ent, why = pmc_constant("traffic.json", scene, cfg, sha)
    if ent:
        roof["traffic"] = ent["hbm_bytes_per_launch"]
        # bytes of the heaviest (level-0) launch over the shadow time of the WHOLE frame (all levels): a lower bound of that launch's rate
        roof["hbm_frac"] = round(ent["hbm_bytes_per_launch"] / (ms_shadow_frame * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)
        roof["traffic_source"] = "constant (level-0 launch; divided by the frame's shadow time over all levels): " + ent["how"]
    else:
        roof["traffic"] = None
        roof["hbm_frac"] = None
        roof["traffic_source"] = why
    alg = BOX_BYTES * cnt.box_tests_shadow + TRI_REF_BYTES * cnt.leaf_tri_refs_shadow
    roof["reference_semantics_bytes"] = {"per_frame_k_shadow": int(alg), "GBs_over_launch_time": round(alg / (ms_shadow_frame * 1e-3) / 1e9, 1),
                                         "note": "SURVEY 8(d) algorithmic bytes (no early-out, no culling); a workload size, NOT a utilisation: above the HBM peak by construction"}
    roof["avg_launch_ms"] = round(avg_ms_shadow, 5)
    roof["launches_per_frame"] = launches_per_frame
    roof["group"] = "shadow"
    roof["timing_source"] = f"HIP events on the launch stream inside the timed region (every {period}th step: {K_t} of {steps} frames)"
    # ---- the shading kernel, same model: tiles of 64 hits x samples
    ms_shade_frame = tim.ms_shade / K_t
    tiles = (cnt.shaded_hits + 63) // 64
    sh_useful = tiles * G * G * COST["shade_sample"]
    sh_total = sh_useful + tiles * COST["shade_tile"]
    t_ns = max(ms_shade_frame, 1e-6) * 1e6
    shade = {"bound": "valu", "group": "shade", "kernel": "k_shade (phongShade over the samples: two normalisations and one libm-exact powf per sample)",
             "unit": "wave-instructions/SIMD/ns", "peak": VALU_PEAK_PER_SIMD_NS, "peak_source": roof["peak_source"],
             "achieved": round(sh_total / t_ns / N_SIMDS, 4), "frac": round(sh_total / t_ns / N_SIMDS / VALU_PEAK_PER_SIMD_NS, 4),
             "useful_frac": round(sh_useful / t_ns / N_SIMDS / VALU_PEAK_PER_SIMD_NS, 4),
             "modelled_valu_wave_instructions_per_frame": {"useful": int(sh_useful), "total": int(sh_total)},
             "work": {"shade": {"tiles_of_64_hits": int(tiles), "samples": G * G}}, "cost_per_step": COST,
             "traffic": None, "hbm_frac": None, "timing_source": roof["timing_source"] if "timing_source" in roof else ""}
    ent, why = pmc_constant("valu.json", scene, cfg, sha)
    if ent and any("k_shade" in k for k in ent["kernels"]):
        insts = sum(v["valu_wave_instructions"] for k, v in ent["kernels"].items() if "k_shade" in k)
        r = insts / t_ns / N_SIMDS
        shade["executed_valu"] = {"constant": True, "wave_instructions_per_frame_level0": int(insts), "per_simd_per_ns": round(r, 4),
                                  "frac": round(r / VALU_PEAK_PER_SIMD_NS, 4), "source": ent["how"]}
        shade["executed_valu"].update(clock_independent(ent["kernels"], lambda k: "k_shade" in k))
    else:
        shade["executed_valu"] = {"constant": True, "frac": None, "why": why or "no k_shade entry"}
    tent, twhy = pmc_constant("traffic.json", scene, cfg, sha)
    if tent and any("k_shade" in k for k in tent.get("kernels", {})):
        tb = sum(v["hbm_bytes"] for k, v in tent["kernels"].items() if "k_shade" in k)
        shade["traffic"] = int(tb)
        shade["hbm_frac"] = round(tb / (max(ms_shade_frame, 1e-6) * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)
        shade["traffic_source"] = "constant (level-0 launch of k_shade; divided by the frame's shade time over all levels): " + tent["how"]
    else:
        shade["traffic_source"] = twhy or "no k_shade entry in profiles/traffic.json"
    roof["ms_per_frame"] = {"trace": round(tim.ms_trace / K_t, 4), "shadow": round(ms_shadow_frame, 4), "shade": round(ms_shade_frame, 4), "device_total": round(tim.ms_total / K_t, 4),
                            "instrumented_frame": {"trace": round(brk.ms_trace, 4), "shadow": round(brk.ms_shadow, 4), "shade": round(brk.ms_shade, 4),
                                                   "resolve": round(brk.ms_resolve, 4), "total": round(brk.ms_total, 4)}}

    # ---- the trace group (closest hit + light-centre visibility + finish), same model
    ms_trace_frame = tim.ms_trace / K_t
    trace = {"bound": "valu", "group": "trace", "kernel": "k_trace (flat scenes) / k_stage x 3 + the leaf-task launches of the two traversal stages (tree scenes)",
             "unit": "wave-instructions/SIMD/ns", "peak": VALU_PEAK_PER_SIMD_NS, "peak_source": roof["peak_source"], "cost_per_step": COST,
             "traffic": None, "hbm_frac": None, "timing_source": roof["timing_source"]}
    if work:
        tr_useful, tr_total = trace_model(work, flat)
        t_ns = max(ms_trace_frame, 1e-6) * 1e6
        trace.update({"achieved": round(tr_total / t_ns / N_SIMDS, 4), "frac": round(tr_total / t_ns / N_SIMDS / VALU_PEAK_PER_SIMD_NS, 4),
                      "useful_frac": round(tr_useful / t_ns / N_SIMDS / VALU_PEAK_PER_SIMD_NS, 4),
                      "modelled_valu_wave_instructions_per_frame": {"useful": int(tr_useful), "total": int(tr_total)}, "work": {"trace": work["trace"]}})
    else:
        trace.update({"achieved": None, "frac": None})
    ent, why = pmc_constant("valu.json", scene, cfg, sha)
    if ent:
        sel = lambda k: "k_trace" in k or "k_stage" in k       # noqa: E731
        insts = sum(v["valu_wave_instructions"] for k, v in ent["kernels"].items() if sel(k))
        r = insts / (max(ms_trace_frame, 1e-6) * 1e6) / N_SIMDS
        trace["executed_valu"] = {"constant": True, "wave_instructions_per_frame_level0": int(insts), "per_simd_per_ns": round(r, 4),
                                  "frac": round(r / VALU_PEAK_PER_SIMD_NS, 4), "source": ent["how"]}
        trace["executed_valu"].update(clock_independent(ent["kernels"], sel))
    else:
        trace["executed_valu"] = {"constant": True, "frac": None, "why": why}
    if tent and any(("k_trace" in k or "k_stage" in k) for k in tent.get("kernels", {})):
        tb = sum(v["hbm_bytes"] for k, v in tent["kernels"].items() if "k_trace" in k or "k_stage" in k)
        trace["traffic"] = int(tb)
        trace["hbm_frac"] = round(tb / (max(ms_trace_frame, 1e-6) * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)
        trace["traffic_source"] = "constant (heaviest launch of every trace kernel; divided by the frame's trace time over all levels): " + tent["how"]
    else:
        trace["traffic_source"] = twhy or "no trace kernels in profiles/traffic.json"
    # rays actually FORMED and walked: the frame's queries minus the sample segments whole tiles (k_beam) or whole (hit, light) units were proven
    # unblocked for before a ray existed.  `value` counts queries resolved; this is the traversal count behind it.
    rays_walked = int(cnt.rays_primary + cnt.rays_bounce + cnt.rays_centre + brk.rays_sample_walked)      # (brk: the instrumented frame of the shipped kernels)

    rec = {"value": round(value, 2), "ms_per_step": round(ms_step, 4), "steps": steps, "warmup": warmup, "rays_per_frame": rays_frame,
           "rays_walked_per_frame": rays_walked, "Mrays_walked_per_s": round(rays_walked * steps / elapsed / 1e6, 2), "launches_per_frame": int(brk.launches_total),
           "config": scene_cfg,
           "rays": rays,
           "roofline": roof}
    shade["ms_per_frame"] = roof["ms_per_frame"]
    shade["timing_source"] = roof["timing_source"]
    trace["ms_per_frame"] = roof["ms_per_frame"]
    rec["roofline_trace"] = trace
    # `roofline` is the group that takes most of the frame; the other one stays beside it
    if ms_shade_frame > ms_shadow_frame:
        rec["roofline"], rec["roofline_shadow"] = shade, roof
    else:
        rec["roofline_shade"] = shade

    if want_graph:
        # extra (untimed for `value`): K frames replayed from ONE captured hipGraph, camera yaw stepping 2*pi/120 per frame (BASELINE cfg5)
        try:
            g = pkg.FrameGraph(ctx, L, _p(0), out_rgb.data_ptr(), out_u8.data_ptr())
            cams = [pkg.default_camera(W, H, float(np.float32(2.0 * np.pi * f / 120.0))) for f in range(min(steps, 120))]
            g.launch(cams[0], stream.cuda_stream)
            torch.cuda.synchronize(dev)
            tg0 = time.perf_counter()
            for cm in cams:
                g.launch(cm, stream.cuda_stream)
            torch.cuda.synchronize(dev)
            rec["graph_replay_ms_per_frame_yaw_path"] = round((time.perf_counter() - tg0) / len(cams) * 1e3, 4)
            tg0 = time.perf_counter()
            for _ in cams:
                g.launch(cam, stream.cuda_stream)
            torch.cuda.synchronize(dev)
            rec["graph_replay_ms_per_frame_same_camera"] = round((time.perf_counter() - tg0) / len(cams) * 1e3, 4)
            rec["graph_replay_note"] = ("yaw path = BASELINE cfg5's camera (2 pi / 120 per frame about the camera's own centre): the object is in view on roughly a fifth of the "
                                        "frames and the others render background only, so its mean is NOT comparable with ms_per_step; same_camera replays the headline view")
            g.close()
        except Exception as e:            # noqa: BLE001 -- the graph path is an extra; never let it take the bench line down
            rec["graph_replay_ms_per_frame_yaw_path"] = f"failed: {e}"

    if want_cpu:
        # CPU baseline beside it: the oracle (a port of the reference's algorithm) on this host's cores, bounded sample of the same workload
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib
        orc = oracle_lib.load()
        osc = orc.load_scene(scene_path)
        threads = max(1, min(16, os.cpu_count() or 2) - 1)     # the reference uses hardware_concurrency()-1 (flyscene.cpp:558); a 1-GPU box's share is 16 cores
        stride = cpu_stride or (8 if scene == "wavy" else (2 if scene == "dodge" else 1))
        n = 0; sec = 0.0; cpu_rays = 0; reps = 0
        while reps == 0 or (sec * threads < 10.0 and reps < 64):
            n1, s1, ost = osc.render_subsample(orc.camera(W, H), orc.lights(area=True, usteps=G, vsteps=G), W, H, stride, max_depth=D, threads=threads)
            n += n1; sec += s1; cpu_rays += ost.total_rays(); reps += 1
        rec["cpu_baseline"] = {
            "value": round(cpu_rays / sec / 1e6, 3), "unit": "Mrays/s", "cores": threads, "kind": "port",
            "sample": f"{reps} x every {stride}th pixel in x and y of the same {W}x{H} frame ({n} pixels, {cpu_rays} rays) in {sec:.2f} s on {threads} threads "
                      f"= {sec * threads:.0f} s of CPU work; oracle/rt_oracle.c (C restatement, no per-node deep copies) -- NOT the unmodified reference, "
                      "which measured 0.165-2.6 Mrays/s on 7 threads (BASELINE.md)",
            "seconds": round(sec, 3)}
        rec["speedup_vs_cpu_port"] = round(value / (cpu_rays / sec / 1e6), 1)
        # the UNMODIFIED reference as the survey session measured it (another host -- 8-vCPU Xeon, 7 threads, -O2 -- at its own 25 samples on the
        # 1440 x 1440 twin of this pixel count); it cannot be built here without a GL stand-in, so this ratio crosses hosts and sample counts and is quoted as such
        ref_measured = {"cube": 2.6, "dodge": 0.165}.get(scene)
        rec["cpu_baseline"]["ratios"] = {
            "vs_port_same_host": {"value": rec["speedup_vs_cpu_port"], "cpu": f"oracle port, {threads} threads, this host"},
            "vs_reference_as_surveyed": ({"value": round(value / ref_measured, 1), "cpu_Mrays_per_s": ref_measured,
                                          "cpu": "unmodified reference, 7 threads of an 8-vCPU Xeon 2.1 GHz (BASELINE.md section 2), 1440x1440, 25 samples -- another host, another sample count"}
                                         if ref_measured else None)}
        osc.close()
    ctx.close()
    hs.close()
    return rec


class HostGatherComm:
    """Stand-in for rt_comm in the gloo rehearsal of `bench.py --gpus N` on a one-GPU box: the same call shape as shard.Comm.gather_rows,
    the exchange itself through host copies and torch.distributed.gather.  Only the exchange is replaced: buffers, events and the two-stream
    pipeline of step_comm run as on the real path (the host copy waits for the gather stream, so render i + 1 does not overlap gather i)."""

    def __init__(self, torch, dist, rank, world):
        self.torch, self.dist, self.rank, self.world = torch, dist, rank, world

    def gather_rows(self, d_local_ptr, nbytes, d_gathered_ptr, root=0, stream_ptr=None, local=None, gathered=None, stream=None):
        torch = self.torch
        with torch.cuda.stream(stream):
            src = local.cpu()                                   # (waits for everything queued on the gather stream, i.e. the `rendered` event)
        bufs = [torch.empty_like(src) for _ in range(self.world)] if self.rank == root else None
        self.dist.gather(src, gather_list=bufs, dst=root)
        if self.rank == root:
            with torch.cuda.stream(stream):
                gathered.copy_(torch.cat(bufs), non_blocking=False)

    def close(self):
        pass


def run_multi(pkg, torch, dist, dev, rank, world, backend, args, outputs=None):
    """N > 1: every rank renders its interleaved row stripes; the step is a hipGraph replay of the frame + ONE gather of the 8-bit rows to
    rank 0 through the library's own RCCL binding (rt_comm_gather_rows), double buffered so that render i+1 overlaps gather i."""
    import numpy as np
    capi = pkg.capi
    on_host = backend != "nccl"
    scene_file, scene_path = scene_of(args.scene)
    W, H, G, D, S = args.width, args.height, args.grid, args.depth, args.stripe
    hs = pkg.HostScene(scene_path, 1000, 15)
    ctx = pkg.Context(dev.index)
    ctx.upload(hs)
    lib = ctx.lib
    cam = pkg.default_camera(W, H)
    L = pkg.make_lights(area=True, usteps=G, vsteps=G)
    max_rows = pkg.shard.max_local_rows(H, S, world)
    block = max_rows * W * 3
    out_rgb = torch.zeros(block, dtype=torch.float32, device=dev)
    u8 = [torch.zeros(block, dtype=torch.uint8, device=dev) for _ in range(2)]
    gathered = [torch.zeros(block * world, dtype=torch.uint8, device=dev) if rank == 0 else None for _ in range(2)]
    stream = torch.cuda.current_stream(dev)

    def _p(collect):
        p = pkg.make_params(W, H, D, 0, H, S, rank, world)
        p.collect_stats = collect
        return p

    def reduce_(t, op):
        if on_host:
            c = t.cpu(); dist.all_reduce(c, op=op); t.copy_(c)
        else:
            dist.all_reduce(t, op=op)

    def render_eager(buf, p, stats=None):
        st = lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(out_rgb.data_ptr()), C.c_void_p(buf.data_ptr()), None,
                                  C.c_void_p(stream.cuda_stream), C.byref(stats) if stats is not None else None)
        capi.check(lib, ctx.handle, st, "rt_render_device")

    cnt = capi.rt_stats()
    render_eager(u8[0], _p(1 if args.full else 0), cnt)
    torch.cuda.synchronize(dev)
    counters = torch.tensor([cnt.total_rays(), cnt.rays_primary, cnt.rays_centre, cnt.rays_sample, cnt.rays_bounce, cnt.pixels_culled], dtype=torch.float64, device=dev)
    reduce_(counters, dist.ReduceOp.SUM)
    tot = [int(x) for x in counters.tolist()]

    # ---- the library's own communicator (RCCL, one per process/GPU); the unique id travels over torch.distributed.
    # Every rank issues the SAME collectives whatever fails locally: rank 0 makes the id in a try block of its own and always takes part in
    # the broadcast (an `ok` byte rides along); the communicator is then built in a second try block and one all_reduce settles the path.
    # (Mismatched NCCL collectives -- rank 0 skipping the broadcast after a failed rt_comm_unique_id -- hang instead of failing.)
    comm, step_kind = None, None
    if on_host and not args.eager:
        comm = HostGatherComm(torch, dist, rank, world)          # gloo rehearsal: the pipelined step with a host-side stand-in for the exchange ONLY
    elif not args.eager:
        idt = torch.zeros(capi.RT_COMM_ID_BYTES + 1, dtype=torch.uint8, device=dev)
        if rank == 0:
            try:
                raw = bytearray(pkg.shard.Comm.unique_id()) + bytearray([1])
                idt.copy_(torch.frombuffer(raw, dtype=torch.uint8))
            except Exception as e:            # noqa: BLE001
                print(f"[bench] rt_comm_unique_id failed on rank 0: {e}; every rank falls back to torch.distributed.gather", file=sys.stderr)
        dist.broadcast(idt, src=0)
        raw = bytes(idt.cpu().numpy().tobytes())
        if raw[-1] == 1:
            try:
                comm = pkg.shard.Comm(dev.index, raw[:-1], world, rank)
            except Exception as e:            # noqa: BLE001
                print(f"[bench] rt_comm_create failed on rank {rank}: {e}; falling back to torch.distributed.gather", file=sys.stderr)
                comm = None
    flag = torch.tensor([1.0 if comm else 0.0], dtype=torch.float64, device=dev)
    reduce_(flag, dist.ReduceOp.MIN)                    # every rank must take the same path
    if flag.item() < 0.5 and comm:
        comm.close(); comm = None

    graphs = None
    if comm:
        try:
            graphs = [pkg.FrameGraph(ctx, L, _p(0), out_rgb.data_ptr(), u8[i].data_ptr()) for i in range(2)]
        except Exception as e:            # noqa: BLE001
            print(f"[bench] graph capture failed on rank {rank}: {e}; eager launches", file=sys.stderr)
            graphs = None
    gstream = torch.cuda.Stream(device=dev) if comm else None
    rendered = [torch.cuda.Event() for _ in range(2)]
    gathered_ev = [torch.cuda.Event() for _ in range(2)]

    def step_comm(i):
        b = i & 1
        if i >= 2:
            stream.wait_event(gathered_ev[b])            # buffer b was read by gather i-2
        if graphs:
            graphs[b].launch(cam, stream.cuda_stream)
        else:
            render_eager(u8[b], _p(0))
        rendered[b].record(stream)
        gstream.wait_event(rendered[b])
        if isinstance(comm, HostGatherComm):
            comm.gather_rows(0, block, 0, 0, None, local=u8[b], gathered=gathered[b], stream=gstream)
        else:
            comm.gather_rows(u8[b].data_ptr(), block, gathered[b].data_ptr() if rank == 0 else 0, 0, gstream.cuda_stream)
        gathered_ev[b].record(gstream)

    last_bufs = []

    def step_torch(i):
        render_eager(u8[0], _p(0))
        src = u8[0].cpu() if on_host else u8[0]
        bufs = [torch.empty_like(src) for _ in range(world)] if rank == 0 else None
        dist.gather(src, gather_list=bufs, dst=0)
        last_bufs[:] = bufs or []

    step = step_comm if comm else step_torch
    exchange = "a HOST-side stand-in for the exchange (gloo rehearsal)" if isinstance(comm, HostGatherComm) else "rt_comm_gather_rows (RCCL via the C ABI)"
    step_kind = ("hipGraph replay" if graphs else "eager launches") + f" + {exchange}, double buffered" if comm \
        else "eager launches + torch.distributed.gather"
    for i in range(max(4, args.warmup)):
        step(i)
    torch.cuda.synchronize(dev)
    dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    torch.cuda.synchronize(dev)
    dist.barrier()
    t1 = time.perf_counter()
    el = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    reduce_(el, dist.ReduceOp.MAX)
    elapsed = float(el.item())
    if outputs is not None and rank == 0:
        blocks = gathered[(args.steps - 1) & 1] if comm else torch.cat(last_bufs)
        outputs["frame_u8"] = pkg.shard.stitch_u8(blocks.cpu().numpy(), block, W, H, S, world)
    K = args.steps
    rec = {"value": round(tot[0] * K / elapsed / 1e6, 2), "ms_per_step": round(elapsed / K * 1e3, 4), "steps": K, "warmup": args.warmup, "rays_per_frame": tot[0],
           "config": {"workload": f"{W}x{H} depth {D} {G * G}-sample area light, {scene_file}, 1 light, row stripes of {S} over {world} GPU(s)",
                      "width": W, "height": H, "max_depth": D, "samples": G * G, "scene": scene_file, "parallelism": f"rows{world}", "step": step_kind},
           "rays": {"primary": tot[1], "centre": tot[2], "sample": tot[3], "bounce": tot[4], "culled_pixels": tot[5]}}
    if not args.full:
        if comm:
            comm.close()
        return rec if rank == 0 else None
    # untimed: one instrumented eager frame for the per-kernel breakdown of rank 0's rows
    brk = capi.rt_stats()
    render_eager(u8[0], _p(0), brk)
    torch.cuda.synchronize(dev)
    # ---- what every rank did: device ms of its share of the frame (one instrumented eager frame) and launches per frame
    mine = torch.tensor([brk.ms_total, float(brk.launches_total)], dtype=torch.float64, device=dev)
    every = [torch.zeros_like(mine) for _ in range(world)]
    if on_host:
        hc = [torch.zeros(2, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(hc, mine.cpu())
        every = hc
    else:
        dist.all_gather(every, mine)
    per_rank = [{"rank": r, "device_ms_per_frame": round(float(e[0]), 4), "launches_per_frame": int(e[1])} for r, e in enumerate(every)]
    # ---- the stitched frame of the last timed step against ONE ungathered render of the whole frame on rank 0
    check = None
    if rank == 0 and comm:
        full = pkg.shard.stitch_u8(gathered[(args.steps - 1) & 1].cpu().numpy(), block, W, H, S, world)
        whole = torch.zeros(H * W * 3, dtype=torch.uint8, device=dev)
        whole_rgb = torch.zeros(H * W * 3, dtype=torch.float32, device=dev)
        pw = pkg.make_params(W, H, D, 0, H, S, 0, 1)
        st = lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(pw), C.c_void_p(whole_rgb.data_ptr()), C.c_void_p(whole.data_ptr()), None,
                                  C.c_void_p(stream.cuda_stream), None)
        capi.check(lib, ctx.handle, st, "rt_render_device (whole frame)")
        torch.cuda.synchronize(dev)
        want = whole.cpu().numpy().reshape(full.shape)
        same = bool(np.array_equal(full, want))
        check = {"assembled_frame_sha256": hashlib.sha256(full.tobytes()).hexdigest(), "ungathered_frame_sha256": hashlib.sha256(want.tobytes()).hexdigest(),
                 "match": same, "nonzero": bool(full.any())}
        if not same:
            check["error"] = f"{int((full != want).sum())} bytes of the stitched frame differ from the plain render of the whole frame"
    if comm:
        comm.close()
    if rank != 0:
        return None
    rec.update({
            "gathered_frame": check, "per_rank": per_rank,
            "roofline": {"bound": "valu", "kernel": "k_shadow", "achieved": None, "peak": VALU_PEAK_PER_SIMD_NS, "unit": "wave-instructions/SIMD/ns", "frac": None,
                         "traffic": None, "note": "the executed-work roofline is reported by the N = 1 run (same kernels, 1/N of the rows per rank)",
                         "timing_source": "one instrumented eager frame of rank 0 outside the timed region (HIP events)",
                         "ms_per_frame": {"instrumented_frame_rank0": {"trace": round(brk.ms_trace, 4), "shadow": round(brk.ms_shadow, 4),
                                                                       "shade": round(brk.ms_shade, 4), "resolve": round(brk.ms_resolve, 4), "total": round(brk.ms_total, 4)}}}})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scene", default="cube", choices=["cube", "dodge", "wavy"],
                    help="wavy = the ~1M-triangle synthetic mesh of BASELINE cfg4 (use with --width 3840 --height 2160 --grid 16 --depth 8)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--grid", type=int, default=8, help="area-light grid side (8 -> 64 samples)")
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--stripe", type=int, default=8)
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the frames of the last timed step as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--full", action="store_true", help="also measure and check everything beside the headline: per-kernel times, roofline, "
                    "PMC constants, graph replay, CPU baseline, tree scenes (N = 1, default scene), the assembled-frame check (N > 1)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-tree-scenes", action="store_true", help="--full, N = 1: skip the dodge / cfg4 sub-records")
    ap.add_argument("--no-work-counters", action="store_true", help="--full: skip the counting-build pass (PMC / rocprof runs: its launches carry the same kernel names)")
    ap.add_argument("--eager", action="store_true", help="N > 1: eager launches + torch.distributed.gather instead of graph replay + rt_comm gather")
    ap.add_argument("--cpu-stride", type=int, default=0, help="oracle pixel stride for the CPU baseline (0 = auto)")
    ap.add_argument("--force-multi", action="store_true", help="N = 1: run the N > 1 step (graph replay + rt_comm gather over a one-rank RCCL communicator, "
                    "double buffered) instead of the single-GPU loop -- the rehearsal of the multi-GPU code path on one GPU")
    args = ap.parse_args()

    import torch
    import rtpkg
    pkg = rtpkg.load()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world == 1 and args.gpus > 1:
        raise SystemExit("bench.py --gpus N>1 must be launched with torch.distributed.run (one rank per GPU)")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the ray-trace path has no CPU fallback")
    # RT_DIST_BACKEND=gloo rehearses the N > 1 path on a ONE-GPU box: every rank renders its stripes on GPU 0 and the
    # gather runs over gloo on host copies.  The real path (default) is one rank per GPU with RCCL.
    backend = os.environ.get("RT_DIST_BACKEND", "nccl")
    gpu_index = local_rank if backend == "nccl" else local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(gpu_index)
    dev = torch.device("cuda", gpu_index)

    base = {"metric": "Mrays/s", "unit": "Mrays/s", "n_gpus": world, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic"}
    if world == 1 and not args.force_multi:
        default_call = args.scene == "cube" and (args.width, args.height, args.grid, args.depth) == (1920, 1080, 8, 4)
        outputs = {} if args.dump_outputs else None
        rec = run_single(pkg, torch, dev, args.scene, args.width, args.height, args.grid, args.depth, args.stripe, args.steps, args.warmup,
                         not args.no_cpu_baseline, args.cpu_stride, True, not args.no_work_counters, args.full, outputs)
        if outputs is not None:
            dump_outputs(args.dump_outputs, outputs)
        out = dict(base)
        out.update(rec)
        if args.full and default_call and not args.no_tree_scenes:
            # the octree traversal the north star is about is NOT in the cube headline (1-node tree): time it here, same invocation
            out["tree_scenes"] = {
                "dodge_1920x1080_d4_s64": run_single(pkg, torch, dev, "dodge", 1920, 1080, 8, 4, args.stripe, min(args.steps, 100), min(args.warmup, 5),
                                                     not args.no_cpu_baseline, 0, False),
                "cfg4_wavy_3840x2160_d8_s256": run_single(pkg, torch, dev, "wavy", 3840, 2160, 16, 8, args.stripe, 5, 2, not args.no_cpu_baseline, 0, False)}
        print(json.dumps(out), flush=True)
        return

    # RCCL prints a version banner on file descriptor 1 when its communicator comes up (NCCL_DEBUG=VERSION in this image): everything the
    # libraries write to stdout goes to stderr from here on, and the ONE JSON line is written to the real stdout at the end
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    def emit(line):
        os.write(real_stdout, (line + "\n").encode())

    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    if backend == "nccl":
        dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    outputs = {} if args.dump_outputs and rank == 0 else None
    rec = run_multi(pkg, torch, dist, dev, rank, world, backend, args, outputs)
    bad = False
    if outputs is not None:
        dump_outputs(args.dump_outputs, outputs)
    if rank == 0:
        out = dict(base)
        out.update(rec)
        emit(json.dumps(out))
        gf = rec.get("gathered_frame")
        bad = bool(gf) and not gf.get("match", True)
    dist.destroy_process_group()
    if bad:
        raise SystemExit("bench.py: the frame stitched from the gathered rows differs from the plain render of the whole frame")


if __name__ == "__main__":
    main()
