"""The one-bounce diffuse gather beside the ambient-occlusion call on the same points (GPU only).

Per scene the points are those of the default 1920 x 1080 camera: the pinhole rays of every pixel (rt_primary_points), their closest hits
and hit points, built on the device; a pixel whose ray hits nothing stays in the batch as a "no point", as in Flyscene.indirect_diffuse.  One
point light at (-1, 1, 1), grids m = 2 and m = 4 (K = 4 and 16 gather rays per point); in one process, alternating, from torch events on
one stream after warm-up, --blocks blocks of --reps repetitions per side:
  (a) rt_closest_hits_device -> rt_hit_points_device -> rt_indirect_diffuse_device, the chain of the Flyscene member;
  (b) rt_indirect_diffuse_device alone on the hit points;
  (c) rt_ambient_occlusion_device alone on the same points, same m and seed, radius 0.5: the yardstick.  An occlusion segment stops at its
      first blocker and is half a unit long; a gather ray is unbounded, needs its closest hit, and every hit walks a segment per light.
A side's figure is the median of its block medians, its spread their range.  There is no earlier route to compare with.

Every scene runs in a child process of its own under a time limit (--limit seconds); the first child that fails or runs out of time ends
the run with its status.

    python tools/indirect_timing.py [--scenes cube,dodge] [--size 1920 1080] [--reps 20] [--blocks 3] [--limit 300] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj"}
GRIDS = (2, 4)
LIGHT, SEED, RADIUS = (-1.0, 1.0, 1.0), 7, 0.5


def scene_step(args, scene):
    import numpy as np
    import torch
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    W, H = args.size
    hs = pkg.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", SCENES[scene]), 1000, 15)
    ctx = pkg.Context(0)
    ctx.upload(hs)
    lib = ctx.lib
    cam = pkg.default_camera(W, H)
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    n = W * H

    pts = np.empty((n, 3), np.float32)
    capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(cam), W, H, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
    centre = torch.tensor(list(cam.center), dtype=torch.float32, device=dev)
    dirs = (torch.from_numpy(pts).to(dev) - centre).contiguous()
    origins = centre.expand(n, 3).contiguous()
    L = pkg.make_lights(points=(LIGHT,), area=False)
    with torch.cuda.stream(stream):
        faces, ts = ctx.closest_hits(origins, dirs)
        P, N = ctx.hit_points(origins, dirs, faces, ts)
        rgb = ctx.indirect_diffuse(P, N, L, GRIDS[0], seed=SEED)         # (also the first AO-family call: the tables are uploaded here)
    stream.synchronize()
    hits = int((faces >= 0).sum().item())
    ao = torch.empty(n, dtype=torch.float32, device=dev)

    def events(call, reps):
        """ms of each of `reps` repetitions of call() on the stream, after three warm ones"""
        with torch.cuda.stream(stream):
            for _ in range(3):
                call()
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
            marks[0].record(stream)
            for k in range(reps):
                call()
                marks[k + 1].record(stream)
        marks[-1].synchronize()
        return [marks[k].elapsed_time(marks[k + 1]) for k in range(reps)]

    rec = {"scene": scene, "size": [W, H], "points": n, "hits": hits, "light": list(LIGHT), "seed": SEED, "ao_radius": RADIUS, "reps": args.reps,
           "blocks": args.blocks, "cases": {}}
    for m in GRIDS:
        K = m * m

        def gather():
            capi.check(lib, ctx.handle, lib.rt_indirect_diffuse_device(ctx.handle, C.byref(L), n, P.data_ptr(), N.data_ptr(), m, SEED, rgb.data_ptr(), sp),
                       "rt_indirect_diffuse_device")

        def side_a():
            capi.check(lib, ctx.handle, lib.rt_closest_hits_device(ctx.handle, n, origins.data_ptr(), dirs.data_ptr(), faces.data_ptr(), ts.data_ptr(), sp),
                       "rt_closest_hits_device")
            capi.check(lib, ctx.handle, lib.rt_hit_points_device(ctx.handle, n, origins.data_ptr(), dirs.data_ptr(), faces.data_ptr(), ts.data_ptr(),
                                                                 P.data_ptr(), N.data_ptr(), sp), "rt_hit_points_device")
            gather()

        def side_c():
            capi.check(lib, ctx.handle, lib.rt_ambient_occlusion_device(ctx.handle, n, P.data_ptr(), N.data_ptr(), m, RADIUS, SEED, None, ao.data_ptr(), sp),
                       "rt_ambient_occlusion_device")

        sides = {"a_hits_points_gather": side_a, "b_gather": gather, "c_ambient_occlusion": side_c}
        medians = {k: [] for k in sides}
        for _ in range(args.blocks):
            for k, call in sides.items():
                medians[k].append(statistics.median(events(call, args.reps)))
        stream.synchronize()
        lit = rgb.max(dim=1).values > 0
        case = {"m": m, "K": K, "gather_rays": hits * K, "points_with_indirect_light": int(lit.sum().item()),
                "mean_rgb_over_hits": [round(float(x), 6) for x in (rgb.to(torch.float64).sum(dim=0) / max(hits, 1)).tolist()],
                "ao_mean_over_hits": round(float(ao[faces >= 0].to(torch.float64).mean().item()), 6)}
        for k, v in medians.items():
            med = statistics.median(v)
            case[k] = {"ms_block_medians": [round(x, 4) for x in v], "ms_median": round(med, 4), "ms_range": round(max(v) - min(v), 4),
                       "rays_per_s": round(hits * K / (med * 1e-3))}
        case["gather_over_ao"] = round(case["b_gather"]["ms_median"] / case["c_ambient_occlusion"]["ms_median"], 3)
        rec["cases"][str(m)] = case
    ctx.close()
    hs.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cube,dodge")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--step", help="(internal) run one scene in this process")
    args = ap.parse_args()
    if args.step:
        scene_step(args, args.step)
        return 0
    records = []
    for scene in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", scene, "--size", str(args.size[0]), str(args.size[1]), "--reps", str(args.reps),
               "--blocks", str(args.blocks)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"indirect_timing: {scene} ran out of its {args.limit} s; stopping", file=sys.stderr)
            return 124
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print(f"indirect_timing: {scene} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        records.append(json.loads(line))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
