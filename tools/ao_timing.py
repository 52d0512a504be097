"""Ambient occlusion in one call against what the device ray queries offered before it (GPU only).

Per scene the points are the closest hits of the default 1920 x 1080 camera, built once on the device (rt_primary_points, closest hits, hit
points, the hits kept).  For m = 4, 6, 8 (K = 16, 36, 64 directions), radius 0.5, in one process, alternating, from torch events on one
stream after warm-up, --blocks blocks of --reps repetitions per side:
  (a) rt_ambient_occlusion_device;
  (b) rt_light_strikes_device alone on the n * K segments, pre-built in device memory by torch with the float32 operations of the
      definition, one rounding each (the one division of the frame is done on the host: torch's device division is not promised to round
      correctly);
  (c) route (b) including the torch segment build and the reduction of the n * K bytes to n counts.
The counts of (a) and (b) must be equal.  A side's figure is the median of its block medians, its spread their range.

Every scene runs in a child process of its own under a time limit (--limit seconds); the first child that fails or runs out of time ends
the run with its status.

    python tools/ao_timing.py [--scenes cube,dodge] [--size 1920 1080] [--reps 20] [--blocks 3] [--limit 300] [--out FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj"}
GRIDS = (4, 6, 8)
RADIUS, SEED = 0.5, 7


def rotation_steps(np, seed, n):
    """r of rt_ao_rotation(seed, i) for i = 0 .. n - 1 (uint32 arithmetic carried in uint64)"""
    m = np.uint64(0xFFFFFFFF)
    h = ((np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1)) & m) ^ np.uint64((seed * 0x85EBCA6B) & 0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m
    h ^= h >> np.uint64(15)
    return (h >> np.uint64(26)).astype(np.int64)


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
    sp = stream.cuda_stream

    pts = np.empty((W * H, 3), np.float32)
    capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(cam), W, H, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
    centre = torch.tensor(list(cam.center), dtype=torch.float32, device=dev)
    dirs = (torch.from_numpy(pts).to(dev) - centre).contiguous()
    origins = centre.expand(W * H, 3).contiguous()
    with torch.cuda.stream(stream):
        faces, ts = ctx.closest_hits(origins, dirs)
        allP, allN = ctx.hit_points(origins, dirs, faces, ts)
        hit = faces >= 0
        P, N = allP[hit].contiguous(), allN[hit].contiguous()
    stream.synchronize()
    n = int(P.shape[0])

    # the per-point inputs of the torch segment build: (c, s) of the point's rotation and the frame's one division, from the host
    cs = np.array([[math.cos((math.pi / 2.0) * r / 64), math.sin((math.pi / 2.0) * r / 64)] for r in range(64)]).astype(np.float32)
    cs = torch.from_numpy(cs[rotation_steps(np, SEED, n)]).to(dev)
    Nh = N.cpu().numpy()
    sg_h = np.copysign(np.float32(1.0), Nh[:, 2])
    a_dev = torch.from_numpy((np.float32(-1.0) / (sg_h + Nh[:, 2])).astype(np.float32)).to(dev)

    def build(m):
        """-> (hit, light) float32 (n * K, 3): the segments of the definition, one torch operation per float32 operation"""
        d = np.empty((m * m, 3), np.float32)
        capi.check(lib, None, lib.rt_ao_directions(m, d.ctypes.data_as(C.POINTER(C.c_float))), "rt_ao_directions")
        D = torch.from_numpy(d).to(dev)
        x, y, z = D[None, :, 0], D[None, :, 1], D[None, :, 2]
        nx, ny, nz = N[:, 0:1], N[:, 1:2], N[:, 2:3]
        sg = torch.copysign(torch.ones_like(nz), nz)
        a = a_dev[:, None]
        b = (nx * ny) * a
        T = (1.0 + (sg * (nx * nx)) * a, sg * b, -(sg * nx))
        B = (b, sg + (ny * ny) * a, -ny)
        c, s = cs[:, 0:1], cs[:, 1:2]
        xr = c * x - s * y
        yr = s * x + c * y
        Q = torch.stack([P[:, q:q + 1] + RADIUS * (((xr * T[q]) + (yr * B[q])) + (z * (nx, ny, nz)[q])) for q in range(3)], dim=-1)
        return P[:, None, :].expand(n, m * m, 3).reshape(-1, 3).contiguous(), Q.reshape(-1, 3).contiguous()

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

    rec = {"scene": scene, "size": [W, H], "points": n, "radius": RADIUS, "seed": SEED, "reps": args.reps, "blocks": args.blocks, "grids": {}}
    for m in GRIDS:
        K = m * m
        with torch.cuda.stream(stream):
            hitp, light = build(m)
            opn, _ = ctx.ambient_occlusion(P, N, m, RADIUS, seed=SEED, want_ao=False)
            vis = ctx.light_strikes_device(hitp, light)
            by_strikes = vis.view(n, K).sum(dim=1, dtype=torch.int32)
        stream.synchronize()
        mismatches = int((opn.to(torch.int32) != by_strikes).sum().item())
        vis_buf = torch.empty(n * K, dtype=torch.uint8, device=dev)
        open_buf = torch.empty(n, dtype=torch.uint16, device=dev)

        def side_a():
            capi.check(lib, ctx.handle, lib.rt_ambient_occlusion_device(ctx.handle, n, P.data_ptr(), N.data_ptr(), m, RADIUS, SEED, open_buf.data_ptr(), None,
                                                                        C.c_void_p(sp)), "rt_ambient_occlusion_device")

        def side_b():
            capi.check(lib, ctx.handle, lib.rt_light_strikes_device(ctx.handle, n * K, hitp.data_ptr(), light.data_ptr(), vis_buf.data_ptr(), C.c_void_p(sp)),
                       "rt_light_strikes_device")

        def side_c():
            h2, l2 = build(m)
            capi.check(lib, ctx.handle, lib.rt_light_strikes_device(ctx.handle, n * K, h2.data_ptr(), l2.data_ptr(), vis_buf.data_ptr(), C.c_void_p(sp)),
                       "rt_light_strikes_device")
            return vis_buf.view(n, K).sum(dim=1, dtype=torch.int32)

        sides = {"a_ambient_occlusion": side_a, "b_light_strikes_prebuilt": side_b, "c_build_strikes_reduce": side_c}
        medians = {k: [] for k in sides}
        for _ in range(args.blocks):
            for k, call in sides.items():
                medians[k].append(statistics.median(events(call, args.reps)))
        g = {"K": K, "segments": n * K, "counts_equal": mismatches == 0, "mismatching_points": mismatches,
             "open_share": round(float(opn.to(torch.float64).mean().item()) / K, 6)}
        for k, v in medians.items():
            med = statistics.median(v)
            g[k] = {"ms_block_medians": [round(x, 4) for x in v], "ms_median": round(med, 4), "ms_range": round(max(v) - min(v), 4),
                    "segments_per_s": round(n * K / (med * 1e-3))}
        g["a_not_above_b_plus_range"] = g["a_ambient_occlusion"]["ms_median"] <= g["b_light_strikes_prebuilt"]["ms_median"] + g["b_light_strikes_prebuilt"]["ms_range"]
        rec["grids"][str(m)] = g
        del hitp, light, vis, vis_buf
        torch.cuda.empty_cache()
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
            print(f"ao_timing: {scene} ran out of its {args.limit} s; stopping", file=sys.stderr)
            return 124
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print(f"ao_timing: {scene} failed with status {r.returncode}; stopping", file=sys.stderr)
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
