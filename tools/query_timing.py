"""Throughput of the device ray queries on the rays of a pinhole frame (GPU only).

Per scene, the 1920 x 1080 primary rays of the default camera are built once in device memory (rt_primary_points for the screen points, the
directions screen - centre on the device).  Then, in rays/s from device events (torch events on one stream) around every one of --reps warm
repetitions: rt_closest_hits_device; rt_light_strikes_device on the segments from the hit points to the default light; rt_trace_rays_device at
depth 0 and 4 with an 8 x 8 area light, at the default chunk and over the chunk sweep (--blocks alternating blocks of --reps per setting:
the spread of a setting is the range of its block medians); beside it rt_trace_rays on host pointers (wall clock: it copies and
synchronises) and the rt_render_device frame of the same view.

Every scene runs in a child process of its own under a time limit (--limit seconds); the first child that fails or runs out of time ends
the run with its status.

    python tools/query_timing.py [--scenes cube,dodge] [--size 1920 1080] [--reps 20] [--blocks 3] [--limit 240] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj"}
CHUNKS = (1 << 16, 1 << 18, 1 << 20, 1 << 22)


def scene_step(args, scene):
    import numpy as np
    import torch
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    W, H = args.size
    n = W * H
    hs = pkg.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", SCENES[scene]), 1000, 15)
    ctx = pkg.Context(0)
    ctx.upload(hs)
    lib = ctx.lib
    cam = pkg.default_camera(W, H)
    L = pkg.make_lights(area=True, usteps=8, vsteps=8)
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream

    pts = np.empty((n, 3), np.float32)
    capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(cam), W, H, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
    centre = torch.tensor(list(cam.center), dtype=torch.float32, device=dev)
    dirs = (torch.from_numpy(pts).to(dev) - centre).contiguous()
    origins = centre.expand(n, 3).contiguous()
    torch.cuda.synchronize(dev)

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
        capi.check(lib, ctx.handle, lib.rt_synchronize(ctx.handle), "rt_synchronize")
        return [marks[k].elapsed_time(marks[k + 1]) for k in range(reps)]

    def figure(ms, rays):
        med = statistics.median(ms)
        return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "rays_per_s": round(rays / (med * 1e-3))}

    rec = {"scene": scene, "size": [W, H], "rays": n, "reps": args.reps, "blocks": args.blocks, "light": "area 8 x 8"}

    faces, ts = ctx.closest_hits(origins, dirs, stream=sp)
    rec["closest_hits_device"] = figure(events(lambda: ctx.closest_hits(origins, dirs, stream=sp), args.reps), n)

    with torch.cuda.stream(stream):
        hit = faces >= 0
        hits = (origins[hit] + ts[hit].unsqueeze(1) * dirs[hit]).contiguous()
        lights = torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float32, device=dev).expand(hits.shape[0], 3).contiguous()
    stream.synchronize()
    m = int(hits.shape[0])
    rec["hits"] = m
    rec["light_strikes_device"] = figure(events(lambda: ctx.light_strikes_device(hits, lights, stream=sp), args.reps), m)
    rec["light_strikes_device"]["segments"] = m

    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)

    def trace(depth):
        capi.check(lib, ctx.handle, lib.rt_trace_rays_device(ctx.handle, C.byref(L), depth, n, origins.data_ptr(), dirs.data_ptr(), rgb.data_ptr(),
                                                             None, None, C.c_void_p(sp)), "rt_trace_rays_device")

    def frame(depth):
        p = pkg.make_params(W, H, depth)
        capi.check(lib, ctx.handle, lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(rgb.data_ptr()), None, None,
                                                         C.c_void_p(sp), None), "rt_render_device")

    o_host, d_host = origins.cpu().numpy(), dirs.cpu().numpy()
    out_host = np.empty((n, 3), np.float32)

    def host_trace(depth):
        fp = lambda a: a.ctypes.data_as(C.c_void_p)
        capi.check(lib, ctx.handle, lib.rt_trace_rays(ctx.handle, C.byref(L), depth, n, fp(o_host), fp(d_host), fp(out_host), None, None), "rt_trace_rays")

    for depth in (0, 4):            # (the context's own chunk size: nothing has set one yet)
        rec[f"trace_rays_device_depth{depth}"] = figure(events(lambda: trace(depth), args.reps), n)
    for depth in (0, 4):
        rec[f"render_device_depth{depth}"] = figure(events(lambda: frame(depth), args.reps), n)
        host_trace(depth)
        wall = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            host_trace(depth)
            wall.append((time.perf_counter() - t0) * 1e3)
        rec[f"trace_rays_host_depth{depth}_wall"] = figure(wall, n)
        sweep = {c: [] for c in CHUNKS}
        for _ in range(args.blocks):
            for c in CHUNKS:
                ctx.set_query_chunk(c)
                sweep[c].append(statistics.median(events(lambda: trace(depth), args.reps)))
        rec[f"chunk_sweep_depth{depth}"] = {str(c): {"ms_block_medians": [round(x, 4) for x in v], "ms_median": round(statistics.median(v), 4),
                                                     "ms_spread": round(max(v) - min(v), 4),
                                                     "rays_per_s": round(n / (statistics.median(v) * 1e-3))} for c, v in sweep.items()}
    ctx.close()
    hs.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cube,dodge")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240)
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
            print(f"query_timing: {scene} ran out of its {args.limit} s; stopping", file=sys.stderr)
            return 124
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print(f"query_timing: {scene} failed with status {r.returncode}; stopping", file=sys.stderr)
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
