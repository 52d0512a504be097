"""The soft-shadow query in one call against what the device ray queries offered before it (GPU only).

Per scene the points are the closest hits of the default 1920 x 1080 camera, built once on the device (rt_primary_points, closest hits, hit
points, the hits kept).  One area light at (0.6, 1.2, 0.2) with a 2 x 2, 4 x 4 and 8 x 8 grid (K = 4, 16, 64 segments per point), with the
cell centres for every point ("uniform") and with a grid of the point's own ("per_point", seed 7); in one process, alternating, from torch
events on one stream after warm-up, --blocks blocks of --reps repetitions per side:
  (a) rt_soft_shadows_device;
  (b) rt_light_strikes_device alone on the n * K segments, pre-built in device memory by torch;
  (c) route (b) and the reduction of the n * K bytes to n counts: the route the device ray queries offered, without its build time;
  (d) route (c) including the torch segment build: the samples with the float32 operations of the definition, one rounding each (the
      two divisions of the light's grid are done on the host: torch's device division is not promised to round correctly), for a
      per-point call the hash of every point's index as well.
The counts of (a) and (c) must be equal.  A side's figure is the median of its block medians, its spread their range.

Every scene runs in a child process of its own under a time limit (--limit seconds); the first child that fails or runs out of time ends
the run with its status.

    python tools/soft_shadows_timing.py [--scenes cube,dodge] [--size 1920 1080] [--reps 20] [--blocks 3] [--limit 300] [--out FILE]
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
GRIDS = (2, 4, 8)
LIGHT, SEED = (0.6, 1.2, 0.2), 7


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
        allP, _ = ctx.hit_points(origins, dirs, faces, ts)
        P = allP[faces >= 0].contiguous()
    stream.synchronize()
    n = int(P.shape[0])
    index = torch.arange(n, dtype=torch.int64, device=dev)

    def jitter():
        """(fu, fv) float32 (n, 1) of rt_shadow_jitter(SEED, i), i = 0 .. n - 1 (uint32 arithmetic carried in int64)"""
        m = 0xFFFFFFFF

        def mixed(g):
            g = g ^ (g >> 15)
            g = (g * 0x2C1B3C6D) & m
            g = g ^ (g >> 12)
            g = (g * 0x297A2D39) & m
            return g ^ (g >> 15)

        g = mixed(mixed(((index * 0x9E3779B1) & m) ^ ((SEED * 0x85EBCA6B) & m)) ^ 0xB5297A4D)
        return ((g >> 16).to(torch.float32) * 2.0 ** -16)[:, None], ((g & 0xFFFF).to(torch.float32) * 2.0 ** -16)[:, None]

    def build(L, g, per_point):
        """-> (hit, light) float32 (n * K, 3): the segments of the definition, one torch operation per float32 operation"""
        K = g * g
        c = np.array(LIGHT, np.float32)
        cx = float(np.float32(c[0] + np.float32(L.len_x) * np.float32(1.0)) / np.float32(g))
        cy = float(np.float32(c[1] + np.float32(L.len_y) * np.float32(1.0)) / np.float32(g))
        z = float(np.float32(c[2] + np.float32(L.len_x) * np.float32(0.0)))
        steps = torch.arange(g, dtype=torch.float32, device=dev)[None, :]
        fu, fv = jitter() if per_point else (0.5, 0.5)
        x = ((steps + fu) * cx).expand(n, g)[:, :, None].expand(n, g, g)            # sample i * g + j: row i gives x, column j gives y
        y = ((steps + fv) * cy).expand(n, g)[:, None, :].expand(n, g, g)
        light = torch.stack([x, y, torch.full_like(x, z)], dim=-1).reshape(-1, 3).contiguous()
        return P[:, None, :].expand(n, K, 3).reshape(-1, 3).contiguous(), light

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

    rec = {"scene": scene, "size": [W, H], "points": n, "light": list(LIGHT), "seed": SEED, "reps": args.reps, "blocks": args.blocks, "cases": {}}
    for g in GRIDS:
        K = g * g
        L = pkg.make_lights(points=(LIGHT,), area=True, usteps=g, vsteps=g)
        for mode in ("uniform", "per_point"):
            params = pkg.shadow_params(per_point=(mode == "per_point"), seed=SEED)
            with torch.cuda.stream(stream):
                hitp, light = build(L, g, mode == "per_point")
                vis_n, _ = ctx.soft_shadows(P, None, L, params, want_share=False)
                vis = ctx.light_strikes_device(hitp, light)
                by_strikes = vis.view(n, K).sum(dim=1, dtype=torch.int32)
            stream.synchronize()
            mismatches = int((vis_n.to(torch.int32) != by_strikes).sum().item())
            vis_buf = torch.empty(n * K, dtype=torch.uint8, device=dev)
            out_buf = torch.empty(n, dtype=torch.uint16, device=dev)

            def side_a():
                capi.check(lib, ctx.handle, lib.rt_soft_shadows_device(ctx.handle, C.byref(L), n, P.data_ptr(), None, C.byref(params), out_buf.data_ptr(), None,
                                                                       C.c_void_p(sp)), "rt_soft_shadows_device")

            def side_b():
                capi.check(lib, ctx.handle, lib.rt_light_strikes_device(ctx.handle, n * K, hitp.data_ptr(), light.data_ptr(), vis_buf.data_ptr(), C.c_void_p(sp)),
                           "rt_light_strikes_device")

            def side_c():
                side_b()
                return vis_buf.view(n, K).sum(dim=1, dtype=torch.int32)

            def side_d():
                h2, l2 = build(L, g, mode == "per_point")
                capi.check(lib, ctx.handle, lib.rt_light_strikes_device(ctx.handle, n * K, h2.data_ptr(), l2.data_ptr(), vis_buf.data_ptr(), C.c_void_p(sp)),
                           "rt_light_strikes_device")
                return vis_buf.view(n, K).sum(dim=1, dtype=torch.int32)

            sides = {"a_soft_shadows": side_a, "b_light_strikes_prebuilt": side_b, "c_strikes_and_count": side_c, "d_build_strikes_count": side_d}
            medians = {k: [] for k in sides}
            for _ in range(args.blocks):
                for k, call in sides.items():
                    medians[k].append(statistics.median(events(call, args.reps)))
            case = {"K": K, "mode": mode, "segments": n * K, "counts_equal": mismatches == 0, "mismatching_points": mismatches,
                    "lit_share": round(float(vis_n.to(torch.float64).mean().item()) / K, 6)}
            for k, v in medians.items():
                med = statistics.median(v)
                case[k] = {"ms_block_medians": [round(x, 4) for x in v], "ms_median": round(med, 4), "ms_range": round(max(v) - min(v), 4),
                           "segments_per_s": round(n * K / (med * 1e-3))}
            ref = case["c_strikes_and_count"]
            case["a_not_above_c_plus_range"] = case["a_soft_shadows"]["ms_median"] <= ref["ms_median"] + ref["ms_range"]
            rec["cases"][f"{K}_{mode}"] = case
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
            print(f"soft_shadows_timing: {scene} ran out of its {args.limit} s; stopping", file=sys.stderr)
            return 124
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print(f"soft_shadows_timing: {scene} failed with status {r.returncode}; stopping", file=sys.stderr)
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
