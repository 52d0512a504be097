"""The guided upsample (rt_upsample_device) beside one iteration of the denoiser, and half- and quarter-resolution ambient occlusion brought
to full size against full-resolution occlusion (GPU only).

Step "kernel": a seeded synthetic 1920 x 1080 RGB image and geometry buffers (denoise_timing.py's: a covered disc with a depth step, two
normals and two albedos, empty outside); the low image and buffers are the pixels (2I, 2J).  In one process, on one stream, from torch events
after warm-up, --blocks blocks of --reps repetitions per side, alternating:
  upsample, upsample_miss   rt_upsample_device at s = 2 with rt_default_upsample_params, without and with the miss mask
  denoise:1, denoise:2      rt_denoise_device with 1 and 2 iterations on the same high image and buffers.  One iteration of k_atrous alone is
                            denoise:2 - denoise:1, as denoise_timing.py takes it: iteration k = 1 (step 2) in its LAST instantiation, plus what
                            iteration 0 costs more as a working-image write than as the last one
  copy                      one torch copy_ of HALF the bytes the upsample must move at minimum: it reads the high buffers (32 bytes per high
                            pixel), the low image and buffers (44 bytes per low pixel) and writes the image (12 per high pixel)
Step "pipeline": dodgeColorTest, 8 x 8 occlusion, radius 0.5, at 1920 x 1080, every pixel a point (a miss has a zero normal and is fully
open), the points built once per size on the device (rt_primary_points, closest hits, hit points):
  full                      rt_ambient_occlusion_device on the width x height points, what ao_timing.py measures (there on the hits alone,
                            recorded here too as full_hits_only)
  low:s, s = 2, 4           rt_gbuffer_device at the low size + rt_ambient_occlusion_device on the low points + rt_gbuffer_device at the high
                            size + rt_upsample_device, four calls on the stream
A side's figure is the median of its block medians, its spread their range.

Every step runs in a child process of its own under a time limit (--limit seconds); the first child that fails or runs out of time ends the
run with its status.

    python tools/upsample_timing.py [--size 1920 1080] [--reps 20] [--blocks 3] [--limit 300] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
GRID, RADIUS, SEED = 8, 0.5, 7


def events(torch, stream, call, reps):
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


def measure(torch, stream, sides, args):
    medians = {k: [] for k in sides}
    for _ in range(args.blocks):
        for k, call in sides.items():
            medians[k].append(statistics.median(events(torch, stream, call, args.reps)))
    return {k: {"ms_block_medians": [round(x, 4) for x in v], "ms_median": round(statistics.median(v), 4), "ms_range": round(max(v) - min(v), 4)}
            for k, v in medians.items()}


def kernel_step(args):
    import numpy as np
    import torch
    import rtpkg
    import denoise_timing
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    W, H = args.size
    s, ch = 2, 3
    img, g = denoise_timing.inputs(np, W, H, ch)
    low, gl = np.ascontiguousarray(img[::s, ::s]), np.ascontiguousarray(g[::s, ::s])
    w, h = low.shape[1], low.shape[0]
    t_img, t_g, t_low, t_gl = (torch.from_numpy(a).to(dev) for a in (img, g, low, gl))
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    ctx = pkg.Context(0)
    lib, hnd = ctx.lib, ctx.handle
    up = pkg.upsample_params(s)
    out, miss = torch.empty_like(t_img), torch.empty((H, W), dtype=torch.uint8, device=dev)
    dn_out = torch.empty_like(t_img)
    scratch = torch.empty(lib.rt_denoise_scratch_bytes(W, H, ch), dtype=torch.uint8, device=dev)
    min_bytes = W * H * (32 + 12) + w * h * (32 + 12)
    src, dst = torch.empty(min_bytes // 2, dtype=torch.uint8, device=dev), torch.empty(min_bytes // 2, dtype=torch.uint8, device=dev)

    def upsample(mask):
        def run():
            capi.check(lib, hnd, lib.rt_upsample_device(hnd, t_low.data_ptr(), ch, t_gl.data_ptr(), t_g.data_ptr(), W, H, C.byref(up), out.data_ptr(),
                                                        miss.data_ptr() if mask else None, sp), "rt_upsample_device")
        return run

    def denoise(n):
        p = pkg.denoise_params(iterations=n)

        def run():
            capi.check(lib, hnd, lib.rt_denoise_device(hnd, t_img.data_ptr(), ch, t_g.data_ptr(), W, H, C.byref(p), scratch.data_ptr(), dn_out.data_ptr(), sp),
                       "rt_denoise_device")
        return run

    upsample(True)()
    stream.synchronize()
    missed = int(miss.sum().item())
    sides = {"upsample": upsample(False), "upsample_miss": upsample(True), "denoise:1": denoise(1), "denoise:2": denoise(2), "copy": lambda: dst.copy_(src)}
    m = measure(torch, stream, sides, args)
    it = m["denoise:2"]["ms_median"] - m["denoise:1"]["ms_median"]
    it_range = m["denoise:2"]["ms_range"] + m["denoise:1"]["ms_range"]
    rec = {"step": "kernel", "size": [W, H], "low_size": [w, h], "factor": s, "channels": ch, "covered_share": round(float((g[..., 0] > 0).mean()), 4),
           "missed_pixels": missed, "reps": args.reps, "blocks": args.blocks, "min_bytes": min_bytes, "sides": m,
           "atrous_iteration_k1_ms": round(it, 4), "atrous_iteration_k1_range_ms": round(it_range, 4),
           "upsample_over_atrous_iteration": round(m["upsample"]["ms_median"] / it, 3),
           "upsample_over_copy": round(m["upsample"]["ms_median"] / m["copy"]["ms_median"], 2),
           "upsample_traffic_GB_per_s": round(min_bytes / (m["upsample"]["ms_median"] * 1e-3) / 1e9, 1),
           "upsample_not_above_iteration_plus_ranges": m["upsample"]["ms_median"] <= it + it_range + m["upsample"]["ms_range"]}
    ctx.close()
    print(json.dumps(rec), flush=True)


def pipeline_step(args):
    import numpy as np
    import torch
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    W, H = args.size
    hs = pkg.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", "dodgeColorTest.obj"), 1000, 15)
    ctx = pkg.Context(0)
    ctx.upload(hs)
    lib, hnd = ctx.lib, ctx.handle
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    cam = pkg.default_camera(W, H)

    def points(c, w, h):
        """(P, N, hits) of the w x h frame of camera c, on the device: every pixel a point, zeros where the ray hits nothing"""
        pts = np.empty((w * h, 3), np.float32)
        capi.check(lib, hnd, lib.rt_primary_points(hnd, C.byref(c), w, h, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
        centre = torch.tensor(list(c.center), dtype=torch.float32, device=dev)
        dirs = (torch.from_numpy(pts).to(dev) - centre).contiguous()
        origins = centre.expand(w * h, 3).contiguous()
        with torch.cuda.stream(stream):
            faces, ts = ctx.closest_hits(origins, dirs)
            P, N = ctx.hit_points(origins, dirs, faces, ts)
        stream.synchronize()
        return P, N, faces >= 0

    def occlusion(P, N, ao):
        n = int(P.shape[0])

        def run():
            capi.check(lib, hnd, lib.rt_ambient_occlusion_device(hnd, n, P.data_ptr(), N.data_ptr(), GRID, RADIUS, SEED, None, ao.data_ptr(), sp),
                       "rt_ambient_occlusion_device")
        return run

    def gbuffer(c, w, h, out):
        p = pkg.make_params(w, h)

        def run():
            capi.check(lib, hnd, lib.rt_gbuffer_device(hnd, C.byref(c), C.byref(p), out.data_ptr(), sp), "rt_gbuffer_device")
        return run

    P, N, hit = points(cam, W, H)
    ao_full = torch.empty(W * H, dtype=torch.float32, device=dev)
    Ph, Nh = P[hit].contiguous(), N[hit].contiguous()
    ao_hits = torch.empty(int(Ph.shape[0]), dtype=torch.float32, device=dev)
    g_high = torch.empty((H, W, 8), dtype=torch.float32, device=dev)
    sides = {"full": occlusion(P, N, ao_full), "full_hits_only": occlusion(Ph, Nh, ao_hits)}
    parts, keep, lows = {}, [], {}
    for s in (2, 4):
        lcam, w, h = pkg.low_camera(cam, s)
        lP, lN, _ = points(lcam, w, h)
        ao_low = torch.empty(w * h, dtype=torch.float32, device=dev)
        g_low = torch.empty((h, w, 8), dtype=torch.float32, device=dev)
        out = torch.empty((H, W), dtype=torch.float32, device=dev)
        up = pkg.upsample_params(s)
        calls = [gbuffer(lcam, w, h, g_low), occlusion(lP, lN, ao_low), gbuffer(cam, W, H, g_high)]

        def upsample(ao_low=ao_low, g_low=g_low, out=out, up=up):
            capi.check(lib, hnd, lib.rt_upsample_device(hnd, ao_low.data_ptr(), 1, g_low.data_ptr(), g_high.data_ptr(), W, H, C.byref(up), out.data_ptr(), None, sp),
                       "rt_upsample_device")
        calls.append(upsample)
        sides[f"low:{s}"] = lambda calls=calls: [c() for c in calls]
        for name, c in zip(("gbuffer_low", "occlusion_low", "gbuffer_high", "upsample"), calls):
            parts[f"low:{s}:{name}"] = c
        keep.append((lP, lN, ao_low, g_low, out, up, lcam))
        lows[s] = (w, h, out)
    m = measure(torch, stream, sides, args)
    mp = measure(torch, stream, parts, args)
    # how far the upsampled images are from the full-resolution one, over the covered pixels (the images of the last timed calls)
    stream.synchronize()
    full_img = ao_full.view(H, W)
    cov = hit.view(H, W)
    rec = {"step": "pipeline", "scene": "dodge", "size": [W, H], "grid": GRID, "radius": RADIUS, "seed": SEED, "points": W * H, "hits": int(hit.sum().item()),
           "reps": args.reps, "blocks": args.blocks, "sides": m, "parts": mp, "low": {}}
    for s, (w, h, out) in lows.items():
        d = (out - full_img)[cov].to(torch.float64)
        rec["low"][str(s)] = {"low_size": [w, h], "full_over_low": round(m["full"]["ms_median"] / m[f"low:{s}"]["ms_median"], 3),
                              "faster_than_full": m[f"low:{s}"]["ms_median"] < m["full"]["ms_median"],
                              "rms_from_full_over_hits": round(float(torch.sqrt((d * d).mean()).item()), 5)}
    ctx.close()
    hs.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--step", help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step:
        {"kernel": kernel_step, "pipeline": pipeline_step}[args.step](args)
        return 0
    records = []
    for step in ("kernel", "pipeline"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--size", str(args.size[0]), str(args.size[1]), "--reps", str(args.reps),
               "--blocks", str(args.blocks)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"upsample_timing: step {step} ran out of its {args.limit} s; stopping", file=sys.stderr)
            return 124
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print(f"upsample_timing: step {step} failed with status {r.returncode}; stopping", file=sys.stderr)
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
