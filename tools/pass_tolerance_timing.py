"""Device time of adaptive-pass frames (rt_set_pass_tolerance) against the same build's rt_set_passes frame, in one process.

For each scene and tolerance: ms/frame of the (0, P) frame with the tolerance and with the feature off, timed in alternating blocks (--reps) of
--frames frames after --warmup (torch events on one stream, as tools/passes_timing.py); medians.  Then one rt_stats frame of each for the ray
share (sum of taken / (P x pixels)), the launches and the per-kernel split (trace / shadow / shade / resolve, summed over the passes).  One
JSON line per case.  RT_LIB selects another build (the off rows of two builds are the A/B of the unchanged path).

    python tools/pass_tolerance_timing.py [--scenes cube,dodge] [--n 2] [--lens 0.08 1.6] [--passes 64] [--min 8] [--tols 0.004,0.01]
                                          [--size 1920 1080] [--grid 8] [--depth 4] [--frames 3] [--warmup 1] [--reps 3] [--off-only] [--out FILE]
    rocprofv3 --kernel-trace --stats ... -- python tools/pass_tolerance_timing.py --scenes cube --profile-frame 0.01     (or: off)
        renders exactly two frames of that one kind and nothing else: the kernel statistics are those of two frames
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cube,dodge")
    ap.add_argument("--n", type=int, default=2)
    ap.add_argument("--lens", type=float, nargs=2, default=(0.08, 1.6))
    ap.add_argument("--passes", type=int, default=64)
    ap.add_argument("--min", type=int, default=8)
    ap.add_argument("--tols", default="0.004,0.01")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--off-only", action="store_true", help="time only the rt_set_passes frame (a build without rt_set_pass_tolerance)")
    ap.add_argument("--profile-frame", help="a tolerance or 'off': two frames of that kind only, for a kernel trace")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    W, H = args.size
    P = args.passes
    stream = torch.cuda.Stream(dev)
    tols = [] if args.off_only else [float(x) for x in args.tols.split(",")]
    records = []
    for scene in args.scenes.split(","):
        hs = pkg.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", SCENES[scene]), 1000, 15)
        ctx = pkg.Context(0)
        ctx.upload(hs)
        lib = ctx.lib
        L = pkg.make_lights(area=True, usteps=args.grid, vsteps=args.grid)
        cam = pkg.default_camera(W, H)
        rgb = torch.zeros(H * W * 3, dtype=torch.float32, device=dev)
        ctx.set_supersampling(args.n)
        ctx.set_lens(*args.lens)
        ctx.set_passes(0, P)

        def frame(tol, stats=None):
            if not args.off_only:
                ctx.set_pass_tolerance(-1.0 if tol is None else tol, args.min)
            p = pkg.make_params(W, H, args.depth)
            capi.check(lib, ctx.handle, lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(rgb.data_ptr()), None, None,
                                                             C.c_void_p(stream.cuda_stream), C.byref(stats) if stats is not None else None), "rt_render_device")

        def timed(tol, k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                for _ in range(k):
                    frame(tol)
                b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / k

        if args.profile_frame:
            tol = None if args.profile_frame == "off" else float(args.profile_frame)
            with torch.cuda.stream(stream):
                frame(tol)
                frame(tol)
            torch.cuda.synchronize(dev)
            ctx.close()
            hs.close()
            continue
        kinds = [None] + tols                      # None: the feature off
        with torch.cuda.stream(stream):
            for tol in kinds:
                for _ in range(args.warmup):
                    frame(tol)
        torch.cuda.synchronize(dev)
        ms = {tol: [] for tol in kinds}
        for _ in range(args.reps):
            for tol in kinds:
                ms[tol].append(timed(tol, args.frames))
        off = statistics.median(ms[None])
        for tol in kinds:
            st = capi.rt_stats()
            frame(tol, st)
            med = statistics.median(ms[tol])
            rec = {"scene": scene, "size": [W, H], "n": args.n, "lens": list(args.lens), "grid": args.grid, "depth": args.depth, "passes": P, "min": args.min,
                   "tol": tol, "frames": args.frames, "reps": args.reps, "ms": round(med, 3), "ms_all": [round(x, 3) for x in ms[tol]],
                   "ms_over_off": round(med / off, 4), "ray_share": round(int(st.pixels) / (P * args.n * args.n * W * H), 4),
                   "launches": int(st.launches_total), "rays_primary": int(st.rays_primary), "rays_sample": int(st.rays_sample),
                   "split_ms": {k: round(float(getattr(st, "ms_" + k)), 3) for k in ("trace", "shadow", "shade", "resolve", "total")}}
            print(json.dumps(rec), flush=True)
            records.append(rec)
        ctx.close()
        hs.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
