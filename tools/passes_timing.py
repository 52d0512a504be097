"""Device time of multi-pass frames (rt_set_passes) against what a caller could do without them, in one process and on one build.

For each scene, n and pass count P: ms/frame of the (0, P) frame, of the workaround -- P single frames of pass 0 summed and scaled with torch
(it cannot reseed, so this compares cost only) -- and of the single frame (P x that is the accumulation-free floor), timed in alternating
blocks (--reps) of --frames frames after --warmup (torch events on one stream, as tools/shutter_timing.py); medians.  One JSON line per case.

    python tools/passes_timing.py [--scenes cube,dodge] [--ns 1,2,4] [--passes 1,4,16] [--size 1920 1080] [--grid 8] [--depth 4]
                                  [--frames 10] [--warmup 3] [--reps 3] [--out FILE]
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
    ap.add_argument("--ns", default="1,2,4")
    ap.add_argument("--passes", default="1,4,16")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    W, H = args.size
    stream = torch.cuda.Stream(dev)
    records = []
    for scene in args.scenes.split(","):
        hs = pkg.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", SCENES[scene]), 1000, 15)
        ctx = pkg.Context(0)
        ctx.upload(hs)
        lib = ctx.lib
        L = pkg.make_lights(area=True, usteps=args.grid, vsteps=args.grid)
        cam = pkg.default_camera(W, H)
        rgb = torch.zeros(H * W * 3, dtype=torch.float32, device=dev)
        total = torch.zeros_like(rgb)

        def render():
            p = pkg.make_params(W, H, args.depth)
            capi.check(lib, ctx.handle, lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(rgb.data_ptr()), None, None,
                                                             C.c_void_p(stream.cuda_stream), None), "rt_render_device")

        def frame(kind, P):
            if kind == "passes":
                ctx.set_passes(0, P)
                render()
            elif kind == "single":
                ctx.set_passes(0, 1)
                render()
            else:                                    # the workaround: P frames, a torch sum, one scale
                ctx.set_passes(0, 1)
                total.zero_()
                for _ in range(P):
                    render()
                    total.add_(rgb)
                total.div_(float(P))

        def timed(kind, P, k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                for _ in range(k):
                    frame(kind, P)
                b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / k

        for n in (int(x) for x in args.ns.split(",")):
            ctx.set_supersampling(n)
            for P in (int(x) for x in args.passes.split(",")):
                kinds = ("passes", "workaround", "single")
                with torch.cuda.stream(stream):
                    for kind in kinds:
                        for _ in range(args.warmup):
                            frame(kind, P)
                torch.cuda.synchronize(dev)
                ms = {kind: [] for kind in kinds}
                for _ in range(args.reps):
                    for kind in kinds:
                        ms[kind].append(timed(kind, P, args.frames))
                ctx.set_passes(0, P)
                st = capi.rt_stats()
                p = pkg.make_params(W, H, args.depth)
                capi.check(lib, ctx.handle, lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(rgb.data_ptr()), None, None,
                                                                 C.c_void_p(stream.cuda_stream), C.byref(st)), "rt_render_device")
                med = {kind: statistics.median(v) for kind, v in ms.items()}
                rec = {"scene": scene, "size": [W, H], "grid": args.grid, "depth": args.depth, "n": n, "passes": P, "frames": args.frames, "reps": args.reps,
                       "ms_passes": round(med["passes"], 4), "ms_workaround": round(med["workaround"], 4), "ms_single": round(med["single"], 4),
                       "ms_single_times_passes": round(med["single"] * P, 4), "passes_over_single_times_passes": round(med["passes"] / (med["single"] * P), 4),
                       "ms_all": {kind: [round(x, 4) for x in v] for kind, v in ms.items()},
                       "launches": int(st.launches_total), "ms_resolve_sum": round(st.ms_resolve, 4), "rays_primary": int(st.rays_primary)}
                print(json.dumps(rec), flush=True)
                records.append(rec)
        ctx.close()
        hs.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
