"""Device time of motion-blurred frames (rt_set_shutter) against the still frame of the same n, in one process and on one build.

For each scene, n and lens setting (off, on): ms/frame of the shutter frame (close = the open camera yawed by --yaw) and of the still frame
(shutter off), timed in alternating blocks (--reps) of --frames frames after --warmup (torch events on one stream, as tools/lens_timing.py);
the per-group split of both (collect_stats = 2 + rt_timing_collect; resolve = total - trace - shadow - shade); rays_sample_walked and the
ray counters of both.  One JSON line per case.

    python tools/shutter_timing.py [--scenes cube,dodge] [--ns 2,4] [--lens 0,1] [--size 1920 1080] [--grid 8] [--depth 4] [--yaw 0.05]
                                   [--aperture 0.08] [--focus 2] [--frames 30] [--reps 3] [--out FILE]
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
    ap.add_argument("--ns", default="2,4")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--lens", default="0,1")
    ap.add_argument("--yaw", type=float, default=0.05)
    ap.add_argument("--aperture", type=float, default=0.08)
    ap.add_argument("--focus", type=float, default=2.0)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
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
        close = pkg.default_camera(W, H, args.yaw)
        rgb = torch.zeros(H * W * 3, dtype=torch.float32, device=dev)
        u8 = torch.zeros(H * W * 3, dtype=torch.uint8, device=dev)

        def render(collect=0, stats=None):
            p = pkg.make_params(W, H, args.depth)
            p.collect_stats = collect
            capi.check(lib, ctx.handle, lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(rgb.data_ptr()),
                                                             C.c_void_p(u8.data_ptr()), None, C.c_void_p(stream.cuda_stream),
                                                             C.byref(stats) if stats is not None else None), "rt_render_device")

        def timed(shutter, k):
            ctx.set_shutter(close if shutter else None)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                for _ in range(k):
                    render()
                b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / k

        def split(shutter):
            ctx.set_shutter(close if shutter else None)
            st = capi.rt_stats()
            render(stats=st)
            lib.rt_timing_collect(ctx.handle, C.byref(capi.rt_stats()))
            for _ in range(args.frames):
                render(collect=2)
            tim = capi.rt_stats()
            capi.check(lib, ctx.handle, lib.rt_timing_collect(ctx.handle, C.byref(tim)), "rt_timing_collect")
            k = float(args.frames)
            out = {"trace": tim.ms_trace / k, "shadow": tim.ms_shadow / k, "shade": tim.ms_shade / k}
            out["resolve"] = tim.ms_total / k - sum(out.values())
            out = {key: round(v, 4) for key, v in out.items()}
            out.update(launches=int(tim.launches_total), rays_primary=int(st.rays_primary), pixels_culled=int(st.pixels_culled),
                       shaded_hits=int(st.shaded_hits), rays_sample=int(st.rays_sample), rays_sample_walked=int(st.rays_sample_walked))
            return out

        for n in (int(x) for x in args.ns.split(",")):
            ctx.set_supersampling(n)
            for lens in (int(x) != 0 for x in args.lens.split(",")):
                ctx.set_lens(args.aperture if lens else 0.0, args.focus)
                for shutter in (False, True):
                    ctx.set_shutter(close if shutter else None)
                    with torch.cuda.stream(stream):
                        for _ in range(args.warmup):
                            render()
                torch.cuda.synchronize(dev)
                ms_still, ms_shutter = [], []
                for _ in range(args.reps):
                    ms_still.append(timed(False, args.frames))
                    ms_shutter.append(timed(True, args.frames))
                rec = {"scene": scene, "size": [W, H], "grid": args.grid, "depth": args.depth, "n": n, "yaw": args.yaw,
                       "lens": [args.aperture, args.focus] if lens else None, "frames": args.frames, "reps": args.reps,
                       "ms_shutter": round(statistics.median(ms_shutter), 4), "ms_still": round(statistics.median(ms_still), 4),
                       "ms_shutter_all": [round(x, 4) for x in ms_shutter], "ms_still_all": [round(x, 4) for x in ms_still],
                       "shutter": split(True), "still": split(False)}
                print(json.dumps(rec), flush=True)
                records.append(rec)
        ctx.close()
        hs.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
