"""Device time of thin-lens frames (rt_set_lens) against the pinhole frame of the same n, in one process.

For each scene and n: ms/frame of the lens frame and of the pinhole frame (aperture 0), timed in alternating blocks (--reps) of --frames
frames after --warmup (torch events on one stream, as tools/aa_timing.py); the per-group split of both (collect_stats = 2 +
rt_timing_collect; resolve = total - trace - shadow - shade); rays_sample_walked and the ray counters of both.  One JSON line per case.

    python tools/lens_timing.py [--scenes cube,dodge] [--size 1920 1080] [--grid 8] [--depth 4] [--aperture 0.08] [--focus 2] [--frames 30] [--reps 3] [--out FILE]
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
        rgb = torch.zeros(H * W * 3, dtype=torch.float32, device=dev)
        u8 = torch.zeros(H * W * 3, dtype=torch.uint8, device=dev)

        def render(collect=0, stats=None):
            p = pkg.make_params(W, H, args.depth)
            p.collect_stats = collect
            capi.check(lib, ctx.handle, lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(rgb.data_ptr()),
                                                             C.c_void_p(u8.data_ptr()), None, C.c_void_p(stream.cuda_stream),
                                                             C.byref(stats) if stats is not None else None), "rt_render_device")

        def timed(aperture, k):
            ctx.set_lens(aperture, args.focus)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                for _ in range(k):
                    render()
                b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / k

        def split(aperture):
            ctx.set_lens(aperture, args.focus)
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
            for aperture in (0.0, args.aperture):
                ctx.set_lens(aperture, args.focus)
                with torch.cuda.stream(stream):
                    for _ in range(args.warmup):
                        render()
            torch.cuda.synchronize(dev)
            ms_pin, ms_lens = [], []
            for _ in range(args.reps):
                ms_pin.append(timed(0.0, args.frames))
                ms_lens.append(timed(args.aperture, args.frames))
            rec = {"scene": scene, "size": [W, H], "grid": args.grid, "depth": args.depth, "n": n, "aperture": args.aperture, "focus": args.focus,
                   "frames": args.frames, "reps": args.reps,
                   "ms_lens": round(statistics.median(ms_lens), 4), "ms_pinhole": round(statistics.median(ms_pin), 4),
                   "ms_lens_all": [round(x, 4) for x in ms_lens], "ms_pinhole_all": [round(x, 4) for x in ms_pin],
                   "lens": split(args.aperture), "pinhole": split(0.0)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
        ctx.close()
        hs.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
