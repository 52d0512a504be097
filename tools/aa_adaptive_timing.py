"""Device time of adaptive supersampled frames (rt_set_supersampling_threshold) against the regular n x n frame, in one process.

For each scene, n and threshold tau: ms/frame of the adaptive frame and of the regular frame (tau < 0) of the same n, timed in alternating
blocks (--reps) of --frames frames after --warmup (torch events on one stream, as tools/aa_timing.py); the refined fraction
(rt_supersampling_refined / W*H); the per-group split of the adaptive frame (collect_stats = 2 + rt_timing_collect, both passes summed;
resolve = total - trace - shadow - shade, which includes k_flag).  One JSON line per case.

    python tools/aa_adaptive_timing.py [--scenes cube,dodge] [--size 1920 1080] [--grid 8] [--depth 4] [--frames 30] [--reps 3] [--out FILE]
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
NS = {"cube": (2, 3, 4), "dodge": (2, 4)}
TAUS = (0.0, 0.05, 0.1, 0.3, float("inf"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cube,dodge")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--depth", type=int, default=4)
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

        def render(collect=0):
            p = pkg.make_params(W, H, args.depth)
            p.collect_stats = collect
            capi.check(lib, ctx.handle, lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(rgb.data_ptr()),
                                                             C.c_void_p(u8.data_ptr()), None, C.c_void_p(stream.cuda_stream), None), "rt_render_device")

        def timed(tau, k):
            ctx.set_supersampling_threshold(tau)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                for _ in range(k):
                    render()
                b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / k

        for n in NS[scene]:
            ctx.set_supersampling(n)
            for tau in TAUS:
                for t in (-1.0, tau):
                    ctx.set_supersampling_threshold(t)
                    with torch.cuda.stream(stream):
                        for _ in range(args.warmup):
                            render()
                torch.cuda.synchronize(dev)
                ms_ad, ms_reg = [], []
                for _ in range(args.reps):
                    ms_reg.append(timed(-1.0, args.frames))
                    ms_ad.append(timed(tau, args.frames))
                refined = ctx.supersampling_refined()
                lib.rt_timing_collect(ctx.handle, C.byref(capi.rt_stats()))
                for _ in range(args.frames):
                    render(collect=2)
                tim = capi.rt_stats()
                capi.check(lib, ctx.handle, lib.rt_timing_collect(ctx.handle, C.byref(tim)), "rt_timing_collect")
                k = float(args.frames)
                split = {"trace": tim.ms_trace / k, "shadow": tim.ms_shadow / k, "shade": tim.ms_shade / k}
                split["resolve_flag"] = tim.ms_total / k - sum(split.values())
                rec = {"scene": scene, "size": [W, H], "grid": args.grid, "depth": args.depth, "n": n, "tau": tau,
                       "ms_adaptive": round(statistics.median(ms_ad), 4), "ms_regular": round(statistics.median(ms_reg), 4),
                       "ms_adaptive_all": [round(x, 4) for x in ms_ad], "ms_regular_all": [round(x, 4) for x in ms_reg],
                       "refined_fraction": round(refined / float(W * H), 5), "pixels": int(tim.pixels),
                       "split_ms": {key: round(v, 4) for key, v in split.items()}, "launches": int(tim.launches_total)}
                print(json.dumps(rec), flush=True)
                records.append(rec)
        ctx.close()
        hs.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
