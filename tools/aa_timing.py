"""Device time of supersampled frames (rt_set_supersampling) against the n*n shifted-viewport workaround, in one process.

For each scene and n: ms/frame of the anti-aliased frame (rt_render_device, float + 8-bit output, torch events around --frames frames after
--warmup, as bench.py times its steps), its per-group split (collect_stats = 2 + rt_timing_collect; resolve = total - trace - shadow - shade),
and for n > 1 the workaround a caller has without the feature: n*n one-ray frames with viewport[0:2] = -o into n*n float frames, summed in
order and divided by n*n (torch).  The two are timed in alternating blocks (--reps); the medians are reported.  One JSON line per case.

    python tools/aa_timing.py [--scenes cube,dodge] [--size 1920 1080] [--grid 8] [--depth 4] [--frames 60] [--reps 3] [--out FILE]
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
NS = {"cube": (1, 2, 3, 4), "dodge": (1, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cube,dodge")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    W, H = args.size
    stream = torch.cuda.Stream(dev)          # a stream of its own: a NULL stream argument would mean the context's stream, not torch's
    records = []
    for scene in args.scenes.split(","):
        hs = pkg.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", SCENES[scene]), 1000, 15)
        ctx = pkg.Context(0)
        ctx.upload(hs)
        lib = ctx.lib
        L = pkg.make_lights(area=True, usteps=args.grid, vsteps=args.grid)
        rgb = torch.zeros(H * W * 3, dtype=torch.float32, device=dev)
        u8 = torch.zeros(H * W * 3, dtype=torch.uint8, device=dev)

        def render(cam, out, collect=0, with_u8=True):
            p = pkg.make_params(W, H, args.depth)
            p.collect_stats = collect
            capi.check(lib, ctx.handle, lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(out.data_ptr()),
                                                             C.c_void_p(u8.data_ptr()) if with_u8 else None, None, C.c_void_p(stream.cuda_stream), None),
                       "rt_render_device")

        def timed(step, k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                for _ in range(k):
                    step()
                b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / k

        for n in NS[scene]:
            o = [(2 * s + 1 - n) / (2.0 * n) for s in range(n)]
            cam = pkg.default_camera(W, H)
            subs = []
            for sy in range(n):
                for sx in range(n):
                    c = pkg.default_camera(W, H)
                    c.viewport[0], c.viewport[1] = -o[sx], -o[sy]       # ctypes rounds to float: -(float)o
                    subs.append(c)
            sub_out = [torch.zeros(H * W * 3, dtype=torch.float32, device=dev) for _ in subs] if n > 1 else []

            def aa():
                ctx.set_supersampling(n)
                render(cam, rgb)

            def workaround():
                ctx.set_supersampling(1)
                for c, buf in zip(subs, sub_out):
                    render(c, buf, with_u8=False)
                acc = torch.zeros_like(rgb)
                for buf in sub_out:
                    acc = acc + buf
                rgb.copy_(acc / float(n * n))

            st = capi.rt_stats()
            ctx.set_supersampling(n)
            p = pkg.make_params(W, H, args.depth)
            capi.check(lib, ctx.handle, lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(rgb.data_ptr()),
                                                             C.c_void_p(u8.data_ptr()), None, C.c_void_p(stream.cuda_stream), C.byref(st)), "stats")
            with torch.cuda.stream(stream):
                for _ in range(args.warmup):
                    aa()
                    if n > 1:
                        workaround()
            torch.cuda.synchronize(dev)
            ms_aa, ms_wa = [], []
            for _ in range(args.reps):
                ms_aa.append(timed(aa, args.frames))
                if n > 1:
                    ms_wa.append(timed(workaround, max(1, args.frames // 2)))
            # per-group split: lean per-kernel events (collect_stats = 2) over the same number of frames
            ctx.set_supersampling(n)
            lib.rt_timing_collect(ctx.handle, C.byref(capi.rt_stats()))
            for _ in range(args.frames):
                render(cam, rgb, collect=2)
            tim = capi.rt_stats()
            capi.check(lib, ctx.handle, lib.rt_timing_collect(ctx.handle, C.byref(tim)), "rt_timing_collect")
            k = float(args.frames)
            split = {"trace": tim.ms_trace / k, "shadow": tim.ms_shadow / k, "shade": tim.ms_shade / k}
            split["resolve"] = tim.ms_total / k - sum(split.values())
            rec = {"scene": scene, "size": [W, H], "grid": args.grid, "depth": args.depth, "n": n, "frames": args.frames, "reps": args.reps,
                   "ms_aa": round(statistics.median(ms_aa), 4), "ms_aa_all": [round(x, 4) for x in ms_aa],
                   "split_ms": {key: round(v, 4) for key, v in split.items()}, "launches": int(tim.launches_total),
                   "sub_samples": int(st.pixels), "rays_primary": int(st.rays_primary), "rays_sample": int(st.rays_sample),
                   "rays_sample_walked": int(st.rays_sample_walked)}
            if n > 1:
                rec["ms_workaround"] = round(statistics.median(ms_wa), 4)
                rec["ms_workaround_all"] = [round(x, 4) for x in ms_wa]
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del sub_out
        ctx.close()
        hs.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
