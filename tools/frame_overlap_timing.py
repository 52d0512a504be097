"""A lone frame with the frame overlap: --frames x (rt_render_device; synchronise) at bench.py's headline settings, the parent's library
against this tree's (GPU only).  A frame that is waited for at once has nothing to overlap with, so what shows here is what the overlapped
route costs by itself: two events recorded and two waited for per frame, and the hop between two streams.

Every run is a process of its own under a time limit (--limit seconds), parent / new alternating, --rounds rounds; the library is chosen with
RT_LIB.  A run reports the median and the range of its per-frame wall times (host clock around the call and rt_synchronize).  The first child
that fails or runs out of time ends the tool with its status.

    python tools/frame_overlap_timing.py --parent-lib PATH [--scene cube|dodge] [--frames 200] [--rounds 4] [--limit 120] [--out FILE]
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
W, H, G, D, S = 1920, 1080, 8, 4, 8


def run(args):
    import torch
    import bench
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    _, path = bench.scene_of(args.scene)
    hs = pkg.HostScene(path, 1000, 15)
    ctx = pkg.Context(0)
    ctx.upload(hs)
    lib = ctx.lib
    cam = pkg.default_camera(W, H)
    L = pkg.make_lights(area=True, usteps=G, vsteps=G)
    p = pkg.make_params(W, H, D, 0, H, S, 0, 1)
    rgb, u8 = torch.zeros(H * W * 3, dtype=torch.float32, device=dev), torch.zeros(H * W * 3, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    if args.overlap_off:
        capi.check(lib, ctx.handle, lib.rt_set_frame_overlap(ctx.handle, 0), "rt_set_frame_overlap")

    def frame():
        capi.check(lib, ctx.handle, lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(rgb.data_ptr()), C.c_void_p(u8.data_ptr()),
                                                         None, None, None), "rt_render_device")
        capi.check(lib, ctx.handle, lib.rt_synchronize(ctx.handle), "rt_synchronize")

    for _ in range(10):
        frame()
    ms = []
    for _ in range(args.frames):
        t0 = time.perf_counter()
        frame()
        ms.append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    hs.close()
    print(json.dumps({"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_p90": round(sorted(ms)[int(0.9 * len(ms))], 4),
                      "frames": args.frames}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's librt_mi355x.so")
    ap.add_argument("--scene", default="cube", choices=["cube", "dodge"])
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true", help="(internal) run in this process with the library RT_LIB names")
    ap.add_argument("--overlap-off", action="store_true", help="(internal) rt_set_frame_overlap(ctx, 0) first")
    args = ap.parse_args()
    if args.child:
        run(args)
        return 0
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    sides = {"parent": (os.path.abspath(args.parent_lib), []), "new": (None, []), "new_overlap_off": (None, ["--overlap-off"])}
    runs = {k: [] for k in sides}
    for _ in range(args.rounds):
        for side, (lib, extra) in sides.items():
            env = dict(os.environ)
            env.pop("RT_LIB", None)
            if lib:
                env["RT_LIB"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--scene", args.scene, "--frames", str(args.frames)] + extra
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, env=env)
            except subprocess.TimeoutExpired:
                print(f"frame_overlap_timing: {side} ran out of its {args.limit} s; stopping", file=sys.stderr)
                return 124
            if r.returncode != 0:
                sys.stderr.write(r.stderr)
                print(f"frame_overlap_timing: {side} failed with status {r.returncode}; stopping", file=sys.stderr)
                return r.returncode if r.returncode > 0 else 1
            rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            print(side, json.dumps(rec), flush=True)
            runs[side].append(rec["ms_median"])
    out = {"what": f"{args.frames} x (rt_render_device; rt_synchronize) at 1920x1080, depth 4, 8x8 light, {args.scene}: the median wall time of a frame per run, "
                   "parent / new / new with rt_set_frame_overlap(ctx, 0) alternating, every run a process of its own",
           "scene": args.scene, "frames": args.frames}
    for side, v in runs.items():
        out[side] = {"runs_ms": v, "median_ms": round(statistics.median(v), 4), "min_ms": min(v), "max_ms": max(v)}
    out["new_median_inside_parent_range"] = out["parent"]["min_ms"] <= out["new"]["median_ms"] <= out["parent"]["max_ms"]
    out["new_median_not_above_parent_max"] = out["new"]["median_ms"] <= out["parent"]["max_ms"]
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
