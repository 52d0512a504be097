"""How much of a headline frame can run under its neighbour's k_shade: K plain frames alternating between TWO contexts (each with its own
stream, working set and output buffers) against the same K frames on ONE context (GPU only).  No library change is involved: two contexts
on one device are what two working sets and two internal streams inside one context could reach at best.

A run: one process creates the contexts on device 0 with the same scene, renders one untimed frame per context for the ray counters,
--warmup frames, synchronises, then --steps frames of plain rt_render_device calls (collect_stats 0, no stats, no hit ids) and ONE
synchronise at the end; ms per frame is the wall time between the two synchronises over --steps.  Side "one" issues every frame on context 0;
side "two" issues frame i on context i & 1.  bench.py's headline settings (1920 x 1080, depth 4, 8 x 8 light), for the cube and for dodge.

--rounds rounds per scene, one / two alternating, every run a process of its own under a time limit (--limit seconds); the first child that
fails or runs out of time ends the probe with its status.  The go rule is evaluated on the cube: every two-context run below the fastest
one-context run, and a median gain above twice --last-gain (the median gain of the last merged headline change, profiles/frame_edges_ab.json).

    python tools/frame_overlap_probe.py [--scenes cube dodge] [--rounds 8] [--steps 200] [--warmup 10] [--limit 120] [--out FILE]
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
    """one side in this process: a JSON line"""
    import torch
    import bench
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    n = 2 if args.side == "two" else 1
    scene_file, path = bench.scene_of(args.scene)
    hs = pkg.HostScene(path, 1000, 15)
    cam = pkg.default_camera(W, H)
    L = pkg.make_lights(area=True, usteps=G, vsteps=G)
    p = pkg.make_params(W, H, D, 0, H, S, 0, 1)
    p.collect_stats = 0
    ctxs, outs, streams = [], [], []
    for _ in range(n):
        c = pkg.Context(0)
        c.upload(hs)
        ctxs.append(c)
        outs.append((torch.zeros(H * W * 3, dtype=torch.float32, device=dev), torch.zeros(H * W * 3, dtype=torch.uint8, device=dev)))
        streams.append(int(c.lib.rt_stream(c.handle)) if args.streams == "own" else torch.cuda.Stream(device=dev).cuda_stream)
    torch.cuda.synchronize(dev)       # (the contexts' streams do not wait for the null stream that zeroed the buffers)

    def frame(k, stats=None):
        c = ctxs[k]
        st = c.lib.rt_render_device(c.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(outs[k][0].data_ptr()), C.c_void_p(outs[k][1].data_ptr()),
                                    None, C.c_void_p(streams[k]), C.byref(stats) if stats is not None else None)
        capi.check(c.lib, c.handle, st, "rt_render_device")

    rays = []
    for k in range(n):
        cnt = capi.rt_stats()
        frame(k, cnt)
        torch.cuda.synchronize(dev)
        rays.append(int(cnt.total_rays()))
    for i in range(args.warmup):
        frame(i % n)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(args.steps):
        frame(i % n)
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    same = all(torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) for o in outs[1:])
    for c in ctxs:
        c.close()
    hs.close()
    print(json.dumps({"side": args.side, "scene": scene_file, "contexts": n, "streams": args.streams, "ms_per_frame": round(ms, 4), "steps": args.steps, "warmup": args.warmup,
                      "rays_per_frame": rays[0], "rays_per_frame_equal": len(set(rays)) == 1, "outputs_equal": bool(same)}), flush=True)


def summary(runs, last_gain):
    one = [r["ms_per_frame"] for r in runs if r["side"] == "one"]
    two = [r["ms_per_frame"] for r in runs if r["side"] == "two"]
    gain = statistics.median(one) - statistics.median(two)
    rec = {"one_context_runs_ms": one, "two_context_runs_ms": two,
           "one_context_median_ms": round(statistics.median(one), 4), "two_context_median_ms": round(statistics.median(two), 4),
           "one_context_min_ms": min(one), "one_context_max_ms": max(one), "two_context_min_ms": min(two), "two_context_max_ms": max(two),
           "median_gain_ms": round(gain, 4), "every_two_context_run_below_one_context_min": max(two) < min(one),
           "median_gain_above_twice_last_gain": gain > 2.0 * last_gain,
           "rays_per_frame": runs[0]["rays_per_frame"],
           "rays_per_frame_equal_in_all_runs": all(r["rays_per_frame_equal"] and r["rays_per_frame"] == runs[0]["rays_per_frame"] for r in runs),
           "outputs_of_the_two_contexts_equal": all(r["outputs_equal"] for r in runs)}
    rec["go"] = rec["every_two_context_run_below_one_context_min"] and rec["median_gain_above_twice_last_gain"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cube", "dodge"], choices=["cube", "dodge"])
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--last-gain", type=float, default=0.0083, help="ms: median gain of the last merged headline change")
    ap.add_argument("--out")
    ap.add_argument("--streams", choices=["own", "torch"], default="own", help="own: every context's frames on its own stream (rt_stream), a non-blocking "
                    "stream created with the context; torch: a stream of torch's pool per context")
    ap.add_argument("--side", choices=["one", "two"], help="(internal) run one side in this process")
    ap.add_argument("--scene", default="cube", help="(internal)")
    args = ap.parse_args()
    if args.side:
        run(args)
        return 0
    rec = {"what": "K plain rt_render_device frames at bench.py's headline settings (1920x1080, depth 4, 8x8 light) on one MI355X: all on ONE context "
                   "and stream, against alternating between TWO contexts with the same scene, each with its own stream and output buffers; one "
                   "synchronise at the end, wall time over K.  Every run a process of its own, one / two alternating.",
           "go_rule": f"on the cube: every two-context run below the fastest one-context run, and median gain > 2 x {args.last_gain} ms",
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "streams": args.streams, "scenes": {}}
    for scene in args.scenes:
        runs = []
        for _ in range(args.rounds):
            for side in ("one", "two"):
                cmd = [sys.executable, os.path.abspath(__file__), "--side", side, "--scene", scene, "--steps", str(args.steps), "--warmup", str(args.warmup),
                       "--streams", args.streams]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
                except subprocess.TimeoutExpired:
                    print(f"frame_overlap_probe: {scene} / {side} ran out of its {args.limit} s; stopping", file=sys.stderr)
                    return 124
                if r.returncode != 0:
                    sys.stderr.write(r.stderr)
                    print(f"frame_overlap_probe: {scene} / {side} failed with status {r.returncode}; stopping", file=sys.stderr)
                    return r.returncode if r.returncode > 0 else 1
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
                print(line, flush=True)
                runs.append(json.loads(line))
        rec["scenes"][scene] = summary(runs, args.last_gain)
        print(json.dumps({scene: rec["scenes"][scene]}), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rec, f, indent=1)
    rec["go"] = bool(rec["scenes"].get("cube", {}).get("go", False))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
