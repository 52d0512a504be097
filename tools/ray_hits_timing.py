"""The ordered multi-hit ray query beside rt_closest_hits_device on the same rays (GPU only).

In one process per scene, alternating, from torch events on one stream after warm-up, --blocks blocks of --reps repetitions per side, on the
hit-producing primary rays of the default 1920 x 1080 camera of cube and dodgeColorTest:
  closest_hits     rt_closest_hits_device (the yardstick: the kernel of the parent commit, unchanged)
  ray_hits_k       rt_ray_hits_device with k = 1, 4, 8 and t_max = +inf, all three outputs
  emulation_k      what the query replaces: k successive rt_closest_hits_device calls, each from the previous hit advanced by 1e-4 of the
                   direction (torch elementwise kernels between the calls) -- k launches and k walks, and not the same answer: it drops
                   coincident faces and depends on the step
A side's figure is the median of its block medians, its spread their range.  Beside them the share of rays per count class at k = 8.

Each scene runs in a child process under a time limit (--limit seconds); a child that fails or runs out of time ends the run with its status.

    python tools/ray_hits_timing.py [--reps 5] [--blocks 5] [--limit 200] [--out FILE]
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

W, H = 1920, 1080
KS = (1, 4, 8)
SCENES = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj"}
STEP = 1e-4


def scene_step(args):
    import numpy as np
    import torch
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    hs = pkg.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", SCENES[args.scene]), 1000, 15)
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    ctx = pkg.Context(0)
    ctx.upload(hs)
    lib, handle = ctx.lib, ctx.handle

    def events(call, reps):
        with torch.cuda.stream(stream):
            for _ in range(2):
                call()
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
            marks[0].record(stream)
            for k in range(reps):
                call()
                marks[k + 1].record(stream)
        marks[-1].synchronize()
        return [marks[k].elapsed_time(marks[k + 1]) for k in range(reps)]

    def measure(sides):
        medians = {k: [] for k in sides}
        for _ in range(args.blocks):
            for k, call in sides.items():
                medians[k].append(statistics.median(events(call, args.reps)))
        stream.synchronize()
        return {k: {"ms_block_medians": [round(x, 4) for x in v], "ms_median": round(statistics.median(v), 4), "ms_range": round(max(v) - min(v), 4)}
                for k, v in medians.items()}

    cam = pkg.default_camera(W, H)
    pts = np.empty((W * H, 3), np.float32)
    capi.check(lib, handle, lib.rt_primary_points(handle, C.byref(cam), W, H, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
    eye = torch.tensor(list(cam.center), dtype=torch.float32, device=dev)
    dirs = (torch.from_numpy(pts).to(dev) - eye).contiguous()
    origins = eye.expand(W * H, 3).contiguous()
    with torch.cuda.stream(stream):
        faces, _ = ctx.closest_hits(origins, dirs)
    stream.synchronize()
    idx = torch.nonzero(faces >= 0).reshape(-1)
    o, d = origins[idx].contiguous(), dirs[idx].contiguous()
    n = int(o.shape[0])
    f1, t1 = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev)
    fk, tk = torch.empty((n, 8), dtype=torch.int32, device=dev), torch.empty((n, 8), dtype=torch.float32, device=dev)
    ck = torch.empty((n,), dtype=torch.int32, device=dev)

    def closest(org=o):
        capi.check(lib, handle, lib.rt_closest_hits_device(handle, n, org.data_ptr(), d.data_ptr(), f1.data_ptr(), t1.data_ptr(), sp), "rt_closest_hits_device")

    def hits(k):
        return lambda: capi.check(lib, handle, lib.rt_ray_hits_device(handle, n, o.data_ptr(), d.data_ptr(), k, float("inf"), fk.data_ptr(), tk.data_ptr(),
                                                                      ck.data_ptr(), sp), "rt_ray_hits_device")

    def emulation(k):
        def call():
            org = o
            for j in range(k):
                closest(org)
                if j + 1 < k:
                    org = torch.where((f1 >= 0)[:, None], org + d * (t1 + STEP)[:, None], org).contiguous()
        return call

    sides = {"closest_hits": closest}
    for k in KS:
        sides[f"ray_hits_{k}"] = hits(k)
    for k in KS:
        sides[f"emulation_{k}"] = emulation(k)
    rec = {"scene": args.scene, "faces": int(hs.view.n_faces), "nodes": int(hs.view.n_nodes), "rays": n, "reps": args.reps, "blocks": args.blocks}
    rec.update(measure(sides))
    with torch.cuda.stream(stream):
        hits(8)()
    stream.synchronize()
    rec["share_per_count_0_to_9"] = [round(float((ck == c).float().mean().item()), 4) for c in range(10)]
    base = rec["closest_hits"]["ms_median"]
    for k in KS:
        rec[f"ray_hits_{k}_over_closest_hits"] = round(rec[f"ray_hits_{k}"]["ms_median"] / base, 3)
        rec[f"emulation_{k}_over_ray_hits_{k}"] = round(rec[f"emulation_{k}"]["ms_median"] / rec[f"ray_hits_{k}"]["ms_median"], 3)
    ctx.close()
    hs.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--limit", type=int, default=200)
    ap.add_argument("--out")
    ap.add_argument("--step", action="store_true", help="(internal) run the scene of --scene in this process")
    ap.add_argument("--scene", default="cube", choices=list(SCENES))
    args = ap.parse_args()
    if args.step:
        scene_step(args)
        return 0
    out = {}
    for scene in SCENES:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", "--scene", scene, "--reps", str(args.reps), "--blocks", str(args.blocks)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"ray_hits_timing: {scene} ran out of its {args.limit} s", file=sys.stderr)
            return 124
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print(f"ray_hits_timing: {scene} failed with status {r.returncode}", file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        out[scene] = json.loads(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
