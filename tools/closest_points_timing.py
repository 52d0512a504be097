"""The closest-point query beside rt_closest_hits_device on as many rays (GPU only).

In one process, alternating, from torch events on one stream after warm-up, --blocks blocks of --reps repetitions per side:
  dodge   the hit points of the default 1920 x 1080 camera on dodgeColorTest, and a 64^3 field over its root box
  wavy    a 64^3 field over the 1,002,530-triangle displaced grid of bench.py's cfg4
each with max_dist = +inf and with max_dist = 2 % of the root box's extent, and rt_closest_hits_device on the same number of rays (the
frame's own rays for the hit points; for a field, rays from the grid points towards the box's centre).  A side's figure is the median of its
block medians, its spread their range.  Beside them: the one-off cost of the first call after an upload (the bounds: two kernels, one
download, the host sweep, one upload), timed on the host round the call and minus a steady call, and the device memory the bounds take.

The scene runs in a child process under a time limit (--limit seconds); a child that fails or runs out of time ends the run with its status.

    python tools/closest_points_timing.py [--scene dodge|wavy] [--reps 5] [--blocks 5] [--limit 400] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1920, 1080
DIMS = (64, 64, 64)
SHARE = 0.02


def scene_step(args):
    import numpy as np
    import torch
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    tmp = tempfile.mkdtemp()
    if args.scene == "wavy":
        import scenes_gen
        path = scenes_gen.wavy_grid(tmp, n=708)
    else:
        path = os.path.join(ROOT, "tests", "golden", "scenes", "dodgeColorTest.obj")
    hs = pkg.HostScene(path, 1000, 15)
    info = hs.info()
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

    box = np.asarray(info["root_box"], np.float32)
    extent = float((box[3:] - box[:3]).max())
    radius = SHARE * extent
    rec = {"scene": args.scene, "faces": int(hs.view.n_faces), "nodes": int(hs.view.n_nodes), "face_refs": int(hs.view.n_face_refs), "max_leaf": info["max_leaf"],
           "extent": round(extent, 6), "radius": round(radius, 6), "reps": args.reps, "blocks": args.blocks}
    a = hs.arrays()
    leaf = (a["node_count_flags"] & 0x80000000) != 0
    rec["chunks"] = int(((a["node_count_flags"][leaf] & 0x7fffffff).astype(np.int64) + 63).__floordiv__(64).sum())
    rec["bounds_bytes"] = 32 * rec["nodes"] + 48 * rec["face_refs"] + 32 * rec["chunks"]

    def sides(points, origins, dirs):
        n = int(points.shape[0])
        f = torch.empty((n,), dtype=torch.int32, device=dev)
        d = torch.empty((n,), dtype=torch.float32, device=dev)
        q = torch.empty((n, 3), dtype=torch.float32, device=dev)
        t = torch.empty((n,), dtype=torch.float32, device=dev)

        def near(r):
            return lambda: capi.check(lib, handle, lib.rt_closest_points_device(handle, n, points.data_ptr(), r, f.data_ptr(), d.data_ptr(), q.data_ptr(), sp),
                                      "rt_closest_points_device")

        def hits():
            capi.check(lib, handle, lib.rt_closest_hits_device(handle, n, origins.data_ptr(), dirs.data_ptr(), f.data_ptr(), t.data_ptr(), sp), "rt_closest_hits_device")
        out = measure({"closest_points": near(float("inf")), "closest_points_2pct": near(radius), "closest_hits": hits})
        with torch.cuda.stream(stream):
            near(radius)()
        stream.synchronize()
        out["n"] = n
        out["within_2pct"] = round(float((f >= 0).float().mean().item()), 4)
        out["points_over_hits"] = round(out["closest_points"]["ms_median"] / out["closest_hits"]["ms_median"], 2)
        return out

    # the first call after the upload: the bounds
    pg = pkg.probe_grid_over(info["root_box"], DIMS, 0.0)
    grid = torch.from_numpy(pkg.probe_grid_positions(pg)).to(dev)
    free0 = torch.cuda.mem_get_info(0)[0]
    one = torch.empty((64,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    capi.check(lib, handle, lib.rt_closest_points_device(handle, 64, grid.data_ptr(), 0.0, one.data_ptr(), None, None, sp), "rt_closest_points_device")
    stream.synchronize()
    t1 = time.perf_counter()
    capi.check(lib, handle, lib.rt_closest_points_device(handle, 64, grid.data_ptr(), 0.0, one.data_ptr(), None, None, sp), "rt_closest_points_device")
    stream.synchronize()
    t2 = time.perf_counter()
    rec["first_call_ms"], rec["steady_call_ms"] = round((t1 - t0) * 1e3, 3), round((t2 - t1) * 1e3, 3)
    rec["bounds_bytes_by_free_memory"] = int(free0 - torch.cuda.mem_get_info(0)[0])

    centre = torch.tensor(((box[:3] + box[3:]) * 0.5).tolist(), dtype=torch.float32, device=dev)
    rec["field_64"] = sides(grid, grid, (centre - grid).contiguous())
    if args.scene == "dodge":
        cam = pkg.default_camera(W, H)
        n = W * H
        pts = np.empty((n, 3), np.float32)
        capi.check(lib, handle, lib.rt_primary_points(handle, C.byref(cam), W, H, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
        eye = torch.tensor(list(cam.center), dtype=torch.float32, device=dev)
        dirs = (torch.from_numpy(pts).to(dev) - eye).contiguous()
        origins = eye.expand(n, 3).contiguous()
        with torch.cuda.stream(stream):
            faces, ts = ctx.closest_hits(origins, dirs)
            P, _ = ctx.hit_points(origins, dirs, faces, ts)
        stream.synchronize()
        idx = torch.nonzero(faces >= 0).reshape(-1)
        rec["frame_hits"] = sides(P[idx].contiguous(), origins[idx].contiguous(), dirs[idx].contiguous())
    ctx.close()
    hs.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="dodge", choices=["dodge", "wavy"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--limit", type=int, default=400)
    ap.add_argument("--out")
    ap.add_argument("--step", action="store_true", help="(internal) run the scene in this process")
    args = ap.parse_args()
    if args.step:
        scene_step(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--scene", args.scene, "--reps", str(args.reps), "--blocks", str(args.blocks)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        print(f"closest_points_timing: {args.scene} ran out of its {args.limit} s", file=sys.stderr)
        return 124
    sys.stderr.write(r.stderr)
    if r.returncode != 0:
        print(f"closest_points_timing: {args.scene} failed with status {r.returncode}", file=sys.stderr)
        return r.returncode if r.returncode > 0 else 1
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(json.loads(line), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
