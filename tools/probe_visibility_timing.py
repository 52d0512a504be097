"""The leak-free probe lookup beside the plain lookup and the one-bounce gather (GPU only).

In one process, alternating, from torch events on one stream after warm-up, --blocks blocks of --reps repetitions per side, on the hit
points of the default 1920 x 1080 camera on dodgeColorTest and a 6 x 5 x 5 volume over the scene's root box (m = 3, direct term):
  (1) rt_probe_irradiance_device,
  (2) rt_probe_irradiance_visible_device, with its mask,
  (3) rt_indirect_diffuse_device at m = 4,
all three on the same points.  A side's figure is the median of its block medians, its spread their range.  The masks say what the new
kernel met: the share of points that see all 8 probes (open), none (blocked) and some (mixed).

The scene runs in a child process under a time limit (--limit seconds); a child that fails or runs out of time ends the run with its status.

    python tools/probe_visibility_timing.py [--scene dodge] [--reps 10] [--blocks 5] [--limit 300] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIGHT, SEED = (-1.0, 1.0, 1.0), 7
W, H = 1920, 1080
DIMS, M = (6, 5, 5), 3


def scene_step(args):
    import numpy as np
    import torch
    import rtpkg
    from probes_timing import scene_path
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    hs = pkg.HostScene(scene_path(args.scene, tempfile.mkdtemp()), 1000, 15)
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    L = pkg.make_lights(points=(LIGHT,), area=False)
    ctx = pkg.Context(0)
    ctx.upload(hs)
    lib, handle = ctx.lib, ctx.handle

    def events(call, reps):
        with torch.cuda.stream(stream):
            for _ in range(3):
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
    n = W * H
    pts = np.empty((n, 3), np.float32)
    capi.check(lib, handle, lib.rt_primary_points(handle, C.byref(cam), W, H, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
    centre = torch.tensor(list(cam.center), dtype=torch.float32, device=dev)
    dirs = (torch.from_numpy(pts).to(dev) - centre).contiguous()
    origins = centre.expand(n, 3).contiguous()
    pg = pkg.probe_grid_over(hs.info()["root_box"], DIMS, 0.0)
    pos = torch.from_numpy(pkg.probe_grid_positions(pg)).to(dev)
    with torch.cuda.stream(stream):
        faces, ts = ctx.closest_hits(origins, dirs)
        P, N = ctx.hit_points(origins, dirs, faces, ts)
        coeff = ctx.light_probes(pos, L, M, direct=True)
    stream.synchronize()
    hit_idx = torch.nonzero(faces >= 0).reshape(-1)
    hits = int(hit_idx.numel())
    Ph, Nh = P[hit_idx].contiguous(), N[hit_idx].contiguous()
    plain = torch.empty((hits, 3), dtype=torch.float32, device=dev)
    seen = torch.empty((hits, 3), dtype=torch.float32, device=dev)
    mask = torch.empty((hits,), dtype=torch.uint8, device=dev)
    rgb = torch.empty((hits, 3), dtype=torch.float32, device=dev)

    def lookup():
        capi.check(lib, handle, lib.rt_probe_irradiance_device(handle, C.byref(pg), coeff.data_ptr(), hits, Ph.data_ptr(), Nh.data_ptr(), plain.data_ptr(), sp),
                   "rt_probe_irradiance_device")

    def visible():
        capi.check(lib, handle, lib.rt_probe_irradiance_visible_device(handle, C.byref(pg), coeff.data_ptr(), hits, Ph.data_ptr(), Nh.data_ptr(), seen.data_ptr(),
                                                                       mask.data_ptr(), sp), "rt_probe_irradiance_visible_device")

    def gather():
        capi.check(lib, handle, lib.rt_indirect_diffuse_device(handle, C.byref(L), hits, Ph.data_ptr(), Nh.data_ptr(), 4, SEED, rgb.data_ptr(), sp),
                   "rt_indirect_diffuse_device")

    rec = {"scene": args.scene, "size": [W, H], "hits": hits, "volume": list(DIMS), "m": M, "light": list(LIGHT), "reps": args.reps, "blocks": args.blocks}
    rec.update(measure({"lookup": lookup, "lookup_visible": visible, "gather_m4": gather}))
    stream.synchronize()
    open_pts, blocked = int((mask == 0xff).sum().item()), int((mask == 0).sum().item())
    rec["points"] = {"open": round(open_pts / hits, 4), "blocked": round(blocked / hits, 4), "mixed": round((hits - open_pts - blocked) / hits, 4)}
    rec["changed_points"] = round(int((plain.view(torch.int32) != seen.view(torch.int32)).any(dim=1).sum().item()) / hits, 4)
    rec["segments"] = hits * 8
    rec["visible_over_lookup"] = round(rec["lookup_visible"]["ms_median"] / rec["lookup"]["ms_median"], 2)
    rec["gather_over_visible"] = round(rec["gather_m4"]["ms_median"] / rec["lookup_visible"]["ms_median"], 2)
    rec["between"] = rec["lookup"]["ms_median"] < rec["lookup_visible"]["ms_median"] < rec["gather_m4"]["ms_median"]
    ctx.close()
    hs.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="dodge")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300)
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
        print(f"probe_visibility_timing: {args.scene} ran out of its {args.limit} s", file=sys.stderr)
        return 124
    sys.stderr.write(r.stderr)
    if r.returncode != 0:
        print(f"probe_visibility_timing: {args.scene} failed with status {r.returncode}", file=sys.stderr)
        return r.returncode if r.returncode > 0 else 1
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(json.loads(line), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
