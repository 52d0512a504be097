"""Bounced light beside its parents (GPU only).

Per scene, in one process, alternating, from torch events on one stream after warm-up, --blocks blocks of --reps repetitions per side:
  (1) a 16 x 16 x 16 volume (4,096 probes) at m = 8: rt_light_probes_device against rt_light_probes_bounce_device, plain and visible, with
      pass 0 of the same volume as the source;
  (2) the hit points of the default 1920 x 1080 camera at m = 4: rt_indirect_diffuse_device against rt_indirect_diffuse_bounce_device, plain
      and visible, with an 8 x 8 x 8 volume (m = 8, no direct term) as the source;
  (3) Flyscene.light_probes on an 8 x 8 x 8 volume at m = 8 with bounces = 0 .. 4, visible and plain: wall-clock time of the whole member
      (host arrays in and out, one synchronisation per pass), the median of --reps calls.
The parents' kernels are those of the commit before this feature instruction for instruction (tools/isa_diff.py), so their side of (1) and
(2) is the parent commit's figure on the same inputs.  A side's figure is the median of its block medians, its spread their range.

Every scene runs in a child process of its own under a time limit (--limit seconds); the first child that fails or runs out of time ends
the run with its status.

    python tools/probe_bounce_timing.py [--scenes dodge,mixed] [--reps 10] [--blocks 3] [--limit 300] [--out FILE]
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

LIGHT, SEED = (-1.0, 1.0, 1.0), 7
W, H = 1920, 1080


def scene_path(scene, tmp):
    if scene == "mixed":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import scenes_gen
        return scenes_gen.mixed_materials(tmp)
    return os.path.join(ROOT, "tests", "golden", "scenes", {"cube": "cube.obj", "dodge": "dodgeColorTest.obj", "toy": "toy.obj"}[scene])


def scene_step(args, scene):
    import numpy as np
    import torch
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    path = scene_path(scene, tempfile.mkdtemp())
    hs = pkg.HostScene(path, 1000, 15)
    box = hs.info()["root_box"]
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

    def volume(d, m):
        pg = pkg.probe_grid_over(box, (d, d, d), 0.0)
        pos = torch.from_numpy(pkg.probe_grid_positions(pg)).to(dev)
        coeff = torch.empty((pos.shape[0], 27), dtype=torch.float32, device=dev)
        capi.check(lib, handle, lib.rt_light_probes_device(handle, C.byref(L), pos.shape[0], pos.data_ptr(), m, 0, coeff.data_ptr(), sp), "rt_light_probes_device")
        stream.synchronize()
        return pg, pos, coeff

    rec = {"scene": scene, "size": [W, H], "light": list(LIGHT), "reps": args.reps, "blocks": args.blocks}

    # (1) the probes
    pg, pos, src = volume(16, 8)
    out = torch.empty_like(src)
    count = pos.shape[0]

    def probes(visible):
        if visible is None:
            return lambda: capi.check(lib, handle, lib.rt_light_probes_device(handle, C.byref(L), count, pos.data_ptr(), 8, 0, out.data_ptr(), sp), "rt_light_probes_device")
        return lambda: capi.check(lib, handle, lib.rt_light_probes_bounce_device(handle, C.byref(L), count, pos.data_ptr(), 8, 0, C.byref(pg), src.data_ptr(), visible,
                                                                                 out.data_ptr(), sp), "rt_light_probes_bounce_device")

    case = measure({"parent": probes(None), "bounce_plain": probes(0), "bounce_visible": probes(1)})
    case.update({"probes": count, "m": 8, "rays": count * 64, "lit_probes": int((src != 0).any(dim=1).sum().item())})
    for k in ("bounce_plain", "bounce_visible"):
        case[k + "_over_parent"] = round(case[k]["ms_median"] / case["parent"]["ms_median"], 3)
    rec["probes_4096_m8"] = case

    # (2) the gather on the frame's hit points
    cam = pkg.default_camera(W, H)
    n = W * H
    pts = np.empty((n, 3), np.float32)
    capi.check(lib, handle, lib.rt_primary_points(handle, C.byref(cam), W, H, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
    centre = torch.tensor(list(cam.center), dtype=torch.float32, device=dev)
    dirs = (torch.from_numpy(pts).to(dev) - centre).contiguous()
    origins = centre.expand(n, 3).contiguous()
    with torch.cuda.stream(stream):
        faces, ts = ctx.closest_hits(origins, dirs)
        P, N = ctx.hit_points(origins, dirs, faces, ts)
    stream.synchronize()
    hit_idx = torch.nonzero(faces >= 0).reshape(-1)
    hits = int(hit_idx.numel())
    Ph, Nh = P[hit_idx].contiguous(), N[hit_idx].contiguous()
    rgb = torch.empty((hits, 3), dtype=torch.float32, device=dev)
    pg8, _, src8 = volume(8, 8)

    def gather(visible):
        if visible is None:
            return lambda: capi.check(lib, handle, lib.rt_indirect_diffuse_device(handle, C.byref(L), hits, Ph.data_ptr(), Nh.data_ptr(), 4, SEED, rgb.data_ptr(), sp),
                                      "rt_indirect_diffuse_device")
        return lambda: capi.check(lib, handle, lib.rt_indirect_diffuse_bounce_device(handle, C.byref(L), hits, Ph.data_ptr(), Nh.data_ptr(), 4, SEED, C.byref(pg8),
                                                                                     src8.data_ptr(), visible, rgb.data_ptr(), sp), "rt_indirect_diffuse_bounce_device")

    case = measure({"parent": gather(None), "bounce_plain": gather(0), "bounce_visible": gather(1)})
    case.update({"points": hits, "m": 4, "rays": hits * 16})
    for k in ("bounce_plain", "bounce_visible"):
        case[k + "_over_parent"] = round(case[k]["ms_median"] / case["parent"]["ms_median"], 3)
    rec["gather_hits_m4"] = case

    # (3) the member, whole
    ctx.close()
    hs.close()
    fs = pkg.Flyscene(scene_path=path)
    fs.initialize(64, 40, False, True)
    fs.lights = [LIGHT]
    member = {}
    for visible in (True, False):
        for b in range(5):
            fs.light_probes((8, 8, 8), 8, bounces=b, visible=visible)
            took = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fs.light_probes((8, 8, 8), 8, bounces=b, visible=visible)
                took.append((time.perf_counter() - t0) * 1e3)
            member[f"{'visible' if visible else 'plain'}_bounces_{b}"] = {"ms_median": round(statistics.median(took), 4), "ms_range": round(max(took) - min(took), 4)}
    rec["flyscene_light_probes_512_m8"] = member
    fs.ctx.close()
    fs.scene.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dodge,mixed")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--step", help="(internal) run one scene in this process")
    args = ap.parse_args()
    if args.step:
        scene_step(args, args.step)
        return 0
    records = []
    for scene in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", scene, "--reps", str(args.reps), "--blocks", str(args.blocks)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"probe_bounce_timing: {scene} ran out of its {args.limit} s; stopping", file=sys.stderr)
            return 124
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print(f"probe_bounce_timing: {scene} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        records.append(json.loads(line))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
