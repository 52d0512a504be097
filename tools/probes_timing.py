"""The light probes beside the one-bounce gather (GPU only).

Per scene, in one process, alternating, from torch events on one stream after warm-up, --blocks blocks of --reps repetitions per side:
  (1) rt_light_probes_device on a 16 x 16 x 16 volume (4,096 probes) at m = 8 against rt_indirect_diffuse_device on 4,096 hit points of the
      default 1920 x 1080 camera at m = 8, and on an 8 x 8 x 8 volume (512 probes) at m = 16 against 512 points at m = 16: the same number
      of rays on both sides.  The probe rays cover the sphere from free space, the gather rays a hemisphere from a surface, so the walks
      are not the same walks; the ratio says what a probe ray costs beside a gather ray, no more.
  (2) the same probe calls in a build whose 27-task sum is compiled out (make ab AB_FLAGS=-DRT_PROBES_NO_SUM, --nosum-lib): the
      difference is the share of the kernel spent in the sum.
  (3) rt_probe_irradiance_device on the hit points and normals of the whole 1920 x 1080 frame (misses stay in the batch as "no point").
  (4) the break-even: an 8 x 8 x 8 volume at m = 8 once, plus a lookup per frame, against rt_indirect_diffuse_device at m = 4 on the
      frame's hit points every frame: the volume is ahead after probes_ms / (gather_ms - lookup_ms) frames.
A side's figure is the median of its block medians, its spread their range.

Every scene runs in a child process of its own under a time limit (--limit seconds); the first child that fails or runs out of time ends
the run with its status.

    python tools/probes_timing.py [--scenes dodge,mixed] [--reps 10] [--blocks 3] [--limit 300] [--nosum-lib PATH] [--out FILE]
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

LIGHT, SEED = (-1.0, 1.0, 1.0), 7
W, H = 1920, 1080
PAIRS = ((16, 8), (8, 16))                    # (probes per axis, m): 4,096 probes at m = 8, 512 at m = 16


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
    tmp = tempfile.mkdtemp()
    hs = pkg.HostScene(scene_path(scene, tmp), 1000, 15)
    box = hs.info()["root_box"]
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    L = pkg.make_lights(points=(LIGHT,), area=False)

    def context(lib_path=None):
        """a context of the shipped library, or of another build of it, with the scene"""
        if lib_path is None:
            ctx = pkg.Context(0)
            ctx.upload(hs)
            return ctx.lib, ctx.handle, ctx
        lib = capi.load_library(lib_path)
        h = C.c_void_p()
        capi.check(lib, None, lib.rt_create(C.byref(h), 0), "rt_create")
        capi.check(lib, h, lib.rt_upload_scene(h, C.byref(hs.view)), "rt_upload_scene")
        return lib, h, None

    lib, handle, ctx = context()
    nosum = context(args.nosum_lib) if args.nosum_lib else None

    def events(call, reps):
        """ms of each of `reps` repetitions of call() on the stream, after three warm ones"""
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

    # the frame's hit points, built on the device
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
    rec = {"scene": scene, "size": [W, H], "hits": hits, "light": list(LIGHT), "reps": args.reps, "blocks": args.blocks, "same_rays": {}}

    def probe_call(lb, h, pos, m, out):
        return lambda: capi.check(lb, h, lb.rt_light_probes_device(h, C.byref(L), pos.shape[0], pos.data_ptr(), m, 0, out.data_ptr(), sp), "rt_light_probes_device")

    def gather_call(Pp, Nn, m, out):
        return lambda: capi.check(lib, handle, lib.rt_indirect_diffuse_device(handle, C.byref(L), Pp.shape[0], Pp.data_ptr(), Nn.data_ptr(), m, SEED, out.data_ptr(), sp),
                                  "rt_indirect_diffuse_device")

    # (1), (2): the same number of rays on both sides
    for d, m in PAIRS:
        pg = pkg.probe_grid_over(box, (d, d, d), 0.0)
        pos = torch.from_numpy(pkg.probe_grid_positions(pg)).to(dev)
        count = pos.shape[0]
        pick = hit_idx[torch.linspace(0, hits - 1, count, device=dev).long()]
        Pp, Nn = P[pick].contiguous(), N[pick].contiguous()
        coeff = torch.empty((count, 27), dtype=torch.float32, device=dev)
        rgb = torch.empty((count, 3), dtype=torch.float32, device=dev)
        sides = {"probes": probe_call(lib, handle, pos, m, coeff), "gather": gather_call(Pp, Nn, m, rgb)}
        if nosum:
            scratch = torch.zeros((count, 27), dtype=torch.float32, device=dev)
            sides["probes_without_sum"] = probe_call(nosum[0], nosum[1], pos, m, scratch)
        case = measure(sides)
        case.update({"probes": dict(case["probes"], count=count, m=m, rays=count * m * m), "lit_probes": int((coeff != 0).any(dim=1).sum().item())})
        case["probes_over_gather"] = round(case["probes"]["ms_median"] / case["gather"]["ms_median"], 3)
        if nosum:
            case["sum_share_of_kernel"] = round(1.0 - case["probes_without_sum"]["ms_median"] / case["probes"]["ms_median"], 4)
        rec["same_rays"][f"{count}_probes_m{m}"] = case

    # (3), (4): the lookup of a whole frame, and the break-even against a per-frame gather at m = 4
    pg = pkg.probe_grid_over(box, (8, 8, 8), 0.0)
    pos = torch.from_numpy(pkg.probe_grid_positions(pg)).to(dev)
    coeff = torch.empty((512, 27), dtype=torch.float32, device=dev)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    Ph, Nh = P[hit_idx].contiguous(), N[hit_idx].contiguous()
    rgb = torch.empty((hits, 3), dtype=torch.float32, device=dev)

    def lookup():
        capi.check(lib, handle, lib.rt_probe_irradiance_device(handle, C.byref(pg), coeff.data_ptr(), n, P.data_ptr(), N.data_ptr(), out.data_ptr(), sp),
                   "rt_probe_irradiance_device")

    frame = measure({"volume_512_m8": probe_call(lib, handle, pos, 8, coeff), "lookup_1080p": lookup, "gather_hits_m4": gather_call(Ph, Nh, 4, rgb)})
    per_frame = frame["gather_hits_m4"]["ms_median"] - frame["lookup_1080p"]["ms_median"]
    frame["break_even_frames"] = round(frame["volume_512_m8"]["ms_median"] / per_frame, 3) if per_frame > 0 else None
    frame["lookup_bytes"] = n * 36 + 512 * 108
    frame["lookup_gbytes_per_s"] = round(frame["lookup_bytes"] / (frame["lookup_1080p"]["ms_median"] * 1e-3) / 1e9, 1)
    rec["frame"] = frame
    if nosum:
        nosum[0].rt_destroy(nosum[1])
    ctx.close()
    hs.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dodge,mixed")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--nosum-lib", help="a build of the library with -DRT_PROBES_NO_SUM (make ab), for the share of the sum")
    ap.add_argument("--out")
    ap.add_argument("--step", help="(internal) run one scene in this process")
    args = ap.parse_args()
    if args.step:
        scene_step(args, args.step)
        return 0
    records = []
    for scene in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", scene, "--reps", str(args.reps), "--blocks", str(args.blocks)]
        if args.nosum_lib:
            cmd += ["--nosum-lib", os.path.abspath(args.nosum_lib)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"probes_timing: {scene} ran out of its {args.limit} s; stopping", file=sys.stderr)
            return 124
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print(f"probes_timing: {scene} failed with status {r.returncode}; stopping", file=sys.stderr)
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
