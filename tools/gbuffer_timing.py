"""The geometry-buffer query against the only route the device ray queries offered to the same numbers, and bench.py of this tree against
a parent tree (GPU only).

Query (default).  Per scene (cube, dodge), 1920 x 1080, default camera, for (n, first, count) = (1, 0, 1) and (2, 0, 4), in one process,
alternating, from torch events on one stream after warm-up, --blocks blocks of --reps repetitions per side:
  (a) rt_gbuffer_device;
  (b) the route without it: per pass, torch builds the n * n * W * H sub-sample rays of the pinhole camera on the device (the raster terms
      of every column and row come from the host, once, outside the timed region: torch's device division is not promised to round
      correctly), rt_closest_hits_device walks them, torch gathers normals and kd by face, sums the sub-samples in the definition's order,
      divides, and accumulates the passes.
The two results are compared bit for bit and the number of differing pixels is recorded.  A side's figure is the median of its block
medians, its spread their range.  Every scene runs in a child process of its own under a time limit (--limit seconds); the first child that
fails or runs out of time ends the run with its status.

Bench (--bench PARENT_ROOT).  `python bench.py --gpus 1 --steps S --warmup W [--scene dodge]` in PARENT_ROOT (a built tree of the parent
commit) and in this tree, alternating parent / new, --rounds rounds per scene, every run a process of its own under the time limit.  The
parent's own range is the run-to-run spread the new median is held against.

    python tools/gbuffer_timing.py [--scenes cube,dodge] [--size 1920 1080] [--reps 20] [--blocks 8] [--limit 300] [--out FILE]
    python tools/gbuffer_timing.py --bench PARENT_ROOT [--rounds 8] [--steps 200] [--warmup 10] [--out FILE]
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

SCENES = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj"}
CASES = ((1, 0, 1), (2, 0, 4))


def scene_step(args, scene):
    import numpy as np
    import torch
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    W, H = args.size
    hs = pkg.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", SCENES[scene]), 1000, 15)
    ctx = pkg.Context(0)
    ctx.upload(hs)
    lib = ctx.lib
    cam = pkg.default_camera(W, H)
    p = pkg.make_params(W, H)
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    arrays = hs.arrays()
    fn = torch.from_numpy(arrays["face_normal"]).to(dev)
    kd = torch.from_numpy(np.ascontiguousarray(arrays["mat_f"][:, 0:3][arrays["mat_id"]])).to(dev)
    table = torch.cat([fn, kd], dim=1).contiguous()                      # (faces, 6)
    centre = torch.tensor(list(cam.center), dtype=torch.float32, device=dev)
    m = np.array(list(cam.inv_view), np.float32).reshape(3, 4)
    M = torch.from_numpy(m).to(dev)

    def raster_terms(n, pss):
        """host, float32 as the device rounds: n0[W, n] and n1[H, n] of every pass -- screen_point's two terms, scaled by k0 / k1"""
        import math
        persp = np.float32(1.0 / math.tan(float(np.float32(cam.fovy / np.float32(2.0))) * (math.pi / 180.0)))
        scale = np.float32(1.0 / float(persp))
        k0, k1 = np.float32(np.float32(cam.aspect) * scale), scale
        vp = [np.float32(v) for v in cam.viewport]
        out = []
        for ps in pss:
            ox, oy = (np.zeros(n, np.float32), np.zeros(n, np.float32))
            capi.check(lib, None, lib.rt_pass_offsets(n, ps, ox.ctypes.data_as(C.POINTER(C.c_float)), oy.ctypes.data_as(C.POINTER(C.c_float))), "rt_pass_offsets")
            fx = (np.arange(W, dtype=np.float32)[:, None] + ox[None, :]).astype(np.float32)
            fy = (np.arange(H, dtype=np.float32)[:, None] + oy[None, :]).astype(np.float32)
            n0 = (2.0 * (fx - vp[0]).astype(np.float32).astype(np.float64) / np.float64(vp[2]) - 1.0).astype(np.float32)
            n1 = (1.0 - 2.0 * (fy - vp[1]).astype(np.float32).astype(np.float64) / np.float64(vp[3])).astype(np.float32)
            out.append((torch.from_numpy((n0 * k0).astype(np.float32)).to(dev), torch.from_numpy((n1 * k1).astype(np.float32)).to(dev)))
        return out

    def route(n, terms, faces, ts):
        """the route without the query -> (H, W, 8); one torch operation per float32 operation of the definition"""
        acc = torch.zeros((H, W, 8), dtype=torch.float32, device=dev) if len(terms) > 1 else None
        for n0, n1 in terms:
            # rays in the order [H, W, sy, sx]: the order of the definition's sum
            x0 = n0[None, :, None, :].expand(H, W, n, n)
            y0 = n1[:, None, :, None].expand(H, W, n, n)
            S = torch.stack([((M[r, 0] * x0 + M[r, 1] * y0) + M[r, 2] * -1.0) + M[r, 3] * 1.0 for r in range(3)], dim=-1)
            D = (S - centre).reshape(-1, 3).contiguous()
            O = centre.expand(D.shape[0], 3).contiguous()
            capi.check(lib, ctx.handle, lib.rt_closest_hits_device(ctx.handle, D.shape[0], O.data_ptr(), D.data_ptr(), faces.data_ptr(), ts.data_ptr(),
                                                                   C.c_void_p(sp)), "rt_closest_hits_device")
            hit = faces >= 0
            v = torch.zeros((D.shape[0], 8), dtype=torch.float32, device=dev)
            f = faces.clamp(min=0).long()
            v[:, 0] = hit.float()
            v[:, 1] = torch.where(hit, ts, torch.zeros_like(ts))
            v[:, 2:8] = torch.where(hit[:, None], table[f], torch.zeros((1, 6), dtype=torch.float32, device=dev))
            v = v.view(H, W, n, n, 8)
            if n == 1:
                g = v[:, :, 0, 0]
            else:
                g = torch.zeros((H, W, 8), dtype=torch.float32, device=dev)
                for sy in range(n):
                    for sx in range(n):
                        g = g + v[:, :, sy, sx]
                g = g / float(n * n)
            acc = g if acc is None else acc + g
        return acc / float(len(terms)) if len(terms) > 1 else acc

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

    rec = {"scene": scene, "size": [W, H], "reps": args.reps, "blocks": args.blocks, "cases": {}}
    for n, first, count in CASES:
        ctx.set_supersampling(n)
        ctx.set_passes(first, count)
        terms = raster_terms(n, range(first, first + count))
        out = torch.empty((H, W, 8), dtype=torch.float32, device=dev)
        faces = torch.empty(n * n * W * H, dtype=torch.int32, device=dev)
        ts = torch.empty(n * n * W * H, dtype=torch.float32, device=dev)

        def side_a():
            capi.check(lib, ctx.handle, lib.rt_gbuffer_device(ctx.handle, C.byref(cam), C.byref(p), out.data_ptr(), C.c_void_p(sp)), "rt_gbuffer_device")

        def side_b():
            return route(n, terms, faces, ts)

        with torch.cuda.stream(stream):
            side_a()
            want = side_b()
        stream.synchronize()
        differ = int((out.view(torch.int32) != want.contiguous().view(torch.int32)).any(dim=-1).sum().item())
        sides = {"a_gbuffer_query": side_a, "b_rays_closest_hits_fold": side_b}
        medians = {k: [] for k in sides}
        for _ in range(args.blocks):
            for k, call in sides.items():
                medians[k].append(statistics.median(events(call, args.reps)))
        g = {"n": n, "passes": [first, count], "sub_samples": n * n * count * W * H, "pixels_that_differ_from_the_route": differ,
             "covered_share": round(float(out[..., 0].double().mean().item()), 6)}
        for k, v in medians.items():
            med = statistics.median(v)
            g[k] = {"ms_block_medians": [round(x, 4) for x in v], "ms_median": round(med, 4), "ms_range": round(max(v) - min(v), 4),
                    "sub_samples_per_s": round(n * n * count * W * H / (med * 1e-3))}
        g["a_over_b"] = round(g["a_gbuffer_query"]["ms_median"] / g["b_rays_closest_hits_fold"]["ms_median"], 4)
        rec["cases"][f"n{n}_passes{first}_{count}"] = g
        del faces, ts, out, want
        torch.cuda.empty_cache()
    ctx.close()
    hs.close()
    print(json.dumps(rec), flush=True)


def run_child(cmd, cwd, limit, what):
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=cwd)
    except subprocess.TimeoutExpired:
        print(f"gbuffer_timing: {what} ran out of its {limit} s; stopping", file=sys.stderr)
        return 124, None
    sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        print(f"gbuffer_timing: {what} failed with status {r.returncode}; stopping", file=sys.stderr)
        return (r.returncode if r.returncode > 0 else 1), None
    return 0, json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def bench(args):
    trees = (("parent", os.path.abspath(args.bench)), ("new", ROOT))
    runs = []
    for scene in args.scenes.split(","):
        for rnd in range(1, args.rounds + 1):
            for build, root in trees:
                cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup)]
                if scene != "cube":
                    cmd += ["--scene", scene]
                status, line = run_child(cmd, root, args.limit, f"bench.py {scene} {build} round {rnd}")
                if status:
                    return status
                run = {"scene": scene, "round": rnd, "build": build}
                run.update({k: line[k] for k in ("ms_per_step", "value", "rays_per_frame") if k in line})
                print(json.dumps(run), flush=True)
                runs.append(run)
    summary = {}
    for scene in args.scenes.split(","):
        ms = {b: [r["ms_per_step"] for r in runs if r["scene"] == scene and r["build"] == b] for b in ("parent", "new")}
        new_med = statistics.median(ms["new"])
        summary[scene] = {"parent_median_ms": round(statistics.median(ms["parent"]), 4), "new_median_ms": round(new_med, 4),
                          "parent_min_ms": min(ms["parent"]), "parent_max_ms": max(ms["parent"]), "new_min_ms": min(ms["new"]), "new_max_ms": max(ms["new"]),
                          "parent_spread_ms": round(max(ms["parent"]) - min(ms["parent"]), 4),
                          "new_median_inside_parent_range": min(ms["parent"]) <= new_med <= max(ms["parent"]),
                          "rays_per_frame_equal_in_all_runs": len({r.get("rays_per_frame") for r in runs if r["scene"] == scene}) == 1}
    out = {"how": f"python bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup} [--scene dodge]: a built tree of the parent commit and this tree, "
                  f"alternating parent / new, {args.rounds} rounds per scene, every run a process of its own",
           "summary": summary, "runs": runs}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(summary), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cube,dodge")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--bench", metavar="PARENT_ROOT")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--step", help="(internal) run one scene in this process")
    args = ap.parse_args()
    if args.step:
        scene_step(args, args.step)
        return 0
    if args.bench:
        return bench(args)
    records = []
    for scene in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", scene, "--size", str(args.size[0]), str(args.size[1]), "--reps", str(args.reps),
               "--blocks", str(args.blocks)]
        status, rec = run_child(cmd, ROOT, args.limit, scene)
        if status:
            return status
        print(json.dumps(rec), flush=True)
        records.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
