"""The temporal reprojection (rt_reproject_device) beside the guided upsample and the time of its compulsory bytes, and one animation step
of 2 x 2 ambient occlusion with and without it against the 8 x 8 occlusion it stands in for (GPU only).

Step "kernel": a seeded synthetic 1920 x 1080 image and geometry buffers (denoise_timing.py's: a covered disc with a depth step, two normals
and two albedos, empty outside), used as the current frame and as the history, every length 8.  In one process, on one stream, from torch
events after warm-up, --blocks blocks of --reps repetitions per side, alternating:
  reproject:C:identity      rt_reproject_device with rt_default_reproject_params, C = 1 and 3 channels, the identity map (one tap per pixel)
  reproject:C:yaw           ... with the map of the yaw cameras 0.42 -> 0.40 of that size (four taps at fractional places, some outside)
  upsample                  rt_upsample_device at s = 2, RGB, on the same frame (the low image and buffers are the pixels (2I, 2J))
  copy:C                    one torch copy_ of HALF the bytes the call must move at minimum: it reads the current image and buffers, the
                            history image, buffers and lengths once and writes the image and the lengths: 12 C + 64 + 2 bytes per pixel
The record also states the time those bytes would take at the rate k_resolve achieves (50 MB in 12.5 us: DESIGN.md 6, Frame edges).
Step "pipeline": dodgeColorTest at 1920 x 1080, every pixel a point, the points built once on the device; the previous frame is the camera
at yaw 0.40, the current one at yaw 0.42:
  step_without              rt_gbuffer_device + 2 x 2 rt_ambient_occlusion_device of the current camera
  step_with                 the same + rt_reproject_device of the previous frame's occlusion and buffers (one channel)
  occlusion8                8 x 8 rt_ambient_occlusion_device on the same points
A side's figure is the median of its block medians, its spread their range.

Every step runs in a child process of its own under a time limit (--limit seconds); the first child that fails or runs out of time ends the
run with its status.

    python tools/reproject_timing.py [--size 1920 1080] [--reps 20] [--blocks 3] [--limit 300] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
RADIUS, SEED = 0.5, 7
RESOLVE_BYTES_PER_S = 50e6 / 12.5e-6


def kernel_step(args):
    import numpy as np
    import torch
    import rtpkg
    import denoise_timing
    from upsample_timing import measure
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    W, H = args.size
    img, g = denoise_timing.inputs(np, W, H, 3)
    t_img, t_g = torch.from_numpy(img).to(dev), torch.from_numpy(g).to(dev)
    t_one = t_img[..., 0].contiguous()
    t_hist, t_hist1, t_gh = t_img.clone(), t_one.clone(), t_g.clone()
    t_len = torch.full((H, W), 8, dtype=torch.uint8, device=dev)
    t_low, t_gl = t_img[::2, ::2].contiguous(), t_g[::2, ::2].contiguous()
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    ctx = pkg.Context(0)
    lib, hnd = ctx.lib, ctx.handle
    rp, up = pkg.reproject_params(), pkg.upsample_params(2)
    out3, out1, up_out = torch.empty_like(t_img), torch.empty_like(t_one), torch.empty_like(t_img)
    len_out = torch.empty_like(t_len)
    maps = {"identity": pkg.reproject_map(pkg.default_camera(W, H, 0.4), pkg.default_camera(W, H, 0.4)),
            "yaw": pkg.reproject_map(pkg.default_camera(W, H, 0.42), pkg.default_camera(W, H, 0.40))}

    def reproject(ch, which):
        m = (C.c_float * 12)(*[float(v) for v in maps[which].reshape(12)])
        cur, hist, out = (t_img, t_hist, out3) if ch == 3 else (t_one, t_hist1, out1)

        def run():
            capi.check(lib, hnd, lib.rt_reproject_device(hnd, cur.data_ptr(), ch, t_g.data_ptr(), hist.data_ptr(), t_gh.data_ptr(), t_len.data_ptr(), W, H, m,
                                                         C.byref(rp), out.data_ptr(), len_out.data_ptr(), sp), "rt_reproject_device")
        return run

    def upsample():
        capi.check(lib, hnd, lib.rt_upsample_device(hnd, t_low.data_ptr(), 3, t_gl.data_ptr(), t_g.data_ptr(), W, H, C.byref(up), up_out.data_ptr(), None, sp),
                   "rt_upsample_device")

    min_bytes = {ch: W * H * (8 * ch + 4 * ch + 64 + 2) for ch in (1, 3)}        # cur + hist in, out; two sets of buffers; lengths in and out
    copies = {ch: (torch.empty(min_bytes[ch] // 2, dtype=torch.uint8, device=dev), torch.empty(min_bytes[ch] // 2, dtype=torch.uint8, device=dev)) for ch in (1, 3)}
    sides = {f"reproject:{ch}:{which}": reproject(ch, which) for ch in (1, 3) for which in ("identity", "yaw")}
    sides["upsample"] = upsample
    for ch in (1, 3):
        sides[f"copy:{ch}"] = lambda ch=ch: copies[ch][1].copy_(copies[ch][0])
    reproject(3, "yaw")()
    stream.synchronize()
    kept = float((len_out[t_g[..., 0] > 0] > 1).float().mean().item())
    m = measure(torch, stream, sides, args)
    rec = {"step": "kernel", "size": [W, H], "covered_share": round(float((g[..., 0] > 0).mean()), 4), "yaw_history_kept_share_of_covered": round(kept, 4),
           "reps": args.reps, "blocks": args.blocks, "min_bytes": min_bytes, "sides": m,
           "ms_of_min_bytes_at_k_resolve_rate": {ch: round(min_bytes[ch] / RESOLVE_BYTES_PER_S * 1e3, 4) for ch in (1, 3)}}
    for ch in (1, 3):
        for which in ("identity", "yaw"):
            t = m[f"reproject:{ch}:{which}"]["ms_median"]
            rec[f"reproject:{ch}:{which}"] = {"over_upsample": round(t / m["upsample"]["ms_median"], 3),
                                             "over_k_resolve_rate": round(t / (min_bytes[ch] / RESOLVE_BYTES_PER_S * 1e3), 3),
                                             "over_copy": round(t / m[f"copy:{ch}"]["ms_median"], 3),
                                             "traffic_GB_per_s": round(min_bytes[ch] / (t * 1e-3) / 1e9, 1)}
    ctx.close()
    print(json.dumps(rec), flush=True)


def pipeline_step(args):
    import numpy as np
    import torch
    import rtpkg
    from upsample_timing import measure
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    W, H = args.size
    hs = pkg.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", "dodgeColorTest.obj"), 1000, 15)
    ctx = pkg.Context(0)
    ctx.upload(hs)
    lib, hnd = ctx.lib, ctx.handle
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    prev, cam = pkg.default_camera(W, H, 0.40), pkg.default_camera(W, H, 0.42)
    prm = pkg.make_params(W, H)

    def points(c):
        pts = np.empty((W * H, 3), np.float32)
        capi.check(lib, hnd, lib.rt_primary_points(hnd, C.byref(c), W, H, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
        centre = torch.tensor(list(c.center), dtype=torch.float32, device=dev)
        dirs = (torch.from_numpy(pts).to(dev) - centre).contiguous()
        origins = centre.expand(W * H, 3).contiguous()
        with torch.cuda.stream(stream):
            faces, ts = ctx.closest_hits(origins, dirs)
            P, N = ctx.hit_points(origins, dirs, faces, ts)
        stream.synchronize()
        return P, N, faces >= 0

    def occlusion(P, N, grid, seed, ao):
        def run():
            capi.check(lib, hnd, lib.rt_ambient_occlusion_device(hnd, W * H, P.data_ptr(), N.data_ptr(), grid, RADIUS, seed, None, ao.data_ptr(), sp),
                       "rt_ambient_occlusion_device")
        return run

    def gbuffer(c, out):
        def run():
            capi.check(lib, hnd, lib.rt_gbuffer_device(hnd, C.byref(c), C.byref(prm), out.data_ptr(), sp), "rt_gbuffer_device")
        return run

    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    Pp, Np, _ = points(prev)
    P, N, hit = points(cam)
    g_prev, g_cur, ao_prev, ao_cur, ao8, acc = new(H, W, 8), new(H, W, 8), new(W * H), new(W * H), new(W * H), new(W * H)
    len_prev, len_out = torch.ones((H, W), dtype=torch.uint8, device=dev), new(H, W, dtype=torch.uint8)
    gbuffer(prev, g_prev)()
    occlusion(Pp, Np, 2, SEED, ao_prev)()
    stream.synchronize()
    rp = pkg.reproject_params()
    m12 = (C.c_float * 12)(*[float(v) for v in pkg.reproject_map(cam, prev).reshape(12)])

    def reproject():
        capi.check(lib, hnd, lib.rt_reproject_device(hnd, ao_cur.data_ptr(), 1, g_cur.data_ptr(), ao_prev.data_ptr(), g_prev.data_ptr(), len_prev.data_ptr(), W, H,
                                                     m12, C.byref(rp), acc.data_ptr(), len_out.data_ptr(), sp), "rt_reproject_device")

    without = [gbuffer(cam, g_cur), occlusion(P, N, 2, SEED + 1, ao_cur)]
    sides = {"step_without": lambda: [c() for c in without], "step_with": lambda: [c() for c in without + [reproject]], "occlusion8": occlusion(P, N, 8, SEED, ao8)}
    parts = {"gbuffer": without[0], "occlusion2": without[1], "reproject": reproject}
    m = measure(torch, stream, sides, args)
    mp = measure(torch, stream, parts, args)
    stream.synchronize()
    cov = hit.view(H, W)
    rms = lambda a: round(float(torch.sqrt(((a.view(H, W) - ao8.view(H, W))[cov].to(torch.float64) ** 2).mean()).item()), 5)
    rec = {"step": "pipeline", "scene": "dodge", "size": [W, H], "radius": RADIUS, "points": W * H, "hits": int(hit.sum().item()), "reps": args.reps,
           "blocks": args.blocks, "sides": m, "parts": mp,
           "step_with_over_without": round(m["step_with"]["ms_median"] / m["step_without"]["ms_median"], 3),
           "occlusion8_over_step_with": round(m["occlusion8"]["ms_median"] / m["step_with"]["ms_median"], 3),
           "history_kept_share_of_hits": round(float((len_out[cov] > 1).float().mean().item()), 4),
           "rms_from_occlusion8_over_hits": {"single_2x2": rms(ao_cur), "two_frames_accumulated": rms(acc)}}
    ctx.close()
    hs.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--step", help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step:
        {"kernel": kernel_step, "pipeline": pipeline_step}[args.step](args)
        return 0
    records = []
    for step in ("kernel", "pipeline"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--size", str(args.size[0]), str(args.size[1]), "--reps", str(args.reps),
               "--blocks", str(args.blocks)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"reproject_timing: step {step} ran out of its {args.limit} s; stopping", file=sys.stderr)
            return 124
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print(f"reproject_timing: step {step} failed with status {r.returncode}; stopping", file=sys.stderr)
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
