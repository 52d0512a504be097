"""The denoiser (rt_denoise_device) against a plain device-to-device copy of the bytes an iteration must move (GPU only).

Per channel count (3, then 1) a seeded synthetic 1920 x 1080 image and geometry buffers (a covered disc with a depth step, two normals and
two albedos, empty outside) are filtered with rt_default_denoise_params' sigmas.  In one process, on one stream, from torch events after
warm-up, --blocks blocks of --reps repetitions per side, alternating:
  call(n), n = 1 .. 5   rt_denoise_device with n iterations (the guide launch and n iteration launches), for the product library (every
                        iteration takes the plain-tap kernel k_atrous) and, where it was built, the A/B library whose iterations 0 and 1
                        (steps 1 and 2) take the LDS-staged kernel k_atrous_lds:
                            make -C raytracer-in-cpp_amd/csrc ab AB_FLAGS=-DRT_DENOISE_STAGED_STEPS=3
  copy                  one torch copy_ of a buffer of HALF the bytes an iteration must move at minimum -- it reads the working image (16 or
                        4 bytes per pixel) and two guide records (32) and writes the working image: 64 or 40 bytes per pixel -- so that the copy's
                        read plus write traffic is that minimum.
Iteration k >= 1 alone is call(k + 1) - call(k); iteration 0 is reported with the guide launch, as call(1).  The figure of merit is an
iteration's time over the copy's.  Both libraries must return the same bits.

Every channel count runs in a child process of its own under a time limit (--limit seconds); the first child that fails or runs out of
time ends the run with its status.

    python tools/denoise_timing.py [--size 1920 1080] [--reps 30] [--blocks 3] [--limit 300] [--out FILE]
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
AB_LIB = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "librt_mi355x_ab.so")
ITERATIONS = 5


def inputs(np, W, H, ch):
    rng = np.random.default_rng(17)
    img = rng.random((H, W, ch), dtype=np.float32)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    inside = (x - W / 2) ** 2 + (y - H / 2) ** 2 < (0.45 * H) ** 2
    g = np.zeros((H, W, 8), np.float32)
    g[..., 0] = 1.0
    g[..., 1] = np.where(x < W / 2, 1.5, 2.25) + y / H * 0.25
    g[..., 2:5] = np.where((y < H / 2)[..., None], np.float32([0.0, 0.0, 1.0]), np.float32([0.6, 0.0, 0.8]))
    g[..., 5:8] = np.where(((x // 200) % 2 == 0)[..., None], np.float32([0.75, 0.5, 0.25]), np.float32([0.5, 0.5, 0.625]))
    g[~inside] = 0.0
    return img, g


def channel_step(args, ch):
    import numpy as np
    import torch
    import rtpkg
    pkg = rtpkg.load()
    capi = pkg.capi
    dev = torch.device("cuda", 0)
    W, H = args.size
    img, g = inputs(np, W, H, ch)
    t_img, t_g = torch.from_numpy(img).to(dev), torch.from_numpy(g).to(dev)
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)

    libs = {"plain_taps": pkg.load_library()}
    if os.path.exists(AB_LIB):
        libs["lds_staged_steps_1_2"] = capi.load_library(AB_LIB)
    ctxs = {}
    for name, lib in libs.items():
        h = C.c_void_p()
        assert lib.rt_create(C.byref(h), 0) == capi.RT_OK
        ctxs[name] = h
    need = libs["plain_taps"].rt_denoise_scratch_bytes(W, H, ch)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty_like(t_img)
    min_bytes = W * H * ((16 if ch == 3 else 4) * 2 + 32)
    src, dst = torch.empty(min_bytes // 2, dtype=torch.uint8, device=dev), torch.empty(min_bytes // 2, dtype=torch.uint8, device=dev)

    def call(name, n):
        p = pkg.denoise_params(iterations=n)
        lib, h = libs[name], ctxs[name]

        def run():
            capi.check(lib, h, lib.rt_denoise_device(h, t_img.data_ptr(), ch, t_g.data_ptr(), W, H, C.byref(p), scratch.data_ptr(), out.data_ptr(), sp),
                       "rt_denoise_device")
        return run

    def events(fn, reps):
        with torch.cuda.stream(stream):
            for _ in range(3):
                fn()
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
            marks[0].record(stream)
            for k in range(reps):
                fn()
                marks[k + 1].record(stream)
        marks[-1].synchronize()
        return [marks[k].elapsed_time(marks[k + 1]) for k in range(reps)]

    # the two libraries agree, bit for bit
    results = {}
    for name in libs:
        call(name, ITERATIONS)()
        stream.synchronize()
        results[name] = out.cpu().numpy().view(np.uint32).copy()
    equal = all(np.array_equal(r, results["plain_taps"]) for r in results.values())

    sides = {"copy": lambda: dst.copy_(src)}
    for name in libs:
        for n in range(1, ITERATIONS + 1):
            sides[f"{name}:{n}"] = call(name, n)
    medians = {k: [] for k in sides}
    for _ in range(args.blocks):
        for k, fn in sides.items():
            medians[k].append(statistics.median(events(fn, args.reps)))
    ms = {k: statistics.median(v) for k, v in medians.items()}
    rng_ = {k: max(v) - min(v) for k, v in medians.items()}
    rec = {"size": [W, H], "channels": ch, "pixels": W * H, "covered_share": round(float((g[..., 0] > 0).mean()), 4), "reps": args.reps, "blocks": args.blocks,
           "libraries_equal_bits": bool(equal), "min_bytes_per_iteration": min_bytes,
           "copy": {"bytes_copied": min_bytes // 2, "ms_median": round(ms["copy"], 4), "ms_range": round(rng_["copy"], 4),
                    "traffic_GB_per_s": round(min_bytes / (ms["copy"] * 1e-3) / 1e9, 1)},
           "variants": {}}
    for name in libs:
        v = {"ms_call": {}, "ms_range": {}, "ms_iteration": {}, "iteration_over_copy": {}}
        for n in range(1, ITERATIONS + 1):
            v["ms_call"][str(n)] = round(ms[f"{name}:{n}"], 4)
            v["ms_range"][str(n)] = round(rng_[f"{name}:{n}"], 4)
        for k in range(1, ITERATIONS):                         # iteration k alone: call(k + 1) - call(k)
            d = ms[f"{name}:{k + 1}"] - ms[f"{name}:{k}"]
            v["ms_iteration"][f"k={k} step={1 << k}"] = round(d, 4)
            v["iteration_over_copy"][f"k={k} step={1 << k}"] = round(d / ms["copy"], 2)
        v["ms_call_5_per_iteration"] = round(ms[f"{name}:{ITERATIONS}"] / ITERATIONS, 4)
        v["ms_guide_plus_iteration_0"] = round(ms[f"{name}:1"], 4)
        rec["variants"][name] = v
    for name, lib in libs.items():
        lib.rt_destroy(ctxs[name])
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--step", type=int, help="(internal) run one channel count in this process")
    args = ap.parse_args()
    if args.step:
        channel_step(args, args.step)
        return 0
    records = []
    for ch in (3, 1):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(ch), "--size", str(args.size[0]), str(args.size[1]), "--reps", str(args.reps),
               "--blocks", str(args.blocks)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"denoise_timing: {ch} channel(s) ran out of its {args.limit} s; stopping", file=sys.stderr)
            return 124
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print(f"denoise_timing: {ch} channel(s) failed with status {r.returncode}; stopping", file=sys.stderr)
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
