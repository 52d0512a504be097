"""The parent's library against this tree's on the benchmark, alternating in one session (GPU only): plain `bench.py --gpus 1 --steps 200
--warmup 10 [--scene dodge]`, --rounds rounds of parent / new per scene, every run a process of its own under a time limit; the library is
chosen with RT_LIB, bench.py and the Python package are this tree's.  --dump adds one `bench.py --dump-outputs` run per library and scene and
compares rgb.npy / rgb_u8.npy byte for byte and the `rays` blocks; --full adds one `bench.py --full --no-cpu-baseline` per library and
records cfg4's ms_per_step.  The first child that fails or runs out of time ends the tool with its status.

The binding asks every library for rt_set_frame_overlap, which the parent's sources do not have: its library for this comparison is the
parent's sources plus that one symbol as an empty function.

    python tools/frame_overlap_ab.py --parent-lib PATH [--scenes cube dodge] [--rounds 8] [--dump] [--full] [--probe FILE] [--out FILE]
"""
import argparse
import filecmp
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(lib, extra, limit):
    env = dict(os.environ)
    env.pop("RT_LIB", None)
    if lib:
        env["RT_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + extra, capture_output=True, text=True, timeout=limit, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-3000:])
        raise SystemExit(r.returncode if r.returncode > 0 else 1)
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--scenes", nargs="+", default=["cube", "dodge"], choices=["cube", "dodge"])
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--limit", type=int, default=150)
    ap.add_argument("--dump", action="store_true")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--probe", help="profiles/frame_overlap_probe.json: the two-context gain the headline is held against")
    ap.add_argument("--out")
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_lib)
    rec = {"what": "the parent's library (its sources plus rt_set_frame_overlap as an empty function, which the binding asks for) against this commit's on one "
                   "MI355X, alternating in one session; bench: python bench.py --gpus 1 --steps 200 --warmup 10 [--scene dodge], every run a process of its "
                   "own; the library is chosen with RT_LIB, bench.py and the Python package are this tree's.",
           "bench": {}}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rec, f, indent=1)

    try:
        for scene in args.scenes:
            runs = {"parent": [], "new": []}
            rays = set()
            for _ in range(args.rounds):
                for side, lib in (("parent", parent), ("new", None)):
                    j = bench(lib, ["--steps", "200", "--warmup", "10", "--scene", scene], args.limit)
                    runs[side].append(j["ms_per_step"])
                    rays.add(j["rays_per_frame"])
                    print(scene, side, j["ms_per_step"], flush=True)
            p, n = runs["parent"], runs["new"]
            gain = statistics.median(p) - statistics.median(n)
            b = {"parent_median_ms": round(statistics.median(p), 4), "new_median_ms": round(statistics.median(n), 4), "parent_min_ms": min(p), "parent_max_ms": max(p),
                 "new_min_ms": min(n), "new_max_ms": max(n), "parent_spread_ms": round(max(p) - min(p), 4), "every_new_run_below_parent_min": max(n) < min(p),
                 "median_gain_ms": round(gain, 4), "new_median_not_above_parent_median_by_more_than_parent_range": statistics.median(n) <= statistics.median(p) + (max(p) - min(p)),
                 "rays_per_frame_equal_in_all_runs": len(rays) == 1, "parent_runs_ms": p, "new_runs_ms": n, "rays_per_frame": sorted(rays)[0]}
            if scene == "cube" and args.probe:
                probe = json.load(open(args.probe))["scenes"]["cube"]["median_gain_ms"]
                b["probe_two_context_gain_ms"] = probe
                b["median_gain_at_least_half_the_probes"] = gain >= 0.5 * probe
                b["median_gain_above_go_threshold"] = gain > 2 * 0.0083
            rec["bench"][scene] = b
            print(json.dumps({scene: b}), flush=True)
            save()
        if args.dump:
            rec["outputs"] = {}
            for scene in args.scenes:
                with tempfile.TemporaryDirectory() as tmp:
                    js = {}
                    for side, lib in (("parent", parent), ("new", None)):
                        js[side] = bench(lib, ["--steps", "20", "--warmup", "2", "--scene", scene, "--dump-outputs", os.path.join(tmp, side)], args.limit)
                    rec["outputs"][scene] = {f: filecmp.cmp(os.path.join(tmp, "parent", f), os.path.join(tmp, "new", f), shallow=False) for f in ("rgb.npy", "rgb_u8.npy")}
                    rec["outputs"][scene]["rays_blocks_equal"] = js["parent"]["rays"] == js["new"]["rays"]
                print(json.dumps({scene: rec["outputs"][scene]}), flush=True)
            save()
        if args.full:
            rec["full"] = {}
            for side, lib in (("parent", parent), ("new", None)):
                j = bench(lib, ["--steps", "200", "--warmup", "10", "--full", "--no-cpu-baseline"], 600)
                t = j["tree_scenes"]
                rec["full"][side] = {"cube_ms_per_step": j["ms_per_step"], "dodge_ms_per_step": t["dodge_1920x1080_d4_s64"]["ms_per_step"],
                                     "cfg4_ms_per_step": t["cfg4_wavy_3840x2160_d8_s256"]["ms_per_step"], "launches_per_frame": j.get("launches_per_frame")}
                print(side, json.dumps(rec["full"][side]), flush=True)
            save()
    except subprocess.TimeoutExpired as e:
        print(f"frame_overlap_ab: a run exceeded its limit ({e.timeout} s); stopping", file=sys.stderr)
        return 124
    return 0


if __name__ == "__main__":
    sys.exit(main())
