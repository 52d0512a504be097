"""Several builds of the library on the benchmark, alternating in one session (GPU only): plain `bench.py --gpus 1 --steps 200 --warmup 10
[--scene dodge]`, --rounds rounds of every library in the order given per scene, every run a process of its own under a time limit; the
library is chosen with RT_LIB (the name `shipped` stands for the tree's own library, RT_LIB unset), bench.py and the Python package are this
tree's.  The first library is the one the others are held against: for each other library the record says whether every run, and whether its
median, lies below the first library's fastest run.  --dump adds one `bench.py --dump-outputs` run of the first and the last library per
scene and compares rgb.npy / rgb_u8.npy byte for byte and the `rays` blocks.  The first child that fails or runs out of time ends the tool.

    python tools/shade_rows_ab.py --lib parent=PATH --lib rows=PATH ... --lib shipped [--scenes cube dodge] [--rounds 4] [--dump] [--out FILE]
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
    ap.add_argument("--lib", action="append", required=True, help="NAME=PATH, or `shipped`")
    ap.add_argument("--scenes", nargs="+", default=["cube", "dodge"], choices=["cube", "dodge"])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--limit", type=int, default=150)
    ap.add_argument("--dump", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    libs = []
    for spec in args.lib:
        name, _, path = spec.partition("=")
        libs.append((name, os.path.abspath(path) if path else None))
    assert len(libs) >= 2 and len({n for n, _ in libs}) == len(libs)
    rec = {"what": "builds of the library on one MI355X, alternating in one session in the order of `libs`; bench: python bench.py --gpus 1 --steps 200 "
                   "--warmup 10 [--scene dodge], every run a process of its own; the library is chosen with RT_LIB, bench.py and the Python package are "
                   "this tree's.  Every library is held against the first.",
           "libs": [n for n, _ in libs], "rounds": args.rounds, "bench": {}}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rec, f, indent=1)

    try:
        for scene in args.scenes:
            runs = {n: [] for n, _ in libs}
            rays = set()
            for _ in range(args.rounds):
                for name, lib in libs:
                    j = bench(lib, ["--steps", "200", "--warmup", "10", "--scene", scene], args.limit)
                    runs[name].append(j["ms_per_step"])
                    rays.add(j["rays_per_frame"])
                    print(scene, name, j["ms_per_step"], flush=True)
            base = runs[libs[0][0]]
            b = {"rays_per_frame_equal_in_all_runs": len(rays) == 1, "rays_per_frame": sorted(rays)[0]}
            for name, _ in libs:
                r = runs[name]
                b[name] = {"runs_ms": r, "median_ms": round(statistics.median(r), 4), "min_ms": min(r), "max_ms": max(r)}
                if r is not base:
                    b[name].update({"median_gain_ms": round(statistics.median(base) - statistics.median(r), 4), "every_run_below_first_min": max(r) < min(base),
                                    "median_below_first_min": statistics.median(r) < min(base), "max_not_above_first_max": max(r) <= max(base)})
                else:
                    b[name]["spread_ms"] = round(max(r) - min(r), 4)
            rec["bench"][scene] = b
            print(json.dumps({scene: b}), flush=True)
            save()
        if args.dump:
            rec["outputs"] = {}
            sides = (libs[0], libs[-1])
            for scene in args.scenes:
                with tempfile.TemporaryDirectory() as tmp:
                    js = {}
                    for name, lib in sides:
                        js[name] = bench(lib, ["--steps", "20", "--warmup", "2", "--scene", scene, "--dump-outputs", os.path.join(tmp, name)], args.limit)
                    a, z = sides[0][0], sides[1][0]
                    rec["outputs"][scene] = {f: filecmp.cmp(os.path.join(tmp, a, f), os.path.join(tmp, z, f), shallow=False) for f in ("rgb.npy", "rgb_u8.npy")}
                    rec["outputs"][scene]["rays_blocks_equal"] = js[a]["rays"] == js[z]["rays"]
                    rec["outputs"][scene]["compared"] = [a, z]
                print(json.dumps({scene: rec["outputs"][scene]}), flush=True)
            save()
    except subprocess.TimeoutExpired as e:
        print(f"shade_rows_ab: a run exceeded its limit ({e.timeout} s); stopping", file=sys.stderr)
        return 124
    return 0


if __name__ == "__main__":
    sys.exit(main())
