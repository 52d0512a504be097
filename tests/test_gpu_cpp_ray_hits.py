"""rtamd::Flyscene::rayHits on a real MI355X, through the group `ray_hits` of tools/flyscene_check.cpp: the member returns, bit for bit,
what the Python mirror (Context.ray_hits on the same scene) returns for the same rays, slot counts and bounds, and refuses what the group
expects it to refuse (the child's exit status).  tests/test_gpu_ray_hits.py holds the mirror against the definition."""
import subprocess

import numpy as np
import pytest

import facade_cases as fc
import switch_table
from facade_cases import H, W, same
from test_gpu_ray_queries import In

pytestmark = pytest.mark.gpu

F = np.float32
TIMEOUT = 14
KS = (1, 3, 8)
T_MAX = (float("inf"), 2.5)


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_ray_hits(rt, scenes, tmp_path, name):
    paths = fc.scene_paths(scenes, tmp_path)
    fs = rt.Flyscene(scene_path=paths[name])
    fs.initialize(W, H, True, False)
    try:
        o, d, _ = fc.rays()
        o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
        n = len(o)
        try:
            status, out, err = fc.run("ray_hits", paths[name], {"O": o, "D": d, "ks": np.array(KS, np.int32), "t_max": np.array(T_MAX, F)}, str(tmp_path), TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.exit(f"flyscene_check ray_hits on {name} ran into its time limit of {TIMEOUT} s: nothing more is started on the device", 3)
        if status < 0 or status in (124, 134, 137, 139):                 # killed by a signal: a fault, an abort
            pytest.exit(f"flyscene_check ray_hits on {name} ended with {status}: nothing more is started on the device\n{err[-3000:]}", 3)
        assert status == 0, f"flyscene_check ray_hits on {name} ended with {status}:\n{err[-3000:]}"
        io, idr = In(rt, o), In(rt, d)
        several = 0
        for k in KS:
            for j, t_max in enumerate(T_MAX):
                f, t, c = fs.ctx.ray_hits(io.buf, idr.buf, k, t_max, n=n)
                fs.ctx.synchronize()
                f, t, c = f.to_numpy(np.int32, (n, k)), t.to_numpy(F, (n, k)), c.to_numpy(np.int32, (n,))
                assert same(out[f"faces_{k}_{j}"], f) and same(out[f"ts_{k}_{j}"], t) and same(out[f"counts_{k}_{j}"], c), (name, k, t_max)
                assert (c > 0).any() and (c == 0).any(), (name, k, t_max)
                several += int((c >= 2).sum())
        assert several > 0
    finally:
        fs.ctx.close()
        fs.scene.close()
