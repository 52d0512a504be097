"""rtamd::Flyscene::closestPoints on a real MI355X, through the group `closest_points` of tools/flyscene_check.cpp: the member returns, bit
for bit, what the Python mirror (Context.closest_points on the same scene) returns for the same points and radii, and refuses what the
group expects it to refuse (the child's exit status).  tests/test_gpu_closest_points.py holds the mirror against the definition."""
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
RADII = (float("inf"), 0.0, 0.35)


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def points(fs):
    """a grid round the scene, its first vertices, a far point and a NaN"""
    box = np.asarray(fs.scene.info()["root_box"], F)
    ax = [np.linspace(box[q] - F(0.2), box[3 + q] + F(0.2), m, dtype=F) for q, m in enumerate((6, 5, 5))]
    grid = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    verts = fs.scene.arrays()["tri_verts"][:8].reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([grid, verts, [[1e4, -1e4, 1e4]], [[np.nan, 0, 0]]]), F)


@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_closest_points(rt, scenes, tmp_path, name):
    paths = fc.scene_paths(scenes, tmp_path)
    fs = rt.Flyscene(scene_path=paths[name])
    fs.initialize(W, H, True, False)
    try:
        P = points(fs)
        try:
            status, out, err = fc.run("closest_points", paths[name], {"P": P, "radii": np.array(RADII, F)}, str(tmp_path), TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.exit(f"flyscene_check closest_points on {name} ran into its time limit of {TIMEOUT} s: nothing more is started on the device", 3)
        if status < 0 or status in (124, 134, 137, 139):                 # killed by a signal: a fault, an abort
            pytest.exit(f"flyscene_check closest_points on {name} ended with {status}: nothing more is started on the device\n{err[-3000:]}", 3)
        assert status == 0, f"flyscene_check closest_points on {name} ended with {status}:\n{err[-3000:]}"
        dev = In(rt, P)
        none = 0
        for k, r in enumerate(RADII):
            f, d, q = fs.ctx.closest_points(dev.buf, r, n=len(P))
            fs.ctx.synchronize()
            f, d, q = f.to_numpy(np.int32, (len(P),)), d.to_numpy(F, (len(P),)), q.to_numpy(F, (len(P), 3))
            assert same(out[f"faces_{k}"], f) and same(out[f"dist2_{k}"], d) and same(out[f"closest_{k}"], q), (name, r)
            none += int((f == -1).sum())
            assert (f >= 0).any(), (name, r)
        assert none > 0
    finally:
        fs.ctx.close()
        fs.scene.close()
