"""rtamd::Flyscene::indirectDiffuse on a real MI355X, through the group `indirect` of tools/flyscene_check.cpp: the member returns, bit for
bit, what tests/indirect_ref.py gets from the definition for this object's lights -- over the CPU checker where that is affordable, over
rt_closest_hits / rt_light_strikes for the large grid -- and refuses what the group expects it to refuse (the child's exit status)."""
import subprocess

import numpy as np
import pytest

import facade_cases as fc
import indirect_ref as ir
import switch_table
from facade_cases import H, W, same

pytestmark = pytest.mark.gpu

F = np.float32
TIMEOUT = 14
ONE = ((-1.0, 1.0, 1.0),)
TWO = ((-1.0, 1.0, 1.0), (1.5, 0.5, -1.0))
GRIDS, SEEDS = (1, 3, 16), (0, 7)
ORACLE_RAYS = 20000


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name", ["mixed", "dodge"])
def test_indirect_diffuse(rt, oracle, scenes, tmp_path, name):
    paths = fc.scene_paths(scenes, tmp_path)
    osc = oracle.load_scene(paths[name])
    fs = rt.Flyscene(scene_path=paths[name])
    fs.initialize(W, H, False, True)
    try:
        _, (P, N) = fc.frame_points(oracle, osc, W, H)
        assert 0 < int(ir.ao_ref.is_point(N).sum()) < len(P), "the frame must hold hits and misses"
        arrays = {"P": P, "N": N, "one": fc.vec3(ONE), "two": fc.vec3(TWO)}
        try:
            status, out, err = fc.run("indirect", paths[name], arrays, str(tmp_path), TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.exit(f"flyscene_check indirect on {name} ran into its time limit of {TIMEOUT} s: nothing more is started on the device", 3)
        if status < 0 or status in (124, 134, 137, 139):                 # killed by a signal: a fault, an abort
            pytest.exit(f"flyscene_check indirect on {name} ended with {status}: nothing more is started on the device\n{err[-3000:]}", 3)
        assert status == 0, f"flyscene_check indirect on {name} ended with {status}:\n{err[-3000:]}"
        color = tuple(rt.make_lights(ONE, area=False).color)               # the colour of an object's lights
        data = ir.SceneData(osc)
        tracers = {"oracle": ir.OracleTracer(osc), "library": ir.LibraryTracer(rt, fs.ctx)}
        shown = 0
        for li, pos in enumerate((ONE, TWO)):
            for m in GRIDS:
                by = "oracle" if len(P) * m * m <= ORACLE_RAYS else "library"
                for seed in SEEDS:
                    want = ir.gather(tracers[by], data, P, N, m, seed, pos, color)
                    got = out[f"rgb_{li + 1}_{m}_{seed}"]
                    assert got.shape == (len(P), 3) and same(got, want), (name, li, m, seed)
                    shown += int((want != 0).any())
        assert shown >= 6, "the fixture must hold points that receive indirect light"
    finally:
        fs.ctx.close()
        fs.scene.close()
        osc.close()
