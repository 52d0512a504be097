"""rtamd::Flyscene::lightProbes and ::probeIrradiance on a real MI355X, through the group `probes` of tools/flyscene_check.cpp: the members
return, bit for bit, what the Python mirror (Flyscene.light_probes, Flyscene.probe_irradiance) returns for the same object -- the grid, the
coefficients, the lookup images at the viewport's size and at another -- and refuse what the group expects them to refuse (the child's
exit status).  One case is also held against tests/probe_ref.py, so that the two do not merely agree with each other."""
import subprocess

import numpy as np
import pytest

import facade_cases as fc
import indirect_ref as ir
import probe_ref as pr
import switch_table
from facade_cases import H, H2, W, W2, same

pytestmark = pytest.mark.gpu

F = np.float32
TIMEOUT = 14
ONE = ((-1.0, 1.0, 1.0),)
TWO = ((-1.0, 1.0, 1.0), (1.5, 0.5, -1.0))
# the cases of group_probes: name -> (dims, m, direct, margin, lights)
CASES = {"a": ((3, 2, 4), 3, False, 0.25, ONE), "b": ((2, 2, 2), 8, True, 0.0, TWO), "c": ((4, 1, 3), 16, True, 0.5, TWO), "d": ((1, 1, 1), 1, False, 0.0, ONE)}


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name", ["mixed", "dodge"])
def test_light_probes_and_probe_irradiance(rt, oracle, scenes, tmp_path, name):
    paths = fc.scene_paths(scenes, tmp_path)
    fs = rt.Flyscene(scene_path=paths[name])
    fs.initialize(W, H, False, True)
    osc = oracle.load_scene(paths[name])
    try:
        arrays = {"one": fc.vec3(ONE), "two": fc.vec3(TWO)}
        try:
            status, out, err = fc.run("probes", paths[name], arrays, str(tmp_path), TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.exit(f"flyscene_check probes on {name} ran into its time limit of {TIMEOUT} s: nothing more is started on the device", 3)
        if status < 0 or status in (124, 134, 137, 139):                 # killed by a signal: a fault, an abort
            pytest.exit(f"flyscene_check probes on {name} ended with {status}: nothing more is started on the device\n{err[-3000:]}", 3)
        assert status == 0, f"flyscene_check probes on {name} ended with {status}:\n{err[-3000:]}"
        lit = 0
        for case, (dims, m, direct, margin, lights) in CASES.items():
            fs.lights = list(lights)
            pg, coeff = fs.light_probes(dims, m, direct=direct, margin=margin)
            assert same(out[f"grid_{case}_origin"], np.array(list(pg.origin), F)) and same(out[f"grid_{case}_step"], np.array(list(pg.step), F)), (name, case)
            assert out[f"grid_{case}_dims"].tolist() == [float(x) for x in dims]
            assert out[f"coeff_{case}"].shape == (dims[0] * dims[1] * dims[2], 27) and same(out[f"coeff_{case}"], coeff), (name, case)
            img, small = fs.probe_irradiance(W, H, (pg, coeff)), fs.probe_irradiance(W2, H2, (pg, coeff))
            assert same(out[f"img_{case}"], img.reshape(-1, 3)) and same(out[f"small_{case}"], small.reshape(-1, 3)), (name, case)
            lit += int((img != 0).any())
            if case == "a":                                              # ... and the definition
                color = tuple(rt.make_lights(ONE, area=False).color)
                grid = pr.Grid.over(fs.scene.info()["root_box"], dims, margin)
                want = pr.probes(ir.OracleTracer(osc), ir.SceneData(osc), grid.positions(), m, lights, color, direct)
                assert same(coeff, want)
                (o, d, f, t), _ = pr.ir.ao_ref.camera_points(oracle, osc, W, H, 0.0)
                HP, HN = pr.ir.ao_ref.hit_points(o, d, f, t, osc.arrays()["face_normal"])
                assert same(img.reshape(-1, 3), pr.lookup(grid, want, HP, HN))
        assert lit >= 2, "the fixture must hold images that are lit"
    finally:
        fs.ctx.close()
        fs.scene.close()
        osc.close()


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n"
        w, h = (int(x) for x in f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)[::-1]


def test_the_cli_writes_the_lookup_image_of_the_python_mirror(rt, scenes, tmp_path):
    """rt_render --probes DX DY DZ M: the volume over the root box with the direct term and no margin, looked up by the frame's camera"""
    import os
    program = os.path.join(os.path.dirname(fc.PROGRAM), "rt_render")
    path = os.path.join(scenes, "dodgeColorTest.obj")
    w, h, dims, m = 72, 40, (3, 2, 4), 3
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(w, h, True, False)
    try:
        want = fs.probe_irradiance(w, h, fs.light_probes(dims, m, direct=True, margin=0.0))
    finally:
        fs.ctx.close()
        fs.scene.close()
    cli = [program, "--scene", path, "--size", str(w), str(h), "--samples", "2", "2", "--depth", "1", "--out", "cli.ppm"]
    r = subprocess.run(cli + ["--probes"] + [str(x) for x in dims] + [str(m)], input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = read_pfm(str(tmp_path / "cli.ppm.probes.pfm"))
    assert got.shape == (h, w, 3) and same(np.ascontiguousarray(got), want) and (want != 0).any()
    for bad in (["--probes", "3", "2", "4", "0"], ["--probes", "3", "2", "4", "17"], ["--probes", "0", "2", "4", "3"], ["--probes", "4096", "4096", "2", "3"]):
        r = subprocess.run(cli + bad, input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=60)
        assert r.returncode == 2, bad
