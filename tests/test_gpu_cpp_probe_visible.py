"""rtamd::Flyscene::probeIrradianceVisible on a real MI355X, through the group `probes_visible` of tools/flyscene_check.cpp: the member
returns, bit for bit, what the Python mirror (Flyscene.probe_irradiance with visible=True) returns for the same object -- at the viewport's
size and at another, beside the plain member -- and refuses what the group expects it to refuse (the child's exit status); rt_render
--probes-visible writes that image.  tests/test_gpu_probe_visible.py holds the mirror against the definition."""
import os
import subprocess

import numpy as np
import pytest

import facade_cases as fc
import switch_table
from facade_cases import H, H2, W, W2, same
from test_gpu_cpp_probes import read_pfm

pytestmark = pytest.mark.gpu

F = np.float32
TIMEOUT = 14
ONE = ((-1.0, 1.0, 1.0),)
# the cases of group_probes_visible: name -> (dims, m, margin); the direct term is on
CASES = {"a": ((6, 5, 5), 3, 0.0), "b": ((3, 1, 4), 2, 0.25), "c": ((1, 1, 1), 1, 0.0)}


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name", ["mixed", "dodge"])
def test_probe_irradiance_visible(rt, scenes, tmp_path, name):
    paths = fc.scene_paths(scenes, tmp_path)
    fs = rt.Flyscene(scene_path=paths[name])
    fs.initialize(W, H, False, True)
    try:
        try:
            status, out, err = fc.run("probes_visible", paths[name], {"one": fc.vec3(ONE)}, str(tmp_path), TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.exit(f"flyscene_check probes_visible on {name} ran into its time limit of {TIMEOUT} s: nothing more is started on the device", 3)
        if status < 0 or status in (124, 134, 137, 139):                 # killed by a signal: a fault, an abort
            pytest.exit(f"flyscene_check probes_visible on {name} ended with {status}: nothing more is started on the device\n{err[-3000:]}", 3)
        assert status == 0, f"flyscene_check probes_visible on {name} ended with {status}:\n{err[-3000:]}"
        fs.lights = list(ONE)
        differ = 0
        for case, (dims, m, margin) in CASES.items():
            probes = fs.light_probes(dims, m, direct=True, margin=margin)
            assert same(out[f"coeff_{case}"], probes[1]), (name, case)
            img, small = fs.probe_irradiance(W, H, probes, visible=True), fs.probe_irradiance(W2, H2, probes, visible=True)
            plain = fs.probe_irradiance(W, H, probes)
            assert same(out[f"visible_{case}"], img.reshape(-1, 3)) and same(out[f"small_{case}"], small.reshape(-1, 3)), (name, case)
            assert same(out[f"plain_{case}"], plain.reshape(-1, 3)), (name, case)
            differ += int(not same(img, plain))
            if case == "c":
                assert same(img, plain), "one probe: the point sees it or falls back to it"
        assert differ >= 1, "the fixture must hold an image in which blocked probes show"
    finally:
        fs.ctx.close()
        fs.scene.close()


def test_the_cli_writes_the_visible_lookup_of_the_python_mirror(rt, scenes, tmp_path):
    """rt_render --probes DX DY DZ M --probes-visible"""
    program = os.path.join(os.path.dirname(fc.PROGRAM), "rt_render")
    path = os.path.join(scenes, "dodgeColorTest.obj")
    w, h, dims, m = 72, 40, (6, 5, 5), 3
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(w, h, True, False)
    try:
        probes = fs.light_probes(dims, m, direct=True, margin=0.0)
        want, plain = fs.probe_irradiance(w, h, probes, visible=True), fs.probe_irradiance(w, h, probes)
    finally:
        fs.ctx.close()
        fs.scene.close()
    cli = [program, "--scene", path, "--size", str(w), str(h), "--samples", "2", "2", "--depth", "1", "--out", "cli.ppm"]
    r = subprocess.run(cli + ["--probes"] + [str(x) for x in dims] + [str(m), "--probes-visible"], input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = read_pfm(str(tmp_path / "cli.ppm.probes.pfm"))
    assert got.shape == (h, w, 3) and same(np.ascontiguousarray(got), want) and not same(want, plain)
    r = subprocess.run(cli + ["--probes-visible"], input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 2, "--probes-visible needs --probes"
