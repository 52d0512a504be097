"""rtamd::Flyscene::lightProbesBounce and indirectDiffuseBounce on a real MI355X, through the group `probes_bounce` of
tools/flyscene_check.cpp: the members return, bit for bit, what the Python mirror (Flyscene.light_probes with bounces=, and
rt_indirect_diffuse_bounce on the same object's lights) returns for the same object, and refuse what the group expects them to refuse (the
child's exit status); rt_render --probes ... --probe-bounces B writes the lookup of that volume.  tests/test_gpu_probe_bounce.py holds the
mirror against the definition."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import facade_cases as fc
import indirect_ref as ir
import switch_table
from facade_cases import H, W, same
from test_gpu_cpp_probes import read_pfm

pytestmark = pytest.mark.gpu

F = np.float32
TIMEOUT = 14
ONE = ((-1.0, 1.0, 1.0),)
# the cases of group_probes_bounce: name -> (dims, m, direct, margin, bounces, visible)
CASES = {"a": ((4, 3, 3), 3, False, 0.0, 2, True), "b": ((4, 3, 3), 3, True, 0.0, 2, False), "c": ((3, 1, 4), 2, True, 0.25, 1, True),
         "d": ((4, 3, 3), 3, True, 0.0, 0, True)}
fp = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name", ["mixed", "dodge"])
def test_probes_bounce(rt, oracle, scenes, tmp_path, name):
    paths = fc.scene_paths(scenes, tmp_path)
    osc = oracle.load_scene(paths[name])
    fs = rt.Flyscene(scene_path=paths[name])
    fs.initialize(W, H, False, True)
    try:
        _, (P, N) = fc.frame_points(oracle, osc, W, H)
        assert 0 < int(ir.ao_ref.is_point(N).sum()) < len(P), "the frame must hold hits and misses"
        arrays = {"P": P, "N": N, "one": fc.vec3(ONE)}
        try:
            status, out, err = fc.run("probes_bounce", paths[name], arrays, str(tmp_path), TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.exit(f"flyscene_check probes_bounce on {name} ran into its time limit of {TIMEOUT} s: nothing more is started on the device", 3)
        if status < 0 or status in (124, 134, 137, 139):                 # killed by a signal: a fault, an abort
            pytest.exit(f"flyscene_check probes_bounce on {name} ended with {status}: nothing more is started on the device\n{err[-3000:]}", 3)
        assert status == 0, f"flyscene_check probes_bounce on {name} ended with {status}:\n{err[-3000:]}"
        fs.lights = list(ONE)
        lib, h = fs.ctx.lib, fs.ctx.handle
        for case, (dims, m, direct, margin, bounces, visible) in CASES.items():
            pg, coeff = fs.light_probes(dims, m, direct=direct, margin=margin, bounces=bounces, visible=visible)
            assert out[f"coeff_{case}"].shape == (dims[0] * dims[1] * dims[2], 27) and same(out[f"coeff_{case}"], coeff), (name, case)
            if not direct:
                L = fs._lights()
                for v in (0, 1):
                    rgb = np.full((len(P), 3), 7, F)
                    rt.capi.check(lib, h, lib.rt_indirect_diffuse_bounce(h, C.byref(L), len(P), fp(P), fp(N), 3, 7, C.byref(pg), fp(coeff), v, fp(rgb)),
                                  "rt_indirect_diffuse_bounce")
                    assert same(out[f"rgb_{case}_{v}"], rgb), (name, case, v)
                plain = np.full((len(P), 3), 7, F)
                rt.capi.check(lib, h, lib.rt_indirect_diffuse(h, C.byref(L), len(P), fp(P), fp(N), 3, 7, fp(plain)), "rt_indirect_diffuse")
                assert not same(out[f"rgb_{case}_1"], plain), "the volume must show in the gather"
        assert not same(out["coeff_b"], out["coeff_d"]), "two bounces must show"
    finally:
        fs.ctx.close()
        fs.scene.close()
        osc.close()


def test_the_cli_writes_the_lookup_of_the_bounced_volume(rt, scenes, tmp_path):
    """rt_render --probes DX DY DZ M --probe-bounces B [--probes-visible]"""
    program = os.path.join(os.path.dirname(fc.PROGRAM), "rt_render")
    path = os.path.join(scenes, "dodgeColorTest.obj")
    w, h, dims, m = 72, 40, (4, 3, 3), 3
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(w, h, True, False)
    try:
        seen = fs.probe_irradiance(w, h, fs.light_probes(dims, m, direct=True, margin=0.0, bounces=2, visible=True), visible=True)
        plain = fs.probe_irradiance(w, h, fs.light_probes(dims, m, direct=True, margin=0.0, bounces=2, visible=False))
        parent = fs.probe_irradiance(w, h, fs.light_probes(dims, m, direct=True, margin=0.0))
    finally:
        fs.ctx.close()
        fs.scene.close()
    cli = [program, "--scene", path, "--size", str(w), str(h), "--samples", "2", "2", "--depth", "1", "--out", "cli.ppm", "--probes"] + [str(x) for x in dims] + [str(m)]
    for extra, want in ((["--probe-bounces", "2", "--probes-visible"], seen), (["--probe-bounces", "2"], plain), (["--probe-bounces", "0"], parent)):
        r = subprocess.run(cli + extra, input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=60)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        got = read_pfm(str(tmp_path / "cli.ppm.probes.pfm"))
        assert got.shape == (h, w, 3) and same(np.ascontiguousarray(got), want), extra
    assert not same(plain, parent)
    for bad in (["--probe-bounces", "-1"], ["--probe-bounces", "65"], ["--probe-bounces", "x"]):
        r = subprocess.run(cli + bad, input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=60)
        assert r.returncode == 2, bad
    r = subprocess.run(cli[:-5] + ["--probe-bounces", "2"], input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 2, "--probe-bounces needs --probes"
