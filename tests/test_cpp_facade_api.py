"""The C++ Flyscene facade without a device: the driver tools/flyscene_check.cpp is built with the rest, an object that was never initialised
fails every member cleanly, the sample grids equal the CPU checker's -- and the conditions tests/test_gpu_cpp_facade.py relies on hold on the
checker alone, so that none of its cases is vacuous."""
import os
import re
import subprocess

import numpy as np
import pytest

import facade_cases as fc
import reproject_ref as rr

F = np.float32
MAKEFILE = os.path.join(fc.ROOT, "raytracer-in-cpp_amd", "csrc", "Makefile")


@pytest.fixture(scope="module")
def paths(scenes, tmp_path_factory):
    return fc.scene_paths(scenes, tmp_path_factory.mktemp("mixed"))


@pytest.fixture(scope="module")
def oscenes(oracle, paths):
    out = {k: oracle.load_scene(p) for k, p in paths.items()}
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(scope="module")
def host(rt, paths, tmp_path_factory):
    """flyscene_check --host, once: (exit status, arrays, stderr)"""
    rt.load_library()                                  # (the package builds nothing on import; the library must exist beside the driver)
    assert os.path.exists(fc.PROGRAM), "make builds raytracer-in-cpp_amd/lib/flyscene_check"
    return fc.run("host", paths["cube"], fc.inputs("host"), str(tmp_path_factory.mktemp("host")), timeout=60, host=True)


def test_the_makefile_builds_the_driver_in_all():
    text = open(MAKEFILE).read()
    all_rule = re.search(r"^all:(.*)$", text, re.M).group(1)
    assert "$(OUT)/flyscene_check" in all_rule
    rule = re.search(r"^\$\(OUT\)/flyscene_check:.*\n\t(.*)$", text, re.M).group(1)
    assert rule.startswith("g++ ") and "-lrt_mi355x" in rule and "sanitize" not in rule
    src = open(os.path.join(fc.ROOT, "tools", "flyscene_check.cpp")).read()
    assert set(re.findall(r'#include "([^"]+)"', src)) == {"flyscene.hpp"}, "the driver is a user of the facade: no internal header"


def test_an_object_without_a_scene_fails_every_member_cleanly(host):
    status, arrays, err = host
    assert status == 0, err
    assert "expected" not in err


def test_a_group_that_needs_a_device_is_refused_in_host_mode(paths, tmp_path):
    fc.write_arrays(str(tmp_path / "in"), fc.inputs("hits"))
    r = subprocess.run([fc.PROGRAM, "--host", "hits", paths["cube"], str(tmp_path / "in"), str(tmp_path / "out")], capture_output=True, timeout=60)
    assert r.returncode == 2


@pytest.mark.parametrize("mode", ["area", "point"])
def test_sample_grids_equal_the_checker(rt, oracle, host, mode):
    _, arrays, err = host
    for u, v in fc.GRIDS:
        got = arrays[f"csp_{mode}_{u}x{v}"]
        want = oracle.light_samples(fc.oracle_lights(oracle, mode, [fc.LIGHT_POINT], u, v), fc.LIGHT_POINT)
        assert got.shape == ((u * v if mode == "area" else 1), 3)
        assert fc.same(got, want), (mode, u, v)
        L = rt.make_lights(points=[fc.LIGHT_POINT], area=(mode == "area"), usteps=u, vsteps=v)
        assert fc.same(got, rt.light_samples(L, 0, 0.5, 0.5)), (mode, u, v)


def test_the_array_files_round_trip(tmp_path):
    arrays = {"a": np.arange(6, dtype=F).reshape(2, 3), "b": np.zeros((0, 3), F), "c": np.array([1, 2, 3], np.uint16), "s": "x/y.obj",
              "n": np.array([10, 13, 10], np.uint8), "k": np.array([2 ** 40], np.uint64), "i": np.array([-1], np.int32)}
    fc.write_arrays(str(tmp_path / "f"), arrays)
    back = fc.read_arrays(str(tmp_path / "f"))
    assert list(back) == list(arrays) and bytes(back["s"]) == b"x/y.obj"
    for k in "abcnki":
        assert fc.same(back[k], arrays[k]), k


# ------------------------------------------------------------------------------------------ the conditions of the GPU file, on the checker alone
def test_the_rays_hold_hits_and_misses_on_every_scene(oscenes):
    o, d, _ = fc.rays()
    for name, osc in oscenes.items():
        hits = sum(osc.closest_hit(o[i], d[i])[0] >= 0 for i in range(len(o)))
        assert 0 < hits < len(o), name
        first = sum(osc.closest_hit(o[i], d[i])[0] >= 0 for i in range(fc.TRACE_RAYS))
        assert 0 < first < fc.TRACE_RAYS, name


def test_the_trace_budgets():
    assert [fc.trace_budget(3, l) for l in fc.TRACE_LEVELS] == [3, 2, 0, 0]
    assert [fc.trace_budget(-1, l) for l in fc.TRACE_LEVELS] == [-1] * 4


def test_depth_and_lights_change_the_traced_colours(rt, oracle, oscenes):
    """the budget, the light list and the mode each change some colour of the 264 rays: a facade that dropped one of them would show.  Every
    budget of the case (3, 2, 0, unlimited) gives colours of its own on the cube; on the mixed scene a budget of 0 does"""
    o, d, _ = fc.rays()
    off = rt.sphere_offsets(65, 1.0, 25)

    def colours(name, mode, points, depth):
        L = fc.oracle_lights(oracle, mode, points, offsets=off)
        return np.stack([oscenes[name].trace_ray(L, o[i], d[i], 0, depth) for i in range(fc.TRACE_RAYS)])

    by_depth = [colours("cube", "area", fc.OWN, k) for k in (3, 2, 0, fc.RT_MAX_DEPTH)]
    assert all(not fc.same(by_depth[i], by_depth[j]) for i in range(4) for j in range(i))
    assert not fc.same(colours("mixed", "area", fc.OWN, 3), colours("mixed", "area", fc.OWN, 0))
    for name in oscenes:
        base = colours(name, "area", fc.THREE, 3)
        assert not fc.same(base, colours(name, "area", fc.OWN, 3)), name
        point, sphere = colours(name, "point", fc.THREE, 3), colours(name, "sphere", fc.THREE, 3)
        assert not fc.same(base, point) and not fc.same(base, sphere) and not fc.same(point, sphere), name


@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_the_points_give_visible_and_blocked_segments(oscenes, name):
    _, _, pts = fc.rays()
    for key, lights in fc.LIGHT_LISTS.items():
        vis = np.stack([oscenes[name].light_strikes(p, fc.vec3(lights))[1] for p in pts[name]])
        assert vis.any() and not vis.all(), (name, key)
        assert vis.shape == (700, len(lights))


@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_the_shadow_images_have_penumbrae(oracle, oscenes, name):
    osc = oscenes[name]
    (o, d, f, t), (P, _) = fc.frame_points(oracle, osc, fc.W, fc.H)
    assert 0 < int((f >= 0).sum()) < len(f), "the frame holds hits and misses"
    for lights in (fc.THREE[:1], fc.THREE):
        img = fc.shadow_image(osc, fc.oracle_lights(oracle, "area", lights), P, f >= 0, fc.W, fc.H)
        assert ((img > 0) & (img < 1)).any(), (name, len(lights))
        assert (img[(f < 0).reshape(fc.H, fc.W)] == 1.0).all()


def test_the_three_frames_of_the_size_sequence_differ(oracle, oscenes):
    osc = oscenes["cube"]
    L = oracle.lights(area=True)
    a = osc.render(oracle.camera(fc.W, fc.H), L, fc.W, fc.H, max_depth=3)[0]
    b = osc.render(oracle.camera(fc.W2, fc.H2), L, fc.W2, fc.H2, max_depth=3)[0]
    # the frame a camera left at 40 x 24 would give at 48 x 32: the viewport and aspect of the small size
    stale = oracle.camera(fc.W2, fc.H2)
    c = osc.render(stale, L, fc.W, fc.H, max_depth=3)[0]
    assert a.shape != b.shape and not fc.same(a, c)
    assert not fc.same(a[:fc.H2, :fc.W2], b)


def test_the_yaw_path_leaves_rejected_and_accepted_pixels(rt, oracle, oscenes):
    """frame 2 of the path against frame 1, by the restatement on the checker's buffers: some pixels take history, some covered ones do not"""
    import gbuffer_ref
    osc = oscenes["cube"]
    gs = [gbuffer_ref.cpu_frame(oracle, osc, oracle.camera(fc.W, fc.H, yaw), fc.W, fc.H) for yaw in fc.YAWS[:2]]
    m = rt.reproject_map(rt.default_camera(fc.W, fc.H, fc.YAWS[1]), rt.default_camera(fc.W, fc.H, fc.YAWS[0]))
    p = rt.reproject_params(sigma_depth=fc.TEMPORAL_SIGMA_DEPTH)
    img = np.zeros((fc.H, fc.W, 3), F)
    _, ln = rr.reproject(img, gs[1], img, gs[0], np.ones((fc.H, fc.W), np.uint8), m, rr.Params(p.max_history, p.sigma_normal, p.sigma_depth, p.sigma_albedo))
    covered = gs[1][..., 0] > 0
    assert (ln[covered] == 2).any() and (ln[covered] == 1).any()
    everything = rt.reproject_params()
    _, ln = rr.reproject(img, gs[1], img, gs[0], np.ones((fc.H, fc.W), np.uint8), m,
                         rr.Params(everything.max_history, everything.sigma_normal, everything.sigma_depth, everything.sigma_albedo))
    assert (ln[covered] == 2).all(), "(the default depth scale accepts every pixel of this path: the case sets a tighter one)"
