"""The C++ Flyscene facade (csrc/flyscene.hpp) member by member on a real MI355X.  tools/flyscene_check.cpp runs one group of calls per child
process and writes what they returned; every array is compared on its bit patterns with the CPU checker wherever it restates the operation,
with the numpy restatements of the queries and filters, and with the Python mirror run on a context of its own -- no tolerance anywhere.
tests/test_cpp_facade_api.py holds the conditions that keep these cases from being vacuous."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

import ao_ref
import denoise_ref as dr
import facade_cases as fc
import reproject_ref as rr
import switch_table
import test_gpu_denoise as gd
import upsample_ref as ur
from facade_cases import H, H2, W, W2, same

pytestmark = pytest.mark.gpu

F = np.float32
# seconds a child may take: ten times the slowest group seen when this file first ran (traceRay on the cube, 12,672 calls: 1.36 s; every
# other group 0.2 s to 1.3 s), so that a hang ends the test and a slow shared machine does not
TIMEOUT = 14


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


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
def groups(rt, paths, tmp_path_factory):
    """group(name, scene key, arrays = its inputs, stdin, tag) -> the arrays the child wrote; one child per (group, scene, tag), started
    once, its exit status 0"""
    done = {}

    def group(name, key="cube", arrays=None, stdin="", tag=""):
        key, scene = key + tag, key
        if (name, key) not in done:
            work = str(tmp_path_factory.mktemp(f"{name}_{key}"))
            arrays = fc.inputs(name, scene, paths, rt.load_library()) if arrays is None else arrays
            t0 = time.perf_counter()
            try:
                status, out, err = fc.run(name, paths[scene], arrays, work, TIMEOUT, stdin=stdin)
            except subprocess.TimeoutExpired:
                pytest.exit(f"flyscene_check {name} on {key} ran into its time limit of {TIMEOUT} s: nothing more is started on the device", 3)
            if status < 0 or status in (124, 134, 137, 139):             # killed by a signal: a fault, an abort
                pytest.exit(f"flyscene_check {name} on {key} ended with {status}: nothing more is started on the device\n{err[-3000:]}", 3)
            assert status == 0, f"flyscene_check {name} on {key} ended with {status}:\n{err[-3000:]}"
            done[(name, key)] = (out, work, time.perf_counter() - t0)
        return done[(name, key)][0]

    group.work = lambda name, key="cube": done[(name, key)][1]
    yield group
    for (name, key), v in done.items():                                 # (shown with -s: what TIMEOUT is sized from)
        print(f"flyscene_check {name} on {key}: {v[2]:.2f} s")


class Mirror:
    """the Python Flyscene on a scene, on a context of its own"""

    def __init__(self, rt, path, w=W, h=H, area=True, point=False):
        self.rt = rt
        self.fs = rt.Flyscene(scene_path=path)
        self.fs.initialize(w, h, area, point)
        self.fs.max_depth = 3

    def mode(self, name):
        fs = self.fs
        fs.areaLight, fs.pointLight = fc.MODES[name]
        fs.sphere_offsets = self.rt.sphere_offsets(fs.sphere_seed, 1.0, 25)

    def frame(self, w=0, h=0):
        return self.fs.raytraceScene(w, h, write_ppm=False).copy()

    def close(self):
        self.fs.reset_history()
        self.fs.ctx.close()
        self.fs.scene.close()


@pytest.fixture(scope="module")
def mirrors(rt, paths):
    made = {}

    def mirror(key):
        if key not in made:
            made[key] = Mirror(rt, paths[key])
        return made[key]

    yield mirror
    for m in made.values():
        m.close()


def checker_frame(oracle, osc, w, h, yaw=0.0, mode="area", points=fc.OWN, depth=3, offsets=None):
    return osc.render(oracle.camera(w, h, yaw), fc.oracle_lights(oracle, mode, points, offsets=offsets), w, h, max_depth=depth)[0]


# ------------------------------------------------------------------------------------------ a. traceRay
@pytest.mark.parametrize("mode", ["area", "point", "sphere"])
@pytest.mark.parametrize("name", ["cube", "dodge", "mixed"])
def test_trace_ray(rt, oracle, oscenes, groups, mirrors, name, mode):
    out = groups("trace", name)
    o, d, _ = fc.rays()
    o, d = o[:fc.TRACE_RAYS], d[:fc.TRACE_RAYS]
    osc, mir = oscenes[name], mirrors(name)
    mir.mode(mode)
    mir.fs.usteps = mir.fs.vsteps = 5
    offsets = rt.sphere_offsets(65, 1.0, 25)
    by_checker = {}
    for depth in fc.TRACE_DEPTHS:
        mir.fs.max_depth = depth
        for level in fc.TRACE_LEVELS:
            budget = fc.trace_budget(depth, level)
            for which, lights in (("own", fc.OWN), ("three", fc.THREE)):
                got = out[f"trace_{mode}_{depth}_{level}_{which}"]
                if (budget, which) not in by_checker:
                    L = fc.oracle_lights(oracle, mode, lights, offsets=offsets)
                    by_checker[(budget, which)] = np.stack([osc.trace_ray(L, o[i], d[i], 0, fc.RT_MAX_DEPTH if budget < 0 else budget)
                                                            for i in range(fc.TRACE_RAYS)])
                assert same(got, by_checker[(budget, which)]), (depth, level, which)
                assert same(got, mir.fs.traceRay(o, d, level, lights)), (depth, level, which)
    mir.mode("area")
    mir.fs.max_depth = 3


# ------------------------------------------------------------------------------------------ b. lightStrikes
@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_light_strikes(oscenes, groups, name):
    out = groups("strikes", name)
    _, _, pts = fc.rays()
    for key, lights in fc.LIGHT_LISTS.items():
        want = [oscenes[name].light_strikes(p, fc.vec3(lights)) for p in pts[name]]
        vis, ret = out[f"vis_{key}"], out[f"ret_{key}"]
        assert vis.shape == (700, len(lights)) and ((vis == 0) | (vis == 1)).all()
        assert np.array_equal(vis.astype(bool), np.stack([v for _, v in want])), key
        assert np.array_equal(ret.astype(bool), np.array([a for a, _ in want])), key
        assert np.array_equal(ret.astype(bool), vis.any(axis=1))


# ------------------------------------------------------------------------------------------ c. closestHits
@pytest.mark.parametrize("name", ["cube", "dodge", "mixed"])
def test_closest_hits(oscenes, groups, name):
    out = groups("hits", name)
    o, d, _ = fc.rays()
    faces, ts = out["faces"], out["ts"]
    assert faces.shape == (1500,) and ts.shape == (1500,)
    want = [oscenes[name].closest_hit(o[i], d[i]) for i in range(1500)]
    wf = np.array([f for f, _ in want], np.int32)
    wt = np.array([t if f >= 0 else -1.0 for f, t in want], F)
    assert np.array_equal(faces, wf)
    assert same(ts, wt)
    miss = faces < 0
    assert (faces[miss] == -1).all() and (fc.bits(ts[miss]) == 0xBF800000).all()


# ------------------------------------------------------------------------------------------ d. ambientOcclusion
@pytest.fixture(scope="module")
def frame_points(oracle, oscenes):
    made = {}

    def points(name, w, h):
        if (name, w, h) not in made:
            made[(name, w, h)] = fc.frame_points(oracle, oscenes[name], w, h)
        return made[(name, w, h)]

    return points


@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_ambient_occlusion(rt, oscenes, groups, mirrors, frame_points, name):
    (_, _, f, _), (P, N) = frame_points(name, W, H)
    out = groups("ao", name, {"P": P, "N": N, "radius": np.array([fc.AO_RADIUS], F)})
    ctx = mirrors(name).fs.ctx
    n = len(P)
    bufs = [rt.hipmem.DeviceBuffer(n * 12).from_numpy(np.ascontiguousarray(a, F)) for a in (P, N)]
    try:
        for m in fc.AO_GRIDS:
            for seed in fc.AO_SEEDS:
                got = out[f"open_{m}_{seed}"]
                assert same(got, ao_ref.counts(oscenes[name], P, N, seed, m, fc.AO_RADIUS)), (m, seed)
                mine, _ = ctx.ambient_occlusion(bufs[0], bufs[1], m, fc.AO_RADIUS, seed=seed, n=n, want_ao=False)
                ctx.synchronize()
                assert same(got, mine.to_numpy(np.uint16, (n,))), (m, seed)
                mine.free()
                assert (got[f < 0] == m * m).all() and (name == "cube" or (got[f >= 0] < m * m).any())        # (the cube is convex: all open)
    finally:
        for b in bufs:
            b.free()


# ------------------------------------------------------------------------------------------ e. softShadows
SHADOW_MODES = {"a55": ("area", 5, 5), "a37": ("area", 3, 7), "point": ("point", 5, 5)}


@pytest.mark.parametrize("mode", list(SHADOW_MODES))
@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_soft_shadows(rt, oracle, oscenes, groups, mirrors, frame_points, name, mode):
    out = groups("shadow", name)
    lib = rt.load_library()
    fu, fv = C.c_float(), C.c_float()
    assert lib.rt_light_jitter_offsets(5, C.byref(fu), C.byref(fv)) == 0
    kind, u, v = SHADOW_MODES[mode]
    mir = mirrors(name)
    mir.mode(kind)
    mir.fs.usteps, mir.fs.vsteps = u, v
    osc = oscenes[name]
    params = {"null": (None, dict()), "pass5": (rt.shadow_params(fu=fu.value, fv=fv.value), dict(fo=(F(fu.value), F(fv.value)))),
              "seed7": (rt.shadow_params(per_point=True, seed=7), dict(per_point=True, seed=7))}
    for count, lights in (("1", fc.THREE[:1]), ("3", fc.THREE)):
        mir.fs.lights = list(lights)
        for w, h in ((W, H), (W2, H2)):
            (_, _, f, _), (P, _) = frame_points(name, w, h)
            hit = f >= 0
            for pname, (sp, ref_kw) in params.items():
                got = out[f"shadow_{mode}_{count}_{w}_{pname}"]
                assert got.shape == (h, w)
                assert same(got, mir.fs.soft_shadows(w, h, sp)), (count, w, pname)
                L = fc.oracle_lights(oracle, kind, lights, u, v)
                assert same(got, fc.shadow_image(osc, L, P, hit, w, h, **ref_kw)), (count, w, pname)
                assert (fc.bits(got.reshape(-1)[~hit]) == 0x3F800000).all()
    assert same(out["before"], out["after"]), "a frame rendered after the calls equals the one before them"
    assert same(out["before"], checker_frame(oracle, osc, W, H, points=fc.THREE[:1]))
    mir.mode("area")
    mir.fs.usteps = mir.fs.vsteps = 5
    mir.fs.lights = list(fc.OWN)


# ------------------------------------------------------------------------------------------ f. createSpherePoint, g. addLight
@pytest.mark.parametrize("mode", ["area", "point", "sphere"])
def test_create_sphere_point(rt, oracle, groups, mirrors, mode):
    out = groups("lights")
    mir = mirrors("cube")
    mir.mode(mode)
    offsets = rt.sphere_offsets(65, 1.0, 25)
    for u, v in fc.GRIDS:
        got = out[f"csp_{mode}_{u}x{v}"]
        assert got.shape == ({"area": u * v, "point": 1, "sphere": 25}[mode], 3)
        want = oracle.light_samples(fc.oracle_lights(oracle, mode, [fc.LIGHT_POINT], u, v, offsets=offsets), fc.LIGHT_POINT)
        assert same(got, want), (u, v)
        mir.fs.usteps, mir.fs.vsteps = u, v
        assert same(got, mir.fs.createSpherePoint(fc.LIGHT_POINT)), (u, v)
        if mode != "sphere":
            L = rt.make_lights(points=[fc.LIGHT_POINT], area=(mode == "area"), usteps=u, vsteps=v)
            assert same(got, rt.light_samples(L, 0, 0.5, 0.5)), (u, v)
    mir.mode("area")
    mir.fs.usteps = mir.fs.vsteps = 5


def test_add_light_stops_at_25(rt, oracle, oscenes, groups):
    out = groups("lights")
    lights = out["lights"]
    centre = np.array(list(rt.default_camera(16, 12).center), F)
    assert lights.shape == (25, 3) and same(lights[0], fc.vec3(fc.OWN)[0]) and all(same(p, centre) for p in lights[1:])
    want = checker_frame(oracle, oscenes["cube"], 16, 12, points=[tuple(float(x) for x in p) for p in lights])
    assert same(out["frame"], want)
    assert not same(want, checker_frame(oracle, oscenes["cube"], 16, 12)), "the added lights change the frame"


# ------------------------------------------------------------------------------------------ h. sizes and state
def counters(stats):
    return np.array([getattr(stats, k) for k in fc.COUNTERS], np.uint64)


@pytest.mark.parametrize("variant", ["plain", "shutter"])
def test_sizes_and_state(rt, oracle, oscenes, groups, paths, variant):
    """raytraceScene(), raytraceScene(40, 24), raytraceScene(), gbuffer(40, 24), gbuffer(), raytraceScene() on a 48 x 32 object: an explicit
    size is for that call alone, for the camera and for the shutter's close camera"""
    out = groups("state", "cube", {"shutter": np.array([variant == "shutter"], F)}, tag=variant)
    mir = Mirror(rt, paths["cube"])
    try:
        fs = mir.fs
        if variant == "shutter":
            fs.shutter_close = rt.default_camera(W, H, 0.05)
            fs.supersample = 2
        want = {0: mir.frame()}
        stats0 = counters(fs.stats)
        want[1] = mir.frame(W2, H2)
        want[2] = mir.frame()
        want[3] = fs.gbuffer(W2, H2)
        want[4] = fs.gbuffer()
        want[5] = mir.frame()
    finally:
        mir.close()
    for k in range(6):
        assert same(out[f"{variant}_{k}"], want[k]), f"call {k} of the sequence differs from the Python mirror"
    assert same(out[f"{variant}_0"], out[f"{variant}_5"]) and same(out[f"{variant}_0"], out[f"{variant}_2"])
    assert np.array_equal(out[f"{variant}_stats0"], stats0), dict(zip(fc.COUNTERS, zip(out[f"{variant}_stats0"].tolist(), stats0.tolist())))
    assert stats0[0] > 0
    if variant == "plain":
        osc = oscenes["cube"]
        for k, (w, h) in ((0, (W, H)), (1, (W2, H2)), (2, (W, H)), (5, (W, H))):
            assert same(out[f"plain_{k}"], checker_frame(oracle, osc, w, h)), k
    else:
        plain = groups("state", "cube", {"shutter": np.zeros(1, F)}, tag="plain")
        assert not same(out["shutter_0"], plain["plain_0"]) and not same(out["shutter_4"], plain["plain_4"]), "the shutter blurs the frame"


# ------------------------------------------------------------------------------------------ i. the stand-alone filters
@pytest.mark.parametrize("ch", [1, 3])
def test_standalone_denoise_upsample_reproject(rt, groups, ch):
    dp, up, rp = rt.denoise_params(), rt.upsample_params(), rt.reproject_params()
    arrays = fc.post_inputs(up.factor)
    m = rt.reproject_map(rt.default_camera(fc.POST_W, fc.POST_H, 0.42), rt.default_camera(fc.POST_W, fc.POST_H, 0.40))
    arrays["rp_m"] = np.ascontiguousarray(m, F).reshape(12)
    out = groups("post", "cube", arrays)
    sn, sz, sa = (float(x) for x in arrays["tight"])
    # denoise
    img, g = arrays[f"dn_img{ch}"], arrays["dn_g"]
    want = dr.denoise(img, g, gd.ref_params(dp))
    assert same(out[f"dn_{ch}_null"], want) and same(out[f"dn_{ch}_def"], want)
    tight = dr.denoise(img, g, dr.Params(2, dp.sigma_color, sn, sz, sa))
    assert same(out[f"dn_{ch}_tight"], tight) and not same(tight, want)
    # upsample: null = the default factor; 3 does not divide 67 x 21
    for name, s, p in (("null", up.factor, ur.Params(up.factor, up.sigma_normal, up.sigma_depth, up.sigma_albedo)),
                       ("def", up.factor, ur.Params(up.factor, up.sigma_normal, up.sigma_depth, up.sigma_albedo)),
                       ("three", 3, ur.Params(3, up.sigma_normal, up.sigma_depth, up.sigma_albedo)), ("tight", 3, ur.Params(3, sn, sz, sa))):
        want, miss = ur.upsample(arrays[f"up{s}_low{ch}"], arrays[f"up{s}_gl"], arrays[f"up{s}_gh"], p, want_miss=True)
        assert same(out[f"up_{ch}_{name}"], want) and same(out[f"upm_{ch}_{name}"], want), name
        assert same(out[f"miss_{ch}_{name}"], miss), name
    assert fc.POST_W % 3 and out[f"miss_{ch}_tight"].any() and not out[f"miss_{ch}_tight"].all()
    # reproject through a yaw map
    args = (arrays[f"rp_cur{ch}"], arrays["rp_gc"], arrays[f"rp_hist{ch}"], arrays["rp_gh"], arrays["rp_len"], m)
    want, ln = rr.reproject(*args, rr.Params(rp.max_history, rp.sigma_normal, rp.sigma_depth, rp.sigma_albedo))
    for name in ("null", "def"):
        assert same(out[f"rp_{ch}_{name}"], want) and same(out[f"rplen_{ch}_{name}"], ln), name
    tight, tln = rr.reproject(*args, rr.Params(4, sn, sz, sa))
    assert same(out[f"rp_{ch}_tight"], tight) and same(out[f"rplen_{ch}_tight"], tln) and not same(tln, ln)


# ------------------------------------------------------------------------------------------ j. the temporal lifecycle
def temporal_mirror(rt, path):
    mir = Mirror(rt, path)
    fs = mir.fs
    fs.usteps = fs.vsteps = 2
    fs.max_depth, fs.passes = 1, 2
    fs.temporal = rt.reproject_params(sigma_depth=fc.TEMPORAL_SIGMA_DEPTH)
    return mir


def test_temporal_lifecycle(rt, groups, paths):
    out = groups("temporal")
    mir = temporal_mirror(rt, paths["cube"])
    try:
        fs = mir.fs
        for k, yaw in enumerate(fc.YAWS):
            fs.camera = rt.default_camera(W, H, yaw)
            assert same(out[f"path{k}"], mir.frame()), k
            assert same(out[f"pathlen{k}"].reshape(H, W), fs.history_lengths()), k
        fs.temporal = None
        plain = mir.frame()                                    # the plain frame with passes (0, 2), at the last camera of the path
    finally:
        mir.close()
    assert (out["pathlen0"] == 1).all() and set(np.unique(out["pathlen1"])) == {1, 2} and (out["pathlen2"] == 3).any()
    # resetHistory: the next frame is itself
    assert (out["resetlen"] == 1).all() and same(out["reset"], plain) and same(out["reset_plain"], plain)
    assert (out["secondlen"] == 2).any()
    # another size drops the history, and so does the way back
    assert out["smalllen"].shape == (W2 * H2,) and (out["smalllen"] == 1).all()
    assert (out["again0len"] == 1).all() and (out["again1len"] == 2).any()
    # a scene change: the first frame after initialize is the first frame of a fresh object
    assert (out["freshlen"] == 1).all()
    assert (out["changedlen"] == 1).all(), "the first frame after initialize was reprojected against the previous scene's history"
    assert same(out["changed"], out["fresh"])
    fresh = temporal_mirror(rt, paths["dodge"])
    try:
        assert same(out["fresh"], fresh.frame())
    finally:
        fresh.close()
    # temporal reuse together with upsampling
    assert int(out["refused_status"][0]) == rt.capi.RT_ERR_INVALID and int(out["refused_written"][0]) == 0
    assert not os.path.exists(os.path.join(groups.work("temporal"), "temporal.out.ppm.refused"))


def test_temporal_lifecycle_of_the_python_mirror(rt, paths):
    mir = temporal_mirror(rt, paths["cube"])
    fresh = None
    try:
        fs = mir.fs
        for yaw in fc.YAWS:
            fs.camera = rt.default_camera(W, H, yaw)
            mir.frame()
        assert (fs.history_lengths() == 3).any()
        fs.reset_history()
        first = mir.frame()
        assert (fs.history_lengths() == 1).all()
        params, fs.temporal = fs.temporal, None
        assert same(first, mir.frame()), "after a reset the frame is the plain frame with passes (0, 2)"
        fs.temporal = params
        mir.frame()
        assert (fs.history_lengths() == 2).any()
        mir.frame(W2, H2)
        assert fs.history_lengths().shape == (H2, W2) and (fs.history_lengths() == 1).all(), "another size drops the history"
        mir.frame()
        mir.frame()
        assert (fs.history_lengths() == 2).any()
        old_ctx, old_scene = fs.ctx, fs.scene
        fs.scene_path = paths["dodge"]
        fs.initialize(W, H, True, False)
        old_ctx.close()
        old_scene.close()
        changed = mir.frame()
        assert (fs.history_lengths() == 1).all(), "the first frame after initialize was reprojected against the previous scene's history"
        fresh = temporal_mirror(rt, paths["dodge"])
        assert same(changed, fresh.frame())
    finally:
        mir.close()
        if fresh is not None:
            fresh.close()


# ------------------------------------------------------------------------------------------ k. objects
def test_two_objects_and_a_second_initialize(rt, oracle, oscenes, groups):
    out = groups("objects", stdin="1 0\n0 1\n0 0\n")
    for a in ("a", "b"):
        for k in (0, 1):
            assert same(out[f"both_{a}{k}"], out[f"alone_{a}{k}"]), (a, k)
    assert same(out["after_b0"], out["alone_b0"]), "the second object renders after the first is destroyed"
    for a, name in (("a", "cube"), ("b", "dodge")):
        for k, yaw in ((0, 0.0), (1, fc.OBJECT_YAW)):
            assert same(out[f"alone_{a}{k}"], checker_frame(oracle, oscenes[name], W, H, yaw)), (a, k)
    assert same(out["twice_cube"], out["alone_a0"])
    assert same(out["twice_mixed"], out["fresh_mixed"]) and same(out["fresh_mixed"], checker_frame(oracle, oscenes["mixed"], W, H))
    assert not same(out["twice_mixed"], out["twice_cube"])


@pytest.mark.parametrize("mode", ["area", "point", "sphere"])
def test_the_prompts_of_initialize_select_the_mode(rt, oracle, oscenes, groups, mode):
    out = groups("objects", stdin="1 0\n0 1\n0 0\n")
    offsets = rt.sphere_offsets(65, 1.0, 25)
    want = oracle.light_samples(fc.oracle_lights(oracle, mode, [fc.LIGHT_POINT], offsets=offsets), fc.LIGHT_POINT)
    assert same(out[f"stdin_csp_{mode}"], want)
    assert same(out[f"stdin_frame_{mode}"], checker_frame(oracle, oscenes["cube"], 16, 12, mode=mode, offsets=offsets))
