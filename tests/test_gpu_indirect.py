"""The one-bounce diffuse gather on a real MI355X: rt_indirect_diffuse_device returns, per point, bit for bit what tests/indirect_ref.py gets
from the definition -- over the CPU checker's closest hit and lightStrikes, and over rt_closest_hits / rt_light_strikes where the checker
takes too long -- in every wave layout, for every batch length around the layout boundaries, with one light and with many, in the order of
the definition's sum; it writes nothing behind element n * 3, refuses what the header says it refuses and leaves the context as it was."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ao_ref
import denoise_ref
import grid_caps as gc
import indirect_ref as ir
import scenes_gen
import switch_table
from test_gpu_ao import GUARD, In, Out, same  # noqa: F401 -- the guarded device arrays of the occlusion tests

pytestmark = pytest.mark.gpu

F = np.float32
GRIDS = (1, 2, 3, 5, 6, 8, 10, 16)
SEED = 7
W, H = 48, 32
FILES = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj", "toy": "toy.obj"}
ONE = ((-1.0, 1.0, 1.0),)
TWO = ((-1.0, 1.0, 1.0), (1.5, 0.5, -1.0))
YELLOW, WHITE = (1.0, 1.0, 0.0), (1.0, 1.0, 1.0)
# rays above which the CPU checker (one ctypes call per ray) takes more than a few seconds: the library's own closest hits and strikes stand in
ORACLE_RAYS = 12000


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def group(m):
    return 64 // math.gcd(m * m, 64)


def lights_of(rt, pos, color):
    L = rt.make_lights(pos, area=False)
    for k in range(3):
        L.color[k] = float(color[k])
    return L


def zero_bits(a):
    return not np.ascontiguousarray(a, F).reshape(-1).view(np.uint32).any()


class Scene:
    """a scene on the GPU and in the CPU checker, its fixed point set (ao_ref.camera_points at 48 x 32, yaw 0.4) and the colour-free part of
    the reference (indirect_ref.Traced) of that set, computed once per (m, lights, tracer)"""

    def __init__(self, rt, oracle, path, points=True):
        self.rt, self.orc = rt, oracle
        self.fs = rt.Flyscene(scene_path=path)
        self.fs.initialize(64, 40, True, False)
        self.ctx, self.lib = self.fs.ctx, self.fs.ctx.lib
        self.osc = oracle.load_scene(path)
        self.data = ir.SceneData(self.osc)
        self.tracers = {"oracle": ir.OracleTracer(self.osc), "library": ir.LibraryTracer(rt, self.ctx)}
        if points:
            self.rays, (self.P, self.N) = ao_ref.camera_points(oracle, self.osc, W, H, 0.4)
            self.n = len(self.P)
        self.ref = {}

    def traced(self, m, pos=ONE, by=None, seed=SEED):
        by = by or ("oracle" if self.n * m * m <= ORACLE_RAYS else "library")
        key = (m, pos, by, seed)
        if key not in self.ref:
            self.ref[key] = ir.trace(self.tracers[by], self.data, self.P, self.N, m, seed, pos)
        return self.ref[key]

    def want(self, m, pos=ONE, color=WHITE, by=None):
        return ir.shade(self.traced(m, pos, by), color)

    def close(self):
        self.ctx.close()
        self.fs.scene.close()
        self.osc.close()


@pytest.fixture(scope="module")
def world(rt, oracle, scenes, tmp_path_factory):
    paths = {k: os.path.join(scenes, v) for k, v in FILES.items()}
    paths["mixed"] = scenes_gen.mixed_materials(str(tmp_path_factory.mktemp("mixed")))
    w = {k: Scene(rt, oracle, p) for k, p in paths.items()}
    w["binades"] = Scene(rt, oracle, ir.binade_ceiling(str(tmp_path_factory.mktemp("binades"))), points=False)
    yield w
    for s in w.values():
        s.close()


def run(sc, P, N, m, pos=ONE, color=WHITE, seed=SEED, stream=None, sync=True):
    """rt_indirect_diffuse_device on DeviceBuffers with guards -> out (n, 3) as read back"""
    n = len(P)
    p, nr = In(sc.rt, P.reshape(-1, 3) if n else np.zeros((1, 3), F)), In(sc.rt, N.reshape(-1, 3) if n else np.zeros((1, 3), F))
    o = Out(sc.rt, n, 3, np.float32)
    got = sc.ctx.indirect_diffuse(p.buf, nr.buf, lights_of(sc.rt, pos, color), m, seed=seed, n=n, out=o.buf, stream=stream)
    assert got is o.buf
    if not sync:
        return o, (p, nr)
    sc.ctx.synchronize()
    p.check(); nr.check()
    return o.read().reshape(n, 3)


def differing(got, want):
    return np.flatnonzero((np.ascontiguousarray(got, F).view(np.uint32) != np.ascontiguousarray(want, F).view(np.uint32)).any(axis=1))[:8]


# ------------------------------------------------------------------------------------------ 1. every layout on every scene
@pytest.mark.parametrize("name", ["mixed", "toy", "dodge", "cube"])
def test_gather_equals_the_reference_in_every_layout(world, name):
    sc = world[name]
    assert sc.n == {"mixed": 93, "toy": 360, "dodge": 242, "cube": 561}[name]
    for m in GRIDS:
        for color in (YELLOW, WHITE):
            want = sc.want(m, color=color)
            got = run(sc, sc.P, sc.N, m, color=color)
            assert got.dtype == np.float32 and same(got, want), (name, m, color, differing(got, want))
            if color == YELLOW:
                assert zero_bits(got[:, 2]), "no blue light: the blue channel is +0.0f"
            if name == "cube":
                assert zero_bits(got), "a convex scene returns nothing"
    nonzero = int((sc.want(3) != 0).any(axis=1).sum())
    print(name, "points with a non-zero gather at m = 3:", nonzero, "of", sc.n)
    if name != "cube":
        assert nonzero >= {"mixed": 80, "toy": 50, "dodge": 5}[name], "the fixture must hold points that receive indirect light"


def test_library_reference_equals_the_oracle_reference(world):
    """the two references of this file agree where both are affordable (so either may stand for the definition)"""
    for name, m, pos in (("mixed", 3, ONE), ("mixed", 5, TWO), ("dodge", 3, ONE), ("toy", 2, TWO)):
        sc = world[name]
        a, b = sc.traced(m, pos, "oracle"), sc.traced(m, pos, "library")
        assert np.array_equal(a.hit, b.hit) and np.array_equal(a.vis, b.vis) and same(a.ct, b.ct) and same(a.kd, b.kd), (name, m)
        assert same(ir.shade(a, WHITE), ir.shade(b, WHITE))


# ------------------------------------------------------------------------------------------ 2. two lights, partly hidden; 25 lights
def test_two_lights_partly_hidden_and_the_loop_bound(world):
    sc = world["mixed"]
    tr = sc.traced(3, TWO, "oracle")
    seen = tr.vis.sum(axis=1)
    one, both, none = int((seen == 1).sum()), int((seen == 2).sum()), int((seen == 0).sum())
    print("gather hits that see one / both / none of the two lights:", one, both, none)
    assert one >= 100 and both >= 80 and none >= 5
    want = ir.shade(tr, WHITE)
    got = run(sc, sc.P, sc.N, 3, pos=TWO)
    assert same(got, want), differing(got, want)
    assert not same(got, sc.want(3)), "the second light shows"
    many = (TWO * 13)[:25]
    want = sc.want(3, many, by="library")
    got = run(sc, sc.P, sc.N, 3, pos=many)
    assert same(got, want), differing(got, want)
    assert np.isfinite(want).all() and (want.max(axis=1) > sc.want(3, TWO).max(axis=1)).any()


# ------------------------------------------------------------------------------------------ 3. batch lengths around the layout boundaries
@pytest.mark.parametrize("m", GRIDS)
def test_batch_lengths_and_guards(world, m):
    sc = world["mixed"]
    g = group(m)
    want = sc.want(m)
    for n in sorted({0, 1, max(g - 1, 0), g, g + 1, 63, 64, 65}):
        # (point i of a call is rotated by its index i: a prefix of the batch is the batch of the prefix)
        got = run(sc, sc.P[:n], sc.N[:n], m)
        assert got.shape == (n, 3) and same(got, want[:n]), (m, n, differing(got, want[:n]))


# ------------------------------------------------------------------------------------------ 4. "no point" inputs
def at_unit_edges(n, m):
    """the first, the last and an interior point of every wave unit"""
    g = group(m)
    idx = set()
    for u0 in range(0, n, g):
        idx |= {u0, min(u0 + g - 1, n - 1), min(u0 + g // 2, n - 1)}
    return np.array(sorted(idx))


@pytest.mark.parametrize("m", [3, 8, 10])
def test_zero_normals_give_zeros_and_leave_the_others_alone(world, m):
    sc = world["mixed"]
    idx = at_unit_edges(sc.n, m) if group(m) > 2 else np.arange(0, sc.n, 3)       # (m = 8: a unit is one point)
    N = sc.N.copy()
    N[idx] = 0.0
    N[idx[::2], 1] = -0.0                                      # (either sign of zero)
    want = sc.want(m).copy()
    assert (want[idx] != 0).any() and len(idx) < sc.n
    want[idx] = 0.0
    got = run(sc, sc.P, N, m)
    assert same(got, want), differing(got, want)
    assert zero_bits(got[idx])
    # all of them: no wave has an active lane
    assert zero_bits(run(sc, sc.P, np.zeros_like(sc.N), m))


# ------------------------------------------------------------------------------------------ 5. more units than the grid holds
def stride_shape(sc, m):
    """about 1.25 caps of wave units, three points more than whole units -> n, asserted to stride as test_gpu_ao.py::test_grid_stride does"""
    K = m * m
    rounds = K // math.gcd(K, 64)
    cus = gc.cu_count(sc.ctx.device)
    units = gc.round_two(gc.ao_cap(cus, rounds)) + 5
    n = (units - 1) * group(m) + 3
    assert -(-n // group(m)) == units
    assert units > gc.ao_cap(cus, rounds) and gc.ao_grid(units, cus, rounds) * gc.WAVES < units, (cus, units, "the batch does not reach the grid of this device")
    assert gc.strides(units, gc.ao_cap(cus, rounds))
    return n


def test_grid_stride_one_round(world):
    """m = 1: the direction is N itself whatever the point's index, so a tiled point set has a tiled answer"""
    sc = world["toy"]
    n = stride_shape(sc, 1)
    base = sc.want(1)
    assert int((base != 0).any(axis=1).sum()) >= 5
    reps = -(-n // sc.n)
    P, N = np.tile(sc.P, (reps, 1))[:n], np.tile(sc.N, (reps, 1))[:n]
    want = np.tile(base, (reps, 1))[:n]
    got = run(sc, P, N, 1)
    assert same(got, want), differing(got, want)


def test_grid_stride_several_rounds(world):
    """m = 3 on a tiled point set: point j of the batch is point j % n0 of the set under the rotation of index j, and there are 64 rotations,
    so the reference is a table of 64 x n0 gathers (each from the definition, with an index that has that rotation) looked up per point"""
    sc = world["mixed"]
    m = 3
    n = stride_shape(sc, m)
    steps = ao_ref.rotation_steps(SEED, np.arange(4096))
    index_of = [int(np.flatnonzero(steps == r)[0]) for r in range(ao_ref.ROTATIONS)]
    P0, N0 = np.tile(sc.P, (ao_ref.ROTATIONS, 1)), np.tile(sc.N, (ao_ref.ROTATIONS, 1))
    i0 = np.repeat(np.array(index_of), sc.n)
    table = ir.gather(sc.tracers["library"], sc.data, P0, N0, m, SEED, ONE, WHITE, i=i0).reshape(ao_ref.ROTATIONS, sc.n, 3)
    assert same(table[ao_ref.rotation_steps(SEED, np.arange(sc.n)), np.arange(sc.n)], sc.want(m)), "the table holds the plain batch"
    reps = -(-n // sc.n)
    P, N = np.tile(sc.P, (reps, 1))[:n], np.tile(sc.N, (reps, 1))[:n]
    j = np.arange(n)
    want = table[ao_ref.rotation_steps(SEED, j), j % sc.n]
    got = run(sc, P, N, m)
    assert same(got, want), differing(got, want)
    assert 0 < int((want != 0).any(axis=1).sum())


# ------------------------------------------------------------------------------------------ 6. the order of the sum
@pytest.mark.parametrize("m", [8, 10, 16])
def test_the_sum_runs_in_the_order_of_the_definition(world, m):
    """the ceiling of strips whose kd differ by 6 binades each: the radiances of a point's rays differ by up to 42 binades, the sum from
    K - 1 down to 0 differs from the definition's in bits, and the device gives the definition's.  m = 8: a unit is one point in one round;
    m = 10: 16 points in 25 rounds, straddling them; m = 16: one point in four rounds."""
    sc = world["binades"]
    Wm = ir.to_world(sc.osc, ir.BINADE_VERTS)
    P, N = ir.binade_points(Wm)
    pos = (tuple(float(x) for x in Wm([0.0, 0.2, 0.0])),)
    tr = ir.trace(sc.tracers["oracle"], sc.data, P, N, m, SEED, pos)
    assert tr.hit.all() and len(set(tr.kd[:, 0].tolist())) >= 6
    fwd, rev = ir.shade(tr, WHITE), ir.shade(tr, WHITE, reverse=True)
    assert len(differing(fwd, rev)) >= 3, "the order must show in this fixture"
    got = run(sc, P, N, m, pos=pos)
    assert same(got, fwd), differing(got, fwd)


# ------------------------------------------------------------------------------------------ 7. refusals
def test_no_scene_and_bad_arguments(rt, world):
    sc = world["mixed"]
    lib, inv, uns = sc.lib, rt.capi.RT_ERR_INVALID, rt.capi.RT_ERR_UNSUPPORTED
    p, nr = In(rt, sc.P), In(rt, sc.N)
    o = Out(rt, sc.n, 3, np.float32)
    fp = lambda x: x.ctypes.data_as(C.c_void_p)
    ho = np.zeros((sc.n, 3), F)
    good = lights_of(rt, ONE, WHITE)

    def calls(h, n, m=3, L=good):
        Lp = C.byref(L) if L is not None else None
        return [lib.rt_indirect_diffuse_device(h, Lp, n, p.buf.ptr, nr.buf.ptr, m, SEED, o.buf.ptr, None),
                lib.rt_indirect_diffuse(h, Lp, n, fp(sc.P), fp(sc.N), m, SEED, fp(ho))]

    empty = rt.Context(0)
    try:
        for n in (sc.n, 0):
            assert calls(empty.handle, n) == [rt.capi.RT_ERR_NO_SCENE] * 2
    finally:
        empty.close()
    h = sc.ctx.handle
    assert calls(h, 0) == [0, 0]
    assert calls(h, -1) == [inv, inv]
    for m in (0, 17, -3):
        assert calls(h, sc.n, m=m) == [inv, inv], m
        assert calls(h, 0, m=m) == [inv, inv], m
    assert calls(h, sc.n, L=None) == [inv, inv] and calls(h, 0, L=None) == [inv, inv]
    # the lights, as rt_render checks them; sphere lights are not supported
    for nl in (0, 26, -1):
        bad = lights_of(rt, ONE, WHITE)
        bad.n_lights = nl
        assert calls(h, sc.n, L=bad) == [inv, inv], nl
    bad = lights_of(rt, ONE, WHITE)
    bad.mode = 7
    assert calls(h, sc.n, L=bad) == [inv, inv]
    bad = rt.make_lights(ONE, area=True, usteps=0, vsteps=5)
    assert calls(h, sc.n, L=bad) == [inv, inv]
    sphere = rt.make_lights(ONE, area=True)
    keep = rt.set_sphere(sphere, rt.sphere_offsets(3, 1.0, 25))                     # noqa: F841 -- keeps the offsets alive
    assert calls(h, sc.n, L=sphere) == [uns, uns]
    # NULL pointers, aliasing: an output that shares a byte with an input
    args = lambda pp, pn, po: lib.rt_indirect_diffuse_device(h, C.byref(good), sc.n, pp, pn, 3, SEED, po, None)
    assert args(None, nr.buf.ptr, o.buf.ptr) == inv and args(p.buf.ptr, None, o.buf.ptr) == inv and args(p.buf.ptr, nr.buf.ptr, None) == inv
    assert args(p.buf.ptr, nr.buf.ptr, nr.buf.ptr) == inv
    assert args(p.buf.ptr, nr.buf.ptr, C.c_void_p(p.buf.address + sc.n * 12 - 2)) == inv
    assert lib.rt_indirect_diffuse(h, C.byref(good), sc.n, fp(sc.P), fp(sc.N), 3, SEED, None) == inv
    sc.ctx.synchronize()
    assert o.untouched()
    p.check(); nr.check()
    assert not ho.any()
    # an area light is taken by its positions: the grid is not looked at
    area = rt.make_lights(ONE, area=True, usteps=5, vsteps=5)
    for k in range(3):
        area.color[k] = 1.0
    assert lib.rt_indirect_diffuse(h, C.byref(area), sc.n, fp(sc.P), fp(sc.N), 3, SEED, fp(ho)) == 0
    assert same(ho, sc.want(3))


# ------------------------------------------------------------------------------------------ 8. the context afterwards
def frame(sc, w, h):
    fs = sc.fs
    fs.areaLight, fs.pointLight, fs.usteps, fs.vsteps, fs.max_depth = True, False, 5, 5, 4
    rgb = fs.raytraceScene(w, h, write_ppm=False).copy()
    st = fs.stats
    return rgb, (int(st.launches_total), int(st.rays_primary), int(st.rays_bounce), int(st.rays_centre), int(st.rays_sample),
                 int(st.pixels), int(st.pixels_culled), int(st.shaded_hits))


def test_gather_calls_leave_the_context_as_it_was(world):
    sc = world["mixed"]
    before, counters_before = frame(sc, 64, 40)
    for m in (3, 8, 10):
        assert same(run(sc, sc.P, sc.N, m), sc.want(m))
    after, counters_after = frame(sc, 64, 40)
    assert same(before, after) and counters_before == counters_after
    assert counters_before[0] > 0 and counters_before[1] > 0


def test_gather_on_a_second_stream_beside_a_frame(rt, world):
    sc = world["toy"]
    hip = rt.hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        want_rgb, _ = frame(sc, 64, 40)
        cam = sc.fs.camera
        L, p = sc.fs._lights(), rt.make_params(64, 40, 4)
        rgb = Out(rt, 64 * 40, 3, np.float32)
        rt.capi.check(sc.lib, sc.ctx.handle, sc.lib.rt_render_device(sc.ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.buf.ptr, None, None, None, None),
                      "rt_render_device")
        o, (ip, inr) = run(sc, sc.P, sc.N, 5, stream=stream.value, sync=False)
        assert hip.hipStreamSynchronize(stream) == 0
        sc.ctx.synchronize()
        assert same(o.read().reshape(sc.n, 3), sc.want(5))
        ip.check(); inr.check()
        assert same(rgb.read().reshape(40, 64, 3), want_rgb)
    finally:
        hip.hipStreamDestroy(stream)


def test_refined_count_survives_a_gather_call(world):
    sc = world["cube"]
    fs = sc.fs
    fs.supersample, fs.supersample_threshold = 2, 0.05
    try:
        frame(sc, 64, 40)
        want = sc.ctx.supersampling_refined()
        frame(sc, 64, 40)
        got = run(sc, sc.P, sc.N, 3)
        assert sc.ctx.supersampling_refined() == want and 0 < want < 64 * 40
        assert zero_bits(got)
    finally:
        fs.supersample, fs.supersample_threshold = 1, -1.0
        sc.ctx.set_supersampling(1)
        sc.ctx.set_supersampling_threshold(-1.0)


# ------------------------------------------------------------------------------------------ 9. RT_NO_CULL and the counting build
WORK_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")


@pytest.mark.parametrize("variant", ["no_cull", "counting"])
def test_switch_and_counting_build_give_the_same_bits(rt, world, monkeypatch, variant):
    if variant == "no_cull":
        monkeypatch.setenv("RT_NO_CULL", "1")
    lib = rt.capi.load_library(WORK_LIB) if variant == "counting" else rt.load_library()
    fp = lambda a: a.ctypes.data_as(C.c_void_p)
    L = lights_of(rt, TWO, WHITE)
    for name in ("mixed", "toy"):
        sc = world[name]
        want = sc.want(3, TWO)
        ctx = C.c_void_p()
        assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK                 # (a fresh context: it reads RT_* when it is made and at upload)
        try:
            rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(sc.fs.scene.view)), "rt_upload_scene")
            out = np.full((sc.n, 3), 7, F)
            P, N = np.ascontiguousarray(sc.P), np.ascontiguousarray(sc.N)
            rt.capi.check(lib, ctx, lib.rt_indirect_diffuse(ctx, C.byref(L), sc.n, fp(P), fp(N), 3, SEED, fp(out)), "rt_indirect_diffuse")
        finally:
            lib.rt_destroy(ctx)
        assert same(out, want), (variant, name, differing(out, want))


# ------------------------------------------------------------------------------------------ 10. torch tensors and the Flyscene member
def test_torch_tensors_and_flyscene_member(world):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no device"
    sc = world["toy"]
    rt = sc.rt
    o, d, f, t = sc.rays
    n, m = len(o), 3
    L = lights_of(rt, ONE, YELLOW)
    # the reference of the whole frame: the index of a point is its ray's, misses keep their places and give zeros
    P, N = ao_ref.hit_points(o, d, f, t, sc.osc.arrays()["face_normal"])
    want = ir.gather(sc.tracers["library"], sc.data, P, N, m, SEED, ONE, YELLOW)
    assert zero_bits(want[f < 0]) and same(want[f >= 0][:8], ir.gather(sc.tracers["oracle"], sc.data, P, N, m, SEED, ONE, YELLOW)[f >= 0][:8])
    assert int((want != 0).any(axis=1).sum()) >= 50
    # the composition through DeviceBuffers ...
    io, id_ = In(rt, o), In(rt, d)
    faces, ts = sc.ctx.closest_hits(io.buf, id_.buf, n=n)
    points, normals = sc.ctx.hit_points(io.buf, id_.buf, faces, ts, n=n)
    rgb = sc.ctx.indirect_diffuse(points, normals, L, m, seed=SEED, n=n)
    sc.ctx.synchronize()
    assert same(rgb.to_numpy(F, (n, 3)), want)
    # ... through tensors ...
    dev = f"cuda:{sc.ctx.device}"
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    tf, tt = sc.ctx.closest_hits(to, td)
    tp, tn = sc.ctx.hit_points(to, td, tf, tt)
    trgb = sc.ctx.indirect_diffuse(tp, tn, L, m, seed=SEED)
    sc.ctx.synchronize()
    torch.cuda.synchronize()
    assert trgb.dtype == torch.float32 and tuple(trgb.shape) == (n, 3) and str(trgb.device) == dev
    assert same(trgb.cpu().numpy(), want)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        tp2, tn2 = sc.ctx.hit_points(to.clone(), td.clone(), tf.clone(), tt.clone())
        trgb2 = sc.ctx.indirect_diffuse(tp2, tn2, L, m, seed=SEED)
    s.synchronize()
    assert same(trgb2.cpu().numpy(), want)
    for bad in (tp.double(), torch.zeros((n, 4), dtype=torch.float32, device=dev)):
        with pytest.raises(ValueError):
            sc.ctx.indirect_diffuse(bad, tn, L, m)
    # ... and through the Flyscene member: the same frame (the rays of ao_ref.camera_points are the pinhole rays of that camera)
    fs = sc.fs
    keep = fs.camera
    try:
        fs.camera = rt.default_camera(fs.width, fs.height, 0.4)
        img = fs.indirect_diffuse(W, H, m, seed=SEED, lights=L)
        fs.areaLight, fs.pointLight = False, True
        own = fs.indirect_diffuse(W, H, m, seed=SEED)                        # lights = None: this object's
        params = rt.denoise_params()
        fs.ctx.set_supersampling(3)                                          # the call sets the one-ray pinhole frame itself
        filtered = fs.indirect_diffuse(W, H, m, seed=SEED, lights=L, denoise=params)
        fs.supersample, fs.passes = 1, 1
        g = fs.gbuffer(W, H)
    finally:
        fs.camera = keep
        fs.areaLight, fs.pointLight = True, False
    assert img.shape == (H, W, 3) and img.dtype == np.float32
    assert same(img.reshape(-1, 3), want)
    own_L = fs._lights()
    assert same(own.reshape(-1, 3), ir.gather(sc.tracers["library"], sc.data, P, N, m, SEED, [tuple(own_L.pos[0])], tuple(own_L.color)))
    ref = denoise_ref.denoise(img, g, denoise_ref.Params(params.iterations, params.sigma_color, params.sigma_normal, params.sigma_depth, params.sigma_albedo))
    assert filtered.shape == (H, W, 3) and same(filtered, ref)
    assert not same(filtered, img)
