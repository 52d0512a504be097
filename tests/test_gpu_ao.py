"""Ambient occlusion on a real MI355X: rt_ambient_occlusion_device returns, per point, bit for bit the count tests/ao_ref.py gets from the
CPU checker's lightStrikes (and rt_light_strikes on the reference segments), in every wave layout, for every batch length around the layout
boundaries, writes nothing behind element n, and leaves the context as it was; rt_hit_points_device equals its restatement."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ao_ref
import grid_caps as gc
import scenes_gen

pytestmark = pytest.mark.gpu

F = np.float32
# K = 1, 4, 9, 25, 36, 64, 100, 256: a wave unit is 64 / gcd(K, 64) = 64, 16, 64, 64, 16, 1, 16, 1 points in K / gcd(K, 64) = 1, 1, 9, 25, 9, 1, 25, 4
# rounds: K dividing 64 (one round), 64 dividing K, and the K whose points straddle rounds
GRIDS = (1, 2, 3, 5, 6, 8, 10, 16)
RADIUS, SEED = 0.5, 7
GUARD = 64                                   # elements behind every output, holding PATTERN bytes
PATTERN = 0xA5
W, H = 48, 32
FILES = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj", "toy": "toy.obj"}


def group(m):
    return 64 // math.gcd(m * m, 64)


class In:
    """an input array on the device; check(): it still holds what was uploaded"""

    def __init__(self, rt, a, dtype=np.float32):
        self.a = np.ascontiguousarray(a, dtype)
        self.buf = rt.hipmem.DeviceBuffer(max(4, self.a.nbytes)).from_numpy(self.a)

    def check(self):
        assert np.array_equal(self.buf.to_numpy(np.uint8, (self.a.nbytes,)), self.a.reshape(-1).view(np.uint8)), "an input was written"


class Out:
    """an output of n * per elements with GUARD elements of PATTERN behind it; read(): the values, after checking the guards"""

    def __init__(self, rt, n, per, dtype):
        self.n, self.per, self.dtype = n, per, np.dtype(dtype)
        self.init = np.full((n * per + GUARD) * self.dtype.itemsize, PATTERN, np.uint8)
        self.buf = rt.hipmem.DeviceBuffer(self.init.nbytes).from_numpy(self.init)

    def read(self):
        raw = self.buf.to_numpy(np.uint8, self.init.shape)
        k = self.n * self.per * self.dtype.itemsize
        assert (raw[k:] == PATTERN).all(), "elements behind n were written"
        return raw[:k].view(self.dtype).reshape((self.n, self.per) if self.per > 1 else (self.n,))

    def untouched(self):
        return (self.buf.to_numpy(np.uint8, self.init.shape) == PATTERN).all()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


class Scene:
    """a scene on the GPU and in the CPU checker, its fixed point set (the closest hits of the 48 x 32 camera at yaw 0.4, ao_ref.camera_points)
    and the reference counts of that set, computed once per (m, radius, seed)"""

    def __init__(self, rt, oracle, path):
        self.rt, self.orc = rt, oracle
        self.fs = rt.Flyscene(scene_path=path)
        self.fs.initialize(64, 40, True, False)
        self.ctx, self.lib = self.fs.ctx, self.fs.ctx.lib
        self.osc = oracle.load_scene(path)
        self.rays, (self.P, self.N) = ao_ref.camera_points(oracle, self.osc, W, H, 0.4)
        self.n = len(self.P)
        self.ref = {}

    def strikes(self, P, Q):
        """rt_light_strikes on the segments Q[i, k] -> P[i]: visible, bool (n, K)"""
        n, K = Q.shape[0], Q.shape[1]
        hit = np.ascontiguousarray(np.broadcast_to(P[:, None, :], Q.shape), F)
        light = np.ascontiguousarray(Q, F)
        vis = np.full(n * K, 7, np.uint8)
        fp = lambda a: a.ctypes.data_as(C.c_void_p)
        self.rt.capi.check(self.lib, self.ctx.handle, self.lib.rt_light_strikes(self.ctx.handle, n * K, fp(hit), fp(light), fp(vis)), "rt_light_strikes")
        assert ((vis == 0) | (vis == 1)).all()
        return vis.reshape(n, K).astype(bool)

    def counts_by_strikes(self, P, N, seed, m, radius):
        Q = ao_ref.segments(P, N, np.arange(len(P)), seed, m, radius)
        c = self.strikes(P, Q).sum(axis=1).astype(np.uint16)
        c[~ao_ref.is_point(N)] = m * m
        return c

    def counts(self, m, radius=RADIUS, seed=SEED, by="oracle"):
        key = (m, radius, seed)
        if key not in self.ref:
            if by == "oracle":
                self.ref[key] = ao_ref.counts(self.osc, self.P, self.N, seed, m, radius)
            else:
                self.ref[key] = self.counts_by_strikes(self.P, self.N, seed, m, radius)
            self.ref[key].setflags(write=False)
        return self.ref[key]

    def close(self):
        self.ctx.close()
        self.fs.scene.close()
        self.osc.close()


@pytest.fixture(scope="module")
def world(rt, oracle, scenes, tmp_path_factory):
    paths = {k: os.path.join(scenes, v) for k, v in FILES.items()}
    paths["mixed"] = scenes_gen.mixed_materials(str(tmp_path_factory.mktemp("mixed")))
    w = {k: Scene(rt, oracle, p) for k, p in paths.items()}
    yield w
    for s in w.values():
        s.close()


def run_ao(sc, P, N, m, radius=RADIUS, seed=SEED, want_open=True, want_ao=True, stream=None, sync=True):
    """rt_ambient_occlusion_device on DeviceBuffers with guards -> (open, ao) as read back (None where left out)"""
    n = len(P)
    p, nr = In(sc.rt, P.reshape(-1, 3) if n else np.zeros((1, 3), F)), In(sc.rt, N.reshape(-1, 3) if n else np.zeros((1, 3), F))
    o = Out(sc.rt, n, 1, np.uint16) if want_open else None
    a = Out(sc.rt, n, 1, np.float32) if want_ao else None
    sc.ctx.ambient_occlusion(p.buf, nr.buf, m, radius, seed=seed, n=n, open=o.buf if o else None, ao=a.buf if a else None,
                             want_open=want_open, want_ao=want_ao, stream=stream)
    if not sync:
        return o, a, (p, nr)
    sc.ctx.synchronize()
    p.check(); nr.check()
    return (o.read() if o else None), (a.read() if a else None)


# ------------------------------------------------------------------------------------------ 1. every layout on every scene
@pytest.mark.parametrize("name", ["mixed", "toy", "dodge", "cube"])
def test_counts_equal_the_reference_in_every_layout(world, name):
    sc = world[name]
    assert sc.n == {"mixed": 93, "toy": 360, "dodge": 242, "cube": 561}[name]
    for m in GRIDS:
        K = m * m
        want = sc.counts(m, by="strikes" if (name == "toy" and m > 8) else "oracle")      # (the CPU checker takes seconds on toy above m = 8)
        got_open, got_ao = run_ao(sc, sc.P, sc.N, m)
        assert got_open.dtype == np.uint16 and np.array_equal(got_open, want), (name, m, np.flatnonzero(got_open != want)[:8])
        assert same(got_ao, ao_ref.ao_of(want, m)), (name, m)
        if name == "cube":
            assert (want == K).all(), "a convex scene occludes nothing"
    if name in ("mixed", "toy"):
        c = sc.counts(3)
        assert int(((c > 0) & (c < 9)).sum()) >= 80, "the fixture must hold partly occluded points"


def test_strikes_reference_equals_the_oracle_reference(world):
    """the two references of this file agree where both are affordable (so either may stand for the definition)"""
    for name, m in (("mixed", 3), ("toy", 5), ("dodge", 8)):
        sc = world[name]
        assert np.array_equal(sc.counts(m), sc.counts_by_strikes(sc.P, sc.N, SEED, m, RADIUS)), (name, m)


# ------------------------------------------------------------------------------------------ 2. batch lengths around the layout boundaries
@pytest.mark.parametrize("m", GRIDS)
def test_batch_lengths_guards_and_null_outputs(world, m):
    sc = world["mixed"]
    g = group(m)
    want = sc.counts(m)
    want_ao = ao_ref.ao_of(want, m)
    for n in sorted({0, 1, max(g - 1, 0), g, g + 1, 63, 64, 65}):
        # (point i of a call is rotated by its index i: a prefix of the batch is the batch of the prefix)
        for want_open, want_a in ((True, True), (True, False), (False, True)):
            o, a = run_ao(sc, sc.P[:n], sc.N[:n], m, want_open=want_open, want_ao=want_a)
            if want_open:
                assert np.array_equal(o, want[:n]), (m, n)
            if want_a:
                assert same(a, want_ao[:n]), (m, n)
    p, nr = In(sc.rt, sc.P), In(sc.rt, sc.N)
    assert sc.lib.rt_ambient_occlusion_device(sc.ctx.handle, 65, p.buf.ptr, nr.buf.ptr, m, RADIUS, SEED, None, None, None) == sc.rt.capi.RT_ERR_INVALID


# ------------------------------------------------------------------------------------------ 3. more units than the grid holds
@pytest.mark.parametrize("name,m,n", [("cube", 16, 40000), ("toy", 1, 8192 * 64 + 64 * 5 + 3), ("mixed", 2, 8192 * 16 + 16 * 3 + 2)])
def test_grid_stride(world, name, m, n):
    """the grid is at most 8 blocks of 4 waves per CU, 8192 wave units on 256 CUs, times the rounds of a unit up to 4 (rt_ao_layout.hpp): these
    batches hold more units, in the one-round kernel and in the kernel of several rounds, so waves stride"""
    sc = world[name]
    units, rounds = -(-n // group(m)), m * m // math.gcd(m * m, 64)
    cus = gc.cu_count(sc.ctx.device)
    assert units > gc.ao_cap(cus, rounds) and gc.ao_grid(units, cus, rounds) * gc.WAVES < units, (cus, units, "the batch does not reach the grid of this device")
    reps = -(-n // sc.n)
    P, N = np.tile(sc.P, (reps, 1))[:n], np.tile(sc.N, (reps, 1))[:n]
    want = sc.counts_by_strikes(P, N, SEED, m, RADIUS)
    o, a = run_ao(sc, P, N, m)
    assert np.array_equal(o, want), np.flatnonzero(o != want)[:8]
    assert same(a, ao_ref.ao_of(want, m))
    if name == "cube":
        assert (o == m * m).all()
    else:
        assert 0 < int((want < m * m).sum()) < n


# ------------------------------------------------------------------------------------------ 4. "no point" inputs
@pytest.mark.parametrize("m", [3, 8, 10])
def test_zero_normals_are_open_and_leave_the_others_alone(world, m):
    sc = world["mixed"]
    N = sc.N.copy()
    N[0::3] = 0.0
    N[3::6, 1] = -0.0                                          # (either sign of zero)
    want = sc.counts(m).copy()
    assert (want[0::3] < m * m).any()
    want[0::3] = m * m
    o, a = run_ao(sc, sc.P, N, m)
    assert np.array_equal(o, want) and same(a, ao_ref.ao_of(want, m))
    assert same(a[0::3], np.full(len(a[0::3]), 1.0, F))
    # all of them: no wave has an active lane
    o, a = run_ao(sc, sc.P, np.zeros_like(sc.N), m)
    assert (o == m * m).all() and same(a, np.full(sc.n, 1.0, F))


# ------------------------------------------------------------------------------------------ 5. hit points
def run_hit_points(sc, o, d, f, t):
    n = len(o)
    io, id_, if_, it = In(sc.rt, o), In(sc.rt, d), In(sc.rt, f, np.int32), In(sc.rt, t)
    p, nr = Out(sc.rt, n, 3, np.float32), Out(sc.rt, n, 3, np.float32)
    sc.ctx.hit_points(io.buf, id_.buf, if_.buf, it.buf, n=n, points=p.buf, normals=nr.buf)
    sc.ctx.synchronize()
    for x in (io, id_, if_, it):
        x.check()
    return p.read(), nr.read()


@pytest.mark.parametrize("name", ["cube", "dodge", "mixed"])
def test_hit_points_equal_the_reference(world, name):
    sc = world[name]
    o, d, f, t = (x.copy() for x in sc.rays)
    fn = sc.osc.arrays()["face_normal"]
    nf = fn.shape[0]
    assert same(fn, sc.fs.scene.arrays()["face_normal"]), "the uploaded normals are the checker's"
    assert 0 < int((f >= 0).sum()) < len(f), "the frame must hold hits and misses"
    hits = np.flatnonzero(f >= 0)
    for k, bad in zip(hits[:6], (nf, nf + 5, -7, np.iinfo(np.int32).max, np.iinfo(np.int32).min, -2)):
        f[k] = bad                                             # ids outside [0, n_faces) with a finite t: six zeros, nothing indexed
    d[hits[6:12]] = -d[hits[6:12]]                             # rays that look the other way: the normal is not flipped / is flipped
    wantP, wantN = ao_ref.hit_points(o, d, f, t, fn)
    P, N = run_hit_points(sc, o, d, f, t)
    assert same(P, wantP) and same(N, wantN)
    out = ~((f >= 0) & (f < nf))
    assert not P[out].any() and not N[out].any() and not np.signbit(N[out]).any() and not np.signbit(P[out]).any()
    if name == "cube":                                         # axis-aligned normals: zeros whose sign bit the flip sets
        live = N[~out]
        assert ((live == 0) & np.signbit(live)).any() and ((live == 0) & ~np.signbit(live)).any()
    for n in (1, 63, 65, 257):                                 # the block boundary
        P, N = run_hit_points(sc, o[:n], d[:n], f[:n], t[:n])
        assert same(P, wantP[:n]) and same(N, wantN[:n]), n


# ------------------------------------------------------------------------------------------ 6. the chain, on the device
@pytest.mark.parametrize("name", ["toy", "mixed"])
def test_closest_hits_to_hit_points_to_occlusion(world, name):
    sc = world[name]
    o, d, f, t = sc.rays
    n, m = len(o), 3
    io, id_ = In(sc.rt, o), In(sc.rt, d)
    faces, ts = sc.ctx.closest_hits(io.buf, id_.buf, n=n)
    points, normals = sc.ctx.hit_points(io.buf, id_.buf, faces, ts, n=n)
    opn, ao = sc.ctx.ambient_occlusion(points, normals, m, RADIUS, seed=SEED, n=n)
    sc.ctx.synchronize()
    assert np.array_equal(faces.to_numpy(np.int32, (n,)), f)
    P, N = ao_ref.hit_points(o, d, f, t, sc.osc.arrays()["face_normal"])
    assert same(points.to_numpy(F, (n, 3)), P) and same(normals.to_numpy(F, (n, 3)), N)
    want = ao_ref.counts(sc.osc, P, N, SEED, m, RADIUS)          # (the index of a point is its ray's: misses keep their places)
    assert np.array_equal(opn.to_numpy(np.uint16, (n,)), want) and same(ao.to_numpy(F, (n,)), ao_ref.ao_of(want, m))
    assert (want[f < 0] == m * m).all() and (want[f >= 0] < m * m).any()


# ------------------------------------------------------------------------------------------ 7. seeds
def test_seeds(world):
    sc = world["mixed"]
    a, _ = run_ao(sc, sc.P, sc.N, 3, seed=7)
    b, _ = run_ao(sc, sc.P, sc.N, 3, seed=8)
    a2, _ = run_ao(sc, sc.P, sc.N, 3, seed=7)
    assert np.array_equal(a, a2) and not np.array_equal(a, b)
    assert np.array_equal(b, ao_ref.counts(sc.osc, sc.P, sc.N, 8, 3, RADIUS))
    c, _ = run_ao(sc, sc.P, sc.N, 3, seed=0xFFFFFFFF)
    assert np.array_equal(c, ao_ref.counts(sc.osc, sc.P, sc.N, 0xFFFFFFFF, 3, RADIUS))


# ------------------------------------------------------------------------------------------ 8. the context afterwards
def frame(sc, w, h):
    fs = sc.fs
    fs.areaLight, fs.pointLight, fs.usteps, fs.vsteps, fs.max_depth = True, False, 5, 5, 4
    rgb = fs.raytraceScene(w, h, write_ppm=False).copy()
    st = fs.stats
    return rgb, (int(st.launches_total), int(st.rays_primary), int(st.rays_bounce), int(st.rays_centre), int(st.rays_sample),
                 int(st.pixels), int(st.pixels_culled), int(st.shaded_hits))


def test_ao_calls_leave_the_context_as_it_was(world):
    sc = world["mixed"]
    before, counters_before = frame(sc, 64, 40)
    for m in (3, 8, 10):
        o, _ = run_ao(sc, sc.P, sc.N, m)
        assert np.array_equal(o, sc.counts(m))
    run_hit_points(sc, *sc.rays)
    after, counters_after = frame(sc, 64, 40)
    assert same(before, after) and counters_before == counters_after
    assert counters_before[0] > 0 and counters_before[1] > 0


def test_ao_on_a_second_stream_beside_a_frame(rt, world):
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
        o, a, (ip, inr) = run_ao(sc, sc.P, sc.N, 5, stream=stream.value, sync=False)
        assert hip.hipStreamSynchronize(stream) == 0
        sc.ctx.synchronize()
        assert np.array_equal(o.read(), sc.counts(5)) and same(a.read(), ao_ref.ao_of(sc.counts(5), 5))
        ip.check(); inr.check()
        assert same(rgb.read().reshape(40, 64, 3), want_rgb)
    finally:
        hip.hipStreamDestroy(stream)


def test_refined_count_survives_an_ao_call(world):
    sc = world["cube"]
    fs = sc.fs
    fs.supersample, fs.supersample_threshold = 2, 0.05
    try:
        frame(sc, 64, 40)
        want = sc.ctx.supersampling_refined()
        frame(sc, 64, 40)
        o, _ = run_ao(sc, sc.P, sc.N, 3)
        assert sc.ctx.supersampling_refined() == want and 0 < want < 64 * 40
        assert (o == 9).all()
    finally:
        fs.supersample, fs.supersample_threshold = 1, -1.0
        sc.ctx.set_supersampling(1)
        sc.ctx.set_supersampling_threshold(-1.0)


# ------------------------------------------------------------------------------------------ 9. RT_NO_CULL and the counting build
WORK_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")


@pytest.mark.parametrize("variant", ["no_cull", "counting"])
def test_switch_and_counting_build_give_the_same_counts(rt, world, monkeypatch, variant):
    if variant == "no_cull":
        monkeypatch.setenv("RT_NO_CULL", "1")
    lib = rt.capi.load_library(WORK_LIB) if variant == "counting" else rt.load_library()
    fp = lambda a: a.ctypes.data_as(C.c_void_p)
    for name in ("mixed", "toy"):
        sc = world[name]
        ctx = C.c_void_p()
        assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK                 # (a fresh context: it reads RT_* when it is made and at upload)
        try:
            rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(sc.fs.scene.view)), "rt_upload_scene")
            o, a = np.full(sc.n, 0xA5A5, np.uint16), np.full(sc.n, 7, F)
            P, N = np.ascontiguousarray(sc.P), np.ascontiguousarray(sc.N)
            rt.capi.check(lib, ctx, lib.rt_ambient_occlusion(ctx, sc.n, fp(P), fp(N), 3, RADIUS, SEED, fp(o), fp(a)), "rt_ambient_occlusion")
        finally:
            lib.rt_destroy(ctx)
        assert np.array_equal(o, sc.counts(3)) and same(a, ao_ref.ao_of(sc.counts(3), 3)), (variant, name)


# ------------------------------------------------------------------------------------------ 10. refusals
def test_no_scene_and_bad_arguments(rt, world):
    sc = world["mixed"]
    lib, inv = sc.lib, rt.capi.RT_ERR_INVALID
    p, nr = In(rt, sc.P), In(rt, sc.N)
    f, t = In(rt, sc.rays[2][:sc.n], np.int32), In(rt, sc.rays[3][:sc.n])
    o, a = Out(rt, sc.n, 1, np.uint16), Out(rt, sc.n, 1, np.float32)
    op, on = Out(rt, sc.n, 3, np.float32), Out(rt, sc.n, 3, np.float32)
    fp = lambda x: x.ctypes.data_as(C.c_void_p)
    ho, ha = np.zeros(sc.n, np.uint16), np.zeros(sc.n, F)

    def calls(h, n, m=3, radius=0.5):
        return [lib.rt_ambient_occlusion_device(h, n, p.buf.ptr, nr.buf.ptr, m, radius, SEED, o.buf.ptr, a.buf.ptr, None),
                lib.rt_ambient_occlusion(h, n, fp(sc.P), fp(sc.N), m, radius, SEED, fp(ho), fp(ha))]

    def hp(h, n):
        return lib.rt_hit_points_device(h, n, p.buf.ptr, nr.buf.ptr, f.buf.ptr, t.buf.ptr, op.buf.ptr, on.buf.ptr, None)

    empty = rt.Context(0)
    try:
        for n in (sc.n, 0):
            assert calls(empty.handle, n) == [rt.capi.RT_ERR_NO_SCENE] * 2 and hp(empty.handle, n) == rt.capi.RT_ERR_NO_SCENE
    finally:
        empty.close()
    h = sc.ctx.handle
    assert calls(h, 0) == [0, 0] and hp(h, 0) == 0
    assert calls(h, -1) == [inv, inv] and hp(h, -1) == inv
    for m in (0, 17, -3):
        assert calls(h, sc.n, m=m) == [inv, inv], m
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        assert calls(h, sc.n, radius=radius) == [inv, inv], radius
        assert calls(h, 0, radius=radius) == [inv, inv], radius
    # NULL inputs, aliasing: an output that shares a byte with an input
    assert lib.rt_ambient_occlusion_device(h, sc.n, None, nr.buf.ptr, 3, 0.5, SEED, o.buf.ptr, a.buf.ptr, None) == inv
    assert lib.rt_ambient_occlusion_device(h, sc.n, p.buf.ptr, None, 3, 0.5, SEED, o.buf.ptr, a.buf.ptr, None) == inv
    assert lib.rt_ambient_occlusion_device(h, sc.n, p.buf.ptr, nr.buf.ptr, 3, 0.5, SEED, o.buf.ptr, nr.buf.ptr, None) == inv
    assert lib.rt_ambient_occlusion_device(h, sc.n, p.buf.ptr, nr.buf.ptr, 3, 0.5, SEED, C.c_void_p(p.buf.address + sc.n * 12 - 2), a.buf.ptr, None) == inv
    assert lib.rt_hit_points_device(h, sc.n, p.buf.ptr, nr.buf.ptr, f.buf.ptr, t.buf.ptr, p.buf.ptr, on.buf.ptr, None) == inv
    assert lib.rt_hit_points_device(h, sc.n, p.buf.ptr, nr.buf.ptr, f.buf.ptr, t.buf.ptr, op.buf.ptr, C.c_void_p(t.buf.address + 4), None) == inv
    assert lib.rt_hit_points_device(h, sc.n, p.buf.ptr, nr.buf.ptr, None, t.buf.ptr, op.buf.ptr, on.buf.ptr, None) == inv
    sc.ctx.synchronize()
    assert o.untouched() and a.untouched() and op.untouched() and on.untouched()
    p.check(); nr.check()
    assert not ho.any() and not ha.any()


# ------------------------------------------------------------------------------------------ 11. torch tensors and the Flyscene member
def test_torch_tensors_and_flyscene_member(world):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no device"
    sc = world["toy"]
    o, d, f, t = sc.rays
    n, m = len(o), 6
    # the composition through DeviceBuffers ...
    io, id_ = In(sc.rt, o), In(sc.rt, d)
    faces, ts = sc.ctx.closest_hits(io.buf, id_.buf, n=n)
    points, normals = sc.ctx.hit_points(io.buf, id_.buf, faces, ts, n=n)
    opn, ao = sc.ctx.ambient_occlusion(points, normals, m, RADIUS, seed=SEED, n=n)
    sc.ctx.synchronize()
    want_open, want_ao = opn.to_numpy(np.uint16, (n,)), ao.to_numpy(F, (n,))
    assert 0 < int((want_open < m * m).sum()) < n
    # ... through tensors ...
    dev = f"cuda:{sc.ctx.device}"
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    tf, tt = sc.ctx.closest_hits(to, td)
    tp, tn = sc.ctx.hit_points(to, td, tf, tt)
    topn, tao = sc.ctx.ambient_occlusion(tp, tn, m, RADIUS, seed=SEED)
    sc.ctx.synchronize()
    torch.cuda.synchronize()
    assert topn.dtype == torch.uint16 and tao.dtype == torch.float32 and tuple(tao.shape) == (n,) and str(tao.device) == dev
    assert np.array_equal(topn.cpu().numpy(), want_open) and same(tao.cpu().numpy(), want_ao)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        tp2, tn2 = sc.ctx.hit_points(to.clone(), td.clone(), tf.clone(), tt.clone())
        _, tao2 = sc.ctx.ambient_occlusion(tp2, tn2, m, RADIUS, seed=SEED, want_open=False)
    s.synchronize()
    assert same(tao2.cpu().numpy(), want_ao)
    for bad in (tp.double(), torch.zeros((n, 4), dtype=torch.float32, device=dev)):
        with pytest.raises(ValueError):
            sc.ctx.ambient_occlusion(bad, tn, m, RADIUS)
    with pytest.raises(ValueError):
        sc.ctx.hit_points(to, td, tf.float(), tt)
    # ... and through the Flyscene member: the same frame (the rays of ao_ref.camera_points are the pinhole rays of that camera)
    fs = sc.fs
    keep = fs.camera
    try:
        fs.camera = sc.rt.default_camera(fs.width, fs.height, 0.4)
        img = fs.ambient_occlusion(W, H, m, RADIUS, seed=SEED)
    finally:
        fs.camera = keep
    assert img.shape == (H, W) and img.dtype == np.float32
    assert same(img.reshape(-1), want_ao)
    assert same(img.reshape(-1)[f < 0], np.full(int((f < 0).sum()), 1.0, F))
