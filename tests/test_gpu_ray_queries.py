"""Device ray queries on a real MI355X: rt_closest_hits_device, rt_light_strikes_device and rt_trace_rays_device return, on caller-owned
device buffers, bit for bit what rt_trace_rays / rt_light_strikes return through host memory (and the CPU checker's closest hit), write
nothing behind element n, leave their inputs and the context as they were, and do not depend on the chunk size; k_closest and k_segments
return the same per ray in batches larger than their grids (tests/grid_caps.py), where waves stride to a second round."""
import ctypes as C
import os

import numpy as np
import pytest

import grid_caps as gc
import scenes_gen

pytestmark = pytest.mark.gpu

PREFIXES = (1, 63, 64, 65, 264, 1500)       # one lane, the wave boundary from both sides, 4 x 64 + 8, all
GUARD = 64                                   # elements behind every output, holding PATTERN bytes
PATTERN = 0xA5


def awkward_rays():
    """the rays and segment points of test_gpu_parity.test_trace_rays_and_light_strikes_batch, by the same construction (seed 1234): zero
    direction components, origins inside the root box, tiny directions; then the 700 points it draws for its first and its second scene"""
    rng = np.random.default_rng(1234)
    n = 1500
    o = (rng.random((n, 3), dtype=np.float32) - 0.5) * 3.0
    d = (rng.random((n, 3), dtype=np.float32) - 0.5) * 2.0
    d[:100, 0] = 0.0
    d[100:200, 1] = 0.0
    d[200:260, 0] = 0.0
    d[200:260, 2] = 0.0
    o[300:400] *= 0.1
    d[400:420] *= 1e-6
    o[500:600] = (0.0, 0.0, 2.0)
    d[500:600] = (rng.random((100, 3), dtype=np.float32) - 0.5) * np.float32(0.6) + np.array([0, -0.3, -1], np.float32)
    hit = np.array([0.05, -0.3, 0.1], np.float32)
    pts = {}
    for name in ("dodge", "cube"):
        p = (rng.random((700, 3), dtype=np.float32) - 0.5) * 4.0
        p[:50, 0] = hit[0]
        pts[name] = p
    return o, d, hit, pts


class Scene:
    """a scene on the GPU with the reference results of the 1500 rays, computed once through the host-pointer calls"""

    def __init__(self, rt, path, rays):
        self.rt = rt
        self.fs = rt.Flyscene(scene_path=path)
        self.fs.initialize(256, 256, True, False)
        self.ctx, self.lib = self.fs.ctx, self.fs.ctx.lib
        self.o, self.d = rays
        self.ref = {}

    def trace_ref(self, u, depth):
        """rt_trace_rays of all 1500 rays (per-ray results: a prefix of the batch is the batch of the prefix)"""
        if (u, depth) not in self.ref:
            fs = self.fs
            fs.areaLight, fs.pointLight, fs.usteps, fs.vsteps, fs.max_depth = True, False, u, u, depth
            rgb = fs.traceRay(self.o, self.d)
            self.ref[(u, depth)] = (rgb.copy(), fs.last_face.copy(), fs.last_t.copy())
        return self.ref[(u, depth)]

    def lights(self, u):
        return self.rt.make_lights(area=True, usteps=u, vsteps=u)

    def close(self):
        self.ctx.close()
        self.fs.scene.close()


@pytest.fixture(scope="module")
def rays():
    return awkward_rays()


@pytest.fixture(scope="module")
def world(rt, scenes, rays, tmp_path_factory):
    o, d, _, _ = rays
    paths = {"cube": os.path.join(scenes, "cube.obj"), "dodge": os.path.join(scenes, "dodgeColorTest.obj"),
             "mixed": scenes_gen.mixed_materials(str(tmp_path_factory.mktemp("mixed")))}
    w = {k: Scene(rt, p, (o, d)) for k, p in paths.items()}
    yield w
    for s in w.values():
        s.close()


class In:
    """an input array on the device; check(): it still holds what was uploaded"""

    def __init__(self, rt, a):
        self.a = np.ascontiguousarray(a, np.float32)
        self.buf = rt.hipmem.DeviceBuffer(max(4, self.a.nbytes)).from_numpy(self.a)

    def check(self):
        assert np.array_equal(self.buf.to_numpy(np.float32, self.a.shape).view(np.uint32), self.a.view(np.uint32)), "an input was written"


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def closest(sc, n, faces=True, ts=True, rays=None):
    """rt_closest_hits_device of the first n of the 1500 rays, or of the n rays (origins, directions) in `rays`"""
    o, d = (In(sc.rt, sc.o[:n]), In(sc.rt, sc.d[:n])) if rays is None else (In(sc.rt, rays[0]), In(sc.rt, rays[1]))
    f = Out(sc.rt, n, 1, np.int32) if faces else None
    t = Out(sc.rt, n, 1, np.float32) if ts else None
    sc.ctx.closest_hits(o.buf, d.buf, n=n, faces=f.buf if f else None, ts=t.buf if t else None, want_faces=faces, want_t=ts)
    sc.ctx.synchronize()
    o.check(); d.check()
    return (f.read() if f else None), (t.read() if t else None)


def traced(sc, n, u, depth, hits=True, stream=None):
    """-> the three Out objects of an enqueued rt_trace_rays_device (not synchronised) and its inputs"""
    o, d = In(sc.rt, sc.o[:n]), In(sc.rt, sc.d[:n])
    rgb = Out(sc.rt, n, 3, np.float32)
    f = Out(sc.rt, n, 1, np.int32) if hits else None
    t = Out(sc.rt, n, 1, np.float32) if hits else None
    sc.ctx.trace_rays_device(sc.lights(u), o.buf, d.buf, max_depth=depth, want_hits=hits, n=n, rgb=rgb.buf,
                             faces=f.buf if f else None, ts=t.buf if t else None, stream=stream)
    return rgb, f, t, (o, d)


def assert_traced(sc, got, n, u, depth):
    rgb, f, t, (o, d) = got
    want_rgb, want_f, want_t = sc.trace_ref(u, depth)
    assert same(rgb.read(), want_rgb[:n]), (n, u, depth)
    if f is not None:
        assert np.array_equal(f.read(), want_f[:n]) and same(t.read(), want_t[:n]), (n, u, depth)
    o.check(); d.check()


# ------------------------------------------------------------------------------------------ 1. closest hits
@pytest.mark.parametrize("name", ["cube", "dodge", "mixed"])
def test_closest_hits_equal_trace_rays(world, name):
    sc = world[name]
    _, want_f, want_t = sc.trace_ref(5, 3)
    for n in PREFIXES:
        f, t = closest(sc, n)
        assert np.array_equal(f, want_f[:n]) and same(t, want_t[:n]), n
        miss = f < 0
        assert (f[miss] == -1).all() and same(t[miss], np.full(int(miss.sum()), -1.0, np.float32)), n
    n = 264
    f, _ = closest(sc, n, ts=False)
    _, t = closest(sc, n, faces=False)
    assert np.array_equal(f, want_f[:n]) and same(t, want_t[:n])
    assert 0 < int((want_f >= 0).sum()) < 1500, "the rays must hold hits and misses"
    # both outputs NULL
    o, d = In(sc.rt, sc.o[:n]), In(sc.rt, sc.d[:n])
    assert sc.lib.rt_closest_hits_device(sc.ctx.handle, n, o.buf.ptr, d.buf.ptr, None, None, None) == sc.rt.capi.RT_ERR_INVALID
    # the host-pointer call
    hf, ht = np.full(1500, 7, np.int32), np.full(1500, 7, np.float32)
    fp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert sc.lib.rt_closest_hits(sc.ctx.handle, 1500, fp(sc.o), fp(sc.d), fp(hf), fp(ht)) == 0
    assert np.array_equal(hf, want_f) and same(ht, want_t)


@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_closest_hits_equal_the_cpu_checker(world, oracle, scenes, name):
    sc = world[name]
    osc = oracle.load_scene(os.path.join(scenes, {"cube": "cube.obj", "dodge": "dodgeColorTest.obj"}[name]))
    f, t = closest(sc, 1500)
    for i in range(1500):
        wf, wt = osc.closest_hit(sc.o[i], sc.d[i])
        assert f[i] == wf, i
        if wf >= 0:
            assert np.float32(t[i]) == np.float32(wt), i
    osc.close()


# ------------------------------------------------------------------------------------------ 2. light strikes
@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_light_strikes_device_equals_light_strikes(world, rays, name):
    sc = world[name]
    _, _, hit, pts = rays
    p = pts[name]
    _, want = sc.fs.lightStrikes(hit, p)
    assert 0 < int(want.sum()) < 700, "the segments must hold visible and blocked ones"
    for n in (700, 1, 65):
        h, l = In(sc.rt, np.broadcast_to(hit, (n, 3))), In(sc.rt, p[:n])
        v = Out(sc.rt, n, 1, np.uint8)
        sc.ctx.light_strikes_device(h.buf, l.buf, n=n, vis=v.buf)
        sc.ctx.synchronize()
        assert np.array_equal(v.read(), want[:n].astype(np.uint8)), n
        h.check(); l.check()


# ------------------------------------------------------------------------------------------ 2b. more rays than the grid holds
def strided_batch(sc, m, mul):
    """n beyond the grid of the lane = ray kernels for the context's device (at least a quarter of a grid's worth of rays in round 2, the
    last wave a partial one) and a map of 0 .. n - 1 onto 0 .. m - 1 that takes every value and is not periodic in a wave or a grid"""
    cus = gc.cu_count(sc.ctx.device)
    n = gc.query_rays(cus)
    assert gc.strides(n, gc.query_cap(cus)) and gc.query_grid(n, cus) * gc.QUERY_BLOCK < n and n % 64 != 0, (cus, n)
    i = np.arange(n, dtype=np.int64)
    idx = (i * mul + i // m) % m
    cap = gc.query_cap(cus)
    assert len(np.unique(idx)) == m and (idx[:64] != idx[64:128]).any() and (idx[:n - cap] != idx[cap:]).any()
    return n, idx


@pytest.mark.parametrize("name", ["cube", "dodge", "mixed"])
def test_closest_hits_beyond_the_grid(world, name):
    """k_closest in its second round: the waves' LDS stacks are used again, the last wave has dead lanes, and each output is optional"""
    sc = world[name]
    n, idx = strided_batch(sc, 1500, 7)
    _, want_f, want_t = sc.trace_ref(5, 3)
    rays = (sc.o[idx], sc.d[idx])
    f, t = closest(sc, n, rays=rays)
    assert np.array_equal(f, want_f[idx]), np.flatnonzero(f != want_f[idx])[:8]
    assert same(t, want_t[idx]), np.flatnonzero(bits(t) != bits(want_t[idx]))[:8]
    miss = f < 0
    assert 0 < int(miss.sum()) < n and (f[miss] == -1).all() and same(t[miss], np.full(int(miss.sum()), -1.0, np.float32))
    f, _ = closest(sc, n, ts=False, rays=rays)
    _, t = closest(sc, n, faces=False, rays=rays)
    assert np.array_equal(f, want_f[idx]) and same(t, want_t[idx])


@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_light_strikes_beyond_the_grid(world, rays, name):
    sc = world[name]
    _, _, hit, pts = rays
    n, idx = strided_batch(sc, 700, 3)
    _, want = sc.fs.lightStrikes(hit, pts[name])
    want = want.astype(np.uint8)
    assert 0 < int(want.sum()) < 700
    h, l = In(sc.rt, np.broadcast_to(hit, (n, 3))), In(sc.rt, pts[name][idx])
    v = Out(sc.rt, n, 1, np.uint8)
    sc.ctx.light_strikes_device(h.buf, l.buf, n=n, vis=v.buf)
    sc.ctx.synchronize()
    got = v.read()
    assert np.array_equal(got, want[idx]), np.flatnonzero(got != want[idx])[:8]
    h.check(); l.check()


# ------------------------------------------------------------------------------------------ 3. traced colour
@pytest.mark.parametrize("name,u,depth", [("cube", 5, 3), ("dodge", 5, 3), ("mixed", 5, 3), ("mixed", 5, 0), ("mixed", 8, 4)])
def test_trace_rays_device_equals_trace_rays(world, name, u, depth):
    sc = world[name]
    for n in PREFIXES:
        got = traced(sc, n, u, depth)
        sc.ctx.synchronize()
        assert_traced(sc, got, n, u, depth)
    got = traced(sc, 264, u, depth, hits=False)         # face / t pointers NULL
    sc.ctx.synchronize()
    assert_traced(sc, got, 264, u, depth)
    if name == "mixed" and depth == 4:
        rgb3, rgb0 = sc.trace_ref(5, 3)[0], sc.trace_ref(5, 0)[0]
        assert not same(rgb3, rgb0), "the mixed-material rays must bounce"


# ------------------------------------------------------------------------------------------ 4. chunks
@pytest.mark.parametrize("name", ["cube", "dodge", "mixed"])
def test_chunks_do_not_change_the_result(world, name):
    sc = world[name]
    inv = sc.rt.capi.RT_ERR_INVALID
    try:
        sc.ctx.set_query_chunk(64)
        for n in (264, 64):                                        # five chunks, the last of 8 rays; exactly one
            got = traced(sc, n, 5, 3)
            sc.ctx.synchronize()
            assert_traced(sc, got, n, 5, 3)
        # out of range: refused, the setting stays (264 rays still run as five chunks: same result, and more launches than one sequence)
        assert sc.lib.rt_set_query_chunk(sc.ctx.handle, 63) == inv and sc.lib.rt_set_query_chunk(sc.ctx.handle, (1 << 24) + 1) == inv
        got = traced(sc, 264, 5, 3)
        sc.ctx.synchronize()
        assert_traced(sc, got, 264, 5, 3)
        # two calls back to back on one stream, no synchronise in between
        a = traced(sc, 264, 5, 3)
        b = traced(sc, 65, 5, 3)
        sc.ctx.synchronize()
        assert_traced(sc, a, 264, 5, 3)
        assert_traced(sc, b, 65, 5, 3)
    finally:
        sc.ctx.set_query_chunk(1 << 22)
    a = traced(sc, 1500, 5, 3)
    b = traced(sc, 264, 5, 3)
    sc.ctx.synchronize()
    assert_traced(sc, a, 1500, 5, 3)
    assert_traced(sc, b, 264, 5, 3)


# ------------------------------------------------------------------------------------------ 5. the context afterwards
def frame(sc, w, h):
    fs = sc.fs
    fs.areaLight, fs.pointLight, fs.usteps, fs.vsteps, fs.max_depth = True, False, 5, 5, 4
    rgb = fs.raytraceScene(w, h, write_ppm=False).copy()
    st = fs.stats
    return rgb, (int(st.launches_total), int(st.rays_primary), int(st.rays_bounce), int(st.rays_centre), int(st.rays_sample),
                 int(st.pixels), int(st.pixels_culled), int(st.shaded_hits))


def test_queries_leave_the_context_as_it_was(world, rays):
    sc = world["cube"]
    _, _, hit, pts = rays
    before, counters_before = frame(sc, 64, 40)
    got = traced(sc, 264, 5, 3)
    closest(sc, 65)
    h, l = In(sc.rt, np.broadcast_to(hit, (65, 3))), In(sc.rt, pts["cube"][:65])
    sc.ctx.light_strikes_device(h.buf, l.buf, n=65)
    sc.ctx.synchronize()
    assert_traced(sc, got, 264, 5, 3)
    after, counters_after = frame(sc, 64, 40)
    assert same(before, after) and counters_before == counters_after
    assert counters_before[0] > 0 and counters_before[1] > 0


def test_refined_count_survives_a_query(world):
    sc = world["cube"]
    fs = sc.fs
    fs.supersample, fs.supersample_threshold = 2, 0.05
    try:
        frame(sc, 64, 40)
        want = sc.ctx.supersampling_refined()
        frame(sc, 64, 40)
        got = traced(sc, 264, 5, 3)
        assert sc.ctx.supersampling_refined() == want and 0 < want < 64 * 40
        assert_traced(sc, got, 264, 5, 3)
    finally:
        fs.supersample, fs.supersample_threshold = 1, -1.0
        sc.ctx.set_supersampling(1)
        sc.ctx.set_supersampling_threshold(-1.0)


# ------------------------------------------------------------------------------------------ 6. no scene, no rays
def test_no_scene_and_no_rays(rt, world):
    sc = world["cube"]
    lib, L = sc.lib, sc.lights(5)
    o, d = In(rt, sc.o[:64]), In(rt, sc.d[:64])
    rgb, f, t, v = Out(rt, 0, 3, np.float32), Out(rt, 0, 1, np.int32), Out(rt, 0, 1, np.float32), Out(rt, 0, 1, np.uint8)

    def calls(h, n):
        fp = lambda a: a.ctypes.data_as(C.c_void_p)
        hf, ht = np.zeros(64, np.int32), np.zeros(64, np.float32)
        return [lib.rt_closest_hits_device(h, n, o.buf.ptr, d.buf.ptr, f.buf.ptr, t.buf.ptr, None),
                lib.rt_closest_hits(h, n, fp(sc.o), fp(sc.d), fp(hf), fp(ht)),
                lib.rt_light_strikes_device(h, n, o.buf.ptr, d.buf.ptr, v.buf.ptr, None),
                lib.rt_trace_rays_device(h, C.byref(L), 3, n, o.buf.ptr, d.buf.ptr, rgb.buf.ptr, f.buf.ptr, t.buf.ptr, None)]

    empty = rt.Context(0)
    try:
        assert calls(empty.handle, 64) == [rt.capi.RT_ERR_NO_SCENE] * 4
        assert calls(empty.handle, 0) == [rt.capi.RT_ERR_NO_SCENE] * 4
    finally:
        empty.close()
    assert calls(sc.ctx.handle, 0) == [0] * 4
    sc.ctx.synchronize()
    assert rgb.untouched() and f.untouched() and t.untouched() and v.untouched()
    assert calls(sc.ctx.handle, -1) == [rt.capi.RT_ERR_INVALID] * 4


# ------------------------------------------------------------------------------------------ 6b. the host forms with an output left out
def test_host_forms_with_one_output_and_with_no_rays(rt, world):
    """the host-pointer forms stage an optional output only where the caller gives one: either output alone is the matching column of the
    call with both, bit for bit (130 rays: two full waves and two lanes), and n = 0 with null pointers is RT_OK"""
    sc = world["cube"]
    lib, h, n = sc.lib, sc.ctx.handle, 130
    fp = lambda a: a.ctypes.data_as(C.c_void_p)
    o, d = np.ascontiguousarray(sc.o[:n]), np.ascontiguousarray(sc.d[:n])

    def hits(faces, ts):
        f, t = (np.full(n, 7, np.int32) if faces else None), (np.full(n, 7, np.float32) if ts else None)
        assert lib.rt_closest_hits(h, n, fp(o), fp(d), fp(f) if faces else None, fp(t) if ts else None) == 0
        return f, t

    f, t = hits(True, True)
    df, dt = closest(sc, n)
    assert np.array_equal(f, df) and same(t, dt) and 0 < int((f >= 0).sum()) < n
    assert np.array_equal(hits(True, False)[0], f) and same(hits(False, True)[1], t)

    # points and normals of those hits (six zeros for a miss: fully open), from the device calls
    bo, bd = In(rt, o), In(rt, d)
    bf, bt = sc.ctx.closest_hits(bo.buf, bd.buf, n=n)
    bp, bn = sc.ctx.hit_points(bo.buf, bd.buf, bf, bt, n=n)
    sc.ctx.synchronize()
    p, nr = bp.to_numpy(np.float32, (n, 3)), bn.to_numpy(np.float32, (n, 3))
    for b in (bf, bt, bp, bn):
        b.free()

    def occlusion(want_open, want_ao):
        op, ao = (np.full(n, 7, np.uint16) if want_open else None), (np.full(n, 7, np.float32) if want_ao else None)
        assert lib.rt_ambient_occlusion(h, n, fp(p), fp(nr), 2, 0.5, 11, fp(op) if want_open else None, fp(ao) if want_ao else None) == 0
        return op, ao

    op, ao = occlusion(True, True)
    assert op.max() <= 4 and same(ao, op.astype(np.float32) / np.float32(4))
    assert np.array_equal(occlusion(True, False)[0], op) and same(occlusion(False, True)[1], ao)

    assert [lib.rt_closest_hits(h, 0, None, None, None, None), lib.rt_light_strikes(h, 0, None, None, None),
            lib.rt_ambient_occlusion(h, 0, None, None, 2, 0.5, 11, None, None), lib.rt_box_intersect(h, 0, None, None, None, None),
            lib.rt_debug_phong_samples(h, 0, None, None, None, None, None, None, None, None),
            lib.rt_tree_probe(h, 0, None, None, None, None, None)] == [0] * 6


# ------------------------------------------------------------------------------------------ 7. torch tensors
def test_torch_tensors(world):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    sc = world["dodge"]
    n = 264
    dev = f"cuda:{sc.ctx.device}"
    o, d = torch.from_numpy(sc.o[:n]).to(dev), torch.from_numpy(sc.d[:n]).to(dev)
    want_rgb, want_f, want_t = sc.trace_ref(5, 3)
    f, t = sc.ctx.closest_hits(o, d)
    rgb, f2, t2 = sc.ctx.trace_rays_device(sc.lights(5), o, d, max_depth=3, want_hits=True)
    sc.ctx.synchronize()
    torch.cuda.synchronize()
    assert f.dtype == torch.int32 and t.dtype == torch.float32 and rgb.shape == (n, 3) and str(rgb.device) == dev
    assert np.array_equal(f.cpu().numpy(), want_f[:n]) and same(t.cpu().numpy(), want_t[:n])
    assert np.array_equal(f2.cpu().numpy(), want_f[:n]) and same(t2.cpu().numpy(), want_t[:n]) and same(rgb.cpu().numpy(), want_rgb[:n])
    # ... and on a stream of torch's own: asynchronous, ordered by that stream
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        o2, d2 = o.clone(), d.clone()
        rgb2 = sc.ctx.trace_rays_device(sc.lights(5), o2, d2, max_depth=3)
        f3, _ = sc.ctx.closest_hits(o2, d2)
    s.synchronize()
    assert same(rgb2.cpu().numpy(), want_rgb[:n]) and np.array_equal(f3.cpu().numpy(), want_f[:n])
    sc.ctx.synchronize()
    for bad in (o.double(), torch.from_numpy(sc.o[:2 * n]).to(dev)[::2], torch.zeros((n, 4), dtype=torch.float32, device=dev)):
        with pytest.raises(ValueError):
            sc.ctx.closest_hits(bad, d)
        with pytest.raises(ValueError):
            sc.ctx.trace_rays_device(sc.lights(5), o, bad)
        with pytest.raises(ValueError):
            sc.ctx.light_strikes_device(bad, d)


# ------------------------------------------------------------------------------------------ 8. the orthographic helper, end to end
def test_orthographic_view_of_the_cube(rt, world, oracle, scenes):
    sc = world["cube"]
    w, h = 24, 16
    o, d = rt.rays.orthographic_rays(rt.default_camera(w, h), w, h, 0.9)
    oi, di = In(rt, o), In(rt, d)
    f, t = sc.ctx.closest_hits(oi.buf, di.buf, n=w * h)
    sc.ctx.synchronize()
    f, t = f.to_numpy(np.int32, (w * h,)), t.to_numpy(np.float32, (w * h,))
    osc = oracle.load_scene(os.path.join(scenes, "cube.obj"))
    for i in range(w * h):
        wf, wt = osc.closest_hit(o[i], d[i])
        assert f[i] == wf, i
        if wf >= 0:
            assert np.float32(t[i]) == np.float32(wt), i
    osc.close()
    assert (f >= 0).any() and (f < 0).any()
