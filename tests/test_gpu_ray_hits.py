"""rt_ray_hits_device on a real MI355X.  Against the restatement over the CPU checker (tests/ray_hits_ref.py), bit for bit -- faces equal, t
and count as bits -- on single leaves of 12, 64 and 65 faces, the seeded soup and the depth-capped tree, 1,536 interleaved rays per case
(tests/test_ray_hits_cases.py shows what they hold: every list length, ties, faces met in several leaves), unbounded, with a t_max that is
some ray's third hit on the bit, and with non-finite rays in the wave.  Everything else GPU against GPU on the full ray sets: entry 0 is
rt_closest_hits_device's answer on every case of query_walk_cases; k = 1 .. 7 are prefixes of k = 8; a thin batch (lanes = triangles) and a
full one give the same lists; the second grid-stride round repeats the first; outputs, guards, sizes, refusals; uploads, streams, tensors,
frames left alone; the culling switch, other path switches and the counting build; Flyscene.thickness, inside and the signed distance field."""
import ctypes as C
import os

import numpy as np
import pytest

import grid_caps as gc
import query_walk_cases as qc
import ray_hits_ref as rh
import switch_table
from test_gpu_ray_queries import In, Out, bits, same

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")
REF_CASES = ("flat12", "flat64", "flat65", "soup8", "cap38")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORK_LIB = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def run(sc, o, d, k=8, t_max=INF, n=None, faces=True, ts=True, counts=True, stream=None, sync=True):
    """rt_ray_hits_device on DeviceBuffers with guards -> (face (n, k), t (n, k), count (n,)) as read back (None where left out)"""
    n = len(o) if n is None else n
    io, idr = In(sc.rt, o), In(sc.rt, d)
    f = Out(sc.rt, n * k, 1, np.int32) if faces else None
    t = Out(sc.rt, n * k, 1, np.float32) if ts else None
    c = Out(sc.rt, n, 1, np.int32) if counts else None
    sc.ctx.ray_hits(io.buf, idr.buf, k, t_max, n=n, stream=stream, faces=f.buf if f else None, ts=t.buf if t else None,
                    counts=c.buf if c else None, want_faces=faces, want_t=ts, want_counts=counts)
    if not sync:
        return f, t, c, (io, idr)
    sc.ctx.synchronize()
    io.check(); idr.check()
    return (f.read().reshape(n, k) if f else None), (t.read().reshape(n, k) if t else None), (c.read() if c else None)


def assert_equal(got, want, what):
    for g, w, name in zip(got, want, ("face", "t", "count")):
        if g is None:
            continue
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        differ = bits(g) != bits(w)
        bad = np.flatnonzero(differ if differ.ndim == 1 else differ.any(axis=1))
        assert len(bad) == 0, (what, name, len(bad), [(int(i), g[i].tolist(), w[i].tolist()) for i in bad[:4]])


class Scene:
    """a case of query_walk_cases on the GPU with its rays in sorted order; the checker's scene on demand"""

    def __init__(self, rt, oracle, dirpath, name):
        self.rt, self.orc, self.name, self.case, self.dir = rt, oracle, name, qc.CASES[name], dirpath
        self.hs = qc.host_scene(rt, dirpath, name)
        self.ctx = rt.Context(0)
        self.ctx.upload(self.hs)
        self.lib = self.ctx.lib
        self.osc = qc.oracle_scene(oracle, dirpath, name)
        self.arrays = self.osc.arrays()
        self.o, self.d, self.where = qc.sorted_rays(qc.rays(self.arrays, self.case.seed))
        self.idx = qc.interleave(len(self.o))
        self.pick = rh.subset(len(self.o))
        for a in (self.o, self.d):
            a.setflags(write=False)
        self._lists = self._k8 = None

    def lists(self):
        """the restatement's full lists of the subset, once"""
        if self._lists is None:
            self._lists = rh.all_hits(self.osc, self.o[self.pick], self.d[self.pick])
        return self._lists

    def k8(self):
        """k = 8, unbounded, on the full ray set in sorted order, once"""
        if self._k8 is None:
            self._k8 = run(self, self.o, self.d)
            for a in self._k8:
                a.setflags(write=False)
        return self._k8

    def close(self):
        self.ctx.close()
        self.hs.close()
        self.osc.close()


@pytest.fixture(scope="module")
def world(rt, oracle, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Scene(rt, oracle, tmp_path_factory.mktemp("hits"), name)
        return made[name]
    yield get
    for s in made.values():
        s.close()


# ------------------------------------------------------------------------------------------ 1. against the restatement, bit for bit
@pytest.mark.parametrize("name", REF_CASES)
def test_equals_the_restatement(world, name):
    sc = world(name)
    o, d = sc.o[sc.pick], sc.d[sc.pick]
    want = rh.outputs(sc.lists(), 8)
    got = run(sc, o, d)
    print(name, "rays per count 0..9:", np.bincount(want[2], minlength=10).tolist())
    assert_equal(got, want, (name, "k = 8, unbounded"))
    # the same rays inside the full batch in sorted order: other neighbours in the wave, the same lists
    assert_equal(tuple(a[sc.pick] for a in sc.k8()), want, (name, "inside the sorted batch"))


@pytest.mark.parametrize("name", REF_CASES)
def test_t_max_is_inclusive_on_the_bit(world, name):
    sc = world(name)
    o, d = sc.o[sc.pick], sc.d[sc.pick]
    lists = sc.lists()
    third = [i for i, h in enumerate(lists) if len(h) >= 4 and h[2][0] < h[3][0] and h[1][0] < h[2][0]]
    assert third, name
    i = third[len(third) // 2]
    t_max = float(lists[i][2][0])
    cut = [[h for h in r if h[0] <= F(t_max)] for r in lists]
    assert len(cut[i]) == 3 and any(len(a) < len(b) for a, b in zip(cut, lists)) and any(len(a) > 0 for a in cut)
    assert_equal(run(sc, o, d, 8, t_max), rh.outputs(cut, 8), (name, "t_max =", t_max))
    below = float(np.nextafter(F(t_max), F(0)))
    got = run(sc, o[i:i + 1], d[i:i + 1], 8, below)
    assert got[2][0] == 2 and got[0][0, 2] == -1, "one step below the third hit: two hits"
    # the restatement run with t_max itself agrees with the cut (on a few rays: it is slow)
    some = slice(max(0, i - 8), i + 8)
    assert rh.all_hits(sc.osc, o[some], d[some], t_max) == cut[some]


@pytest.mark.parametrize("name", qc.NONFINITE_CASES)
def test_non_finite_rays(world, name):
    sc = world(name)
    o, d, finite = qc.nonfinite_rays(sc.arrays, sc.case.seed)
    want = rh.ray_hits(sc.osc, o, d)
    got = run(sc, o, d)
    assert_equal(got, want, (name, "non-finite"))
    assert (want[2][finite] > 0).any()
    alone = run(sc, o[finite], d[finite])
    assert_equal(alone, tuple(a[finite] for a in got), (name, "the finite rays alone"))


# ------------------------------------------------------------------------------------------ 2. entry 0 is the closest hit, on every case
@pytest.mark.parametrize("name", list(qc.CASES))
def test_first_entry_equals_the_closest_hit(world, name):
    sc = world(name)
    n = len(sc.o)
    io, idr = In(sc.rt, sc.o), In(sc.rt, sc.d)
    cf, ct = Out(sc.rt, n, 1, np.int32), Out(sc.rt, n, 1, np.float32)
    sc.ctx.closest_hits(io.buf, idr.buf, n=n, faces=cf.buf, ts=ct.buf)
    sc.ctx.synchronize()
    cf, ct = cf.read(), ct.read()
    assert 0 < (cf >= 0).sum() < n
    for k, (f, t, c) in ((1, run(sc, sc.o, sc.d, 1)), (8, sc.k8())):
        bad = np.flatnonzero((f[:, 0] != cf) | (bits(t[:, 0]) != bits(ct)))
        assert len(bad) == 0, (name, k, [(int(i), int(f[i, 0]), int(cf[i]), float(t[i, 0]), float(ct[i])) for i in bad[:6]])
        assert np.array_equal(c == 0, cf < 0), (name, k)
    # interleaved: other neighbours in every wave, the same lists
    fi, ti, ci = run(sc, sc.o[sc.idx], sc.d[sc.idx])
    assert_equal((fi, ti, ci), tuple(a[sc.idx] for a in sc.k8()), (name, "interleaved"))


# ------------------------------------------------------------------------------------------ 3. the prefix rule
@pytest.mark.parametrize("name", ("flat65", "soup8", "cap38"))
def test_smaller_k_is_a_prefix(world, name):
    sc = world(name)
    f8, t8, c8 = sc.k8()
    # (the single leaf of 65 faces holds rays of up to seven hits; the soup and the capped tree hold rays of more than eight)
    assert (c8 == 0).any() and ((c8 == 9).any() if name != "flat65" else c8.max() >= 5)
    used = np.arange(8)[None, :] < np.minimum(c8, 8)[:, None]
    assert (f8[~used] == -1).all() and same(t8[~used], np.full(int((~used).sum()), -1.0, F)) and (f8[used] >= 0).all()
    for k in range(1, 8):
        f, t, c = run(sc, sc.o, sc.d, k)
        assert_equal((f, t, c), (np.ascontiguousarray(f8[:, :k]), np.ascontiguousarray(t8[:, :k]), np.minimum(c8, k + 1).astype(np.int32)), (name, k))


# ------------------------------------------------------------------------------------------ 4. both leaf mappings
def test_both_leaf_mappings_give_the_same_lists(world):
    sc = world("soup9")
    f8, t8, c8 = sc.k8()
    leaves = qc.TREES["soup9"]
    m = 6
    assert leaves[2] == (0, 0, 106) and all(qc.tri_mode(cnt, m) for cnt in (65, 400, leaves[3])), "six live rays walk every leaf lanes = triangles"
    assert not qc.tri_mode(65, 64), "a full wave walks the smallest leaves lanes = rays (staged)"
    hit = np.flatnonzero(c8 >= 2)
    assert len(hit) >= 64
    for at in range(0, 60, m):
        pick = hit[at:at + m]
        got = run(sc, sc.o[pick], sc.d[pick])
        assert_equal(got, tuple(a[pick] for a in (f8, t8, c8)), ("soup9", "thin batch", at))
    # a wave of six live rays among rays that miss the root box
    far = np.tile(np.array([[1e6, 1e6, 1e6]], F), (64, 1))
    o, d = far.copy(), np.tile(np.array([[1.0, 0.0, 0.0]], F), (64, 1))
    lanes = np.array([0, 9, 31, 32, 62, 63])
    o[lanes], d[lanes] = sc.o[hit[:6]], sc.d[hit[:6]]
    got = run(sc, o, d)
    assert_equal(tuple(a[lanes] for a in got), tuple(a[hit[:6]] for a in (f8, t8, c8)), ("soup9", "six lanes of a wave"))
    assert (np.delete(got[2], lanes) == 0).all()


# ------------------------------------------------------------------------------------------ 5. the second grid-stride round
def test_the_second_grid_stride_round(world):
    sc = world("flat12")
    cus = gc.cu_count()
    n = gc.query_rays(cus)
    assert gc.strides(n, gc.query_cap(cus)) and gc.query_grid(n, cus) == gc.BLOCKS_PER_CU * cus and n % 64 != 0
    block = 4099                                            # (prime: the copies start at every lane)
    f8, t8, c8 = (a[:block] for a in sc.k8())
    assert_equal((f8, t8, c8), run(sc, sc.o[:block], sc.d[:block]), "the block")
    assert len(np.unique(c8)) >= 4, "lists of 0, 1, 2 and 3 or more hits"
    reps = -(-n // block)
    o, d = np.tile(sc.o[:block], (reps, 1))[:n], np.tile(sc.d[:block], (reps, 1))[:n]
    f, t, c = run(sc, o, d, 4)
    for name_, got, first in (("face", f, f8[:, :4]), ("t", t, t8[:, :4]), ("count", c, np.minimum(c8, 5))):
        want = np.tile(first, (reps,) + (1,) * (first.ndim - 1))[:n]
        assert np.array_equal(bits(got), bits(np.ascontiguousarray(want).astype(got.dtype))), name_


# ------------------------------------------------------------------------------------------ 6. outputs, guards, sizes, refusals
def test_optional_outputs_and_sizes(world):
    sc = world("soup8")
    f8, t8, c8 = sc.k8()
    for n in (1, 63, 64, 65):
        for k in (8, 3):
            want = (np.ascontiguousarray(f8[:n, :k]), np.ascontiguousarray(t8[:n, :k]), np.minimum(c8[:n], k + 1).astype(np.int32))
            assert_equal(run(sc, sc.o[:n], sc.d[:n], k), want, (n, k))
    want = tuple(np.ascontiguousarray(a[:65]) for a in (f8, t8, c8))
    for faces, ts, counts in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        got = run(sc, sc.o[:65], sc.d[:65], faces=faces, ts=ts, counts=counts)
        assert [g is not None for g in got] == [faces, ts, counts]
        assert_equal(got, want, (faces, ts, counts))
    # n below the buffers' length: the rest stays as it was (the guards of Out begin at n * k and n)
    got = run(sc, sc.o[:200], sc.d[:200], 5, n=70)
    assert_equal(got, (np.ascontiguousarray(f8[:70, :5]), np.ascontiguousarray(t8[:70, :5]), np.minimum(c8[:70], 6).astype(np.int32)), "n = 70 of 200")


def test_refusals(rt, world):
    sc = world("flat12")
    lib, h, capi = sc.lib, sc.ctx.handle, rt.capi
    n, k = 64, 8
    buf = rt.hipmem.DeviceBuffer(n * 4 * (3 + 3 + k + k + 1))
    o = buf.address
    d, f = o + n * 12, o + n * 24
    t, c = f + n * k * 4, f + 2 * n * k * 4
    call = lambda *a: lib.rt_ray_hits_device(h, *a, None)                                     # noqa: E731
    inv = capi.RT_ERR_INVALID
    assert call(n, o, d, k, INF, f, t, c) == capi.RT_OK
    assert call(0, None, None, k, INF, None, None, None) == capi.RT_OK
    assert call(0, None, None, 0, INF, None, None, None) == inv and call(0, None, None, k, float("nan"), None, None, None) == inv
    assert call(-1, o, d, k, INF, f, t, c) == inv
    assert call(n, None, d, k, INF, f, t, c) == inv and call(n, o, None, k, INF, f, t, c) == inv
    for bad_k in (0, 9, -3):
        assert call(n, o, d, bad_k, INF, f, t, c) == inv and b"k must be" in lib.rt_last_error(h)
    for bad_t in (float("nan"), 0.0, -1.0, -INF):
        assert call(n, o, d, k, bad_t, f, t, c) == inv and b"t_max" in lib.rt_last_error(h)
    assert call(n, o, d, k, INF, None, None, None) == inv and b"all null" in lib.rt_last_error(h)
    assert call(n, o, d, k, 1e-30, f, None, None) == capi.RT_OK and call(n, o, d, 1, INF, None, t, None) == capi.RT_OK and call(n, o, d, k, INF, None, None, c) == capi.RT_OK
    for bad in ((d + n * 12 - 4, t, c), (f, o, c), (f, t, d + 4)):
        assert call(n, o, d, k, INF, *bad) == inv and b"overlaps an input" in lib.rt_last_error(h), bad
    assert call(n, o, d, k, INF, f, f + n * k * 4 - 4, c) == inv and b"two outputs" in lib.rt_last_error(h)
    assert call(n, o, d, k, INF, f, t, t + 4) == inv and call(n, o, d, k, INF, c - n * k * 4 + 4, None, c) == inv
    assert call(n, o, d, 4, INF, f, f + n * 4 * 4, c) == capi.RT_OK, "k = 4: the ranges are half as long"
    assert lib.rt_ray_hits_device(None, n, o, d, k, INF, f, t, c, None) == inv
    sc.ctx.synchronize()
    # the host-pointer form refuses the same and answers the same
    O, D = np.array(sc.o[:n]), np.array(sc.d[:n])
    hf, ht, hc = np.zeros((n, k), np.int32), np.zeros((n, k), F), np.zeros(n, np.int32)
    p = lambda a: a.ctypes.data                                                                # noqa: E731
    assert lib.rt_ray_hits(h, n, p(O), p(D), 9, INF, p(hf), p(ht), p(hc)) == inv
    assert lib.rt_ray_hits(h, n, p(O), p(D), k, 0.0, p(hf), p(ht), p(hc)) == inv
    assert lib.rt_ray_hits(h, n, p(O), p(D), k, INF, None, None, None) == inv
    assert lib.rt_ray_hits(h, n, p(O), p(D), k, INF, p(hf), p(ht), p(hc)) == capi.RT_OK
    assert_equal((hf, ht, hc), tuple(np.ascontiguousarray(a[:n]) for a in sc.k8()), "host pointers")
    only = np.zeros(n, np.int32)
    assert lib.rt_ray_hits(h, n, p(O), p(D), 2, INF, None, None, p(only)) == capi.RT_OK and np.array_equal(only, np.minimum(hc, 3))
    fresh = rt.Context(0)
    try:
        assert lib.rt_ray_hits_device(fresh.handle, n, o, d, k, INF, f, t, c, None) == capi.RT_ERR_NO_SCENE
        assert lib.rt_ray_hits(fresh.handle, n, p(O), p(D), k, INF, p(hf), p(ht), p(hc)) == capi.RT_ERR_NO_SCENE
    finally:
        fresh.close()
        buf.free()


# ------------------------------------------------------------------------------------------ 7. the context and streams
def test_a_second_upload_changes_the_answers(rt, world):
    a, b = world("flat12"), world("soup8")
    ctx = rt.Context(0)
    me = type("S", (), {"rt": rt, "ctx": ctx})
    try:
        ctx.upload(a.hs)
        assert_equal(run(me, a.o[:2048], a.d[:2048]), tuple(x[:2048] for x in a.k8()), "first scene")
        ctx.upload(b.hs)
        assert_equal(run(me, b.o[:2048], b.d[:2048]), tuple(x[:2048] for x in b.k8()), "second scene on the live context")
        ctx.upload(a.hs)
        assert_equal(run(me, a.o[:2048], a.d[:2048], 3), (a.k8()[0][:2048, :3], a.k8()[1][:2048, :3], np.minimum(a.k8()[2][:2048], 4)), "and back")
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def fly(rt, scenes):
    fs = rt.Flyscene(scene_path=os.path.join(scenes, "dodgeColorTest.obj"))
    fs.initialize(64, 40, True, False)
    yield fs
    fs.ctx.close()
    fs.scene.close()


def frame(fs, w=64, h=40):
    fs.areaLight, fs.pointLight, fs.usteps, fs.vsteps, fs.max_depth = True, False, 5, 5, 4
    rgb = fs.raytraceScene(w, h, write_ppm=False).copy()
    st = fs.stats
    return rgb, (int(st.launches_total), int(st.rays_primary), int(st.rays_bounce), int(st.rays_centre), int(st.rays_sample), int(st.pixels),
                 int(st.pixels_culled), int(st.shaded_hits))


def camera_rays(rt, fs, w, h):
    """the pinhole rays of the object's camera: (origins, directions) float32 (w * h, 3)"""
    pts = np.empty((w * h, 3), F)
    cam = fs.camera if (w, h) == (fs.width, fs.height) else None
    if cam is None:
        cam = rt.default_camera(w, h)
        cam.center, cam.inv_view = fs.camera.center, fs.camera.inv_view
    rt.capi.check(fs.ctx.lib, fs.ctx.handle, fs.ctx.lib.rt_primary_points(fs.ctx.handle, C.byref(cam), w, h, pts.ctypes.data_as(C.POINTER(C.c_float))),
                  "rt_primary_points")
    centre = np.asarray(list(cam.center), F)
    return np.ascontiguousarray(np.broadcast_to(centre, pts.shape)), (pts - centre).astype(F)


def test_calls_leave_the_context_as_it_was(rt, fly):
    me = type("S", (), {"rt": rt, "ctx": fly.ctx})
    o, d = camera_rays(rt, fly, 64, 40)
    fly.supersample, fly.supersample_threshold = 2, 0.05
    try:
        before, counters_before = frame(fly)
        refined = fly.ctx.supersampling_refined()
        first = run(me, o, d)
        assert (first[2] > 0).any()
        assert fly.ctx.supersampling_refined() == refined and refined > 0
        after, counters_after = frame(fly)
        assert same(before, after) and counters_before == counters_after and counters_before[0] > 0
        assert_equal(run(me, o, d), first, "after a frame")
    finally:
        fly.supersample, fly.supersample_threshold = 1, -1.0


def test_a_call_on_a_second_stream_beside_a_frame(rt, fly):
    me = type("S", (), {"rt": rt, "ctx": fly.ctx})
    o, d = camera_rays(rt, fly, 64, 40)
    hip = rt.hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        want_rgb, _ = frame(fly)
        want = run(me, o, d)
        cam, L, p = fly.camera, fly._lights(), rt.make_params(64, 40, 4)
        rgb = Out(rt, 64 * 40, 3, np.float32)
        rt.capi.check(fly.ctx.lib, fly.ctx.handle,
                      fly.ctx.lib.rt_render_device(fly.ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.buf.ptr, None, None, None, None), "rt_render_device")
        f, t, c, ins = run(me, o, d, stream=stream.value, sync=False)
        assert hip.hipStreamSynchronize(stream) == 0
        fly.ctx.synchronize()
        n = len(o)
        assert_equal((f.read().reshape(n, 8), t.read().reshape(n, 8), c.read()), want, "beside a frame")
        for a in ins:
            a.check()
        assert same(rgb.read().reshape(40, 64, 3), want_rgb)
    finally:
        hip.hipStreamDestroy(stream)


def test_torch_tensors_on_the_current_stream(world):
    import torch
    sc = world("soup8")
    f8, t8, c8 = sc.k8()
    O, D = (torch.from_numpy(np.array(a[:300])).to("cuda:0") for a in (sc.o, sc.d))
    with torch.cuda.stream(torch.cuda.Stream(0)):
        f, t, c = sc.ctx.ray_hits(O, D, 8)
        f1, t1, c1 = sc.ctx.ray_hits(O, D, 1, want_counts=False)
        torch.cuda.current_stream(0).synchronize()
    assert tuple(f.shape) == (300, 8) and f.dtype == torch.int32 and t.dtype == torch.float32 and tuple(c.shape) == (300,)
    assert_equal((f.cpu().numpy(), t.cpu().numpy(), c.cpu().numpy()), tuple(np.ascontiguousarray(a[:300]) for a in (f8, t8, c8)), "tensors")
    assert c1 is None and tuple(f1.shape) == (300, 1) and np.array_equal(f1.cpu().numpy()[:, 0], f8[:300, 0]) and same(t1.cpu().numpy()[:, 0], np.ascontiguousarray(t8[:300, 0]))
    f, t, c = sc.ctx.ray_hits(O, D, 2, t_max=0.5)                    # torch's default stream
    assert (c.cpu().numpy() <= 3).all() and (t.cpu().numpy() <= 0.5).all()
    with pytest.raises(ValueError):
        sc.ctx.ray_hits(O, D, 9)
    with pytest.raises(ValueError):
        sc.ctx.ray_hits(O, D[:-1].contiguous(), 8)


# ------------------------------------------------------------------------------------------ 8. switches and the counting build
@pytest.mark.parametrize("env", [{"RT_NO_CULL": "1"}, {"RT_STAGED_TRACE": "0"}, {"RT_TRACE_BUDGET": "1", "RT_TASK_TARGET": "1"}, {"RT_NO_SHAFT": "1", "RT_NO_BEAM": "1"}],
                         ids=lambda e: "+".join(e))
@pytest.mark.parametrize("name", ("soup8", "cap38"))
def test_path_switches_give_the_same_bits(rt, world, monkeypatch, name, env):
    sc = world(name)
    want = sc.k8()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    other = rt.Context(0)
    try:
        other.upload(sc.hs)
        me = type("S", (), {"rt": rt, "ctx": other})
        assert_equal(run(me, sc.o, sc.d), want, (name, env))
        pick = sc.idx[:2048]
        assert_equal(run(me, sc.o[pick], sc.d[pick], 2, 0.75), run(sc, sc.o[pick], sc.d[pick], 2, 0.75), (name, env, "k = 2, bounded"))
    finally:
        other.close()


@pytest.mark.parametrize("name", ("flat65", "soup8"))
def test_counting_build_gives_the_same_bits(rt, world, name):
    lib = rt.capi.load_library(WORK_LIB)
    sc = world(name)
    ctx = C.c_void_p()
    assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
    try:
        rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(sc.hs.view)), "rt_upload_scene")
        n = 4096
        O, D = np.array(sc.o[sc.idx[:n]]), np.array(sc.d[sc.idx[:n]])
        p = lambda a: a.ctypes.data                                                            # noqa: E731
        for k in (8, 3):
            f, t, c = np.full((n, k), 7, np.int32), np.full((n, k), 7, F), np.full(n, 7, np.int32)
            rt.capi.check(lib, ctx, lib.rt_ray_hits(ctx, n, p(O), p(D), k, INF, p(f), p(t), p(c)), "rt_ray_hits")
            f8, t8, c8 = (a[sc.idx[:n]] for a in sc.k8())
            assert_equal((f, t, c), (np.ascontiguousarray(f8[:, :k]), np.ascontiguousarray(t8[:, :k]), np.minimum(c8, k + 1).astype(np.int32)), (name, k))
    finally:
        lib.rt_destroy(ctx)


# ------------------------------------------------------------------------------------------ 9. the front ends
W, H = 48, 32


@pytest.fixture(scope="module")
def cube(rt, oracle, scenes):
    path = os.path.join(scenes, "cube.obj")
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(W, H, True, False)
    osc = oracle.load_scene(path)
    yield fs, osc
    osc.close()
    fs.ctx.close()
    fs.scene.close()


def test_thickness_equals_the_restatement(rt, cube):
    fs, osc = cube
    o, d = camera_rays(rt, fs, W, H)
    _, t, c = rh.ray_hits(osc, o, d)
    thick, more = fs.thickness(W, H)
    assert thick.shape == (H, W) and thick.dtype == F and more.shape == (H, W) and more.dtype == bool
    assert same(thick, rt.thickness_of(t, c).reshape(H, W)) and not more.any()
    through = c.reshape(H, W) >= 2
    # (a ray through an edge of the cube meets two faces at one t: a pair of thickness zero, so "> 0" holds for the plain pixels only)
    assert through.any() and (~through).any() and (thick >= 0).all() and (thick[c.reshape(H, W) == 0] == 0).all()
    # the same by hand on the pixels whose ray enters and leaves the box: t of the exit minus t of the entry
    two = np.flatnonzero(c == 2)
    assert len(two) > 0 and same(thick.reshape(-1)[two], (t[two, 1] - t[two, 0]).astype(F)) and (thick.reshape(-1)[two] > 0).sum() >= len(two) - 8


def test_inside_and_the_signed_distance_field(rt, cube):
    fs, osc = cube
    box = np.asarray(fs.scene.info()["root_box"], F)
    lo, hi = box[:3], box[3:]
    rng = np.random.default_rng(3)
    inner = (lo + (F(0.05) + F(0.9) * rng.random((40, 3), dtype=F)) * (hi - lo)).astype(F)
    outer = inner.copy()
    side = rng.integers(0, 3, 40)
    outer[np.arange(40), side] = np.where(rng.integers(0, 2, 40) == 1, hi[side] + F(0.3) * (hi - lo)[side], lo[side] - F(0.3) * (hi - lo)[side])
    P = np.concatenate([inner, outer]).astype(F)
    for direction in ((1.0, 0.0, 0.0), (0.3, -0.8, 0.52)):
        got = fs.inside(P, direction)
        assert got.dtype == np.int8 and got.shape == (80,)
        _, _, c = rh.ray_hits(osc, P, np.broadcast_to(np.asarray(direction, F), P.shape))
        assert np.array_equal(got, rt.parity_of(c)), direction
        assert (got[:40] == 1).all() and (got[40:] == 0).all(), (direction, got.tolist())
    dims, margin = (5, 4, 3), 0.25
    pg, dist, faces = fs.distance_field(dims, margin=margin)
    pg2, sdist, sfaces, undecided = fs.distance_field(dims, margin=margin, signed=True)
    pos = rt.probe_grid_positions(pg)
    side = fs.inside(pos)
    assert bytes(pg) == bytes(pg2) and np.array_equal(faces, sfaces) and undecided.dtype == bool and not undecided.any()
    assert same(sdist, np.where(side == 1, -dist, dist).astype(F))
    strictly = ((pos > lo) & (pos < hi)).all(axis=1)
    assert strictly.any() and (sdist[strictly] < 0).all() and (sdist[((pos < lo) | (pos > hi)).any(axis=1)] > 0).all()
    assert len(fs.distance_field(dims, margin=margin, signed=False)) == 3
