"""rt_closest_points_device on a real MI355X: face, dist2 and point equal brute force over the referenced faces (tests/closest_point_ref.py,
the numpy restatement of the header's definition) in every bit -- tolerance 0 -- on the flat cube, on dodgeColorTest, on a seeded soup, a
depth-capped tree with over-full leaves, lost nodes and unreachable faces, single leaves of 12, 64 and 65 faces and scales 2^-20 and 2^20;
for coherent grids, the same points shuffled, hit points a few ulps off their faces, vertices, edge midpoints and centroids, points 1e4
extents away and non-finite ones; for the radii +inf, 0, the median distance and one step below and above a point's own distance; for n =
1, 63, 64, 65, 257 and a batch that takes a second grid-stride round.  The calls refuse what the header says they refuse, leave the context
and a frame beside them as they were, and rebuild their bounds after a second upload.  The facade's field and clearance are the same numbers.

A finite radius needs no second brute force: the candidates are the faces with d2 <= r2, so the answer is the unbounded answer where its
d2 <= r2 and "none" elsewhere (a smaller d2 would have been the unbounded answer)."""
import ctypes as C
import os

import numpy as np
import pytest

import closest_point_ref as cp
import grid_caps as gc
import query_walk_cases as qc
import switch_table
from test_closest_points_api import scene_of_query, unreachable_probe_points
from test_gpu_ray_queries import In, Out, bits, same

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")
SCENES = ("cube", "dodge", "soup8", "cap34", "flat12", "flat64", "flat65", "soup8_2^-20", "soup8_2^20")
PREFIXES = (1, 63, 64, 65, 257)
FIRST_FACES = 16


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def run(sc, P, max_dist=INF, n=None, faces=True, dist2=True, closest=True, stream=None, sync=True):
    """rt_closest_points_device on DeviceBuffers with guards -> (face, dist2, point) as read back (None where left out)"""
    n = len(P) if n is None else n
    p = In(sc.rt, P if len(P) else np.zeros((1, 3), F))
    f = Out(sc.rt, n, 1, np.int32) if faces else None
    d = Out(sc.rt, n, 1, np.float32) if dist2 else None
    q = Out(sc.rt, n, 3, np.float32) if closest else None
    sc.ctx.closest_points(p.buf, max_dist, n=n, stream=stream, faces=f.buf if f else None, dist2=d.buf if d else None, closest=q.buf if q else None,
                          want_faces=faces, want_dist2=dist2, want_closest=closest)
    if not sync:
        return f, d, q, p
    sc.ctx.synchronize()
    p.check()
    return (f.read() if f else None), (d.read() if d else None), (q.read() if q else None)


def within(want, P, max_dist):
    """the unbounded answer `want` cut at a radius (see the module's docstring)"""
    f, d, q = want
    with np.errstate(over="ignore"):
        r2 = F(max_dist) * F(max_dist)
    keep = (f >= 0) & (d <= r2)
    return np.where(keep, f, -1).astype(np.int32), np.where(keep, d, F(np.inf)).astype(F), np.where(keep[:, None], q, P).astype(F)


def assert_equal(got, want, what):
    for g, w, name in zip(got, want, ("face", "dist2", "point")):
        if g is None:
            continue
        differ = (g != w) if name == "face" else (bits(g) != bits(w))
        bad = np.flatnonzero(differ if differ.ndim == 1 else differ.any(axis=1))
        assert len(bad) == 0, (what, name, len(bad), [(int(i), g[i].tolist(), w[i].tolist(), int(want[0][i])) for i in bad[:6]])


def step_ulps(x, k):
    """x moved by k float32 steps (k < 0: down)"""
    out = x.astype(F).copy()
    for _ in range(abs(k)):
        out = np.nextafter(out, F(np.inf) if k > 0 else F(-np.inf))
    return out


class Scene:
    """a scene on the GPU, its referenced faces and its point sets with the unbounded brute-force answer, computed once"""

    def __init__(self, rt, scenes, dirpath, name):
        self.rt, self.name = rt, name
        if name in ("cube", "dodge"):
            self.hs = rt.HostScene(os.path.join(scenes, {"cube": "cube.obj", "dodge": "dodgeColorTest.obj"}[name]))
        else:
            self.hs = qc.host_scene(rt, dirpath, name)
        self.ctx = rt.Context(0)
        self.ctx.upload(self.hs)
        self.lib = self.ctx.lib
        self.info = self.hs.info()
        self.a, self.faces = scene_of_query(self.hs)
        self.tv = self.a["tri_verts"]
        self.sets = self.point_sets()
        self.P = np.ascontiguousarray(np.concatenate(list(self.sets.values())), F)
        self.where, at = {}, 0
        for k, v in self.sets.items():
            self.where[k] = slice(at, at + len(v))
            at += len(v)
        # (the shuffled points are the grid's: their answers are the grid's, permuted -- one brute force less)
        rest = cp.brute_force(self.P[self.where["hits"].start:], self.tv, self.faces)
        grid = cp.brute_force(self.sets["grid"], self.tv, self.faces)
        self.want = tuple(np.concatenate([g, g[self.perm], r]) for g, r in zip(grid, rest))
        for a in (self.P,) + self.want:
            a.setflags(write=False)

    def point_sets(self):
        rng = np.random.default_rng(77)
        box = np.asarray(self.info["root_box"], F)
        lo, hi = box[:3], box[3:]
        ext = F((hi - lo).max())
        c = ((lo + hi) * F(0.5)).astype(F)
        sets = {}
        # a coherent grid over the root box grown by a quarter of its extent, and the same points shuffled
        ax = [np.linspace(lo[q] - F(0.25) * ext, hi[q] + F(0.25) * ext, m, dtype=F) for q, m in enumerate((7, 6, 5))]
        grid = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).astype(F)
        sets["grid"] = grid
        self.perm = rng.permutation(len(grid))
        sets["shuffled"] = grid[self.perm]
        # hit points of closest_hits, moved a few float32 steps along the face normal: they reach the face region
        T = self.tv.reshape(-1, 3, 3)[self.faces]
        cen = ((T[:, 0] + T[:, 1] + T[:, 2]) / F(3)).astype(F)
        pick = rng.integers(0, len(cen), 96)
        o = (c + (rng.random((96, 3), dtype=F) - F(0.5)) * (F(3) * ext)).astype(F)
        d = (cen[pick] - o).astype(F)
        io, idr = In(self.rt, o), In(self.rt, d)
        f, t = self.ctx.closest_hits(io.buf, idr.buf, n=96)
        self.ctx.synchronize()
        f, t = f.to_numpy(np.int32, (96,)), t.to_numpy(F, (96,))
        ok = f >= 0
        assert ok.sum() >= 32, self.name
        hit = (o[ok] + d[ok] * t[ok, None]).astype(F)
        nrm = self.a["face_normal"][f[ok]].astype(F)
        sets["hits"] = np.concatenate([np.where(nrm > 0, step_ulps(hit, k), np.where(nrm < 0, step_ulps(hit, -k), hit)) for k in (2, -3)]).astype(F)
        # every vertex, edge midpoint and centroid of the first faces
        Tf = T[:FIRST_FACES]
        self.first_faces = len(Tf)
        A, B, Cc = Tf[:, 0], Tf[:, 1], Tf[:, 2]
        sets["on_faces"] = np.concatenate([A, B, Cc, (A + B) * F(0.5), (B + Cc) * F(0.5), (A + Cc) * F(0.5), ((A + B) + Cc) / F(3)]).astype(F)
        # 1e4 extents away, and non-finite points
        corners = np.array([[(i >> q) & 1 for q in range(3)] for i in range(8)], F) * F(2) - F(1)
        sets["far"] = (c + corners * (F(1e4) * ext)).astype(F)
        bad = np.tile(c, (11, 1)).astype(F)
        k = 0
        for v in (np.nan, np.inf, -np.inf):
            for q in range(3):
                bad[k, q] = v
                k += 1
        bad[9], bad[10] = np.nan, np.inf
        sets["nonfinite"] = bad
        if self.info["unreachable_faces"]:
            sets["lost"] = unreachable_probe_points(self.a, self.faces)[1].astype(F)
        return sets

    def close(self):
        self.ctx.close()
        self.hs.close()


@pytest.fixture(scope="module")
def world(rt, scenes, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Scene(rt, scenes, tmp_path_factory.mktemp("near"), name)
        return made[name]
    yield get
    for s in made.values():
        s.close()


# ------------------------------------------------------------------------------------------ 1. every scene, every point set, tolerance 0
@pytest.mark.parametrize("name", SCENES)
def test_equals_brute_force_over_the_referenced_faces(world, name):
    sc = world(name)
    got = run(sc, sc.P)
    assert_equal(got, sc.want, name)
    f, d, q = sc.want
    finite = np.isfinite(sc.P).all(axis=1)
    assert (f[finite] >= 0).all() and np.isfinite(d[finite]).all()
    nan = np.isnan(sc.P).any(axis=1)
    assert (f[nan] == -1).all() and np.isinf(d[nan]).all() and same(q[nan], sc.P[nan]), "a NaN point has no candidate and gets itself back"
    on = sc.where["on_faces"]
    assert (d[on][:sc.first_faces] == 0).all(), "vertex A of a face is its own nearest point: d1 = d2 = 0, region A, whatever the triangle"
    # the hit points reach the face region of their nearest face (uniformly random points do in about 0.1 % of pairs)
    hits = sc.where["hits"]
    T = sc.tv.reshape(-1, 3, 3)[f[hits]]
    region = cp.closest(sc.P[hits], T[:, 0], T[:, 1], T[:, 2])[2]
    assert (region == 6).sum() >= len(region) // 2, (name, np.bincount(region, minlength=7).tolist())


def test_the_fixtures_are_what_they_claim(world):
    cube, capped = world("cube"), world("cap34")
    assert cube.info["flat_nodes"] == 1 and len(cube.tv) == 12 and len(cube.faces) == 12
    dodge = world("dodge")
    assert dodge.info["flat_nodes"] == 169 and dodge.info["max_leaf"] == 979
    assert capped.info["unreachable_faces"] > 0 and capped.info["lost_nodes"] > 0 and capped.info["max_leaf"] > qc.CASES["cap34"].cap
    # the rule "referenced faces": some point's nearest face over ALL faces is a lost one, and the query does not return it
    lost = np.setdiff1d(np.arange(len(capped.tv)), capped.faces)
    P = capped.P[capped.where["lost"]]
    f_all, _, _ = cp.brute_force(P, capped.tv, np.arange(len(capped.tv)))
    assert np.isin(f_all, lost).any()
    assert not np.isin(capped.want[0], lost).any()
    for name, faces in (("flat12", 12), ("flat64", 64), ("flat65", 65)):
        sc = world(name)
        assert sc.info["flat_nodes"] == 1 and len(sc.tv) == faces


def test_ties_go_to_the_lowest_face_id(world):
    sc = world("cube")
    T = sc.tv.reshape(-1, 3, 3)
    d2, _, _ = cp.closest(sc.P[:, None], T[None, :, 0], T[None, :, 1], T[None, :, 2])
    least = np.where(np.isnan(d2), F(np.inf), d2).min(axis=1)
    tied = (d2 == least[:, None]).sum(axis=1)
    # (the grid points beyond a corner in all three axes, twice, and the 8 far points at the least: a shared vertex is the same floats)
    assert (tied > 1).sum() >= 40, "the cube's shared vertices tie"
    first = np.argmax(d2 == least[:, None], axis=1)
    ok = tied > 1
    assert np.array_equal(sc.want[0][ok], first[ok])
    got = run(sc, sc.P)
    assert np.array_equal(got[0][ok], first[ok])


# ------------------------------------------------------------------------------------------ 2. radii
def radii_round(d2):
    """the largest float32 r with r * r < d2 and the smallest with r * r >= d2"""
    r = np.sqrt(F(d2))
    while F(r) * F(r) >= F(d2):
        r = np.nextafter(F(r), F(0))
    below = F(r)
    while F(r) * F(r) < F(d2):
        r = np.nextafter(F(r), F(np.inf))
    return below, F(r)


# (the capped tree takes the median alone: each of its 296 faces is referenced some ten thousand times and nearly every leaf's box holds
# nearly every point, so a call walks most of three million references whatever the radius -- two seconds a call)
@pytest.mark.parametrize("name", ("cube", "dodge", "soup8", "cap34", "flat12", "flat64", "flat65", "soup8_2^-20", "soup8_2^20"))
def test_radii(world, name):
    sc = world(name)
    f, d, _ = sc.want
    some = np.flatnonzero((f >= 0) & np.isfinite(d) & (d > 0))
    median = float(np.sqrt(np.median(d[some])))
    i = int(some[len(some) // 3])
    below, above = radii_round(d[i])
    radii = (("zero", 0.0), ("median", median), ("below", float(below)), ("above", float(above)))
    if name == "cap34":
        want = within(sc.want, sc.P, median)
        assert_equal(run(sc, sc.P, median), want, (name, "median", median))
        assert (want[0] == -1).any() and (want[0] >= 0).any()
        return
    for what, r in radii:
        want = within(sc.want, sc.P, r)
        got = run(sc, sc.P, r)
        assert_equal(got, want, (name, what, r))
        assert (want[0] == -1).any() and (want[0] >= 0).any(), (name, what)
    assert within(sc.want, sc.P, float(below))[0][i] == -1 and within(sc.want, sc.P, float(above))[0][i] == f[i]
    assert_equal(run(sc, sc.P, 3e38), sc.want, (name, "r * r overflows to +inf"))


# ------------------------------------------------------------------------------------------ 3. sizes and outputs
@pytest.mark.parametrize("name", ("cube", "dodge"))
def test_prefixes_and_optional_outputs(world, name):
    sc = world(name)
    for kind in ("grid", "shuffled"):              # (257 points from the start of either set: the coherent grid, or the shuffled one and what follows it)
        at = sc.where[kind].start
        for n in PREFIXES:
            assert_equal(run(sc, sc.P[at:at + n]), tuple(w[at:at + n] for w in sc.want), (name, kind, n))
    P, want = sc.P[:65], tuple(w[:65] for w in sc.want)
    for faces, dist2, closest in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        got = run(sc, P, faces=faces, dist2=dist2, closest=closest)
        assert [g is not None for g in got] == [faces, dist2, closest]
        assert_equal(got, want, (name, faces, dist2, closest))
    # n below the buffer's length: the rest stays as it was (the guards of Out begin at n)
    assert_equal(run(sc, sc.P[:200], n=70), tuple(w[:70] for w in sc.want), (name, "n = 70 of 200"))


def test_the_second_grid_stride_round(world):
    sc = world("cube")
    cus = gc.cu_count()
    n = gc.query_rays(cus)
    assert gc.strides(n, gc.query_cap(cus)) and gc.query_grid(n, cus) == gc.BLOCKS_PER_CU * cus
    rng = np.random.default_rng(5)
    P = ((rng.random((n, 3), dtype=F) - F(0.5)) * F(4)).astype(F)
    got = run(sc, P)
    want = cp.brute_force(P, sc.tv, sc.faces)
    assert_equal(got, want, "round two")
    cap = gc.query_cap(cus)
    assert len(np.unique(want[0][cap:])) == 12, "every face is some point's answer behind the first round"


def test_torch_tensors_on_the_current_stream(world):
    import torch
    sc = world("dodge")
    P = torch.from_numpy(np.array(sc.P[:300])).to("cuda:0")
    with torch.cuda.stream(torch.cuda.Stream(0)):
        f, d, q = sc.ctx.closest_points(P, max_dist=INF)
        torch.cuda.current_stream(0).synchronize()
    assert_equal((f.cpu().numpy(), d.cpu().numpy(), q.cpu().numpy()), tuple(w[:300] for w in sc.want), "tensors")
    f, d, q = sc.ctx.closest_points(P, want_dist2=False, want_closest=False)
    assert d is None and q is None and np.array_equal(f.cpu().numpy(), sc.want[0][:300])


# ------------------------------------------------------------------------------------------ 4. refusals
def test_refusals(rt, world):
    sc = world("cube")
    lib, h, capi = sc.lib, sc.ctx.handle, rt.capi
    n = 64
    buf = rt.hipmem.DeviceBuffer(n * 12 * 4)
    p, f, d, q = buf.address, buf.address + n * 12, buf.address + n * 16, buf.address + n * 20
    call = lambda *a: lib.rt_closest_points_device(h, *a, None)                                     # noqa: E731
    assert call(n, p, INF, f, d, q) == capi.RT_OK
    assert call(0, None, INF, None, None, None) == capi.RT_OK and call(0, None, float("nan"), None, None, None) == capi.RT_ERR_INVALID
    assert call(-1, p, INF, f, d, q) == capi.RT_ERR_INVALID
    assert call(n, None, INF, f, d, q) == capi.RT_ERR_INVALID
    assert call(n, p, INF, None, None, None) == capi.RT_ERR_INVALID and b"all null" in lib.rt_last_error(h)
    assert call(n, p, float("nan"), f, d, q) == capi.RT_ERR_INVALID and call(n, p, -1.0, f, d, q) == capi.RT_ERR_INVALID
    assert call(n, p, 0.0, f, None, None) == capi.RT_OK and call(n, p, INF, None, d, None) == capi.RT_OK and call(n, p, INF, None, None, q) == capi.RT_OK
    for bad in ((p + n * 12 - 4, d, q), (f, p, q), (f, d, p + 4)):
        assert call(n, p, INF, *bad) == capi.RT_ERR_INVALID and b"overlaps" in lib.rt_last_error(h), bad
    assert call(n, p, INF, f, f + 4, None) == capi.RT_ERR_INVALID and call(n, p, INF, None, d, d + n * 4 - 4) == capi.RT_ERR_INVALID
    assert lib.rt_closest_points_device(None, n, p, INF, f, d, q, None) == capi.RT_ERR_INVALID
    sc.ctx.synchronize()
    # the host-pointer form refuses the same
    P = np.zeros((n, 3), F)
    out = np.zeros(n, np.int32)
    assert lib.rt_closest_points(h, n, P.ctypes.data, float("nan"), out.ctypes.data, None, None) == capi.RT_ERR_INVALID
    assert lib.rt_closest_points(h, n, P.ctypes.data, INF, None, None, None) == capi.RT_ERR_INVALID
    fresh = rt.Context(0)
    try:
        assert lib.rt_closest_points_device(fresh.handle, n, p, INF, f, d, q, None) == capi.RT_ERR_NO_SCENE
        assert lib.rt_closest_points(fresh.handle, n, P.ctypes.data, INF, out.ctypes.data, None, None) == capi.RT_ERR_NO_SCENE
    finally:
        fresh.close()
        buf.free()


# ------------------------------------------------------------------------------------------ 5. the context
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


def test_calls_leave_the_context_as_it_was(rt, world, fly):
    sc = world("dodge")
    me = type("S", (), {"rt": rt, "ctx": fly.ctx})
    fly.supersample, fly.supersample_threshold = 2, 0.05
    try:
        before, counters_before = frame(fly)
        refined = fly.ctx.supersampling_refined()
        for r in (INF, 0.05):
            assert_equal(run(me, sc.P[:400], r), within(tuple(w[:400] for w in sc.want), sc.P[:400], r), r)
        assert fly.ctx.supersampling_refined() == refined and refined > 0
        after, counters_after = frame(fly)
        assert same(before, after) and counters_before == counters_after and counters_before[0] > 0
    finally:
        fly.supersample, fly.supersample_threshold = 1, -1.0


def test_a_call_on_a_second_stream_beside_a_frame(rt, world, fly):
    sc = world("dodge")
    me = type("S", (), {"rt": rt, "ctx": fly.ctx})
    hip = rt.hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        want_rgb, _ = frame(fly)
        run(me, sc.P[:64])                                   # (the bounds exist: the call below only enqueues)
        cam, L, p = fly.camera, fly._lights(), rt.make_params(64, 40, 4)
        rgb = Out(rt, 64 * 40, 3, np.float32)
        rt.capi.check(fly.ctx.lib, fly.ctx.handle,
                      fly.ctx.lib.rt_render_device(fly.ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.buf.ptr, None, None, None, None), "rt_render_device")
        f, d, q, ip = run(me, sc.P, stream=stream.value, sync=False)
        assert hip.hipStreamSynchronize(stream) == 0
        fly.ctx.synchronize()
        assert_equal((f.read(), d.read(), q.read()), sc.want, "beside a frame")
        ip.check()
        assert same(rgb.read().reshape(40, 64, 3), want_rgb)
    finally:
        hip.hipStreamDestroy(stream)


def test_a_second_upload_rebuilds_the_bounds(rt, world):
    cube, dodge = world("cube"), world("dodge")
    ctx = rt.Context(0)
    me = type("S", (), {"rt": rt, "ctx": ctx})
    try:
        ctx.upload(cube.hs)
        assert_equal(run(me, cube.P), cube.want, "first scene")
        ctx.upload(dodge.hs)
        assert_equal(run(me, dodge.P), dodge.want, "second scene on the live context")
        assert_equal(run(me, dodge.P), run(dodge, dodge.P), "a fresh context")
        ctx.upload(cube.hs)
        assert_equal(run(me, cube.P, 0.3), within(cube.want, cube.P, 0.3), "and back")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 6. the facade
def test_distance_field_and_probe_clearance(rt, world, scenes):
    fs = rt.Flyscene(scene_path=os.path.join(scenes, "cube.obj"))
    fs.initialize(64, 40, True, False)
    me = type("S", (), {"rt": rt, "ctx": fs.ctx})
    try:
        for dims, margin, r in (((5, 4, 3), 0.25, INF), ((3, 1, 2), 0.0, 0.4), ((1, 1, 1), 0.0, INF)):
            pg, dist, faces = fs.distance_field(dims, margin=margin, max_dist=r)
            pos = rt.probe_grid_positions(pg)
            f, d2, _ = run(me, pos, r)
            assert dist.dtype == F and dist.shape == (len(pos),) and same(dist, np.sqrt(d2)) and np.array_equal(faces, f), dims
            ref = rt.probe_grid_over(fs.scene.info()["root_box"], dims, margin)
            assert bytes(pg) == bytes(ref)
        # half an extent-free margin away: the points beside a face lie 0.5 from it, those beside an edge 0.707
        _, dist, faces = fs.distance_field((3, 1, 2), margin=0.5, max_dist=0.6)
        assert (faces == -1).any() and (faces >= 0).any() and np.isinf(dist[faces == -1]).all() and (np.abs(dist[faces >= 0] - 0.5) < 1e-6).all()
        # placement: probes over the box grown by a margin keep clear of the surface; one put on a face by hand does not
        probes = fs.light_probes((3, 3, 3), 2, margin=0.25)
        clear = fs.probe_clearance(probes)
        assert clear.shape == (27,) and (clear > 0).all()
        T = world("cube").tv.reshape(-1, 3, 3)[0]
        on_face = ((T[0] + T[1]) * F(0.5)).astype(F)
        by_hand = (rt.probe_grid(on_face, (1.0, 1.0, 1.0), (1, 1, 1)), None)
        assert fs.probe_clearance(by_hand).tolist() == [0.0]
    finally:
        fs.ctx.close()
        fs.scene.close()
