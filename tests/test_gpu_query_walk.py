"""The query kernels' tree walk on a real MI355X, on the scenes, rays and segments of tests/query_walk_cases.py: k_closest returns the CPU
checker's face and, bit for bit, its t for every ray -- aimed at centroids, vertices, edges and duplicated faces, axis-parallel with both
signs of zero, 1e4 and 1e-4 times too long, starting on a face or 1e4 extents away, coherent bundles and every family interleaved in
every wave -- and k_segments the checker's lightStrikes for every segment, on single leaves of 12, 64 and 65 faces, on leaves of several
64-triangle chunks, on depth-capped trees with over-full leaves and lost nodes and on a soup scaled by 2^-20 .. 2^20; with the culling
switched off the results are the same bits; non-finite rays miss and leave their wave's other rays alone; rt_trace_rays, the frame-side
walk, agrees on the same rays; and the compound queries (occlusion, soft shadows, geometry buffers, gather, probes, visible lookup) equal
their restatements over the checker alone.  The checker is the reference for every ray: the library is never its own reference here.
tests/test_query_walk_cases.py holds the conditions (hit shares, ties, leaf modes) on the checker alone."""
import types

import numpy as np
import pytest

import ao_ref
import gbuffer_ref
import indirect_ref as ir
import probe_ref as pr
import probe_visible_ref as pv
import query_walk_cases as qc
import shadow_ref
import switch_table
import test_gpu_ao as gao
import test_gpu_gbuffer as ggb
import test_gpu_indirect as gin
import test_gpu_probe_visible as gpv
import test_gpu_probes as gpr
import test_gpu_ray_queries as queries
import test_gpu_soft_shadows as gss

pytestmark = pytest.mark.gpu

F = np.float32
LIGHT = ((-1.0, 1.0, 1.0),)
WHITE = (1.0, 1.0, 1.0)
CW, CH, POINTS = 32, 24, 256          # the camera of the compound queries and the most points they take


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


class Scene:
    """a case on the GPU and in the CPU checker"""

    def __init__(self, rt, oracle, dirpath, name):
        self.rt, self.orc, self.name, self.case = rt, oracle, name, qc.CASES[name]
        self.path = qc.scene_path(dirpath, name)
        self.hs = qc.host_scene(rt, dirpath, name)
        self.ctx = rt.Context(0)
        self.ctx.upload(self.hs)
        self.lib = self.ctx.lib
        self.osc = qc.oracle_scene(oracle, dirpath, name)
        self.arrays = self.osc.arrays()

    def close(self):
        self.ctx.close()
        self.hs.close()
        self.osc.close()


class Walk(Scene):
    """... with its rays in both orders, its segments, and the checker's answer to each, computed once"""

    def __init__(self, rt, oracle, dirpath, name):
        super().__init__(rt, oracle, dirpath, name)
        self.o, self.d, self.where = qc.sorted_rays(qc.rays(self.arrays, self.case.seed))
        self.idx = qc.interleave(len(self.o))
        self.want_f, self.want_t = qc.reference_hits(self.osc, self.o, self.d)
        self.hit, self.light, self.seg_where, _ = qc.segments(self.arrays, self.case.seed)
        self.seg_idx = qc.interleave(len(self.hit))
        self.want_vis = qc.reference_strikes(self.osc, self.hit, self.light)
        for a in (self.o, self.d, self.want_f, self.want_t, self.hit, self.light, self.want_vis):
            a.setflags(write=False)
        self.got = {}


@pytest.fixture(scope="module", params=list(qc.CASES))
def walk(request, rt, oracle, tmp_path_factory):
    w = Walk(rt, oracle, tmp_path_factory.mktemp("walk"), request.param)
    yield w
    w.close()


def closest(rt, ctx, o, d):
    """k_closest on guarded device buffers -> (face, t)"""
    return queries.closest(types.SimpleNamespace(rt=rt, ctx=ctx), len(o), rays=(o, d))


def strikes(rt, ctx, hit, light):
    """k_segments on guarded device buffers -> visible, uint8"""
    n = len(hit)
    h, l = queries.In(rt, hit), queries.In(rt, light)
    v = queries.Out(rt, n, 1, np.uint8)
    ctx.light_strikes_device(h.buf, l.buf, n=n, vis=v.buf)
    ctx.synchronize()
    h.check(); l.check()
    return v.read()


def family_of(w, i):
    return next(k for k, s in w.where.items() if s.start <= i < s.stop)


def seg_family_of(w, i):
    return next(k for k, s in w.seg_where.items() if s.start <= i < s.stop)


def assert_hits(w, f, t, want_f, want_t, order):
    """face ids equal, t the same bits wherever there is a hit, -1 / -1.0f for a miss"""
    bad = np.flatnonzero(f != want_f)
    src = bad if order == "sorted" else w.idx[bad]
    assert len(bad) == 0, (w.name, order, [(int(i), family_of(w, int(s)), int(f[i]), int(want_f[i])) for i, s in zip(bad[:8], src[:8])])
    hit = want_f >= 0
    bad = np.flatnonzero(hit & (queries.bits(t) != queries.bits(want_t)))
    src = bad if order == "sorted" else w.idx[bad]
    assert len(bad) == 0, (w.name, order, [(int(i), family_of(w, int(s)), float(t[i]), float(want_t[i])) for i, s in zip(bad[:8], src[:8])])
    assert queries.same(t[~hit], np.full(int((~hit).sum()), -1.0, F)), (w.name, order)


# ------------------------------------------------------------------------------------------ 1. k_closest against the checker, both orders
def test_closest_hits_equal_the_checker(walk):
    w = walk
    f, t = closest(w.rt, w.ctx, w.o, w.d)
    w.got["closest"] = (f, t)
    assert_hits(w, f, t, w.want_f, w.want_t, "sorted")
    fi, ti = closest(w.rt, w.ctx, w.o[w.idx], w.d[w.idx])
    assert_hits(w, fi, ti, w.want_f[w.idx], w.want_t[w.idx], "interleaved")
    assert np.array_equal(fi, f[w.idx]) and queries.same(ti, t[w.idx]), "the interleaved result is the permuted sorted one, bit for bit"


# ------------------------------------------------------------------------------------------ 2. k_segments against the checker
def test_light_strikes_equal_the_checker(walk):
    w = walk
    vis = strikes(w.rt, w.ctx, w.hit, w.light)
    w.got["strikes"] = vis
    bad = np.flatnonzero(vis != w.want_vis)
    assert len(bad) == 0, (w.name, "sorted", [(int(i), seg_family_of(w, int(i)), int(vis[i])) for i in bad[:8]])
    assert (vis[w.seg_where["same"]] == 1).all() and (vis[w.seg_where["outside"]] == 1).all()
    # interleaved: the segments that never meet the root box thin out every wave (lanes = triangles also in a single leaf of 65 faces)
    vi = strikes(w.rt, w.ctx, w.hit[w.seg_idx], w.light[w.seg_idx])
    bad = np.flatnonzero(vi != w.want_vis[w.seg_idx])
    assert len(bad) == 0, (w.name, "interleaved", [(int(i), seg_family_of(w, int(w.seg_idx[i])), int(vi[i])) for i in bad[:8]])


# ------------------------------------------------------------------------------------------ 3. the culling may only skip work
def test_culling_off_gives_the_same_bits(walk, monkeypatch):
    w = walk
    monkeypatch.setenv("RT_NO_CULL", "1")
    plain = w.rt.Context(0)
    try:
        plain.upload(w.hs)
        monkeypatch.delenv("RT_NO_CULL")
        for order, pick in (("sorted", slice(None)), ("interleaved", w.idx)):
            f, t = closest(w.rt, plain, w.o[pick], w.d[pick])
            cf, ct = w.got["closest"] if "closest" in w.got else closest(w.rt, w.ctx, w.o, w.d)
            assert np.array_equal(f, cf[pick]) and queries.same(t, ct[pick]), (w.name, order, np.flatnonzero(f != cf[pick])[:8])
        cv = w.got["strikes"] if "strikes" in w.got else strikes(w.rt, w.ctx, w.hit, w.light)
        for order, pick in (("sorted", slice(None)), ("interleaved", w.seg_idx)):
            vis = strikes(w.rt, plain, w.hit[pick], w.light[pick])
            assert np.array_equal(vis, cv[pick]), (w.name, order, np.flatnonzero(vis != cv[pick])[:8])
        # ... and the un-culled walk is the checker's too
        assert np.array_equal(f, w.want_f[w.idx]) and np.array_equal(vis, w.want_vis[w.seg_idx])
    finally:
        plain.close()


# ------------------------------------------------------------------------------------------ 4. non-finite rays
@pytest.mark.parametrize("name", qc.NONFINITE_CASES)
def test_non_finite_rays_miss_and_leave_their_wave_alone(rt, oracle, tmp_path, name):
    sc = Scene(rt, oracle, tmp_path, name)
    try:
        o, d, finite = qc.nonfinite_rays(sc.arrays, sc.case.seed)
        want_f, want_t = qc.reference_hits(sc.osc, o, d)
        assert (want_f[~finite] == -1).all() and (want_f[finite] >= 0).any()
        f, t = closest(rt, sc.ctx, o, d)
        miss = want_f < 0
        assert (f[miss] == -1).all() and queries.same(t[miss], np.full(int(miss.sum()), -1.0, F)), (name, f[~finite], t[~finite])
        assert np.array_equal(f, want_f) and queries.same(t[~miss], want_t[~miss])
        # the finite rays alone, in a wave without the others: unchanged
        ff, tf = closest(rt, sc.ctx, o[finite], d[finite])
        assert np.array_equal(ff, f[finite]) and queries.same(tf, t[finite])
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------ 5. the frame-side walk on the same rays
@pytest.mark.parametrize("name", qc.COMPOUND_CASES)
def test_trace_rays_agrees_on_the_same_rays(rt, oracle, tmp_path, name):
    """rt_trace_rays at depth 0 (Flyscene.traceRay): the listed-ray launch sequence of the frames, a second path through the tree"""
    sc = Scene(rt, oracle, tmp_path, name)
    try:
        o, d, _ = qc.sorted_rays(qc.rays(sc.arrays, sc.case.seed))
        f, t = closest(rt, sc.ctx, o, d)
        fs = rt.Flyscene(scene_path=sc.path)
        fs.ctx, fs.scene, fs.max_depth = sc.ctx, sc.hs, 0
        fs.traceRay(o, d)
        assert np.array_equal(fs.last_face, f), (name, np.flatnonzero(fs.last_face != f)[:8])
        assert queries.same(fs.last_t, t), (name, np.flatnonzero(queries.bits(fs.last_t) != queries.bits(t))[:8])
        assert 0 < int((f >= 0).sum()) < len(f)
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------ 6. the compound queries over the checker alone
class Compound(Scene):
    """... with at most 256 hit points of the 32 x 24 camera at yaw 0.4 (ao_ref.camera_points) and the 2 x 2 x 2 probe grid over the scene box"""

    def __init__(self, rt, oracle, dirpath, name):
        super().__init__(rt, oracle, dirpath, name)
        _, (P, N) = ao_ref.camera_points(oracle, self.osc, CW, CH, 0.4)
        assert len(P) >= 64, "the camera must see the scene"
        pick = np.unique(np.linspace(0, len(P) - 1, min(POINTS, len(P))).astype(int))
        self.P, self.N = np.ascontiguousarray(P[pick], F), np.ascontiguousarray(N[pick], F)
        self.n = len(self.P)
        self.data = ir.SceneData(self.osc)
        self.tracer = ir.OracleTracer(self.osc)
        w = np.asarray(self.arrays["wverts"], F)
        lo, hi = w.min(axis=0), w.max(axis=0)
        self.grid = pr.Grid.over(np.concatenate([lo, hi]), (2, 2, 2))
        # from the corners of the box every probe ray misses (the coefficients are the direct term or zero): a second grid inside it
        q = F(0.25) * (hi - lo)
        self.inner = pr.Grid.over(np.concatenate([lo + q, hi - q]).astype(F), (2, 2, 2))


@pytest.fixture(scope="module", params=list(qc.COMPOUND_CASES))
def compound(request, rt, oracle, tmp_path_factory):
    c = Compound(rt, oracle, tmp_path_factory.mktemp("compound"), request.param)
    yield c
    c.close()


@pytest.mark.parametrize("m", [2, 3])
def test_ambient_occlusion_equals_the_checker(compound, m):
    sc = compound
    want = ao_ref.counts(sc.osc, sc.P, sc.N, gao.SEED, m, gao.RADIUS)
    got_open, got_ao = gao.run_ao(sc, sc.P, sc.N, m)
    assert np.array_equal(got_open, want), (sc.name, m, np.flatnonzero(got_open != want)[:8])
    assert gao.same(got_ao, ao_ref.ao_of(want, m))
    assert ((want > 0) & (want < m * m)).any(), "the points must hold partly occluded ones"


@pytest.mark.parametrize("params", ["centre", "seed7"])
def test_soft_shadows_equal_the_checker(compound, params):
    sc = compound
    L = sc.rt.make_lights(points=gss.THREE[:1], area=True, usteps=3, vsteps=3)
    sp = gss.make_params(sc.rt, sc.lib, params)
    want = shadow_ref.oracle_counts(sc.osc, shadow_ref.Lights(L), sc.P, sc.N, bool(sp.per_point), sp.seed, (F(sp.fu), F(sp.fv)))
    vis, share = gss.run(sc, L, sp, sc.P, sc.N)
    assert np.array_equal(vis, want), (sc.name, params, np.flatnonzero(vis != want)[:8])
    assert gss.same(share, shadow_ref.share_of(want, 9))
    assert 0 < int(want.astype(np.int64).sum()) < 9 * sc.n, "lit and shadowed"


@pytest.mark.parametrize("n", [1, 2])
def test_gbuffer_equals_the_checker(compound, n):
    sc = compound
    ggb.gp.set_frame(sc.ctx, n)
    try:
        got = ggb.gbuffer(sc, CW, CH)
    finally:
        ggb.gp.set_frame(sc.ctx, 1)
    want = gbuffer_ref.cpu_frame(sc.orc, sc.osc, sc.orc.camera(CW, CH, ggb.YAW), CW, CH, n)
    assert ggb.same(got, want), (sc.name, n, ggb.differing(got, want))
    full, empty, _ = gbuffer_ref.coverage(got)
    assert full > 0 and empty > 0


def test_indirect_diffuse_equals_the_checker(compound):
    sc = compound
    want = ir.gather(sc.tracer, sc.data, sc.P, sc.N, 2, gin.SEED, LIGHT, WHITE)
    got = gin.run(sc, sc.P, sc.N, 2, pos=LIGHT, color=WHITE)
    assert gin.same(got, want), (sc.name, gin.differing(got, want))
    assert (want != 0).any(), "some point must receive indirect light"


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("which", ["box", "inner"])
def test_light_probes_equal_the_checker(compound, which, direct):
    sc = compound
    P = (sc.grid if which == "box" else sc.inner).positions()
    assert len(P) == 8
    tr = pr.trace(sc.tracer, sc.data, P, 2, LIGHT)
    want = pr.shade(tr, WHITE, direct)
    got = gpr.run(sc, P, 2, pos=LIGHT, color=WHITE, direct=direct)
    assert gpr.same(got, want), (sc.name, which, direct, gpr.differing(got, want))
    if which == "inner":
        assert tr.hit.sum() >= 8 and tr.vis.any() and (pr.shade(tr, WHITE, False) != 0).any(), "probe rays must hit lit faces"
    else:
        assert tr.seen.any() and not tr.seen.all(), "the light is seen from some corners of the box"


def test_visible_probe_lookup_equals_the_checker(compound):
    sc = compound
    coeff = np.random.default_rng(41).standard_normal((8, 27)).astype(F)
    want_rgb, want_mask = pv.lookup(sc.tracer, sc.grid, coeff, sc.P, sc.N)
    got_rgb, got_mask = gpv.run(sc, sc.grid, coeff, sc.P, sc.N)
    assert gpv.same(got_mask, want_mask), (sc.name, gpv.differing(got_mask, want_mask))
    assert gpv.same(got_rgb, want_rgb), (sc.name, gpv.differing(got_rgb, want_rgb))
    assert len(set(int(x) for x in want_mask)) >= 2, "the points must differ in the probes they see"
