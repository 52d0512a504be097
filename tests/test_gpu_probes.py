"""The light probes on a real MI355X: rt_light_probes_device returns, per probe, bit for bit what tests/probe_ref.py gets from the definition
-- over the CPU checker's closest hit and lightStrikes, and over rt_closest_hits / rt_light_strikes where the checker takes too long -- in
every wave layout, for every batch length around the layout boundaries, with and without the direct term, in the order of the definition's
sum; rt_probe_irradiance_device returns the definition's lookup; both write nothing behind their outputs, refuse what the header says they
refuse and leave the context as it was."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ao_ref
import grid_caps as gc
import indirect_ref as ir
import probe_ref as pr
import scenes_gen
import switch_table
from test_gpu_ao import GUARD, In, Out, same  # noqa: F401 -- the guarded device arrays of the occlusion tests

pytestmark = pytest.mark.gpu

F = np.float32
GRIDS = (1, 2, 3, 4, 8, 10, 16)
FILES = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj", "toy": "toy.obj"}
ONE = ((-1.0, 1.0, 1.0),)
TWO = ((-1.0, 1.0, 1.0), (1.5, 0.5, -1.0))
YELLOW, WHITE = (1.0, 1.0, 0.0), (1.0, 1.0, 1.0)
DIMS, MARGIN = (6, 5, 5), 0.3                   # 150 probes: more than 2 * 64 + 1, inside and outside the mesh
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


def differing(got, want):
    return np.flatnonzero((np.ascontiguousarray(got, F).view(np.uint32) != np.ascontiguousarray(want, F).view(np.uint32)).any(axis=1))[:8]


class Scene:
    """a scene on the GPU and in the CPU checker, its fixed probe set (a DIMS grid over the bounding box of its vertices grown by MARGIN) and
    the colour-free part of the reference (probe_ref.Traced) of that set, computed once per (m, lights, tracer)"""

    def __init__(self, rt, oracle, path):
        self.rt, self.orc = rt, oracle
        self.fs = rt.Flyscene(scene_path=path)
        self.fs.initialize(64, 40, True, False)
        self.ctx, self.lib = self.fs.ctx, self.fs.ctx.lib
        self.osc = oracle.load_scene(path)
        self.data = ir.SceneData(self.osc)
        self.tracers = {"oracle": ir.OracleTracer(self.osc), "library": ir.LibraryTracer(rt, self.ctx)}
        w = np.asarray(self.osc.arrays()["wverts"], F)
        self.grid = pr.Grid.over(np.concatenate([w.min(axis=0), w.max(axis=0)]), DIMS, MARGIN)
        self.P = self.grid.positions()
        self.n = len(self.P)
        self.ref = {}

    def traced(self, m, pos=ONE, by=None):
        by = by or ("oracle" if self.n * m * m <= ORACLE_RAYS else "library")
        key = (m, pos, by)
        if key not in self.ref:
            self.ref[key] = pr.trace(self.tracers[by], self.data, self.P, m, pos)
        return self.ref[key]

    def want(self, m, pos=ONE, color=WHITE, direct=False, by=None):
        return pr.shade(self.traced(m, pos, by), color, direct)

    def close(self):
        self.ctx.close()
        self.fs.scene.close()
        self.osc.close()


@pytest.fixture(scope="module")
def world(rt, oracle, scenes, tmp_path_factory):
    paths = {k: os.path.join(scenes, v) for k, v in FILES.items()}
    paths["mixed"] = scenes_gen.mixed_materials(str(tmp_path_factory.mktemp("mixed")))
    paths["binades"] = ir.binade_ceiling(str(tmp_path_factory.mktemp("binades")))
    w = {k: Scene(rt, oracle, p) for k, p in paths.items()}
    yield w
    for s in w.values():
        s.close()


def run(sc, P, m, pos=ONE, color=WHITE, direct=False, stream=None, sync=True):
    """rt_light_probes_device on DeviceBuffers with guards -> coefficients (n, 27) as read back"""
    n = len(P)
    p = In(sc.rt, P.reshape(-1, 3) if n else np.zeros((1, 3), F))
    o = Out(sc.rt, n, 27, np.float32)
    got = sc.ctx.light_probes(p.buf, lights_of(sc.rt, pos, color), m, direct=direct, n=n, out=o.buf, stream=stream)
    assert got is o.buf
    if not sync:
        return o, p
    sc.ctx.synchronize()
    p.check()
    return o.read().reshape(n, 27)


# ------------------------------------------------------------------------------------------ 1. every layout on every scene
@pytest.mark.parametrize("name", ["mixed", "toy", "dodge", "cube"])
def test_probes_equal_the_reference_in_every_layout(world, name):
    sc = world[name]
    assert sc.n == 150
    for m in GRIDS:
        for color, direct in ((YELLOW, False), (WHITE, True)):
            want = sc.want(m, color=color, direct=direct)
            got = run(sc, sc.P, m, color=color, direct=direct)
            assert got.dtype == np.float32 and same(got, want), (name, m, color, direct, differing(got, want))
            if color == YELLOW:
                assert zero_bits(got.reshape(-1, 9, 3)[:, :, 2]), "no blue light: the blue channel is +0.0f"
    nonzero = int((sc.want(3) != 0).any(axis=1).sum())
    print(name, "probes with non-zero coefficients at m = 3:", nonzero, "of", sc.n)
    assert nonzero >= 1, "on the convex cube too: a probe outside it sees its lit faces, unlike the gather of a point on it"
    seen = sc.traced(3).seen[:, 0]
    assert seen.any(), "the fixture must hold probes that see the light"
    if name != "cube":
        assert nonzero >= 15


def test_library_reference_equals_the_oracle_reference(world):
    """the two references of this file agree where both are affordable (so either may stand for the definition)"""
    for name, m, pos in (("mixed", 3, ONE), ("mixed", 4, TWO), ("dodge", 3, ONE), ("toy", 2, TWO), ("cube", 8, TWO)):
        sc = world[name]
        a, b = sc.traced(m, pos, "oracle"), sc.traced(m, pos, "library")
        assert np.array_equal(a.hit, b.hit) and np.array_equal(a.vis, b.vis) and same(a.ct, b.ct) and same(a.kd, b.kd), (name, m)
        assert np.array_equal(a.seen, b.seen)
        assert same(pr.shade(a, WHITE, True), pr.shade(b, WHITE, True))


# ------------------------------------------------------------------------------------------ 2. two lights, partly hidden
def test_two_lights_partly_hidden_from_hits_and_from_probes(world):
    sc = world["mixed"]
    tr = sc.traced(3, TWO, "oracle")
    per_hit = tr.vis.sum(axis=1)
    one, both = int((per_hit == 1).sum()), int((per_hit == 2).sum())
    per_probe = tr.seen.sum(axis=1)
    print("probe-ray hits that see one / both lights:", one, both, " probes that see 0 / 1 / 2 lights:", [int((per_probe == k).sum()) for k in range(3)])
    assert one >= 20 and both >= 20, "a light hidden from some hits"
    assert (per_probe == 1).any() and (per_probe == 2).any(), "a probe from which a light is hidden"
    for direct in (False, True):
        want = pr.shade(tr, WHITE, direct)
        got = run(sc, sc.P, 3, pos=TWO, direct=direct)
        assert same(got, want), (direct, differing(got, want))
    assert not same(sc.want(3, TWO), sc.want(3)), "the second light shows"
    assert not same(sc.want(3, TWO, direct=True), sc.want(3, TWO)), "the direct term shows"
    # direct is a switch: any non-zero value turns it on
    p, o = In(sc.rt, sc.P), Out(sc.rt, sc.n, 27, np.float32)
    L = lights_of(sc.rt, TWO, WHITE)
    sc.rt.capi.check(sc.lib, sc.ctx.handle, sc.lib.rt_light_probes_device(sc.ctx.handle, C.byref(L), sc.n, p.buf.ptr, 3, -5, o.buf.ptr, None), "rt_light_probes_device")
    sc.ctx.synchronize()
    assert same(o.read().reshape(sc.n, 27), sc.want(3, TWO, direct=True))


# ------------------------------------------------------------------------------------------ 3. batch lengths around the layout boundaries
@pytest.mark.parametrize("m", GRIDS)
def test_batch_lengths_and_guards(world, m):
    sc = world["mixed"]
    g = group(m)
    assert (m, g, m * m // math.gcd(m * m, 64)) in {(1, 64, 1), (2, 16, 1), (3, 64, 9), (4, 4, 1), (8, 1, 1), (10, 16, 25), (16, 1, 4)}
    want = sc.want(m, direct=True)
    for n in sorted({0, 1, max(g - 1, 0), g, g + 1, 2 * g + 1}):
        # (a probe's answer depends on its position alone: a prefix of the batch is the batch of the prefix)
        got = run(sc, sc.P[:n], m, direct=True)
        assert got.shape == (n, 27) and same(got, want[:n]), (m, n, differing(got, want[:n]))


# ------------------------------------------------------------------------------------------ 4. the order of the sum
@pytest.mark.parametrize("m", [8, 10, 16])
def test_the_sum_runs_in_the_order_of_the_definition(world, m):
    """probes between a lit floor and the ceiling of strips whose kd differ by 6 binades each: the sum from K - 1 down to 0 differs from the
    definition's in bits, and the device gives the definition's.  m = 8: a unit is one probe in one round; m = 10: 16 probes in 25 rounds,
    straddling them; m = 16: one probe in four rounds."""
    from test_probes_api import binade_probes
    sc = world["binades"]
    P, pos = binade_probes(ir.to_world(sc.osc, ir.BINADE_VERTS))
    tr = pr.trace(sc.tracers["oracle" if len(P) * m * m <= ORACLE_RAYS else "library"], sc.data, P, m, pos)
    assert len(set(tr.kd[:, 0].tolist())) >= 6
    fwd, rev = pr.shade(tr, WHITE), pr.shade(tr, WHITE, reverse=True)
    assert len(differing(fwd, rev)) >= 3, "the order must show in this fixture"
    got = run(sc, P, m, pos=pos)
    assert same(got, fwd), differing(got, fwd)


# ------------------------------------------------------------------------------------------ 5. more units than the grid holds
def stride_shape(sc, m):
    """about 1.25 caps of wave units, three probes more than whole units (one probe more where a unit is one probe) -> n, asserted to stride
    as test_gpu_indirect.py's stride_shape does"""
    K = m * m
    rounds = K // math.gcd(K, 64)
    cus = gc.cu_count(sc.ctx.device)
    units = gc.round_two(gc.ao_cap(cus, rounds)) + 5
    n = (units - 1) * group(m) + min(3, group(m))
    assert -(-n // group(m)) == units
    assert units > gc.ao_cap(cus, rounds) and gc.ao_grid(units, cus, rounds) * gc.WAVES < units, (cus, units, "the batch does not reach the grid of this device")
    assert gc.strides(units, gc.ao_cap(cus, rounds))
    return n


@pytest.mark.parametrize("m", [1, 16])
def test_grid_stride(world, m):
    """m = 1: 64 probes of one ray each per unit, one round; m = 16: one probe per unit in four rounds.  A probe's answer depends on its
    position alone, so a tiled probe set has a tiled answer."""
    sc = world["toy"]
    n = stride_shape(sc, m)
    base = sc.want(m, direct=True)
    assert int((base != 0).any(axis=1).sum()) >= 5
    reps = -(-n // sc.n)
    P = np.tile(sc.P, (reps, 1))[:n]
    got = run(sc, P, m, direct=True)
    want = np.tile(base, (reps, 1))[:n]
    assert same(got, want), differing(got, want)


# ------------------------------------------------------------------------------------------ 6. probes that meet everything at once, or nothing
def test_a_probe_inside_a_solid_and_one_far_outside(world):
    """every ray of the probe at the cube's centre hits at once, and every hit faces away from the light or is hidden from it; no ray of
    the far probe hits: 27 positive zeros, or -- with direct -- the direct terms of the lights lightStrikes calls visible, alone"""
    sc = world["cube"]
    w = np.asarray(sc.osc.arrays()["wverts"], F)
    centre = ((w.min(axis=0) + w.max(axis=0)) * F(0.5)).astype(F)
    P = np.stack([centre, np.array([50.0, 40.0, 30.0], F)])
    for m in (1, 2, 3, 8):
        tr = pr.trace(sc.tracers["oracle"], sc.data, P, m, ONE)
        assert tr.hit[0].all() and not tr.hit[1].any(), "every ray of the inner probe hits, none of the outer"
        assert tr.seen[1, 0], "nothing lies between the far probe and the light"
        got = run(sc, P, m)
        assert got.shape == (2, 27) and zero_bits(got), m
        got = run(sc, P, m, direct=True)
        assert same(got, pr.shade(tr, WHITE, True))
        only = pr.add_direct(np.zeros((2, 9, 3), F), P, ONE, WHITE, tr.seen).reshape(2, 27)
        assert same(got, only) and (got[1] != 0).any(), "the direct term alone"


# ------------------------------------------------------------------------------------------ 7. the lookup
def lookup_run(sc, grid, Cf, P, N, stream=None):
    rt = sc.rt
    n = len(P)
    c, p, nr = In(rt, Cf), In(rt, P if n else np.zeros((1, 3), F)), In(rt, N if n else np.zeros((1, 3), F))
    o = Out(rt, n, 3, np.float32)
    g = rt.probe_grid(grid.origin, grid.step, grid.dims)
    got = sc.ctx.probe_irradiance(g, c.buf, p.buf, nr.buf, n=n, out=o.buf, stream=stream)
    assert got is o.buf
    sc.ctx.synchronize()
    c.check(); p.check(); nr.check()
    return o.read().reshape(n, 3)


def lookup_points(grid, n, rng):
    """points inside and outside the grid, some exactly on probes, normals of every kind"""
    lo = grid.origin.astype(np.float64)
    hi = lo + grid.step.astype(np.float64) * (np.array(grid.dims) - 1)
    span = np.maximum(hi - lo, 1.0)
    P = (lo - 0.5 * span + rng.random((n, 3)) * 2.0 * span).astype(F)
    N = rng.standard_normal((n, 3)).astype(F)
    pos = grid.positions()
    k = min(n, len(pos))
    P[:k] = pos[:k]                                            # exactly on probes
    if n > 40:
        N[20:24] = 0.0
        N[22, 1] = -0.0                                        # no point, either sign of zero
        P[24] = np.nan
        P[25] = (np.inf, -np.inf, 0.0)
        N[26] = (0.0, 0.0, 1.0)
    return P, N


@pytest.mark.parametrize("dims", [(3, 2, 4), (2, 3, 1), (1, 4, 1), (1, 1, 1)])
def test_lookup_equals_the_reference(world, dims):
    sc = world["cube"]
    rng = np.random.default_rng(sum(dims))
    grid = pr.Grid((-0.7, 0.1, 0.3), (0.4, 0.25, 0.11), dims)
    Cf = rng.standard_normal((grid.cells, 27)).astype(F)
    for n in (0, 1, 255, 256, 257, 1000):
        P, N = lookup_points(grid, n, rng)
        want = pr.lookup(grid, Cf, P, N)
        got = lookup_run(sc, grid, Cf, P, N)
        assert got.shape == (n, 3) and same(got, want), (dims, n, differing(got, want))
        if n == 1000:
            assert zero_bits(got[20:24]) and (got[:20] != 0).all()


def test_lookup_grid_stride(world):
    sc = world["cube"]
    cus = gc.cu_count(sc.ctx.device)
    n = gc.query_rays(cus)
    assert gc.strides(n, gc.query_cap(cus)) and gc.query_grid(n, cus) * gc.QUERY_BLOCK < n
    rng = np.random.default_rng(5)
    grid = pr.Grid((-1.0, -1.0, -1.0), (0.5, 0.4, 0.7), (5, 6, 4))
    Cf = rng.standard_normal((grid.cells, 27)).astype(F)
    P, N = lookup_points(grid, n, rng)
    want = pr.lookup(grid, Cf, P, N)
    got = lookup_run(sc, grid, Cf, P, N)
    assert same(got, want), differing(got, want)


def test_lookup_needs_no_scene(rt):
    ctx = rt.Context(0)
    try:
        class Bare:
            pass
        sc = Bare()
        sc.rt, sc.ctx = rt, ctx
        rng = np.random.default_rng(9)
        grid = pr.Grid((0, 0, 0), (1, 1, 1), (2, 2, 2))
        Cf = rng.standard_normal((8, 27)).astype(F)
        P, N = lookup_points(grid, 100, rng)
        assert same(lookup_run(sc, grid, Cf, P, N), pr.lookup(grid, Cf, P, N))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 8. refusals
def test_no_scene_and_bad_arguments(rt, world):
    sc = world["mixed"]
    lib, inv, uns = sc.lib, rt.capi.RT_ERR_INVALID, rt.capi.RT_ERR_UNSUPPORTED
    p = In(rt, sc.P)
    o = Out(rt, sc.n, 27, np.float32)
    fp = lambda x: x.ctypes.data_as(C.c_void_p)
    ho = np.zeros((sc.n, 27), F)
    good = lights_of(rt, ONE, WHITE)

    def calls(h, n, m=3, L=good):
        Lp = C.byref(L) if L is not None else None
        return [lib.rt_light_probes_device(h, Lp, n, p.buf.ptr, m, 1, o.buf.ptr, None), lib.rt_light_probes(h, Lp, n, fp(sc.P), m, 1, fp(ho))]

    empty = rt.Context(0)
    try:
        for n in (sc.n, 0):
            assert calls(empty.handle, n) == [rt.capi.RT_ERR_NO_SCENE] * 2
        assert b"before rt_upload_scene" in lib.rt_last_error(empty.handle)
    finally:
        empty.close()
    h = sc.ctx.handle
    assert calls(h, 0) == [0, 0]
    assert calls(h, -1) == [inv, inv]
    for m in (0, 17, -3):
        assert calls(h, sc.n, m=m) == [inv, inv], m
        assert calls(h, 0, m=m) == [inv, inv], m
        assert b"the grid size m must be in 1 .. 16" in lib.rt_last_error(h)
    assert calls(h, sc.n, L=None) == [inv, inv] and calls(h, 0, L=None) == [inv, inv]
    for nl in (0, 26, -1):
        bad = lights_of(rt, ONE, WHITE)
        bad.n_lights = nl
        assert calls(h, sc.n, L=bad) == [inv, inv], nl
    bad = lights_of(rt, ONE, WHITE)
    bad.mode = 7
    assert calls(h, sc.n, L=bad) == [inv, inv]
    sphere = rt.make_lights(ONE, area=True)
    keep = rt.set_sphere(sphere, rt.sphere_offsets(3, 1.0, 25))                     # noqa: F841 -- keeps the offsets alive
    assert calls(h, sc.n, L=sphere) == [uns, uns]
    assert b"sphere lights are not supported" in lib.rt_last_error(h)
    # NULL pointers, aliasing: an output that shares a byte with the input
    args = lambda pp, po: lib.rt_light_probes_device(h, C.byref(good), sc.n, pp, 3, 0, po, None)
    assert args(None, o.buf.ptr) == inv and args(p.buf.ptr, None) == inv
    assert args(p.buf.ptr, p.buf.ptr) == inv
    assert args(p.buf.ptr, C.c_void_p(p.buf.address + sc.n * 12 - 2)) == inv
    assert args(C.c_void_p(o.buf.address + sc.n * 108 - 4), o.buf.ptr) == inv
    assert b"the output overlaps the input" in lib.rt_last_error(h)
    assert lib.rt_light_probes(h, C.byref(good), sc.n, fp(sc.P), 3, 0, None) == inv
    sc.ctx.synchronize()
    assert o.untouched()
    p.check()
    assert not ho.any()
    # an area light is taken by its positions: the grid is not looked at
    area = rt.make_lights(ONE, area=True, usteps=5, vsteps=5)
    for k in range(3):
        area.color[k] = 1.0
    assert lib.rt_light_probes(h, C.byref(area), sc.n, fp(sc.P), 3, 1, fp(ho)) == 0
    assert same(ho, sc.want(3, direct=True))


def test_lookup_refusals(rt, world):
    sc = world["mixed"]
    lib, inv, h = sc.lib, rt.capi.RT_ERR_INVALID, sc.ctx.handle
    n = 64
    grid = pr.Grid((0, 0, 0), (1, 1, 1), (2, 2, 2))
    rng = np.random.default_rng(2)
    Cf = rng.standard_normal((8, 27)).astype(F)
    P, N = lookup_points(grid, n, rng)
    c, p, nr = In(rt, Cf), In(rt, P), In(rt, N)
    o = Out(rt, n, 3, np.float32)
    ho = np.zeros((n, 3), F)
    fp = lambda x: x.ctypes.data_as(C.c_void_p)
    G = lambda step=(1, 1, 1), dims=(2, 2, 2): rt.probe_grid((0, 0, 0), step, dims)

    def calls(g, nn=n):
        gp = C.byref(g) if g is not None else None
        return [lib.rt_probe_irradiance_device(h, gp, c.buf.ptr, nn, p.buf.ptr, nr.buf.ptr, o.buf.ptr, None),
                lib.rt_probe_irradiance(h, gp, fp(Cf), nn, fp(P), fp(N), fp(ho))]

    assert calls(G(), 0) == [0, 0] and calls(G(), -1) == [inv, inv] and calls(None) == [inv, inv] and calls(None, 0) == [inv, inv]
    for g in (G(dims=(0, 2, 2)), G(dims=(2, -1, 2)), G(dims=(4096, 4096, 2)), G(step=(0, 1, 1)), G(step=(1, -1, 1)), G(step=(1, 1, float("inf"))),
              G(step=(float("nan"), 1, 1))):
        assert calls(g) == [inv, inv] and calls(g, 0) == [inv, inv], (list(g.step), list(g.dims))
    assert b"rt_probe_irradiance: " in lib.rt_last_error(h)
    g = G()
    dev = lambda pc, pp, pn, po: lib.rt_probe_irradiance_device(h, C.byref(g), pc, n, pp, pn, po, None)
    assert dev(None, p.buf.ptr, nr.buf.ptr, o.buf.ptr) == inv and dev(c.buf.ptr, None, nr.buf.ptr, o.buf.ptr) == inv
    assert dev(c.buf.ptr, p.buf.ptr, None, o.buf.ptr) == inv and dev(c.buf.ptr, p.buf.ptr, nr.buf.ptr, None) == inv
    assert dev(c.buf.ptr, p.buf.ptr, nr.buf.ptr, p.buf.ptr) == inv and dev(c.buf.ptr, p.buf.ptr, nr.buf.ptr, nr.buf.ptr) == inv
    assert dev(c.buf.ptr, p.buf.ptr, nr.buf.ptr, C.c_void_p(c.buf.address + 8 * 108 - 4)) == inv, "the coefficients count as an input of dims product * 27 floats"
    assert b"the output overlaps an input" in lib.rt_last_error(h)
    sc.ctx.synchronize()
    assert o.untouched() and not ho.any()
    c.check(); p.check(); nr.check()
    assert calls(G()) == [0, 0]
    sc.ctx.synchronize()
    assert same(o.read().reshape(n, 3), pr.lookup(grid, Cf, P, N)) and same(ho, pr.lookup(grid, Cf, P, N))


# ------------------------------------------------------------------------------------------ 9. the context afterwards
def frame(sc, w, h):
    fs = sc.fs
    fs.areaLight, fs.pointLight, fs.usteps, fs.vsteps, fs.max_depth = True, False, 5, 5, 4
    rgb = fs.raytraceScene(w, h, write_ppm=False).copy()
    st = fs.stats
    return rgb, (int(st.launches_total), int(st.rays_primary), int(st.rays_bounce), int(st.rays_centre), int(st.rays_sample),
                 int(st.pixels), int(st.pixels_culled), int(st.shaded_hits))


def test_probe_calls_leave_the_context_as_it_was(world):
    sc = world["mixed"]
    before, counters_before = frame(sc, 64, 40)
    for m in (3, 8, 10):
        assert same(run(sc, sc.P, m, direct=True), sc.want(m, direct=True))
    after, counters_after = frame(sc, 64, 40)
    assert same(before, after) and counters_before == counters_after
    assert counters_before[0] > 0 and counters_before[1] > 0


def test_probes_on_a_second_stream_beside_a_frame(rt, world):
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
        o, ip = run(sc, sc.P, 3, direct=True, stream=stream.value, sync=False)
        assert hip.hipStreamSynchronize(stream) == 0
        sc.ctx.synchronize()
        assert same(o.read().reshape(sc.n, 27), sc.want(3, direct=True))
        ip.check()
        assert same(rgb.read().reshape(40, 64, 3), want_rgb)
    finally:
        hip.hipStreamDestroy(stream)


def test_refined_count_and_pass_map_survive_the_calls(rt, world):
    sc = world["cube"]
    fs = sc.fs
    rng = np.random.default_rng(4)
    lgrid = pr.Grid((0, 0, 0), (1, 1, 1), (2, 2, 2))
    Cf = rng.standard_normal((8, 27)).astype(F)
    LP, LN = lookup_points(lgrid, 300, rng)
    fs.supersample, fs.supersample_threshold = 2, 0.05
    try:
        frame(sc, 64, 40)
        want = sc.ctx.supersampling_refined()
        frame(sc, 64, 40)
        got = run(sc, sc.P, 3)
        assert same(lookup_run(sc, lgrid, Cf, LP, LN), pr.lookup(lgrid, Cf, LP, LN))
        assert sc.ctx.supersampling_refined() == want and 0 < want < 64 * 40
        assert same(got, sc.want(3))
    finally:
        fs.supersample, fs.supersample_threshold = 1, -1.0
        sc.ctx.set_supersampling(1)
        sc.ctx.set_supersampling_threshold(-1.0)
    # an adaptive-pass frame's map
    w, h = 64, 40
    try:
        sc.ctx.set_passes(0, 12)
        sc.ctx.set_pass_tolerance(0.01, 4)
        cam, L, p = rt.default_camera(w, h, 0.4), fs._lights(), rt.make_params(w, h, 2)
        rgb = np.zeros((h, w, 3), F)
        st = rt.capi.rt_stats()
        render = lambda: rt.capi.check(sc.lib, sc.ctx.handle, sc.lib.rt_render(sc.ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p),
                                                                              None, C.byref(st)), "rt_render")
        render()
        first = rgb.copy()
        pm = sc.ctx.pass_map(w, h)
        assert pm.shape == (h, w) and (pm < 12).any() and (pm > 0).any()
        assert same(run(sc, sc.P, 8, direct=True), sc.want(8, direct=True))
        assert same(lookup_run(sc, lgrid, Cf, LP, LN), pr.lookup(lgrid, Cf, LP, LN))
        assert np.array_equal(sc.ctx.pass_map(w, h), pm)
        render()
        assert same(rgb, first)
    finally:
        sc.ctx.set_passes(0, 1)
        sc.ctx.set_pass_tolerance(-1.0, 8)


# ------------------------------------------------------------------------------------------ 10. RT_NO_CULL and the counting build
WORK_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")


@pytest.mark.parametrize("variant", ["no_cull", "counting"])
def test_switch_and_counting_build_give_the_same_bits(rt, world, monkeypatch, variant):
    if variant == "no_cull":
        monkeypatch.setenv("RT_NO_CULL", "1")
    lib = rt.capi.load_library(WORK_LIB) if variant == "counting" else rt.load_library()
    fp = lambda a: a.ctypes.data_as(C.c_void_p)
    L = lights_of(rt, TWO, WHITE)
    rng = np.random.default_rng(6)
    for name in ("mixed", "toy"):
        sc = world[name]
        ctx = C.c_void_p()
        assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK                 # (a fresh context: it reads RT_* when it is made and at upload)
        try:
            rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(sc.fs.scene.view)), "rt_upload_scene")
            for m in (3, 8):
                out = np.full((sc.n, 27), 7, F)
                rt.capi.check(lib, ctx, lib.rt_light_probes(ctx, C.byref(L), sc.n, fp(np.ascontiguousarray(sc.P)), m, 1, fp(out)), "rt_light_probes")
                want = sc.want(m, TWO, direct=True)
                assert same(out, want), (variant, name, m, differing(out, want))
            g = rt.probe_grid(sc.grid.origin, sc.grid.step, sc.grid.dims)
            P, N = lookup_points(sc.grid, 500, rng)
            rgb = np.full((500, 3), 7, F)
            rt.capi.check(lib, ctx, lib.rt_probe_irradiance(ctx, C.byref(g), fp(out), 500, fp(P), fp(N), fp(rgb)), "rt_probe_irradiance")
            assert same(rgb, pr.lookup(sc.grid, out, P, N))
        finally:
            lib.rt_destroy(ctx)


# ------------------------------------------------------------------------------------------ 11. torch tensors and the Flyscene members
def test_torch_tensors_and_flyscene_members(world):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no device"
    sc = world["toy"]
    rt = sc.rt
    m = 3
    L = lights_of(rt, ONE, YELLOW)
    want = sc.want(m, color=YELLOW, direct=True)
    dev = f"cuda:{sc.ctx.device}"
    tp = torch.from_numpy(sc.P).to(dev)
    tc = sc.ctx.light_probes(tp, L, m, direct=True)
    sc.ctx.synchronize()
    torch.cuda.synchronize()
    assert tc.dtype == torch.float32 and tuple(tc.shape) == (sc.n, 27) and str(tc.device) == dev
    assert same(tc.cpu().numpy(), want)
    rng = np.random.default_rng(8)
    P, N = lookup_points(sc.grid, 700, rng)
    g = rt.probe_grid(sc.grid.origin, sc.grid.step, sc.grid.dims)
    want_rgb = pr.lookup(sc.grid, want, P, N)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        tc2 = sc.ctx.light_probes(tp.clone(), L, m, direct=True)
        trgb = sc.ctx.probe_irradiance(g, tc2, torch.from_numpy(P).to(dev), torch.from_numpy(N).to(dev))
    s.synchronize()
    assert trgb.dtype == torch.float32 and tuple(trgb.shape) == (700, 3) and same(trgb.cpu().numpy(), want_rgb)
    for bad in (tp.double(), torch.zeros((sc.n, 4), dtype=torch.float32, device=dev)):
        with pytest.raises(ValueError):
            sc.ctx.light_probes(bad, L, m)
    with pytest.raises(ValueError):
        sc.ctx.probe_irradiance(g, tc[:-1].contiguous(), torch.from_numpy(P).to(dev), torch.from_numpy(N).to(dev))
    # the Flyscene members: a volume over the scene's root box, looked up at the closest hits of the camera
    fs = sc.fs
    keep = fs.camera
    try:
        fs.camera = rt.default_camera(fs.width, fs.height, 0.4)
        fs.areaLight, fs.pointLight = False, True
        pg, coeff = fs.light_probes((3, 2, 4), m, direct=True, margin=0.25)
        img = fs.probe_irradiance(48, 32, (pg, coeff))
    finally:
        fs.camera = keep
        fs.areaLight, fs.pointLight = True, False
    box = fs.scene.info()["root_box"]
    ref_grid = pr.Grid.over(box, (3, 2, 4), 0.25)
    got_grid = pr.Grid.of(pg)
    assert same(got_grid.origin, ref_grid.origin) and same(got_grid.step, ref_grid.step) and got_grid.dims == (3, 2, 4)
    own = fs._lights()
    ref_coeff = pr.probes(sc.tracers["library"], sc.data, ref_grid.positions(), m, [tuple(own.pos[0])], tuple(own.color), direct=True)
    assert coeff.shape == (24, 27) and same(coeff, ref_coeff)
    (o, d, f, t), _ = ao_ref.camera_points(sc.orc, sc.osc, 48, 32, 0.4)
    HP, HN = ao_ref.hit_points(o, d, f, t, sc.osc.arrays()["face_normal"])
    ref_img = pr.lookup(ref_grid, ref_coeff, HP, HN)
    assert img.shape == (32, 48, 3) and img.dtype == np.float32 and same(img.reshape(-1, 3), ref_img)
    assert zero_bits(ref_img[f < 0]) and (ref_img[f >= 0] != 0).any()
