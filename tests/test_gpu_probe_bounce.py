"""Bounced light on a real MI355X: rt_light_probes_bounce_device and rt_indirect_diffuse_bounce_device return, bit for bit, what
tests/probe_bounce_ref.py gets from the definition over rt_closest_hits / rt_light_strikes (indirect_ref.LibraryTracer, as the parents'
tests use it) -- in every wave layout, in the plain and in the visible mode, with traced, random and single-layer sources; a source of zeros
gives the parents' device output in every bit; on the sealed rooms the visible feedback keeps the dark room exactly black and the plain one
leaks; the strided round; the calls leave the context as it was and refuse what the header says they refuse; the Flyscene members."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ao_ref
import grid_caps as gc
import indirect_ref as ir
import probe_bounce_ref as pb
import probe_ref as pr
import probe_visible_ref as pv
import scenes_gen
import switch_table
from test_gpu_ao import In, Out, same

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["rooms", "mixed", "soup"]
ONE = ((-1.0, 1.0, 1.0),)
WHITE, WARM = (1.0, 1.0, 1.0), (1.0, 0.75, 0.5)
SEED = 11
EXTRA = 37                                       # positions behind the 16 of the grid: 53 is a multiple of no group size
fp = lambda a: a.ctypes.data_as(C.c_void_p)


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
    g, w = np.ascontiguousarray(got, F).reshape(len(got), -1), np.ascontiguousarray(want, F).reshape(len(want), -1)
    return np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)).any(axis=1))[:8]


class Scene:
    """a scene on the GPU and in the CPU checker; its 4 x 2 x 2 source grid (room_grid on the two rooms, else over the bounding box of the
    vertices); its probe set (the 16 positions of that grid, then EXTRA seeded positions in and round the box); its gather points (on the
    two rooms room_b_points and their mirror images in room A, else seeded hits of the probe rays with their turned face normals); three
    sources (traced: pass 0 of the grid at m = 4 without the direct term; random, with negative lobes; flat: random on the 4 x 1 x 2 grid
    through the box's middle); and the traced part of the reference, computed once per m"""

    def __init__(self, rt, oracle, path, seed, rooms):
        self.rt, self.orc = rt, oracle
        self.fs = rt.Flyscene(scene_path=path)
        self.fs.initialize(64, 40, True, False)
        self.ctx, self.lib = self.fs.ctx, self.fs.ctx.lib
        self.osc = oracle.load_scene(path)
        self.data = ir.SceneData(self.osc)
        self.tracer = ir.LibraryTracer(rt, self.ctx)
        w = np.asarray(self.osc.arrays()["wverts"], F)
        lo, hi = w.min(axis=0).astype(np.float64), w.max(axis=0).astype(np.float64)
        rng = np.random.default_rng(seed)
        if rooms:
            self.W = ir.to_world(self.osc, pv.ROOM_VERTS)
            self.grid = pv.room_grid(self.W)
            self.pos = (tuple(float(v) for v in self.W(pv.ROOM_LIGHT)),)
            self.wall = float(self.W([0, 0, 0])[0])
        else:
            self.grid = pr.Grid.over(np.concatenate([lo, hi]).astype(F), (4, 2, 2), -0.1)
            self.pos = ONE
        g = self.grid
        mid = g.origin[1] + F(0.5) * g.step[1]
        self.flat = pr.Grid((g.origin[0], mid, g.origin[2]), g.step, (4, 1, 2))
        self.P = np.ascontiguousarray(np.concatenate([g.positions(), (lo - 0.1 * (hi - lo) + rng.random((EXTRA, 3)) * 1.2 * (hi - lo)).astype(F)]), F)
        self.n = len(self.P)
        traced = np.full((g.cells, 27), 7, F)
        L = lights_of(rt, self.pos, WHITE)
        rt.capi.check(self.lib, self.ctx.handle, self.lib.rt_light_probes(self.ctx.handle, C.byref(L), g.cells, fp(g.positions()), 4, 0, fp(traced)), "rt_light_probes")
        self.src = {"traced": (g, traced), "random": (g, (0.5 * rng.standard_normal((g.cells, 27))).astype(F)),
                    "flat": (self.flat, (0.5 * rng.standard_normal((self.flat.cells, 27))).astype(F))}
        self.ref, self.vis, self.gref = {}, {}, {}
        if rooms:
            PB, NB = pv.room_b_points(self.W)
            PA = PB.copy()
            PA[:, 0] = 2 * F(self.wall) - PB[:, 0]
            self.GP, self.GN = np.concatenate([PB, PA]), np.concatenate([NB, NB])
        else:
            h = self.traced(4).hits
            pick = rng.permutation(len(h.H))[:150]
            self.GP, self.GN = h.H[pick].copy(), h.Nf[pick].copy()
        self.GN[5] = 0.0                                          # no point
        self.GP, self.GN = np.ascontiguousarray(self.GP, F), np.ascontiguousarray(self.GN, F)

    def traced(self, m):
        if m not in self.ref:
            self.ref[m] = pb.trace_probes(self.tracer, self.data, self.P, m, self.pos)
        return self.ref[m]

    def seen(self, m, which):
        key = (m, "flat" if which == "flat" else "grid")
        if key not in self.vis:
            self.vis[key] = pb.source_visibility(self.tracer, self.src[which][0], self.traced(m).hits)
        return self.vis[key]

    def want(self, m, which, visible, direct=False, color=WHITE):
        grid, coeff = self.src[which]
        tr = self.traced(m)
        return pb.shade_probes(tr, color, direct, pb.source_lookup(grid, coeff, tr.hits, self.seen(m, which) if visible else None))

    def gather_traced(self, m):
        if m not in self.gref:
            self.gref[m] = pb.trace_gather(self.tracer, self.data, self.GP, self.GN, m, SEED, self.pos)
        return self.gref[m]

    def gather_want(self, m, which, visible, color=WHITE):
        grid, coeff = self.src[which]
        hits, live = self.gather_traced(m)
        vis = pb.source_visibility(self.tracer, grid, hits) if visible else None
        return pb.shade_gather(hits, live, color, pb.source_lookup(grid, coeff, hits, vis))

    def close(self):
        self.ctx.close()
        self.fs.scene.close()
        self.osc.close()


@pytest.fixture(scope="module")
def world(rt, oracle, tmp_path_factory):
    paths = {"rooms": pv.two_rooms(str(tmp_path_factory.mktemp("rooms"))), "mixed": scenes_gen.mixed_materials(str(tmp_path_factory.mktemp("mixed"))),
             "soup": scenes_gen.random_soup(str(tmp_path_factory.mktemp("soup")), 41, 200)}
    w = {k: Scene(rt, oracle, paths[k], 300 + i, k == "rooms") for i, k in enumerate(NAMES)}
    yield w
    for s in w.values():
        s.close()


def run_probes(sc, P, m, source, visible, direct=False, color=WHITE, stream=None, sync=True):
    """rt_light_probes_bounce_device on DeviceBuffers with guards -> coefficients (n, 27) as read back"""
    rt, n = sc.rt, len(P)
    grid, coeff = source
    p, c = In(rt, P.reshape(-1, 3) if n else np.zeros((1, 3), F)), In(rt, coeff)
    o = Out(rt, n, 27, np.float32)
    g = rt.probe_grid(grid.origin, grid.step, grid.dims)
    got = sc.ctx.light_probes(p.buf, lights_of(rt, sc.pos, color), m, direct=direct, n=n, out=o.buf, stream=stream, source=(g, c.buf), visible=visible)
    assert got is o.buf
    if not sync:
        return o, (p, c)
    sc.ctx.synchronize()
    p.check(); c.check()
    return o.read().reshape(n, 27)


def run_gather(sc, P, N, m, source, visible, color=WHITE, stream=None):
    rt, n = sc.rt, len(P)
    grid, coeff = source
    p, nr, c = In(rt, P), In(rt, N), In(rt, coeff)
    o = Out(rt, n, 3, np.float32)
    g = rt.probe_grid(grid.origin, grid.step, grid.dims)
    got = sc.ctx.indirect_diffuse(p.buf, nr.buf, lights_of(rt, sc.pos, color), m, seed=SEED, n=n, out=o.buf, stream=stream, source=(g, c.buf), visible=visible)
    assert got is o.buf
    sc.ctx.synchronize()
    p.check(); nr.check(); c.check()
    return o.read().reshape(n, 3)


# ------------------------------------------------------------------------------------------ 1. bit equality with the checker
@pytest.mark.parametrize("name", NAMES)
def test_probes_equal_the_reference(world, name):
    """m = 2: 16 probes per wave; 8: one probe, one round; 10: 16 probes straddling 25 rounds; 16: one probe in four rounds"""
    sc = world[name]
    assert sc.n == 53 and all(sc.n % group(m) for m in (2, 10))
    for m in (2, 8, 10, 16):
        for visible in ((False, True) if m in (2, 10) else (False,)):
            for which, direct, color in (("traced", False, WHITE), ("random", True, WARM), ("flat", False, WARM)):
                want = sc.want(m, which, visible, direct, color)
                got = run_probes(sc, sc.P, m, sc.src[which], visible, direct, color)
                assert got.dtype == np.float32 and same(got, want), (name, m, visible, which, differing(got, want))
    # the fixture: the source shows, the visible mode differs from the plain one, and hits are clamped
    tr = sc.traced(2)
    parent = pb.shade_probes(tr, WHITE, False)
    assert len(differing(sc.want(2, "traced", False), parent)) >= 8, "the source must show"
    I = pb.source_lookup(*sc.src["random"], tr.hits)
    assert (I < 0).sum() >= 8 and (I > 0).sum() >= 8
    if name != "soup":
        assert len(differing(sc.want(10, "random", True), sc.want(10, "random", False))) >= 1, "blocked corners must occur"
    print(name, "hits at m = 2:", len(tr.hits.H), " hits without a normal:", int((~(tr.hits.Nf != 0).any(axis=1)).sum()))


@pytest.mark.parametrize("name", NAMES)
def test_gather_equals_the_reference(world, name):
    sc = world[name]
    if name == "rooms":
        assert len(sc.GP) == 144
    for m in (3, 8, 10):
        for visible in (False, True):
            for which in (("traced", "flat") if m == 3 else ("random",)):
                want = sc.gather_want(m, which, visible)
                got = run_gather(sc, sc.GP, sc.GN, m, sc.src[which], visible)
                assert got.dtype == np.float32 and same(got, want), (name, m, visible, which, differing(got, want))
                assert zero_bits(got[5])
    parent = ir.gather(sc.tracer, sc.data, sc.GP, sc.GN, 3, SEED, sc.pos, WHITE)
    assert len(differing(sc.gather_want(3, "traced", False), parent)) >= 8, "the source must show"


def test_culling_off_and_the_counting_build_give_the_same_bits(rt, world, monkeypatch):
    work = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")
    for variant in ("no_cull", "counting"):
        if variant == "no_cull":
            monkeypatch.setenv("RT_NO_CULL", "1")
        else:
            monkeypatch.delenv("RT_NO_CULL", raising=False)
        lib = rt.capi.load_library(work) if variant == "counting" else rt.load_library()
        for name in ("rooms", "mixed"):
            sc = world[name]
            L = lights_of(rt, sc.pos, WHITE)
            grid, coeff = sc.src["random"]
            g = rt.probe_grid(grid.origin, grid.step, grid.dims)
            ctx = C.c_void_p()
            assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK             # (a fresh context: it reads RT_* when it is made and at upload)
            try:
                rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(sc.fs.scene.view)), "rt_upload_scene")
                out, rgb = np.full((sc.n, 27), 7, F), np.full((len(sc.GP), 3), 7, F)
                rt.capi.check(lib, ctx, lib.rt_light_probes_bounce(ctx, C.byref(L), sc.n, fp(sc.P), 10, 1, C.byref(g), fp(coeff), 1, fp(out)), "rt_light_probes_bounce")
                rt.capi.check(lib, ctx, lib.rt_indirect_diffuse_bounce(ctx, C.byref(L), len(sc.GP), fp(sc.GP), fp(sc.GN), 3, SEED, C.byref(g), fp(coeff), 1, fp(rgb)),
                              "rt_indirect_diffuse_bounce")
            finally:
                lib.rt_destroy(ctx)
            assert same(out, sc.want(10, "random", True, True)), (variant, name)
            assert same(rgb, sc.gather_want(3, "random", True)), (variant, name)


# ------------------------------------------------------------------------------------------ 2. a source of zeros
@pytest.mark.parametrize("name", NAMES)
def test_a_zero_source_gives_the_parents_output(world, name):
    sc = world[name]
    zero = (sc.grid, np.zeros((sc.grid.cells, 27), F))
    for m in (2, 10):
        for direct in (False, True):
            p, o = In(sc.rt, sc.P), Out(sc.rt, sc.n, 27, np.float32)
            sc.ctx.light_probes(p.buf, lights_of(sc.rt, sc.pos, WARM), m, direct=direct, n=sc.n, out=o.buf)
            sc.ctx.synchronize()
            parent = o.read().reshape(sc.n, 27)
            for visible in (False, True):
                assert same(run_probes(sc, sc.P, m, zero, visible, direct, WARM), parent), (name, m, direct, visible)
    assert (parent != 0).any()
    p, nr, o = In(sc.rt, sc.GP), In(sc.rt, sc.GN), Out(sc.rt, len(sc.GP), 3, np.float32)
    sc.ctx.indirect_diffuse(p.buf, nr.buf, lights_of(sc.rt, sc.pos, WARM), 3, seed=SEED, n=len(sc.GP), out=o.buf)
    sc.ctx.synchronize()
    parent = o.read().reshape(-1, 3)
    for visible in (False, True):
        assert same(run_gather(sc, sc.GP, sc.GN, 3, zero, visible, WARM), parent), (name, visible)


# ------------------------------------------------------------------------------------------ 3. the sealed rooms
def device_feedback(sc, m, bounces, visible):
    """pass 0 by the parent call, then `bounces` passes that take the previous volume as their source, two buffers swapped"""
    pos = sc.grid.positions()
    p, o = In(sc.rt, pos), Out(sc.rt, len(pos), 27, np.float32)
    sc.ctx.light_probes(p.buf, lights_of(sc.rt, sc.pos, WHITE), m, n=len(pos), out=o.buf)
    sc.ctx.synchronize()
    out = [o.read().reshape(len(pos), 27)]
    for _ in range(bounces):
        out.append(run_probes(sc, pos, m, (sc.grid, out[-1]), visible))
    return out


def test_sealed_rooms_on_the_device(world):
    sc = world["rooms"]
    pos = sc.grid.positions()
    room_b = pos[:, 0] > sc.wall
    assert room_b.sum() == 8
    seen, leaky = device_feedback(sc, 4, 3, True), device_feedback(sc, 4, 3, False)
    for b in range(4):
        assert zero_bits(seen[b][room_b]), f"visible pass {b}: room B stays exactly +0.0f"
    assert (leaky[1][room_b] != 0).any() and (leaky[3][room_b] != 0).any(), "the plain lookup leaks"
    assert (seen[1][~room_b][:, 0:3] > seen[0][~room_b][:, 0:3]).all(), "room A's DC grows with the first bounce"
    for visible, got in ((True, seen), (False, leaky)):
        want = pb.feedback(sc.tracer, sc.data, sc.grid, 4, sc.pos, WHITE, False, 3, visible)
        for b in range(4):
            assert same(got[b], want[b]), (visible, b, differing(got[b], want[b]))


# ------------------------------------------------------------------------------------------ 4. more units than the grid holds
def stride_shape(sc, m):
    K = m * m
    rounds = K // math.gcd(K, 64)
    cus = gc.cu_count(sc.ctx.device)
    units = gc.round_two(gc.ao_cap(cus, rounds)) + 5
    n = (units - 1) * group(m) + min(3, group(m))
    assert -(-n // group(m)) == units
    assert units > gc.ao_cap(cus, rounds) and gc.ao_grid(units, cus, rounds) * gc.WAVES < units, (cus, units, "the batch does not reach the grid of this device")
    assert gc.strides(units, gc.ao_cap(cus, rounds))
    return n, gc.ao_cap(cus, rounds) * group(m)


def test_probes_grid_stride(world):
    """a probe's answer depends on its position alone: a tiled probe set has a tiled answer (the checker's, on the 53), and the same
    batch in chunks of half a cap, which do not stride, gives the same bits everywhere"""
    sc = world["mixed"]
    n, cap = stride_shape(sc, 2)
    chunk = cap // 2
    reps = -(-n // sc.n)
    P = np.ascontiguousarray(np.tile(sc.P, (reps, 1))[:n])
    got = run_probes(sc, P, 2, sc.src["random"], True, True)
    want = sc.want(2, "random", True, True)
    sample = np.concatenate([np.arange(0, 2 * sc.n), np.arange(n - 2 * sc.n, n)])
    assert same(got[sample], want[sample % sc.n]), differing(got[sample], want[sample % sc.n])
    for a in range(0, n, chunk):
        part = run_probes(sc, P[a:a + chunk], 2, sc.src["random"], True, True)
        assert same(part, got[a:a + chunk]), (a, differing(part, got[a:a + chunk]))


def test_gather_grid_stride(world):
    """the rotation of a gather point depends on its index in the batch, so a chunk of the batch is another query and cannot stand for
    it: the checker, run with the indices of the batch, covers the first 200 points and every fifth point of the strided round"""
    sc = world["mixed"]
    n, cap = stride_shape(sc, 2)
    k = len(sc.GP)
    reps = -(-n // k)
    P, N = np.ascontiguousarray(np.tile(sc.GP, (reps, 1))[:n]), np.ascontiguousarray(np.tile(sc.GN, (reps, 1))[:n])
    got = run_gather(sc, P, N, 2, sc.src["random"], False)
    sample = np.concatenate([np.arange(0, 200), np.arange(cap, n, 5), np.arange(n - 40, n)])
    assert (sample >= cap).sum() >= 1000
    grid, coeff = sc.src["random"]
    want = pb.gather(sc.tracer, sc.data, P[sample], N[sample], 2, SEED, sc.pos, WHITE, grid, coeff, False, i=sample)
    assert same(got[sample], want), differing(got[sample], want)
    assert (want != 0).any()


# ------------------------------------------------------------------------------------------ 5. refusals
def test_no_scene_and_bad_arguments(rt, world):
    sc = world["mixed"]
    lib, inv, uns, h = sc.lib, rt.capi.RT_ERR_INVALID, rt.capi.RT_ERR_UNSUPPORTED, sc.ctx.handle
    n, k = sc.n, len(sc.GP)
    grid, coeff = sc.src["random"]
    p, c, gp, gn = In(rt, sc.P), In(rt, coeff), In(rt, sc.GP), In(rt, sc.GN)
    o, rgb = Out(rt, n, 27, np.float32), Out(rt, k, 3, np.float32)
    ho, hrgb = np.zeros((n, 27), F), np.zeros((k, 3), F)
    good = lights_of(rt, sc.pos, WHITE)
    G = lambda step=None, dims=None: rt.probe_grid(grid.origin, grid.step if step is None else step, grid.dims if dims is None else dims)

    def calls(hh, g, nn=None, m=3, L=good, src=True):
        gp_ = C.byref(g) if g is not None else None
        n1, n2 = (n, k) if nn is None else (nn, nn)
        return [lib.rt_light_probes_bounce_device(hh, C.byref(L), n1, p.buf.ptr, m, 0, gp_, c.buf.ptr if src else None, 1, o.buf.ptr, None),
                lib.rt_light_probes_bounce(hh, C.byref(L), n1, fp(sc.P), m, 0, gp_, fp(coeff) if src else None, 0, fp(ho)),
                lib.rt_indirect_diffuse_bounce_device(hh, C.byref(L), n2, gp.buf.ptr, gn.buf.ptr, m, SEED, gp_, c.buf.ptr if src else None, 0, rgb.buf.ptr, None),
                lib.rt_indirect_diffuse_bounce(hh, C.byref(L), n2, fp(sc.GP), fp(sc.GN), m, SEED, gp_, fp(coeff) if src else None, 1, fp(hrgb))]

    empty = rt.Context(0)
    try:
        for nn in (None, 0):
            assert calls(empty.handle, G(), nn) == [rt.capi.RT_ERR_NO_SCENE] * 4
        assert b"before rt_upload_scene" in lib.rt_last_error(empty.handle)
    finally:
        empty.close()
    assert calls(h, G(), 0) == [0] * 4 and calls(h, G(), -1) == [inv] * 4
    for m in (0, 17, -3):
        assert calls(h, G(), m=m) == [inv] * 4 and calls(h, G(), 0, m=m) == [inv] * 4, m
    # the source: a NULL or bad grid whatever n is, NULL coefficients
    assert calls(h, None) == [inv] * 4 and calls(h, None, 0) == [inv] * 4
    for g in (G(dims=(0, 2, 2)), G(dims=(2, -1, 2)), G(dims=(4096, 4096, 2)), G(step=(0, 1, 1)), G(step=(1, 1, float("inf"))), G(step=(float("nan"), 1, 1))):
        assert calls(h, g) == [inv] * 4 and calls(h, g, 0) == [inv] * 4, (list(g.step), list(g.dims))
    assert calls(h, G(), src=False) == [inv] * 4
    assert b"source" in lib.rt_last_error(h)
    sphere = rt.make_lights(ONE, area=True)
    keep = rt.set_sphere(sphere, rt.sphere_offsets(3, 1.0, 25))                     # noqa: F841 -- keeps the offsets alive
    assert calls(h, G(), L=sphere) == [uns] * 4
    # an output that shares a byte with the source: in place, its last byte, its first byte
    g = G()
    probes = lambda src, out: lib.rt_light_probes_bounce_device(h, C.byref(good), grid.cells, p.buf.ptr, 3, 0, C.byref(g), src, 0, out, None)
    gather = lambda src, out: lib.rt_indirect_diffuse_bounce_device(h, C.byref(good), k, gp.buf.ptr, gn.buf.ptr, 3, SEED, C.byref(g), src, 0, out, None)
    assert probes(c.buf.ptr, c.buf.ptr) == inv, "an update in place"
    assert b"the output overlaps the source" in lib.rt_last_error(h)
    assert probes(C.c_void_p(o.buf.address + 4), o.buf.ptr) == inv
    assert gather(c.buf.ptr, C.c_void_p(c.buf.address + grid.cells * 108 - 1)) == inv and gather(C.c_void_p(rgb.buf.address + k * 12 - 1), rgb.buf.ptr) == inv
    assert probes(c.buf.ptr, p.buf.ptr) == inv and gather(c.buf.ptr, gn.buf.ptr) == inv, "the parents' own rule"
    sc.ctx.synchronize()
    assert o.untouched() and rgb.untouched() and not ho.any() and not hrgb.any()
    for a in (p, c, gp, gn):
        a.check()
    # and what is not refused, in all four forms
    assert calls(h, G()) == [0] * 4
    sc.ctx.synchronize()
    assert same(o.read().reshape(n, 27), sc.want(3, "random", True)) and same(ho, sc.want(3, "random", False))
    assert same(rgb.read().reshape(k, 3), sc.gather_want(3, "random", False)) and same(hrgb, sc.gather_want(3, "random", True))


# ------------------------------------------------------------------------------------------ 6. the context afterwards
def frame(sc, w, h):
    fs = sc.fs
    fs.areaLight, fs.pointLight, fs.usteps, fs.vsteps, fs.max_depth = True, False, 5, 5, 4
    rgb = fs.raytraceScene(w, h, write_ppm=False).copy()
    st = fs.stats
    return rgb, (int(st.launches_total), int(st.rays_primary), int(st.rays_bounce), int(st.rays_centre), int(st.rays_sample),
                 int(st.pixels), int(st.pixels_culled), int(st.shaded_hits))


def test_the_calls_leave_the_context_as_it_was(world):
    sc = world["mixed"]
    fs = sc.fs
    fs.supersample, fs.supersample_threshold = 2, 0.05
    try:
        before, counters_before = frame(sc, 64, 40)
        refined = sc.ctx.supersampling_refined()
        assert same(run_probes(sc, sc.P, 10, sc.src["random"], True), sc.want(10, "random", True))
        assert same(run_gather(sc, sc.GP, sc.GN, 3, sc.src["random"], True), sc.gather_want(3, "random", True))
        assert sc.ctx.supersampling_refined() == refined and 0 < refined < 64 * 40
        after, counters_after = frame(sc, 64, 40)
    finally:
        fs.supersample, fs.supersample_threshold = 1, -1.0
        sc.ctx.set_supersampling(1)
        sc.ctx.set_supersampling_threshold(-1.0)
    assert same(before, after) and counters_before == counters_after
    assert counters_before[0] > 0 and counters_before[1] > 0


def test_on_a_second_stream_beside_a_frame(rt, world):
    sc = world["rooms"]
    hip = rt.hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        want_frame, _ = frame(sc, 64, 40)
        cam = sc.fs.camera
        L, p = sc.fs._lights(), rt.make_params(64, 40, 4)
        img = Out(rt, 64 * 40, 3, np.float32)
        rt.capi.check(sc.lib, sc.ctx.handle, sc.lib.rt_render_device(sc.ctx.handle, C.byref(cam), C.byref(L), C.byref(p), img.buf.ptr, None, None, None, None),
                      "rt_render_device")
        o, ins = run_probes(sc, sc.P, 10, sc.src["traced"], True, stream=stream.value, sync=False)
        assert hip.hipStreamSynchronize(stream) == 0
        sc.ctx.synchronize()
        assert same(o.read().reshape(sc.n, 27), sc.want(10, "traced", True))
        for a in ins:
            a.check()
        assert same(img.read().reshape(40, 64, 3), want_frame)
    finally:
        hip.hipStreamDestroy(stream)


def test_a_second_upload_on_a_live_context_is_honoured(rt, world):
    """one context sees the rooms, then the mixed scene, then the rooms again: every call answers for the scene that is uploaded"""
    lib = rt.load_library()
    ctx = C.c_void_p()
    assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
    try:
        for name in ("rooms", "mixed", "rooms"):
            sc = world[name]
            rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(sc.fs.scene.view)), "rt_upload_scene")
            L = lights_of(rt, sc.pos, WHITE)
            grid, coeff = sc.src["traced"]
            g = rt.probe_grid(grid.origin, grid.step, grid.dims)
            out, rgb = np.full((sc.n, 27), 7, F), np.full((len(sc.GP), 3), 7, F)
            rt.capi.check(lib, ctx, lib.rt_light_probes_bounce(ctx, C.byref(L), sc.n, fp(sc.P), 2, 0, C.byref(g), fp(coeff), 1, fp(out)), "rt_light_probes_bounce")
            rt.capi.check(lib, ctx, lib.rt_indirect_diffuse_bounce(ctx, C.byref(L), len(sc.GP), fp(sc.GP), fp(sc.GN), 3, SEED, C.byref(g), fp(coeff), 0, fp(rgb)),
                          "rt_indirect_diffuse_bounce")
            assert same(out, sc.want(2, "traced", True)) and same(rgb, sc.gather_want(3, "traced", False)), name
    finally:
        lib.rt_destroy(ctx)


# ------------------------------------------------------------------------------------------ 7. the front ends
def test_flyscene_members(world):
    sc = world["mixed"]
    rt, fs, lib, h = sc.rt, sc.fs, sc.lib, sc.ctx.handle
    dims, m = (4, 3, 3), 4
    fs.areaLight, fs.pointLight = False, True
    try:
        L = fs._lights()
        pg0, parent = fs.light_probes(dims, m, direct=True)
        pg, none = fs.light_probes(dims, m, direct=True, bounces=0)
        assert same(none, parent) and (parent != 0).any(), "bounces = 0 is the parent"
        pos = rt.probe_grid_positions(pg)
        want0 = np.empty((len(pos), 27), F)
        rt.capi.check(lib, h, lib.rt_light_probes(h, C.byref(L), len(pos), fp(pos), m, 1, fp(want0)), "rt_light_probes")
        assert same(parent, want0)
        for visible in (True, False):
            a, b, c = (np.empty((len(pos), 27), F) for _ in range(3))
            rt.capi.check(lib, h, lib.rt_light_probes(h, C.byref(L), len(pos), fp(pos), m, 0, fp(a)), "rt_light_probes")
            rt.capi.check(lib, h, lib.rt_light_probes_bounce(h, C.byref(L), len(pos), fp(pos), m, 0, C.byref(pg), fp(a), int(visible), fp(b)), "pass 1")
            rt.capi.check(lib, h, lib.rt_light_probes_bounce(h, C.byref(L), len(pos), fp(pos), m, 1, C.byref(pg), fp(b), int(visible), fp(c)), "pass 2")
            _, got = fs.light_probes(dims, m, direct=True, bounces=2, visible=visible)
            assert same(got, c), visible
            assert not same(got, parent), "two bounces must show"
        _, dflt = fs.light_probes(dims, m, direct=True, bounces=2)
        _, seen = fs.light_probes(dims, m, direct=True, bounces=2, visible=True)
        assert same(dflt, seen), "visible is the default"
        with pytest.raises(ValueError):
            fs.light_probes(dims, m, bounces=-1)
        # the final gather over a bounced volume: the parent's frame with the source at every hit
        _, vol = fs.light_probes(dims, m, direct=False, bounces=2)
        W, H = 24, 16
        keep = fs.camera
        try:
            fs.camera = rt.default_camera(fs.width, fs.height, 0.4)
            img = fs.indirect_diffuse(W, H, 3, seed=SEED, lights=L, probes=(pg, vol))
            plain = fs.indirect_diffuse(W, H, 3, seed=SEED, lights=L, probes=(pg, vol), visible=False)
            without = fs.indirect_diffuse(W, H, 3, seed=SEED, lights=L)
        finally:
            fs.camera = keep
        (o, d, f, t), _ = ao_ref.camera_points(sc.orc, sc.osc, W, H, 0.4)
        HP, HN = ao_ref.hit_points(o, d, f, t, sc.osc.arrays()["face_normal"])
        lpos, lcol = [tuple(L.pos[0])], tuple(L.color)
        grid = pr.Grid.of(pg)
        assert img.shape == (H, W, 3) and img.dtype == np.float32
        assert same(img.reshape(-1, 3), pb.gather(sc.tracer, sc.data, HP, HN, 3, SEED, lpos, lcol, grid, vol, True))
        assert same(plain.reshape(-1, 3), pb.gather(sc.tracer, sc.data, HP, HN, 3, SEED, lpos, lcol, grid, vol, False))
        assert same(without.reshape(-1, 3), ir.gather(sc.tracer, sc.data, HP, HN, 3, SEED, lpos, lcol)) and not same(img, without)
    finally:
        fs.areaLight, fs.pointLight = True, False
