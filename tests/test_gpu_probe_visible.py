"""The leak-free probe lookup on a real MI355X: rt_probe_irradiance_visible_device returns, per point, bit for bit the colour and the mask
that tests/probe_visible_ref.py gets from the definition -- over rt_light_strikes for the whole point sets, and over the CPU checker's
lightStrikes where that is affordable -- on five scenes, with traced and with random coefficients, for every batch length round the
wave unit of 8 points and for more units than the grid holds; where a point sees all of its probes it equals the plain lookup in every
bit; it writes nothing behind its outputs, refuses what the header says it refuses and leaves the context as it was.

The classes of the fixture (probe_visible_ref.classes): every scene must hold 16 points or more that see all of their probes (class 1) and
16 or more with some probes blocked and some USED (class 2); points that see no probe of weight (class 3) need a solid thicker than a
cell is wide or a point inside a wall, which only the two-room scene is built to have: 16 or more there."""
import ctypes as C
import os

import numpy as np
import pytest

import ao_ref
import grid_caps as gc
import indirect_ref as ir
import probe_ref as pr
import probe_visible_ref as pv
import scenes_gen
import switch_table
from test_gpu_ao import GUARD, In, Out, same  # noqa: F401 -- the guarded device arrays of the occlusion tests

pytestmark = pytest.mark.gpu

F = np.float32
FILES = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj", "toy": "toy.obj"}
NAMES = ["rooms", "mixed", "toy", "dodge", "cube"]
ONE = ((-1.0, 1.0, 1.0),)
WHITE = (1.0, 1.0, 1.0)
DIMS, MARGIN = (6, 5, 5), 0.3                   # the grid of tests/test_gpu_probes.py, built again here
W, H = 48, 32
FREE = 600                                      # seeded points in free space
LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 8 * 37 + 1)


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def lights_of(rt, pos, color):
    L = rt.make_lights(pos, area=False)
    for k in range(3):
        L.color[k] = float(color[k])
    return L


def zero_bits(a):
    return not np.ascontiguousarray(a).reshape(-1).view(np.uint8).any()


def differing(got, want):
    g, w = np.ascontiguousarray(got).reshape(len(got), -1), np.ascontiguousarray(want).reshape(len(want), -1)
    return np.flatnonzero((g.view(np.uint8) != w.view(np.uint8)).any(axis=1))[:8]


fp = lambda a: a.ctypes.data_as(C.c_void_p)


class Scene:
    """a scene on the GPU and in the CPU checker, the DIMS grid over the bounding box of its vertices grown by MARGIN, its fixed point set
    (the closest hits of the 48 x 32 camera at yaw 0.4 -- the pixels that hit --, then FREE seeded points in and round the grid, the first
    of them no points and NaN positions), two coefficient volumes (traced at m = 3 with the direct term, and seeded random) and the
    reference of both, computed once"""

    def __init__(self, rt, oracle, path, seed, extra=None):
        self.rt, self.orc = rt, oracle
        self.fs = rt.Flyscene(scene_path=path)
        self.fs.initialize(64, 40, True, False)
        self.ctx, self.lib = self.fs.ctx, self.fs.ctx.lib
        self.osc = oracle.load_scene(path)
        self.tracers = {"oracle": ir.OracleTracer(self.osc), "library": ir.LibraryTracer(rt, self.ctx)}
        w = np.asarray(self.osc.arrays()["wverts"], F)
        self.grid = pr.Grid.over(np.concatenate([w.min(axis=0), w.max(axis=0)]), DIMS, MARGIN)
        _, (HP, HN) = ao_ref.camera_points(oracle, self.osc, W, H, 0.4)
        rng = np.random.default_rng(seed)
        lo = self.grid.origin.astype(np.float64)
        span = self.grid.step.astype(np.float64) * (np.array(DIMS) - 1)
        FP = (lo - 0.15 * span + rng.random((FREE, 3)) * 1.3 * span).astype(F)
        FN = rng.standard_normal((FREE, 3)).astype(F)
        FN[0:4] = 0.0
        FN[2, 1] = -0.0                                        # no point, either sign of zero
        FP[4] = np.nan
        FP[5, 1] = np.nan                                      # NaN positions: cell 0 on that axis
        FP[6, 2] = np.nan
        parts = [(HP, HN), (FP, FN)] + ([extra(self.osc)] if extra else [])
        self.P = np.ascontiguousarray(np.concatenate([p for p, _ in parts]), F)
        self.N = np.ascontiguousarray(np.concatenate([n for _, n in parts]), F)
        self.hits, self.n = len(HP), len(self.P)
        self.special = slice(self.hits, self.hits + 7)
        # the coefficients: real ones, and a random volume
        pos = self.grid.positions()
        real = np.full((len(pos), 27), 7, F)
        L = lights_of(rt, ONE, WHITE)
        rt.capi.check(self.lib, self.ctx.handle, self.lib.rt_light_probes(self.ctx.handle, C.byref(L), len(pos), fp(pos), 3, 1, fp(real)), "rt_light_probes")
        self.coeff = {"real": real, "random": rng.standard_normal((len(pos), 27)).astype(F)}
        self.vis = pv.visibility(self.tracers["library"], self.grid, self.P, self.N)
        self.cls = pv.classes(self.grid, self.P, self.N, self.vis)
        self.want = {k: pv.lookup_visible(self.grid, c, self.P, self.N, self.vis) for k, c in self.coeff.items()}

    def close(self):
        self.ctx.close()
        self.fs.scene.close()
        self.osc.close()


def rooms_extra(osc):
    """points inside the partition's slab (they see no probe: both faces lie between) and the points behind it of the CPU test"""
    Wm = ir.to_world(osc, pv.ROOM_VERTS)
    rng = np.random.default_rng(23)
    inside = np.stack([rng.uniform(-0.04, 0.04, 40), rng.uniform(0.1, 1.4, 40), rng.uniform(-0.9, 0.9, 40)], axis=1)
    PB, NB = pv.room_b_points(Wm)
    return np.concatenate([Wm(inside), PB]), np.concatenate([rng.standard_normal((40, 3)).astype(F), NB])


@pytest.fixture(scope="module")
def world(rt, oracle, scenes, tmp_path_factory):
    paths = {k: os.path.join(scenes, v) for k, v in FILES.items()}
    paths["mixed"] = scenes_gen.mixed_materials(str(tmp_path_factory.mktemp("mixed")))
    paths["rooms"] = pv.two_rooms(str(tmp_path_factory.mktemp("rooms")))
    w = {k: Scene(rt, oracle, paths[k], 100 + i, rooms_extra if k == "rooms" else None) for i, k in enumerate(NAMES)}
    yield w
    for s in w.values():
        s.close()


def run(sc, grid, Cf, P, N, want_mask=True, stream=None, sync=True):
    """rt_probe_irradiance_visible_device on DeviceBuffers with guards -> (rgb (n, 3), mask (n,) or None) as read back"""
    rt = sc.rt
    n = len(P)
    c, p, nr = In(rt, Cf), In(rt, P if n else np.zeros((1, 3), F)), In(rt, N if n else np.zeros((1, 3), F))
    o, k = Out(rt, n, 3, np.float32), (Out(rt, n, 1, np.uint8) if want_mask else None)
    g = rt.probe_grid(grid.origin, grid.step, grid.dims)
    got = sc.ctx.probe_irradiance_visible(g, c.buf, p.buf, nr.buf, n=n, out=o.buf, mask=k.buf if want_mask else None, want_mask=want_mask, stream=stream)
    assert got[0] is o.buf and (got[1] is k.buf if want_mask else got[1] is None)
    if not sync:
        return o, k, (c, p, nr)
    sc.ctx.synchronize()
    c.check(); p.check(); nr.check()
    return o.read().reshape(n, 3), (k.read().reshape(n) if want_mask else None)


def plain_run(sc, grid, Cf, P, N):
    rt = sc.rt
    n = len(P)
    c, p, nr, o = In(rt, Cf), In(rt, P), In(rt, N), Out(rt, n, 3, np.float32)
    sc.ctx.probe_irradiance(rt.probe_grid(grid.origin, grid.step, grid.dims), c.buf, p.buf, nr.buf, n=n, out=o.buf)
    sc.ctx.synchronize()
    return o.read().reshape(n, 3)


# ------------------------------------------------------------------------------------------ 1. every scene, both volumes
@pytest.mark.parametrize("name", NAMES)
def test_colour_and_mask_equal_the_reference(world, name):
    sc = world[name]
    counts = [int((sc.cls == k).sum()) for k in range(4)]
    print(name, "points:", sc.n, " no point / all seen / some blocked / none used:", counts)
    assert counts[0] >= 4 and counts[1] >= 16 and counts[2] >= 16, "the fixture must hold points of the classes"
    if name == "rooms":
        assert counts[3] >= 16
    for kind in ("real", "random"):
        want_rgb, want_mask = sc.want[kind]
        got_rgb, got_mask = run(sc, sc.grid, sc.coeff[kind], sc.P, sc.N)
        assert got_mask.dtype == np.uint8 and same(got_mask, want_mask), (name, kind, differing(got_mask, want_mask))
        assert got_rgb.dtype == np.float32 and same(got_rgb, want_rgb), (name, kind, differing(got_rgb, want_rgb))
        # class 2 is where a wrong blend would show: the reference differs from the plain lookup there
        plain = plain_run(sc, sc.grid, sc.coeff[kind], sc.P, sc.N)
        assert same(plain, pr.lookup(sc.grid, sc.coeff[kind], sc.P, sc.N))
        one, two, three = sc.cls == 1, sc.cls == 2, sc.cls == 3
        assert same(got_rgb[one], plain[one]), "a point that sees all of its probes gets the plain lookup in every bit"
        assert same(got_rgb[three], plain[three]), "a point that sees none falls back to the plain blend"
        if kind == "random":
            assert len(differing(got_rgb[two], plain[two])) >= 8
        # no mask asked for: the same colours
        only_rgb, none = run(sc, sc.grid, sc.coeff[kind], sc.P, sc.N, want_mask=False)
        assert none is None and same(only_rgb, want_rgb)
    # no points and NaN positions
    rgb, mask = sc.want["random"]
    sp = sc.special
    assert zero_bits(rgb[sp][:4]) and zero_bits(mask[sp][:4]) and (sc.cls[sp][:4] == 0).all()
    assert np.isfinite(rgb[sp][4:7]).all() and (rgb[sp][4:7] != 0).any(), "a NaN position takes cell 0 and still has a colour"


def test_library_reference_equals_the_oracle_reference(world):
    """the two tracers give equal references where the CPU checker is affordable (every fifth point of each scene)"""
    for name in NAMES:
        sc = world[name]
        pick = np.arange(0, sc.n, 5)
        a = pv.visibility(sc.tracers["oracle"], sc.grid, sc.P[pick], sc.N[pick])
        assert np.array_equal(a, sc.vis[pick]), name
        rgb, mask = pv.lookup_visible(sc.grid, sc.coeff["real"], sc.P[pick], sc.N[pick], a)
        assert same(rgb, sc.want["real"][0][pick]) and same(mask, sc.want["real"][1][pick])


# ------------------------------------------------------------------------------------------ 2. batch lengths round the wave unit
@pytest.mark.parametrize("name", ["rooms", "dodge"])
def test_batch_lengths_and_guards(world, name):
    sc = world[name]
    want_rgb, want_mask = sc.want["random"]
    # (a point's answer depends on the point alone: a prefix of the batch is the batch of the prefix; start where the classes mix)
    first = sc.hits - 40
    for n in LENGTHS:
        sl = slice(first, first + n)
        rgb, mask = run(sc, sc.grid, sc.coeff["random"], sc.P[sl], sc.N[sl])
        assert rgb.shape == (n, 3) and mask.shape == (n,)
        assert same(rgb, want_rgb[sl]) and same(mask, want_mask[sl]), (name, n, differing(rgb, want_rgb[sl]))
    assert len(set(sc.cls[first:first + LENGTHS[-1]].tolist())) >= 3


# ------------------------------------------------------------------------------------------ 3. the leak, on the device
def test_the_leak_is_gone_on_the_device(world):
    sc = world["rooms"]
    Wm = ir.to_world(sc.osc, pv.ROOM_VERTS)
    grid = pv.room_grid(Wm)
    pos = grid.positions()
    coeff = np.full((len(pos), 27), 7, F)
    L = lights_of(sc.rt, [tuple(float(v) for v in Wm(pv.ROOM_LIGHT))], WHITE)
    sc.rt.capi.check(sc.lib, sc.ctx.handle, sc.lib.rt_light_probes(sc.ctx.handle, C.byref(L), len(pos), fp(pos), 4, 0, fp(coeff)), "rt_light_probes")
    wall = float(Wm([0, 0, 0])[0])
    assert zero_bits(coeff[pos[:, 0] > wall]) and (coeff[pos[:, 0] < wall] != 0).any(axis=1).all()
    P, N = pv.room_b_points(Wm)
    plain = plain_run(sc, grid, coeff, P, N)
    assert 2 * int((plain > 0).any(axis=1).sum()) >= len(P), "the plain lookup leaks"
    rgb, mask = run(sc, grid, coeff, P, N)
    assert zero_bits(rgb) and ((mask & 0x55) == 0).all() and ((mask & 0xAA) == 0xAA).all()
    want = pv.lookup(sc.tracers["oracle"], grid, coeff, P, N)
    assert same(rgb, want[0]) and same(mask, want[1])


# ------------------------------------------------------------------------------------------ 4. more units than the grid holds
def test_grid_stride(world):
    sc = world["toy"]
    cus = gc.cu_count(sc.ctx.device)
    units = gc.round_two(gc.ao_cap(cus, 1)) + 5
    n = (units - 1) * 8 + 3
    assert -(-n // 8) == units and units > gc.ao_cap(cus, 1) and gc.ao_grid(units, cus, 1) * gc.WAVES < units, (cus, units, "the batch does not reach the grid")
    assert gc.strides(units, gc.ao_cap(cus, 1))
    reps = -(-n // sc.n)
    P, N = np.tile(sc.P, (reps, 1))[:n], np.tile(sc.N, (reps, 1))[:n]
    want_rgb, want_mask = (np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:n] for a in sc.want["random"])
    rgb, mask = run(sc, sc.grid, sc.coeff["random"], P, N)
    assert same(rgb, want_rgb) and same(mask, want_mask), differing(rgb, want_rgb)
    second = np.arange(gc.ao_cap(cus, 1) * 8, n)               # the points of the units behind the first round
    assert (sc.cls[second % sc.n] == 2).sum() >= 16, "the strided round holds points with blocked probes"


# ------------------------------------------------------------------------------------------ 5. refusals
def test_no_scene_and_bad_arguments(rt, world):
    sc = world["mixed"]
    lib, inv, h = sc.lib, rt.capi.RT_ERR_INVALID, sc.ctx.handle
    n = 64
    grid = sc.grid
    Cf, P, N = sc.coeff["random"], sc.P[sc.hits:sc.hits + n], sc.N[sc.hits:sc.hits + n]
    c, p, nr = In(rt, Cf), In(rt, P), In(rt, N)
    o, k = Out(rt, n, 3, np.float32), Out(rt, n, 1, np.uint8)
    ho, hk = np.zeros((n, 3), F), np.zeros(n, np.uint8)
    G = lambda step=None, dims=None: rt.probe_grid(grid.origin, grid.step if step is None else step, grid.dims if dims is None else dims)

    def calls(hh, g, nn=n):
        gp = C.byref(g) if g is not None else None
        return [lib.rt_probe_irradiance_visible_device(hh, gp, c.buf.ptr, nn, p.buf.ptr, nr.buf.ptr, o.buf.ptr, k.buf.ptr, None),
                lib.rt_probe_irradiance_visible(hh, gp, fp(Cf), nn, fp(P), fp(N), fp(ho), fp(hk))]

    empty = rt.Context(0)
    try:
        for nn in (n, 0):
            assert calls(empty.handle, G(), nn) == [rt.capi.RT_ERR_NO_SCENE] * 2
        assert b"before rt_upload_scene" in lib.rt_last_error(empty.handle)
    finally:
        empty.close()
    assert calls(h, G(), 0) == [0, 0] and calls(h, G(), -1) == [inv, inv] and calls(h, None) == [inv, inv] and calls(h, None, 0) == [inv, inv]
    for g in (G(dims=(0, 2, 2)), G(dims=(2, -1, 2)), G(dims=(4096, 4096, 2)), G(step=(0, 1, 1)), G(step=(1, -1, 1)), G(step=(1, 1, float("inf"))),
              G(step=(float("nan"), 1, 1))):
        assert calls(h, g) == [inv, inv] and calls(h, g, 0) == [inv, inv], (list(g.step), list(g.dims))
    assert b"rt_probe_irradiance_visible: " in lib.rt_last_error(h)
    g = G()
    dev = lambda pc, pp, pn, po, pk: lib.rt_probe_irradiance_visible_device(h, C.byref(g), pc, n, pp, pn, po, pk, None)
    cb, pb, nb, ob, kb = c.buf.ptr, p.buf.ptr, nr.buf.ptr, o.buf.ptr, k.buf.ptr
    assert dev(None, pb, nb, ob, kb) == inv and dev(cb, None, nb, ob, kb) == inv and dev(cb, pb, None, ob, kb) == inv and dev(cb, pb, nb, None, kb) == inv
    assert dev(cb, pb, nb, pb, kb) == inv and dev(cb, pb, nb, nb, kb) == inv
    assert dev(cb, pb, nb, C.c_void_p(c.buf.address + len(Cf) * 108 - 4), kb) == inv, "the coefficients count as an input of dims product * 27 floats"
    assert b"the output overlaps an input" in lib.rt_last_error(h)
    assert dev(cb, pb, nb, ob, pb) == inv and dev(cb, pb, nb, ob, C.c_void_p(nr.buf.address + n * 12 - 1)) == inv
    assert dev(cb, pb, nb, ob, ob) == inv and dev(cb, pb, nb, ob, C.c_void_p(o.buf.address + n * 12 - 1)) == inv, "the two outputs share a byte"
    assert dev(cb, pb, nb, ob, C.c_void_p(c.buf.address + 5)) == inv
    assert b"the mask overlaps" in lib.rt_last_error(h)
    sc.ctx.synchronize()
    assert o.untouched() and k.untouched() and not ho.any() and not hk.any()
    c.check(); p.check(); nr.check()
    # and what is not refused: both forms, and the host form without a mask
    assert calls(h, G()) == [0, 0]
    sc.ctx.synchronize()
    want_rgb, want_mask = pv.lookup_visible(grid, Cf, P, N, sc.vis[sc.hits:sc.hits + n])
    assert same(o.read().reshape(n, 3), want_rgb) and same(k.read(), want_mask) and same(ho, want_rgb) and same(hk, want_mask)
    ho2 = np.zeros((n, 3), F)
    assert lib.rt_probe_irradiance_visible(h, C.byref(g), fp(Cf), n, fp(P), fp(N), fp(ho2), None) == 0 and same(ho2, want_rgb)
    assert dev(cb, pb, nb, ob, None) == 0
    sc.ctx.synchronize()


# ------------------------------------------------------------------------------------------ 6. the context afterwards
def frame(sc, w, h):
    fs = sc.fs
    fs.areaLight, fs.pointLight, fs.usteps, fs.vsteps, fs.max_depth = True, False, 5, 5, 4
    rgb = fs.raytraceScene(w, h, write_ppm=False).copy()
    st = fs.stats
    return rgb, (int(st.launches_total), int(st.rays_primary), int(st.rays_bounce), int(st.rays_centre), int(st.rays_sample),
                 int(st.pixels), int(st.pixels_culled), int(st.shaded_hits))


def test_the_call_leaves_the_context_as_it_was(world):
    sc = world["mixed"]
    fs = sc.fs
    fs.supersample, fs.supersample_threshold = 2, 0.05
    try:
        before, counters_before = frame(sc, 64, 40)
        refined = sc.ctx.supersampling_refined()
        rgb, mask = run(sc, sc.grid, sc.coeff["real"], sc.P, sc.N)
        assert same(rgb, sc.want["real"][0]) and same(mask, sc.want["real"][1])
        assert sc.ctx.supersampling_refined() == refined and 0 < refined < 64 * 40
        after, counters_after = frame(sc, 64, 40)
    finally:
        fs.supersample, fs.supersample_threshold = 1, -1.0
        sc.ctx.set_supersampling(1)
        sc.ctx.set_supersampling_threshold(-1.0)
    assert same(before, after) and counters_before == counters_after
    assert counters_before[0] > 0 and counters_before[1] > 0


def test_on_a_second_stream_beside_a_frame(rt, world):
    sc = world["toy"]
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
        o, k, ins = run(sc, sc.grid, sc.coeff["real"], sc.P, sc.N, stream=stream.value, sync=False)
        assert hip.hipStreamSynchronize(stream) == 0
        sc.ctx.synchronize()
        assert same(o.read().reshape(sc.n, 3), sc.want["real"][0]) and same(k.read(), sc.want["real"][1])
        for a in ins:
            a.check()
        assert same(img.read().reshape(40, 64, 3), want_frame)
    finally:
        hip.hipStreamDestroy(stream)


# ------------------------------------------------------------------------------------------ 7. the counting build, tensors, the Flyscene member
WORK_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")


def test_counting_build_gives_the_same_bits(rt, world):
    lib = rt.capi.load_library(WORK_LIB)
    sc = world["rooms"]
    ctx = C.c_void_p()
    assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
    try:
        rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(sc.fs.scene.view)), "rt_upload_scene")
        g = rt.probe_grid(sc.grid.origin, sc.grid.step, sc.grid.dims)
        rgb, mask = np.full((sc.n, 3), 7, F), np.full(sc.n, 7, np.uint8)
        rt.capi.check(lib, ctx, lib.rt_probe_irradiance_visible(ctx, C.byref(g), fp(sc.coeff["random"]), sc.n, fp(sc.P), fp(sc.N), fp(rgb), fp(mask)),
                      "rt_probe_irradiance_visible")
        assert same(rgb, sc.want["random"][0]) and same(mask, sc.want["random"][1])
    finally:
        lib.rt_destroy(ctx)


def test_torch_tensors_and_the_flyscene_member(world):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no device"
    sc = world["dodge"]
    rt = sc.rt
    dev = f"cuda:{sc.ctx.device}"
    g = rt.probe_grid(sc.grid.origin, sc.grid.step, sc.grid.dims)
    tc, tp, tn = (torch.from_numpy(a).to(dev) for a in (sc.coeff["real"], sc.P, sc.N))
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        trgb, tmask = sc.ctx.probe_irradiance_visible(g, tc, tp, tn)
        only, none = sc.ctx.probe_irradiance_visible(g, tc, tp, tn, want_mask=False)
    s.synchronize()
    assert trgb.dtype == torch.float32 and tuple(trgb.shape) == (sc.n, 3) and tmask.dtype == torch.uint8 and tuple(tmask.shape) == (sc.n,)
    assert same(trgb.cpu().numpy(), sc.want["real"][0]) and same(tmask.cpu().numpy(), sc.want["real"][1])
    assert none is None and same(only.cpu().numpy(), sc.want["real"][0])
    with pytest.raises(ValueError):
        sc.ctx.probe_irradiance_visible(g, tc[:-1].contiguous(), tp, tn)
    with pytest.raises(ValueError):
        sc.ctx.probe_irradiance_visible(g, tc, tp.double(), tn)
    # the Flyscene member: a volume over the scene's root box, looked up at the closest hits of the camera
    fs = sc.fs
    keep = fs.camera
    try:
        fs.camera = rt.default_camera(fs.width, fs.height, 0.4)
        fs.areaLight, fs.pointLight = False, True
        pg, coeff = fs.light_probes(DIMS, 3, direct=True, margin=0.0)
        img = fs.probe_irradiance(W, H, (pg, coeff), visible=True)
        plain = fs.probe_irradiance(W, H, (pg, coeff))
    finally:
        fs.camera = keep
        fs.areaLight, fs.pointLight = True, False
    grid = pr.Grid.of(pg)
    (o, d, f, t), _ = ao_ref.camera_points(sc.orc, sc.osc, W, H, 0.4)
    HP, HN = ao_ref.hit_points(o, d, f, t, sc.osc.arrays()["face_normal"])
    want, _ = pv.lookup(sc.tracers["library"], grid, coeff, HP, HN)
    assert img.shape == (H, W, 3) and img.dtype == np.float32 and same(img.reshape(-1, 3), want)
    assert same(plain.reshape(-1, 3), pr.lookup(grid, coeff, HP, HN)) and not same(img, plain), "the default is the plain lookup"
