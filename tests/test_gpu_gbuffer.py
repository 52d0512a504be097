"""The geometry-buffer query on a real MI355X: rt_gbuffer_device returns, bit for bit, the eight floats per pixel that the RT_GBUFFER_CHANNELS
section of include/rt_mi355x.h defines -- against the CPU frame of tests/gbuffer_ref.py over the oracle (pinhole) and against the rays of
lens_ref / shutter_ref put through rt_closest_hits_device (lens, shutter) -- for every sample setting, row range and shard, and for frames
of more tiles than the grid holds (tests/grid_caps.py), where waves stride to a second round; it writes nothing outside its output, refuses
what it must and leaves the context as it was.  Every comparison is on the bit patterns."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gbuffer_child
import gbuffer_ref as gr
import grid_caps as gc
import lens_ref
import passes_ref
import scenes_gen
import shutter_ref
import switch_table
import test_gbuffer_api
import test_gpu_lens as gl
import test_gpu_passes as gp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")
WORK_LIB = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")
F = np.float32
YAW = 0.4
SIZES = ((37, 21), (48, 32))                 # not a multiple of the 8 x 8 tile / a multiple of it
SETTINGS = ((1, 0, 1), (2, 0, 1), (3, 5, 1), (2, 1, 3), (4, 255, 1))        # (n, first, count)
GUARD = 64                                   # floats in front of and behind every output, holding PATTERN
PATTERN = 0xA5A5A5A5
NEG0 = 0x80000000
LENS = (0.08, 1.8)
FILES = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj"}


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def differing(a, b):
    return int((bits(a) != bits(b)).any(axis=-1).sum())


class Scene:
    """a scene on the GPU and in the CPU checker; the CPU passes G_p of the pinhole camera at yaw 0.4, computed once per (w, h, n, p)"""

    def __init__(self, rt, oracle, path):
        self.rt, self.orc, self.path = rt, oracle, path
        self.hs, self.ctx = gl.open_ctx(rt, path)
        self.lib = self.ctx.lib
        self.osc = oracle.load_scene(path)
        self.fn = self.osc.arrays()["face_normal"]
        self.kd = gr.face_kd(self.osc)
        assert same(self.fn, self.hs.arrays()["face_normal"]), "the uploaded normals are the checker's"
        self.passes = {}

    def cpu_pass(self, w, h, n, p):
        key = (w, h, n, p)
        if key not in self.passes:
            g = gr.cpu_pass(self.orc, self.osc, self.orc.camera(w, h, YAW), w, h, n, p)
            g.setflags(write=False)
            self.passes[key] = g
        return self.passes[key]

    def cpu_frame(self, w, h, n, first, count):
        return gr.fold_passes([self.cpu_pass(w, h, n, p) for p in range(first, first + count)])

    def settings(self, n=1, passes=(0, 1), lens=None, close=None, tau=-1.0):
        gp.set_frame(self.ctx, n, lens, close, passes, tau)
        self.ctx.set_pass_tolerance(-1.0, 8)

    def close(self):
        self.ctx.close()
        self.hs.close()
        self.osc.close()


@pytest.fixture(scope="module")
def world(rt, oracle, scenes, tmp_path_factory):
    paths = {k: os.path.join(scenes, v) for k, v in FILES.items()}
    paths["mixed"] = scenes_gen.mixed_materials(str(tmp_path_factory.mktemp("mixed")))
    w = {k: Scene(rt, oracle, p) for k, p in paths.items()}
    yield w
    for s in w.values():
        s.close()


class Out:
    """a device output of `floats` floats with GUARD floats of PATTERN on both sides (the output itself starts 16-byte aligned)"""

    def __init__(self, rt, floats):
        self.floats = floats
        self.init = np.full(floats + 2 * GUARD, PATTERN, np.uint32)
        self.buf = rt.hipmem.DeviceBuffer(self.init.nbytes).from_numpy(self.init)
        self.ptr = C.c_void_p(self.buf.address + GUARD * 4)

    def raw(self):
        return self.buf.to_numpy(np.uint32, self.init.shape)

    def read(self, shape):
        raw = self.raw()
        assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + self.floats:] == PATTERN).all(), "floats outside the output were written"
        body = raw[GUARD:GUARD + self.floats]
        assert (body != PATTERN).all(), "floats of the output were left unwritten"
        return body.view(F).reshape(shape)

    def untouched(self):
        return (self.raw() == PATTERN).all()

    def free(self):
        self.buf.free()


def call(sc, cam, p, stream=None, sync=True):
    """rt_gbuffer_device of the context's settings between guards -> float32 (local rows, W, 8)"""
    rows = sc.lib.rt_local_rows(C.byref(p))
    o = Out(sc.rt, rows * p.width * 8)
    sc.rt.capi.check(sc.lib, sc.ctx.handle, sc.lib.rt_gbuffer_device(sc.ctx.handle, C.byref(cam), C.byref(p), o.ptr, stream), "rt_gbuffer_device")
    if not sync:
        return o
    sc.ctx.synchronize()
    try:
        return o.read((rows, p.width, 8))
    finally:
        o.free()


def gbuffer(sc, w, h, yaw=YAW, **rows):
    return call(sc, sc.rt.default_camera(w, h, yaw), sc.rt.make_params(w, h, **rows))


# ------------------------------------------------------------------------------------------ 1. pinhole against the CPU frame
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["cube", "dodge", "mixed"])
def test_pinhole_equals_the_cpu_frame(world, name, size):
    sc = world[name]
    w, h = size
    parts = {}
    for n, first, count in SETTINGS:
        sc.settings(n, (first, count))
        got = gbuffer(sc, w, h)
        want = sc.cpu_frame(w, h, n, first, count)
        print(f"{name} {w}x{h} n={n} passes=({first}, {count}): {differing(got, want)} pixels differ, coverage {gr.coverage(got)}")
        assert same(got, want), (n, first, count, differing(got, want))
        if count == 1:
            parts[(n, first)] = gr.coverage(got)
            full, empty, _ = parts[(n, first)]
            assert full > 0 and empty > 0, "the frame must hold covered and empty pixels"
    key = (os.path.basename(sc.path), w, h)
    if key in test_gbuffer_api.SPECIFIED:              # the partly covered pixels the definition was specified with: no test passes on empty frames
        assert (parts[(2, 0)][2], parts[(3, 5)][2]) == test_gbuffer_api.SPECIFIED[key]
    assert parts[(1, 0)][2] == 0
    if name == "mixed":
        sc.settings(2, (0, 1))
        g = gbuffer(sc, w, h)
        assert len({tuple(x) for x in g[g[..., 0] == 1.0][:, 5:8].tolist()}) >= 4, "the materials show"


@pytest.mark.parametrize("name", ["cube", "dodge", "mixed"])
def test_one_pixel_and_one_tile_frames(world, name):
    sc = world[name]
    for w, h in ((1, 1), (8, 8)):
        for n, first, count in ((1, 0, 1), (3, 5, 1), (2, 1, 3)):
            sc.settings(n, (first, count))
            g = gbuffer(sc, w, h)
            assert same(g, sc.cpu_frame(w, h, n, first, count)), (w, h, n, first, count)
            if w == 8:          # (the raster point of pixel (0, 0) is the frame's corner: the 1 x 1 frame looks past the model, the 8 x 8 frame at it)
                assert (g[..., 0] > 0).any()


# ------------------------------------------------------------------------------------------ 2. the -0.0f rule
def test_negative_zero_normals_survive_one_ray_and_no_sum(world):
    sc = world["dodge"]
    w, h = SIZES[0]
    sc.settings(1, (0, 1))
    one = gbuffer(sc, w, h)
    hit = one[..., 0] == 1.0
    assert same(one, sc.cpu_frame(w, h, 1, 0, 1))
    assert (bits(one[hit][:, 2:5]) == NEG0).any(), "n = 1, count = 1 stores v itself"
    assert (bits(one[~hit]) == 0).all(), "a miss is eight +0.0f"
    for n, passes in ((2, (0, 1)), (1, (0, 2))):
        sc.settings(n, passes)
        g = gbuffer(sc, w, h)
        assert same(g, sc.cpu_frame(w, h, n, *passes))
        assert not (bits(g) == NEG0).any(), "a sum starts from +0.0f: 0.0f + -0.0f = +0.0f"


# ------------------------------------------------------------------------------------------ 3. lens, shutter, both
def ref_blur_pass(sc, a, b, w, h, n, p, lens, rows=None):
    """G_p by the definitions: raster offsets from rt_pass_offsets, scrambles from passes_ref, rays from shutter_ref (close == open where the
    shutter is off: K(t) is then the open camera bit for bit), the pre-test by rt_box_intersect on the root box, the hit by the existing
    Context.closest_hits, the values and the fold by gbuffer_ref"""
    rt, ctx, lib = sc.rt, sc.ctx, sc.lib
    ox, oy = passes_ref.library_offsets(lib, n, p)
    n0, n1 = gp.raster_terms(rt, ctx, a, w, h, n, ox, oy)
    frame_rows = np.arange(h) if rows is None else np.asarray(rows)
    n0, n1 = n0[frame_rows], n1[frame_rows]
    full = None if lens is None else (lens[0], lens[1], lens_ref.library_table(lib, n))
    with passes_ref.pass_scrambles(p):
        O, P, D = shutter_ref.shutter_rays(n0, n1, shutter_ref.pose(a), shutter_ref.pose(b if b is not None else a), n, frame_rows, lens=full)
    N = O.size // 3
    O, P, D = (np.ascontiguousarray(x.reshape(N, 3)) for x in (O, P, D))
    node0 = sc.hs.view.nodes[0]
    boxes = np.ascontiguousarray(np.broadcast_to(np.array(list(node0.bmin) + list(node0.bmax), F), (N, 6)))
    pre = np.zeros(N, np.uint8)
    vptr = lambda x: x.ctypes.data_as(C.c_void_p)
    rt.capi.check(lib, ctx.handle, lib.rt_box_intersect(ctx.handle, N, vptr(boxes), vptr(O), vptr(P), vptr(pre)), "rt_box_intersect")
    bo, bd = rt.hipmem.DeviceBuffer(N * 12).from_numpy(O), rt.hipmem.DeviceBuffer(N * 12).from_numpy(D)
    faces, ts = ctx.closest_hits(bo, bd, n=N)
    ctx.synchronize()
    face, t = faces.to_numpy(np.int32, (N,)), ts.to_numpy(F, (N,))
    for x in (bo, bd, faces, ts):
        x.free()
    face[pre == 0] = -1
    shape = (len(frame_rows), w, n, n)
    return gr.fold_subsamples(gr.sample_values(face.reshape(shape), t.reshape(shape), sc.fn, sc.kd), n)


def ref_blur_frame(sc, a, b, w, h, n, passes, lens, rows=None):
    return gr.fold_passes([ref_blur_pass(sc, a, b, w, h, n, p, lens, rows) for p in range(passes[0], passes[0] + passes[1])])


def blur_cameras(rt, w, h):
    """open = yaw 0.4, close = a yaw of 0.05 from it"""
    return rt.default_camera(w, h, YAW), rt.default_camera(w, h, YAW + 0.05)


@pytest.mark.parametrize("mode", ["lens", "shutter", "both"])
@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_lens_and_shutter_equal_the_reference_rays(world, name, mode):
    sc = world[name]
    w, h = SIZES[0]
    a, b = blur_cameras(sc.rt, w, h)
    lens = LENS if mode in ("lens", "both") else None
    close = b if mode in ("shutter", "both") else None
    sharp = {}
    for n in (2, 3) + ((1,) if mode == "shutter" else ()):
        for passes in ((0, 1), (2, 2)):
            sc.settings(n, passes, lens, close)
            got = call(sc, a, sc.rt.make_params(w, h))
            want = ref_blur_frame(sc, a, close, w, h, n, passes, lens)
            print(f"{name} {mode} n={n} passes={passes}: {differing(got, want)} pixels differ, coverage {gr.coverage(got)}")
            assert same(got, want), (n, passes, differing(got, want))
            full, empty, part = gr.coverage(got)
            assert full > 0 and empty > 0 and (part > 0 or n == 1 and passes[1] == 1)
            if n not in sharp:
                sc.settings(n, passes)
                sharp[n] = call(sc, a, sc.rt.make_params(w, h))
            assert not same(got, sharp[n]), "the blur must show"


# ------------------------------------------------------------------------------------------ 4. agreement with the frame
@pytest.mark.parametrize("name", ["cube", "dodge", "mixed"])
def test_one_ray_buffers_agree_with_the_frame(world, name):
    sc = world[name]
    rt, lib, ctx = sc.rt, sc.lib, sc.ctx
    w, h = SIZES[0]
    sc.settings()
    cam = rt.default_camera(w, h, YAW)
    g = call(sc, cam, rt.make_params(w, h))
    L = gl.area_lights(rt, 5)
    _, hit, _ = gl.render(rt, ctx, cam, L, w, h, 1, hits=True)
    assert ((g[..., 0] == 1.0) == (hit >= 0)).all() and set(np.unique(g[..., 0]).tolist()) == {0.0, 1.0}
    assert same(g[hit >= 0][:, 2:5], sc.fn[hit[hit >= 0]])
    assert same(g[hit >= 0][:, 5:8], sc.kd[hit[hit >= 0]])
    # depth: the t of rt_trace_rays for the pixel's own ray
    pts = np.zeros((h, w, 3), F)
    vptr = lambda x: x.ctypes.data_as(C.c_void_p)
    rt.capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(cam), w, h, vptr(pts)), "rt_primary_points")
    centre = np.array(list(cam.center), F)
    O = np.ascontiguousarray(np.broadcast_to(centre, (h * w, 3)))
    D = np.ascontiguousarray((pts.reshape(-1, 3) - centre).astype(F))
    col, face, t = np.zeros((h * w, 3), F), np.zeros(h * w, np.int32), np.zeros(h * w, F)
    rt.capi.check(lib, ctx.handle, lib.rt_trace_rays(ctx.handle, C.byref(L), 0, h * w, vptr(O), vptr(D), vptr(col), vptr(face), vptr(t)), "rt_trace_rays")
    face, t = face.reshape(h, w), t.reshape(h, w)
    assert np.array_equal(face[hit >= 0], hit[hit >= 0])
    assert same(g[hit >= 0][:, 1], t[hit >= 0])


# ------------------------------------------------------------------------------------------ 4b. more tiles than the grid holds
def strided_frame(sc):
    """(w, h, first frame row whose tiles all lie behind round 1, last frame row whose tiles all lie in it + 1) of a frame with at least a
    quarter of a grid's worth of tiles in round 2 on the context's device, round 2 starting in the middle of a tile row"""
    cus = gc.cu_count(sc.ctx.device)
    w, h = gc.gbuffer_frame(cus)
    tx, _, tiles = gc.gb_tiles(w, h)
    assert gc.strides(tiles, gc.gb_cap(cus)) and gc.gb_grid(tiles, cus) * gc.WAVES < tiles, (cus, w, h)
    assert gc.gb_cap(cus) % tx != 0 and (w % gc.GB_TILE != 0 or h % gc.GB_TILE != 0)
    return w, h, gc.gbuffer_round_two_row(w, cus), gc.GB_TILE * (gc.gb_cap(cus) // tx)


def one_ray_frame(sc, cam, w, h):
    """the buffers of the one-ray pinhole frame by the construction of test_one_ray_buffers_agree_with_the_frame, for every pixel: the raster
    points of rt_primary_points, the root-box pre-test by rt_box_intersect (as in ref_blur_pass), face and t of rt_trace_rays at depth 0, the
    eight floats by gbuffer_ref.sample_values"""
    rt, lib, ctx = sc.rt, sc.lib, sc.ctx
    N = w * h
    vptr = lambda x: x.ctypes.data_as(C.c_void_p)
    pts = np.zeros((N, 3), F)
    rt.capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(cam), w, h, vptr(pts)), "rt_primary_points")
    centre = np.array(list(cam.center), F)
    O = np.ascontiguousarray(np.broadcast_to(centre, (N, 3)))
    D = np.ascontiguousarray((pts - centre).astype(F))
    node0 = sc.hs.view.nodes[0]
    boxes = np.ascontiguousarray(np.broadcast_to(np.array(list(node0.bmin) + list(node0.bmax), F), (N, 6)))
    pre = np.zeros(N, np.uint8)
    rt.capi.check(lib, ctx.handle, lib.rt_box_intersect(ctx.handle, N, vptr(boxes), vptr(O), vptr(pts), vptr(pre)), "rt_box_intersect")
    L = gl.area_lights(rt, 5)
    col, face, t = np.zeros((N, 3), F), np.zeros(N, np.int32), np.zeros(N, F)
    rt.capi.check(lib, ctx.handle, lib.rt_trace_rays(ctx.handle, C.byref(L), 0, N, vptr(O), vptr(D), vptr(col), vptr(face), vptr(t)), "rt_trace_rays")
    face[pre == 0] = -1
    return gr.sample_values(face.reshape(h, w), t.reshape(h, w), sc.fn, sc.kd)


@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_pinhole_frame_beyond_the_grid(world, name):
    """k_gbuffer in its second round, every pixel: waves take tiles of another tile column and row, with their LDS stacks used again"""
    sc = world[name]
    w, h, row2, row1 = strided_frame(sc)
    sc.settings()
    cam = sc.rt.default_camera(w, h, YAW)
    got = call(sc, cam, sc.rt.make_params(w, h))
    for part in (got[:row1], got[row2:]):
        full, empty, partly = gr.coverage(part)
        assert full > 0 and empty > 0 and partly == 0, "covered and empty pixels in the first round and behind it"
    want = one_ray_frame(sc, cam, w, h)
    print(f"{name} {w}x{h}: {differing(got, want)} pixels differ, coverage {gr.coverage(got)}")
    assert same(got, want), differing(got, want)


@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_pinhole_frame_beyond_the_grid_equals_the_cpu_frame(world, name):
    """the same call against the CPU frame over the oracle, on every 7th row and the last one"""
    sc = world[name]
    w, h, row2, _ = strided_frame(sc)
    sc.settings()
    got = gbuffer(sc, w, h)
    rows = sorted(set(range(0, h, 7)) | {h - 1})
    cpu = gr.cpu_pass(sc.orc, sc.osc, sc.orc.camera(w, h, YAW), w, h, 1, 0, rows=rows)
    assert same(got[rows], cpu), differing(got[rows], cpu)
    assert gr.coverage(cpu[np.array(rows) >= row2])[0] > 0


def test_blur_frame_beyond_the_grid(world):
    """the lens and the shutter on, two sub-samples a side and two passes: the strided tiles keep their pass and frame accumulators apart"""
    sc = world["dodge"]
    w, h, row2, row1 = strided_frame(sc)
    a, b = blur_cameras(sc.rt, w, h)
    rng = np.random.default_rng(24)
    rows = np.sort(np.concatenate([rng.choice(row1, 16, replace=False), row2 + rng.choice(h - row2, 8, replace=False)]))
    assert len(rows) == 24 and int((rows >= row2).sum()) >= 8
    sc.settings(2, (1, 2), LENS, b)
    try:
        got = call(sc, a, sc.rt.make_params(w, h))
        want = ref_blur_frame(sc, a, b, w, h, 2, (1, 2), LENS, rows=rows)
    finally:
        sc.settings()
    print(f"dodge {w}x{h} rows {rows.tolist()}: {differing(got[rows], want)} pixels differ, coverage {gr.coverage(want)}")
    assert same(got[rows], want), differing(got[rows], want)
    for part in (want[rows < row1], want[rows >= row2]):
        full, empty, partly = gr.coverage(part)
        assert full > 0 and empty > 0 and partly > 0


# ------------------------------------------------------------------------------------------ 5. rows and shards
@pytest.mark.parametrize("mode", ["pinhole", "both"])
def test_row_ranges_and_shards_equal_the_full_call(world, mode):
    sc = world["dodge"]
    rt = sc.rt
    w, h = SIZES[0]
    a, b = blur_cameras(rt, w, h)
    sc.settings(3, (5, 2), LENS if mode == "both" else None, b if mode == "both" else None)
    full = call(sc, a, rt.make_params(w, h))
    assert gr.coverage(full)[2] > 0
    part = call(sc, a, rt.make_params(w, h, row0=5, row1=14))
    assert part.shape == (9, w, 8) and same(part, full[5:14])
    for rank in (0, 1):
        rows = [y for y in range(h) if (y // 2) % 2 == rank]
        got = call(sc, a, rt.make_params(w, h, stripe=2, rank=rank, nranks=2))
        assert got.shape == (len(rows), w, 8) and same(got, full[rows]), rank
    rows = [y for y in range(3, 20) if ((y - 3) // 3) % 2 == 1]
    assert same(call(sc, a, rt.make_params(w, h, row0=3, row1=20, stripe=3, rank=1, nranks=2)), full[rows])
    if mode == "both":                                 # and the reference itself, on rows that do not start at 0
        assert same(part, ref_blur_frame(sc, a, b, w, h, 3, (5, 2), LENS, rows=range(5, 14)))
    # an empty row range: nothing to do
    o = Out(rt, 8)
    p = rt.make_params(w, h, row0=7, row1=7)
    assert sc.lib.rt_gbuffer_device(sc.ctx.handle, C.byref(a), C.byref(p), o.ptr, None) == rt.capi.RT_OK
    sc.ctx.synchronize()
    assert o.untouched()
    o.free()


# ------------------------------------------------------------------------------------------ 6. guards
def test_refusals_write_nothing(rt, world):
    sc = world["cube"]
    lib, h_ = sc.lib, sc.ctx.handle
    inv, w, h = rt.capi.RT_ERR_INVALID, 37, 21
    cam, p = rt.default_camera(w, h, YAW), rt.make_params(w, h)
    o = Out(rt, w * h * 8)
    host = np.full(w * h * 8, 7.0, F)
    hptr = C.c_void_p(host.ctypes.data)
    sc.settings()

    def both(handle, cam_, p_, dev=o.ptr, hst=hptr):
        return [lib.rt_gbuffer_device(handle, cam_, p_, dev, None), lib.rt_gbuffer(handle, cam_, p_, hst)]

    def named():
        return b"rt_gbuffer" in lib.rt_last_error(h_)

    # NULL arguments; an output that is not 16-byte aligned (the device call only)
    assert both(h_, None, C.byref(p)) == [inv, inv] and named()
    assert both(h_, C.byref(cam), None) == [inv, inv] and named()
    assert both(h_, C.byref(cam), C.byref(p), None, None) == [inv, inv] and named()
    for off in (4, 8, 12):
        assert lib.rt_gbuffer_device(h_, C.byref(cam), C.byref(p), C.c_void_p(o.ptr.value + off), None) == inv
    assert b"rt_gbuffer_device" in lib.rt_last_error(h_) and b"aligned" in lib.rt_last_error(h_)
    # the checks of a frame's params
    for bad in (rt.make_params(0, h), rt.make_params(w, -1), rt.make_params(w, h, row0=5, row1=4), rt.make_params(w, h, row1=h + 1),
                rt.make_params(w, h, stripe=0), rt.make_params(w, h, rank=2, nranks=2)):
        assert both(h_, C.byref(cam), C.byref(bad)) == [inv, inv] and named()
    # a frame of sub-samples that is too large
    sc.settings(4)
    big = rt.make_params(1 << 30, 4, row1=1)
    assert both(h_, C.byref(cam), C.byref(big)) == [rt.capi.RT_ERR_UNSUPPORTED] * 2 and named()
    sc.settings()
    # before rt_upload_scene
    empty = rt.Context(0)
    try:
        assert both(empty.handle, C.byref(cam), C.byref(p)) == [rt.capi.RT_ERR_NO_SCENE] * 2
        assert b"rt_gbuffer" in lib.rt_last_error(empty.handle)
    finally:
        empty.close()
    # adaptive pass counts ON; OFF again when count <= min_passes or tol < 0
    sc.ctx.set_passes(0, 9)
    sc.ctx.set_pass_tolerance(0.01, 8)
    assert both(h_, C.byref(cam), C.byref(p)) == [inv, inv] and named() and b"rt_set_pass_tolerance" in lib.rt_last_error(h_)
    sc.ctx.set_passes(0, 8)
    assert lib.rt_gbuffer(h_, C.byref(cam), C.byref(p), hptr) == rt.capi.RT_OK
    host[:] = 7.0
    sc.settings()
    # a close camera whose perspective differs
    close = rt.default_camera(w, h, YAW + 0.05)
    close.fovy = 45.0
    sc.ctx.set_shutter(close)
    assert both(h_, C.byref(cam), C.byref(p)) == [inv, inv] and named()
    sc.ctx.set_shutter(None)
    sc.ctx.synchronize()
    assert o.untouched() and (host == 7.0).all()
    # and the valid call between the same guards writes exactly rows * W * 8 floats
    assert lib.rt_gbuffer_device(h_, C.byref(cam), C.byref(p), o.ptr, None) == rt.capi.RT_OK
    sc.ctx.synchronize()
    assert same(o.read((h, w, 8)), sc.cpu_frame(w, h, 1, 0, 1))
    assert lib.rt_gbuffer(h_, C.byref(cam), C.byref(p), hptr) == rt.capi.RT_OK
    assert same(host.reshape(h, w, 8), sc.cpu_frame(w, h, 1, 0, 1))
    o.free()


# ------------------------------------------------------------------------------------------ 7. the context afterwards
def frame(sc, w, h, n=1, tau=-1.0, depth=3):
    sc.settings(n, tau=tau)
    st = sc.rt.capi.rt_stats()
    cam, L = sc.rt.default_camera(w, h, YAW), gl.area_lights(sc.rt, 5)
    rgb, _, st = gl.render(sc.rt, sc.ctx, cam, L, w, h, depth)
    return rgb, gl.counters(st), int(st.launches_total)


def test_refined_count_and_later_frames_survive_a_call(world):
    sc = world["cube"]
    w, h = 64, 40
    before = frame(sc, w, h)
    adaptive = frame(sc, w, h, 2, 0.05)
    want = sc.ctx.supersampling_refined()
    assert 0 < want < w * h
    frame(sc, w, h, 2, 0.05)
    g = gbuffer(sc, w, h)                              # (n = 2, the threshold ignored: the regular frame)
    assert same(g, sc.cpu_frame(w, h, 2, 0, 1))
    assert sc.ctx.supersampling_refined() == want
    again = frame(sc, w, h, 2, 0.05)
    assert same(again[0], adaptive[0]) and again[1:] == adaptive[1:]
    after = frame(sc, w, h)
    assert same(after[0], before[0]) and after[1:] == before[1:]


def test_a_call_on_a_second_stream_beside_a_frame(rt, world):
    sc = world["dodge"]
    hip = rt.hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    w, h = 96, 64
    try:
        a, b = blur_cameras(rt, w, h)
        sc.settings(2, (1, 2), LENS, b)
        p = rt.make_params(w, h, 3)
        L = gl.area_lights(rt, 5)
        solo_g = call(sc, a, p)
        solo_rgb, _ = gl.render_device(rt, sc.ctx, a, L, w, h, 3)
        rgb = Out(rt, w * h * 3)
        rt.capi.check(sc.lib, sc.ctx.handle, sc.lib.rt_render_device(sc.ctx.handle, C.byref(a), C.byref(L), C.byref(p), rgb.ptr, None, None, None, None),
                      "rt_render_device")
        o = call(sc, a, p, stream=stream, sync=False)
        assert hip.hipStreamSynchronize(stream) == 0
        sc.ctx.synchronize()
        assert same(o.read((h, w, 8)), solo_g)
        assert same(rgb.read((h, w, 3)), solo_rgb)
        o.free(); rgb.free()
    finally:
        hip.hipStreamDestroy(stream)


# ------------------------------------------------------------------------------------------ 8. path switches and the counting build
def in_process(world):
    """what tests/gbuffer_child.py computes, here"""
    out = {}
    for name in ("cube", "dodge"):
        for key, g in gbuffer_child.buffers(world[name].rt, world[name].ctx).items():
            out[FILES[name] + ":" + key] = g
    return out


@pytest.mark.parametrize("switch", ["RT_NO_CULL", "RT_NO_PLANE_CULL", "RT_NO_SHAFT", "RT_STAGED_TRACE"])
def test_result_is_unchanged_under_the_path_switches(world, scenes, tmp_path, switch):
    want = in_process(world)
    env = dict(os.environ)
    env[switch] = "0" if switch == "RT_STAGED_TRACE" else "1"
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "gbuffer_child.py"), out] + [os.path.join(scenes, FILES[k]) for k in ("cube", "dodge")],
                       env=env, capture_output=True, timeout=240)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = np.load(out)
    assert sorted(got.files) == sorted(want)
    for k in want:
        assert same(got[k], want[k]), (switch, k, differing(got[k], want[k]))
        assert gr.coverage(got[k])[0] > 0


def test_counting_build_gives_the_same_buffers(rt, world):
    want = in_process(world)
    lib = rt.capi.load_library(WORK_LIB)
    for name in ("cube", "dodge"):
        ctx = C.c_void_p()
        assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
        try:
            rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(world[name].hs.view)), "rt_upload_scene")
            got = gbuffer_child.buffers(rt, ctx, lib)
        finally:
            lib.rt_destroy(ctx)
        for key, g in got.items():
            assert same(g, want[FILES[name] + ":" + key]), (name, key)


# ------------------------------------------------------------------------------------------ 9. front ends
def test_torch_tensor_on_a_second_stream_and_device_buffer(world):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no device"
    sc = world["dodge"]
    w, h = SIZES[0]
    cam = sc.rt.default_camera(w, h, YAW)
    sc.settings(2, (1, 3))
    want = sc.cpu_frame(w, h, 2, 1, 3)
    dev = f"cuda:{sc.ctx.device}"
    t = sc.ctx.gbuffer(cam, w, h)                                   # torch's current (default) stream
    assert t.dtype == torch.float32 and tuple(t.shape) == (h, w, 8) and str(t.device) == dev
    assert same(t.cpu().numpy(), want)
    s = torch.cuda.Stream(device=dev)
    canary = torch.full((h * w * 8 + 2 * GUARD,), 3.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        view = canary[GUARD:GUARD + h * w * 8]
        back = sc.ctx.gbuffer(cam, w, h, out=view)
        rows = sc.ctx.gbuffer(cam, w, h, rows=(5, 14))
    s.synchronize()
    assert back is view and same(view.cpu().numpy().reshape(h, w, 8), want)
    assert (canary[:GUARD] == 3.0).all() and (canary[-GUARD:] == 3.0).all()
    assert tuple(rows.shape) == (9, w, 8) and same(rows.cpu().numpy(), want[5:14])
    buf = sc.rt.hipmem.DeviceBuffer(h * w * 8 * 4)
    assert sc.ctx.gbuffer(cam, w, h, out=buf) is buf
    sc.ctx.synchronize()
    assert same(buf.to_numpy(F, (h, w, 8)), want)
    buf.free()
    for bad in (torch.zeros((h, w, 8), dtype=torch.float64, device=dev), torch.zeros((h, w, 7), dtype=torch.float32, device=dev),
                torch.zeros((h, w, 8), dtype=torch.float32)):
        with pytest.raises(ValueError):
            sc.ctx.gbuffer(cam, w, h, out=bad)
    with pytest.raises(ValueError):
        sc.ctx.gbuffer(cam, w, h, out=sc.rt.hipmem.DeviceBuffer(64))


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n"
        w, h = (int(x) for x in f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)[::-1]


def test_flyscene_member_and_the_cli_files(rt, scenes, tmp_path):
    w, h = SIZES[0]
    path = os.path.join(scenes, FILES["dodge"])
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(w, h, True, False)
    try:
        fs.supersample, fs.passes = 2, 2
        g = fs.gbuffer(w, h)
        assert g.shape == (h, w, 8) and g.dtype == np.float32
        lib = fs.ctx.lib
        for st in (lib.rt_set_supersampling(fs.ctx.handle, 2), lib.rt_set_passes(fs.ctx.handle, 0, 2)):
            assert st == 0
        direct = np.zeros((h, w, 8), F)
        p = rt.make_params(w, h)
        rt.capi.check(lib, fs.ctx.handle, lib.rt_gbuffer(fs.ctx.handle, C.byref(fs.camera), C.byref(p), direct.ctypes.data_as(C.c_void_p)), "rt_gbuffer")
        assert same(g, direct) and gr.coverage(g)[2] > 0
    finally:
        fs.ctx.close()
        fs.scene.close()
    r = subprocess.run([RT_RENDER, "--scene", path, "--size", str(w), str(h), "--samples", "2", "2", "--depth", "1", "--aa", "2", "--passes", "2",
                        "--gbuffer", "gb", "--out", "result.ppm"], input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=240)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    geom, normal, albedo = (read_pfm(str(tmp_path / f"gb.{k}.pfm")) for k in ("geom", "normal", "albedo"))
    assert same(geom[..., :2], g[..., :2]) and (bits(geom[..., 2]) == 0).all()
    assert same(normal, g[..., 2:5]) and same(albedo, g[..., 5:8])
    assert os.path.exists(str(tmp_path / "result.ppm"))
