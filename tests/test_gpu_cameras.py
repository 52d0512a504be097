"""Frames of general cameras on the device, against the CPU oracle.  Tolerance 0 throughout.

Every other frame test renders through yaw cameras, whose inv_view has four exact zeros and a one: the sums of the primary-ray generator
never run as written, and the camera's position never leaves the routes the yaw sweep reaches.  Here the camera set of
tests/camera_cases.py (pitched and translated fly cameras pinned against the reference, a camera inside the root box, one facing away,
the model in the last partial tile, one face over the whole frame, and cameras only the ABI can express: sheared, mirrored, other fields
of view, an aspect that is not w / h, a shifted viewport) renders three scenes -- cube.obj (the flat path), the mixed-material scene
(bounces, depth 4) and dodgeColorTest.obj (the staged trace, the pair beams and the shaft walk; once more under a 16 x 16 light) -- and
float RGB, level-0 hit ids, ray counters and the 8-bit image must equal the oracle's, with primary culling on and off, through graph
replays (the camera block read from device memory) and through row shards.  tests/test_camera_cases.py shows without a device that the
set is not vacuous.  The sampling features run one general camera each against the restatements their own files use.
"""
import numpy as np
import pytest

import camera_cases as cc
import gbuffer_ref as gr
import passes_ref
import switch_table
import test_gpu_gbuffer as gg
import test_gpu_lens as gl
import test_gpu_passes as gp
import test_gpu_primary_cull as gpc
import test_gpu_shutter as gs
import test_gpu_supersample as gss

F = np.float32
DEPTH = 4
CONFIGS = {"cube": ("cube.obj", 8), "mixed": ("mixed", 8), "dodge": ("dodgeColorTest.obj", 8), "dodge16": ("dodgeColorTest.obj", 16)}
ORACLE_COUNTERS = ("rays_primary", "rays_bounce", "rays_centre", "rays_sample", "pixels_culled", "shaded_hits")
bits_equal, diff, quantise_u8 = gl.bits_equal, gl.diff, gl.quantise_u8
# the cameras a graph replays (three general ones and a yaw camera: the captured kernels read each from the device's camera block) and
# the two whose frames are stitched from row shards
GRAPH_CAMERAS = ("fly3", "sheared", "mirrored")
GRAPH_YAW = 0.55
SHARD_CAMERAS = ("fly4", "vporigin")


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def sizes_of(name):
    return ((61, 45),) if name == "corner" else cc.SIZES


class World:
    """one scene on the device and in the oracle, its lights on both sides, and the oracle's frames, rendered once per (camera, size)"""

    def __init__(self, rt, oracle, key, tmp):
        self.rt, self.oracle, self.key = rt, oracle, key
        scene, grid = CONFIGS[key]
        path = cc.scene_path(scene, tmp)
        self.hs, self.ctx = gl.open_ctx(rt, path)
        self.osc = oracle.load_scene(path)
        self.box = list(self.hs.info()["root_box"])
        self.L = rt.make_lights(points=gl.THREE[:1], area=True, usteps=grid, vsteps=grid)
        self.oL = oracle.lights(area=True, usteps=grid, vsteps=grid, points=gl.THREE[:1])
        self.frames = {}

    def cameras(self, name, w, h):
        if isinstance(name, float):
            return self.rt.default_camera(w, h, name), self.oracle.camera(w, h, name)
        return cc.pair(self.rt, self.oracle, name, w, h, self.box, self.osc)

    def expected(self, name, w, h):
        """(rgb, hit ids, counters) of the oracle"""
        if (name, w, h) not in self.frames:
            rgb, hits, st = self.osc.render(self.cameras(name, w, h)[1], self.oL, w, h, max_depth=DEPTH, threads=8, want_hits=True)
            cnt = {k: int(getattr(st, k)) for k in ORACLE_COUNTERS if k != "pixels_culled"}
            cnt["pixels_culled"] = int(st.precull_tests - st.rays_primary)
            for a in (rgb, hits):
                a.setflags(write=False)
            self.frames[(name, w, h)] = (rgb, hits, cnt)
        return self.frames[(name, w, h)]

    def close(self):
        self.ctx.close(); self.hs.close(); self.osc.close()


@pytest.fixture(scope="module")
def worlds(rt, oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cameras")
    made = {}

    def get(key):
        if key not in made:
            made[key] = World(rt, oracle, key, tmp)
        return made[key]
    yield get
    for w in made.values():
        w.close()


def assert_equals_oracle(got, want, what):
    """got: the six of test_gpu_primary_cull.frame; want: World.expected"""
    rgb, hits, cnt = want
    assert bits_equal(got[0], rgb), (what, "rt_render rgb", diff(got[0], rgb))
    assert np.array_equal(got[1], hits), (what, "level-0 hit ids", int((got[1] != hits).sum()))
    assert bits_equal(got[3], rgb), (what, "rt_render_device rgb", diff(got[3], rgb))
    assert np.array_equal(got[4], quantise_u8(rgb)), (what, "8-bit")
    for st in (got[2], got[5]):
        assert {k: st[k] for k in ORACLE_COUNTERS} == cnt, (what, {k: st[k] for k in ORACLE_COUNTERS}, cnt)


# ------------------------------------------------------------------------------------------ 1. eager frames, culling on and off
@pytest.mark.gpu
@pytest.mark.parametrize("name", cc.NAMES)
@pytest.mark.parametrize("key", list(CONFIGS))
def test_frame_equals_the_oracle_with_culling_on_and_off(rt, worlds, key, name):
    wd = worlds(key)
    ctx = wd.ctx
    try:
        for (w, h) in sizes_of(name):
            cam, _ = wd.cameras(name, w, h)
            want = wd.expected(name, w, h)
            ctx.set_primary_cull(True)
            on = gpc.frame(rt, ctx, cam, wd.L, w, h, DEPTH)
            ctx.set_primary_cull(False)
            off = gpc.frame(rt, ctx, cam, wd.L, w, h, DEPTH)
            print(f"{key} {name} {w}x{h}: {float((want[1] >= 0).mean()):.3f} of the pixels hit, {want[2]}; differs from the oracle in "
                  f"{diff(on[0], want[0])} pixels")
            assert_equals_oracle(on, want, (key, name, w, h, "culling on"))
            assert_equals_oracle(off, want, (key, name, w, h, "culling off"))
            gpc.same(on, off, (key, name, w, h))
            rect = rt.primary_rect(cam, wd.box, w, h)
            if name == "away":
                assert on[2]["pixels_culled"] == off[2]["pixels_culled"] == w * h and on[2]["rays_primary"] == 0
            elif name == "corner":
                tx, ty = (w + 7) // 8, (h + 7) // 8
                assert rect != gpc.pc.whole(w, h) and rect[2] > rect[0] >= tx - 2 and rect[3] > rect[1] >= ty - 2, rect       # the window path runs
                assert (want[1] >= 0).any()
            elif name == "inside":
                assert rect == gpc.pc.whole(w, h) and (want[1] >= 0).any() and on[2]["pixels_culled"] == 0
            elif name == "closeup":
                assert (want[1] >= 0).all() and np.unique(want[1]).size == 1
            else:
                assert 0.10 <= float((want[1] >= 0).mean()) <= 0.90
    finally:
        ctx.set_primary_cull(True)


# ------------------------------------------------------------------------------------------ 2. graph replays
@pytest.mark.gpu
@pytest.mark.parametrize("key", list(CONFIGS))
def test_one_graph_replays_general_and_yaw_cameras(rt, worlds, key):
    """the graph is created once; every replay takes its camera from the block rt_graph_launch uploads"""
    wd = worlds(key)
    ctx = wd.ctx
    w, h = 61, 45
    out, out8 = rt.hipmem.DeviceBuffer(h * w * 3 * 4), rt.hipmem.DeviceBuffer(h * w * 3)
    ctx.set_primary_cull(True)
    g = rt.FrameGraph(ctx, wd.L, rt.make_params(w, h, DEPTH), out.address, out8.address)
    try:
        order = GRAPH_CAMERAS[:2] + (GRAPH_YAW,) + GRAPH_CAMERAS[2:] + GRAPH_CAMERAS[:1]
        got = []
        for name in order:
            g.launch(wd.cameras(name, w, h)[0])
            gst = gpc.stats(g.stats())                                          # rt_graph_stats synchronises: the launch is asynchronous
            got.append((out.to_numpy(F, (h, w, 3)), out8.to_numpy(np.uint8, (h, w, 3)), gst))
        for name, (rgb, u8, gst) in zip(order, got):
            want = wd.expected(name, w, h)
            st = rt.capi.rt_stats()
            eager, eager8 = gl.render_device(rt, ctx, wd.cameras(name, w, h)[0], wd.L, w, h, DEPTH, stats=st)
            assert bits_equal(rgb, eager) and np.array_equal(u8, eager8), (key, name, "replay against the eager frame", diff(rgb, eager))
            assert bits_equal(rgb, want[0]) and np.array_equal(u8, quantise_u8(want[0])), (key, name, "replay against the oracle", diff(rgb, want[0]))
            assert {k: gst[k] for k in ORACLE_COUNTERS} == want[2] == {k: gpc.stats(st)[k] for k in ORACLE_COUNTERS}, (key, name)
        assert len({r[0].tobytes() for r in got[:4]}) == 4, "four cameras, four frames"
    finally:
        g.close(); out.free(); out8.free()


# ------------------------------------------------------------------------------------------ 3. row shards
@pytest.mark.gpu
@pytest.mark.parametrize("key", list(CONFIGS))
def test_two_ranks_of_a_stripe_four_shard_stitch_to_the_frame(rt, worlds, key):
    wd = worlds(key)
    w, h = 61, 45
    for name in SHARD_CAMERAS:
        cam, _ = wd.cameras(name, w, h)
        want = wd.expected(name, w, h)
        rgb, hits, u8 = np.full((h, w, 3), np.nan, F), np.full((h, w), -7, np.int32), np.zeros((h, w, 3), np.uint8)
        total = {k: 0 for k in ORACLE_COUNTERS}
        for rank in range(2):
            ys = gpc.pc.shard_rows(h, 4, 2, rank)
            part = gpc.frame(rt, wd.ctx, cam, wd.L, w, h, DEPTH, stripe=4, rank=rank, nranks=2)
            assert bits_equal(part[0], part[3])
            rgb[ys], hits[ys], u8[ys] = part[0], part[1], part[4]
            for k in ORACLE_COUNTERS:
                total[k] += part[2][k]
        assert bits_equal(rgb, want[0]), (key, name, diff(rgb, want[0]))
        assert np.array_equal(hits, want[1]) and np.array_equal(u8, quantise_u8(want[0])), (key, name)
        assert total == want[2], (key, name, total, want[2])


# ------------------------------------------------------------------------------------------ 4. the sampling features, one general camera each
def fly_pair(wd, w, h):
    """two fly cameras that differ in pitch and translation, close enough for a shutter"""
    a = wd.oracle.fly_camera(w, h, 0.6, 0.35, (-0.8, 0.63, 0.84))
    b = wd.oracle.fly_camera(w, h, 0.6, 0.42, (-0.76, 0.66, 0.8))
    return cc.rt_camera(wd.rt, a), cc.rt_camera(wd.rt, b)


def reset(ctx):
    gp.set_frame(ctx)
    ctx.set_primary_cull(True)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["cube", "mixed", "dodge"])
def test_supersampling_equals_the_oracle_with_shifted_viewports(rt, worlds, key):
    wd = worlds(key)
    w, h, n = 61, 45, 2
    cam, ocam = wd.cameras("fly2", w, h)
    try:
        wd.ctx.set_supersampling(n)
        rgb, u8 = gl.render_device(rt, wd.ctx, cam, wd.L, w, h, DEPTH)
        subs = [wd.osc.render(gss.shifted(cc.ocamera_of(cam), n, sx, sy), wd.oL, w, h, max_depth=DEPTH, threads=8)[0] for sy in range(n) for sx in range(n)]
        want = gss.box(subs, n)
        assert bytes(ocam) == bytes(cam)
        assert bits_equal(rgb, want), (key, diff(rgb, want))
        assert np.array_equal(u8, quantise_u8(want))
        assert not bits_equal(subs[0], subs[3])
    finally:
        reset(wd.ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["cube", "dodge"])
def test_lens_equals_the_fold_of_the_reference_rays(rt, worlds, key):
    wd = worlds(key)
    w, h, n = 61, 45, 2
    cam, _ = wd.cameras("fly1", w, h)
    try:
        want, culled = gl.gpu_lens_frame(rt, wd.ctx, wd.hs, cam, wd.L, w, h, n, DEPTH, gl.AP, 1.6)
        wd.ctx.set_supersampling(n)
        pin, _ = gl.render_device(rt, wd.ctx, cam, wd.L, w, h, DEPTH)
        wd.ctx.set_lens(gl.AP, 1.6)
        st = rt.capi.rt_stats()
        rgb, u8 = gl.render_device(rt, wd.ctx, cam, wd.L, w, h, DEPTH, stats=st)
        assert bits_equal(rgb, want), (key, diff(rgb, want))
        assert np.array_equal(u8, quantise_u8(want)) and int(st.pixels_culled) == culled
        assert not bits_equal(rgb, pin), "the lens must change the frame"
    finally:
        reset(wd.ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["cube", "dodge"])
def test_shutter_between_two_fly_cameras_equals_the_fold_of_the_reference_rays(rt, worlds, key):
    wd = worlds(key)
    w, h, n = 61, 45, 2
    a, b = fly_pair(wd, w, h)
    try:
        want, culled, _ = gs.gpu_shutter_frame(rt, wd.ctx, wd.hs, a, b, wd.L, w, h, n, DEPTH)
        wd.ctx.set_supersampling(n)
        still, _ = gl.render_device(rt, wd.ctx, a, wd.L, w, h, DEPTH)
        wd.ctx.set_shutter(b)
        st = rt.capi.rt_stats()
        rgb, u8 = gl.render_device(rt, wd.ctx, a, wd.L, w, h, DEPTH, stats=st)
        assert bits_equal(rgb, want), (key, diff(rgb, want))
        assert np.array_equal(u8, quantise_u8(want)) and int(st.pixels_culled) == culled
        assert not bits_equal(rgb, still), "the shutter must change the frame"
    finally:
        reset(wd.ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["cube", "dodge"])
def test_two_passes_equal_the_fold_of_the_reference_passes(rt, worlds, key):
    wd = worlds(key)
    w, h = 61, 45
    cam, _ = wd.cameras("fly4", w, h)
    try:
        p0 = wd.expected("fly4", w, h)[0]                                   # pass 0 of a plain frame is the plain frame: the oracle's
        p1, _, _ = gp.ref_pass_frame(rt, wd.ctx, wd.hs, cam, None, wd.L, w, h, 1, 1, DEPTH, None)
        want = passes_ref.fold_passes([p0, p1])
        gp.set_frame(wd.ctx, passes=(0, 2))
        rgb, u8 = gl.render_device(rt, wd.ctx, cam, wd.L, w, h, DEPTH)
        host, _, _ = gl.render(rt, wd.ctx, cam, wd.L, w, h, DEPTH)
        assert bits_equal(rgb, want), (key, diff(rgb, want))
        assert bits_equal(host, want) and np.array_equal(u8, quantise_u8(want))
        assert not bits_equal(p0, p1)
    finally:
        reset(wd.ctx)


class GScene:
    """what test_gpu_gbuffer.call and one_ray_frame take"""

    def __init__(self, wd):
        self.rt, self.lib, self.ctx, self.hs = wd.rt, wd.ctx.lib, wd.ctx, wd.hs
        self.fn = wd.osc.arrays()["face_normal"]
        self.kd = gr.face_kd(wd.osc)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["cube", "mixed", "dodge"])
def test_gbuffer_of_the_one_ray_frame(rt, oracle, worlds, key):
    wd = worlds(key)
    w, h = 61, 45
    sc = GScene(wd)
    cam, ocam = wd.cameras("fly5", w, h)
    reset(wd.ctx)
    got = gg.call(sc, cam, rt.make_params(w, h))
    want = gr.cpu_pass(oracle, wd.osc, ocam, w, h, 1, 0)
    assert gg.same(got, want), (key, "the CPU pass", gg.differing(got, want))
    assert gg.same(got, gg.one_ray_frame(sc, cam, w, h)), (key, "the one-ray frame")
    hits = wd.expected("fly5", w, h)[1]
    assert ((got[..., 0] == 1.0) == (hits >= 0)).all() and 0.1 < float((hits >= 0).mean()) < 0.9
