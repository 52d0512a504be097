"""Primary culling (rt_set_primary_cull) on the device: culling on and off must agree bit for bit -- float RGB, 8-bit output, hit ids and
every counter of rt_stats -- for the cameras and frame shapes of tests/test_primary_cull.py, through eager frames, row shards, graph
replays and the other primary-ray paths, on a flat and on a tree scene.  Tolerance 0 everywhere.

(Primary frames have no `t` output: rt_render and rt_render_device return hit ids only, so those are what is compared.)
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import switch_table
import test_gpu_lens as gl
import test_primary_cull as pc

SCENES = pc.SCENES
WORK_LIB = gl.WORK_LIB
F = np.float32
bits_equal, diff, open_ctx, render, render_device, area_lights = gl.bits_equal, gl.diff, gl.open_ctx, gl.render, gl.render_device, gl.area_lights
# every counter of rt_stats that is a function of the frame (the ms_* fields are times; rays_sample_walked follows the order in which the
# trace kernel's waves append their hits, see tests/test_gpu_passes.py)
STATS = ("rays_primary", "rays_bounce", "rays_centre", "rays_sample", "pixels", "pixels_culled", "shaded_hits", "box_tests", "leaf_tri_refs",
         "box_tests_shadow", "leaf_tri_refs_shadow", "launches_trace", "launches_shadow", "launches_shade", "launches_total")


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def stats(st):
    return {k: int(getattr(st, k)) for k in STATS}


def frame(rt, ctx, cam, L, w, h, depth, **shard):
    """one view through both eager entry points: (rgb, hit ids, stats of rt_render | rgb, 8-bit, stats of rt_render_device)"""
    p = rt.make_params(w, h, depth, shard.get("row0", 0), shard.get("row1", h), shard.get("stripe", 1), shard.get("rank", 0), shard.get("nranks", 1))
    rows = ctx.lib.rt_local_rows(C.byref(p))
    rgb = np.full((rows, w, 3), np.nan, F)
    hit = np.full((rows, w), -7, np.int32)
    st = rt.capi.rt_stats()
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p),
                                                         hit.ctypes.data_as(C.c_void_p), C.byref(st)), "rt_render")
    st2 = rt.capi.rt_stats()
    rgb2, u8 = render_device(rt, ctx, cam, L, w, h, depth, stats=st2, **shard)
    return rgb, hit, stats(st), rgb2, u8, stats(st2)


def same(a, b, what):
    assert bits_equal(a[0], b[0]), (what, "rt_render rgb", diff(a[0], b[0]))
    assert np.array_equal(a[1], b[1]), (what, "hit ids", int((a[1] != b[1]).sum()))
    assert a[2] == b[2], (what, "rt_render stats", a[2], b[2])
    assert bits_equal(a[3], b[3]), (what, "rt_render_device rgb", diff(a[3], b[3]))
    assert np.array_equal(a[4], b[4]), (what, "8-bit")
    assert a[5] == b[5], (what, "rt_render_device stats", a[5], b[5])
    assert bits_equal(a[0], a[3]), (what, "the two entry points")


# ------------------------------------------------------------------------------------------ 1. the camera and shape set
@pytest.mark.gpu
@pytest.mark.parametrize("name", pc.NAMES)
def test_on_and_off_agree_over_the_camera_and_shape_set(rt, name):
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    box = hs.info()["root_box"]
    L = area_lights(rt)
    culled_some = kept_all = False
    try:
        for (w, h) in pc.SHAPES:
            for yaw in pc.YAWS:
                cam = pc.camera(rt, w, h, yaw, box)
                ctx.set_primary_cull(True)
                on = frame(rt, ctx, cam, L, w, h, 4)
                ctx.set_primary_cull(False)
                off = frame(rt, ctx, cam, L, w, h, 4)
                same(on, off, (name, w, h, yaw))
                assert not np.isnan(on[0]).any() and (on[1] >= -1).all()
                assert on[2]["pixels_culled"] + on[2]["rays_primary"] == w * h
                rect = rt.primary_rect(cam, box, w, h)
                outside = pc.outside_mask(rect, w, h)
                assert (on[1][outside] == -1).all() and int(outside.sum()) <= on[2]["pixels_culled"]
                culled_some = culled_some or outside.mean() > 0.5
                kept_all = kept_all or not outside.any()
    finally:
        ctx.set_primary_cull(True)
        ctx.close(); hs.close()
    assert culled_some and kept_all


@pytest.mark.gpu
@pytest.mark.parametrize("name", pc.NAMES)
def test_on_and_off_agree_on_shards_and_row_ranges(rt, name):
    w, h = 101, 67
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    try:
        for yaw in (0.0, 0.55, 0.9, 2.0):
            cam = rt.default_camera(w, h, yaw)
            ctx.set_primary_cull(False)
            full = frame(rt, ctx, cam, L, w, h, 4)
            shards = [dict(stripe=s, rank=r, nranks=n) for (s, n) in pc.SPLITS + ((1, 2),) for r in range(n)] + [dict(row0=5, row1=h - 3), dict(row0=3, row1=h, stripe=8, rank=1, nranks=2)]
            for sh in shards:
                ys = pc.shard_rows(h, sh.get("stripe", 1), sh.get("nranks", 1), sh.get("rank", 0), sh.get("row0", 0), sh.get("row1", h))
                ctx.set_primary_cull(True)
                on = frame(rt, ctx, cam, L, w, h, 4, **sh)
                ctx.set_primary_cull(False)
                off = frame(rt, ctx, cam, L, w, h, 4, **sh)
                same(on, off, (name, yaw, sh))
                assert bits_equal(on[0], full[0][ys]) and np.array_equal(on[1], full[1][ys]) and np.array_equal(on[4], full[4][ys]), (name, yaw, sh)
    finally:
        ctx.set_primary_cull(True)
        ctx.close(); hs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,yaw", [("cube.obj", 640, 360, 0.0), ("cube.obj", 333, 190, 0.55), ("dodgeColorTest.obj", 480, 270, 0.2)])
def test_on_and_off_agree_on_larger_frames(rt, name, w, h, yaw):
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    cam = rt.default_camera(w, h, yaw)
    try:
        ctx.set_primary_cull(True)
        on = frame(rt, ctx, cam, L, w, h, 4)
        ctx.set_primary_cull(False)
        off = frame(rt, ctx, cam, L, w, h, 4)
    finally:
        ctx.close(); hs.close()
    same(on, off, (name, w, h, yaw))
    assert on[2]["pixels_culled"] > w * h // 3


# ------------------------------------------------------------------------------------------ 2. the other primary-ray paths
@pytest.mark.gpu
@pytest.mark.parametrize("name,env", [
    ("cube.obj", {"RT_TRACE_DYNAMIC": "1"}),
    ("cube.obj", {"RT_NO_DEEP": "1"}),
    ("cube.obj", {"RT_SHADOW_UNITS": "1"}),
    ("dodgeColorTest.obj", {"RT_STAGED_TRACE": "0"}),
    ("dodgeColorTest.obj", {"RT_STAGED_TRACE": "0", "RT_TRACE_DYNAMIC": "1"}),
    ("dodgeColorTest.obj", {"RT_TRACE_BUDGET": "0"}),
    ("dodgeColorTest.obj", {"RT_TRACE_BUDGET": "1"}),
])
def test_on_and_off_agree_under_the_path_switches(rt, monkeypatch, name, env):
    w, h = 200, 136
    L = area_lights(rt)
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    base = [frame(rt, ctx, rt.default_camera(w, h, yaw), L, w, h, 4) for yaw in (0.0, 0.7)]
    ctx.close()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = rt.Context(0)
    ctx.upload(hs)
    try:
        for k, yaw in enumerate((0.0, 0.7)):
            cam = rt.default_camera(w, h, yaw)
            ctx.set_primary_cull(True)
            on = frame(rt, ctx, cam, L, w, h, 4)
            ctx.set_primary_cull(False)
            off = frame(rt, ctx, cam, L, w, h, 4)
            same(on, off, (name, env, yaw))
            assert bits_equal(on[0], base[k][0]) and np.array_equal(on[1], base[k][1]) and np.array_equal(on[4], base[k][4])
    finally:
        ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 3. graphs
@pytest.mark.gpu
@pytest.mark.parametrize("name", pc.NAMES)
def test_graph_replays_compute_the_rectangle_of_each_camera(rt, name):
    w, h = 320, 200
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    box = hs.info()["root_box"]
    out, out8 = rt.hipmem.DeviceBuffer(h * w * 3 * 4), rt.hipmem.DeviceBuffer(h * w * 3)
    ctx.set_primary_cull(True)
    g = rt.FrameGraph(ctx, L, rt.make_params(w, h, 4), out.address, out8.address)
    ctx.set_primary_cull(False)                             # a setting changed after the capture does not change the graph's frames
    yaws = (0.0, 0.9, 0.2, 2.0, 0.55, 1.2, 0.0, math.pi, 0.7)
    got = []
    for yaw in yaws:
        g.launch(rt.default_camera(w, h, yaw))
        st = g.stats()
        got.append((out.to_numpy(F, (h, w, 3)), out8.to_numpy(np.uint8, (h, w, 3)), stats(st)))
    g.close()
    rects = set()
    try:
        for yaw, (rgb, u8, gst) in zip(yaws, got):
            st = rt.capi.rt_stats()
            want, want8 = render_device(rt, ctx, rt.default_camera(w, h, yaw), L, w, h, 4, stats=st)        # eager, culling off
            assert bits_equal(rgb, want), (yaw, diff(rgb, want))
            assert np.array_equal(u8, want8), yaw
            est = stats(st)
            for k in ("rays_primary", "rays_bounce", "rays_centre", "rays_sample", "pixels", "pixels_culled", "shaded_hits", "launches_total"):
                assert gst[k] == est[k], (yaw, k, gst[k], est[k])
            rects.add(rt.primary_rect(rt.default_camera(w, h, yaw), box, w, h))
    finally:
        ctx.close(); hs.close(); out.free(); out8.free()
    assert len(rects) >= 5, "the sweep must move the rectangle from replay to replay"


# ------------------------------------------------------------------------------------------ 4. the frames that cannot cull
@pytest.mark.gpu
@pytest.mark.parametrize("name", pc.NAMES)
def test_sampled_frames_fall_back_to_the_whole_frame(rt, name):
    w, h = 120, 72
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    box = hs.info()["root_box"]
    L = area_lights(rt)
    cam, close = rt.default_camera(w, h, 0.3), rt.default_camera(w, h, 0.4)
    settings = [dict(n=2), dict(n=1, lens=(0.05, 2.0)), dict(n=2, lens=(0.05, 2.0)), dict(n=1, close=close), dict(n=1, passes=(0, 3)), dict(n=1, passes=(2, 1)),
                dict(n=3, tau=0.05)]
    try:
        for s in settings:
            ctx.set_supersampling(s.get("n", 1)); ctx.set_supersampling_threshold(s.get("tau", -1.0)); ctx.set_lens(*s.get("lens", (0.0, 2.0)))
            ctx.set_shutter(s.get("close")); ctx.set_passes(*s.get("passes", (0, 1)))
            # the fallback engaged: the rectangle such a frame uploads is the whole frame
            assert rt.primary_rect(cam, box, w, h, supersampling=s.get("n", 1), aperture=s.get("lens", (0.0, 2.0))[0], shutter="close" in s,
                                   passes=s.get("passes", (0, 1))) == pc.whole(w, h), s
            res = []
            for on in (True, False):
                ctx.set_primary_cull(on)
                st = rt.capi.rt_stats()
                rgb, u8 = render_device(rt, ctx, cam, L, w, h, 4, stats=st)
                res.append((rgb, u8, stats(st)))
            assert bits_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2], s
        # back to the plain frame: it culls again and is still the frame it was
        ctx.set_supersampling(1); ctx.set_supersampling_threshold(-1.0); ctx.set_lens(0.0, 2.0); ctx.set_shutter(None); ctx.set_passes(0, 1)
        ctx.set_primary_cull(True)
        on = frame(rt, ctx, cam, L, w, h, 4)
        ctx.set_primary_cull(False)
        off = frame(rt, ctx, cam, L, w, h, 4)
        same(on, off, (name, "plain again"))
        # rt_trace_rays is not a primary frame: same colours whatever the setting, right behind a frame that left a small rectangle in the camera block
        fs_o = np.tile(np.array([[0.0, 0.0, 2.0]], F), (300, 1))
        fs_d = np.stack([np.linspace(-1.2, 1.2, 300), np.linspace(-0.7, 0.7, 300), np.full(300, -1.0)], axis=1).astype(F)
        cols = []
        for on_ in (True, False):
            ctx.set_primary_cull(on_)
            render_device(rt, ctx, rt.default_camera(w, h, 0.9), L, w, h, 4)
            out = np.full((300, 3), np.nan, F)
            face = np.full(300, -7, np.int32)
            t = np.full(300, np.nan, F)
            rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_trace_rays(ctx.handle, C.byref(L), 4, 300, fs_o.ctypes.data_as(C.c_void_p), fs_d.ctypes.data_as(C.c_void_p),
                                                                  out.ctypes.data_as(C.c_void_p), face.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)), "rt_trace_rays")
            cols.append((out, face, t))
        assert bits_equal(cols[0][0], cols[1][0]) and np.array_equal(cols[0][1], cols[1][1]) and bits_equal(cols[0][2], cols[1][2])
        assert (cols[0][1] >= 0).any() and (cols[0][1] < 0).any()
    finally:
        ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 5. the culled tiles are really skipped
@pytest.mark.gpu
def test_counting_build_visits_fewer_primary_tiles(rt):
    """step counter 13 of the counting build counts the units the trace kernels take from their queues: on the flat scene the queue of the
    primary launch runs over the rectangle's tiles only"""
    if not os.path.exists(WORK_LIB):
        pytest.fail("librt_mi355x_work.so is not built")
    w, h = 320, 200
    lib = rt.capi.load_library(WORK_LIB)
    hs = rt.HostScene(os.path.join(SCENES, "cube.obj"), 1000, 15)
    box = hs.info()["root_box"]
    L = area_lights(rt)
    cam = rt.default_camera(w, h, 0.0)
    p = rt.make_params(w, h, 4)
    ctx = C.c_void_p()
    assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
    units, frames = [], []
    try:
        rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(hs.view)), "rt_upload_scene")
        for on in (1, 0):
            assert lib.rt_set_primary_cull(ctx, on) == rt.capi.RT_OK
            rgb = np.full((h, w, 3), np.nan, F)
            st = rt.capi.rt_stats()
            rt.capi.check(lib, ctx, lib.rt_render(ctx, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), None, C.byref(st)), "rt_render")
            work = (C.c_uint64 * 768)()
            rt.capi.check(lib, ctx, lib.rt_debug_work_counters(ctx, work, 768), "rt_debug_work_counters")
            units.append(int(work[13]))
            frames.append((rgb, stats(st)))
    finally:
        lib.rt_destroy(ctx)
        hs.close()
    rect = rt.primary_rect(cam, box, w, h)
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    kept = (rect[2] - rect[0]) * (rect[3] - rect[1])
    print(f"trace units with culling on {units[0]}, off {units[1]}; the frame has {tiles} primary tiles, the rectangle keeps {kept}")
    assert bits_equal(frames[0][0], frames[1][0]) and frames[0][1] == frames[1][1]
    assert units[1] - units[0] == tiles - kept and kept < tiles // 2
