"""Camera motion blur (rt_set_shutter) through every frame entry point.  Tolerance 0 throughout.

The expected frames never come from the frame path under test: the camera K(t) and the ray of every sub-sample are built by
tests/shutter_ref.py (the definition in the doc comment of rt_set_shutter, float32) and traced by the CPU oracle (its screen_to_world on K(t),
orc_box_intersect as pre-cull, orc_trace_ray) or, at full size, by rt_trace_rays / rt_box_intersect, which ignore the shutter; the fold is
the one of test_gpu_lens.py.  close == open ties the per-lane generator to the shipped one on every pixel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lens_ref
import oracle_lib
import shutter_ref
import switch_table
import test_gpu_lens as gl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCENES = os.path.join(HERE, "golden", "scenes")
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")
WORK_LIB = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")
F = np.float32
AP = 0.08
YAW = 0.05
bits_equal, diff, fold, offsets, quantise_u8, counters = gl.bits_equal, gl.diff, gl.fold, gl.offsets, gl.quantise_u8, gl.counters
open_ctx, render, render_device, area_lights, lights_pair = gl.open_ctx, gl.render, gl.render_device, gl.area_lights, gl.lights_pair


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def copy_cam(cam):
    return type(cam).from_buffer_copy(bytes(cam))


def as_ocamera(cam):
    return oracle_lib.ocamera.from_buffer_copy(bytes(cam))


def shifted(cam, delta):
    """a copy of cam translated by delta (centre and the translation column of inv_view): same orientation"""
    out = copy_cam(cam)
    return gl.move_camera(out, [cam.center[k] + delta[k] for k in range(3)])


def shutter_pair(rt, w, h, kind, yaw0=0.0):
    """(open, close) for the shutters the tests use: a yaw of 0.05 rad, a translation, both"""
    a = rt.default_camera(w, h, yaw0)
    if kind == "yaw":
        return a, rt.default_camera(w, h, yaw0 + YAW)
    if kind == "move":
        return a, shifted(a, (0.06, -0.03, 0.05))
    return a, shifted(rt.default_camera(w, h, yaw0 + YAW), (0.06, -0.03, 0.05))


# ------------------------------------------------------------------------------------------ 1. the oracle, small frames
def oracle_shutter_frame(oracle, osc, a, b, oL, w, h, n, depth, lens):
    """(frame, pre-culled sub-samples) by shutter_ref + the unchanged oracle; a / b the cameras at shutter open / close, lens None or
    (aperture, focus, T)"""
    o = offsets(n)
    oa, ob = as_ocamera(a), as_ocamera(b)
    root = osc.node(0)["box"]
    bmin, bmax = np.ascontiguousarray(root[:3]), np.ascontiguousarray(root[3:])
    fp = C.POINTER(C.c_float)
    col = np.ones((h, w, n, n, 3), F)
    culled = 0
    for j, i, sy, sx in np.ndindex(h, w, n, n):
        K = shutter_ref.shutter_camera(oa, ob, shutter_ref.shutter_time(i, j, sx, sy, n))
        S = oracle.screen_to_world(K, float(F(i) + o[sx]), float(F(j) + o[sy]))
        point = None
        if lens is not None:
            r, k = lens_ref.rotation_and_point(i, j, sx, sy, n)
            point = lens[2][r, k]
        O, P, D = shutter_ref.shutter_ray(S, shutter_ref.pose(K), lens=lens, lens_point=point)
        O, P = np.ascontiguousarray(O), np.ascontiguousarray(P)
        if not oracle.lib.orc_box_intersect(bmin.ctypes.data_as(fp), bmax.ctypes.data_as(fp), O.ctypes.data_as(fp), P.ctypes.data_as(fp)):
            culled += 1
            continue
        col[j, i, sy, sx] = osc.trace_ray(oL, O, D, 0, depth)
    return fold(col, n), culled


ORACLE_CASES = [
    # scene, n, lights, shutter, lens on, depth
    ("cube.obj", 1, "area5", "yaw", False, 4),                       # n = 1: one time per pixel
    ("cube.obj", 2, "point", "move", False, 0),
    ("cube.obj", 3, "three", "both", False, 4),
    ("cube.obj", 4, "sphere", "yaw", False, 4),
    ("cube.obj", 2, "area5", "both", True, 4),
    ("cube.obj", 3, "point", "yaw", True, 0),
    ("cube.obj", 1, "three", "move", True, 4),                        # n = 1 with the lens: the lens centre of K(t)
    ("dodgeColorTest.obj", 2, "area5", "yaw", False, 4),              # tree with big leaves: the leaf-task launches run, without a cone
    ("dodgeColorTest.obj", 3, "sphere", "move", False, 0),
    ("dodgeColorTest.obj", 4, "three", "both", False, 4),
    ("dodgeColorTest.obj", 1, "point", "both", False, 4),
    ("dodgeColorTest.obj", 4, "area5", "yaw", True, 4),
    ("dodgeColorTest.obj", 2, "three", "move", True, 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("which,n,kind,shutter,lens_on,depth", ORACLE_CASES)
def test_shutter_frame_equals_the_oracle_on_the_reference_rays(rt, oracle, which, n, kind, shutter, lens_on, depth):
    path = os.path.join(SCENES, which)
    hs, ctx = open_ctx(rt, path)
    osc = oracle.load_scene(path)
    w, h = 40, 28
    L, oL = lights_pair(rt, oracle, kind)
    a, b = shutter_pair(rt, w, h, shutter, 0.2)
    try:
        lens = (AP, 1.8, lens_ref.library_table(ctx.lib, n)) if lens_on else None
        want, culled = oracle_shutter_frame(oracle, osc, a, b, oL, w, h, n, depth, lens)
        ctx.set_supersampling(n)
        if lens_on:
            ctx.set_lens(AP, 1.8)
        still, _ = render_device(rt, ctx, a, L, w, h, depth)
        ctx.set_shutter(b)
        st = rt.capi.rt_stats()
        rgb, u8 = render_device(rt, ctx, a, L, w, h, depth, stats=st)
        print(f"{which} n={n} {kind} {shutter} lens={lens_on} depth={depth}: differs from the oracle in {diff(rgb, want)} pixels, from the still frame in "
              f"{diff(rgb, still)}, culled {int(st.pixels_culled)} / {culled}")
        assert np.isfinite(want).all()
        assert bits_equal(rgb, want), (diff(rgb, want), float(np.abs(rgb - want).max()))
        assert np.array_equal(u8, quantise_u8(want))
        assert int(st.pixels_culled) == culled
        assert int(st.pixels) == n * n * w * h
        assert ctx.supersampling_refined() == (0 if n == 1 else w * h)
        assert not bits_equal(want, still), "the shutter must change the frame"
    finally:
        osc.close(); ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 2. full size, GPU against GPU
def raster_terms(rt, ctx, cam, w, h, n):
    """n0, n1 [h, w, n, n]: the camera-independent vector (normalised x * aspect*scale, normalised y * scale) of every sub-sample's raster
    point -- x and y of rt_primary_points with an identity inv_view, exactly"""
    o = offsets(n)
    ident = copy_cam(cam)
    for k in range(12):
        ident.inv_view[k] = 1.0 if k in (0, 5, 10) else 0.0
    n0, n1 = np.zeros((h, w, n, n), F), np.zeros((h, w, n, n), F)
    for sy in range(n):
        for sx in range(n):
            # (float)i - (-o) == (float)i + o: the sub-sample's raster points are the pixels' of the shifted viewport
            ident.viewport[0], ident.viewport[1] = float(-o[sx]), float(-o[sy])
            pts = np.zeros((h, w, 3), F)
            rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_primary_points(ctx.handle, C.byref(ident), w, h, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
            assert (pts[..., 2] == F(-1.0)).all()
            n0[:, :, sy, sx], n1[:, :, sy, sx] = pts[..., 0], pts[..., 1]
    return n0, n1


def gpu_shutter_frame(rt, ctx, hs, a, b, L, w, h, n, depth, lens=None):
    """the fold of rt_trace_rays on the shutter_ref rays, rt_box_intersect on the root box as pre-cull (both ignore the shutter);
    lens None or (aperture, focus)"""
    lib = ctx.lib
    n0, n1 = raster_terms(rt, ctx, a, w, h, n)
    full = None if lens is None else (lens[0], lens[1], lens_ref.library_table(lib, n))
    O, P, D = shutter_ref.shutter_rays(n0, n1, shutter_ref.pose(a), shutter_ref.pose(b), n, np.arange(h), lens=full)
    N = O.size // 3
    O, P, D = (np.ascontiguousarray(x.reshape(N, 3)) for x in (O, P, D))
    node0 = hs.view.nodes[0]
    box = np.array(list(node0.bmin) + list(node0.bmax), F)
    boxes = np.ascontiguousarray(np.broadcast_to(box, (N, 6)))
    pre = np.zeros(N, np.uint8)
    vptr = lambda x: x.ctypes.data_as(C.c_void_p)
    rt.capi.check(lib, ctx.handle, lib.rt_box_intersect(ctx.handle, N, vptr(boxes), vptr(O), vptr(P), vptr(pre)), "rt_box_intersect")
    col, face = np.zeros((N, 3), F), np.zeros(N, np.int32)
    rt.capi.check(lib, ctx.handle, lib.rt_trace_rays(ctx.handle, C.byref(L), depth, N, vptr(O), vptr(D), vptr(col), vptr(face), None), "rt_trace_rays")
    col[pre == 0] = 1.0                                                                       # BACKGROUND
    face[pre == 0] = -1
    return fold(col.reshape(h, w, n, n, 3), n), int((pre == 0).sum()), face.reshape(h, w, n, n)


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,n,lens", [("cube.obj", 1920, 1080, 2, None), ("dodgeColorTest.obj", 480, 270, 3, (AP, 2.0))])
def test_full_size_shutter_frame_equals_the_fold_of_rt_trace_rays(rt, name, w, h, n, lens):
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "both")
    want, culled, _ = gpu_shutter_frame(rt, ctx, hs, a, b, L, w, h, n, 4, lens)
    ctx.set_supersampling(n)
    if lens:
        ctx.set_lens(*lens)
    ctx.set_shutter(b)
    st = rt.capi.rt_stats()
    rgb, u8 = render_device(rt, ctx, a, L, w, h, 4, stats=st)
    ctx.close(); hs.close()
    assert bits_equal(rgb, want), (diff(rgb, want), float(np.abs(rgb - want).max()))
    assert np.array_equal(u8, quantise_u8(want))
    assert int(st.pixels_culled) == culled and int(st.pixels) == n * n * w * h
    assert int(st.rays_primary) > 0 and int(st.rays_sample) > 0


# ------------------------------------------------------------------------------------------ 3. close == open is the still frame
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_still_shutter_is_the_still_frame(rt, name):
    w, h = 200, 136
    L = area_lights(rt)
    cam = rt.default_camera(w, h, 0.3)
    for q in (1, 4, 6, 9):                                    # the yaw leaves zeros here: make them negative zeros
        assert cam.inv_view[q] == 0.0
        cam.inv_view[q] = -0.0
    same = copy_cam(cam)
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    try:
        for lens_on in (False, True):
            ctx.set_lens(AP if lens_on else 0.0, 2.0)
            for n in (1, 2, 3, 4):
                ctx.set_supersampling(n)
                ctx.set_shutter(None)
                s0, s1 = rt.capi.rt_stats(), rt.capi.rt_stats()
                off, off8 = render_device(rt, ctx, cam, L, w, h, 4, stats=s0)
                ctx.set_shutter(same)
                on, on8 = render_device(rt, ctx, cam, L, w, h, 4, stats=s1)
                assert bits_equal(on, off), (lens_on, n, diff(on, off))
                assert np.array_equal(on8, off8), (lens_on, n)
                assert counters(s1) == counters(s0) and int(s1.pixels) == int(s0.pixels), (lens_on, n)
    finally:
        ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 4. off is off
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_shutter_off_is_the_frame_it_was_launch_for_launch(rt, name):
    w, h = 200, 136
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "yaw", 0.3)
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    settings = [(1, -1.0), (2, -1.0), (3, -1.0), (4, -1.0), (2, 0.05)]

    def frames():
        out = []
        for lens_on in (False, True):
            ctx.set_lens(AP if lens_on else 0.0, 2.0)
            for n, tau in settings:
                ctx.set_supersampling(n); ctx.set_supersampling_threshold(tau)
                st = rt.capi.rt_stats()
                rgb, u8 = render_device(rt, ctx, a, L, w, h, 4, stats=st)
                out.append((rgb, u8, dict(counters(st), pixels=int(st.pixels), launches=int(st.launches_total)), ctx.supersampling_refined()))
        return out

    never = frames()
    ctx.set_shutter(None)
    null = frames()
    ctx.set_shutter(b)
    ctx.set_lens(0.0, 2.0); ctx.set_supersampling(2); ctx.set_supersampling_threshold(-1.0)
    on, _ = render_device(rt, ctx, a, L, w, h, 4)
    ctx.set_shutter(None)
    back = frames()
    ctx.set_lens(0.0, 2.0); ctx.set_supersampling(2); ctx.set_supersampling_threshold(-1.0)
    close_still, _ = render_device(rt, ctx, b, L, w, h, 4)
    ctx.close(); hs.close()
    assert not bits_equal(on, never[1][0]) and not bits_equal(on, close_still), "the exposure is neither still frame"
    for other in (null, back):
        for x, y in zip(never, other):
            assert bits_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] and x[3] == y[3]
    assert 0 < never[4][3] < w * h, "the adaptive frame refines some pixels"


# ------------------------------------------------------------------------------------------ 5. shards, row ranges, the gather
@pytest.mark.gpu
def test_shards_and_row_ranges_equal_the_full_frame(rt):
    w, h, n = 256, 157, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "both", 0.3)
    ctx.set_supersampling(n)
    ctx.set_shutter(b)
    full, full8 = render_device(rt, ctx, a, L, w, h, 4)
    for stripe in (8, 1, 5):
        for nranks in (2, 3):
            for rank in range(nranks):
                ys = [y for y in range(h) if (y // stripe) % nranks == rank]
                rgb, u8 = render_device(rt, ctx, a, L, w, h, 4, stripe=stripe, rank=rank, nranks=nranks)
                assert bits_equal(rgb, full[ys]), (stripe, nranks, rank, diff(rgb, full[ys]))
                assert np.array_equal(u8, full8[ys])
    rgb, u8 = render_device(rt, ctx, a, L, w, h, 4, row0=5, row1=h - 3)
    assert bits_equal(rgb, full[5:h - 3]) and np.array_equal(u8, full8[5:h - 3])
    import torch
    stripe = 8
    p = rt.make_params(w, h, 4, 0, h, stripe, 0, 1)
    comm = rt.shard.Comm(0, rt.shard.Comm.unique_id(), 1, 0)
    local = torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda")
    gathered = torch.zeros_like(local)
    torch.cuda.synchronize()
    st = ctx.lib.rt_render_gather(ctx.handle, comm.handle, C.byref(a), C.byref(L), C.byref(p), C.c_void_p(local.data_ptr()), local.numel(),
                                  C.c_void_p(gathered.data_ptr()), 0, None)
    rt.capi.check(ctx.lib, ctx.handle, st, "rt_render_gather")
    torch.cuda.synchronize()
    frame = np.zeros(w * h * 3, np.uint8)
    g = gathered.cpu().numpy()
    assert ctx.lib.rt_stitch_rows(g.ctypes.data_as(C.c_void_p), local.numel(), w, h, stripe, 1, frame.ctypes.data_as(C.c_void_p)) == 0
    want, _, _ = gpu_shutter_frame(rt, ctx, hs, a, b, L, w, h, n, 4)
    comm.close(); ctx.close(); hs.close()
    assert np.array_equal(frame, full8.reshape(-1))
    assert bits_equal(full, want), diff(full, want)


# ------------------------------------------------------------------------------------------ 6. graphs
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_graph_takes_both_cameras_per_launch_and_keeps_its_shutter(rt, name):
    w, h, n = 320, 200, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    ctx.set_supersampling(n)
    pairs = [shutter_pair(rt, w, h, "yaw", 0.0), shutter_pair(rt, w, h, "both", 0.3), shutter_pair(rt, w, h, "move", -0.5)]
    ctx.set_shutter(pairs[0][1])
    out, out8 = rt.hipmem.DeviceBuffer(h * w * 3 * 4), rt.hipmem.DeviceBuffer(h * w * 3)
    g = rt.FrameGraph(ctx, L, rt.make_params(w, h, 4), out.address, out8.address)
    ctx.set_shutter(pairs[2][1])                            # changing the context's shutter after capture changes nothing
    got = []
    for k, (a, b) in enumerate(pairs):
        if k == 2:
            ctx.set_shutter(None)                           # ... nor does clearing it
        g.launch(a, close=b)
        assert int(g.stats().pixels) == n * n * w * h
        got.append((out.to_numpy(F, (h, w, 3)), out8.to_numpy(np.uint8, (h, w, 3))))
    still_cam = rt.default_camera(w, h, 0.3)
    g.launch(still_cam)                                     # rt_graph_launch on a shutter graph: close = cam, a still frame
    g.stats()
    got_still = out.to_numpy(F, (h, w, 3))
    # a close camera with another perspective is refused and the output stays
    bad = copy_cam(pairs[0][1]); bad.fovy = 45.0
    assert ctx.lib.rt_graph_launch_shutter(g.handle, C.byref(pairs[0][0]), C.byref(bad), None) == rt.capi.RT_ERR_INVALID
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_synchronize(ctx.handle), "rt_synchronize")
    assert bits_equal(out.to_numpy(F, (h, w, 3)), got_still)
    g.close()
    for (a, b), (rgb, u8) in zip(pairs, got):
        ctx.set_shutter(b)
        want, want8 = render_device(rt, ctx, a, L, w, h, 4)
        assert bits_equal(rgb, want), diff(rgb, want)
        assert np.array_equal(u8, want8)
    ctx.set_shutter(None)
    want_still, _ = render_device(rt, ctx, still_cam, L, w, h, 4)
    assert bits_equal(got_still, want_still), diff(got_still, want_still)
    assert not bits_equal(got[0][0], got[1][0]) and not bits_equal(got[1][0], want_still)
    # a graph captured with the shutter off refuses two cameras and leaves its output alone
    import torch
    g2 = rt.FrameGraph(ctx, L, rt.make_params(w, h, 4), out.address, out8.address)
    g2.launch(still_cam)
    g2.stats()
    before = out.to_numpy(F, (h, w, 3))
    a, b = pairs[0]
    assert ctx.lib.rt_graph_launch_shutter(g2.handle, C.byref(a), C.byref(b), None) == rt.capi.RT_ERR_INVALID
    assert b"shutter off" in ctx.lib.rt_last_error(ctx.handle)
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_synchronize(ctx.handle), "rt_synchronize")
    torch.cuda.synchronize()
    assert bits_equal(out.to_numpy(F, (h, w, 3)), before) and bits_equal(before, want_still)
    g2.close()
    ctx.close(); hs.close(); out.free(); out8.free()


# ------------------------------------------------------------------------------------------ 7. the other primary-ray paths and the culling switches
PATH_CASES = [
    ("dodgeColorTest.obj", {"RT_NO_CULL": "1"}),
    ("dodgeColorTest.obj", {"RT_NO_SHAFT": "1"}),
    ("dodgeColorTest.obj", {"RT_TRACE_BUDGET": "1"}),
    ("dodgeColorTest.obj", {"RT_TRACE_BUDGET": "0"}),
    ("cube.obj", {"RT_TRACE_DYNAMIC": "1"}),
    ("cube.obj", {"RT_NO_CULL": "1"}),
    ("cube.obj", {"RT_NO_BEAM": "1"}),
]


# (the ids keep the numbers the cases had when env0 and env1 set RT_STAGED_TRACE=0: a shutter frame on a tree has no fused trace kernel any more,
#  it is staged whatever the switch says)
@pytest.mark.gpu
@pytest.mark.parametrize("name,env", PATH_CASES, ids=[f"{name}-env{i + 2}" for i, (name, _) in enumerate(PATH_CASES)])
def test_shutter_frame_under_the_path_and_culling_switches(rt, monkeypatch, name, env):
    w, h, n = 256, 160, 2
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "both", 0.3)
    frames = []
    for e in ({}, env):
        for k, v in e.items():
            monkeypatch.setenv(k, v)                 # read by rt_create / rt_upload_scene
        hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
        ctx.set_supersampling(n)
        ctx.set_shutter(b)
        rgb, _, st = render(rt, ctx, a, L, w, h, 4)
        frames.append((rgb, counters(st)))
        ctx.close(); hs.close()
    assert bits_equal(frames[1][0], frames[0][0]), diff(frames[1][0], frames[0][0])
    assert frames[1][1] == frames[0][1]


# ------------------------------------------------------------------------------------------ 8. statistics modes, the adaptive override, hit ids
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_collect_stats_modes_and_the_adaptive_override(rt, name):
    w, h, n = 256, 160, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "yaw")
    ctx.set_supersampling(n)
    ctx.set_shutter(b)
    base, _, st0 = render(rt, ctx, a, L, w, h, 4)
    p = rt.make_params(w, h, 4, collect_stats=True)
    counted, _, st1 = render(rt, ctx, a, L, w, h, 4, p=p)
    assert bits_equal(counted, base) and counters(st1) == counters(st0) and int(st1.pixels) == int(st0.pixels) == n * n * w * h
    assert int(st1.box_tests) > 0 and st0.ms_total > 0
    lib = ctx.lib
    lib.rt_timing_collect(ctx.handle, C.byref(rt.capi.rt_stats()))
    p.collect_stats = 2
    for _ in range(3):
        last, _, _ = render(rt, ctx, a, L, w, h, 4, p=p)
    assert bits_equal(last, base)
    tim = rt.capi.rt_stats()
    rt.capi.check(lib, ctx.handle, lib.rt_timing_collect(ctx.handle, C.byref(tim)), "rt_timing_collect")
    assert tim.ms_total > 0 and int(tim.pixels) == int(st0.pixels) and int(tim.launches_total) == int(st0.launches_total)
    # tau = 0.1 with the shutter on is tau = -1: the regular shutter frame, every pixel refined
    ctx.set_supersampling_threshold(0.1)
    ad, _, st_ad = render(rt, ctx, a, L, w, h, 4)
    assert ctx.supersampling_refined() == w * h
    assert bits_equal(ad, base) and counters(st_ad) == counters(st0) and int(st_ad.pixels) == int(st0.pixels)
    assert int(st_ad.launches_total) == int(st0.launches_total)
    ctx.set_shutter(None)                                   # ... and the adaptive frame is back with the still camera
    render(rt, ctx, a, L, w, h, 4)
    assert 0 < ctx.supersampling_refined() < w * h
    ctx.close(); hs.close()


@pytest.mark.gpu
def test_hit_ids_follow_the_supersampling_rule(rt):
    w, h = 96, 64
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "both")
    ctx.set_shutter(b)
    rgb, hit, _ = render(rt, ctx, a, L, w, h, 4, hits=True)            # n = 1: the level-0 hit of the pixel's ray
    want, _, face = gpu_shutter_frame(rt, ctx, hs, a, b, L, w, h, 1, 4)
    assert bits_equal(rgb, want)
    assert (hit >= 0).any() and (hit < 0).any()
    assert np.array_equal(hit, face[:, :, 0, 0])
    ctx.set_supersampling(2)
    p = rt.make_params(w, h, 4)
    vptr = lambda x: x.ctypes.data_as(C.c_void_p)
    assert ctx.lib.rt_render(ctx.handle, C.byref(a), C.byref(L), C.byref(p), vptr(rgb), vptr(hit), None) == rt.capi.RT_ERR_INVALID
    ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 9. validation on a live context
@pytest.mark.gpu
def test_invalid_shutters_are_refused_and_change_nothing(rt):
    import torch
    w, h, n = 64, 48, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    lib, c = ctx.lib, rt.capi
    L = area_lights(rt, 4)
    a, b = shutter_pair(rt, w, h, "yaw")
    ctx.set_supersampling(n)
    ctx.set_shutter(b)
    want, _, _ = render(rt, ctx, a, L, w, h, 4)
    # rt_set_shutter: a non-finite pose keeps the previous setting
    for q, v in ((0, float("nan")), (2, float("inf")), (3, float("-inf")), (14, float("nan"))):
        bad = copy_cam(b)
        if q < 3:
            bad.center[q] = v
        else:
            bad.inv_view[q - 3] = v
        assert lib.rt_set_shutter(ctx.handle, C.byref(bad)) == c.RT_ERR_INVALID, q
        assert b"rt_set_shutter" in lib.rt_last_error(ctx.handle)
        got, _, _ = render(rt, ctx, a, L, w, h, 4)
        assert bits_equal(got, want), q
    # render time: fovy, aspect and viewport of close must be open's, bit for bit
    p = rt.make_params(w, h, 4)
    vptr = lambda x: x.ctypes.data_as(C.c_void_p)
    comm = rt.shard.Comm(0, rt.shard.Comm.unique_id(), 1, 0)
    for field in ("fovy", "aspect", "viewport"):
        bad = copy_cam(b)
        if field == "viewport":
            bad.viewport[1] = 0.5
        else:
            setattr(bad, field, getattr(bad, field) * 1.5)
        assert lib.rt_set_shutter(ctx.handle, C.byref(bad)) == c.RT_OK
        rgb = np.full((h, w, 3), 3.0, F)
        assert lib.rt_render(ctx.handle, C.byref(a), C.byref(L), C.byref(p), vptr(rgb), None, None) == c.RT_ERR_INVALID, field
        assert b"shutter" in lib.rt_last_error(ctx.handle)
        assert (rgb == 3.0).all()
        d_rgb = torch.full((h, w, 3), 3.0, dtype=torch.float32, device="cuda")
        d_u8 = torch.full((h * w * 3,), 77, dtype=torch.uint8, device="cuda")
        gathered = torch.full((h * w * 3,), 78, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert lib.rt_render_device(ctx.handle, C.byref(a), C.byref(L), C.byref(p), C.c_void_p(d_rgb.data_ptr()), C.c_void_p(d_u8.data_ptr()), None, None,
                                    None) == c.RT_ERR_INVALID, field
        assert lib.rt_render_gather(ctx.handle, comm.handle, C.byref(a), C.byref(L), C.byref(p), C.c_void_p(d_u8.data_ptr()), d_u8.numel(),
                                    C.c_void_p(gathered.data_ptr()), 0, None) == c.RT_ERR_INVALID, field
        rt.capi.check(lib, ctx.handle, lib.rt_synchronize(ctx.handle), "rt_synchronize")
        torch.cuda.synchronize()
        assert bool((d_rgb == 3.0).all()) and bool((d_u8 == 77).all()) and bool((gathered == 78).all())
        ctx.set_shutter(b)
        got, _, _ = render(rt, ctx, a, L, w, h, 4)
        assert bits_equal(got, want), field
    comm.close(); ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 10. front ends and the counting build
@pytest.mark.gpu
def test_python_flyscene_and_cli_write_the_shutter_frame(rt, tmp_path):
    path, w, h, n = os.path.join(SCENES, "cube.obj"), 64, 64, 2
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(w, h, True, False)
    fs.supersample = n
    fs.shutter_close = rt.default_camera(w, h, YAW)
    fs.output_path = str(tmp_path / "py.ppm")
    rgb = fs.raytraceScene()
    L = fs._lights()
    p = rt.make_params(w, h, -1)
    abi = np.zeros((h, w, 3), F)
    rt.capi.check(fs.ctx.lib, fs.ctx.handle, fs.ctx.lib.rt_render(fs.ctx.handle, C.byref(rt.default_camera(w, h)), C.byref(L), C.byref(p),
                                                                   abi.ctypes.data_as(C.c_void_p), None, None), "rt_render")
    want, _, _ = gpu_shutter_frame(rt, fs.ctx, fs.scene, rt.default_camera(w, h), fs.shutter_close, L, w, h, n, -1)
    fs.shutter_close = None
    still = fs.raytraceScene(write_ppm=False)
    fs.ctx.close(); fs.scene.close()
    assert bits_equal(rgb, abi) and bits_equal(rgb, want), diff(rgb, want)
    assert not bits_equal(still, rgb)
    r = subprocess.run([RT_RENDER, "--scene", path, "--aa", str(n), "--shutter", str(YAW), "--size", str(w), str(h), "--out", str(tmp_path / "cli.ppm")],
                       input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert (tmp_path / "cli.ppm").read_bytes() == (tmp_path / "py.ppm").read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_counting_build_renders_the_shutter_frame(rt, name):
    assert os.path.exists(WORK_LIB), "the counting build is part of `make all`"
    hs = rt.HostScene(os.path.join(SCENES, name), 1000, 15)
    w, h, n = 96, 64, 3
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "both")
    frames = []
    for lib in (rt.load_library(), rt.capi.load_library(WORK_LIB)):
        ctx = C.c_void_p()
        assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
        try:
            rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(hs.view)), "rt_upload_scene")
            rt.capi.check(lib, ctx, lib.rt_set_supersampling(ctx, n), "rt_set_supersampling")
            rt.capi.check(lib, ctx, lib.rt_set_shutter(ctx, C.byref(b)), "rt_set_shutter")
            p = rt.make_params(w, h, 4)
            rgb = np.full((h, w, 3), np.nan, F)
            st = rt.capi.rt_stats()
            rt.capi.check(lib, ctx, lib.rt_render(ctx, C.byref(a), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), None, C.byref(st)),
                          "rt_render")
            frames.append((rgb, counters(st)))
        finally:
            lib.rt_destroy(ctx)
    hs.close()
    assert bits_equal(frames[1][0], frames[0][0])
    assert frames[1][1] == frames[0][1]
