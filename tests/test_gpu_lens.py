"""Thin-lens depth of field (rt_set_lens) through every frame entry point.  Tolerance 0 throughout.

The expected frames never come from the frame path under test: the rays of every sub-sample are built by tests/lens_ref.py (the six steps of
the doc comment of rt_set_lens, float32, with the LIBRARY's lens table as data) and traced by the CPU oracle (orc_box_intersect as pre-cull,
orc_trace_ray) or, at full size, by rt_trace_rays / rt_box_intersect, which ignore the lens; the fold is box() of test_gpu_supersample.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lens_ref
import switch_table

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCENES = os.path.join(HERE, "golden", "scenes")
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")
WORK_LIB = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")
THREE = ((-1.0, 1.0, 1.0), (0.8, 0.4, 1.5), (0.0, 0.0, 2.0))
COUNTERS = ("rays_primary", "rays_centre", "rays_sample", "rays_bounce", "shaded_hits", "pixels_culled")
F = np.float32
AP = 0.08


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def offsets(n):
    return [F((2 * s + 1 - n) / (2.0 * n)) for s in range(n)]


def quantise_u8(rgb):
    q = np.trunc(F(255) * np.asarray(rgb, F))
    return np.clip(np.minimum(q, F(255)), 0, None).astype(np.uint8)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def diff(a, b):
    return int((np.ascontiguousarray(a, F).view(np.uint32) != np.ascontiguousarray(b, F).view(np.uint32)).any(axis=-1).sum())


def fold(colours, n):
    """colours[H, W, n, n, 3] -> acc = 0.0f + the sub-sample colours (sy outer, sx inner), acc / (float)(n*n)"""
    acc = np.zeros(colours.shape[:2] + (3,), F)
    for sy in range(n):
        for sx in range(n):
            acc = (acc + colours[:, :, sy, sx]).astype(F)
    return (acc / F(n * n)).astype(F)


def open_ctx(rt, path, cap=1000):
    hs = rt.HostScene(path, cap, 15)
    ctx = rt.Context(0)
    ctx.upload(hs)
    return hs, ctx


def counters(st):
    return {k: int(getattr(st, k)) for k in COUNTERS}


def move_camera(cam, centre):
    """camera centre (and the translation column of inv_view) moved to `centre`: same orientation"""
    for k in range(3):
        cam.center[k] = float(centre[k])
        cam.inv_view[4 * k + 3] = float(centre[k])
    return cam


def render(rt, ctx, cam, L, w, h, depth, hits=False, p=None):
    p = p or rt.make_params(w, h, depth)
    rgb = np.full((h, w, 3), np.nan, F)
    hit = np.full((h, w), -7, np.int32) if hits else None
    st = rt.capi.rt_stats()
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p),
                                                         hit.ctypes.data_as(C.c_void_p) if hits else None, C.byref(st)), "rt_render")
    return rgb, hit, st


def render_device(rt, ctx, cam, L, w, h, depth, row0=0, row1=None, stripe=1, rank=0, nranks=1, stats=None):
    """rt_render_device: float and 8-bit rows of ONE launch"""
    import torch
    p = rt.make_params(w, h, depth, row0, h if row1 is None else row1, stripe, rank, nranks)
    rows = ctx.lib.rt_local_rows(C.byref(p))
    d_rgb = torch.full((rows, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    d_u8 = torch.full((rows, w, 3), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = ctx.lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(d_rgb.data_ptr()), C.c_void_p(d_u8.data_ptr()),
                                  None, None, C.byref(stats) if stats is not None else None)
    rt.capi.check(ctx.lib, ctx.handle, st, "rt_render_device")
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_synchronize(ctx.handle), "rt_synchronize")
    return d_rgb.cpu().numpy(), d_u8.cpu().numpy()


def area_lights(rt, grid=8):
    return rt.make_lights(points=THREE[:1], area=True, usteps=grid, vsteps=grid)


def lights_pair(rt, oracle, kind):
    if kind == "area5":
        return rt.make_lights(points=THREE[:1], area=True, usteps=5, vsteps=5), oracle.lights(area=True, usteps=5, vsteps=5, points=THREE[:1])
    if kind == "point":
        return rt.make_lights(points=THREE[:1], area=False), oracle.lights(area=False, points=THREE[:1])
    if kind == "three":
        return rt.make_lights(points=THREE, area=True, usteps=5, vsteps=5), oracle.lights(area=True, usteps=5, vsteps=5, points=THREE)
    off = rt.sphere_offsets(65, 1.0, 25)
    L = rt.set_sphere(rt.make_lights(points=THREE[:1], area=False), off)
    oL = oracle.lights(area=False, points=THREE[:1])
    oL.mode, oL.n_offsets = 2, off.shape[0]
    oL.offsets = off.ctypes.data_as(C.POINTER(C.c_float))
    oL._keep = off
    return L, oL


# ------------------------------------------------------------------------------------------ 1. the oracle, small frames
def oracle_lens_frame(oracle, osc, ocam, oL, w, h, n, depth, aperture, focus, T):
    """(frame, pre-culled sub-samples, distinct rotations) by lens_ref + the unchanged oracle"""
    o = offsets(n)
    S = np.zeros((h, w, n, n, 3), F)
    for j in range(h):
        for i in range(w):
            for sy in range(n):
                for sx in range(n):
                    S[j, i, sy, sx] = oracle.screen_to_world(ocam, float(F(i) + o[sx]), float(F(j) + o[sy]))
    centre, m = np.array(list(ocam.center), F), np.array(list(ocam.inv_view), F)
    O, P, D = lens_ref.lens_rays(S, centre, m, aperture, focus, T, n)
    root = osc.node(0)["box"]
    bmin, bmax = np.ascontiguousarray(root[:3]), np.ascontiguousarray(root[3:])
    fp = C.POINTER(C.c_float)
    col = np.ones((h, w, n, n, 3), F)
    culled = 0
    for idx in np.ndindex(h, w, n, n):
        oo, pp = np.ascontiguousarray(O[idx]), np.ascontiguousarray(P[idx])
        if not oracle.lib.orc_box_intersect(bmin.ctypes.data_as(fp), bmax.ctypes.data_as(fp), oo.ctypes.data_as(fp), pp.ctypes.data_as(fp)):
            culled += 1
            continue
        col[idx] = osc.trace_ray(oL, oo, D[idx], 0, depth)
    rots = {lens_ref.lens_hash(i, j) >> 26 for j in range(h) for i in range(w)}
    return fold(col, n), culled, len(rots)


ORACLE_CASES = [
    # scene, n, lights, focus, yaw, camera centre (None: the default), depth
    ("cube.obj", 2, "area5", 2.0, 0.0, None, 2),
    ("cube.obj", 4, "point", 1.5, 0.3, None, 2),                      # focus in front of the model, yawed camera (U, V not axis-aligned)
    ("cube.obj", 3, "three", 3.0, 0.0, None, 2),                      # focus behind the model
    ("cube.obj", 1, "area5", 2.0, 0.0, None, 2),                      # n = 1: the lens centre, by the lens path
    ("cube.obj", 2, "sphere", 0.5, 0.0, (0.1, 0.05, 0.3), 2),         # camera centre inside the root box
    ("dodgeColorTest.obj", 3, "area5", 2.0, 0.0, None, 2),            # tree with big leaves: the leaf-task launches run
    ("dodgeColorTest.obj", 2, "sphere", 1.2, 0.3, None, 2),
    ("dodgeColorTest.obj", 4, "three", 2.0, 0.0, None, 2),
    ("mixed", 2, "area5", 2.0, 0.4, None, 4),                         # mirror / refraction / Fresnel: the eye matters
    ("mixed", 4, "sphere", 2.6, 0.4, None, 4),
    ("mixed", 3, "three", 1.4, 0.4, None, 4),
]


@pytest.mark.gpu
@pytest.mark.parametrize("which,n,kind,focus,yaw,centre,depth", ORACLE_CASES)
def test_lens_frame_equals_the_oracle_on_the_reference_rays(rt, oracle, tmp_path, which, n, kind, focus, yaw, centre, depth):
    if which == "mixed":
        import scenes_gen
        path = scenes_gen.mixed_materials(str(tmp_path))
    else:
        path = os.path.join(SCENES, which)
    hs, ctx = open_ctx(rt, path)
    osc = oracle.load_scene(path)
    w, h = 32, 24
    L, oL = lights_pair(rt, oracle, kind)
    cam, ocam = rt.default_camera(w, h, yaw), oracle.camera(w, h, yaw)
    if centre is not None:
        move_camera(cam, centre); move_camera(ocam, centre)
    try:
        T = lens_ref.library_table(ctx.lib, n)
        want, culled, rots = oracle_lens_frame(oracle, osc, ocam, oL, w, h, n, depth, AP, focus, T)
        ctx.set_supersampling(n)
        pin, _ = render_device(rt, ctx, cam, L, w, h, depth)
        ctx.set_lens(AP, focus)
        st = rt.capi.rt_stats()
        rgb, u8 = render_device(rt, ctx, cam, L, w, h, depth, stats=st)
        print(f"{which} n={n} {kind} focus={focus}: differs from the oracle in {diff(rgb, want)} pixels, from the pinhole frame in {diff(rgb, pin)}, "
              f"culled {int(st.pixels_culled)} / {culled}, rotations {rots}")
        assert np.isfinite(want).all()
        assert bits_equal(rgb, want), (diff(rgb, want), float(np.abs(rgb - want).max()))
        assert np.array_equal(u8, quantise_u8(want))
        assert int(st.pixels_culled) == culled
        assert int(st.pixels) == n * n * w * h
        assert ctx.supersampling_refined() == (0 if n == 1 else w * h)
        if n > 1:
            assert not bits_equal(want, pin), "the lens must change the frame"
    finally:
        osc.close(); ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 2. full size, GPU against GPU
def gpu_lens_frame(rt, ctx, hs, cam, L, w, h, n, depth, aperture, focus, rows=None):
    """the fold of rt_trace_rays on the lens_ref rays, rt_box_intersect on the root box as pre-cull (both ignore the lens)"""
    lib = ctx.lib
    o = offsets(n)
    S = np.zeros((h, w, n, n, 3), F)
    vp = (cam.viewport[0], cam.viewport[1])
    for sy in range(n):
        for sx in range(n):
            # (float)i - (-o) == (float)i + o: the sub-sample's screen points are the pixels' of the shifted viewport
            cam.viewport[0], cam.viewport[1] = float(-o[sx]), float(-o[sy])
            pts = np.zeros((h, w, 3), F)
            rt.capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(cam), w, h, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
            S[:, :, sy, sx] = pts
    cam.viewport[0], cam.viewport[1] = vp
    T = lens_ref.library_table(lib, n)
    O, P, D = lens_ref.lens_rays(S, np.array(list(cam.center), F), np.array(list(cam.inv_view), F), aperture, focus, T, n, rows=rows)
    N = O.size // 3
    O, P, D = (np.ascontiguousarray(a.reshape(N, 3)) for a in (O, P, D))
    node0 = hs.view.nodes[0]
    box = np.array(list(node0.bmin) + list(node0.bmax), F)
    boxes = np.ascontiguousarray(np.broadcast_to(box, (N, 6)))
    pre = np.zeros(N, np.uint8)
    vptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rt.capi.check(lib, ctx.handle, lib.rt_box_intersect(ctx.handle, N, vptr(boxes), vptr(O), vptr(P), vptr(pre)), "rt_box_intersect")
    col = np.zeros((N, 3), F)
    rt.capi.check(lib, ctx.handle, lib.rt_trace_rays(ctx.handle, C.byref(L), depth, N, vptr(O), vptr(D), vptr(col), None, None), "rt_trace_rays")
    col[pre == 0] = 1.0                                                                       # BACKGROUND
    return fold(col.reshape(h, w, n, n, 3), n), int((pre == 0).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,n", [("cube.obj", 1920, 1080, 2), ("dodgeColorTest.obj", 480, 270, 3)])
def test_full_size_lens_frame_equals_the_fold_of_rt_trace_rays(rt, name, w, h, n):
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    cam, L = rt.default_camera(w, h), area_lights(rt)
    want, culled = gpu_lens_frame(rt, ctx, hs, cam, L, w, h, n, 4, AP, 2.0)
    ctx.set_supersampling(n)
    ctx.set_lens(AP, 2.0)
    st = rt.capi.rt_stats()
    rgb, u8 = render_device(rt, ctx, cam, L, w, h, 4, stats=st)
    ctx.close(); hs.close()
    assert bits_equal(rgb, want), (diff(rgb, want), float(np.abs(rgb - want).max()))
    assert np.array_equal(u8, quantise_u8(want))
    assert int(st.pixels_culled) == culled and int(st.pixels) == n * n * w * h
    assert int(st.rays_primary) > 0 and int(st.rays_sample) > 0


# ------------------------------------------------------------------------------------------ 3. off is off
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_aperture_zero_is_the_pinhole_frame_launch_for_launch(rt, name):
    w, h = 200, 136
    cam, L = rt.default_camera(w, h, 0.3), area_lights(rt)
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    settings = [(1, -1.0), (2, -1.0), (3, -1.0), (4, -1.0), (2, 0.05)]

    def frames():
        out = []
        for n, tau in settings:
            ctx.set_supersampling(n); ctx.set_supersampling_threshold(tau)
            st = rt.capi.rt_stats()
            rgb, u8 = render_device(rt, ctx, cam, L, w, h, 4, stats=st)
            out.append((rgb, u8, dict(counters(st), pixels=int(st.pixels), launches=int(st.launches_total)), ctx.supersampling_refined()))
        return out

    never = frames()
    ctx.set_lens(0.0, 2.0)
    zero = frames()
    ctx.set_lens(AP, 2.0)
    ctx.set_supersampling(2); ctx.set_supersampling_threshold(-1.0)
    on, _ = render_device(rt, ctx, cam, L, w, h, 4)
    ctx.set_lens(0.0, 2.0)
    back = frames()
    ctx.set_lens(0.0, float("nan"))                        # aperture 0: the focus is not looked at
    ctx.close(); hs.close()
    assert not bits_equal(on, never[1][0])
    for other in (zero, back):
        for a, b in zip(never, other):
            assert bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    assert 0 < never[4][3] < w * h, "the adaptive frame refines some pixels"


# ------------------------------------------------------------------------------------------ 4. shards, row ranges, the gather
@pytest.mark.gpu
def test_shards_and_row_ranges_equal_the_full_frame(rt):
    w, h, n = 256, 157, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    cam, L = rt.default_camera(w, h, 0.3), area_lights(rt)
    ctx.set_supersampling(n)
    ctx.set_lens(AP, 1.8)
    full, full8 = render_device(rt, ctx, cam, L, w, h, 4)
    for stripe in (8, 1, 5):
        for nranks in (2, 3):
            for rank in range(nranks):
                ys = [y for y in range(h) if (y // stripe) % nranks == rank]
                rgb, u8 = render_device(rt, ctx, cam, L, w, h, 4, stripe=stripe, rank=rank, nranks=nranks)
                assert bits_equal(rgb, full[ys]), (stripe, nranks, rank, diff(rgb, full[ys]))
                assert np.array_equal(u8, full8[ys])
    rgb, u8 = render_device(rt, ctx, cam, L, w, h, 4, row0=5, row1=h - 3)
    assert bits_equal(rgb, full[5:h - 3]) and np.array_equal(u8, full8[5:h - 3])
    import torch
    stripe = 8
    p = rt.make_params(w, h, 4, 0, h, stripe, 0, 1)
    comm = rt.shard.Comm(0, rt.shard.Comm.unique_id(), 1, 0)
    local = torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda")
    gathered = torch.zeros_like(local)
    torch.cuda.synchronize()
    st = ctx.lib.rt_render_gather(ctx.handle, comm.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(local.data_ptr()), local.numel(),
                                  C.c_void_p(gathered.data_ptr()), 0, None)
    rt.capi.check(ctx.lib, ctx.handle, st, "rt_render_gather")
    torch.cuda.synchronize()
    frame = np.zeros(w * h * 3, np.uint8)
    g = gathered.cpu().numpy()
    assert ctx.lib.rt_stitch_rows(g.ctypes.data_as(C.c_void_p), local.numel(), w, h, stripe, 1, frame.ctypes.data_as(C.c_void_p)) == 0
    # a row range against the reference rays with the FULL frame's rows in the hash
    want, _ = gpu_lens_frame(rt, ctx, hs, cam, L, w, h, n, 4, AP, 1.8)
    comm.close(); ctx.close(); hs.close()
    assert np.array_equal(frame, full8.reshape(-1))
    assert bits_equal(full, want), diff(full, want)


# ------------------------------------------------------------------------------------------ 5. graphs
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_graph_replays_the_lens_frame_and_keeps_its_lens(rt, name):
    w, h, n = 320, 200, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    ctx.set_supersampling(n)
    ctx.set_lens(AP, 2.0)
    out, out8 = rt.hipmem.DeviceBuffer(h * w * 3 * 4), rt.hipmem.DeviceBuffer(h * w * 3)
    g = rt.FrameGraph(ctx, L, rt.make_params(w, h, 4), out.address, out8.address)
    ctx.set_lens(0.2, 1.0)                                  # changing the lens after capture does not change the graph's frames
    yaws, got = (0.0, 0.3, -0.5), []
    for k, yaw in enumerate(yaws):
        if k == 2:
            ctx.set_lens(0.0, 2.0)
        g.launch(rt.default_camera(w, h, yaw))
        st = g.stats()
        assert int(st.pixels) == n * n * w * h
        got.append((out.to_numpy(F, (h, w, 3)), out8.to_numpy(np.uint8, (h, w, 3))))
    g.close()
    ctx.set_lens(AP, 2.0)
    for yaw, (rgb, u8) in zip(yaws, got):
        want, want8 = render_device(rt, ctx, rt.default_camera(w, h, yaw), L, w, h, 4)
        assert bits_equal(rgb, want), (yaw, diff(rgb, want))
        assert np.array_equal(u8, want8), yaw
    ctx.set_lens(0.0, 2.0)
    pin, _ = render_device(rt, ctx, rt.default_camera(w, h, 0.0), L, w, h, 4)
    ctx.close(); hs.close(); out.free(); out8.free()
    assert not bits_equal(got[0][0], got[1][0]) and not bits_equal(got[0][0], pin)


# ------------------------------------------------------------------------------------------ 6. the other primary-ray paths and the culling switches
PATH_CASES = [
    ("dodgeColorTest.obj", {"RT_NO_CULL": "1"}),
    ("dodgeColorTest.obj", {"RT_NO_SHAFT": "1"}),
    ("dodgeColorTest.obj", {"RT_TRACE_BUDGET": "1"}),
    ("dodgeColorTest.obj", {"RT_TRACE_BUDGET": "0"}),
    ("cube.obj", {"RT_TRACE_DYNAMIC": "1"}),
    ("cube.obj", {"RT_NO_CULL": "1"}),
    ("cube.obj", {"RT_NO_BEAM": "1"}),
]


# (the ids keep the numbers the cases had when env0 and env1 set RT_STAGED_TRACE=0: a lens frame on a tree has no fused trace kernel any more,
#  it is staged whatever the switch says)
@pytest.mark.gpu
@pytest.mark.parametrize("name,env", PATH_CASES, ids=[f"{name}-env{i + 2}" for i, (name, _) in enumerate(PATH_CASES)])
def test_lens_frame_under_the_path_and_culling_switches(rt, monkeypatch, name, env):
    w, h, n = 256, 160, 2
    cam, L = rt.default_camera(w, h, 0.3), area_lights(rt)
    frames = []
    for e in ({}, env):
        for k, v in e.items():
            monkeypatch.setenv(k, v)                 # read by rt_create / rt_upload_scene
        hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
        ctx.set_supersampling(n)
        ctx.set_lens(AP, 2.0)
        rgb, _, st = render(rt, ctx, cam, L, w, h, 4)
        frames.append((rgb, counters(st)))
        ctx.close(); hs.close()
    assert bits_equal(frames[1][0], frames[0][0]), diff(frames[1][0], frames[0][0])
    assert frames[1][1] == frames[0][1]


# ------------------------------------------------------------------------------------------ 7. statistics modes, the adaptive override, hit ids
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_collect_stats_modes_and_the_adaptive_override(rt, name):
    w, h, n = 256, 160, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    cam, L = rt.default_camera(w, h), area_lights(rt)
    ctx.set_supersampling(n)
    ctx.set_lens(AP, 2.0)
    base, _, st0 = render(rt, ctx, cam, L, w, h, 4)
    p = rt.make_params(w, h, 4, collect_stats=True)
    counted, _, st1 = render(rt, ctx, cam, L, w, h, 4, p=p)
    assert bits_equal(counted, base) and counters(st1) == counters(st0) and int(st1.pixels) == int(st0.pixels) == n * n * w * h
    assert int(st1.box_tests) > 0 and st0.ms_total > 0
    lib = ctx.lib
    lib.rt_timing_collect(ctx.handle, C.byref(rt.capi.rt_stats()))
    p.collect_stats = 2
    for _ in range(3):
        render(rt, ctx, cam, L, w, h, 4, p=p)
    tim = rt.capi.rt_stats()
    rt.capi.check(lib, ctx.handle, lib.rt_timing_collect(ctx.handle, C.byref(tim)), "rt_timing_collect")
    assert tim.ms_total > 0 and int(tim.pixels) == int(st0.pixels) and int(tim.launches_total) == int(st0.launches_total)
    # tau = 0.1 with the lens on is tau = -1: the regular lens frame, every pixel refined
    ctx.set_supersampling_threshold(0.1)
    ad, _, st_ad = render(rt, ctx, cam, L, w, h, 4)
    assert ctx.supersampling_refined() == w * h
    assert bits_equal(ad, base) and counters(st_ad) == counters(st0) and int(st_ad.pixels) == int(st0.pixels)
    assert int(st_ad.launches_total) == int(st0.launches_total)
    ctx.set_lens(0.0, 2.0)                                  # ... and the adaptive frame is back with the pinhole
    render(rt, ctx, cam, L, w, h, 4)
    assert 0 < ctx.supersampling_refined() < w * h
    ctx.close(); hs.close()


@pytest.mark.gpu
def test_hit_ids_follow_the_supersampling_rule(rt):
    w, h = 96, 64
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    cam, L = rt.default_camera(w, h), area_lights(rt)
    ctx.set_lens(AP, 2.0)
    rgb, hit, _ = render(rt, ctx, cam, L, w, h, 4, hits=True)          # n = 1: the level-0 hit of the lens ray
    S = np.zeros((h, w, 1, 1, 3), F)
    pts = np.zeros((h, w, 3), F)
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_primary_points(ctx.handle, C.byref(cam), w, h, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
    S[:, :, 0, 0] = pts
    O, P, D = lens_ref.lens_rays(S, np.array(list(cam.center), F), np.array(list(cam.inv_view), F), AP, 2.0, lens_ref.library_table(ctx.lib, 1), 1)
    N = w * h
    O, D = np.ascontiguousarray(O.reshape(N, 3)), np.ascontiguousarray(D.reshape(N, 3))
    col, face = np.zeros((N, 3), F), np.zeros(N, np.int32)
    vptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_trace_rays(ctx.handle, C.byref(L), 4, N, vptr(O), vptr(D), vptr(col), vptr(face), None), "rt_trace_rays")
    assert (hit >= 0).any()
    assert np.array_equal(hit.reshape(-1)[hit.reshape(-1) >= 0], face[hit.reshape(-1) >= 0])
    ctx.set_supersampling(2)
    p = rt.make_params(w, h, 4)
    assert ctx.lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), vptr(rgb), vptr(hit), None) == rt.capi.RT_ERR_INVALID
    ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 8. validation on a live context
@pytest.mark.gpu
def test_invalid_lenses_keep_the_previous_setting(rt):
    w, h, n = 64, 48, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    lib, c = ctx.lib, rt.capi
    cam, L = rt.default_camera(w, h), area_lights(rt, 4)
    ctx.set_supersampling(n)
    assert lib.rt_set_lens(ctx.handle, 0.05, 1.7) == c.RT_OK
    want, _, _ = render(rt, ctx, cam, L, w, h, 4)
    inf, nan = float("inf"), float("nan")
    for a, f in ((-0.1, 2.0), (nan, 2.0), (inf, 2.0), (-inf, 2.0), (0.1, 0.0), (0.1, -1.0), (0.1, nan), (0.1, inf), (0.1, -inf)):
        assert lib.rt_set_lens(ctx.handle, a, f) == c.RT_ERR_INVALID, (a, f)
        assert b"rt_set_lens" in lib.rt_last_error(ctx.handle)
        got, _, _ = render(rt, ctx, cam, L, w, h, 4)
        assert bits_equal(got, want), (a, f)
    for a, f in ((0.0, 0.0), (0.0, -3.0), (0.0, nan)):
        assert lib.rt_set_lens(ctx.handle, a, f) == c.RT_OK, (a, f)
    pin, _, _ = render(rt, ctx, cam, L, w, h, 4)
    ctx.close(); hs.close()
    assert not bits_equal(pin, want)


# ------------------------------------------------------------------------------------------ 9. front ends and the counting build
@pytest.mark.gpu
def test_python_flyscene_and_cli_write_the_lens_frame(rt, tmp_path):
    path, w, h, n = os.path.join(SCENES, "cube.obj"), 64, 64, 2
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(w, h, True, False)
    fs.supersample, fs.aperture, fs.focus = n, AP, 1.8
    fs.output_path = str(tmp_path / "py.ppm")
    rgb = fs.raytraceScene()
    L = fs._lights()
    want, _ = gpu_lens_frame(rt, fs.ctx, fs.scene, rt.default_camera(w, h), L, w, h, n, -1, AP, 1.8)
    fs.ctx.close(); fs.scene.close()
    assert bits_equal(rgb, want), diff(rgb, want)
    r = subprocess.run([RT_RENDER, "--scene", path, "--size", str(w), str(h), "--aa", str(n), "--lens", str(AP), "1.8", "--out",
                        str(tmp_path / "cli.ppm")], input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert (tmp_path / "cli.ppm").read_bytes() == (tmp_path / "py.ppm").read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_counting_build_renders_the_lens_frame(rt, name):
    assert os.path.exists(WORK_LIB), "the counting build is part of `make all`"
    hs = rt.HostScene(os.path.join(SCENES, name), 1000, 15)
    w, h, n = 96, 64, 3
    cam, L = rt.default_camera(w, h), area_lights(rt)
    frames = []
    for lib in (rt.load_library(), rt.capi.load_library(WORK_LIB)):
        ctx = C.c_void_p()
        assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
        try:
            rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(hs.view)), "rt_upload_scene")
            rt.capi.check(lib, ctx, lib.rt_set_supersampling(ctx, n), "rt_set_supersampling")
            rt.capi.check(lib, ctx, lib.rt_set_lens(ctx, AP, 2.0), "rt_set_lens")
            p = rt.make_params(w, h, 4)
            rgb = np.full((h, w, 3), np.nan, F)
            st = rt.capi.rt_stats()
            rt.capi.check(lib, ctx, lib.rt_render(ctx, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), None, C.byref(st)),
                          "rt_render")
            frames.append((rgb, counters(st)))
        finally:
            lib.rt_destroy(ctx)
    hs.close()
    assert bits_equal(frames[1][0], frames[0][0])
    assert frames[1][1] == frames[0][1]
