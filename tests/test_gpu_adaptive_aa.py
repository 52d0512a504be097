"""Adaptive supersampling (rt_set_supersampling_threshold): refined pixels are the regular n x n pixels, every other pixel is the one-ray
pixel, chosen by the float32 rule of adaptive_ref.refine on the whole one-ray frame.  Tolerance 0 throughout.

Expected frames: from the CPU oracle (one-ray frame + n*n shifted-viewport frames, as tests/test_gpu_supersample.py builds the regular frame),
or from the GPU's own n = 1 frame and its regular n x n frame (threshold < 0)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import switch_table
from adaptive_ref import adaptive_frame, refine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCENES = os.path.join(HERE, "golden", "scenes")
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")
THREE = ((-1.0, 1.0, 1.0), (0.8, 0.4, 1.5), (0.0, 0.0, 2.0))
COUNTERS = ("rays_primary", "rays_centre", "rays_sample", "rays_bounce", "shaded_hits", "pixels_culled")
INF = float("inf")


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def offsets(n):
    return [np.float32((2 * s + 1 - n) / (2.0 * n)) for s in range(n)]


def shifted(cam, n, sx, sy):
    o = offsets(n)
    cam.viewport[0] = float(-o[sx])
    cam.viewport[1] = float(-o[sy])
    return cam


def box(frames, n):
    acc = np.zeros_like(frames[0], dtype=np.float32)
    for f in frames:
        acc = (acc + f).astype(np.float32)
    return (acc / np.float32(n * n)).astype(np.float32)


def quantise_u8(rgb):
    q = np.trunc(np.float32(255) * np.asarray(rgb, np.float32))
    return np.clip(np.minimum(q, np.float32(255)), 0, None).astype(np.uint8)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def diff(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=-1).sum())


def open_ctx(rt, path):
    hs = rt.HostScene(path, 1000, 15)
    ctx = rt.Context(0)
    ctx.upload(hs)
    return hs, ctx


def setting(ctx, n, tau):
    ctx.set_supersampling(n)
    ctx.set_supersampling_threshold(tau)


def render(rt, ctx, cam, L, w, h, depth, p=None):
    p = p or rt.make_params(w, h, depth)
    rgb = np.full((h, w, 3), np.nan, np.float32)
    st = rt.capi.rt_stats()
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), None,
                                                         C.byref(st)), "rt_render")
    return rgb, st


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


def counters(st):
    return {k: int(getattr(st, k)) for k in COUNTERS}


def area_lights(rt, grid=8):
    return rt.make_lights(points=THREE[:1], area=True, usteps=grid, vsteps=grid)


def gpu_pair(rt, ctx, cam, L, w, h, n, depth=4):
    """the GPU's own one-ray frame and regular n x n frame (threshold < 0)"""
    setting(ctx, 1, -1.0)
    one, _ = render(rt, ctx, cam, L, w, h, depth)
    setting(ctx, n, -1.0)
    reg, st = render(rt, ctx, cam, L, w, h, depth)
    return one, reg, st


# ------------------------------------------------------------------------------------------ 1. the oracle, small frames
def lights_pair(rt, oracle, kind):
    if kind == "area8":
        return rt.make_lights(points=THREE[:1], area=True, usteps=8, vsteps=8), oracle.lights(area=True, usteps=8, vsteps=8, points=THREE[:1])
    if kind == "three":
        return rt.make_lights(points=THREE, area=True, usteps=5, vsteps=5), oracle.lights(area=True, usteps=5, vsteps=5, points=THREE)
    off = rt.sphere_offsets(65, 1.0, 25)
    L = rt.set_sphere(rt.make_lights(points=THREE[:1], area=False), off)
    oL = oracle.lights(area=False, points=THREE[:1])
    oL.mode, oL.n_offsets = 2, off.shape[0]
    oL.offsets = off.ctypes.data_as(C.POINTER(C.c_float))
    oL._keep = off
    return L, oL


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cube.obj", "dodgeColorTest.obj", "mixed"])
@pytest.mark.parametrize("kind", ["area8", "three", "sphere"])
def test_adaptive_frame_equals_the_oracle(rt, oracle, tmp_path, which, kind):
    if which == "mixed":
        import scenes_gen
        path, yaw = scenes_gen.mixed_materials(str(tmp_path)), 0.4
    else:
        path, yaw = os.path.join(SCENES, which), 0.0
    hs, ctx = open_ctx(rt, path)
    osc = oracle.load_scene(path)
    w, h, depth = 40, 24, 4
    L, oL = lights_pair(rt, oracle, kind)
    partial = 0
    try:
        one = osc.render(oracle.camera(w, h, yaw), oL, w, h, max_depth=depth, threads=8)[0]
        for n in (2, 3, 4):
            reg = box([osc.render(shifted(oracle.camera(w, h, yaw), n, sx, sy), oL, w, h, max_depth=depth, threads=8)[0]
                       for sy in range(n) for sx in range(n)], n)
            for tau in (0.0, 0.05, 0.3):
                setting(ctx, n, tau)
                rgb, u8 = render_device(rt, ctx, rt.default_camera(w, h, yaw), L, w, h, depth)
                mask = refine(one, tau)
                want = adaptive_frame(one, reg, tau)
                assert bits_equal(rgb, want), (n, tau, diff(rgb, want))
                assert np.array_equal(u8, quantise_u8(want)), (n, tau)
                assert ctx.supersampling_refined() == int(mask.sum()), (n, tau)
                partial += 0 < mask.sum() < mask.size
    finally:
        osc.close(); ctx.close(); hs.close()
    assert partial > 0, "some case must refine some pixels but not all"


# ------------------------------------------------------------------------------------------ 2. full size, GPU against GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,n", [("cube.obj", 1920, 1080, 4), ("dodgeColorTest.obj", 960, 540, 2), ("cube.obj", 1920, 1081, 3)])
def test_full_size_adaptive_frame(rt, name, w, h, n):
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    cam, L, tau = rt.default_camera(w, h), area_lights(rt), 0.05
    one, reg, _ = gpu_pair(rt, ctx, cam, L, w, h, n)
    setting(ctx, n, tau)
    st = rt.capi.rt_stats()
    rgb, u8 = render_device(rt, ctx, cam, L, w, h, 4, stats=st)
    refined = ctx.supersampling_refined()
    ctx.close(); hs.close()
    mask = refine(one, tau)
    want = adaptive_frame(one, reg, tau)
    assert bits_equal(rgb, want), diff(rgb, want)
    assert np.array_equal(u8, quantise_u8(want))
    assert refined == int(mask.sum()) and 0 < refined < w * h
    assert int(st.pixels) == w * h + n * n * refined
    assert int(st.rays_primary) > 0 and int(st.launches_total) > 0


# ------------------------------------------------------------------------------------------ 3. endpoints
@pytest.mark.gpu
def test_endpoints(rt):
    w, h, n = 320, 200, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    cam, L = rt.default_camera(w, h), area_lights(rt)
    setting(ctx, 1, -1.0)
    one, u1 = render_device(rt, ctx, cam, L, w, h, 4)
    assert ctx.supersampling_refined() == 0
    setting(ctx, n, INF)
    rgb, u8 = render_device(rt, ctx, cam, L, w, h, 4)
    assert bits_equal(rgb, one) and np.array_equal(u8, u1)
    assert ctx.supersampling_refined() == 0
    setting(ctx, n, -1.0)
    reg, st_reg = render(rt, ctx, cam, L, w, h, 4)
    assert ctx.supersampling_refined() == w * h
    setting(ctx, 1, 0.0)                                   # n = 1 ignores the threshold
    got, _ = render(rt, ctx, cam, L, w, h, 4)
    assert bits_equal(got, one)
    ctx.close(); hs.close()
    # tau < 0 is today's regular frame and its counters on a fresh context
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    ctx.set_supersampling(n)
    reg2, st2 = render(rt, ctx, cam, L, w, h, 4)
    ctx.close(); hs.close()
    assert bits_equal(reg, reg2)
    assert counters(st_reg) == counters(st2) and int(st_reg.pixels) == int(st2.pixels) == n * n * w * h
    assert int(st_reg.launches_total) == int(st2.launches_total)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (1, 17), (17, 1)])
def test_tiny_frames(rt, w, h):
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    cam, L = rt.default_camera(w, h), area_lights(rt, 4)
    for n in (2, 3):
        one, reg, _ = gpu_pair(rt, ctx, cam, L, w, h, n)
        setting(ctx, n, 0.0)
        rgb, u8 = render_device(rt, ctx, cam, L, w, h, 4)
        want = adaptive_frame(one, reg, 0.0)
        assert bits_equal(rgb, want), (n, diff(rgb, want))
        assert np.array_equal(u8, quantise_u8(want))
        assert ctx.supersampling_refined() == int(refine(one, 0.0).sum())
    ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 4. shards, row ranges, the gather
@pytest.mark.gpu
def test_shards_and_row_ranges_equal_the_full_frame(rt):
    w, h, n, tau = 256, 157, 2, 0.05
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    cam, L = rt.default_camera(w, h), area_lights(rt)
    setting(ctx, n, tau)
    full, full8 = render_device(rt, ctx, cam, L, w, h, 4)
    assert 0 < ctx.supersampling_refined() < w * h
    for stripe in (8, 1, 5):
        for nranks in (2, 3):
            for rank in range(nranks):
                ys = [y for y in range(h) if (y // stripe) % nranks == rank]
                rgb, u8 = render_device(rt, ctx, cam, L, w, h, 4, stripe=stripe, rank=rank, nranks=nranks)
                assert bits_equal(rgb, full[ys]), (stripe, nranks, rank, diff(rgb, full[ys]))
                assert np.array_equal(u8, full8[ys])
    rgb, u8 = render_device(rt, ctx, cam, L, w, h, 4, row0=5, row1=h - 3)
    assert bits_equal(rgb, full[5:h - 3]) and np.array_equal(u8, full8[5:h - 3])
    # rt_render_gather over a one-rank communicator, then rt_stitch_rows
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
    comm.close(); ctx.close(); hs.close()
    assert np.array_equal(frame, full8.reshape(-1))


# ------------------------------------------------------------------------------------------ 5. graphs
@pytest.mark.gpu
def test_graph_keeps_the_threshold_it_was_captured_with(rt):
    w, h, n, tau = 320, 200, 2, 0.05
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    L = area_lights(rt)
    setting(ctx, n, tau)
    out, out8 = rt.hipmem.DeviceBuffer(h * w * 3 * 4), rt.hipmem.DeviceBuffer(h * w * 3)
    g = rt.FrameGraph(ctx, L, rt.make_params(w, h, 4), out.address, out8.address)
    ctx.set_supersampling_threshold(INF)
    yaws = (0.0, 0.3, -0.5)
    got = []
    for yaw in yaws:
        g.launch(rt.default_camera(w, h, yaw))
        st = g.stats()
        got.append((out.to_numpy(np.float32, (h, w, 3)), out8.to_numpy(np.uint8, (h, w, 3)), int(st.pixels)))
    g.close()
    ctx.set_supersampling_threshold(tau)
    for yaw, (rgb, u8, pixels) in zip(yaws, got):
        want, want8 = render_device(rt, ctx, rt.default_camera(w, h, yaw), L, w, h, 4)
        refined = ctx.supersampling_refined()
        assert bits_equal(rgb, want), (yaw, diff(rgb, want))
        assert np.array_equal(u8, want8), yaw
        assert 0 < refined < w * h and pixels == w * h + n * n * refined
    ctx.close(); hs.close(); out.free(); out8.free()


# ------------------------------------------------------------------------------------------ 6. the other primary-ray paths
@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"RT_STAGED_TRACE": "0"}, {"RT_TRACE_DYNAMIC": "1"}, {"RT_NO_CULL": "1"}])
def test_primary_ray_variants(rt, monkeypatch, env):
    w, h, n, tau = 256, 160, 2, 0.05
    cam, L = rt.default_camera(w, h), area_lights(rt)
    frames = []
    for e in ({}, env):
        for k, v in e.items():
            monkeypatch.setenv(k, v)
        hs, ctx = open_ctx(rt, os.path.join(SCENES, "dodgeColorTest.obj"))
        setting(ctx, n, tau)
        frames.append(render(rt, ctx, cam, L, w, h, 4)[0])
        assert 0 < ctx.supersampling_refined() < w * h
        ctx.close(); hs.close()
    assert bits_equal(frames[1], frames[0]), diff(frames[1], frames[0])


# ------------------------------------------------------------------------------------------ 7. settings changing on one context
@pytest.mark.gpu
def test_changing_settings_on_one_context(rt):
    w, h = 200, 136
    cam, L = rt.default_camera(w, h, 0.3), area_lights(rt)
    hs, ref = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    setting(ref, 1, -1.0)
    one, _ = render(rt, ref, cam, L, w, h, 4)
    regs = {}
    for n in (2, 3, 4):
        setting(ref, n, -1.0)
        regs[n] = render(rt, ref, cam, L, w, h, 4)[0]
    ref.close()
    ctx = rt.Context(0)
    ctx.upload(hs)
    for n, tau in ((4, 0.05), (2, 0.3), (3, 0.0), (3, 0.3), (4, 0.0), (2, 0.05)):
        setting(ctx, n, tau)
        rgb, st = render(rt, ctx, cam, L, w, h, 4)
        want = adaptive_frame(one, regs[n], tau)
        assert bits_equal(rgb, want), (n, tau, diff(rgb, want))
        assert int(st.pixels) == w * h + n * n * int(refine(one, tau).sum())
    ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ collect_stats 1 and 2
@pytest.mark.gpu
def test_collect_stats_modes(rt):
    w, h, n, tau = 256, 160, 2, 0.05
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    cam, L = rt.default_camera(w, h), area_lights(rt)
    setting(ctx, n, tau)
    base, st0 = render(rt, ctx, cam, L, w, h, 4)
    p = rt.make_params(w, h, 4, collect_stats=True)
    counted, st1 = render(rt, ctx, cam, L, w, h, 4, p=p)
    assert bits_equal(counted, base) and counters(st1) == counters(st0) and int(st1.pixels) == int(st0.pixels)
    assert int(st1.box_tests) > 0
    assert st0.ms_total > 0 and st0.ms_resolve > 0
    lib = ctx.lib
    lib.rt_timing_collect(ctx.handle, C.byref(rt.capi.rt_stats()))
    p.collect_stats = 2
    for _ in range(3):
        render(rt, ctx, cam, L, w, h, 4, p=p)
    tim = rt.capi.rt_stats()
    rt.capi.check(lib, ctx.handle, lib.rt_timing_collect(ctx.handle, C.byref(tim)), "rt_timing_collect")
    ctx.close(); hs.close()
    assert tim.ms_total > 0 and int(tim.pixels) == int(st0.pixels)
    assert int(tim.launches_total) == int(st0.launches_total)


# ------------------------------------------------------------------------------------------ 8. the CLI and the Python Flyscene
@pytest.mark.gpu
def test_cli_writes_the_adaptive_frame(rt, tmp_path):
    path, w, h, n, tau = os.path.join(SCENES, "cube.obj"), 64, 64, 2, 0.1
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(w, h, True, False)
    fs.supersample, fs.supersample_threshold = n, tau
    fs.output_path = str(tmp_path / "py.ppm")
    rgb = fs.raytraceScene()
    refined = fs.ctx.supersampling_refined()
    L = fs._lights()
    one, reg, _ = gpu_pair(rt, fs.ctx, rt.default_camera(w, h), L, w, h, n, depth=-1)
    fs.ctx.close(); fs.scene.close()
    want = adaptive_frame(one, reg, tau)
    assert bits_equal(rgb, want) and refined == int(refine(one, tau).sum()) and refined > 0
    r = subprocess.run([RT_RENDER, "--scene", path, "--size", str(w), str(h), "--aa", str(n), "--aa-threshold", str(tau), "--out",
                        str(tmp_path / "cli.ppm")], input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert (tmp_path / "cli.ppm").read_bytes() == (tmp_path / "py.ppm").read_bytes()
