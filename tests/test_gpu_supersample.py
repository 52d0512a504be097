"""Supersampling (rt_set_supersampling): n x n sub-samples per pixel, box filter, through every frame entry point.  Tolerance 0 throughout.

The expected frames come from the definition in include/rt_mi355x.h: for a camera whose viewport origin is (0, 0), sub-sample (sx, sy) of
pixel (i, j) is pixel (i, j) of the one-ray frame rendered with viewport[0] = -o[sx], viewport[1] = -o[sy] ((float)i - (-o) == (float)i + o),
so the n*n shifted-viewport frames -- of the CPU oracle or of the GPU's own n = 1 path -- summed in float32 (sy outer, sx inner) and divided by
float32(n*n) are the anti-aliased frame bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import switch_table

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCENES = os.path.join(HERE, "golden", "scenes")
WORK_LIB = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")
THREE = ((-1.0, 1.0, 1.0), (0.8, 0.4, 1.5), (0.0, 0.0, 2.0))
COUNTERS = ("rays_primary", "rays_centre", "rays_sample", "rays_bounce", "shaded_hits", "pixels_culled")


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    """every RT_* variable the library reads is cleared: the frames compared here are the defaults"""
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
    """acc = 0.0f + the sub-sample frames in the defined order (sy outer, sx inner), then acc / (float)(n*n)"""
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


def scene_path(which, tmp_path):
    if which == "mixed":
        import scenes_gen
        return scenes_gen.mixed_materials(str(tmp_path)), 0.4
    return os.path.join(SCENES, which), 0.0


def open_ctx(rt, path):
    hs = rt.HostScene(path, 1000, 15)
    ctx = rt.Context(0)
    ctx.upload(hs)
    return hs, ctx


def render(rt, ctx, cam, L, w, h, depth, hits=False):
    """rt_render: float frame (+ hit ids) and the ray counters"""
    p = rt.make_params(w, h, depth)
    rgb = np.full((h, w, 3), np.nan, np.float32)
    hit = np.full((h, w), -7, np.int32) if hits else None
    st = rt.capi.rt_stats()
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p),
                                                         hit.ctypes.data_as(C.c_void_p) if hits else None, C.byref(st)), "rt_render")
    return rgb, hit, st


def render_device(rt, ctx, cam, L, w, h, depth, rgb=True, stripe=1, rank=0, nranks=1, stats=None):
    """rt_render_device: float and 8-bit frames of ONE launch"""
    import torch
    p = rt.make_params(w, h, depth, 0, h, stripe, rank, nranks)
    rows = ctx.lib.rt_local_rows(C.byref(p))
    d_rgb = torch.full((rows, w, 3), float("nan"), dtype=torch.float32, device="cuda") if rgb else None
    d_u8 = torch.full((rows, w, 3), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = ctx.lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(d_rgb.data_ptr()) if rgb else None,
                                  C.c_void_p(d_u8.data_ptr()), None, None, C.byref(stats) if stats is not None else None)
    rt.capi.check(ctx.lib, ctx.handle, st, "rt_render_device")
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_synchronize(ctx.handle), "rt_synchronize")
    return (d_rgb.cpu().numpy() if rgb else None), d_u8.cpu().numpy()


def counters(st):
    return {k: int(getattr(st, k)) for k in COUNTERS}


def cube_lights(rt, grid=8):
    return rt.make_lights(points=THREE[:1], area=True, usteps=grid, vsteps=grid)


# ------------------------------------------------------------------------------------------ n = 1 is the one-ray frame
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_n1_is_the_one_ray_frame(rt, name):
    w, h = 200, 136
    cam, L = rt.default_camera(w, h), cube_lights(rt)
    runs = []
    for steps in ((), (1,), (2, 1)):
        hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
        for n in steps:
            ctx.set_supersampling(n)
        rgb, hit, st = render(rt, ctx, cam, L, w, h, 4, hits=True)
        runs.append((rgb, hit, dict(counters(st), pixels=int(st.pixels))))
        ctx.close(); hs.close()
    assert runs[0][2]["pixels"] == w * h and (runs[0][1] >= 0).any()
    for rgb, hit, cnt in runs[1:]:
        assert bits_equal(rgb, runs[0][0])
        assert np.array_equal(hit, runs[0][1])
        assert cnt == runs[0][2]


# ------------------------------------------------------------------------------------------ the oracle, small frames
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
def test_aa_frame_equals_the_oracle_with_shifted_viewports(rt, oracle, tmp_path, which, kind):
    """k_trace (cube), k_stage (dodge) and bounces + Fresnel (mixed) under an area light, three lights and the sphere light, n = 2, 3, 4"""
    path, yaw = scene_path(which, tmp_path)
    hs, ctx = open_ctx(rt, path)
    osc = oracle.load_scene(path)
    w, h, depth = 40, 24, 4
    L, oL = lights_pair(rt, oracle, kind)
    try:
        for n in (2, 3, 4):
            ctx.set_supersampling(n)
            rgb, u8 = render_device(rt, ctx, rt.default_camera(w, h, yaw), L, w, h, depth)
            subs = [osc.render(shifted(oracle.camera(w, h, yaw), n, sx, sy), oL, w, h, max_depth=depth, threads=8)[0]
                    for sy in range(n) for sx in range(n)]
            want = box(subs, n)
            assert bits_equal(rgb, want), (n, int((rgb != want).any(axis=-1).sum()), float(np.abs(rgb - want).max()))
            assert np.array_equal(u8, quantise_u8(want)), n
            assert not all(bits_equal(s, subs[0]) for s in subs[1:]), "the sub-samples must differ somewhere"
    finally:
        osc.close(); ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ full size, GPU against GPU, and the counters
@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,n", [("cube.obj", 1920, 1080, 2), ("dodgeColorTest.obj", 960, 540, 3), ("cube.obj", 1920, 1081, 3)])
def test_full_size_aa_equals_the_shifted_gpu_frames(rt, name, w, h, n):
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = cube_lights(rt)
    subs, total = [], dict.fromkeys(COUNTERS, 0)
    for sy in range(n):
        for sx in range(n):
            rgb, _, st = render(rt, ctx, shifted(rt.default_camera(w, h), n, sx, sy), L, w, h, 4)
            subs.append(rgb)
            for k, v in counters(st).items():
                total[k] += v
    want = box(subs, n)
    ctx.set_supersampling(n)
    st = rt.capi.rt_stats()
    rgb, u8 = render_device(rt, ctx, rt.default_camera(w, h), L, w, h, 4, stats=st)
    ctx.close(); hs.close()
    assert bits_equal(rgb, want), (int((rgb != want).any(axis=-1).sum()), float(np.abs(rgb - want).max()))
    assert np.array_equal(u8, quantise_u8(want))
    assert int(st.pixels) == n * n * w * h
    assert counters(st) == total
    assert total["rays_primary"] > 0 and total["rays_sample"] > 0


# ------------------------------------------------------------------------------------------ the other primary-ray paths
@pytest.mark.gpu
@pytest.mark.parametrize("name,env", [
    ("dodgeColorTest.obj", {"RT_STAGED_TRACE": "0"}),                            # the fused k_trace on a tree
    ("dodgeColorTest.obj", {"RT_STAGED_TRACE": "0", "RT_TRACE_DYNAMIC": "1"}),   # ... pulling tiles from the queue
    ("dodgeColorTest.obj", {"RT_TRACE_DYNAMIC": "1"}),
    ("dodgeColorTest.obj", {"RT_NO_CULL": "1"}),
    ("cube.obj", {"RT_TRACE_DYNAMIC": "1"}),
    ("cube.obj", {"RT_NO_CULL": "1"}),
])
def test_aa_frame_on_the_other_primary_paths(rt, monkeypatch, name, env):
    w, h, n = 256, 160, 2
    cam, L = rt.default_camera(w, h), cube_lights(rt)
    frames = []
    for e in ({}, env):
        for k, v in e.items():
            monkeypatch.setenv(k, v)                 # read by rt_create / rt_upload_scene
        hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
        ctx.set_supersampling(n)
        frames.append(render(rt, ctx, cam, L, w, h, 4)[0])
        ctx.close(); hs.close()
    assert bits_equal(frames[1], frames[0]), int((frames[1] != frames[0]).any(axis=-1).sum())


# ------------------------------------------------------------------------------------------ row shards
@pytest.mark.gpu
def test_row_shards_stitch_to_the_aa_frame(rt):
    w, h, n, stripe, nranks = 1920, 1080, 2, 8, 3
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    cam, L = rt.default_camera(w, h), cube_lights(rt)
    ctx.set_supersampling(n)
    _, whole = render_device(rt, ctx, cam, L, w, h, 4, rgb=False)
    blocks = [render_device(rt, ctx, cam, L, w, h, 4, rgb=False, stripe=stripe, rank=r, nranks=nranks)[1].reshape(-1) for r in range(nranks)]
    ctx.close(); hs.close()
    block_bytes = max(b.size for b in blocks)
    assert sum(b.size for b in blocks) == w * h * 3
    gathered = np.zeros(nranks * block_bytes, np.uint8)
    for r, b in enumerate(blocks):
        gathered[r * block_bytes:r * block_bytes + b.size] = b
    frame = np.zeros(w * h * 3, np.uint8)
    lib = rt.load_library()
    assert lib.rt_stitch_rows(gathered.ctypes.data_as(C.c_void_p), block_bytes, w, h, stripe, nranks, frame.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(frame, whole.reshape(-1))


# ------------------------------------------------------------------------------------------ captured graphs
@pytest.mark.gpu
def test_graph_replays_the_aa_frame(rt):
    w, h, n = 320, 200, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    L = cube_lights(rt)
    ctx.set_supersampling(n)
    out, out8 = rt.hipmem.DeviceBuffer(h * w * 3 * 4), rt.hipmem.DeviceBuffer(h * w * 3)
    g = rt.FrameGraph(ctx, L, rt.make_params(w, h, 4), out.address, out8.address)
    got = []
    for yaw in (0.0, 0.3, -0.5):
        g.launch(rt.default_camera(w, h, yaw))
        st = g.stats()                               # synchronises
        assert int(st.pixels) == n * n * w * h
        got.append((out.to_numpy(np.float32, (h, w, 3)), out8.to_numpy(np.uint8, (h, w, 3))))
    g.close()
    for yaw, (rgb, u8) in zip((0.0, 0.3, -0.5), got):
        want, want8 = render_device(rt, ctx, rt.default_camera(w, h, yaw), L, w, h, 4)
        assert bits_equal(rgb, want), yaw
        assert np.array_equal(u8, want8), yaw
    assert not bits_equal(got[0][0], got[1][0])
    ctx.close(); hs.close(); out.free(); out8.free()


@pytest.mark.gpu
def test_graph_keeps_the_supersampling_it_was_captured_with(rt):
    w, h = 320, 200
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    L, cam = cube_lights(rt), rt.default_camera(w, h, 0.3)
    want, want8 = render_device(rt, ctx, cam, L, w, h, 4)           # n = 1
    out, out8 = rt.hipmem.DeviceBuffer(h * w * 3 * 4), rt.hipmem.DeviceBuffer(h * w * 3)
    g = rt.FrameGraph(ctx, L, rt.make_params(w, h, 4), out.address, out8.address)
    ctx.set_supersampling(2)                                          # no eager frame in between
    g.launch(cam)
    st = g.stats()
    rgb, u8 = out.to_numpy(np.float32, (h, w, 3)), out8.to_numpy(np.uint8, (h, w, 3))
    g.close(); ctx.close(); hs.close(); out.free(); out8.free()
    assert int(st.pixels) == w * h
    assert bits_equal(rgb, want) and np.array_equal(u8, want8)


# ------------------------------------------------------------------------------------------ rejections
@pytest.mark.gpu
def test_rejections(rt):
    import torch
    c = rt.capi
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    lib = ctx.lib
    w, h = 24, 16
    cam, L = rt.default_camera(w, h), cube_lights(rt, 4)
    p = rt.make_params(w, h, 4)
    assert lib.rt_set_supersampling(ctx.handle, 3) == c.RT_OK
    for bad in (0, 5, -1):
        assert lib.rt_set_supersampling(ctx.handle, bad) == c.RT_ERR_INVALID
    _, _, st = render(rt, ctx, cam, L, w, h, 4)
    assert int(st.pixels) == 9 * w * h, "an invalid n keeps the previous setting"
    ctx.set_supersampling(2)
    rgb = np.zeros((h, w, 3), np.float32)
    hit = np.zeros((h, w), np.int32)
    assert lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), hit.ctypes.data_as(C.c_void_p), None) == c.RT_ERR_INVALID
    d_rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    d_hit = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    assert lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(d_rgb.data_ptr()), None, C.c_void_p(d_hit.data_ptr()),
                                None, None) == c.RT_ERR_INVALID
    # 25 lights x 1024 samples at 4K with n = 4: ~420 GB of visibility words alone -- refused before anything is freed or launched
    big = rt.make_lights(points=[(-1.0 + 0.05 * i, 1.0, 1.0) for i in range(25)], area=True, usteps=32, vsteps=32)
    W, H = 3840, 2160
    ctx.set_supersampling(4)
    d_u8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    pb = rt.make_params(W, H, 4)
    assert lib.rt_render_device(ctx.handle, C.byref(rt.default_camera(W, H)), C.byref(big), C.byref(pb), None, C.c_void_p(d_u8.data_ptr()), None,
                                None, None) == c.RT_ERR_UNSUPPORTED
    assert b"GB" in lib.rt_last_error(ctx.handle)
    del d_u8
    ctx.set_supersampling(2)
    got, _, st = render(rt, ctx, cam, L, w, h, 4)                   # the context still renders
    ctx.close()
    ctx2 = rt.Context(0)
    ctx2.upload(hs)
    ctx2.set_supersampling(2)
    want, _, _ = render(rt, ctx2, cam, L, w, h, 4)
    ctx2.close(); hs.close()
    assert int(st.pixels) == 4 * w * h
    assert bits_equal(got, want)


# ------------------------------------------------------------------------------------------ front ends and the counting build
@pytest.mark.gpu
def test_python_flyscene_and_cli_write_the_aa_frame(rt, tmp_path):
    path, w, h, n = os.path.join(SCENES, "cube.obj"), 64, 64, 2
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(w, h, True, False)
    fs.supersample = n
    fs.output_path = str(tmp_path / "py.ppm")
    fs.raytraceScene()
    assert int(fs.stats.pixels) == n * n * w * h
    with pytest.raises(ValueError):
        fs.raytraceScene(write_ppm=False, want_hits=True)
    # the expected float frame: the shifted-viewport frames of the same context at n = 1, written by rt_write_ppm
    fs.ctx.set_supersampling(1)
    L = fs._lights()
    want = box([render(rt, fs.ctx, shifted(rt.default_camera(w, h), n, sx, sy), L, w, h, -1)[0] for sy in range(n) for sx in range(n)], n)
    lib = fs.ctx.lib
    assert lib.rt_write_ppm(str(tmp_path / "want.ppm").encode(), want.ctypes.data_as(C.c_void_p), w, h) == 0
    fs.ctx.close(); fs.scene.close()
    assert (tmp_path / "py.ppm").read_bytes() == (tmp_path / "want.ppm").read_bytes()
    # rt_render --aa 2 (stdin: area light, not point -- the reference's two prompts)
    r = subprocess.run([RT_RENDER, "--scene", path, "--size", str(w), str(h), "--aa", str(n), "--out", str(tmp_path / "cli.ppm")],
                       input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert (tmp_path / "cli.ppm").read_bytes() == (tmp_path / "py.ppm").read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_counting_build_renders_the_aa_frame(rt, name):
    assert os.path.exists(WORK_LIB), "the counting build is part of `make all`"
    hs = rt.HostScene(os.path.join(SCENES, name), 1000, 15)
    w, h, n = 96, 64, 3
    cam, L = rt.default_camera(w, h), cube_lights(rt)
    frames = []
    for lib in (rt.load_library(), rt.capi.load_library(WORK_LIB)):
        ctx = C.c_void_p()
        assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
        try:
            rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(hs.view)), "rt_upload_scene")
            rt.capi.check(lib, ctx, lib.rt_set_supersampling(ctx, n), "rt_set_supersampling")
            p = rt.make_params(w, h, 4)
            rgb = np.full((h, w, 3), np.nan, np.float32)
            st = rt.capi.rt_stats()
            rt.capi.check(lib, ctx, lib.rt_render(ctx, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), None, C.byref(st)),
                          "rt_render")
            frames.append((rgb, counters(st)))
        finally:
            lib.rt_destroy(ctx)
    hs.close()
    assert bits_equal(frames[1][0], frames[0][0])
    assert frames[1][1] == frames[0][1]
