"""The builds and outputs the default parity tests never compare: the counting build (librt_mi355x_work.so, bench.py's executed-work
counters), k_resolve's 8-bit frame and the distributed output path (render -> 8-bit rows -> rt_stitch_rows -> rt_write_ppm_u8), and the
culling devices at full size."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import switch_table

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCENES = os.path.join(HERE, "golden", "scenes")
KA = json.load(open(os.path.join(HERE, "golden", "survey_known_answers.json")))
WORK_LIB = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")
RT_WORK_SHADOW = 640          # rt_device.hpp: offset of the shadow kernels' step counters in Control::prof
THREE = ((-1.0, 1.0, 1.0), (0.8, 0.4, 1.5), (0.0, 0.0, 2.0))
SWITCHES = tuple(switch_table.SWITCHES)      # every RT_* variable the library reads: cleared, so the frames compared here are the defaults


def counters(st):
    return (st.rays_primary, st.rays_bounce, st.rays_centre, st.rays_sample, st.shaded_hits)


def quantise_u8(rgb):
    """k_resolve's 8-bit value, in float32: min(255, trunc(255 * c)), clipped at 0"""
    q = np.trunc(np.float32(255) * np.asarray(rgb, np.float32))
    return np.clip(np.minimum(q, np.float32(255)), 0, None).astype(np.uint8)


def scene(rt, which, tmp_path):
    import scenes_gen
    if which == "mixed":
        return scenes_gen.mixed_materials(str(tmp_path)), 0.4
    return os.path.join(SCENES, which), 0.0


def render_lib(rt, lib, hs, cam, L, w, h, depth):
    ctx = C.c_void_p()
    assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
    try:
        rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(hs.view)), "rt_upload_scene")
        p = rt.make_params(w, h, depth)
        rgb = np.zeros((h, w, 3), np.float32)
        hits = np.zeros((h, w), np.int32)
        st = rt.capi.rt_stats()
        rt.capi.check(lib, ctx, lib.rt_render(ctx, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p),
                                              C.byref(st)), "rt_render")
        buf = (C.c_uint64 * 768)()
        wc = lib.rt_debug_work_counters(ctx, buf, 768)
        return rgb, hits, st, wc, np.array(buf, np.uint64)
    finally:
        lib.rt_destroy(ctx)


# ------------------------------------------------------------------------------------------ the counting build renders the product's frames
@pytest.mark.gpu
@pytest.mark.parametrize("which,grid,lights,depth,expect", [
    ("cube.obj", 8, 1, 4, ("trace_units", "beams_tested")),                       # flat fold: no shadow units, k_beam settles the hits
    ("mixed", 8, 3, 4, ("trace_units", "beams_tested")),
    ("dodgeColorTest.obj", 8, 1, 2, ("trace_units", "units", "shaft_groups")),
    ("dodgeColorTest.obj", 16, 1, 2, ("trace_units", "units", "shaft_groups", "beams_tested")),   # k_pair_beam in front of the shaft walk
])
def test_counting_build_renders_the_product_frame(rt, tmp_path, monkeypatch, which, grid, lights, depth, expect):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    assert os.path.exists(WORK_LIB), "the counting build is part of `make all`"
    work = rt.capi.load_library(WORK_LIB)
    prod = rt.load_library()
    path, yaw = scene(rt, which, tmp_path)
    hs = rt.HostScene(path, 1000, 15)
    w, h = 192, 128
    cam, L = rt.default_camera(w, h, yaw), rt.make_lights(points=THREE[:lights], area=True, usteps=grid, vsteps=grid)
    rgb0, hits0, st0, wc0, _ = render_lib(rt, prod, hs, cam, L, w, h, depth)
    rgb1, hits1, st1, wc1, prof = render_lib(rt, work, hs, cam, L, w, h, depth)
    hs.close()
    assert wc0 == rt.capi.RT_ERR_UNSUPPORTED, "the product library carries no step counters"
    assert wc1 == rt.capi.RT_OK
    assert (hits0 >= 0).sum() > 0.02 * hits0.size
    assert np.array_equal(hits1, hits0), f"{int((hits1 != hits0).sum())} face ids differ"
    assert np.array_equal(rgb1.view(np.uint32), rgb0.view(np.uint32)), float(np.abs(rgb1 - rgb0).max())
    assert counters(st1) == counters(st0)
    if which == "mixed":
        assert st0.rays_bounce > 0
    named = {"trace_units": prof[13], "units": prof[RT_WORK_SHADOW + 13], "shaft_groups": prof[RT_WORK_SHADOW + 88],
             "beams_tested": prof[RT_WORK_SHADOW + 76]}
    for k in expect:
        assert named[k] > 0, (k, {n: int(v) for n, v in named.items()})
    # only the step counters write: the words between and behind the two regions of Control::prof stay what the frame's memset left
    outside = np.r_[96:RT_WORK_SHADOW, RT_WORK_SHADOW + 96:768]
    assert not prof[outside].any(), {int(i): int(prof[i]) for i in outside[prof[outside] != 0][:8]}


# ------------------------------------------------------------------------------------------ k_resolve's 8-bit frame
def render_device(rt, ctx, cam, L, w, h, depth, rgb=True, stripe=1, rank=0, nranks=1):
    import torch
    p = rt.make_params(w, h, depth, 0, h, stripe, rank, nranks)
    n = ctx.lib.rt_local_rows(C.byref(p)) * w * 3
    d_rgb = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda") if rgb else None
    d_u8 = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = ctx.lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(d_rgb.data_ptr()) if rgb else None,
                                  C.c_void_p(d_u8.data_ptr()), None, None, None)
    rt.capi.check(ctx.lib, ctx.handle, st, "rt_render_device")
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_synchronize(ctx.handle), "rt_synchronize")
    return (d_rgb.cpu().numpy() if rgb else None), d_u8.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("which,lights,grid,depth", [("cube.obj", 1, 8, 4), ("dodgeColorTest.obj", 1, 8, 2), ("mixed", 3, 5, 4), ("mixed", 8, 2, 4)])
def test_u8_frame_is_the_quantised_float_frame(rt, oracle, tmp_path, which, lights, grid, depth):
    """d_out_u8 == clip(min(255, trunc(255 * rgb)), 0) of the float frame of the same launch, and the oracle's writePPMImage quantisation.
    The mixed scene under eight lights (the three of the other tests and five more) drives channels past 1: the saturation branch."""
    pts = list(THREE) + [(1.5, 1.5, 0.5), (-1.5, 0.8, -1.0), (0.0, 2.0, 0.0), (1.0, -0.5, 2.0), (-0.5, 1.2, 1.8)]
    path, yaw = scene(rt, which, tmp_path)
    hs = rt.HostScene(path, 1000, 15)
    ctx = rt.Context(0)
    ctx.upload(hs)
    w, h = 200, 136
    rgb, u8 = render_device(rt, ctx, rt.default_camera(w, h, yaw), rt.make_lights(points=pts[:lights], area=True, usteps=grid, vsteps=grid), w, h, depth)
    ctx.close(); hs.close()
    assert not np.isnan(rgb).any()
    want = quantise_u8(rgb)
    assert np.array_equal(u8, want.reshape(-1)), f"{int((u8 != want.reshape(-1)).sum())} bytes differ"
    assert np.array_equal(np.clip(oracle.quantise(rgb), 0, None).astype(np.uint8), want)
    assert (u8 > 0).mean() > 0.02
    if lights == 8:
        assert (rgb >= 1).any() and (u8 == 255).any(), "the eight-light frame must saturate some channel"


def test_u8_ppm_writer_equals_the_float_writer(rt, tmp_path):
    """rt_write_ppm_u8 of the quantised frame is byte for byte rt_write_ppm of the float frame (values in [0, 1] and above: the float writer
    leaves negatives unclamped, the 8-bit frame cannot hold them)."""
    lib = rt.load_library()
    rng = np.random.default_rng(5)
    h, w = 7, 11
    rgb = rng.uniform(0, 1.2, (h, w, 3)).astype(np.float32)
    rgb.reshape(-1)[:8] = np.array([0.0, 1.0, 1.0 / 255, np.nextafter(np.float32(1.0 / 255), np.float32(0)), 254.5 / 255, 2.0, 1.0e3, 0.999], np.float32)
    a, b = tmp_path / "f.ppm", tmp_path / "u.ppm"
    assert lib.rt_write_ppm(str(a).encode(), rgb.ctypes.data_as(C.c_void_p), w, h) == 0
    u8 = np.ascontiguousarray(quantise_u8(rgb))
    assert lib.rt_write_ppm_u8(str(b).encode(), u8.ctypes.data_as(C.c_void_p), w, h) == 0
    assert a.read_bytes() == b.read_bytes()
    text = b.read_bytes().decode().split("\n")
    assert text[:3] == ["P3", f"{w} {h}", "255"]
    rows = text[3:]
    assert rows[-1] == "" and len(rows) == h + 1
    assert [int(x) for r in rows[:-1] for x in r.split()] == u8.reshape(-1).tolist()
    assert lib.rt_write_ppm_u8(str(tmp_path / "nodir" / "x.ppm").encode(), u8.ctypes.data_as(C.c_void_p), w, h) == rt.capi.RT_ERR_IO
    assert lib.rt_write_ppm_u8(str(b).encode(), u8.ctypes.data_as(C.c_void_p), 0, h) == rt.capi.RT_ERR_INVALID


# ------------------------------------------------------------------------------------------ the reference's md5s through the 8-bit path
def known_md5(scene_name, size, area):
    want = [c["md5"] for c in KA["result_ppm_md5"] if c["scene"] == scene_name and c["size"] == size and c["area"] == area]
    assert len(want) == 1
    return want[0]


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,size,area", [("cube.obj", 1000, 0), ("cube.obj", 1000, 1), ("cube.obj", 1440, 1), ("dodgeColorTest.obj", 1440, 1)])
def test_reference_md5_through_the_u8_output(rt, tmp_path, scene_name, size, area):
    """rt_render_device (8-bit output only) + rt_write_ppm_u8 at the reference's settings: result.ppm hashes to the reference's md5."""
    hs = rt.HostScene(os.path.join(SCENES, scene_name), 1000, 15)
    ctx = rt.Context(0)
    ctx.upload(hs)
    _, u8 = render_device(rt, ctx, rt.default_camera(size, size), rt.make_lights(area=bool(area), usteps=5, vsteps=5), size, size, -1, rgb=False)
    ctx.close(); hs.close()
    out = tmp_path / "result.ppm"
    assert ctx.lib.rt_write_ppm_u8(str(out).encode(), u8.ctypes.data_as(C.c_void_p), size, size) == 0
    assert hashlib.md5(out.read_bytes()).hexdigest() == known_md5(scene_name, size, area)


@pytest.mark.gpu
def test_reference_md5_through_eight_row_ranks(rt, tmp_path):
    """The multi-GPU output path on one GPU: eight ranks render their interleaved 8-row stripes (rt_params.stripe/rank/nranks), the 8-bit
    blocks are laid out as a gather would leave them, rt_stitch_rows de-interleaves and rt_write_ppm_u8 writes the reference's file."""
    scene_name, size, n = "dodgeColorTest.obj", 1440, 8
    hs = rt.HostScene(os.path.join(SCENES, scene_name), 1000, 15)
    ctx = rt.Context(0)
    ctx.upload(hs)
    cam, L = rt.default_camera(size, size), rt.make_lights(area=True, usteps=5, vsteps=5)
    blocks = [render_device(rt, ctx, cam, L, size, size, -1, rgb=False, stripe=8, rank=r, nranks=n)[1] for r in range(n)]
    ctx.close(); hs.close()
    block_bytes = max(b.size for b in blocks)
    assert {b.size for b in blocks} == {23 * 8 * size * 3, 22 * 8 * size * 3}          # 180 stripes over 8 ranks
    gathered = np.zeros(n * block_bytes, np.uint8)
    for r, b in enumerate(blocks):
        gathered[r * block_bytes:r * block_bytes + b.size] = b
    frame = np.zeros(size * size * 3, np.uint8)
    lib = rt.load_library()
    assert lib.rt_stitch_rows(gathered.ctypes.data_as(C.c_void_p), block_bytes, size, size, 8, n, frame.ctypes.data_as(C.c_void_p)) == 0
    out = tmp_path / "result.ppm"
    assert lib.rt_write_ppm_u8(str(out).encode(), frame.ctypes.data_as(C.c_void_p), size, size) == 0
    assert hashlib.md5(out.read_bytes()).hexdigest() == known_md5(scene_name, size, 1)


# ------------------------------------------------------------------------------------------ full-size culling
@pytest.mark.gpu
def test_full_size_culling_equals_no_cull(rt, monkeypatch):
    """dodgeColorTest.obj at 1920 x 1080, depth 4, 8 x 8 samples: every culling device on (the default) and off (RT_NO_CULL=1) give the
    same face ids and RGB bits."""
    w, h = 1920, 1080
    hs = rt.HostScene(os.path.join(SCENES, "dodgeColorTest.obj"), 1000, 15)
    cam, L = rt.default_camera(w, h), rt.make_lights(area=True, usteps=8, vsteps=8)
    frames = []
    for no_cull in (False, True):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        if no_cull:
            monkeypatch.setenv("RT_NO_CULL", "1")
        ctx = rt.Context(0)
        ctx.upload(hs)
        p = rt.make_params(w, h, 4)
        rgb = np.zeros((h, w, 3), np.float32)
        hits = np.zeros((h, w), np.int32)
        st = rt.capi.rt_stats()
        rc = ctx.lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), C.byref(st))
        rt.capi.check(ctx.lib, ctx.handle, rc, "rt_render")
        ctx.close()
        frames.append((rgb, hits, st))
    hs.close()
    (rgb0, hits0, st0), (rgb1, hits1, st1) = frames
    assert (hits0 >= 0).sum() > 0.1 * hits0.size
    assert np.array_equal(hits0, hits1), f"{int((hits0 != hits1).sum())} face ids differ"
    assert np.array_equal(rgb0.view(np.uint32), rgb1.view(np.uint32)), float(np.abs(rgb0 - rgb1).max())
    assert counters(st0) == counters(st1)
