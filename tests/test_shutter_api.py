"""Camera motion blur (rt_set_shutter, rt_graph_launch_shutter, rt_shutter_time, rt_shutter_camera) at the C ABI, the binding and the
front ends, and the numpy restatement the GPU tests build their rays with (tests/shutter_ref.py) -- everything that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lens_ref
import shutter_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")
F = np.float32


def lib_time(lib, n, i, j, sx, sy):
    t = C.c_float(-1.0)
    assert lib.rt_shutter_time(n, i, j, sx, sy, C.byref(t)) == 0
    return F(t.value)


def random_camera(rt, rng, scale=2.0):
    cam = rt.default_camera(64, 48)
    for k in range(3):
        cam.center[k] = float(F(rng.standard_normal() * scale))
    for k in range(12):
        cam.inv_view[k] = float(F(rng.standard_normal() * scale))
    return cam


def cam_bits(cam):
    return bytes(cam)


def test_header_declares_the_shutter():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\brt_status\s+rt_set_shutter\s*\(\s*rt_ctx\s*\*\s*ctx\s*,\s*const\s+rt_camera\s*\*\s*close\s*\)\s*;", code)
    assert re.search(r"\brt_status\s+rt_graph_launch_shutter\s*\(\s*rt_graph\s*\*\s*g\s*,\s*const\s+rt_camera\s*\*\s*open\s*,\s*const\s+rt_camera\s*\*\s*close\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", code)
    assert re.search(r"\brt_status\s+rt_shutter_time\s*\(\s*int32_t\s+n\s*,\s*uint32_t\s+i\s*,\s*uint32_t\s+j\s*,\s*int32_t\s+sx\s*,\s*int32_t\s+sy\s*,"
                     r"\s*float\s*\*\s*t\s*\)\s*;", code)
    assert re.search(r"\brt_status\s+rt_shutter_camera\s*\(\s*const\s+rt_camera\s*\*\s*open\s*,\s*const\s+rt_camera\s*\*\s*close\s*,\s*float\s+t\s*,"
                     r"\s*rt_camera\s*\*\s*out\s*\)\s*;", code)


def test_binding_has_the_symbols_with_their_argtypes(rt):
    sig = {name: (res, args) for name, res, args in rt.capi._SIGNATURES}
    cam = C.POINTER(rt.capi.rt_camera)
    want = {
        "rt_set_shutter": (C.c_int, [C.c_void_p, cam]),
        "rt_graph_launch_shutter": (C.c_int, [C.c_void_p, cam, cam, C.c_void_p]),
        "rt_shutter_time": (C.c_int, [C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
        "rt_shutter_camera": (C.c_int, [cam, cam, C.c_float, cam]),
    }
    lib = rt.load_library()
    for name, (res, args) in want.items():
        assert sig[name] == (res, args), name
        assert name in rt.capi.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert hasattr(rt.Context, "set_shutter")
    assert "close" in rt.FrameGraph.launch.__code__.co_varnames


@pytest.mark.parametrize("poison", [None, 0.0, float("nan"), float("inf")])
def test_null_context_is_invalid_without_a_device(rt, poison):
    lib = rt.load_library()
    if poison is None:
        assert lib.rt_set_shutter(None, None) == rt.capi.RT_ERR_INVALID
        return
    cam = rt.default_camera(64, 48, 0.05)
    cam.inv_view[5] = poison
    assert lib.rt_set_shutter(None, C.byref(cam)) == rt.capi.RT_ERR_INVALID


def test_host_functions_reject_bad_arguments(rt):
    lib, inv = rt.load_library(), rt.capi.RT_ERR_INVALID
    t = C.c_float(7.0)
    for n, sx, sy in ((0, 0, 0), (5, 0, 0), (-1, 0, 0), (2, 2, 0), (2, 0, 2), (2, -1, 0), (3, 0, -1), (1, 1, 0)):
        assert lib.rt_shutter_time(n, 3, 4, sx, sy, C.byref(t)) == inv, (n, sx, sy)
    assert t.value == 7.0
    assert lib.rt_shutter_time(2, 3, 4, 0, 0, None) == inv
    a, b, out = rt.default_camera(64, 48), rt.default_camera(64, 48, 0.1), rt.capi.rt_camera()
    assert lib.rt_shutter_camera(None, C.byref(b), 0.5, C.byref(out)) == inv
    assert lib.rt_shutter_camera(C.byref(a), None, 0.5, C.byref(out)) == inv
    assert lib.rt_shutter_camera(C.byref(a), C.byref(b), 0.5, None) == inv
    assert lib.rt_graph_launch_shutter(None, C.byref(a), C.byref(b), None) == inv


def test_scramble_values_of_the_header_comment():
    text = open(HEADER).read()
    listed = re.findall(r"g\((\d+), (\d+)\) = 0x([0-9A-Fa-f]{8})", text)
    assert len(listed) >= 5
    for i, j, g in listed:
        assert shutter_ref.shutter_g(int(i), int(j)) == int(g, 16), (i, j)
    pins = {(0, 0): 0x18FEA250, (1, 0): 0x83B87A41, (0, 1): 0x0B4F00CA, (7, 3): 0xE22EC469, (1919, 1079): 0x67E7315C}
    for (i, j), g in pins.items():
        assert shutter_ref.shutter_g(i, j) == g
        assert shutter_ref.shutter_g(i, j) == int(shutter_ref.shutter_g_array(i, j))


def test_time_pins(rt):
    lib = rt.load_library()
    for (i, j, n, sx, sy), (slot, t) in {(7, 3, 3, 1, 0): (1, 0.20927937), (1919, 1079, 4, 3, 2): (10, 0.6503668), (0, 0, 1, 0, 0): (0, 0.09762573)}.items():
        s, u, tt = shutter_ref.slot_u_t(i, j, sx, sy, n)
        assert s == slot and tt == F(t), (i, j, n, s, tt)
        assert lib_time(lib, n, i, j, sx, sy) == F(t)
        assert 0.0 <= float(u) < 1.0


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_shutter_time_equals_the_restatement(rt, n):
    lib = rt.load_library()
    W, H = 40, 30
    arr = shutter_ref.shutter_times(W, n, np.arange(H))
    shifts = set()
    for j in range(H):
        for i in range(W):
            slots = []
            for sy in range(n):
                for sx in range(n):
                    slot, u, t = shutter_ref.slot_u_t(i, j, sx, sy, n)
                    got = lib_time(lib, n, i, j, sx, sy)
                    assert got.view(np.uint32) == t.view(np.uint32) == arr[j, i, sy, sx].view(np.uint32), (i, j, sx, sy)
                    assert 0.0 <= float(t) < 1.0
                    assert int(np.floor(float(t) * n * n)) == slot
                    slots.append(slot)
            assert sorted(slots) == list(range(n * n)), "a pixel's sub-samples take every time slot once"
            shifts.add(slots[0])
    assert shifts == set(range(n * n)), "the cyclic shift varies from pixel to pixel"


def test_times_fill_the_exposure_evenly():
    for n in (1, 2, 3, 4):
        t = shutter_ref.shutter_times(64, n, np.arange(64)).astype(np.float64).reshape(-1)
        assert t.min() >= 0.0 and t.max() < 1.0
        hist = np.histogram(t, bins=8, range=(0.0, 1.0))[0]
        assert np.abs(hist / (t.size / 8.0) - 1.0).max() <= 0.07, (n, hist)
    # time slots and lens points of a pixel's sub-samples are not one cyclic shift of each other (sx*n + sy against sy*n + sx)
    n, differs = 3, 0
    for i in range(8):
        for j in range(8):
            d = {(shutter_ref.slot_u_t(i, j, sx, sy, n)[0] - lens_ref.rotation_and_point(i, j, sx, sy, n)[1]) % (n * n) for sy in range(n) for sx in range(n)}
            differs += len(d) > 1
    assert differs == 64


def test_shutter_camera_equals_the_numpy_blend(rt):
    lib = rt.load_library()
    rng = np.random.default_rng(11)
    out = rt.capi.rt_camera()
    for k in range(1200):
        a, b = random_camera(rt, rng), random_camera(rt, rng)
        if k % 3 == 0:                                   # some values do not move: the d == 0 branch, with both zero signs
            for q in rng.integers(0, 12, 4):
                b.inv_view[q] = a.inv_view[q]
            a.center[1], b.center[1] = -0.0, 0.0
        b.fovy, b.aspect = 17.0, 3.0                     # never looked at
        t = float(F(rng.random())) if k % 7 else float(shutter_ref.shutter_time(k, k // 3, 0, 0, 1))
        assert lib.rt_shutter_camera(C.byref(a), C.byref(b), t, C.byref(out)) == 0
        want = shutter_ref.shutter_pose(shutter_ref.pose(a), shutter_ref.pose(b), F(t))
        assert np.array_equal(shutter_ref.pose(out).view(np.uint32), want.view(np.uint32)), k
        assert out.fovy == a.fovy and out.aspect == a.aspect and list(out.viewport) == list(a.viewport)
        assert cam_bits(shutter_ref.shutter_camera(a, b, t)) == cam_bits(out)


def test_still_shutter_is_the_open_camera_bit_for_bit(rt):
    lib = rt.load_library()
    a = rt.default_camera(200, 136, 0.3)
    for q in (1, 4, 6, 9):
        a.inv_view[q] = -0.0
    a.center[1] = -0.0
    same = rt.capi.rt_camera.from_buffer_copy(bytes(a))
    for t in (0.0, 0.25, 0.9999999, float(shutter_ref.shutter_time(7, 3, 1, 0, 3))):
        out = rt.capi.rt_camera()
        assert lib.rt_shutter_camera(C.byref(a), C.byref(same), t, C.byref(out)) == 0
        assert cam_bits(out) == cam_bits(a), t
        assert lib.rt_shutter_camera(C.byref(a), C.byref(same), t, C.byref(a)) == 0, "out may alias open"
        assert cam_bits(a) == cam_bits(same)
    k = shutter_ref.shutter_pose(shutter_ref.pose(a), shutter_ref.pose(same), F(0.4))
    assert np.array_equal(k.view(np.uint32), shutter_ref.pose(a).view(np.uint32))


def test_array_forms_equal_the_scalar_forms():
    rng = np.random.default_rng(5)
    n, W = 3, 5
    rows = [7, 8, 20, 21]
    open15, close15 = rng.standard_normal(15).astype(F), rng.standard_normal(15).astype(F)
    close15[[2, 6, 9]] = open15[[2, 6, 9]]
    n0, n1 = rng.standard_normal((len(rows), W, n, n)).astype(F), rng.standard_normal((len(rows), W, n, n)).astype(F)
    T = lens_ref.lens_table_double(n).astype(F)
    for lens in (None, (0.08, 1.5, T)):
        O, P, D = shutter_ref.shutter_rays(n0, n1, open15, close15, n, rows, lens=lens)
        for lr, j in enumerate(rows):
            for i in range(W):
                for sy in range(n):
                    for sx in range(n):
                        K = shutter_ref.shutter_pose(open15, close15, shutter_ref.shutter_time(i, j, sx, sy, n))
                        S = shutter_ref.screen_points(K[3:15], n0[lr, i, sy, sx], n1[lr, i, sy, sx])
                        r, k = lens_ref.rotation_and_point(i, j, sx, sy, n)
                        o, p, d = shutter_ref.shutter_ray(S, K, lens=lens, lens_point=T[r, k])
                        idx = (lr, i, sy, sx)
                        assert np.array_equal(o, O[idx]) and np.array_equal(p, P[idx]) and np.array_equal(d, D[idx]), (lens is not None, idx)
        assert np.array_equal(D, (P - O).astype(F))


def test_screen_points_is_the_last_step_of_screen_to_world(oracle):
    """the numpy 3 x 4 product, fed with the raster terms an identity inv_view exposes, against the checker's screenToWorld"""
    w, h = 61, 47
    ident = oracle.camera(w, h)
    for k in range(12):
        ident.inv_view[k] = 1.0 if k in (0, 5, 10) else 0.0
    rng = np.random.default_rng(3)
    checked = 0
    for yaw in (0.0, 0.05, -0.7):
        cam = oracle.camera(w, h, yaw)
        for k in (3, 7, 11):
            cam.inv_view[k] += float(F(rng.standard_normal() * 0.3))
        m = np.array(list(cam.inv_view), F)
        for _ in range(1100):
            x, y = float(F(rng.uniform(-2, w + 2))), float(F(rng.uniform(-2, h + 2)))
            n01 = oracle.screen_to_world(ident, x, y)
            assert n01[2] == F(-1.0)
            got = shutter_ref.screen_points(m, n01[0], n01[1])
            assert np.array_equal(got.view(np.uint32), oracle.screen_to_world(cam, x, y).view(np.uint32)), (yaw, x, y)
            checked += 1
    assert checked >= 3000


def test_cli_usage_names_the_flag_and_rejects_bad_yaws():
    assert os.path.exists(RT_RENDER), "rt_render is part of `make all`"
    bad = subprocess.run([RT_RENDER, "--bogus"], capture_output=True, timeout=60)
    assert bad.returncode == 2 and b"--shutter YAW" in bad.stderr
    for flag in (b"--scene", b"--size W H", b"--samples U V", b"--depth D", b"--aa N", b"--aa-threshold T", b"--lens APERTURE FOCUS", b"--out"):
        assert flag in bad.stderr, flag
    for yaw in ("nan", "inf", "-inf", "abc", "0.05x", ""):
        r = subprocess.run([RT_RENDER, "--aa", "2", "--shutter", yaw], capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--shutter" in r.stderr, yaw
    r = subprocess.run([RT_RENDER, "--aa", "2", "--shutter"], capture_output=True, timeout=60)
    assert r.returncode == 2 and b"--shutter" in r.stderr, "a missing value"


def test_flyscene_default_is_the_still_camera(rt):
    assert rt.Flyscene().shutter_close is None
