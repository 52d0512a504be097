"""Device ray queries, the parts that need no GPU: the five entry points are declared, bound and exported, refuse a NULL context, and the
two host ray generators of rays.py do what their docstrings define."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rt_closest_hits_device", "rt_closest_hits", "rt_light_strikes_device", "rt_trace_rays_device", "rt_set_query_chunk"]


def test_header_declares_the_query_calls():
    text = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    assert "device ray queries" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\brt_status\s+" + name + r"\s*\(", code), name


def test_binding_and_library_hold_the_query_calls(rt):
    lib = rt.load_library()
    for name in NAMES:
        assert name in rt.capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name


def test_null_context_is_invalid(rt):
    lib = rt.load_library()
    buf = (C.c_float * 6)()
    p = C.cast(buf, C.c_void_p)
    L = rt.capi.rt_lights()
    lib.rt_default_lights(C.byref(L), 1)
    inv = rt.capi.RT_ERR_INVALID
    assert lib.rt_closest_hits_device(None, 1, p, p, p, p, None) == inv
    assert lib.rt_closest_hits(None, 1, p, p, p, p) == inv
    assert lib.rt_light_strikes_device(None, 1, p, p, p, None) == inv
    assert lib.rt_trace_rays_device(None, C.byref(L), 0, 1, p, p, p, None, None, None) == inv
    assert lib.rt_set_query_chunk(None, 1 << 20) == inv
    # ... also with n = 0, which a context would accept
    assert lib.rt_closest_hits_device(None, 0, None, None, None, None, None) == inv
    assert lib.rt_trace_rays_device(None, C.byref(L), 0, 0, None, None, None, None, None, None) == inv


W, H = 5, 3


def test_orthographic_rays(rt):
    f = np.float32
    cam = rt.default_camera(W, H, 0.4)
    half = 0.75
    o, d = rt.rays.orthographic_rays(cam, W, H, half)
    assert o.shape == (W * H, 3) and d.shape == (W * H, 3) and o.dtype == np.float32 and d.dtype == np.float32
    assert (d.view(np.uint32) == d.view(np.uint32)[0]).all(), "all directions are one vector, bit for bit"
    m = np.asarray(list(cam.inv_view), f).reshape(3, 4)
    assert np.array_equal(d[0].view(np.uint32), (-m[:, 2]).view(np.uint32))
    assert abs(float(np.linalg.norm(d[0].astype(np.float64))) - 1.0) < 1e-6          # (a rigid camera: the view axis has unit length)

    def origin(i, j):                  # the docstring, one pixel at a time
        n0 = f(2.0 * i / W - 1.0)
        n1 = f(1.0 - 2.0 * j / H)
        x = n0 * (f(f(W) / f(H)) * f(half))
        y = n1 * f(half)
        return np.array([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * f(-1.0)) + m[r, 3] for r in range(3)], f)

    for i in range(W):
        assert np.array_equal(o[i].view(np.uint32), origin(i, 0).view(np.uint32)), ("row 0", i)
    for j in range(H):
        assert np.array_equal(o[j * W].view(np.uint32), origin(0, j).view(np.uint32)), ("column 0", j)
    # the default pose: the window is centred on the view axis' foot point (0, 0, 1), half_height high at the top edge, x grows with i
    cam0 = rt.default_camera(W, H)
    o0, d0 = rt.rays.orthographic_rays(cam0, W, H, half)
    assert np.array_equal(d0[0], np.array([0, 0, -1], f))
    assert np.array_equal(o0[0], np.array([-f(f(W) / f(H)) * f(half), f(half), 1.0], f))
    assert (np.diff(o0.reshape(H, W, 3)[0, :, 0]) > 0).all() and (np.diff(o0.reshape(H, W, 3)[:, 0, 1]) < 0).all()


def test_panorama_rays(rt):
    c = (0.25, -0.5, 1.5)
    o, d = rt.rays.panorama_rays(c, W, H)
    assert o.shape == (W * H, 3) and d.shape == (W * H, 3) and o.dtype == np.float32 and d.dtype == np.float32
    assert (o == np.asarray(c, np.float32)).all()
    # three float32 roundings of a unit vector's components move its length by at most 2^-24 (+ the double arithmetic, far below): 2 ulp of 1.0f
    norm = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(norm - 1.0).max() <= 2.0 * float(np.spacing(np.float32(1.0)))

    def direction(i, j):               # the docstring, one pixel at a time
        lon = 2.0 * np.pi * (i + 0.5) / W - np.pi
        lat = np.pi * (j + 0.5) / H
        v = np.array([np.sin(lat) * np.sin(lon), np.cos(lat), -np.sin(lat) * np.cos(lon)])
        return (v / np.sqrt((v * v).sum())).astype(np.float32)

    for i in range(W):
        assert np.array_equal(d[i], direction(i, 0)), ("row 0", i)
    for j in range(H):
        assert np.array_equal(d[j * W], direction(0, j)), ("column 0", j)
    mid = d.reshape(H, W, 3)[H // 2, W // 2]                  # the middle pixel of an odd frame looks along -z
    assert abs(float(mid[0])) < 1e-6 and abs(float(mid[1])) < 1e-6 and mid[2] < -0.999999
    assert d.reshape(H, W, 3)[0, :, 1].min() > 0 and d.reshape(H, W, 3)[H - 1, :, 1].max() < 0
