"""Thin-lens depth of field (rt_set_lens, rt_lens_table) at the C ABI, the binding and the front ends, and the numpy restatement the GPU
tests build their rays with (tests/lens_ref.py) -- everything that needs no device."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import lens_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")


def test_header_declares_the_lens():
    text = open(HEADER).read()
    assert re.search(r"^#define\s+RT_LENS_ROTATIONS\s+64\b", text, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\brt_status\s+rt_set_lens\s*\(\s*rt_ctx\s*\*\s*ctx\s*,\s*float\s+aperture\s*,\s*float\s+focus\s*\)\s*;", code)
    assert re.search(r"\brt_status\s+rt_lens_table\s*\(\s*int32_t\s+n\s*,\s*float\s*\*\s*out\s*\)\s*;", code)


def test_binding_has_the_symbols_with_their_argtypes(rt):
    sig = {name: (res, args) for name, res, args in rt.capi._SIGNATURES}
    assert sig["rt_set_lens"] == (C.c_int, [C.c_void_p, C.c_float, C.c_float])
    assert sig["rt_lens_table"] == (C.c_int, [C.c_int32, C.POINTER(C.c_float)])
    assert "rt_set_lens" in rt.capi.EXPORTED_SYMBOLS and "rt_lens_table" in rt.capi.EXPORTED_SYMBOLS
    assert rt.capi.RT_LENS_ROTATIONS == 64 == lens_ref.RT_LENS_ROTATIONS
    lib = rt.load_library()
    assert lib.rt_set_lens.argtypes == [C.c_void_p, C.c_float, C.c_float] and lib.rt_set_lens.restype is C.c_int
    assert lib.rt_lens_table.argtypes == [C.c_int32, C.POINTER(C.c_float)] and lib.rt_lens_table.restype is C.c_int


@pytest.mark.parametrize("aperture,focus", [(0.0, 2.0), (0.08, 2.0), (-1.0, 2.0), (float("nan"), 2.0), (0.08, 0.0), (0.08, float("inf"))])
def test_null_context_is_invalid_without_a_device(rt, aperture, focus):
    assert rt.load_library().rt_set_lens(None, aperture, focus) == rt.capi.RT_ERR_INVALID


def test_lens_table_rejects_bad_arguments(rt):
    lib = rt.load_library()
    buf = np.full(lens_ref.RT_LENS_ROTATIONS * 25 * 2, 7.0, np.float32)
    for n in (0, -1, 5, 100):
        assert lib.rt_lens_table(n, buf.ctypes.data_as(C.POINTER(C.c_float))) == rt.capi.RT_ERR_INVALID
    assert (buf == 7.0).all()
    assert lib.rt_lens_table(2, None) == rt.capi.RT_ERR_INVALID


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_lens_table_is_the_rotated_concentric_grid(rt, n):
    T = lens_ref.library_table(rt.load_library(), n)
    assert np.isfinite(T).all()
    assert ((T.astype(np.float64) ** 2).sum(axis=-1) <= 1.0 + 1e-6).all()
    want = lens_ref.lens_table_double(n)
    w32 = want.astype(np.float32)
    ulp = np.maximum(np.spacing(np.abs(w32)), np.float32(1e-45))
    assert (np.abs(T.astype(np.float64) - want) <= ulp.astype(np.float64)).all(), "within one float ulp of the double restatement"
    for r in range(lens_ref.RT_LENS_ROTATIONS):
        a = (math.pi / 2.0) * r / lens_ref.RT_LENS_ROTATIONS
        x, y = T[0, :, 0].astype(np.float64), T[0, :, 1].astype(np.float64)
        rot = np.stack([x * math.cos(a) - y * math.sin(a), x * math.sin(a) + y * math.cos(a)], axis=-1)
        assert np.abs(T[r] - rot).max() <= 1e-6, r
    if n == 1:
        assert (T == 0.0).all()
    else:
        assert len({tuple(p) for p in T[0]}) == n * n, "n*n distinct lens points"
        assert len({T[r].tobytes() for r in range(lens_ref.RT_LENS_ROTATIONS)}) == lens_ref.RT_LENS_ROTATIONS, "64 different patterns"
    if n % 2 == 1:
        assert (T[:, (n * n) // 2] == 0.0).all(), "the centre cell maps to the lens centre"


def test_hash_values_of_the_header_comment():
    text = open(HEADER).read()
    listed = re.findall(r"h\((\d+), (\d+)\) = 0x([0-9A-Fa-f]{8})", text)
    assert len(listed) >= 5
    for i, j, h in listed:
        assert lens_ref.lens_hash(int(i), int(j)) == int(h, 16), (i, j)
    ii, jj = np.meshgrid(np.arange(40), np.arange(30), indexing="xy")
    arr = lens_ref.lens_hash_array(ii, jj)
    assert all(int(arr[j, i]) == lens_ref.lens_hash(i, j) for i in (0, 1, 17, 39) for j in (0, 5, 29))
    assert len(set((arr >> np.uint64(26)).reshape(-1).tolist())) == 64, "every rotation occurs in a small frame"


def test_rotation_and_point_ranges():
    for n in (1, 2, 3, 4):
        ks = set()
        for i in range(16):
            for j in range(16):
                per_pixel = [lens_ref.rotation_and_point(i, j, sx, sy, n) for sy in range(n) for sx in range(n)]
                assert len({r for r, _ in per_pixel}) == 1 and 0 <= per_pixel[0][0] < 64
                assert sorted(k for _, k in per_pixel) == list(range(n * n)), "a pixel's sub-samples use every lens point once"
                ks.add(per_pixel[0][1])
        assert ks == set(range(n * n)), "the cyclic shift varies from pixel to pixel"


def test_lens_rays_array_form_equals_the_scalar_form():
    rng = np.random.default_rng(5)
    n, H, W = 3, 4, 5
    T = lens_ref.lens_table_double(n).astype(np.float32)
    S = rng.standard_normal((H, W, n, n, 3)).astype(np.float32)
    c = np.array([0.1, -0.2, 2.0], np.float32)
    m = rng.standard_normal(12).astype(np.float32)
    rows = [7, 8, 20, 21]
    O, P, D = lens_ref.lens_rays(S, c, m, 0.08, 1.5, T, n, rows=rows)
    for lr, j in enumerate(rows):
        for i in range(W):
            for sy in range(n):
                for sx in range(n):
                    r, k = lens_ref.rotation_and_point(i, j, sx, sy, n)
                    o, p, d = lens_ref.lens_ray(S[lr, i, sy, sx], c, m, 0.08, 1.5, T[r, k])
                    assert np.array_equal(o, O[lr, i, sy, sx]) and np.array_equal(p, P[lr, i, sy, sx]) and np.array_equal(d, D[lr, i, sy, sx])
    assert np.array_equal(D, (P - O).astype(np.float32))


def test_cli_usage_names_the_flag_and_rejects_bad_lenses():
    assert os.path.exists(RT_RENDER), "rt_render is part of `make all`"
    bad = subprocess.run([RT_RENDER, "--bogus"], capture_output=True, timeout=60)
    assert bad.returncode == 2 and b"--lens APERTURE FOCUS" in bad.stderr
    for a, f in (("nan", "2"), ("abc", "2"), ("0.1x", "2"), ("", "2"), ("-0.1", "2"), ("inf", "2"), ("0.1", "0"), ("0.1", "-1"), ("0.1", "nan"),
                 ("0.1", "inf"), ("0.1", "")):
        r = subprocess.run([RT_RENDER, "--aa", "2", "--lens", a, f], capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--lens" in r.stderr, (a, f)
    r = subprocess.run([RT_RENDER, "--lens", "0.1"], capture_output=True, timeout=60)
    assert r.returncode == 2


def test_flyscene_default_is_the_pinhole(rt):
    fs = rt.Flyscene()
    assert fs.aperture == 0.0 and fs.focus > 0.0
    assert hasattr(rt.Context, "set_lens")
