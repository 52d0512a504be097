"""Adaptive supersampling (rt_set_supersampling_threshold, rt_supersampling_refined) at the C ABI, the binding and the front ends, and the
float32 refine rule the GPU tests build their expected frames with -- everything that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from adaptive_ref import refine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")


def test_header_declares_both_functions():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\brt_status\s+rt_set_supersampling_threshold\s*\(\s*rt_ctx\s*\*\s*ctx\s*,\s*float\s+threshold\s*\)\s*;", code)
    assert re.search(r"\brt_status\s+rt_supersampling_refined\s*\(\s*rt_ctx\s*\*\s*ctx\s*,\s*uint64_t\s*\*\s*refined\s*\)\s*;", code)


def test_binding_has_the_symbols_with_their_argtypes(rt):
    sig = {name: (res, args) for name, res, args in rt.capi._SIGNATURES}
    assert sig["rt_set_supersampling_threshold"] == (C.c_int, [C.c_void_p, C.c_float])
    assert sig["rt_supersampling_refined"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)])
    lib = rt.load_library()
    assert lib.rt_set_supersampling_threshold.argtypes == [C.c_void_p, C.c_float]
    assert lib.rt_set_supersampling_threshold.restype is C.c_int
    assert lib.rt_supersampling_refined.argtypes == [C.c_void_p, C.POINTER(C.c_uint64)]
    assert lib.rt_supersampling_refined.restype is C.c_int


@pytest.mark.parametrize("tau", [-1.0, 0.0, 0.05, float("inf"), float("nan")])
def test_null_context_is_invalid_without_a_device(rt, tau):
    lib = rt.load_library()
    assert lib.rt_set_supersampling_threshold(None, tau) == rt.capi.RT_ERR_INVALID
    out = C.c_uint64(7)
    assert lib.rt_supersampling_refined(None, C.byref(out)) == rt.capi.RT_ERR_INVALID
    assert out.value == 7


def test_cli_usage_names_the_flag_and_rejects_bad_thresholds():
    assert os.path.exists(RT_RENDER), "rt_render is part of `make all`"
    bad = subprocess.run([RT_RENDER, "--bogus"], capture_output=True, timeout=60)
    assert bad.returncode == 2 and b"--aa-threshold T" in bad.stderr
    for t in ("nan", "NaN", "abc", "0.1x", ""):
        r = subprocess.run([RT_RENDER, "--aa", "2", "--aa-threshold", t], capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--aa-threshold" in r.stderr, t


def test_flyscene_default_is_the_regular_frame(rt):
    fs = rt.Flyscene()
    assert fs.supersample == 1
    assert fs.supersample_threshold < 0


# ------------------------------------------------------------------------------------------ the numpy rule itself
def test_refine_3x3_single_bright_pixel():
    c = np.zeros((3, 3, 3), np.float32)
    c[1, 1, 2] = 0.5
    want = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
    assert np.array_equal(refine(c, 0.0), want)
    assert np.array_equal(refine(c, 0.4999), want)
    assert not refine(c, 0.5).any(), "a difference equal to tau does not refine"
    assert not refine(c, np.inf).any()


def test_refine_1xN_and_Nx1():
    row = np.zeros((1, 7, 3), np.float32)
    row[0, 3, 0] = 1.0
    assert np.array_equal(refine(row, 0.1)[0], np.array([0, 0, 1, 1, 1, 0, 0], bool))
    col = row.transpose(1, 0, 2).copy()
    assert np.array_equal(refine(col, 0.1)[:, 0], np.array([0, 0, 1, 1, 1, 0, 0], bool))
    edge = np.zeros((1, 5, 3), np.float32)
    edge[0, 0, 1] = 1.0                                   # a neighbour outside the frame never counts
    assert np.array_equal(refine(edge, 0.1)[0], np.array([1, 1, 0, 0, 0], bool))
    assert not refine(np.ones((1, 1, 3), np.float32), 0.0).any(), "a 1 x 1 frame has no neighbours"


def test_refine_float32_and_nan():
    c = np.zeros((1, 2, 3), np.float32)
    c[0, 1, 0] = np.float32(0.1)
    assert refine(c, np.float32(0.1)).sum() == 0
    assert refine(c, np.nextafter(np.float32(0.1), np.float32(0))).sum() == 2
    n = np.zeros((1, 3, 3), np.float32)
    n[0, 1, 0] = np.nan
    assert not refine(n, 0.0).any(), "a NaN never causes refinement"
    n[0, 1, 1] = 1.0
    assert refine(n, 0.0).all()
