"""Adaptive pass counts (rt_set_pass_tolerance, rt_pass_map) at the C ABI, the binding and the front ends, and the numpy restatement of the
rule that the GPU tests build their expectations with (tests/pass_tolerance_ref.py) -- everything that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pass_tolerance_ref as ptr
import passes_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")
F = np.float32


def test_header_declares_the_two_functions():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\brt_status\s+rt_set_pass_tolerance\s*\(\s*rt_ctx\s*\*\s*ctx\s*,\s*float\s+tol\s*,\s*int32_t\s+min_passes\s*\)\s*;", code)
    assert re.search(r"\brt_status\s+rt_pass_map\s*\(\s*rt_ctx\s*\*\s*ctx\s*,\s*uint16_t\s*\*\s*out\s*,\s*size_t\s+n_pixels\s*\)\s*;", code)


def test_binding_has_the_symbols_with_their_argtypes(rt):
    sig = {name: (res, args) for name, res, args in rt.capi._SIGNATURES}
    want = {
        "rt_set_pass_tolerance": (C.c_int, [C.c_void_p, C.c_float, C.c_int32]),
        "rt_pass_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    }
    lib = rt.load_library()
    for name, (res, args) in want.items():
        assert sig[name] == (res, args), name
        assert name in rt.capi.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert hasattr(rt.Context, "set_pass_tolerance") and hasattr(rt.Context, "pass_map")
    fs = rt.Flyscene()
    assert fs.pass_tolerance == -1.0 and fs.pass_min == 8, "the default: off, eight passes before the rule"


def test_null_context_is_rejected(rt):
    lib = rt.load_library()
    for tol, m in ((0.01, 8), (-1.0, 8), (float("nan"), 8), (0.01, 1), (float("inf"), 2)):
        assert lib.rt_set_pass_tolerance(None, tol, m) == rt.capi.RT_ERR_INVALID
    out = np.zeros(4, np.uint16)
    assert lib.rt_pass_map(None, out.ctypes.data_as(C.c_void_p), 4) == rt.capi.RT_ERR_INVALID
    assert (out == 0).all()


# ---------------------------------------------------------------------------------------------------- the restatement of the rule
def by_hand(samples, tol, m):
    """the rule for ONE channel value per pass (all three channels alike), spelt out with scalar float32 operations"""
    s1, s2, taken, active = F(0.0), F(0.0), 0, True
    count = len(samples)
    for k in range(1, count + 1):
        if active:
            f = F(samples[k - 1])
            s1 = F(s1 + f)
            s2 = F(s2 + F(f * f))
            taken = k
        if active and m <= k < count:
            kf = F(k)
            d = F(F(kf * s2) - F(s1 * s1))
            T = F(F(F(F(tol) * F(tol)) * F(kf * kf)) * F(kf - F(1.0)))
            if d <= T:
                active = False
    return F(s1 / F(taken)), taken


@pytest.mark.parametrize("tol,m", [(0.004, 4), (0.02, 4), (0.02, 2), (0.0, 2), (0.3, 3)])
def test_restatement_equals_the_scalar_rule(tol, m):
    rng = np.random.default_rng(11)
    count, npx = 12, 300
    base = rng.random((npx, 1), dtype=F)
    noise = (rng.random((count, npx, 1), dtype=F) - F(0.5)) * rng.choice(np.array([0.0, 0.003, 0.03, 0.5], F), (1, npx, 1))
    frames = [np.repeat((base + noise[k]).astype(F), 3, axis=-1) for k in range(count)]
    got, taken = ptr.fold_adaptive(frames, tol, m)
    assert taken.dtype == np.uint16 and got.dtype == F
    for i in range(npx):
        want, t = by_hand([frames[k][i, 0] for k in range(count)], tol, m)
        assert int(taken[i]) == t, i
        assert got[i, 0].view(np.uint32) == want.view(np.uint32), i
    assert m <= int(taken.min()) and int(taken.max()) <= count


def test_restatement_properties():
    rng = np.random.default_rng(5)
    frames = [rng.random((6, 7, 3), dtype=F) for _ in range(9)]
    # a pixel that stays active to the end is the rt_set_passes pixel: tol = 0 stops nothing on noisy samples
    got, taken = ptr.fold_adaptive(frames, 0.0, 2)
    assert (taken == 9).all() and np.array_equal(got.view(np.uint32), passes_ref.fold_passes(frames).view(np.uint32))
    # +inf: the (first, min_passes) frame
    got, taken = ptr.fold_adaptive(frames, float("inf"), 4)
    assert (taken == 4).all() and np.array_equal(got.view(np.uint32), passes_ref.fold_passes(frames[:4]).view(np.uint32))
    # all three channels must pass: one noisy channel keeps the pixel
    flat = [np.full((1, 3), 0.5, F) for _ in range(9)]
    for k in range(9):
        flat[k][0, 2] = F(0.1 + 0.09 * k)
    _, taken = ptr.fold_adaptive(flat, 0.01, 2)
    assert int(taken[0]) == 9
    # a NaN never converges, a constant pixel stops at min_passes
    nan = [np.full((2, 3), 0.25, F) for _ in range(6)]
    nan[1][0, 1] = np.nan
    _, taken = ptr.fold_adaptive(nan, 1e9, 3)
    assert [int(t) for t in taken] == [6, 3]
    assert ptr.classes(np.array([3, 4, 6, 6, 3]), 3, 6) == (2, 1, 2)


@pytest.mark.parametrize("name,tol,want", [("cube.obj", 0.004, (2478, 16, 66)), ("dodgeColorTest.obj", 0.02, (2449, 34, 77))])
def test_oracle_frames_show_the_three_classes(rt, oracle, name, tol, want):
    """the CPU oracle's one-ray frames with the viewport shifted by rt_pass_offsets are the GPU's single passes bit for bit (tests/test_gpu_passes.py
    pins that); folded by the rule they stop at min_passes, in between and never, in the counts the feature was specified with"""
    w, h, depth, yaw, count, m = 64, 40, 4, 0.2, 16, 4
    lib = rt.load_library()
    osc = oracle.load_scene(os.path.join(SCENES, name))
    oL = oracle.lights(area=True, usteps=5, vsteps=5, points=((-1.0, 1.0, 1.0),))
    frames = []
    try:
        for p in range(count):
            ox, oy = passes_ref.library_offsets(lib, 1, p)
            cam = oracle.camera(w, h, yaw)
            cam.viewport[0], cam.viewport[1] = float(-ox[0]), float(-oy[0])
            frames.append(osc.render(cam, oL, w, h, max_depth=depth, threads=4, want_hits=True)[0])
    finally:
        osc.close()
    _, taken = ptr.fold_adaptive(frames, tol, m)
    assert ptr.classes(taken, m, count) == want


# ---------------------------------------------------------------------------------------------------- the command line
def test_cli_usage_names_the_flag_and_rejects_bad_values():
    assert os.path.exists(RT_RENDER), "rt_render is part of `make all`"
    bad = subprocess.run([RT_RENDER, "--bogus"], capture_output=True, timeout=60)
    assert bad.returncode == 2 and b"--pass-tolerance T [MIN]" in bad.stderr and b"--passes P" in bad.stderr
    for args in (["nan"], ["abc"], ["0.01x"], [""], ["0.01", "1"], ["0.01", "0"], ["0.01", "257"], ["0.01", "4.5"], ["0.01", "x"]):
        r = subprocess.run([RT_RENDER, "--pass-tolerance"] + args, capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--pass-tolerance" in r.stderr, args
    r = subprocess.run([RT_RENDER, "--passes", "16", "--pass-tolerance"], capture_output=True, timeout=60)
    assert r.returncode == 2 and b"--pass-tolerance" in r.stderr, "a missing value"
