"""The light jitter offsets (rt_light_jitter_offsets) at the C ABI and the binding, and the Python restatement of the jittered samples and of a
depth-0 pass frame (tests/light_jitter_ref.py), tied to the CPU oracle -- everything needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import light_jitter_ref as ljr
import passes_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
SCENES = os.path.join(HERE, "golden", "scenes")
F = np.float32

# p -> (fu bits, fv bits), as the issue and the header give them
OFFSET_PINS = {
    1: (0x3F333333, 0x3F249249),
    2: (0x3F666666, 0x3F492492),
    5: (0x3F0A3D71, 0x3E5B6DB7),
    7: (0x3F70A3D7, 0x3F053978),
    255: (0x3F0B0F28, 0x3F76ABA9),
}
TWO_LIGHTS = ((-1.0, 1.0, 1.0), (1.0, 1.5, 1.0))
# scene, (w, h), yaw, light positions (None: the default light), (usteps, vsteps)
SHAPES = {
    "cube": ("cube.obj", (24, 16), 0.0, None, (4, 4)),
    "cube-two-lights": ("cube.obj", (24, 16), 0.3, TWO_LIGHTS, (3, 3)),
    "toy": ("toy.obj", (24, 16), 0.0, None, (4, 4)),
    "dodge": ("dodgeColorTest.obj", (24, 16), 0.0, None, (4, 4)),
}


def bits(x):
    return int(np.asarray(x, F).reshape(1).view(np.uint32)[0])


def test_header_declares_the_function():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\brt_status\s+rt_light_jitter_offsets\s*\(\s*int32_t\s+p\s*,\s*float\s*\*\s*fu\s*,\s*float\s*\*\s*fv\s*\)\s*;", code)
    for p, (bu, bv) in OFFSET_PINS.items():
        assert f"p = {p}: {bu:08X} {bv:08X}" in text, p


def test_binding_has_the_symbol_with_its_argtypes(rt):
    sig = {name: (res, args) for name, res, args in rt.capi._SIGNATURES}
    fp = C.POINTER(C.c_float)
    lib = rt.load_library()
    assert sig["rt_light_jitter_offsets"] == (C.c_int, [C.c_int32, fp, fp])
    assert "rt_light_jitter_offsets" in rt.capi.EXPORTED_SYMBOLS
    assert lib.rt_light_jitter_offsets.argtypes == [C.c_int32, fp, fp] and lib.rt_light_jitter_offsets.restype is C.c_int


def test_offset_known_answers(rt):
    lib = rt.load_library()
    for p, want in OFFSET_PINS.items():
        got = tuple(bits(x) for x in ljr.library_offsets(lib, p))
        assert got == want, (p, [hex(b) for b in got])
        assert tuple(bits(x) for x in ljr.jitter_offsets(p)) == want, p
    assert tuple(bits(x) for x in ljr.library_offsets(lib, 0)) == (0x3F000000, 0x3F000000), "pass 0 is the cell centre"


def test_offsets_equal_the_restatement_for_every_pass(rt):
    lib = rt.load_library()
    pairs = set()
    for p in range(ljr.RT_MAX_PASSES):
        fu, fv = ljr.library_offsets(lib, p)
        wu, wv = ljr.jitter_offsets(p)
        assert (bits(fu), bits(fv)) == (bits(wu), bits(wv)), p
        assert F(0.0) <= fu < F(1.0) and F(0.0) <= fv < F(1.0), (p, fu, fv)
        pairs.add((bits(fu), bits(fv)))
    assert len(pairs) == ljr.RT_MAX_PASSES, "the 256 float pairs are pairwise distinct"
    assert passes_ref.wrapped(0, 5) == 0.0 and passes_ref.wrapped(0, 7) == 0.0


def test_offsets_reject_bad_arguments(rt):
    lib, inv = rt.load_library(), rt.capi.RT_ERR_INVALID
    fu, fv = C.c_float(7.0), C.c_float(9.0)
    for p in (-1, 256, 1000, -256):
        assert lib.rt_light_jitter_offsets(p, C.byref(fu), C.byref(fv)) == inv, p
    assert lib.rt_light_jitter_offsets(3, None, C.byref(fv)) == inv
    assert lib.rt_light_jitter_offsets(3, C.byref(fu), None) == inv
    assert fu.value == 7.0 and fv.value == 9.0
    assert lib.rt_light_jitter_offsets(255, C.byref(fu), C.byref(fv)) == 0


def test_samples_are_the_cell_centres_at_a_half_and_one_addition_from_the_index(oracle):
    L = oracle.lights(area=True, usteps=3, vsteps=5, points=TWO_LIGHTS)
    for l in range(2):
        lp = [L.pos[l][k] for k in range(3)]
        want = oracle.light_samples(L, lp)
        got = ljr.light_samples(3, 5, L.len_x, L.len_y, lp, ljr.CENTRE)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "the oracle's own createSpherePoint"
    fo = ljr.jitter_offsets(5)
    s = ljr.light_samples(3, 5, L.len_x, L.len_y, TWO_LIGHTS[0], fo)
    cx = F(F(F(-1.0) + F(L.len_x)) / F(3))
    cy = F(F(F(1.0) + F(L.len_y)) / F(5))
    for i in range(3):
        for j in range(5):
            assert s[i * 5 + j, 0] == F(F(F(i) + fo[0]) * cx) and s[i * 5 + j, 1] == F(F(F(j) + fo[1]) * cy) and s[i * 5 + j, 2] == F(1.0)
    # a shift moves every sample, and by less than one cell
    c = ljr.light_samples(3, 5, L.len_x, L.len_y, TWO_LIGHTS[0], ljr.CENTRE)
    assert (s[:, 0] != c[:, 0]).all() and (s[:, 1] != c[:, 1]).all()
    assert (np.abs(s[:, 0] - c[:, 0]) < abs(cx)).all() and (np.abs(s[:, 1] - c[:, 1]) < abs(cy)).all()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_restatement_at_the_cell_centres_is_the_oracles_depth_0_frame(oracle, shape):
    name, (w, h), yaw, points, (u, v) = SHAPES[shape]
    osc = oracle.load_scene(os.path.join(SCENES, name))
    try:
        cam, L = oracle.camera(w, h, yaw), oracle.lights(area=True, usteps=u, vsteps=v, points=points)
        want, _, _ = osc.render(cam, L, w, h, max_depth=0, threads=4)
        got, _ = ljr.pass_frame(oracle, osc, cam, L, w, h)
    finally:
        osc.close()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())
    assert (want != ljr.BACKGROUND).any(), "the frame must show the object"
