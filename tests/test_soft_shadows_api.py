"""Soft shadows, the parts that need no GPU: the five entry points are declared, bound and exported and refuse a NULL context; the host half
of the definition (rt_shadow_jitter, rt_light_samples, rt_default_shadow_params) equals tests/shadow_ref.py, tests/light_jitter_ref.py and
the header's pins; and the measurement that motivates the per-point jitter, reproduced on the CPU with the defined hash."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref
import light_jitter_ref
import scenes_gen
import shadow_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rt_default_shadow_params", "rt_shadow_jitter", "rt_light_samples", "rt_soft_shadows_device", "rt_soft_shadows"]
F = np.float32
# (seed, i) -> g, fu, fv with the floats as bits: the pins of the header
PINS = {(0, 0): (0x31315BDB, 0x3E44C400, 0x3EB7B600), (0, 1): (0x977B0A53, 0x3F177B00, 0x3D253000), (7, 5): (0xB6706ADC, 0x3F367000, 0x3ED5B800),
        (0xFFFFFFFF, 0xFFFFFFFF): (0x888E5787, 0x3F088E00, 0x3EAF0E00), (3, 2073599): (0x43D51905, 0x3E87AA00, 0x3DC82800)}


def bits(v):
    return int(np.asarray(v, F).reshape(1).view(np.uint32)[0])


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint32), b.reshape(-1).view(np.uint32))


def test_header_declares_the_soft_shadow_calls():
    text = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    assert "soft shadows" in text
    assert "NO FRAME USES IT YET" not in text and "AND NO FRAME USES IT" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES[1:]:
        assert re.search(r"\brt_status\s+" + name + r"\s*\(", code), name
    assert re.search(r"\bvoid\s+rt_default_shadow_params\s*\(", code)
    assert re.search(r"typedef\s+struct\s+rt_shadow_params\s*\{\s*int32_t\s+per_point;\s*uint32_t\s+seed;\s*float\s+fu,\s*fv;\s*\}\s*rt_shadow_params;", code)


def test_binding_and_library_hold_the_soft_shadow_calls(rt):
    lib = rt.load_library()
    for name in NAMES:
        assert name in rt.capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert C.sizeof(rt.capi.rt_shadow_params) == 16
    for name in ("shadow_params", "shadow_jitter", "light_samples"):
        assert callable(getattr(rt, name)) and callable(getattr(rt.flyscene, name)), name
    assert callable(rt.Context.soft_shadows) and callable(rt.Flyscene.soft_shadows)


def test_null_context_is_invalid(rt):
    lib = rt.load_library()
    buf = (C.c_float * 6)()
    p = C.cast(buf, C.c_void_p)
    L, sp = rt.make_lights(), rt.shadow_params()
    inv = rt.capi.RT_ERR_INVALID
    assert lib.rt_soft_shadows_device(None, C.byref(L), 1, p, p, C.byref(sp), p, p, None) == inv
    assert lib.rt_soft_shadows(None, C.byref(L), 1, p, p, C.byref(sp), p, p) == inv
    # ... also with n = 0, which a context would accept
    assert lib.rt_soft_shadows_device(None, C.byref(L), 0, None, None, C.byref(sp), None, None, None) == inv
    assert lib.rt_soft_shadows(None, C.byref(L), 0, None, None, C.byref(sp), None, None) == inv


# ------------------------------------------------------------------------------------------ 1. rt_shadow_jitter
def lib_jitter(lib, seed, i):
    fu, fv = C.c_float(float("nan")), C.c_float(float("nan"))
    assert lib.rt_shadow_jitter(seed, i, C.byref(fu), C.byref(fv)) == 0
    return F(fu.value), F(fv.value)


def test_jitter_equals_the_reference_and_the_pins(rt):
    lib = rt.load_library()
    for (seed, i), (g, fu, fv) in PINS.items():
        assert shadow_ref.hash32(seed, i) == g, (seed, i)
        for got in (lib_jitter(lib, seed, i), shadow_ref.jitter(seed, i), rt.shadow_jitter(seed, i)):
            assert (bits(got[0]), bits(got[1])) == (fu, fv), (seed, i)
    rng = np.random.default_rng(20262)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, 1 << 32, size=(3596, 2), dtype=np.uint64)]
    pairs += [(7, i) for i in range(500)]
    assert len(pairs) == 4096
    for seed, i in pairs:
        got, want = lib_jitter(lib, seed, i), shadow_ref.jitter(seed, i)
        assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1]), (seed, i)
        assert 0.0 <= got[0] < 1.0 and 0.0 <= got[1] < 1.0
        # exact: a multiple of 2^-16
        assert float(got[0]) * 65536.0 == int(float(got[0]) * 65536.0) and float(got[1]) * 65536.0 == int(float(got[1]) * 65536.0)
    idx = np.array([i for _, i in pairs[:1000]], np.uint64)
    for seed in (0, 7, 0xFFFFFFFF):
        assert same(shadow_ref.jitters(seed, idx), np.array([shadow_ref.jitter(seed, int(i)) for i in idx], F))
    inv = rt.capi.RT_ERR_INVALID
    f = C.c_float()
    assert lib.rt_shadow_jitter(0, 0, None, C.byref(f)) == inv and lib.rt_shadow_jitter(0, 0, C.byref(f), None) == inv


# ------------------------------------------------------------------------------------------ 2. rt_light_samples
POSITIONS = ((-1.0, 1.0, 1.0), (0.6, 1.2, 0.2), (0.0, 0.0, 0.0), (-0.3, -2.5, -0.75), (0.0, -0.0, 2.0))


def lib_samples(lib, L, light, fo, n):
    out = np.full((n, 3), np.nan, F)
    s = lib.rt_light_samples(C.byref(L), light, float(fo[0]), float(fo[1]), out.ctypes.data_as(C.c_void_p))
    return s, out


@pytest.mark.parametrize("grid", [(1, 1), (2, 2), (5, 5), (8, 8), (3, 7), (32, 32)])
def test_light_samples_equal_the_restatement(rt, grid):
    lib = rt.load_library()
    u, v = grid
    L = rt.make_lights(POSITIONS, area=True, usteps=u, vsteps=v)
    offsets = [light_jitter_ref.CENTRE, light_jitter_ref.library_offsets(lib, 5), shadow_ref.jitter(7, 5), (F(0.0), F(0.99998474))]
    assert bits(offsets[1][0]) == 0x3F0A3D71 and bits(offsets[1][1]) == 0x3E5B6DB7
    for fo in offsets:
        for l, c in enumerate(POSITIONS):
            want = light_jitter_ref.light_samples(u, v, L.len_x, L.len_y, c, fo)
            s, got = lib_samples(lib, L, l, fo, u * v)
            assert s == 0 and same(got, want), (grid, l, fo)
            assert same(rt.light_samples(L, l, fo[0], fo[1]), want)
    # the restatement of this file's reference puts the lights back to back
    assert same(shadow_ref.samples(shadow_ref.Lights(L), offsets[2]),
                np.concatenate([light_jitter_ref.light_samples(u, v, L.len_x, L.len_y, c, offsets[2]) for c in POSITIONS]))


def test_centre_samples_are_the_frames_samples(rt, oracle):
    """(0.5f, 0.5f): the samples the CPU checker's renderer takes (orc_light_samples), in every bit"""
    lib = rt.load_library()
    for u, v in ((5, 5), (3, 7), (32, 32)):
        L = rt.make_lights(POSITIONS, area=True, usteps=u, vsteps=v)
        oL = oracle.lights(area=True, usteps=u, vsteps=v, points=POSITIONS)
        for l, c in enumerate(POSITIONS):
            s, got = lib_samples(lib, L, l, (0.5, 0.5), u * v)
            assert s == 0 and same(got, oracle.light_samples(oL, c)), (u, v, l)


def test_light_samples_point_sphere_and_refusals(rt):
    lib = rt.load_library()
    inv, uns = rt.capi.RT_ERR_INVALID, rt.capi.RT_ERR_UNSUPPORTED
    L = rt.make_lights(POSITIONS, area=False)
    for l, c in enumerate(POSITIONS):
        s, got = lib_samples(lib, L, l, (0.25, 0.75), 1)
        assert s == 0 and same(got, np.array([c], F))
        s, again = lib_samples(lib, L, l, (float("nan"), 7.0), 1)              # (jitter is not looked at)
        assert s == 0 and same(again, got)
    L = rt.make_lights(POSITIONS, area=True)
    keep = rt.set_sphere(L, rt.sphere_offsets(3, 1.0, 25))                          # noqa: F841 -- keeps the offsets alive
    assert L.mode == rt.capi.RT_LIGHT_SPHERE
    s, got = lib_samples(lib, L, 0, (0.5, 0.5), 25)
    assert s == uns and np.isnan(got).all()
    with pytest.raises(ValueError):
        rt.light_samples(L, 0, 0.5, 0.5)
    L = rt.make_lights(POSITIONS, area=True, usteps=5, vsteps=5)
    for light in (-1, len(POSITIONS), 25, 1 << 30):
        s, got = lib_samples(lib, L, light, (0.5, 0.5), 25)
        assert s == inv and np.isnan(got).all(), light
    out = np.zeros((25, 3), F)
    assert lib.rt_light_samples(None, 0, 0.5, 0.5, out.ctypes.data_as(C.c_void_p)) == inv
    assert lib.rt_light_samples(C.byref(L), 0, 0.5, 0.5, None) == inv
    for u, v, nl in ((0, 5, 1), (5, 0, 1), (33, 32, 1), (5, 5, 0), (5, 5, 26)):
        bad = rt.make_lights(POSITIONS, area=True, usteps=u, vsteps=v)
        bad.n_lights = nl if nl != 1 else bad.n_lights
        assert lib.rt_light_samples(C.byref(bad), 0, 0.5, 0.5, out.ctypes.data_as(C.c_void_p)) == inv, (u, v, nl)
    assert not out.any()


# ------------------------------------------------------------------------------------------ 3. rt_default_shadow_params
def test_default_shadow_params(rt):
    lib = rt.load_library()
    p = rt.capi.rt_shadow_params(7, 7, 0.1, 0.2)
    lib.rt_default_shadow_params(C.byref(p))
    assert (p.per_point, p.seed, bits(p.fu), bits(p.fv)) == (0, 0, 0x3F000000, 0x3F000000)
    lib.rt_default_shadow_params(None)
    q = rt.shadow_params()
    assert (q.per_point, q.seed, q.fu, q.fv) == (0, 0, 0.5, 0.5)
    q = rt.shadow_params(per_point=True, seed=0x1FFFFFFFF, fu=0.25)
    assert (q.per_point, q.seed, q.fu, q.fv) == (1, 0xFFFFFFFF, 0.25, 0.5)


# ------------------------------------------------------------------------------------------ 4. what the per-point jitter is for
def test_per_point_jitter_and_the_filter_beat_cell_centres(oracle, tmp_path):
    """Mixed-materials scene, 192 x 120, yaw 0.44, one light at (0.6, 1.2, 0.2); truth = the cell centres of a 16 x 16 light.  A 4 x 4 light
    with a grid of the point's own (seed 0, point index = raster index), filtered with the existing denoiser, is closer to the truth than the
    unfiltered cell centres of a 4 x 4 light, over the covered pixels and over the partly lit ones.  The four RMS distances of this run,
    (centres, centres filtered, jitter, jitter filtered), are recorded in DESIGN.md 6: all covered pixels 0.0281, 0.0279, 0.0346, 0.0197;
    partly lit 0.0541, 0.0534, 0.0666, 0.0374."""
    osc = oracle.load_scene(scenes_gen.mixed_materials(str(tmp_path)))
    try:
        r = shadow_ref.direction(oracle, osc, 192, 120, 0.44, (0.6, 1.2, 0.2), 4, 16, denoise_ref.Params(2, 0.5, 0.5, 0.125, 0.25), seed=0)
    finally:
        osc.close()
    for name in ("all", "partly_lit"):
        print(name, " ".join(f"{k} {v:.4f}" for k, v in r[name].items()))
    assert (r["covered"], r["partly"]) == (1433, 387)
    assert r["all"]["jitter_filtered"] < r["all"]["centres"]
    assert r["partly_lit"]["jitter_filtered"] < r["partly_lit"]["centres"]
