"""Ambient occlusion, the parts that need no GPU: the five entry points are declared, bound and exported and refuse a NULL context; the
host half of the definition (rt_ao_directions, rt_ao_rotation) equals tests/ao_ref.py and the header's pins; the frame is orthonormal; and
the reference's own counts on the fixed point sets are the recorded ones."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ao_ref
import scenes_gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rt_ambient_occlusion_device", "rt_ambient_occlusion", "rt_hit_points_device", "rt_ao_directions", "rt_ao_rotation"]
F = np.float32


def bits(a):
    return [f"{int(v):08X}" for v in np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)]


def test_header_declares_the_ao_calls():
    text = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    assert "ambient occlusion" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\brt_status\s+" + name + r"\s*\(", code), name
    assert re.search(r"#define\s+RT_AO_MAX_GRID\s+16\b", code) and re.search(r"#define\s+RT_AO_ROTATIONS\s+64\b", code)


def test_binding_and_library_hold_the_ao_calls(rt):
    lib = rt.load_library()
    for name in NAMES:
        assert name in rt.capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name


def test_null_context_is_invalid(rt):
    lib = rt.load_library()
    buf = (C.c_float * 6)()
    p = C.cast(buf, C.c_void_p)
    inv = rt.capi.RT_ERR_INVALID
    assert lib.rt_ambient_occlusion_device(None, 1, p, p, 3, 0.5, 0, p, p, None) == inv
    assert lib.rt_ambient_occlusion(None, 1, p, p, 3, 0.5, 0, p, p) == inv
    assert lib.rt_hit_points_device(None, 1, p, p, p, p, p, p, None) == inv
    # ... also with n = 0, which a context would accept
    assert lib.rt_ambient_occlusion_device(None, 0, None, None, 3, 0.5, 0, None, None, None) == inv
    assert lib.rt_ambient_occlusion(None, 0, None, None, 3, 0.5, 0, None, None) == inv
    assert lib.rt_hit_points_device(None, 0, None, None, None, None, None, None, None) == inv


def lib_directions(lib, m):
    out = np.full((m * m, 3), np.nan, F)
    assert lib.rt_ao_directions(m, out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    return out


def test_directions_equal_the_reference_and_the_pins(rt):
    lib = rt.load_library()
    tables = {}
    for m in range(1, 17):
        got, want = lib_directions(lib, m), ao_ref.directions(m)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), m
        tables[m] = got
    pins = {(1, 0): "00000000 00000000 3F800000", (2, 0): "BEB504F3 BEB504F3 3F5DB3D7", (2, 3): "3EB504F3 3EB504F3 3F5DB3D7",
            (3, 5): "3F2AAAAB 00000000 3F3ECFA6", (4, 7): "3F397530 BE46C5E5 3F2953FD", (16, 0): "BF29B4A4 BF29B4A4 3EB22B20",
            (16, 255): "3F29B4A4 3F29B4A4 3EB22B20"}
    for (m, k), want in pins.items():
        assert " ".join(bits(tables[m][k])) == want, (m, k)
    for m, d in tables.items():
        # three float32 roundings of a unit vector's components move its length by less than 2^-24 each way: 2 ulp of 1.0f
        norm = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
        assert np.abs(norm - 1.0).max() <= 2.0 * float(np.spacing(F(1.0))), m
        assert d[:, 2].min() > 0.34, m
        # cosine weighting: the mean of z over the hemisphere is 2/3; the m x m midpoint rule is within 1/m of it
        assert abs(float(d[:, 2].astype(np.float64).mean()) - 2.0 / 3.0) <= 1.0 / m, m
    assert abs(float(tables[16][:, 2].min()) - 0.3479) < 1e-4


def test_directions_refuse_bad_arguments(rt):
    lib = rt.load_library()
    out = np.zeros((17 * 17, 3), F)
    po = out.ctypes.data_as(C.POINTER(C.c_float))
    inv = rt.capi.RT_ERR_INVALID
    assert lib.rt_ao_directions(0, po) == inv and lib.rt_ao_directions(17, po) == inv and lib.rt_ao_directions(-1, po) == inv
    assert lib.rt_ao_directions(3, None) == inv
    assert not out.any()
    r, c, s = C.c_int32(), C.c_float(), C.c_float()
    assert lib.rt_ao_rotation(0, 0, None, C.byref(c), C.byref(s)) == inv
    assert lib.rt_ao_rotation(0, 0, C.byref(r), None, C.byref(s)) == inv
    assert lib.rt_ao_rotation(0, 0, C.byref(r), C.byref(c), None) == inv


def lib_rotation(lib, seed, i):
    r, c, s = C.c_int32(-1), C.c_float(), C.c_float()
    assert lib.rt_ao_rotation(seed, i, C.byref(r), C.byref(c), C.byref(s)) == 0
    return int(r.value), F(c.value), F(s.value)


def test_rotation_equals_the_reference_and_the_pins(rt):
    lib = rt.load_library()
    for (seed, i), (h, r) in {(0, 0): (0x00000000, 0), (0, 1): (0x205F0435, 8), (7, 5): (0x93F76A67, 36), (7, 8191): (0xEE08AF40, 59),
                              (0xFFFFFFFF, 0xFFFFFFFF): (0x1DEC3226, 7)}.items():
        assert ao_ref.hash32(seed, i) == h and h >> 26 == r, (seed, i)
        assert lib_rotation(lib, seed, i)[0] == r, (seed, i)
    by_r = {}
    rng = np.random.default_rng(20261)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, 1 << 32, size=(1000, 2), dtype=np.uint64)]
    pairs += [(7, i) for i in range(200)]
    for seed, i in pairs:
        r, c, s = lib_rotation(lib, seed, i)
        wr, wc, ws = ao_ref.rotation(seed, i)
        assert r == wr and bits(c) == bits(wc) and bits(s) == bits(ws), (seed, i)
        assert 0 <= r < 64
        by_r[r] = (c, s)
    assert len(by_r) == 64, "the pairs must reach every rotation step"
    idx = np.array([i for _, i in pairs[:1000]], np.uint64)
    for seed in (0, 7, 0xFFFFFFFF):
        assert ao_ref.rotation_steps(seed, idx).tolist() == [ao_ref.rotation(seed, int(i))[0] for i in idx]
    for r, (c, s) in {0: ("3F800000", "00000000"), 1: ("3F7FEC43", "3CC90AB0"), 17: ("3F6A09A7", "3ECF7BCA"), 63: ("3CC90AB0", "3F7FEC43")}.items():
        assert bits(by_r[r][0]) == [c] and bits(by_r[r][1]) == [s], r


def test_frame_pins_and_orthonormality():
    pins = {(0.0, 0.0, 1.0): ("3F800000 80000000 80000000", "80000000 3F800000 80000000"),
            (0.0, 0.0, -1.0): ("3F800000 80000000 00000000", "00000000 BF800000 80000000"),
            (0.36, 0.48, -0.8): ("3F6D9168 BDC49BA7 3EB851EC", "3DC49BA7 BF5F3B64 BEF5C28F")}
    for n, (wt, wb) in pins.items():
        T, B = ao_ref.frame(np.array(n, F))
        assert " ".join(bits(T)) == wt and " ".join(bits(B)) == wb, n
    rng = np.random.default_rng(7)
    v = rng.normal(size=(1000, 3))
    v[:20, 2] = -np.abs(v[:20, 2]) - 3.0                 # some close to -z, where the naive basis breaks down
    N = (v / np.sqrt((v * v).sum(axis=1, keepdims=True))).astype(F)
    T, B = ao_ref.frame(N)
    T64, B64, N64 = T.astype(np.float64), B.astype(np.float64), N.astype(np.float64)
    for a, b, want in ((T64, T64, 1.0), (B64, B64, 1.0), (N64, N64, 1.0), (T64, B64, 0.0), (T64, N64, 0.0), (B64, N64, 0.0)):
        assert np.abs((a * b).sum(axis=1) - want).max() < 1e-6
    # right-handed: T x B = N
    assert np.abs(np.cross(T64, B64) - N64).max() < 1e-6


def test_segments_of_a_plain_point():
    """one point by hand: N = +z, r = 0 (seed 0, i 0): the directions themselves, scaled by the radius"""
    P = np.array([[0.25, -0.5, 0.125]], F)
    Q = ao_ref.segments(P, np.array([[0, 0, 1]], F), [0], 0, 3, 0.5)
    D = ao_ref.directions(3)
    assert Q.shape == (1, 9, 3)
    assert np.array_equal(Q[0], (P + F(0.5) * D).astype(F))
    assert not ao_ref.is_point(np.array([[0.0, -0.0, 0.0]], F))[0] and ao_ref.is_point(np.array([[0.0, 1e-30, 0.0]], F))[0]


# ---- the reference's own counts on the fixed point sets: the closest hits of the 48 x 32 default camera at yaw 0.4, seed 7
RECORDED = {
    "mixed": {"points": 93, "sums": {(2, 0.25): 321, (3, 0.5): 602, (8, 0.5): 4255, (16, 0.5): 16983}, "partly": {3: 88, 8: 93}},
    "toy": {"points": 360, "sums": {(1, 0.5): 340, (3, 0.5): 2942, (6, 0.25): 11738, (8, 0.5): 20416}, "partly": {3: 107, 8: 222}},
    "dodge": {"points": 242, "sums": {(3, 0.5): 2139, (16, 0.5): 60801}, "partly": {3: 7, 16: 14}},
    "cube": {"points": 561, "sums": {(1, 0.5): 561, (3, 0.5): 9 * 561, (8, 0.25): 64 * 561}, "partly": {3: 0, 8: 0}},
}


@pytest.mark.parametrize("name", ["mixed", "toy", "dodge", "cube"])
def test_reference_counts_on_the_fixed_point_sets(oracle, scenes, tmp_path, name):
    path = {"mixed": lambda: scenes_gen.mixed_materials(str(tmp_path)), "toy": lambda: os.path.join(scenes, "toy.obj"),
            "dodge": lambda: os.path.join(scenes, "dodgeColorTest.obj"), "cube": lambda: os.path.join(scenes, "cube.obj")}[name]()
    osc = oracle.load_scene(path)
    try:
        _, (P, N) = ao_ref.camera_points(oracle, osc)
        rec = RECORDED[name]
        assert len(P) == rec["points"]
        for (m, radius), want in rec["sums"].items():
            c = ao_ref.counts(osc, P, N, 7, m, radius)
            assert c.dtype == np.uint16 and c.max() <= m * m
            assert int(c.sum()) == want, (m, radius)
            if m in rec["partly"]:
                assert int(((c > 0) & (c < m * m)).sum()) == rec["partly"][m], m
        if name in ("mixed", "toy"):
            assert rec["partly"][3] >= 80, "an all-open scene tests nothing"
    finally:
        osc.close()
