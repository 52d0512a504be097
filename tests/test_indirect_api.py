"""The one-bounce diffuse gather, the parts that need no GPU: the two entry points are declared, bound and exported and refuse a NULL context;
the layout arithmetic the kernel adds is checked against a brute-force model; and the pins of the restatement itself (tests/indirect_ref.py
on the CPU checker): a point whose gather rays all miss gives +0.0f bits, and a two-triangle case worked by hand."""
import ctypes as C
import os
import re

import numpy as np

import ao_ref
import indirect_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rt_indirect_diffuse_device", "rt_indirect_diffuse"]
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


def test_header_declares_the_calls_and_the_definition():
    text = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    assert "indirect diffuse" in text and "tests/indirect_ref.py" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\brt_status\s+" + name + r"\s*\(", code), name


def test_binding_and_library_hold_the_calls(rt):
    lib = rt.load_library()
    for name in NAMES:
        assert name in rt.capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert callable(rt.Context.indirect_diffuse) and callable(rt.Flyscene.indirect_diffuse)
    hpp = open(os.path.join(ROOT, "raytracer-in-cpp_amd", "csrc", "flyscene.hpp")).read()
    assert re.search(r"\bbool\s+indirectDiffuse\s*\(", hpp)
    assert "group_indirect" in open(os.path.join(ROOT, "tools", "flyscene_check.cpp")).read()


def test_null_context_is_invalid(rt):
    lib = rt.load_library()
    buf = (C.c_float * 6)()
    p = C.cast(buf, C.c_void_p)
    L = rt.make_lights()
    inv = rt.capi.RT_ERR_INVALID
    assert lib.rt_indirect_diffuse_device(None, C.byref(L), 1, p, p, 3, 0, p, None) == inv
    assert lib.rt_indirect_diffuse(None, C.byref(L), 1, p, p, 3, 0, p) == inv
    # ... also with n = 0, which a context would accept
    assert lib.rt_indirect_diffuse_device(None, C.byref(L), 0, None, None, 3, 0, None, None) == inv
    assert lib.rt_indirect_diffuse(None, C.byref(L), 0, None, None, 3, 0, None) == inv


def test_owner_ranges_cover_every_direction_once_in_ascending_order():
    """gather_range of csrc/rt_gather_layout.hpp, restated: over the rounds, the lanes an owner adds are its point's directions 0 .. K-1, each
    once, ascending -- for every grid size"""
    for m in range(1, ao_ref.MAX_GRID + 1):
        K = m * m
        g = 64
        while K % g:
            g >>= 1
        group, rounds = 64 // g, K // g
        for p in range(64):
            seen = []
            for r in range(rounds):
                lo = p * K - r * 64
                a, b = max(lo, 0), min(lo + K, 64)
                if b <= a:
                    continue
                k0 = a - lo
                for q in range(a, b):
                    e = r * 64 + q
                    assert (e // K, e % K) == (p, k0 + q - a)
                    seen.append(e % K)
            assert seen == (list(range(K)) if p < group else []), (m, p)


# ------------------------------------------------------------------------------------------ the restatement's own pins
def test_two_triangles_by_hand(oracle, tmp_path):
    """In the file's coordinates (the loader's similarity keeps angles and visibility; to_world maps points, so the hand-worked values hold to
    float32 rounding, a few 1e-7).  m = 1: the one direction is N itself.  From P = (0, 0, 0), N = (0, 1, 0) the ray meets the ceiling (y = 1,
    kd (0.5, 0.25, 0.125)) at H = (0, 1, 0); the ceiling's normal, turned against the ray, is (0, -1, 0).  A light at (0, 0.5, 0): ld =
    (0, -1, 0), ct = 1, so out = colour * kd.  A light at (1, 0, 0) is hidden by the blocker and adds nothing.  A light at (-1, 0, 0) is
    visible: pos - H = (-1, -1, 0), ct = 1 / sqrt(2)."""
    osc = oracle.load_scene(ir.two_triangles(str(tmp_path)))
    try:
        data, tracer, W = ir.SceneData(osc), ir.OracleTracer(osc), ir.to_world(osc, ir.TWO_VERTS)
        assert np.allclose(W(ir.TWO_VERTS), osc.arrays()["wverts"], rtol=0, atol=1e-6)
        P, N = W([[0, 0, 0]]), np.array([[0, 1, 0]], F)
        assert np.array_equal(bits(ir.directions(N, np.arange(1), 5, 1)[0, 0]), bits(N[0])), "m = 1: d = N in every bit"
        f, t = osc.closest_hit(P[0], N[0])
        assert f == 0 and abs(t - float(W([0, 1, 0])[1] - P[0, 1])) < 1e-6
        kd = np.array([0.5, 0.25, 0.125], F)
        tol = dict(rtol=0, atol=4e-7)
        out = ir.gather(tracer, data, P, N, 1, 5, W([(0, 0.5, 0)]), (1, 1, 0))
        assert np.allclose(out, [[0.5, 0.25, 0.0]], **tol) and bits(out)[2] == 0, "blue: (0 * kd) * ct = +0"
        tr = ir.trace(tracer, data, P, N, 1, 5, W([(0, 0.5, 0), (1, 0, 0), (-1, 0, 0)]))
        assert tr.hit.tolist() == [[True]] and tr.vis.tolist() == [[True, False, True]]
        assert np.allclose(tr.ct[0], [1.0, 2.0 ** -0.5, 2.0 ** -0.5], **tol), "(the cosine of the hidden light is formed and not used)"
        out = ir.shade(tr, (1, 1, 1))
        assert np.array_equal(bits(out), bits((kd * tr.ct[0, 0]) + (kd * tr.ct[0, 2]))), "R = (0 + kd * ct0) + kd * ct2; K = 1"
        assert np.allclose(out, kd * (1.0 + 2.0 ** -0.5), **tol)
        # the hidden light alone: a hit that sees nothing brings back +0
        out = ir.gather(tracer, data, P, N, 1, 5, W([(1, 0, 0)]), (1, 1, 1))
        assert not bits(out).any()
        # m = 2: four directions with z = 0.866, all of which meet the ceiling; the mean of four radiances, each <= kd
        tr = ir.trace(tracer, data, P, N, 2, 5, W([(0, 0.5, 0)]))
        out = ir.shade(tr, (1, 1, 1))
        assert tr.hit.all() and tr.vis.all() and (out > 0).all() and (out[0] <= kd).all()
        assert np.array_equal(bits(out), bits((((kd * tr.ct[0, 0] + kd * tr.ct[1, 0]) + kd * tr.ct[2, 0]) + kd * tr.ct[3, 0]) / F(4)))
    finally:
        osc.close()


def test_rays_that_all_miss_give_positive_zeros(oracle, tmp_path):
    osc = oracle.load_scene(ir.two_triangles(str(tmp_path)))
    try:
        data, tracer, W = ir.SceneData(osc), ir.OracleTracer(osc), ir.to_world(osc, ir.TWO_VERTS)
        P = W([[0, 2, 0], [0, 0, 0], [0, 0, 0]])                    # above the ceiling looking up; below it looking down; "no point"
        N = np.array([[0, 1, 0], [0, -1, 0], [-0.0, 0, 0]], F)
        for m in (1, 3, 8):
            tr = ir.trace(tracer, data, P, N, m, 7, W([(0, 0.5, 0)]))
            assert not tr.hit.any() and tr.live.tolist() == [True, True, False]
            out = ir.shade(tr, (1, 1, 1))
            assert out.shape == (3, 3) and not bits(out).any(), m
    finally:
        osc.close()


def test_the_order_of_the_sum_shows_on_the_binade_ceiling(oracle, tmp_path):
    """the fixture of the order test of tests/test_gpu_indirect.py, on the CPU: the reversed sum differs in bits"""
    osc = oracle.load_scene(ir.binade_ceiling(str(tmp_path)))
    try:
        data, tracer = ir.SceneData(osc), ir.OracleTracer(osc)
        assert sorted(set(data.kd[:, 0].tolist())) == sorted({0.5} | {2.0 ** (-6 * j) for j in range(ir.STRIPS)})
        W = ir.to_world(osc, ir.BINADE_VERTS)
        P, N = ir.binade_points(W)
        tr = ir.trace(tracer, data, P, N, 8, 7, W([(0.0, 0.2, 0.0)]))
        assert tr.hit.all(), "every gather ray meets the ceiling"
        assert len(set(tr.kd[:, 0].tolist())) >= 6, "the rays meet strips across many binades"
        fwd, rev = ir.shade(tr, (1, 1, 1)), ir.shade(tr, (1, 1, 1), reverse=True)
        assert (bits(fwd) != bits(rev)).any()
    finally:
        osc.close()


# ------------------------------------------------------------------------------------------ what the image filters do for a small grid
def test_quality_of_a_small_grid_raw_and_filtered_is_recorded(oracle, tmp_path):
    """Mixed-materials scene, 64 x 40, yaw 0.4, one white light at (-1, 1, 1): kd * out with 2 x 2 gather rays, raw and after the default
    denoiser (5 iterations, sigmas 1, 0.5, 0.125, 0.25), against 16 x 16 rays, as RMS distance over the pixels where the truth is not zero.
    The figures of this run are recorded in DESIGN.md 6 (Indirect diffuse): raw 0.02604, filtered 0.01841, ratio 0.707.  No ratio is
    required, so none is asserted -- only that the measurement is the one written down (the pixel counts) and that its figures are finite
    and positive."""
    import denoise_ref
    import scenes_gen
    osc = oracle.load_scene(scenes_gen.mixed_materials(str(tmp_path)))
    try:
        r = ir.quality(oracle, osc, 64, 40, 0.4, [(-1.0, 1.0, 1.0)], (1, 1, 1), 2, 16, denoise_ref.Params(5, 1.0, 0.5, 0.125, 0.25), seed=7)
    finally:
        osc.close()
    print("indirect quality:", " ".join(f"{k} {v:.5f}" if isinstance(v, float) else f"{k} {v}" for k, v in r.items()))
    assert (r["covered"], r["pixels"]) == (149, 148)
    assert np.isfinite([r["raw"], r["filtered"], r["ratio"]]).all() and r["raw"] > 0 and r["filtered"] > 0
