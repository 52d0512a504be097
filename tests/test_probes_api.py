"""The light probes, the parts that need no GPU: the eight entry points are declared, bound and exported and refuse a NULL context; the host
tables equal their numpy restatement bit for bit; closed forms the projection must reproduce (uniform radiance, a hemisphere, the direct
term); the lookup by hand; the pins of the restatement itself (tests/probe_ref.py on the CPU checker); the layout program under the
sanitizers; and the quality measurement of DESIGN.md 6."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import indirect_ref as ir
import probe_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer-in-cpp_amd", "csrc")
NAMES = ["rt_probe_directions", "rt_probe_weights", "rt_sh9", "rt_probe_grid_positions", "rt_light_probes_device", "rt_light_probes",
         "rt_probe_irradiance_device", "rt_probe_irradiance"]
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


def fp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_header_declares_the_calls_and_the_definition():
    text = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    assert "light probes" in text and "tests/probe_ref.py" in text and "#define RT_PROBE_COEFFS 27" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\brt_status\s+" + name + r"\s*\(", code), name
    assert re.search(r"typedef\s+struct\s+rt_probe_grid\s*\{\s*float\s+origin\[3\];\s*float\s+step\[3\];\s*int32_t\s+dims\[3\];\s*\}\s*rt_probe_grid;", code)


def test_binding_and_library_hold_the_calls(rt):
    lib = rt.load_library()
    for name in NAMES:
        assert name in rt.capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert rt.capi.RT_PROBE_COEFFS == 27 and C.sizeof(rt.capi.rt_probe_grid) == 36
    for owner, members in ((rt.Context, ("light_probes", "probe_irradiance")), (rt.Flyscene, ("light_probes", "probe_irradiance")),
                           (rt, ("probe_grid", "probe_grid_over", "probe_grid_positions"))):
        for mname in members:
            assert callable(getattr(owner, mname)), mname
    hpp = open(os.path.join(CSRC, "flyscene.hpp")).read()
    assert re.search(r"\bbool\s+lightProbes\s*\(", hpp) and re.search(r"\bbool\s+probeIrradiance\s*\(", hpp)
    assert "group_probes" in open(os.path.join(ROOT, "tools", "flyscene_check.cpp")).read()
    assert "--probes" in open(os.path.join(CSRC, "rt_render_main.cpp")).read()


def test_null_context_and_null_arrays_are_invalid(rt):
    lib = rt.load_library()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    L = rt.make_lights()
    g = rt.probe_grid((0, 0, 0), (1, 1, 1), (1, 1, 1))
    inv = rt.capi.RT_ERR_INVALID
    for n, q in ((1, p), (0, None)):                        # ... also with n = 0, which a context would accept
        assert lib.rt_light_probes_device(None, C.byref(L), n, q, 3, 0, q, None) == inv
        assert lib.rt_light_probes(None, C.byref(L), n, q, 3, 0, q) == inv
        assert lib.rt_probe_irradiance_device(None, C.byref(g), q, n, q, q, q, None) == inv
        assert lib.rt_probe_irradiance(None, C.byref(g), q, n, q, q, q) == inv
    assert lib.rt_probe_directions(3, None) == inv and lib.rt_probe_weights(3, None) == inv
    for m in (0, 17, -1):
        assert lib.rt_probe_directions(m, p) == inv and lib.rt_probe_weights(m, p) == inv
    assert lib.rt_sh9(None, p) == inv and lib.rt_sh9(p, None) == inv
    assert lib.rt_probe_grid_positions(None, p) == inv and lib.rt_probe_grid_positions(C.byref(g), None) == inv
    assert not any(buf)


# ------------------------------------------------------------------------------------------ the tables
def test_tables_equal_the_restatement_for_every_grid_size(rt):
    lib = rt.load_library()
    for m in range(1, 17):
        d, w = np.full((m * m + 1, 3), 7, F), np.full((m * m + 1, 9), 7, F)
        assert lib.rt_probe_directions(m, fp(d)) == 0 and lib.rt_probe_weights(m, fp(w)) == 0
        assert (d[-1] == 7).all() and (w[-1] == 7).all(), "exactly K entries are written"
        assert np.array_equal(bits(d[:-1]), bits(pr.directions(m))), m
        assert np.array_equal(bits(w[:-1]), bits(pr.weights(m))), m
        n = np.sqrt((d[:-1].astype(np.float64) ** 2).sum(axis=1))
        assert np.abs(n - 1).max() < 1e-7, "unit directions"
        if m > 1:
            assert np.abs(d[:-1].astype(np.float64).sum(axis=0)).max() < 2e-5 * m * m, "the set is balanced over the sphere"
    # the entries the header records
    d, w = pr.directions(2), pr.weights(2)
    assert [f"{x:08x}" for x in bits(d[:2])] == ["24748d50", "3f5db3d7", "3f000000", "a53769fc", "bf5db3d7", "3f000000"]
    assert [f"{x:08x}" for x in bits(w[0])] == ["3f62dfc5", "3f62dfc4", "3f02fc5f", "247a41b0", "2435bb80", "3ebe3d5d", "bd7da728", "23d1d8b6", "bea4c09e"]
    assert [f"{x:08x}" for x in bits(pr.directions(16)[37])] == ["bece9088", "3f1a92a7", "3f300000"]
    assert [f"{x:08x}" for x in bits(pr.weights(16)[37])] == ["3c62dfc5", "3c1e2db5", "3c341b02", "bbd3620f", "bb560c1a", "3bb66021", "3ad409bb", "bb73b807",
                                                               "bab15293"]


def test_sh9_equals_the_restatement(rt):
    lib = rt.load_library()
    rng = np.random.default_rng(11)
    V = np.concatenate([rng.standard_normal((200, 3)).astype(F), np.array([[0.6, 0, 0.8], [0, 0, 0], [-0.0, 1, 0], [1e20, -1e20, 1e-30], [np.inf, 1, np.nan]], F)])
    want = pr.sh9(V)
    for v, wv in zip(V, want):
        out = np.full(10, 7, F)
        assert lib.rt_sh9(fp(np.ascontiguousarray(v)), fp(out)) == 0 and out[9] == 7
        assert np.array_equal(bits(out[:9]), bits(wv)), v
    assert [f"{x:08x}" for x in bits(pr.sh9(np.array([0.6, 0, 0.8], F)))] == ["3e906ebb", "00000000", "3ec821b0", "3e961944", "00000000", "00000000", "3e948fe3",
                                                                           "3f06409b", "3e4960e8"]


def test_grid_positions_equal_the_restatement(rt):
    lib = rt.load_library()
    for origin, step, dims in (((0.0, 1.0, 2.0), (1.0, 0.5, 2.0), (2, 3, 1)), ((-1.3, 0.7, 0.1), (0.3, 0.11, 1e-3), (3, 2, 4)), ((5, 5, 5), (1, 1, 1), (1, 1, 1))):
        g = rt.probe_grid(origin, step, dims)
        ref = pr.Grid.of(g)
        out = np.full((ref.cells + 1, 3), 7, F)
        assert lib.rt_probe_grid_positions(C.byref(g), fp(out)) == 0 and (out[-1] == 7).all()
        assert np.array_equal(bits(out[:-1]), bits(ref.positions()))
        assert np.array_equal(bits(rt.probe_grid_positions(g)), bits(ref.positions()))
    want = pr.Grid((0.0, 1.0, 2.0), (1.0, 0.5, 2.0), (2, 3, 1)).positions()
    assert want.tolist() == [[0, 1, 2], [1, 1, 2], [0, 1.5, 2], [1, 1.5, 2], [0, 2, 2], [1, 2, 2]], "ix fastest, then iy"
    inv = rt.capi.RT_ERR_INVALID
    out = np.zeros((8, 3), F)
    for origin, step, dims in (((0, 0, 0), (1, 1, 1), (0, 1, 1)), ((0, 0, 0), (1, 0, 1), (1, 1, 1)), ((0, 0, 0), (1, 1, -1), (1, 1, 1)),
                               ((0, 0, 0), (1, float("inf"), 1), (1, 1, 1)), ((0, 0, 0), (float("nan"), 1, 1), (1, 1, 1)), ((0, 0, 0), (1, 1, 1), (4096, 4096, 2))):
        assert lib.rt_probe_grid_positions(C.byref(rt.probe_grid(origin, step, dims)), fp(out)) == inv, (step, dims)
    assert not out.any()
    # probe_grid_over: the outermost probes on the grown box, a single probe in the middle of its axis
    g = pr.Grid.of(rt.probe_grid_over((-1.0, -0.5, 0.0, 1.0, 0.5, 0.25), (3, 1, 2), margin=0.25))
    ref = pr.Grid.over((-1.0, -0.5, 0.0, 1.0, 0.5, 0.25), (3, 1, 2), margin=0.25)
    assert np.array_equal(bits(g.origin), bits(ref.origin)) and np.array_equal(bits(g.step), bits(ref.step)) and g.dims == ref.dims == (3, 1, 2)
    assert g.origin.tolist() == [-1.25, 0.0, -0.25] and g.step.tolist() == [1.25, 1.0, 0.75]


# ------------------------------------------------------------------------------------------ closed forms of the projection
def test_uniform_radiance_evaluates_to_one_minus_the_midpoint_bias():
    """R = 1 in every direction: only Y0 and Y6 survive the sums over phi.  The band-0 term is exact, (4 pi / K) K Y0 Y0 = 1.  In z the
    directions are the midpoint rule with m cells of width 2 / m, which integrates z^2 over [-1, 1] to 2/3 - 2 / (3 m^2): the band-2 term is
    (4 pi / K) (1/4) Y6(0, 0, 1) sum_k Y6(d_k) = (5 / 8) (3 * (1/3 - 1 / (3 m^2)) - 1) = -0.625 / m^2."""
    got = {}
    for m in (1, 3, 4, 8, 16):
        C_ = pr.project(np.ones((1, m * m, 3), F), pr.weights(m))
        got[m] = float(pr.evaluate(C_, (0, 0, 1))[0, 0])
        print("uniform radiance at +z, m =", m, got[m])
        assert abs(got[m] - (1 - 0.625 / (m * m))) < 1e-5, m
    for m, v in ((1, 0.375), (3, 0.930556), (4, 0.960938), (8, 0.990234), (16, 0.997561)):
        assert abs(got[m] - v) < 1e-5


def test_a_hemisphere_of_radiance_evaluates_to_one_minus_half_that_bias():
    """R = 1 where d_z > 0 at even m (no cell centre on the equator): band 0 gives 1/2, band 1 (2/3)(3 / (4 pi))(4 pi / K) sum z over the
    upper half = 2 * (1/4) exactly (the midpoint rule is exact for z), band 2 half of the uniform case: 1 - 0.3125 / m^2"""
    for m, v in ((4, 0.980469), (8, 0.995117), (16, 0.998780)):
        R = np.zeros((1, m * m, 3), F)
        R[0, pr.directions(m)[:, 2] > 0] = 1
        got = float(pr.evaluate(pr.project(R, pr.weights(m)), (0, 0, 1))[0, 1])
        print("hemisphere at +z, m =", m, got)
        assert abs(got - (1 - 0.3125 / (m * m))) < 1e-5 and abs(got - v) < 1e-5


def test_the_direct_term_alone():
    """sum_j b_j Y_j(w) Y_j(n) = 1/4 + (1/2) n.w + (5/32)(3 (n.w)^2 - 1), by the addition theorem with b = (pi, 2 pi / 3, pi / 4): 1.0625 at n = w,
    0.0625 at n = -w, 0.09375 across"""
    C_ = np.zeros((1, 9, 3), F)
    pr.add_direct(C_, np.zeros((1, 3), F), [(0.6, 0.0, 0.8)], (1, 1, 1), np.ones((1, 1), bool))
    assert np.abs(pr.evaluate(C_, (0.6, 0, 0.8)) - 1.0625).max() < 1e-5
    assert np.abs(pr.evaluate(C_, (-0.6, 0, -0.8)) - 0.0625).max() < 1e-5
    assert np.abs(pr.evaluate(C_, (0.8, 0, -0.6)) - (0.25 - 5 / 32)).max() < 1e-5
    hidden = np.zeros((1, 9, 3), F)
    pr.add_direct(hidden, np.zeros((1, 3), F), [(0.6, 0.0, 0.8)], (1, 1, 1), np.zeros((1, 1), bool))
    assert not bits(hidden).any()


# ------------------------------------------------------------------------------------------ the lookup by hand
def test_lookup_on_a_small_grid_by_hand():
    grid = pr.Grid((0.0, 1.0, 2.0), (1.0, 0.5, 2.0), (2, 3, 1))
    rng = np.random.default_rng(3)
    Cf = rng.standard_normal((grid.cells, 27)).astype(F)
    pos = grid.positions()
    N = np.array([0.6, 0.0, 0.8], F)
    on = pr.lookup(grid, Cf, pos, np.tile(N, (6, 1)))
    assert np.array_equal(bits(on), bits(pr.evaluate(Cf, N))), "a point on a probe returns that probe's coefficients"
    # outside points clamp to the nearest probe; the single layer in z reads the same whatever z is
    out = pos + np.array([[-3, -5, 9], [4, -5, -9], [-3, 0, 1], [4, 0, 2], [-3, 7, 3], [4, 7, np.inf]], F)
    assert np.array_equal(bits(pr.lookup(grid, Cf, out, np.tile(N, (6, 1)))), bits(on))
    # NaN coordinates go to cell 0, whose near corner has all the weight
    nanp = np.full((1, 3), np.nan, F)
    assert np.array_equal(bits(pr.lookup(grid, Cf, nanp, N[None])), bits(on[:1]))
    # the middle of an edge and of a cell: weights 1/2 and 1/4, exact in float32
    mid = pr.lookup(grid, Cf, [[0.5, 1.0, 2.0], [0.5, 1.25, 5.0]], np.tile(N, (2, 1)))
    B_edge = (F(0.5) * Cf[0] + F(0.5) * Cf[1]).astype(F)
    B_cell = (((F(0.25) * Cf[0] + F(0.25) * Cf[1]) + F(0.25) * Cf[2]) + F(0.25) * Cf[3]).astype(F)
    # (on the edge the far row of y has weight 0: its two corners add +-0 and change nothing)
    assert np.array_equal(bits(mid[0]), bits(pr.evaluate(B_edge, N)[0])) and np.array_equal(bits(mid[1]), bits(pr.evaluate(B_cell, N)[0]))
    # no point: +0.0f whatever the rest is
    z = pr.lookup(grid, np.full_like(Cf, np.nan), [[0.5, 1.25, 2.0]] * 2, [[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0]])
    assert not bits(z).any()
    # a grid of one probe: that probe everywhere
    one = pr.Grid((5, 5, 5), (1, 1, 1), (1, 1, 1))
    assert np.array_equal(bits(pr.lookup(one, Cf[:1], [[-9, 0, 99]], N[None])), bits(pr.evaluate(Cf[:1], N)))


# ------------------------------------------------------------------------------------------ the restatement's own pins
def test_a_probe_under_the_ceiling_by_hand(oracle, tmp_path):
    """Two triangles, in the file's coordinates (the loader's similarity keeps angles and visibility).  m = 2: the directions are (0, +-0.866,
    +-0.5) up to 1e-16 in x.  From P = (0, 0, 0) rays 0 and 2 (d_y > 0) meet the ceiling (y = 1, kd (0.5, 0.25, 0.125)) at (0, 1, +-0.577), rays
    1 and 3 meet nothing.  A light at (0, 0.5, 0) is visible from both hits; the ceiling's normal turned against the ray is (0, -1, 0), so
    ct = 0.5 / sqrt(0.25 + 1/3) = 0.654654.  C[j][c] = R_c * W[0][j] + R_c * W[2][j]; band 0: kd_c * ct * 2 * (pi * 0.282095) = kd_c *
    1.160347.  A probe at (0.02, 0.98, 0) sees that light but not the one at (1, 0, 0), which the blocker hides."""
    osc = oracle.load_scene(ir.two_triangles(str(tmp_path)))
    try:
        data, tracer, W = ir.SceneData(osc), ir.OracleTracer(osc), ir.to_world(osc, ir.TWO_VERTS)
        P = W([[0, 0, 0], [0.02, 0.98, 0]])
        pos = W([(0, 0.5, 0), (1, 0, 0)])
        tr = pr.trace(tracer, data, P, 2, pos[:1])
        assert tr.hit.tolist()[0] == [True, False, True, False]
        ct = 0.5 / np.sqrt(0.25 + 1.0 / 3.0)
        assert np.allclose(tr.ct[:2, 0], ct, rtol=0, atol=1e-6) and tr.vis[:2].all()
        kd = np.array([0.5, 0.25, 0.125], F)
        C_ = pr.shade(tr, (1, 1, 1)).reshape(2, 9, 3)
        Wt = pr.weights(2)
        R0, R2 = (kd * tr.ct[0, 0]).astype(F), (kd * tr.ct[1, 0]).astype(F)
        by_hand = ((R0[None, :] * Wt[0][:, None]) + F(0.0) * Wt[1][:, None]) + (R2[None, :] * Wt[2][:, None]) + F(0.0) * Wt[3][:, None]
        assert np.array_equal(bits(C_[0]), bits(by_hand))
        assert np.allclose(C_[0, 0], kd * ct * 2 * np.pi * 0.28209479, rtol=0, atol=1e-6)
        assert np.allclose(C_[0, 2], 0, atol=1e-7) and (C_[0, 1] > 0).all(), "the light comes from +y, symmetric in z"
        # the yellow light leaves blue at +0
        assert not bits(pr.shade(tr, (1, 1, 0)).reshape(2, 9, 3)[:, :, 2]).any()
        # direct: the second probe sees light 0 and not light 1
        tr2 = pr.trace(tracer, data, P, 2, pos)
        assert tr2.seen.tolist() == [[True, True], [True, False]]
        plain, direct = pr.shade(tr2, (1, 1, 1)), pr.shade(tr2, (1, 1, 1), direct=True)
        only0 = pr.add_direct(plain.reshape(2, 9, 3).copy(), P, pos[:1], (1, 1, 1), tr2.seen[:, :1]).reshape(2, 27)
        assert np.array_equal(bits(direct[1]), bits(only0[1])) and not np.array_equal(bits(direct[0]), bits(only0[0]))
        assert not np.array_equal(bits(direct), bits(plain))
    finally:
        osc.close()


def binade_probes(Wm):
    """14 probes between the floor and the ceiling of indirect_ref.binade_ceiling, and the light below them"""
    xs = np.linspace(-0.9, 0.9, 7)
    return Wm([[x, 0.3, z] for x in xs for z in (-0.3, 0.4)]), (tuple(float(v) for v in Wm([0.0, 0.2, 0.0])),)


def test_the_order_of_the_sum_shows_on_the_binade_ceiling(oracle, tmp_path):
    """the fixture of the order test of tests/test_gpu_probes.py, on the CPU: the reversed sum differs in bits"""
    osc = oracle.load_scene(ir.binade_ceiling(str(tmp_path)))
    try:
        data, tracer = ir.SceneData(osc), ir.OracleTracer(osc)
        P, pos = binade_probes(ir.to_world(osc, ir.BINADE_VERTS))
        tr = pr.trace(tracer, data, P, 8, pos)
        assert tr.hit.sum() >= 14 * 40 and len(set(tr.kd[:, 0].tolist())) >= 6, "the rays meet the floor and strips across many binades"
        fwd, rev = pr.shade(tr, (1, 1, 1)), pr.shade(tr, (1, 1, 1), reverse=True)
        differ = int((bits(fwd).reshape(14, 27) != bits(rev).reshape(14, 27)).any(axis=1).sum())
        print("probes whose reversed sum differs in bits:", differ, "of 14")
        assert differ >= 1
    finally:
        osc.close()


def test_the_layout_check_program_holds_under_the_sanitizers(tmp_path):
    """the task map and the carried sums of k_probes, the grid rule, the lookup arithmetic and the argument rules:
    tools/probe_layout_check.cpp, built and run as the Makefile does"""
    r = subprocess.run(["make", "-C", CSRC, "probe_check", f"OUT={tmp_path}"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
    assert b"all checks held" in r.stdout
    assert b"-ffp-contract=off" in r.stdout and b"-fsanitize=address,undefined" in r.stdout


# ------------------------------------------------------------------------------------------ what a small volume is worth
@pytest.mark.parametrize("name", ["mixed", "dodge"])
def test_quality_of_a_small_volume_is_recorded(oracle, scenes, tmp_path, name):
    """48 x 32, yaw 0.4, one white light at (-1, 1, 1): kd * lookup from an 8 x 8 x 8 volume of m = 8 probes over the bounding box of the
    scene's vertices against kd * rt_indirect_diffuse at m = 16, as an RMS distance over the pixels where the truth is not zero.  Nobody
    has a bound for this, so none is asserted: the figures of this run are recorded in profiles/probes_ab.json and DESIGN.md 6."""
    import scenes_gen
    path = scenes_gen.mixed_materials(str(tmp_path)) if name == "mixed" else os.path.join(scenes, "dodgeColorTest.obj")
    osc = oracle.load_scene(path)
    try:
        r = pr.quality(oracle, osc, 48, 32, 0.4, [(-1.0, 1.0, 1.0)], (1, 1, 1), (8, 8, 8), 8, 16, seed=7)
    finally:
        osc.close()
    print("probe quality:", name, " ".join(f"{k} {v:.5f}" if isinstance(v, float) else f"{k} {v}" for k, v in r.items()))
    assert r["probes"] == 512 and r["covered"] == {"mixed": 93, "dodge": 242}[name]
    assert np.isfinite([r["rms"], r["truth_rms"]]).all()
