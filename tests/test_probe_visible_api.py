"""The leak-free probe lookup, the parts that need no GPU: the two entry points are declared, bound and exported and refuse a NULL context;
on a two-room scene the plain lookup of tests/probe_ref.py leaks the lit room's light through the partition and the visible lookup of
tests/probe_visible_ref.py, over the CPU checker's lightStrikes, returns exactly +0.0f there; the blend by hand on a 2 x 2 x 2 grid with
prescribed visibility bits; the layout program under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import indirect_ref as ir
import probe_ref as pr
import probe_visible_ref as pv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer-in-cpp_amd", "csrc")
NAMES = ["rt_probe_irradiance_visible_device", "rt_probe_irradiance_visible"]
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


def test_header_declares_the_calls_and_the_definition():
    text = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    assert "leak-free probe lookup" in text and "tests/probe_visible_ref.py" in text
    for phrase in ("Case A", "Case B", "out_c = s_c / W", "ONE polygon thick"):
        assert phrase in text, phrase
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\brt_status\s+" + name + r"\s*\(", code), name
    assert re.search(r"rt_probe_irradiance_visible_device\s*\([^)]*uint8_t\s*\*\s*d_mask[^)]*void\s*\*\s*stream\s*\)", code)


def test_binding_and_library_hold_the_calls(rt):
    lib = rt.load_library()
    sigs = {s[0]: s for s in rt.capi._SIGNATURES}
    for name, nargs in zip(NAMES, (9, 8)):
        assert name in rt.capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(sigs[name][2]) == nargs
    assert callable(rt.Context.probe_irradiance_visible)
    import inspect
    assert "visible" in inspect.signature(rt.Flyscene.probe_irradiance).parameters
    assert inspect.signature(rt.Flyscene.probe_irradiance).parameters["visible"].default is False
    hpp = open(os.path.join(CSRC, "flyscene.hpp")).read()
    assert re.search(r"\bbool\s+probeIrradianceVisible\s*\(", hpp)
    assert "group_probes_visible" in open(os.path.join(ROOT, "tools", "flyscene_check.cpp")).read()
    assert "--probes-visible" in open(os.path.join(CSRC, "rt_render_main.cpp")).read()
    assert "k_probe_lookup_visible" in open(os.path.join(CSRC, "rt_kernels.hip")).read()


def test_null_context_and_null_arrays_are_invalid(rt):
    lib = rt.load_library()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    g = rt.probe_grid((0, 0, 0), (1, 1, 1), (1, 1, 1))
    inv = rt.capi.RT_ERR_INVALID
    for n, q in ((1, p), (0, None)):                        # ... also with n = 0, which a context would accept
        assert lib.rt_probe_irradiance_visible_device(None, C.byref(g), q, n, q, q, q, q, None) == inv
        assert lib.rt_probe_irradiance_visible_device(None, C.byref(g), q, n, q, q, q, None, None) == inv
        assert lib.rt_probe_irradiance_visible(None, C.byref(g), q, n, q, q, q, q) == inv
        assert lib.rt_probe_irradiance_visible(None, None, q, n, q, q, q, None) == inv
    assert not any(buf)


# ------------------------------------------------------------------------------------------ the leak and its removal
def test_the_leak_shows_on_two_rooms_and_the_visible_lookup_removes_it(oracle, tmp_path):
    """The conditions on the fixture first (room B is dark: every probe in it holds +0.0f; the plain lookup is > 0 at half or more of the
    points behind the partition -- that is the leak, on the reference alone), then the claim: the visible lookup is +0.0f at every one of
    them and every mask clears the bits of the room-A corners."""
    osc = oracle.load_scene(pv.two_rooms(str(tmp_path)))
    try:
        data, tracer, W = ir.SceneData(osc), ir.OracleTracer(osc), ir.to_world(osc, pv.ROOM_VERTS)
        grid = pv.room_grid(W)
        light = [tuple(float(v) for v in W(pv.ROOM_LIGHT))]
        scale = float(W([1, 0, 0])[0] - W([0, 0, 0])[0])
        assert all(float(s) > pv.ROOM_W * scale for s in grid.step), "the partition is thinner than a grid step"
        coeff = pr.probes(tracer, data, grid.positions(), 4, light, (1, 1, 1))
        pos = grid.positions()
        wall = float(W([0, 0, 0])[0])
        room_b = pos[:, 0] > wall
        assert room_b.sum() == 8 and (~room_b).sum() == 8, "two layers of probes in each room"
        assert not bits(coeff[room_b]).any(), "every room-B probe holds exactly +0.0f"
        assert (coeff[~room_b] != 0).any(axis=1).all(), "every room-A probe is lit"
        P, N = pv.room_b_points(W)
        assert len(P) >= 64 and (P[:, 0] > wall).all() and (P[:, 0] - wall <= 0.5 * float(grid.step[0])).all()
        plain = pr.lookup(grid, coeff, P, N)
        leaking = int((plain > 0).any(axis=1).sum())
        print("points behind the partition where the plain lookup is > 0:", leaking, "of", len(P), " largest:", float(plain.max()))
        assert 2 * leaking >= len(P), "the leak, shown on the reference alone"
        vis = pv.visibility(tracer, grid, P, N)
        got, mask = pv.lookup_visible(grid, coeff, P, N, vis)
        assert not bits(got).any(), "the visible lookup is exactly +0.0f behind the partition"
        assert ((mask & 0x55) == 0).all(), "the room-A corners (dx = 0) are blocked"
        assert ((mask & 0xAA) == 0xAA).all(), "the room-B corners are seen"
        assert (pv.classes(grid, P, N, vis) == 2).all()
        # in room A, away from the partition's shadow, nothing is blocked and the two lookups agree in every bit
        PA = P.copy()
        PA[:, 0] = 2 * F(wall) - P[:, 0] - F(1.0 * scale)
        visA = pv.visibility(tracer, grid, PA, N)
        assert visA.all() and np.array_equal(bits(pv.lookup_visible(grid, coeff, PA, N, visA)[0]), bits(pr.lookup(grid, coeff, PA, N)))
        assert (pr.lookup(grid, coeff, PA, N) != 0).any()
    finally:
        osc.close()


# ------------------------------------------------------------------------------------------ the blend by hand
def hand_fixture():
    grid = pr.Grid((0.0, 1.0, 2.0), (1.0, 0.5, 2.0), (2, 2, 2))
    rng = np.random.default_rng(17)
    Cf = rng.standard_normal((8, 27)).astype(F)
    P = np.array([[0.25, 1.375, 2.5]], F)                   # weights (x) 0.75 0.25, (y) 0.25 0.75, (z) 0.75 0.25: all exact
    N = np.array([[0.6, 0.0, 0.8]], F)
    return grid, Cf, P, N


def vis_of(byte, n=1):
    return np.tile(np.array([(byte >> b) & 1 for b in range(8)], bool), (n, 1))


def test_case_a_equals_the_plain_lookup_bit_for_bit():
    grid, Cf, P, N = hand_fixture()
    plain = pr.lookup(grid, Cf, P, N)
    got, mask = pv.lookup_visible(grid, Cf, P, N, vis_of(0xff))
    assert np.array_equal(bits(got), bits(plain)) and mask.tolist() == [0xff]
    # all blocked: the plain blend, not black
    got, mask = pv.lookup_visible(grid, Cf, P, N, vis_of(0x00))
    assert np.array_equal(bits(got), bits(plain)) and mask.tolist() == [0] and (plain != 0).all()
    rng = np.random.default_rng(5)
    PP = (rng.random((200, 3)) * 4 - 1).astype(F) + grid.origin
    NN = rng.standard_normal((200, 3)).astype(F)
    for byte in (0xff, 0x00):
        assert np.array_equal(bits(pv.lookup_visible(grid, Cf, PP, NN, vis_of(byte, 200))[0]), bits(pr.lookup(grid, Cf, PP, NN)))


def test_one_blocked_corner_gives_the_renormalised_blend_by_hand():
    grid, Cf, P, N = hand_fixture()
    wx, wy, wz = (F(0.75), F(0.25)), (F(0.25), F(0.75)), (F(0.75), F(0.25))
    B, Wsum = np.zeros(27, F), F(0.0)
    for b in range(8):
        if b == 5:
            continue
        w = F(F(wz[b >> 2] * wy[(b >> 1) & 1]) * wx[b & 1])
        Wsum = F(Wsum + w)
        B = (B + w * Cf[b]).astype(F)                      # probe index (iz * 2 + iy) * 2 + ix = b
    Y = pr.sh9(N[0])
    want = np.zeros(3, F)
    for j in range(9):
        want = (want + B[j * 3:j * 3 + 3] * Y[j]).astype(F)
    want = (want / Wsum).astype(F)
    got, mask = pv.lookup_visible(grid, Cf, P, N, vis_of(0xff & ~0x20))
    assert np.array_equal(bits(got[0]), bits(want)) and mask.tolist() == [0xdf]
    assert float(Wsum) == 1.0 - 0.25 * 0.25 * 0.25 and not np.array_equal(bits(got), bits(pr.lookup(grid, Cf, P, N)))


def test_a_blocked_corner_of_weight_zero_changes_nothing():
    grid, Cf, P, N = hand_fixture()
    P = P.copy()
    P[0, 0] = 0.0                                           # on the plane of the near probes: the corners dx = 1 have weight 0
    seen_all_but, _ = pv.lookup_visible(grid, Cf, P, N, vis_of(0xff & ~0x02))
    both_blocked, _ = pv.lookup_visible(grid, Cf, P, N, vis_of(0xff & ~0x0a))
    only_near, mask = pv.lookup_visible(grid, Cf, P, N, vis_of(0x55))
    plain = pr.lookup(grid, Cf, P, N)
    # (case B over the corners of weight > 0, whose weights add up to 1 exactly; the plain blend adds +-0 for the others)
    for got in (seen_all_but, both_blocked, only_near):
        assert np.array_equal(bits(got), bits(plain))
    assert mask.tolist() == [0x55]
    # and a blocked corner that has weight is not nothing
    assert not np.array_equal(bits(pv.lookup_visible(grid, Cf, P, N, vis_of(0xff & ~0x04))[0]), bits(plain))


def test_an_axis_of_one_layer_is_handled_as_defined():
    _, Cf, P, N = hand_fixture()
    grid = pr.Grid((0.0, 1.0, 2.0), (1.0, 0.5, 2.0), (2, 1, 2))
    read, w, idx, Pc = pv.corners(grid, P)
    assert read.tolist() == [True, True, False, False, True, True, False, False]
    assert idx[0].tolist() == [0, 1, 0, 0, 2, 3, 0, 0] and w[0, :2].tolist() == [0.5625, 0.1875]
    assert Pc[0, 5].tolist() == [1.0, 1.0, 4.0]
    plain = pr.lookup(grid, Cf[:4], P, N)
    got, mask = pv.lookup_visible(grid, Cf[:4], P, N, vis_of(0xff))
    assert np.array_equal(bits(got), bits(plain)) and mask.tolist() == [0x33], "the bits of corners that are not read stay 0"
    got, mask = pv.lookup_visible(grid, Cf[:4], P, N, vis_of(0x32 | 0xcc))
    assert mask.tolist() == [0x32] and not np.array_equal(bits(got), bits(plain))
    B = ((F(0.1875) * Cf[1] + F(0.1875) * Cf[2]).astype(F) + F(0.0625) * Cf[3]).astype(F)
    Wsum = F(F(F(0.1875) + F(0.1875)) + F(0.0625))
    want = (pr.evaluate(B, N[0])[0] / Wsum).astype(F)
    assert np.array_equal(bits(got[0]), bits(want))
    # no point: +0.0f and mask 0 whatever the rest is
    z, mask = pv.lookup_visible(grid, np.full_like(Cf[:4], np.nan), np.tile(P, (2, 1)), [[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0]], vis_of(0xff, 2))
    assert not bits(z).any() and mask.tolist() == [0, 0]


def test_the_layout_check_program_holds_under_the_sanitizers(tmp_path):
    """the lane / task / staging map of k_probe_lookup_visible for every n mod 8 and every pattern of skipped corners, the choice of the
    corners, the arithmetic and the argument rule: tools/probe_visible_layout_check.cpp, built and run as the Makefile does"""
    r = subprocess.run(["make", "-C", CSRC, "probe_visible_check", f"OUT={tmp_path}"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
    assert b"all checks held" in r.stdout
    assert b"-ffp-contract=off" in r.stdout and b"-fsanitize=address,undefined" in r.stdout
