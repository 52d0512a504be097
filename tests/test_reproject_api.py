"""The temporal reprojection (rt_reproject_device, rt_reproject, rt_reproject_map) without a device: the pins of the definition, header,
binding and library agree, the defaults are the header's, rt_reproject_map equals the Python restatement (tests/reproject_ref.py) bit for
bit and sends a pixel where a double-precision evaluation of the two cameras sends it, a still camera accumulates the running mean, the
argument rules hold, the launcher's grid and tile are the denoiser's and the inputs of the GPU tests take every branch.

rt_create needs a device, so with a context only the NULL-context rule can be called here; every other RT_ERR_INVALID / RT_ERR_UNSUPPORTED
rule is decided by rt_reproject_layout.hpp's rp_args, which tools/reproject_layout_check.cpp covers under a sanitizer (run below)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reproject_ref as rr
import test_upsample_api as ua
from test_upsample_api import bits, covered_gbuffer, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
CSRC = os.path.join(ROOT, "raytracer-in-cpp_amd", "csrc")
F = np.float32
INF = float("inf")
CALLS = {"rt_default_reproject_params": 1, "rt_reproject_map": 3, "rt_reproject_device": 14, "rt_reproject": 13}
DEFAULT_BITS = (32, 0x40000000, 0x3C800000, 0x3E800000)      # max_history, sigma normal, depth, albedo
DEFAULTS = (2.0, 0.015625, 0.25)
INHERITED = (2.0, 0.125, 0.25)                               # rt_default_upsample_params: the depth scale that lost the experiment below
TIGHT = ua.TIGHT
ALL_INF = ua.ALL_INF
SIZES = ((1, 1), (63, 1), (64, 4), (65, 5), (1, 9), (130, 7))        # (width, rows)
PIN_YAW = ("370396E1 3F8230F7 00000000 BFF84A4B", "366BCAA8 3C3D2C6A 3F800000 BF0F84E2", "33EBCAA8 39BD2C6A 00000000 3F7B83D9")
PIN_DEFAULT = ("00000000 3F866801 00000000 C2BFFC34", "00000000 3CEC6257 3F800000 C1E3024C", "00000000 3860208F 00000000 3F728C31")


def identity(**entries):
    """the identity map with entries replaced: x_W=0.5 is m[x][W] = 0.5f"""
    m = rr.IDENTITY.copy()
    for k, v in entries.items():
        m["xyd".index(k[0]), "EUVW".index(k[2])] = v
    return m


def maps(rt, width, rows):
    """name -> map (3, 4) of the GPU test: the identity, half-pixel and whole-pixel shifts in each direction, a yaw pair of the image's
    own size and a map that sends part of the image behind the previous camera (den = 1 - y / 2 - x / 40)"""
    out = {"identity": identity()}
    for name, v in (("half", 0.5), ("whole", 1.0)):
        for axis in "xy":
            for sign in (1.0, -1.0):
                out[f"{name}{'+' if sign > 0 else '-'}{axis}"] = identity(**{f"{axis}_W": sign * v})
    out["yaw"] = rt.reproject_map(rt.default_camera(max(width, 2), max(rows, 2), 0.42), rt.default_camera(max(width, 2), max(rows, 2), 0.40))
    out["behind"] = identity(d_V=-0.5, d_U=-0.025)
    return out


def synthetic(rows, width, ch, seed=31):
    """seeded inputs -> (cur, g_cur, hist, g_hist, len_hist): the buffers of the upsample's synthetic() (holes, fractional alpha, a depth
    step, two normals, three albedos) as the current frame; the history's buffers are those with a seeded tenth of the covered pixels
    0.25 deeper and further holes; the lengths are drawn from {0, 1, 2, 31, 254, 255}"""
    rng = np.random.default_rng(seed + 1000 * rows + 7 * width)
    _, _, g = ua.synthetic(rows, width, 3, 2)
    cur, hist = rng.random((rows, width, 3)).astype(F), rng.random((rows, width, 3)).astype(F)
    gh = g.copy()
    flip = (rng.random((rows, width)) < 0.1) & (gh[..., 0] > 0)
    gh[flip, 1] = (gh[flip, 1] + F(0.25) * gh[flip, 0]).astype(F)
    gh[rng.random((rows, width)) < 0.05] = 0.0
    lens = np.array([0, 1, 2, 31, 254, 255], np.uint8)[rng.integers(0, 6, (rows, width))]
    if ch == 1:
        cur, hist = cur[..., 0].copy(), hist[..., 0].copy()
    return cur, g, hist, gh, lens


# ------------------------------------------------------------------------------------------ the pins
def test_the_pins_of_the_header():
    text = open(HEADER).read()
    assert "tests/reproject_ref.py" in text
    g2 = covered_gbuffer(1, 2)
    one = np.ones((1, 2), np.uint8)
    P = rr.Params
    out, ln = rr.reproject(np.array([[0.0, 1.0]], F), g2, np.array([[1.0, 0.0]], F), g2, one, identity(), P())
    assert bits(out).tolist() == [[0x3F000000, 0x3F000000]] and ln.tolist() == [[2, 2]] and "-> 3F000000 3F000000, len {2, 2}" in text
    out, ln, taps = rr.reproject(np.zeros((1, 2), F), g2, np.array([[1.0, 0.0]], F), g2, one, identity(x_W=0.5), P(), True)
    assert bits(out).tolist() == [[0x3E800000, 0]] and ln.tolist() == [[2, 2]] and taps.tolist() == [[2, 1]] and "-> 3E800000" in text
    out, ln = rr.reproject(np.array([[0.0, 1.0]], F), g2, np.array([[1.0, 0.0]], F), covered_gbuffer(1, 2, [1.0, 3.0]), one, identity(), P(255, INF, 0.25, INF))
    assert bits(out).tolist() == [[0x3F000000, 0x3F800000]] and ln.tolist() == [[2, 1]] and "-> 3F000000 3F800000" in text
    out, ln = rr.reproject(np.array([[0.0, 1.0]], F), g2, np.array([[1.0, 0.0]], F), g2, np.array([[255, 0]], np.uint8), identity(), P(4))
    assert bits(out).tolist() == [[0x3F400000, 0x3F800000]] and ln.tolist() == [[4, 1]] and "-> 3F400000 3F800000, len {4, 1}" in text
    g3 = covered_gbuffer(3, 1)
    out, ln = rr.reproject(np.zeros((3, 1), F), g3, np.array([[1.0], [2.0], [3.0]], F), g3, np.ones((3, 1), np.uint8), identity(y_W=-1.0), P())
    assert bits(out).tolist() == [[0], [0x3F000000], [0x3F800000]] and ln.tolist() == [[1], [2], [2]]
    for line in PIN_YAW + PIN_DEFAULT:
        assert line in text


def test_the_pinned_maps(rt):
    for (cur, prev), pin in ((((96, 64, 0.42), (96, 64, 0.40)), PIN_YAW), (((1920, 1080, 0.05), (1920, 1080, 0.0)), PIN_DEFAULT)):
        m = rt.reproject_map(rt.default_camera(*cur), rt.default_camera(*prev))
        assert tuple(" ".join("%08X" % v for v in row) for row in bits(m)) == pin
        assert same(m, rr.reproject_map(rt.default_camera(*cur), rt.default_camera(*prev)))


# ------------------------------------------------------------------------------------------ header, binding, library
def test_header_binding_and_library_agree(rt):
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    sigs = dict((s[0], s) for s in rt.capi._SIGNATURES)
    lib = rt.load_library()
    for name, nargs in CALLS.items():
        m = re.search(r"\b(?:rt_status|size_t|void)\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == nargs
        assert name in rt.capi.EXPORTED_SYMBOLS and len(sigs[name][2]) == nargs
        assert getattr(lib, name).argtypes == sigs[name][2]
    assert re.search(r"^\s*#\s*define\s+RT_REPROJECT_MAX_HISTORY\s+255\s*$", code, flags=re.M) and rt.capi.RT_REPROJECT_MAX_HISTORY == 255 == rr.MAX_HISTORY
    assert C.sizeof(rt.capi.rt_reproject_params) == 16
    names = ["max_history", "sigma_normal", "sigma_depth", "sigma_albedo"]
    assert [f[0] for f in rt.capi.rt_reproject_params._fields_] == names
    m = re.search(r"typedef struct rt_reproject_params \{(.*?)\} rt_reproject_params;", code, flags=re.S)
    assert m and re.findall(r"\b(max_history|sigma_\w+)\b", m.group(1)) == names


def test_front_ends_and_sources(rt):
    assert callable(rt.Context.reproject) and callable(rt.reproject_params) and callable(rt.reproject_map)
    fs = rt.Flyscene()
    assert fs.temporal is None and fs.history_lengths() is None and callable(fs.reset_history)
    assert "temporal" in rt.Flyscene.ambient_occlusion.__code__.co_varnames
    hpp = open(os.path.join(CSRC, "flyscene.hpp")).read()
    assert "setTemporal(const rt_reproject_params *" in hpp and "void resetHistory()" in hpp and "bool reproject(" in hpp
    assert "--temporal" in open(os.path.join(CSRC, "rt_render_main.cpp")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^reproject_check:", mk, flags=re.M) and re.search(r"^SRC\s*:=.*\brt_reproject\.hip\b", mk, flags=re.M)
    for target in ("librt_mi355x.so", "librt_mi355x_work.so"):
        assert re.search(r"^\$\(OUT\)/%s:.*rt_reproject_layout\.hpp" % re.escape(target), mk, flags=re.M), target
    for other in ("rt_kernels.hip", "rt_denoise.hip", "rt_upsample.hip"):
        assert "k_reproject" not in open(os.path.join(CSRC, other)).read(), "the operator is a translation unit of its own"
    unit = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "rt_reproject.hip")).read())          # (the code, not its comments)
    assert "k_reproject" in unit and "getenv" not in unit and "__shared__" not in unit and "atomic" not in unit and "Graph" not in unit
    lay = open(os.path.join(CSRC, "rt_reproject_layout.hpp")).read()
    assert "rt_kernels" not in lay and "hip_runtime" not in lay


def test_the_launch_takes_the_denoisers_tiles_and_grid():
    unit, capi, lay = (open(os.path.join(CSRC, f)).read() for f in ("rt_reproject.hip", "rt_capi.cpp", "rt_reproject_layout.hpp"))
    assert "constexpr int kRpThreads = kDnTileH * 64;" in unit and "__global__ __launch_bounds__(kRpThreads) void k_reproject(" in unit
    assert "for (uint32_t tile = blockIdx.x; tile < T.tiles; tile += gridDim.x) {" in unit
    assert "const DnLane L = dn_lane(T, width, rows, tile, wave, lane);" in unit and "const uint64_t p = dn_pixel(width, L.x, L.y);" in unit
    assert "const DnTiles T = dn_tiles(width, rows);" in unit
    assert unit.count("<<<grid, kRpThreads, 0, st>>>") == 2
    assert "launch_reproject(dn_grid(dn_tiles(width, rows).tiles, c->cus), stream_or_own(c, stream), " in capi
    assert "constexpr int32_t kRpMaxHistory = 255;" in lay and '#include "rt_denoise_layout.hpp"' in lay


def test_default_params_bits(rt):
    lib = rt.load_library()
    p = rt.capi.rt_reproject_params()
    lib.rt_default_reproject_params(C.byref(p))
    got = (p.max_history,) + tuple(int(np.array([getattr(p, n)], F).view(np.uint32)[0]) for n in ("sigma_normal", "sigma_depth", "sigma_albedo"))
    assert got == DEFAULT_BITS
    u = rt.upsample_params()
    assert (p.sigma_normal, p.sigma_albedo) == (u.sigma_normal, u.sigma_albedo) and p.sigma_depth == u.sigma_depth / 8 == DEFAULTS[1]
    text = open(HEADER).read()
    for b in DEFAULT_BITS[1:]:
        assert "(%08X)" % b in text
    lib.rt_default_reproject_params(None)                # tolerated
    q = rt.reproject_params(max_history=4, sigma_depth=INF)
    assert (q.max_history, q.sigma_normal, q.sigma_depth, q.sigma_albedo) == (4, 2.0, INF, 0.25)
    assert rr.Params(p.max_history, p.sigma_normal, p.sigma_depth, p.sigma_albedo).valid()
    assert not rr.Params(0).valid() and not rr.Params(256).valid() and not rr.Params(4, 0.0).valid() and not rr.Params(4, 1.0, float("nan")).valid()


# ------------------------------------------------------------------------------------------ the map
def moved(rt, w, h, yaw, shift):
    """the yaw camera with its centre (and the translation column of inv_view) moved by `shift`"""
    cam = rt.default_camera(w, h, yaw)
    for k in range(3):
        cam.center[k] = float(F(cam.center[k]) + F(shift[k]))
        cam.inv_view[k * 4 + 3] = float(F(cam.inv_view[k * 4 + 3]) + F(shift[k]))
    return cam


def camera_pairs(rt):
    pairs = []
    for w, h in ((37, 21), (96, 64), (1920, 1080)):
        for y0, y1 in ((0.0, 0.05), (0.4, 0.42), (0.8, 0.6), (0.2, 0.0)):
            pairs.append((rt.default_camera(w, h, y1), rt.default_camera(w, h, y0)))
        pairs.append((moved(rt, w, h, 0.42, (0.0625, -0.03125, 0.125)), rt.default_camera(w, h, 0.4)))
        pairs.append((rt.default_camera(w, h, 0.1), moved(rt, w, h, 0.0, (-0.25, 0.0, 0.5))))
    return pairs


def test_the_map_equals_the_restatement_bit_for_bit(rt):
    pairs = camera_pairs(rt)
    assert len(pairs) >= 12
    for cur, prev in pairs:
        got, want = rt.reproject_map(cur, prev), rr.reproject_map(cur, prev)
        assert want is not None and same(got, want), (list(cur.viewport), bits(got).tolist(), bits(want).tolist())
        assert not same(got, rr.IDENTITY)
    assert any(rr.reproject_map(c, p)[0, 0] != 0 for c, p in pairs), "a translated centre gives an E column"


def test_equal_cameras_give_the_identity_by_rule(rt):
    for w, h, yaw in ((37, 21, 0.0), (96, 64, 0.4), (1920, 1080, 0.8)):
        cam = rt.default_camera(w, h, yaw)
        m = rt.reproject_map(cam, rt.default_camera(w, h, yaw))
        assert bits(m).tolist() == bits(rr.IDENTITY).tolist() == [[0, 0x3F800000, 0, 0], [0, 0, 0x3F800000, 0], [0, 0, 0, 0x3F800000]]
        assert same(rr.reproject_map(cam, cam), rr.IDENTITY)
        arith = rr.reproject_map(cam, cam, double=True)          # the arithmetic alone comes close, and need not arrive
        assert np.abs(arith - rr.IDENTITY).max() < 1e-9 * max(w, h)


def test_the_map_refuses_what_it_must(rt):
    lib = rt.load_library()
    good = rt.default_camera(96, 64, 0.4)
    m = (C.c_float * 12)(*([7.0] * 12))
    inv = rt.capi.RT_ERR_INVALID
    assert lib.rt_reproject_map(None, C.byref(good), m) == inv and lib.rt_reproject_map(C.byref(good), None, m) == inv
    assert lib.rt_reproject_map(C.byref(good), C.byref(good), None) == inv

    def broken(change):
        cam = rt.default_camera(96, 64, 0.42)
        change(cam)
        return cam

    def field(name, k, v):
        def change(cam):
            if k is None:
                setattr(cam, name, v)
            else:
                getattr(cam, name)[k] = v
        return change

    bad = [field("center", 1, float("nan")), field("inv_view", 5, INF), field("fovy", None, float("nan")), field("aspect", None, -INF),
           field("viewport", 0, float("nan")), field("viewport", 2, 0.0), field("viewport", 3, 0.0)]
    for change in bad:
        for cur, prev in ((broken(change), good), (good, broken(change))):
            assert lib.rt_reproject_map(C.byref(cur), C.byref(prev), m) == inv
            assert rr.reproject_map(cur, prev) is None
            with pytest.raises(ValueError):
                rt.reproject_map(cur, prev)

    def flatten(cam):
        for k in range(3):
            cam.inv_view[8 + k] = cam.inv_view[k]           # two equal rows: singular
    assert lib.rt_reproject_map(C.byref(good), C.byref(broken(flatten)), m) == inv and rr.reproject_map(good, broken(flatten)) is None
    assert lib.rt_reproject_map(C.byref(broken(flatten)), C.byref(good), m) == rt.capi.RT_OK, "only the previous camera is inverted"
    m = (C.c_float * 12)(*([7.0] * 12))
    assert lib.rt_reproject_map(C.byref(good), C.byref(broken(flatten)), m) == inv and list(m) == [7.0] * 12, "a refusal writes nothing"


def test_the_map_sends_raster_points_where_the_cameras_say(rt):
    """C_prev + z' * (screenToWorld_prev(x', y') - C_prev) = C_cur + z * (screenToWorld_cur(x, y) - C_cur), with rt_screen_to_world's own
    float results as the world points.  Bound: screenToWorld rounds its raster-to-[-1, 1] step and four products and sums to float32, a
    relative 2^-24 each on values of at most |C| + z |D| <= 8; a raster unit is 2 / width of the screen plane at distance 1, so an error e
    in the world moves x' by at most e * z-scaled width / 2 pixels.  With ten such roundings per camera, two cameras and the twelve
    float casts of the map, 64 * 2^-24 * max(width, rows) pixels is a safe ceiling; z' (about 1) gets the same count without the width."""
    lib = rt.load_library()
    eps = 2.0 ** -24
    worst = 0.0
    for cur, prev in camera_pairs(rt):
        w, h = int(cur.viewport[2]), int(cur.viewport[3])
        m = rt.reproject_map(cur, prev).astype(np.float64)
        o = (C.c_float * 3)()
        for x, y, z in ((0, 0, 1.0), (w - 1, h - 1, 2.5), (w // 2, h // 3, 1.75), (w // 5, h - 1, 0.75)):
            lib.rt_screen_to_world(C.byref(cur), C.c_float(x), C.c_float(y), o)
            Cc = np.array(list(cur.center), np.float64)
            P = Cc + z * (np.array(list(o), np.float64) - Cc)
            num = m[:, 0] / z + m[:, 1] * x + m[:, 2] * y + m[:, 3]
            xp, yp, zp = num[0] / num[2], num[1] / num[2], z * num[2]
            o2 = (C.c_float * 3)()
            lib.rt_screen_to_world(C.byref(prev), C.c_float(xp), C.c_float(yp), o2)
            Cp = np.array(list(prev.center), np.float64)
            Q = Cp + zp * (np.array(list(o2), np.float64) - Cp)
            err = float(np.abs(Q - P).max())
            worst = max(worst, err * max(w, h))
            # the world error of 64 roundings of values up to 8, and the float rounding of (xp, yp) handed to rt_screen_to_world
            assert err <= 64 * eps * 8 + 4.0 * eps * max(w, h) * 2.0 / min(w, h), (w, h, x, y, z, err)
    print(f"largest world distance times the image size: {worst:.3e}")


# ------------------------------------------------------------------------------------------ the map against the oracle's frames
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
# recorded in DESIGN.md §5, Temporal reprojection: covered pixels, largest |x' - x'_double| and |y' - ...| in pixels, largest |z' - ...| / z',
# pixels away from every change of face id in both frames, and how many of those find their own face in the yaw-0.40 frame
MAP_MEASURED = {"cube": (2264, 1419), "dodge": (961, 367)}   # (7.9e-06 px, 1.2e-07; 98.3 % of all agree), (1.4e-05 px, 1.3e-07; 96.9 %)


def oracle_frame(oracle, osc, w, h, yaw):
    """(faces [h, w], ts [h, w]) of the one-ray pinhole frame of the oracle at `yaw` (t = -1 where nothing is hit)"""
    import ao_ref
    (_, _, f, t), _ = ao_ref.camera_points(oracle, osc, w, h, yaw)
    return f.reshape(h, w), t.reshape(h, w)


@pytest.mark.parametrize("name", ["cube", "dodge"])
def test_the_map_against_the_oracles_frames(rt, oracle, name):
    """Covered pixels of the oracle's 96 x 64 frame at yaw 0.42, reprojected to yaw 0.40 with the oracle's depths through the LIBRARY's
    map in float32 (steps 2 of the definition), against the same point found in double: P = C + z B_cur (x, y, 1), then
    z' (x', y', 1) = B_prev^-1 (P - C_prev) solved by numpy in float64.  Margin: each num_r is a sum of four terms of magnitude at most
    max(width, rows) + 2 whose factors carry the 2^-24 of a float entry, with three more roundings for the sums and one for the product:
    at most 8 * 2^-24 relative to that magnitude; the quotient adds its own rounding and the denominator's 8: 17 * 2^-24 * (size + 2)
    pixels for x' and y', rounded up to 32; z' = z * den is 8 + 1 roundings, taken as 16 * 2^-24 relative.  The face id at the rounded
    (x', y') of the yaw-0.40 frame is the pixel's own wherever both places are at least 2 pixels from any change of face id."""
    W, H = 96, 64
    osc = oracle.load_scene(os.path.join(SCENES, "cube.obj" if name == "cube" else "dodgeColorTest.obj"))
    try:
        f1, t1 = oracle_frame(oracle, osc, W, H, 0.42)
        f0, _ = oracle_frame(oracle, osc, W, H, 0.40)
    finally:
        osc.close()
    cur, prev = rt.default_camera(W, H, 0.42), rt.default_camera(W, H, 0.40)
    m = rt.reproject_map(cur, prev)
    cov = f1 >= 0
    z = np.where(cov, t1, F(1.0)).astype(F)
    xp, yp, zr, den = rr.project(m, W, H, z)
    Bc, Bp = np.array(rr.ray_matrix(rr.Cam(cur))), np.array(rr.ray_matrix(rr.Cam(prev)))
    Cc, Cp = np.array(list(cur.center), np.float64), np.array(list(prev.center), np.float64)
    ys, xs = np.nonzero(cov)
    pts = Cc[:, None] + z[ys, xs].astype(np.float64) * (Bc @ np.stack([xs, ys, np.ones(len(xs))]).astype(np.float64))
    v = np.linalg.solve(Bp, pts - Cp[:, None])
    xd, yd, zd = v[0] / v[2], v[1] / v[2], v[2]
    eps = 2.0 ** -24
    dx, dy = np.abs(xp[ys, xs] - xd).max(), np.abs(yp[ys, xs] - yd).max()
    dz = (np.abs(zr[ys, xs] - zd) / zd).max()
    assert (den[ys, xs] > 0).all()
    assert max(dx, dy) <= 32 * eps * (max(W, H) + 2) and dz <= 16 * eps, (dx, dy, dz)
    rx, ry = np.rint(xd).astype(int), np.rint(yd).astype(int)
    inside = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    calm1, calm0 = ~ua.near_a_change_of_face(f1, 2), ~ua.near_a_change_of_face(f0, 2)
    sel = inside & calm1[ys, xs]
    sel[inside] &= calm0[ry[inside], rx[inside]]
    agree = f0[ry[sel], rx[sel]] == f1[ys[sel], xs[sel]]
    every = f0[ry[inside], rx[inside]] == f1[ys[inside], xs[inside]]
    print(f"{name}: {int(cov.sum())} covered, |dx| {dx:.3e} |dy| {dy:.3e} px, |dz|/z {dz:.3e}; {int(sel.sum())} calm pixels, {int(agree.sum())} agree; "
          f"of all {int(inside.sum())} inside the frame {every.mean():.4f} agree")
    assert sel.sum() > 0 and agree.all()
    if MAP_MEASURED[name] is not None:
        assert (int(cov.sum()), int(sel.sum())) == MAP_MEASURED[name]


# ------------------------------------------------------------------------------------------ usefulness, measured once on the CPU
EXPERIMENT = dict(width=64, height=40, frames=8, yaw0=0.30, step=0.02, grid=2, radius=0.5, truth_grid=16)
# as recorded in DESIGN.md §5: RMS distance from 16 x 16 occlusion at the last camera over its covered pixels, of the last 2 x 2 frame alone and
# of the image accumulated over the 8 frames with rt_default_reproject_params, and the share of covered pixels of the last frame at len 1
# measured (mixed / dodgeColorTest): single 0.11600 / 0.02824; accumulated 0.08499 / 0.02414, history lost at 12.5 % / 2.8 % of the covered
# pixels; with the upsample's depth scale 0.125 instead of 0.015625: 0.08149 / 0.04837 -- worse than the single frame on dodgeColorTest
USE_MEASURED = {"mixed": 152, "dodge": 394}


@pytest.mark.parametrize("name", ["mixed", "dodge"])
def test_accumulated_occlusion_is_closer_to_the_truth_than_a_single_frame(rt, oracle, tmp_path, name):
    """2 x 2 ambient occlusion with seed = frame index over 8 frames at yaw 0.30 .. 0.44, 64 x 40, accumulated with the restatement under
    rt_default_reproject_params and the library's maps, against 16 x 16 occlusion at the last camera.  Asserted: the direction."""
    import ao_ref
    import gbuffer_ref as gr
    import scenes_gen
    e = EXPERIMENT
    w, h = e["width"], e["height"]
    path = scenes_gen.mixed_materials(str(tmp_path)) if name == "mixed" else os.path.join(SCENES, "dodgeColorTest.obj")
    osc = oracle.load_scene(path)
    try:
        fn = osc.arrays()["face_normal"]

        def occlusion(yaw, seed, grid):
            (o, d, f, t), _ = ao_ref.camera_points(oracle, osc, w, h, yaw)
            P, N = ao_ref.hit_points(o, d, f, t, fn)
            return ao_ref.ao_of(ao_ref.counts(osc, P, N, seed, grid, e["radius"]), grid).reshape(h, w)

        yaws = [e["yaw0"] + e["step"] * k for k in range(e["frames"])]
        frames = [(occlusion(y, k, e["grid"]), gr.cpu_frame(oracle, osc, oracle.camera(w, h, y), w, h, 1, 0, 1)) for k, y in enumerate(yaws)]
        truth = occlusion(yaws[-1], 0, e["truth_grid"])
    finally:
        osc.close()
    d = rt.reproject_params()
    p = rr.Params(d.max_history, d.sigma_normal, d.sigma_depth, d.sigma_albedo)
    acc, ln = frames[0][0], np.ones((h, w), np.uint8)
    for k in range(1, e["frames"]):
        m = rt.reproject_map(rt.default_camera(w, h, yaws[k]), rt.default_camera(w, h, yaws[k - 1]))
        acc, ln = rr.reproject(frames[k][0], frames[k][1], acc, frames[k - 1][1], ln, m, p)
    cov = frames[-1][1][..., 0] > 0
    rms = lambda a: float(np.sqrt(np.mean((a[cov].astype(np.float64) - truth[cov]) ** 2)))
    single, accumulated, lost = rms(frames[-1][0]), rms(acc), float((ln[cov] == 1).mean())
    print(f"{name}: {int(cov.sum())} covered pixels; single frame {single:.5f}, accumulated {accumulated:.5f}, history lost at {lost:.4f}, "
          f"mean length {ln[cov].mean():.2f}")
    assert accumulated < single
    assert same(acc[~cov], frames[-1][0][~cov]) and (ln[~cov] == 1).all()
    if USE_MEASURED[name] is not None:
        assert int(cov.sum()) == USE_MEASURED[name]


# ------------------------------------------------------------------------------------------ properties of the restatement
def test_a_still_camera_accumulates_the_running_mean():
    """identity map, equal buffers: out = hist + (cur - hist) / n, so k calls from len = 1 hold the mean of k + 1 frames -- within (k + 1)
    roundings of a value below 1 per step, 3 * 2^-24 each (a subtraction, a division, an addition) -- and len saturates at max_history"""
    rows, width, frames = 9, 23, 12
    rng = np.random.default_rng(3)
    _, g, _, _, _ = synthetic(rows, width, 3)
    imgs = rng.random((frames, rows, width, 3)).astype(F)
    cov = (g[..., 0] > 0) & (g[..., 1] / np.where(g[..., 0] > 0, g[..., 0], 1) > 0)
    for cap in (255, 5):
        acc, ln = imgs[0], np.ones((rows, width), np.uint8)
        for k in range(1, frames):
            acc, ln, taps = rr.reproject(imgs[k], g, acc, g, ln, rr.IDENTITY, rr.Params(cap, *DEFAULTS), True)
            assert (taps[cov] == 1).all() and (taps[~cov] == 0).all(), "one tap of weight 1.0f per covered pixel"
            assert (ln[cov] == min(k + 1, cap)).all() and (ln[~cov] == 1).all()
            assert same(acc[~cov], imgs[k][~cov]), "the background is the current frame"
            if k + 1 <= cap:
                mean = imgs[:k + 1].astype(np.float64).mean(axis=0)
                assert np.abs(acc.astype(np.float64) - mean)[cov].max() <= 3 * (k + 1) * 2.0 ** -24
        assert (ln[cov] == min(frames, cap)).all()


def test_lost_history_starts_again_at_one():
    rows, width = 6, 40
    g = covered_gbuffer(rows, width)
    cur, hist = np.full((rows, width), 0.25, F), np.full((rows, width), 0.75, F)
    ln = np.full((rows, width), 9, np.uint8)
    P = rr.Params(32, *DEFAULTS)
    out, lo = rr.reproject(cur, g, hist, g, ln, identity(x_W=-3.0), P)               # the first three columns come from outside the frame
    assert (lo[:, :2] == 1).all() and same(out[:, :2], cur[:, :2]) and (lo[:, 3:] == 10).all()
    hidden = covered_gbuffer(rows, width, np.where(np.arange(width) < 20, 1.0, 3.0)[None, :].repeat(rows, 0))
    out, lo = rr.reproject(cur, g, hist, hidden, ln, identity(), P)                    # the right half was behind something else
    assert (lo[:, 20:] == 1).all() and same(out[:, 20:], cur[:, 20:]) and (lo[:, :20] == 10).all()
    out, lo = rr.reproject(cur, g, hist, g, ln, identity(d_W=-1.0, d_U=0.05), P)       # den = x / 20 - 1: behind the previous camera up to x = 20
    assert (lo[:, :21] == 1).all() and same(out[:, :21], cur[:, :21])
    out, lo = rr.reproject(cur, g, hist, g, np.zeros((rows, width), np.uint8), identity(), P)
    assert (lo == 1).all() and same(out, cur), "len_hist == 0 is no history"


def test_the_inputs_of_the_gpu_tests_take_every_branch(rt):
    for width, rows in SIZES:
        cur, g, hist, gh, lens = synthetic(rows, width, 1)
        if width * rows < 256:
            continue
        for name, m in maps(rt, width, rows).items():
            for sig in (ALL_INF, DEFAULTS, TIGHT):
                out, lo, taps = rr.reproject(cur, g, hist, gh, lens, m, rr.Params(32, *sig), True)
                cov = g[..., 0] > 0
                assert (lo[~cov] == 1).all() and same(out[~cov], cur[~cov])
                assert (taps > 0).any() and (taps[cov] == 0).any(), (name, sig)
                if name.startswith("half"):
                    assert (taps >= 2).any()
        out, lo = rr.reproject(cur, g, hist, gh, lens, maps(rt, width, rows)["identity"], rr.Params(255))
        assert {1, 2, 3, 32, 255} <= set(np.unique(lo).tolist())
        behind = rr.project(maps(rt, width, rows)["behind"], width, rows, np.ones((rows, width), F))[3]
        assert (behind > 0).any() and (behind <= 0).any()


# ------------------------------------------------------------------------------------------ argument rules
def test_a_null_context_is_refused_and_writes_nothing(rt):
    lib = rt.load_library()
    p = rt.reproject_params()
    m = (C.c_float * 12)(*rr.IDENTITY.reshape(-1).tolist())
    cur, g, hist, ln, out, lo = np.zeros(6, F), np.zeros(48, F), np.zeros(6, F), np.ones(6, np.uint8), np.full(6, 7.0, F), np.full(6, 9, np.uint8)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    inv = rt.capi.RT_ERR_INVALID
    assert lib.rt_reproject_device(None, ptr(cur), 1, ptr(g), ptr(hist), ptr(g), ptr(ln), 3, 2, m, C.byref(p), ptr(out), ptr(lo), None) == inv
    assert lib.rt_reproject(None, ptr(cur), 1, ptr(g), ptr(hist), ptr(g), ptr(ln), 3, 2, m, C.byref(p), ptr(out), ptr(lo)) == inv
    assert lib.rt_reproject_device(None, None, 0, None, None, None, None, 0, -1, None, None, None, None, None) == inv
    assert lib.rt_reproject(None, None, 0, None, None, None, None, 0, -1, None, None, None, None) == inv
    assert (out == 7.0).all() and (lo == 9).all()


def test_the_layout_check_program_holds_under_the_sanitizers(tmp_path):
    """every other argument rule, the overlap rule, the tap arithmetic at the edges of (-1, width) and the map's refusals:
    tools/reproject_layout_check.cpp, built and run as the Makefile does"""
    r = subprocess.run(["make", "-C", CSRC, "reproject_check", f"OUT={tmp_path}"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
    assert b"reproject_layout_check: all checks held" in r.stdout
    src = open(os.path.join(ROOT, "tools", "reproject_layout_check.cpp")).read()
    for rule in ("INT32_MAX", "out + k", "len_out + k", "nextafterf", "the host form has no overlap rule"):
        assert rule in src


def test_python_side_refusals_need_no_device(rt):
    with pytest.raises(ValueError):
        rt.Context.reproject(None, object(), None, None, None, None, 4, 4, rr.IDENTITY, params=rt.reproject_params(), channels=2)
    with pytest.raises(ValueError):
        rt.Context.reproject(None, object(), None, None, None, None, 4, 4, rr.IDENTITY[:2], params=rt.reproject_params(), channels=1)
