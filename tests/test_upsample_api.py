"""The guided upsample (rt_upsample_device, rt_upsample) without a device: the pins of the definition, header, binding and library agree, the
low size and the defaults are the header's, the argument rules hold, the numpy restatement (tests/upsample_ref.py) has the properties the
definition promises, the launcher's grid and tile are the denoiser's, the inputs of the GPU tests meet the conditions put on them, and on the
recorded experiment the guides bring half-resolution ambient occlusion closer to the full-resolution image than plain bilinear does.

rt_create needs a device, so with a context only the NULL-context rule can be called here; every other RT_ERR_INVALID / RT_ERR_UNSUPPORTED
rule is decided by rt_upsample_layout.hpp's up_args, which tools/upsample_layout_check.cpp covers under a sanitizer (run below)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ao_ref
import gbuffer_ref as gr
import scenes_gen
import upsample_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
CSRC = os.path.join(ROOT, "raytracer-in-cpp_amd", "csrc")
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
F = np.float32
INF = float("inf")
CALLS = {"rt_default_upsample_params": 1, "rt_upsample_low_size": 5, "rt_upsample_device": 11, "rt_upsample": 10}
DEFAULT_BITS = (2, 0x40000000, 0x3E000000, 0x3E800000)       # factor, sigma normal, depth, albedo
FACTORS = (2, 3, 4, 8)
SIZES = ((1, 1), (2, 1), (5, 3), (64, 4), (65, 5), (127, 9), (131, 7))        # (width, rows) of the high image
TIGHT = (0.1, 0.02, 0.05)                                    # sigma normal, depth, albedo: stops every tap whose guide differs at all
ALL_INF = (INF, INF, INF)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def covered_gbuffer(rows, w, depth=None):
    g = np.zeros((rows, w, 8), F)
    g[..., 0] = 1.0
    g[..., 1] = 1.0 if depth is None else np.asarray(depth, F).reshape(rows, w)
    g[..., 2:5] = (0.0, 0.0, 1.0)
    g[..., 5:8] = (0.5, 0.5, 0.5)
    return g


def synthetic(rows, width, ch, s, seed=28):
    """a seeded random low image and hand-made buffers of both sizes -> (low, g_low, g_high): random holes and a block of them, fractional
    alpha, a depth step with a gentle slope and a jitter of 0.25 at 12 % of the pixels, two normals with -0.0f components, three albedos.  The low
    buffers are the high ones at the pixels (sI, sJ), except for a seeded twentieth of them, which take the other jitter: so every guide stops
    some taps and passes others, and a high pixel that lies on a low pixel can miss too.  The seed is fixed at one for which the tight sigmas
    leave 8 % to 38 % of the covered pixels without a tap at every factor and size (test_the_tight_sigmas_... below asserts 1 % to 50 %)"""
    rng = np.random.default_rng(seed + 1000 * rows + 7 * width + s)
    w, r = ur.low_size(width, rows, s)
    low = rng.random((r, w, 3)).astype(F)                      # (three channels drawn whatever ch is: the buffers are the same for 1 and 3)
    alpha = np.ones((rows, width), F)
    alpha[rng.random((rows, width)) < 0.2] = 0.5
    x, y = np.arange(width, dtype=F)[None, :], np.arange(rows, dtype=F)[:, None]
    jitter = np.where(rng.random((rows, width)) < 0.12, F(0.25), F(0.0)).astype(F)
    z = (np.where(x * 2 < width, F(1.5), F(2.25)) + x * F(0.001953125) + y * F(0.00390625) + jitter).astype(F)
    N = np.zeros((rows, width, 3), F)
    N[..., 2] = 1.0
    N[..., 0] = -0.0
    N[:, 3 * width // 5:, :] = (0.6, -0.0, 0.8)                 # (every boundary is a column: an image of few rows has them too)
    A = np.zeros((rows, width, 3), F)
    A[...] = (0.75, 0.5, 0.25)
    A[:, width // 3:] = (0.5, 0.5, 0.625)
    A[:, 2 * width // 3 + 1:] = (0.25, 0.75, 0.5)
    g = np.empty((rows, width, 8), F)
    g[..., 0] = alpha
    g[..., 1] = (z * alpha).astype(F)
    g[..., 2:5] = (N * alpha[..., None]).astype(F)
    g[..., 5:8] = (A * alpha[..., None]).astype(F)
    holes = rng.random((rows, width)) < 0.1
    if rows >= 4 and width >= 20:
        holes[0:2, 8:17] = True
    g[holes] = 0.0
    gl = g[::s, ::s].copy()
    assert gl.shape == (r, w, 8)
    flip = (rng.random((r, w)) < 0.05) & (gl[..., 0] > 0)
    gl[flip, 1] = (gl[flip, 1] + F(0.25) * gl[flip, 0]).astype(F)
    return (low if ch == 3 else low[..., 0].copy()), gl, g


def miss_share(g_high, miss):
    """the share of the covered high pixels at miss = 1"""
    cov = g_high[..., 0] > 0
    return float(miss[cov].sum()) / float(cov.sum())


# ------------------------------------------------------------------------------------------ the pins
def test_the_pins_of_the_header():
    text = open(HEADER).read()
    assert "tests/upsample_ref.py" in text
    one = np.array([[1.0, 0.0]], F)
    a = ur.upsample(one, covered_gbuffer(1, 2), covered_gbuffer(1, 4), ur.Params(2))
    assert bits(a).tolist() == [[0x3F800000, 0x3F000000, 0, 0]] and "3F800000 3F000000 00000000 00000000" in text
    b = ur.upsample(one, covered_gbuffer(1, 2), covered_gbuffer(1, 5), ur.Params(3))
    assert bits(b).tolist() == [[0x3F800000, 0x3F2AAAAB, 0x3EAAAAAB, 0, 0]] and "3F800000 3F2AAAAB 3EAAAAAB 00000000 00000000" in text
    assert F(F(2) / F(3)) + F(F(1) / F(3)) == F(1.0)
    gl = covered_gbuffer(1, 2, [1.0, 1.5])
    c, mc = ur.upsample(one, gl, covered_gbuffer(1, 3, [1.0, 1.125, 1.5]), ur.Params(2, INF, 0.25, INF), True)
    assert bits(c).tolist() == [[0x3F800000, 0x3F52380F, 0]] and mc.tolist() == [[0, 0, 0]] and "3F800000 3F52380F 00000000" in text
    d, md = ur.upsample(one, gl, covered_gbuffer(1, 3, [1.0, 3.0, 1.5]), ur.Params(2, INF, 0.25, INF), True)
    assert bits(d).tolist() == [[0x3F800000, 0, 0]] and md.tolist() == [[0, 1, 0]]
    e = ur.upsample(np.array([[0.25], [0.75]], F), covered_gbuffer(2, 1), covered_gbuffer(3, 2), ur.Params(2))
    assert same(e, np.array([[0.25, 0.25], [0.5, 0.5], [0.75, 0.75]], F))


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
    assert sigs["rt_default_upsample_params"][1] is None and sigs["rt_upsample_low_size"][1] is C.c_int
    assert re.search(r"^\s*#\s*define\s+RT_UPSAMPLE_MAX_FACTOR\s+8\s*$", code, flags=re.M) and rt.capi.RT_UPSAMPLE_MAX_FACTOR == 8 == ur.MAX_FACTOR
    assert C.sizeof(rt.capi.rt_upsample_params) == 16
    names = ["factor", "sigma_normal", "sigma_depth", "sigma_albedo"]
    assert [f[0] for f in rt.capi.rt_upsample_params._fields_] == names
    m = re.search(r"typedef struct rt_upsample_params \{(.*?)\} rt_upsample_params;", code, flags=re.S)
    assert m and re.findall(r"\b(factor|sigma_\w+)\b", m.group(1)) == names


def test_front_ends_exist(rt):
    assert callable(rt.Context.upsample) and callable(rt.upsample_params) and callable(rt.low_camera)
    fs = rt.Flyscene()
    assert fs.upsample is None
    assert "upsample" in rt.Flyscene.ambient_occlusion.__code__.co_varnames
    hpp = open(os.path.join(CSRC, "flyscene.hpp")).read()
    assert "setUpsample(const rt_upsample_params *" in hpp and "bool upsample(" in hpp
    assert "--upsample" in open(os.path.join(CSRC, "rt_render_main.cpp")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^upsample_check:", mk, flags=re.M) and re.search(r"^SRC\s*:=.*\brt_upsample\.hip\b", mk, flags=re.M)
    for target in ("librt_mi355x.so", "librt_mi355x_work.so"):
        assert re.search(r"^\$\(OUT\)/%s:.*rt_upsample_layout\.hpp" % re.escape(target), mk, flags=re.M), target
    for other in ("rt_kernels.hip", "rt_denoise.hip"):
        assert "k_upsample" not in open(os.path.join(CSRC, other)).read(), "the operator is a translation unit of its own"
    unit = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "rt_upsample.hip")).read())          # (the code, not its comments)
    assert "k_upsample" in unit and "getenv" not in unit and "__shared__" not in unit and "atomic" not in unit
    assert "rt_kernels" not in open(os.path.join(CSRC, "rt_upsample_layout.hpp")).read() and "hip_runtime" not in open(os.path.join(CSRC, "rt_upsample_layout.hpp")).read()


def test_the_launch_takes_the_denoisers_tiles_and_grid():
    """the grid and tile constants of the launcher, pinned to the sources as tests/test_grid_stride_shapes.py pins the denoiser's"""
    unit, capi, lay = (open(os.path.join(CSRC, f)).read() for f in ("rt_upsample.hip", "rt_capi.cpp", "rt_upsample_layout.hpp"))
    assert "constexpr int kUpThreads = kDnTileH * 64;" in unit and "__global__ __launch_bounds__(kUpThreads) void k_upsample(" in unit
    assert "for (uint32_t tile = blockIdx.x; tile < T.tiles; tile += gridDim.x) {" in unit
    assert "const DnLane L = dn_lane(T, width, rows, tile, wave, lane);" in unit and "const uint64_t p = dn_pixel(width, L.x, L.y);" in unit
    assert "const DnTiles T = dn_tiles(width, rows);" in unit
    assert unit.count("<<<grid, kUpThreads, 0, st>>>") == 2
    assert "launch_upsample(dn_grid(dn_tiles(width, rows).tiles, c->cus), stream_or_own(c, stream), " in capi
    assert "constexpr int32_t kUpMaxFactor = 8;" in lay and '#include "rt_denoise_layout.hpp"' in lay


# ------------------------------------------------------------------------------------------ low size, defaults
def test_low_size_through_the_library(rt):
    lib = rt.load_library()
    w, r = C.c_int32(-7), C.c_int32(-7)
    for s in range(2, 9):
        for width, rows in ((1, 1), (s - 1, s), (s, s + 1), (s + 1, 1), (1920, 1080), (2 ** 31 - 1, 0), (5, 2 ** 31 - 1)):
            assert lib.rt_upsample_low_size(width, rows, s, C.byref(w), C.byref(r)) == rt.capi.RT_OK
            assert (w.value, r.value) == ur.low_size(width, rows, s) == (-(-width // s), -(-rows // s)), (width, rows, s)
    w.value = r.value = -7
    for bad in ((0, 4, 2), (-1, 4, 2), (4, -1, 2), (4, 4, 1), (4, 4, 9), (4, 4, 0), (4, 4, -2)):
        assert lib.rt_upsample_low_size(*bad, C.byref(w), C.byref(r)) == rt.capi.RT_ERR_INVALID and (w.value, r.value) == (-7, -7), bad
    assert lib.rt_upsample_low_size(4, 4, 2, None, C.byref(r)) == rt.capi.RT_ERR_INVALID
    assert lib.rt_upsample_low_size(4, 4, 2, C.byref(w), None) == rt.capi.RT_ERR_INVALID and (w.value, r.value) == (-7, -7)


def test_default_params_bits(rt):
    lib = rt.load_library()
    p = rt.capi.rt_upsample_params()
    lib.rt_default_upsample_params(C.byref(p))
    got = (p.factor,) + tuple(int(np.array([getattr(p, n)], F).view(np.uint32)[0]) for n in ("sigma_normal", "sigma_depth", "sigma_albedo"))
    assert got == DEFAULT_BITS
    text = open(HEADER).read()
    for b in DEFAULT_BITS[1:]:
        assert "(%08X)" % b in text
    d = rt.capi.rt_denoise_params()
    lib.rt_default_denoise_params(C.byref(d))
    assert (p.sigma_depth, p.sigma_albedo) == (d.sigma_depth, d.sigma_albedo), "the depth and albedo scales are the denoiser's"
    lib.rt_default_upsample_params(None)                 # tolerated
    q = rt.upsample_params(factor=4, sigma_depth=INF)
    assert (q.factor, q.sigma_normal, q.sigma_depth, q.sigma_albedo) == (4, 2.0, INF, 0.25)
    assert ur.Params(p.factor, p.sigma_normal, p.sigma_depth, p.sigma_albedo).valid()


def test_the_low_camera(rt):
    """viewport[2] and [3] divided by (float)s, everything else the high camera's; default_camera(w, r) in every bit where s divides both"""
    raw = lambda c: bytes(C.string_at(C.byref(c), C.sizeof(c)))
    for s, (width, rows) in ((2, (96, 64)), (4, (96, 64)), (8, (96, 64)), (3, (96, 63)), (2, (1920, 1080)), (4, (1920, 1080))):
        for yaw in (0.0, 0.4):
            cam = rt.default_camera(width, rows, yaw)
            low, w, r = rt.low_camera(cam, s)
            assert (w, r) == (width // s, rows // s)
            assert raw(low) == raw(rt.default_camera(w, r, yaw)), (s, width, rows, yaw)
    cam = rt.default_camera(97, 65, 0.4)
    low, w, r = rt.low_camera(cam, 2)
    assert (w, r) == (49, 33) and low.aspect == cam.aspect and list(low.center) == list(cam.center) and list(low.inv_view) == list(cam.inv_view)
    assert same(np.array(list(low.viewport), F), ur.low_viewport(list(cam.viewport), 2)) and list(low.viewport) == [0.0, 0.0, 48.5, 32.5]


# ------------------------------------------------------------------------------------------ argument rules
def test_a_null_context_is_refused_and_writes_nothing(rt):
    lib = rt.load_library()
    p = rt.upsample_params()
    low, gl, gh, out, miss = np.zeros(2, F), np.zeros(16, F), np.zeros(48, F), np.full(6, 7.0, F), np.full(6, 9, np.uint8)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.rt_upsample_device(None, ptr(low), 1, ptr(gl), ptr(gh), 3, 2, C.byref(p), ptr(out), ptr(miss), None) == rt.capi.RT_ERR_INVALID
    assert lib.rt_upsample(None, ptr(low), 1, ptr(gl), ptr(gh), 3, 2, C.byref(p), ptr(out), ptr(miss)) == rt.capi.RT_ERR_INVALID
    assert lib.rt_upsample_device(None, None, 0, None, None, 0, -1, None, None, None, None) == rt.capi.RT_ERR_INVALID
    assert lib.rt_upsample(None, None, 0, None, None, 0, -1, None, None, None) == rt.capi.RT_ERR_INVALID
    assert (out == 7.0).all() and (miss == 9).all()


def test_the_layout_check_program_holds_under_the_sanitizers(tmp_path):
    """every other argument rule, the low size, the taps, the nearest pixel and the scales: tools/upsample_layout_check.cpp, built and run as the
    Makefile does"""
    r = subprocess.run(["make", "-C", CSRC, "upsample_check", f"OUT={tmp_path}"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
    assert b"upsample_layout_check: all checks held" in r.stdout
    src = open(os.path.join(ROOT, "tools", "upsample_layout_check.cpp")).read()
    for rule in ("INT32_MAX", "out + k", "miss + k", "s - 1, s, s + 1", "the host form has no overlap rule"):
        assert rule in src


def test_params_validity_of_the_restatement():
    assert ur.Params(2).valid() and ur.Params(8, 1e-30, INF, 2.0).valid()
    for bad in (ur.Params(1), ur.Params(9), ur.Params(0), ur.Params(2, 0.0), ur.Params(2, 1.0, -1.0), ur.Params(2, 1.0, float("nan")), ur.Params(2, 1.0, 1.0, -INF)):
        assert not bad.valid()


# ------------------------------------------------------------------------------------------ properties of the restatement
@pytest.mark.parametrize("s", FACTORS)
def test_a_high_pixel_on_a_low_pixel_takes_it_bit_for_bit(s):
    """out[sJ, sI] == low[J, I] on random images whose low buffers are the high buffers at those pixels, whatever the sigmas: the one tap has
    weight 1.0f * 1.0f, or -- where a guide value is such that even equal values stop the tap -- the nearest low pixel is that pixel.  (The
    one value that does not come back is -0.0f: 0.0f + 1.0f * -0.0f is +0.0f, as the header says.)"""
    rng = np.random.default_rng(40 + s)
    for width, rows in ((5, 3), (65, 5), (37, 21)):
        for ch in (1, 3):
            low, _, gh = synthetic(rows, width, ch, s)
            gl = gh[::s, ::s].copy()
            low = (low * F(1000.0) - F(500.0)).astype(F)
            low.reshape(-1)[rng.integers(0, low.size, 3)] = (np.inf, -3.5, 1e-42)
            for sig in (ALL_INF, (2.0, 0.125, 0.25), TIGHT, (1e-30, 1e-30, 1e-30)):
                out, miss = ur.upsample(low, gl, gh, ur.Params(s, *sig), True)
                assert same(out[::s, ::s], low), (width, rows, ch, sig)
                if sig[0] != 1e-30:
                    assert not miss[::s, ::s].any()
                else:
                    assert np.array_equal(miss[::s, ::s] == 1, gh[::s, ::s, 0] > 0), "0 / 0 stops the tap of a covered pixel: the nearest pixel is the same one"
    one = np.array([[-0.0]], F)
    assert bits(ur.upsample(one, covered_gbuffer(1, 1), covered_gbuffer(1, 1), ur.Params(s))).tolist() == [[0]]


@pytest.mark.parametrize("s", FACTORS)
def test_a_constant_image_stays_constant_where_a_tap_is_left(s):
    """sum_c / sumw with sum_c = the sum of wt * v and sumw the sum of wt: not exact in general -- so what is asserted is what the definition
    gives, every bit, for values v whose products wt * v are exact multiples (v a power of two): v itself wherever miss == 0"""
    for width, rows in ((65, 5), (37, 21)):
        _, gl, gh = synthetic(rows, width, 3, s)
        w, r = ur.low_size(width, rows, s)
        for v in (0.5, -4.0, 0.0):
            low = np.full((r, w, 3), v, F)
            for sig in (ALL_INF, (2.0, 0.125, 0.25), TIGHT):
                out, miss = ur.upsample(low, gl, gh, ur.Params(s, *sig), True)
                assert same(out[miss == 0], np.full((int((miss == 0).sum()), 3), v, F)), (width, rows, v, sig)
                assert same(out[miss == 1], np.full((int((miss == 1).sum()), 3), v, F)), "the nearest pixel of a constant image is the constant too"


@pytest.mark.parametrize("s", FACTORS)
def test_every_sigma_infinite_on_a_covered_image_is_plain_bilinear(s):
    rng = np.random.default_rng(60 + s)
    for width, rows in ((1, 1), (2, 1), (5, 3), (65, 5), (23, 17)):
        w, r = ur.low_size(width, rows, s)
        for ch in (1, 3):
            low = rng.random((r, w, ch)).astype(F) if ch == 3 else rng.random((r, w)).astype(F)
            gl, gh = covered_gbuffer(r, w, rng.random((r, w)) + 1), covered_gbuffer(rows, width, rng.random((rows, width)) + 1)
            out, miss = ur.upsample(low, gl, gh, ur.Params(s), True)
            assert same(out, ur.bilinear(low, width, rows, s)) and not miss.any(), (width, rows, ch)


def test_background_and_surface_never_mix():
    rows, width, s = 9, 20, 2
    gh = covered_gbuffer(rows, width)
    gh[:, 10:] = 0.0
    gl = gh[::s, ::s].copy()
    low = np.zeros((5, 10), F)
    low[:, :5] = 0.25
    low[:, 5:] = 0.75
    out, miss = ur.upsample(low, gl, gh, ur.Params(s), True)
    assert same(out[:, :10], np.full((rows, 10), 0.25, F)) and same(out[:, 10:], np.full((rows, 10), 0.75, F)) and not miss.any()
    gl[:, 5:, 0] = 1.0                                   # the low frame saw a surface where the high frame sees none: those pixels miss
    out, miss = ur.upsample(low, gl, gh, ur.Params(s), True)
    assert miss[:, 10:].all() and not miss[:, :10].any() and same(out[:, 10:], np.full((rows, 10), 0.75, F))


# ------------------------------------------------------------------------------------------ the inputs of the GPU tests
def enough_pixels(size):
    """the sizes on which a share of the covered pixels means something: (1, 1), (2, 1) and (5, 3) hold at most 15 pixels, one of which is 7 %
    or more, and at s = 8 every pixel of theirs shares one low pixel"""
    return size[0] * size[1] >= 256


@pytest.mark.parametrize("s", FACTORS)
def test_the_tight_sigmas_leave_a_share_of_the_covered_pixels_without_a_tap(s):
    """between 1 % and 50 % of the covered pixels at miss = 1, in the restatement itself, on every size of the GPU test that holds enough
    pixels for a share to mean something; with every sigma +inf only the coverage rule is left and far fewer miss"""
    for size in SIZES:
        width, rows = size
        low, gl, gh = synthetic(rows, width, 1, s)
        _, miss = ur.upsample(low, gl, gh, ur.Params(s, *TIGHT), True)
        _, free = ur.upsample(low, gl, gh, ur.Params(s), True)
        if enough_pixels(size):
            share = miss_share(gh, miss)
            print(f"s {s} {width}x{rows}: tight {share:.3f}, every sigma +inf {miss_share(gh, free):.3f}")
            assert 0.01 <= share <= 0.5, (s, size, share)
            assert miss_share(gh, free) < share
            cov = gh[..., 0] > 0
            assert (gh[..., 0] == 0.5).any() and (~cov).any() and cov.any()


# ------------------------------------------------------------------------------------------ usefulness, measured once on the CPU
EXPERIMENT = dict(width=96, height=64, factor=2, yaw=0.4, radius=0.5, seed=0, grid=8, reach=2)
# RMS distance from the full-resolution image over the high pixels within two pixels of a change of face id, as recorded in DESIGN.md §5:
# plain bilinear (every sigma +inf), the denoiser's sigmas (0.5, 0.125, 0.25) and rt_default_upsample_params (2.0, 0.125, 0.25)
MEASURED = {"mixed": dict(pixels=790, bilinear=0.07788, inherited=0.04682, guided=0.04720),
            "dodge": dict(pixels=930, bilinear=0.04371, inherited=0.06054, guided=0.02544)}


def near_a_change_of_face(faces, reach):
    """the pixels within `reach` pixels (in x and in y) of a pixel whose face id differs from a 4-neighbour's"""
    h, w = faces.shape
    ch = np.zeros((h, w), bool)
    dx, dy = faces[:, 1:] != faces[:, :-1], faces[1:, :] != faces[:-1, :]
    ch[:, 1:] |= dx
    ch[:, :-1] |= dx
    ch[1:, :] |= dy
    ch[:-1, :] |= dy
    out = np.zeros((h, w), bool)
    ys, xs = np.nonzero(ch)
    for oy in range(-reach, reach + 1):
        for ox in range(-reach, reach + 1):
            out[np.clip(ys + oy, 0, h - 1), np.clip(xs + ox, 0, w - 1)] = True
    return out


@pytest.mark.parametrize("name", ["mixed", "dodge"])
def test_guided_occlusion_is_closer_to_full_resolution_than_bilinear(rt, oracle, tmp_path, name):
    """8 x 8 ambient occlusion at 96 x 64 and at 48 x 32, the low image upsampled by 2 with rt_default_upsample_params and with every sigma
    +inf.  Measured (mixed / dodgeColorTest): bilinear 0.07788 / 0.04371, guided 0.04720 / 0.02544; with the denoiser's normal scale 0.5
    instead of 2.0: 0.04682 / 0.06054 -- worse than bilinear on dodgeColorTest, which is why the default differs.  Asserted: the direction."""
    e = EXPERIMENT
    path = scenes_gen.mixed_materials(str(tmp_path)) if name == "mixed" else os.path.join(SCENES, "dodgeColorTest.obj")
    osc = oracle.load_scene(path)
    try:
        frames = {}
        for w, h in ((e["width"], e["height"]), ur.low_size(e["width"], e["height"], e["factor"])):
            (o, d, f, t), _ = ao_ref.camera_points(oracle, osc, w, h, e["yaw"])
            P, N = ao_ref.hit_points(o, d, f, t, osc.arrays()["face_normal"])
            ao = ao_ref.ao_of(ao_ref.counts(osc, P, N, e["seed"], e["grid"], e["radius"]), e["grid"]).reshape(h, w)
            frames[w] = (ao, gr.cpu_frame(oracle, osc, oracle.camera(w, h, e["yaw"]), w, h, 1, 0, 1), f.reshape(h, w))
    finally:
        osc.close()
    (full, gh, faces), (low, gl, low_faces) = frames[e["width"]], frames[e["width"] // e["factor"]]
    s = e["factor"]
    assert same(gl, gh[::s, ::s]) and np.array_equal(low_faces, faces[::s, ::s]), "low pixel (I, J) is high pixel (sI, sJ), ray for ray"
    edge = near_a_change_of_face(faces, e["reach"])
    rms = lambda a: float(np.sqrt(np.mean((a[edge].astype(np.float64) - full[edge]) ** 2)))
    p = rt.upsample_params()
    assert p.factor == s
    guided = ur.upsample(low, gl, gh, ur.Params(s, p.sigma_normal, p.sigma_depth, p.sigma_albedo))
    plain = ur.upsample(low, gl, gh, ur.Params(s))
    inherited = ur.upsample(low, gl, gh, ur.Params(s, 0.5, p.sigma_depth, p.sigma_albedo))
    print(f"{name}: {int(edge.sum())} pixels near a change of face; bilinear {rms(plain):.5f} guided {rms(guided):.5f} "
          f"(the denoiser's normal scale: {rms(inherited):.5f})")
    m = MEASURED[name]
    assert int(edge.sum()) == m["pixels"]
    assert rms(guided) < rms(plain)
    assert same(guided[::s, ::s], low)
