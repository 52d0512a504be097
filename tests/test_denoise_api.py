"""The denoiser (rt_denoise_device, rt_denoise) without a device: the pin of the definition, header, binding and library agree, the scratch
size is the layout's sum, the defaults are the header's bits, the argument rules hold, the numpy restatement (tests/denoise_ref.py) has the
properties the definition promises, and on the recorded experiment the filter brings 2 x 2-grid ambient occlusion closer to 16 x 16.

rt_create needs a device, so with a context only the NULL-context rule can be called here; every other RT_ERR_INVALID / RT_ERR_UNSUPPORTED
rule is decided by rt_denoise_layout.hpp's dn_args, which tools/denoise_layout_check.cpp covers under a sanitizer (run below)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ao_ref
import denoise_ref as dr
import gbuffer_ref as gr
import scenes_gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
CSRC = os.path.join(ROOT, "raytracer-in-cpp_amd", "csrc")
F = np.float32
INF = float("inf")
CALLS = {"rt_denoise_scratch_bytes": 3, "rt_denoise_device": 10, "rt_denoise": 8, "rt_default_denoise_params": 1}
DEFAULT_BITS = (5, 0x3F800000, 0x3F000000, 0x3E000000, 0x3E800000)      # iterations, sigma colour, normal, depth, albedo


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def covered_gbuffer(rows, w, depth=1.0, normal=(0.0, 0.0, 1.0), albedo=(0.5, 0.5, 0.5)):
    g = np.zeros((rows, w, 8), F)
    g[..., 0] = 1.0
    g[..., 1] = depth
    g[..., 2:5] = normal
    g[..., 5:8] = albedo
    return g


def layout_bytes(w, r, ch):
    """rt_denoise_layout.hpp's dn_layout: two float4 guide records per pixel, two working images, each part 16-byte aligned"""
    px = w * r
    work = (px * (16 if ch == 3 else 4) + 15) // 16 * 16
    return px * 32 + 2 * work


# ------------------------------------------------------------------------------------------ the pin
def test_the_pin_of_the_header():
    g = covered_gbuffer(1, 2)
    out = dr.denoise(np.array([[1.0, 0.0]], F), g, dr.Params(1))
    assert bits(out).tolist() == [[0x3F19999A, 0x3ECCCCCD]]
    assert same(out, np.array([[F(9 / 64) / F(15 / 64), F(3 / 32) / F(15 / 64)]], F))
    text = open(HEADER).read()
    assert "3F19999A, 3ECCCCCD" in text and "tests/denoise_ref.py" in text


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
    assert sigs["rt_denoise_scratch_bytes"][1] is C.c_size_t and sigs["rt_default_denoise_params"][1] is None
    assert re.search(r"^\s*#\s*define\s+RT_DENOISE_MAX_ITERATIONS\s+8\s*$", code, flags=re.M) and rt.capi.RT_DENOISE_MAX_ITERATIONS == 8
    assert C.sizeof(rt.capi.rt_denoise_params) == 20
    assert [f[0] for f in rt.capi.rt_denoise_params._fields_] == ["iterations", "sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"]
    m = re.search(r"typedef struct rt_denoise_params \{(.*?)\} rt_denoise_params;", code, flags=re.S)
    assert m and re.findall(r"\b(iterations|sigma_\w+)\b", m.group(1)) == ["iterations", "sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"]


def test_front_ends_exist(rt):
    assert callable(rt.Context.denoise) and callable(rt.denoise_params)
    fs = rt.Flyscene()
    assert fs.denoise is None
    assert "denoise" in rt.Flyscene.ambient_occlusion.__code__.co_varnames
    hpp = open(os.path.join(CSRC, "flyscene.hpp")).read()
    assert "setDenoise(const rt_denoise_params *" in hpp and "bool denoise(" in hpp
    assert "--denoise" in open(os.path.join(CSRC, "rt_render_main.cpp")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^denoise_check:", mk, flags=re.M) and re.search(r"^SRC\s*:=.*\brt_denoise\.hip\b", mk, flags=re.M)
    for target in ("librt_mi355x.so", "librt_mi355x_work.so"):
        assert re.search(r"^\$\(OUT\)/%s:.*rt_denoise_layout\.hpp" % re.escape(target), mk, flags=re.M), target
    assert "k_atrous" not in open(os.path.join(CSRC, "rt_kernels.hip")).read(), "the filter is a translation unit of its own"
    assert "getenv" not in open(os.path.join(CSRC, "rt_denoise.hip")).read()


# ------------------------------------------------------------------------------------------ scratch size, defaults
def test_scratch_bytes_is_the_layouts_sum(rt):
    lib = rt.load_library()
    for w, r in ((1, 1), (3, 2), (37, 21), (48, 32), (70, 5), (1920, 1080), (1, 2 ** 31 - 1), (2 ** 31 - 1, 1), (46341, 46340)):
        for ch in (1, 3):
            got = lib.rt_denoise_scratch_bytes(w, r, ch)
            assert got == layout_bytes(w, r, ch) and got % 16 == 0, (w, r, ch)
    assert lib.rt_denoise_scratch_bytes(1920, 1080, 3) == 1920 * 1080 * 64
    for bad in ((0, 4, 3), (-1, 4, 3), (4, -1, 3), (4, 4, 0), (4, 4, 2), (4, 4, 4), (2 ** 31 - 1, 2, 1), (46341, 46341, 3)):
        assert lib.rt_denoise_scratch_bytes(*bad) == 0, bad
    assert lib.rt_denoise_scratch_bytes(4, 0, 3) == 0


def test_default_params_bits(rt):
    lib = rt.load_library()
    p = rt.capi.rt_denoise_params()
    lib.rt_default_denoise_params(C.byref(p))
    got = (p.iterations,) + tuple(int(np.array([getattr(p, n)], F).view(np.uint32)[0]) for n in ("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"))
    assert got == DEFAULT_BITS
    text = open(HEADER).read()
    for b in DEFAULT_BITS[1:]:
        assert "(%08X)" % b in text
    lib.rt_default_denoise_params(None)                  # tolerated
    q = rt.denoise_params(iterations=3, sigma_depth=INF)
    assert (q.iterations, q.sigma_color, q.sigma_depth) == (3, 1.0, INF)
    assert dr.Params(*[p.iterations, p.sigma_color, p.sigma_normal, p.sigma_depth, p.sigma_albedo]).valid()


# ------------------------------------------------------------------------------------------ argument rules
def test_a_null_context_is_refused_and_writes_nothing(rt):
    lib = rt.load_library()
    p = rt.denoise_params()
    img, g, out = np.zeros(6, F), np.zeros(48, F), np.full(6, 7.0, F)
    scr = np.zeros(256 // 4, F)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.rt_denoise_device(None, ptr(img), 1, ptr(g), 3, 2, C.byref(p), ptr(scr), ptr(out), None) == rt.capi.RT_ERR_INVALID
    assert lib.rt_denoise(None, ptr(img), 1, ptr(g), 3, 2, C.byref(p), ptr(out)) == rt.capi.RT_ERR_INVALID
    assert lib.rt_denoise_device(None, None, 0, None, 0, -1, None, None, None, None) == rt.capi.RT_ERR_INVALID
    assert lib.rt_denoise(None, None, 0, None, 0, -1, None, None) == rt.capi.RT_ERR_INVALID
    assert (out == 7.0).all()


def test_the_layout_check_program_holds_under_the_sanitizers(tmp_path):
    """every other argument rule, the scratch layout, the tiles and the scales: tools/denoise_layout_check.cpp, built and run as the Makefile does"""
    r = subprocess.run(["make", "-C", CSRC, "denoise_check", f"OUT={tmp_path}"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
    assert b"denoise_layout_check: all checks held" in r.stdout
    src = open(os.path.join(ROOT, "tools", "denoise_layout_check.cpp")).read()
    for rule in ("INT32_MAX", "out + k", "scr + k", "the host form has no overlap rule"):
        assert rule in src


def test_params_validity_of_the_restatement():
    assert dr.Params(1).valid() and dr.Params(8, 1e-30, INF, 1.0, 2.0).valid()
    for bad in (dr.Params(0), dr.Params(9), dr.Params(5, 0.0), dr.Params(5, 1.0, -1.0), dr.Params(5, 1.0, 1.0, float("nan")), dr.Params(5, 1.0, 1.0, 1.0, -INF)):
        assert not bad.valid()


# ------------------------------------------------------------------------------------------ properties of the restatement
def test_uncovered_pixels_pass_through_bit_for_bit():
    rng = np.random.default_rng(5)
    rows, w = 9, 13
    img = rng.random((rows, w, 3)).astype(F)
    img[2, 3] = (np.nan, -0.0, np.inf)
    g = covered_gbuffer(rows, w)
    holes = rng.random((rows, w)) < 0.3
    holes[2, 3] = True
    g[holes] = 0.0
    g[4, 4] = (-1.0, 1.0, 0.0, 0.0, 1.0, 0.5, 0.5, 0.5)        # alpha < 0 is not covered either
    holes[4, 4] = True
    for p in (dr.Params(1), dr.Params(5, 1.0, 0.5, 0.125, 0.25)):
        out = dr.denoise(img, g, p)
        assert np.array_equal(bits(out)[holes], bits(img)[holes])
        assert not same(out[~holes], img[~holes]) and np.isfinite(out[~holes]).all(), "the covered pixels are filtered, from covered pixels only"


def test_a_pixel_alone_in_depth_comes_back_bit_for_bit():
    """sigma_depth tiny: all 24 neighbours differ in depth, only the centre tap is left and the pixel is (h * v) / h with h = 9/64.  That is v
    itself, bit for bit, whenever h * v is exact -- every value of at most 20 significant bits, as here.  (The definition rounds the
    product and the quotient: a value with a full 24-bit significand may come back one ulp off, 9.7 % of uniform random floats do; for
    those the result is still exactly the centre tap's own quotient, checked last.)"""
    rng = np.random.default_rng(6)
    rows, w = 7, 7
    img = (rng.integers(0, 1 << 20, (rows, w, 3)).astype(F) / F(1 << 20)).astype(F)
    g = covered_gbuffer(rows, w)
    g[..., 1] = (1.0 + np.arange(rows * w, dtype=F).reshape(rows, w) / 8).astype(F)          # 49 different depths
    for k_iter in (1, 3):
        out = dr.denoise(img, g, dr.Params(k_iter, INF, INF, 1e-3, INF))
        assert same(out, img)
    one = dr.denoise(img[..., 0], g, dr.Params(2, INF, INF, 1e-30, INF))                          # s2 underflows to 0: inf and NaN quotients
    assert same(one, img[..., 0])
    assert not same(dr.denoise(img, g, dr.Params(1, INF, INF, INF, INF)), img)
    full = rng.random((rows, w, 3)).astype(F)                                                      # full significands: the centre tap alone
    h = F(0.375) * F(0.375)
    out = dr.denoise(full, g, dr.Params(1, INF, INF, 1e-3, INF))
    assert same(out, ((h * full).astype(F) / h).astype(F))
    assert np.abs(bits(out).astype(np.int64) - bits(full).astype(np.int64)).max() <= 1


def test_two_sides_of_a_depth_step_never_mix():
    rows, w = 12, 20
    img = np.zeros((rows, w, 3), F)
    img[:, :9] = (0.25, 0.5, 0.75)
    img[:, 9:] = (0.75, 0.125, 0.0625)
    g = covered_gbuffer(rows, w)
    g[:, 9:, 1] = 3.0
    for it in (1, 5):
        out = dr.denoise(img, g, dr.Params(it, INF, INF, 0.01, INF))
        assert same(out, img), "a weighted mean of equal values is that value; nothing crosses the step"
    mixed = dr.denoise(img, g, dr.Params(1, INF, INF, INF, INF))
    assert not same(mixed[:, 7:11], img[:, 7:11])


# ------------------------------------------------------------------------------------------ usefulness, measured once on the CPU
EXPERIMENT = dict(width=64, height=40, yaw=0.4, radius=0.5, seed=0, coarse=2, fine=16)
MEASURED = dict(raw=0.11402, denoised=0.06690)          # RMS against the 16 x 16 grid over the covered pixels, as recorded in DESIGN.md §5


def test_denoised_coarse_occlusion_is_closer_to_the_fine_grid(rt, oracle, tmp_path):
    """2 x 2-grid ambient occlusion of the mixed-materials scene, raw and filtered with rt_default_denoise_params, against the 16 x 16 grid:
    measured raw 0.11402, denoised 0.06690 (ratio 0.587).  Asserted: the direction, on exactly that input."""
    e = EXPERIMENT
    osc = oracle.load_scene(scenes_gen.mixed_materials(str(tmp_path)))
    try:
        w, h = e["width"], e["height"]
        (o, d, f, t), _ = ao_ref.camera_points(oracle, osc, w, h, e["yaw"])
        P, N = ao_ref.hit_points(o, d, f, t, osc.arrays()["face_normal"])
        ao = lambda m: ao_ref.ao_of(ao_ref.counts(osc, P, N, e["seed"], m, e["radius"]), m).reshape(h, w)
        raw, fine = ao(e["coarse"]), ao(e["fine"])
        g = gr.cpu_frame(oracle, osc, oracle.camera(w, h, e["yaw"]), w, h, 1, 0, 1)
    finally:
        osc.close()
    p = rt.denoise_params()
    out = dr.denoise(raw, g, dr.Params(p.iterations, p.sigma_color, p.sigma_normal, p.sigma_depth, p.sigma_albedo))
    cov = g[..., 0] > 0
    assert np.array_equal(cov, (f >= 0).reshape(h, w)) and cov.sum() > 100
    rms = lambda a: float(np.sqrt(np.mean((a[cov].astype(np.float64) - fine[cov]) ** 2)))
    print(f"raw {rms(raw):.5f} denoised {rms(out):.5f} ratio {rms(out) / rms(raw):.3f} over {int(cov.sum())} covered pixels")
    assert rms(out) < rms(raw)
    assert same(out[~cov], raw[~cov])
