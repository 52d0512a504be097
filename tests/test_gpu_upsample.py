"""The guided upsample on a real MI355X: rt_upsample_device returns, bit for bit, what the "upsampling" section of include/rt_mi355x.h defines --
against tests/upsample_ref.py -- for synthetic images that take every branch at every factor and size, with and without the miss mask, for
images of more tiles than its grid holds (tests/grid_caps.py: blocks stride to a second round), for NaN, infinite and negative values in the
image and the buffers, and for real one-ray frames with their two sets of geometry buffers; it writes nothing outside its output and its
mask, leaves its inputs and the context as they were, refuses what it must, needs no scene, and every front end (host form,
Context.upsample, Flyscene.upsample, Flyscene.ambient_occlusion(upsample=), rt_render --upsample, the counting build) gives the same bits.
Every comparison is on the bit patterns.  No graph is captured anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import grid_caps as gc
import scenes_gen
import switch_table
import test_gpu_denoise as gd
import test_gpu_lens as gl
import test_upsample_api as ua
import upsample_ref as ur
from test_gpu_denoise import Guarded, PATTERN, bits, differing, same, same_but_nan_payloads

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")
WORK_LIB = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")
F = np.float32
INF = float("inf")
YAW = 0.4
DEFAULTS = (2.0, 0.125, 0.25)
SIGMA_SETS = (ua.ALL_INF, DEFAULTS, ua.TIGHT)
MISS_PATTERN = 0xA5


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def ref_params(p):
    return ur.Params(p.factor, p.sigma_normal, p.sigma_depth, p.sigma_albedo)


def device_call(rt, lib, handle, low, g_low, g_high, p, want_miss=True, stream=None, sync=None, nan_ok=False):
    """rt_upsample_device on guarded buffers -> (out in the high shape, miss or None); checks the guards, that every output float and mask byte
    was written and that the inputs are unchanged.  sync: a callable that waits for the call (default: hipDeviceSynchronize)"""
    rows, width = g_high.shape[:2]
    ch = 3 if low.ndim == 3 else 1
    d_low, d_gl, d_gh = Guarded(rt, low.nbytes, low), Guarded(rt, g_low.nbytes, g_low), Guarded(rt, g_high.nbytes, g_high)
    d_out = Guarded(rt, width * rows * ch * 4)
    d_miss = Guarded(rt, width * rows) if want_miss else None
    try:
        st = lib.rt_upsample_device(handle, d_low.ptr, ch, d_gl.ptr, d_gh.ptr, width, rows, C.byref(p), d_out.ptr, d_miss.ptr if want_miss else None, stream)
        rt.capi.check(lib, handle, st, "rt_upsample_device")
        (sync or rt.hipmem.synchronize)()
        assert d_out.guards_hold(), "bytes outside the output were written"
        assert d_low.untouched() and d_gl.untouched() and d_gh.untouched(), "an input was written"
        out = d_out.body()
        assert (out != PATTERN).all(), "floats of the output were left unwritten"
        miss = None
        if want_miss:
            assert d_miss.guards_hold(), "bytes outside the mask were written"
            raw = d_miss.body().view(np.uint8)
            miss = raw[:width * rows].reshape(rows, width).copy()
            assert (raw[width * rows:] == MISS_PATTERN).all(), "bytes behind the mask were written"
            assert np.isin(miss, (0, 1)).all(), "mask bytes were left unwritten"
        return out.view(F).reshape((rows, width, 3) if ch == 3 else (rows, width)), miss
    finally:
        for b in (d_low, d_gl, d_gh, d_out, d_miss):
            if b is not None:
                b.free()


@pytest.fixture(scope="module")
def bare(rt):
    """a context WITHOUT a scene: the operator needs none"""
    ctx = rt.Context(0)
    yield ctx
    ctx.close()


_REFS = {}


def reference(key, low, g_low, g_high, p):
    """the restatement's (out, miss), computed once per case and kept read-only"""
    if key not in _REFS:
        out, miss = ur.upsample(low, g_low, g_high, ref_params(p), True)
        out.setflags(write=False)
        miss.setflags(write=False)
        _REFS[key] = (out, miss)
    return _REFS[key]


# ------------------------------------------------------------------------------------------ 1. synthetic images: every factor, size, sigma set
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("size", ua.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("s", ua.FACTORS)
def test_synthetic_images_equal_the_restatement(rt, bare, s, size, ch):
    width, rows = size
    low, g_low, g_high = ua.synthetic(rows, width, ch, s)
    for k, sig in enumerate(SIGMA_SETS):
        p = rt.upsample_params(s, *sig)
        want, want_miss = reference(("syn", s, size, ch, k), low, g_low, g_high, p)
        if sig == ua.TIGHT and ua.enough_pixels(size):
            assert 0.01 <= ua.miss_share(g_high, want_miss) <= 0.5, "the tight set must leave a share of the covered pixels without a tap"
        got, miss = device_call(rt, bare.lib, bare.handle, low, g_low, g_high, p)
        assert same(got, want), (sig, differing(got, want))
        assert np.array_equal(miss, want_miss), (sig, int((miss != want_miss).sum()))
        bare_out, none = device_call(rt, bare.lib, bare.handle, low, g_low, g_high, p, want_miss=False)
        assert none is None and same(bare_out, want), "without d_miss the image is the same"
    if ua.enough_pixels(size):
        outs = [reference(("syn", s, size, ch, k), low, g_low, g_high, None)[0] for k in range(3)]
        assert not same(outs[0], outs[1]) and not same(outs[1], outs[2]), "the three sigma sets give three images"


def test_the_pins_on_the_device(rt, bare):
    one = np.array([[1.0, 0.0]], F)
    cg = ua.covered_gbuffer
    call = lambda low, a, b, p: device_call(rt, bare.lib, bare.handle, low, a, b, p)
    out, miss = call(one, cg(1, 2), cg(1, 4), rt.upsample_params(2, INF, INF, INF))
    assert bits(out).tolist() == [[0x3F800000, 0x3F000000, 0, 0]] and not miss.any()
    out, miss = call(one, cg(1, 2), cg(1, 5), rt.upsample_params(3, INF, INF, INF))
    assert bits(out).tolist() == [[0x3F800000, 0x3F2AAAAB, 0x3EAAAAAB, 0, 0]] and not miss.any()
    low_g = cg(1, 2, [1.0, 1.5])
    out, miss = call(one, low_g, cg(1, 3, [1.0, 1.125, 1.5]), rt.upsample_params(2, INF, 0.25, INF))
    assert bits(out).tolist() == [[0x3F800000, 0x3F52380F, 0]] and miss.tolist() == [[0, 0, 0]]
    out, miss = call(one, low_g, cg(1, 3, [1.0, 3.0, 1.5]), rt.upsample_params(2, INF, 0.25, INF))
    assert bits(out).tolist() == [[0x3F800000, 0, 0]] and miss.tolist() == [[0, 1, 0]]
    out, miss = call(np.array([[0.25], [0.75]], F), cg(2, 1), cg(3, 2), rt.upsample_params(2, INF, INF, INF))
    assert same(out, np.array([[0.25, 0.25], [0.5, 0.5], [0.75, 0.75]], F)) and not miss.any()


# ------------------------------------------------------------------------------------------ 2. refusals on the device, no scene
def test_refusals_write_nothing_and_name_the_call(rt, bare):
    lib, h_ = bare.lib, bare.handle
    inv = rt.capi.RT_ERR_INVALID
    width, rows, ch, s = 37, 21, 3, 2
    low, g_low, g_high = ua.synthetic(rows, width, ch, s)
    p = rt.upsample_params(s)
    d_low, d_gl, d_gh = Guarded(rt, low.nbytes, low), Guarded(rt, g_low.nbytes, g_low), Guarded(rt, g_high.nbytes, g_high)
    d_out, d_miss = Guarded(rt, width * rows * ch * 4), Guarded(rt, width * rows)
    host_out, host_miss = np.full((rows, width, ch), 7.0, F), np.full((rows, width), 9, np.uint8)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    at = lambda b, off=0: C.c_void_p(b.address + off)

    def dev(low_=d_low.ptr, ch_=ch, gl_=d_gl.ptr, gh_=d_gh.ptr, w_=width, r_=rows, p_=p, out=d_out.ptr, miss=d_miss.ptr):
        return lib.rt_upsample_device(h_, low_, ch_, gl_, gh_, w_, r_, C.byref(p_) if p_ is not None else None, out, miss, None)

    def host(low_=vp(low), ch_=ch, gl_=vp(g_low), gh_=vp(g_high), w_=width, r_=rows, p_=p, out=vp(host_out), miss=vp(host_miss)):
        return lib.rt_upsample(h_, low_, ch_, gl_, gh_, w_, r_, C.byref(p_) if p_ is not None else None, out, miss)

    def named(what=b"rt_upsample"):
        return what in lib.rt_last_error(h_)

    # 1-10: NULL pointers, channels, width, rows
    for kw in (dict(low_=None), dict(gl_=None), dict(gh_=None), dict(p_=None), dict(out=None), dict(ch_=2), dict(ch_=0), dict(ch_=4), dict(w_=0), dict(w_=-3),
               dict(r_=-1)):
        assert dev(**kw) == inv and named(b"rt_upsample_device"), kw
        assert host(**kw) == inv and named(), kw
    # 11-12: the factor and the sigmas out of range
    for bad in (rt.upsample_params(1), rt.upsample_params(9), rt.upsample_params(0), rt.upsample_params(-2), rt.upsample_params(2, 0.0),
                rt.upsample_params(2, 1.0, -1.0), rt.upsample_params(2, 1.0, float("nan")), rt.upsample_params(2, 1.0, 1.0, -INF)):
        assert dev(p_=bad) == inv and named(b"rt_upsample_device") and host(p_=bad) == inv and named()
    # 13: too many pixels
    assert dev(w_=2 ** 31 - 1, r_=2) == rt.capi.RT_ERR_UNSUPPORTED and named(b"rt_upsample_device")
    assert host(w_=46341, r_=46341) == rt.capi.RT_ERR_UNSUPPORTED and named()
    # 14-16: an output or a geometry buffer that is not 16-byte aligned (the device call only)
    for off in (4, 8, 12):
        assert dev(out=at(d_out, off)) == inv and named(b"aligned")
        assert dev(gl_=at(d_gl, off)) == inv and named(b"aligned")
        assert dev(gh_=at(d_gh, off)) == inv and named(b"aligned")
    # 17-23: each overlap pair: out / miss, out / low, out / low buffers, out / high buffers, miss / low, miss / low buffers, miss / high buffers
    assert dev(miss=at(d_out, width * rows * ch * 4 - 1)) == inv and named(b"overlaps")
    assert dev(out=d_low.ptr) == inv and named(b"overlaps")
    assert dev(low_=at(d_out, 16)) == inv and named(b"overlaps")
    assert dev(out=d_gl.ptr) == inv and named(b"overlaps")
    assert dev(out=at(d_gh, (g_high.nbytes - 1) // 16 * 16)) == inv and named(b"overlaps")
    assert dev(miss=at(d_low, low.nbytes - 1)) == inv and named(b"overlaps")
    assert dev(miss=d_gl.ptr) == inv and named(b"overlaps")
    assert dev(miss=at(d_gh, g_high.nbytes - 1)) == inv and named(b"overlaps")
    # rows == 0: RT_OK, nothing enqueued
    assert dev(r_=0) == rt.capi.RT_OK and host(r_=0) == rt.capi.RT_OK
    rt.hipmem.synchronize()
    for b in (d_low, d_gl, d_gh, d_out, d_miss):
        assert b.untouched()
    assert (host_out == 7.0).all() and (host_miss == 9).all()
    # and the valid calls between the same guards, on a context that never saw a scene
    want, want_miss = reference(("refusals",), low, g_low, g_high, p)
    assert dev() == rt.capi.RT_OK
    rt.hipmem.synchronize()
    assert d_out.guards_hold() and d_miss.guards_hold() and d_low.untouched() and d_gl.untouched() and d_gh.untouched()
    assert same(d_out.body().view(F).reshape(want.shape), want)
    assert np.array_equal(d_miss.body().view(np.uint8)[:width * rows].reshape(rows, width), want_miss)
    assert host() == rt.capi.RT_OK
    assert same(host_out, want) and np.array_equal(host_miss, want_miss)
    host_out[...] = 7.0
    assert host(miss=None) == rt.capi.RT_OK and same(host_out, want), "the host form without a mask"
    for b in (d_low, d_gl, d_gh, d_out, d_miss):
        b.free()


# ------------------------------------------------------------------------------------------ 3. non-finite inputs
def poisoned(rows, width, ch, s, seed=5):
    """synthetic() with a seeded ~8 % of the low pixels NaN / +inf / -inf / negative, ~5 % of the alphas of both buffers NaN / -1 / +inf /
    -0.0 and one of g[1..7] NaN at a further ~4 % of their pixels"""
    low, g_low, g_high = ua.synthetic(rows, width, ch, s)
    low, g_low, g_high = low.copy(), g_low.copy(), g_high.copy()
    rng = np.random.default_rng(seed + rows + width + s)
    ys, xs = np.nonzero(rng.random(low.shape[:2]) < 0.08)
    value = np.array([np.nan, np.inf, -np.inf, -2.5], F)[np.arange(len(ys)) % 4]
    if ch == 3:
        low[ys, xs, rng.integers(0, 3, len(ys))] = value
    else:
        low[ys, xs] = value
    for g in (g_low, g_high):
        bad_alpha = rng.random(g.shape[:2]) < 0.05
        bad_g = (rng.random(g.shape[:2]) < 0.04) & ~bad_alpha
        ys, xs = np.nonzero(bad_alpha)
        g[ys, xs, 0] = np.array([np.nan, -1.0, np.inf, -0.0], F)[np.arange(len(ys)) % 4]
        ys, xs = np.nonzero(bad_g)
        g[ys, xs, rng.integers(1, 8, len(ys))] = np.nan
    return low, g_low, g_high


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("s", [2, 3])
def test_non_finite_inputs_follow_the_definition(rt, bare, s, ch):
    """NaN and infinities in the low image, NaN / negative / infinite / -0.0f alphas and NaN guide values are inputs the definition covers: a
    pixel is covered exactly when a > 0.0f, a tap whose u is not > 0.0f is stopped"""
    width, rows = 67, 21
    low, g_low, g_high = poisoned(rows, width, ch, s)
    assert np.isnan(low).any() and np.isinf(low).any() and (low < 0).any()
    for g in (g_low, g_high):
        assert np.isnan(g[..., 0]).any() and (g[..., 0] < 0).any() and np.isinf(g[..., 0]).any() and np.isnan(g[..., 1:]).any()
    for k, sig in enumerate(SIGMA_SETS):
        p = rt.upsample_params(s, *sig)
        want, want_miss = reference(("poison", s, ch, k), low, g_low, g_high, p)
        got, miss = device_call(rt, bare.lib, bare.handle, low, g_low, g_high, p)
        assert same_but_nan_payloads(got, want), sig
        assert np.array_equal(miss, want_miss), sig
    assert want_miss.any() and not want_miss.all()


# ------------------------------------------------------------------------------------------ 4. strided rounds
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("which", ["column", "frame"])
def test_strided_tiles(rt, bare, which, ch):
    """k_upsample beyond its grid: a pixel column of more tiles than one round holds, and a frame of several tile columns whose second round
    starts in the middle of a tile row (the shapes of the denoiser's strided tests), s = 2"""
    cus = gc.cu_count(bare.device)
    width, rows = gc.atrous_column(cus) if which == "column" else gc.denoise_frame(cus)
    tiles = gc.dn_tiles(width, rows)[2]
    assert gc.strides(tiles, gc.dn_cap(cus)) and gc.dn_grid(tiles, cus) < tiles, (cus, width, rows)
    low, g_low, g_high = ua.synthetic(rows, width, ch, 2)
    p = rt.upsample_params(2, *DEFAULTS)
    want, want_miss = reference(("strided", which, ch), low, g_low, g_high, p)
    got, miss = device_call(rt, bare.lib, bare.handle, low, g_low, g_high, p)
    assert same(got, want), differing(got, want)
    assert np.array_equal(miss, want_miss)


# ------------------------------------------------------------------------------------------ 5. real frames
@pytest.fixture(scope="module")
def world(rt, scenes, tmp_path_factory):
    paths = {"cube": os.path.join(scenes, "cube.obj"), "mixed": scenes_gen.mixed_materials(str(tmp_path_factory.mktemp("mixed")))}
    w = {k: gd.Scene(rt, p) for k, p in paths.items()}
    yield w
    for s in w.values():
        s.close()


def gbuffer_of(sc, cam, w, h):
    buf = sc.rt.hipmem.DeviceBuffer(w * h * 8 * 4)
    try:
        sc.ctx.gbuffer(cam, w, h, out=buf)
        sc.ctx.synchronize()
        return buf.to_numpy(F, (h, w, 8))
    finally:
        buf.free()


@pytest.mark.parametrize("name", ["cube", "mixed"])
def test_real_frames_equal_the_restatement_and_keep_the_low_pixels(world, name):
    """a 48 x 32 one-ray pinhole frame upsampled to 96 x 64 with its two rt_gbuffer_device buffers: the restatement's bits; with the defaults
    the pixels (2I, 2J) are the low frame's; and the low frame is high[::2, ::2] of the 96 x 64 render -- the camera claim"""
    sc = world[name]
    rt = sc.rt
    W, H, s = 96, 64, 2
    sc.settings()
    cam = rt.default_camera(W, H, YAW)
    lcam, w, h = rt.low_camera(cam, s)
    assert (w, h) == (48, 32)
    L = gl.area_lights(rt, 5)
    low, _ = gl.render_device(rt, sc.ctx, lcam, L, w, h, 2)
    high, _ = gl.render_device(rt, sc.ctx, cam, L, W, H, 2)
    g_low, g_high = gbuffer_of(sc, lcam, w, h), gbuffer_of(sc, cam, W, H)
    assert same(low, high[::s, ::s]), "low pixel (I, J) is high pixel (2I, 2J), ray for ray"
    assert same(g_low, g_high[::s, ::s])
    assert (g_high[..., 0] == 1.0).any() and (g_high[..., 0] == 0.0).any()
    for k, sig in enumerate((DEFAULTS, ua.ALL_INF, ua.TIGHT)):
        p = rt.upsample_params(s, *sig)
        want, want_miss = reference(("real", name, k), low, g_low, g_high, p)
        got, miss = device_call(rt, sc.lib, sc.ctx.handle, low, g_low, g_high, p)
        print(f"{name} sigmas {sig}: {differing(got, want)} floats differ, {int(want_miss.sum())} pixels miss")
        assert same(got, want) and np.array_equal(miss, want_miss), sig
        if sig == DEFAULTS:
            assert same(got[::s, ::s], low) and not miss[::s, ::s].any()
            assert same(rt.upsample_params().sigma_normal, DEFAULTS[0])


def frame(sc, w, h, n=1, tau=-1.0, depth=3):
    return gd.frame(sc, w, h, n, tau, depth)


def test_refined_count_pass_map_and_later_frames_survive_a_call(world):
    sc = world["cube"]
    rt = sc.rt
    w, h = 64, 40
    low, g_low, g_high = ua.synthetic(h, w, 3, 2)
    p = rt.upsample_params()
    want, want_miss = reference(("ctx",), low, g_low, g_high, p)
    before = frame(sc, w, h)
    adaptive = frame(sc, w, h, 2, 0.05)
    refined = sc.ctx.supersampling_refined()
    assert 0 < refined < w * h
    got, miss = device_call(rt, sc.lib, sc.ctx.handle, low, g_low, g_high, p, sync=sc.ctx.synchronize)
    assert same(got, want) and np.array_equal(miss, want_miss)
    assert sc.ctx.supersampling_refined() == refined
    again = frame(sc, w, h, 2, 0.05)
    assert same(again[0], adaptive[0]) and again[1:] == adaptive[1:]
    after = frame(sc, w, h)
    assert same(after[0], before[0]) and after[1:] == before[1:]
    # an adaptive-pass frame's map
    sc.settings(1, (0, 12))
    sc.ctx.set_pass_tolerance(0.01, 4)
    cam, L = rt.default_camera(w, h, YAW), gl.area_lights(rt, 5)
    rgb, _, _ = gl.render(rt, sc.ctx, cam, L, w, h, 2)
    pm = sc.ctx.pass_map(w, h)
    assert same(device_call(rt, sc.lib, sc.ctx.handle, low, g_low, g_high, p)[0], want)
    assert np.array_equal(sc.ctx.pass_map(w, h), pm)
    rgb2, _, _ = gl.render(rt, sc.ctx, cam, L, w, h, 2)
    assert same(rgb2, rgb)
    sc.settings()


def test_a_call_on_a_second_stream_beside_a_frame(rt, world):
    sc = world["mixed"]
    hip = rt.hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    w, h = 96, 64
    try:
        sc.settings(2, (1, 2), gd.LENS)
        cam, L = rt.default_camera(w, h, YAW), gl.area_lights(rt, 5)
        prm = rt.make_params(w, h, 3)
        solo_rgb, _ = gl.render_device(rt, sc.ctx, cam, L, w, h, 3)
        low, g_low, g_high = ua.synthetic(h, w, 3, 2)
        up = rt.upsample_params()
        want, want_miss = reference(("stream",), low, g_low, g_high, up)
        rgb = Guarded(rt, w * h * 12)
        rt.capi.check(sc.lib, sc.ctx.handle, sc.lib.rt_render_device(sc.ctx.handle, C.byref(cam), C.byref(L), C.byref(prm), rgb.ptr, None, None, None, None),
                      "rt_render_device")

        def wait():
            assert hip.hipStreamSynchronize(stream) == 0

        beside, miss = device_call(rt, sc.lib, sc.ctx.handle, low, g_low, g_high, up, stream=stream, sync=wait)
        sc.ctx.synchronize()
        assert same(beside, want) and np.array_equal(miss, want_miss)
        assert rgb.guards_hold() and same(rgb.body().view(F).reshape(h, w, 3), solo_rgb)
        rgb.free()
    finally:
        hip.hipStreamDestroy(stream)
        sc.settings()


# ------------------------------------------------------------------------------------------ 6. front ends
def test_context_upsample_on_tensors_and_device_buffers(rt, bare):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no device"
    width, rows, s = 37, 21, 3
    dev = f"cuda:{bare.device}"
    for ch in (1, 3):
        low, g_low, g_high = ua.synthetic(rows, width, ch, s)
        p = rt.upsample_params(s, *DEFAULTS)
        want, want_miss = reference(("front", ch), low, g_low, g_high, p)
        shape = want.shape
        t_low, t_gl, t_gh = (torch.from_numpy(a).to(dev) for a in (low, g_low, g_high))
        out = bare.upsample(t_low, t_gl, t_gh, width, rows, p)                        # torch's current (default) stream
        assert out.dtype == torch.float32 and tuple(out.shape) == shape and str(out.device) == dev
        assert same(out.cpu().numpy(), want)
        out, miss = bare.upsample(t_low, t_gl, t_gh, width, rows, p, miss=True)
        assert miss.dtype == torch.uint8 and tuple(miss.shape) == (rows, width)
        assert same(out.cpu().numpy(), want) and np.array_equal(miss.cpu().numpy(), want_miss)
        st = torch.cuda.Stream(device=dev)
        guard = gd.GUARD
        canary = torch.full((want.size + 2 * guard,), 3.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            view = canary[guard:guard + want.size]
            back = bare.upsample(t_low, t_gl, t_gh, width, rows, p, out=view)
        st.synchronize()
        assert back is view and same(view.cpu().numpy().reshape(shape), want)
        assert (canary[:guard] == 3.0).all() and (canary[-guard:] == 3.0).all()
        assert same(t_low.cpu().numpy(), low) and same(t_gl.cpu().numpy(), g_low) and same(t_gh.cpu().numpy(), g_high)
        b_low, b_gl, b_gh = (rt.hipmem.DeviceBuffer(a.nbytes).from_numpy(a) for a in (low, g_low, g_high))
        b_out, b_miss = rt.hipmem.DeviceBuffer(want.nbytes), rt.hipmem.DeviceBuffer(max(16, width * rows))
        res = bare.upsample(b_low, b_gl, b_gh, width, rows, p, out=b_out, miss=b_miss)          # channels from the buffer's size
        assert res[0] is b_out and res[1] is b_miss
        bare.synchronize()
        assert same(b_out.to_numpy(F, shape), want) and np.array_equal(b_miss.to_numpy(np.uint8, (rows, width)), want_miss)
        fresh = bare.upsample(b_low, b_gl, b_gh, width, rows, p, channels=ch)
        bare.synchronize()
        assert same(fresh.to_numpy(F, shape), want)
        with pytest.raises(ValueError):
            bare.upsample(t_low, t_gl[:-1], t_gh, width, rows, p)
        with pytest.raises(ValueError):
            bare.upsample(t_low.double(), t_gl, t_gh, width, rows, p)
        with pytest.raises(ValueError):
            bare.upsample(b_low, b_gl, b_gh, width, rows, p, out=rt.hipmem.DeviceBuffer(16))
        with pytest.raises(ValueError):
            bare.upsample(t_low, t_gl, t_gh, width, rows, p, miss=b_miss)
        with pytest.raises(ValueError):
            bare.upsample(t_low, t_gl, t_gh, width, rows, rt.upsample_params(9))
        for b in (b_low, b_gl, b_gh, b_out, b_miss, fresh):
            b.free()
    low, g_low, g_high = ua.synthetic(20, 38, 3, 2)
    got = bare.upsample(*(torch.from_numpy(a).to(dev) for a in (low, g_low, g_high)), 38, 20)
    assert same(got.cpu().numpy(), reference(("front", "default"), low, g_low, g_high, rt.upsample_params())[0])


def test_flyscene_occlusion_through_the_low_camera(rt, world):
    W, H, s = 96, 64, 2
    w, h = 48, 32
    fs = rt.Flyscene(scene_path=world["mixed"].path)
    fs.initialize(W, H, True, False)
    try:
        fs.camera = rt.default_camera(W, H, YAW)
        full = fs.ambient_occlusion(W, H, 2, 0.5, seed=3)
        fs.supersample, fs.passes = 1, 1
        g_high = fs.gbuffer(W, H)
        fs.camera = rt.default_camera(w, h, YAW)            # the same pipeline by hand: the low camera is the default camera of 48 x 32
        fs.width, fs.height = w, h
        low = fs.ambient_occlusion(w, h, 2, 0.5, seed=3)
        g_low = fs.gbuffer(w, h)
        fs.camera = rt.default_camera(W, H, YAW)
        fs.width, fs.height = W, H
        up = rt.upsample_params(s)
        fs.ctx.set_supersampling(3)                          # the call sets the one-ray pinhole frame itself
        got = fs.ambient_occlusion(W, H, 2, 0.5, seed=3, upsample=up)
        assert got.shape == full.shape and same(got, ur.upsample(low, g_low, g_high, ref_params(up)))
        assert same(got[::s, ::s], low) and not same(got, full)
        dp = rt.denoise_params(2)
        got = fs.ambient_occlusion(W, H, 2, 0.5, seed=3, denoise=dp, upsample=up)
        filtered = dr.denoise(low, g_low, gd.ref_params(dp))
        assert same(got, ur.upsample(filtered, g_low, g_high, ref_params(up))), "denoise= runs at low resolution on the low buffers"
        assert same(fs.ambient_occlusion(W, H, 2, 0.5, seed=3), full), "upsample=None is today's image"
    finally:
        fs.ctx.close()
        fs.scene.close()


def test_flyscene_member_and_the_cli(rt, scenes, tmp_path):
    W, H, s = 72, 40, 2
    w, h = 36, 20
    path = os.path.join(scenes, "dodgeColorTest.obj")
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(W, H, True, False)
    try:
        fs.usteps = fs.vsteps = 2
        fs.max_depth, fs.supersample, fs.passes = 1, 2, 2
        fs.output_path = str(tmp_path / "python.ppm")
        assert fs.upsample is None
        plain = fs.raytraceScene(W, H, write_ppm=False).copy()
        g_high = fs.gbuffer(W, H)
        low = fs.raytraceScene(w, h, write_ppm=False).copy()                        # by hand: the low camera is the default camera of 36 x 20
        g_low = fs.gbuffer(w, h)
        fs.upsample = rt.upsample_params(s)
        got = fs.raytraceScene(W, H, write_ppm=True)
        assert got.shape == plain.shape and same(got, ur.upsample(low, g_low, g_high, ref_params(fs.upsample))) and not same(got, plain)
        with pytest.raises(ValueError):
            fs.raytraceScene(W, H, write_ppm=False, want_hits=True)
        fs.denoise = rt.denoise_params(2)
        both = fs.raytraceScene(W, H, write_ppm=False)
        assert same(both, ur.upsample(dr.denoise(low, g_low, gd.ref_params(fs.denoise)), g_low, g_high, ref_params(fs.upsample)))
        fs.denoise = fs.upsample = None
        assert same(fs.raytraceScene(W, H, write_ppm=False), plain), "unset is today's frame"
    finally:
        fs.ctx.close()
        fs.scene.close()
    cli = ["--scene", path, "--size", str(W), str(H), "--samples", "2", "2", "--depth", "1", "--aa", "2", "--passes", "2"]
    r = subprocess.run([RT_RENDER] + cli + ["--upsample", str(s), "--out", "result.ppm"], input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=240)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(str(tmp_path / "result.ppm"), "rb").read() == open(str(tmp_path / "python.ppm"), "rb").read()
    r = subprocess.run([RT_RENDER] + cli + ["--upsample", str(s), "2.0", "0.125", "0.25", "--out", "sigmas.ppm"], input=b"1\n0\n", capture_output=True,
                       cwd=str(tmp_path), timeout=240)
    assert r.returncode == 0 and open(str(tmp_path / "sigmas.ppm"), "rb").read() == open(str(tmp_path / "python.ppm"), "rb").read()
    r = subprocess.run([RT_RENDER] + cli + ["--out", "plain.ppm"], input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=240)
    assert r.returncode == 0 and open(str(tmp_path / "plain.ppm"), "rb").read() != open(str(tmp_path / "result.ppm"), "rb").read()
    for bad in (["--upsample", "1"], ["--upsample", "9"], ["--upsample", "2", "0.5"], ["--upsample", "2", "0.5", "-1", "1"],
                ["--pass-tolerance", "0.01", "--upsample", "2"]):
        r = subprocess.run([RT_RENDER] + cli + bad, input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=240)
        assert r.returncode == 2 and (b"--upsample" in r.stderr), bad


def test_counting_build_gives_the_same_bits(rt):
    lib = rt.capi.load_library(WORK_LIB)
    ctx = C.c_void_p()
    assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
    try:
        for ch in (1, 3):
            low, g_low, g_high = ua.synthetic(21, 37, ch, 3)
            p = rt.upsample_params(3, *DEFAULTS)
            want, want_miss = reference(("front", ch), low, g_low, g_high, p)
            got, miss = device_call(rt, lib, ctx, low, g_low, g_high, p)
            assert same(got, want) and np.array_equal(miss, want_miss)
            out, m = np.zeros(want.shape, F), np.zeros((21, 37), np.uint8)
            vp = lambda a: C.c_void_p(a.ctypes.data)
            rt.capi.check(lib, ctx, lib.rt_upsample(ctx, vp(low), ch, vp(g_low), vp(g_high), 37, 21, C.byref(p), vp(out), vp(m)), "rt_upsample")
            assert same(out, want) and np.array_equal(m, want_miss)
    finally:
        lib.rt_destroy(ctx)
