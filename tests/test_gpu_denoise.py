"""The denoiser on a real MI355X: rt_denoise_device returns, bit for bit, what the "denoising" section of include/rt_mi355x.h defines -- against
tests/denoise_ref.py -- for synthetic images that take every branch, for images of more tiles and pixels than its grids hold (tests/grid_caps.py:
blocks stride to a second round), for images wider and higher than the reach of the eighth iteration (far taps inside the image), for NaN,
infinite and negative values in the image and the buffers, and for real frames, buffers and occlusion images; it writes nothing
outside its output and its scratch, leaves its inputs and the context as they were, refuses what it must, needs no scene, and every front
end (host form, Context.denoise, Flyscene.denoise, Flyscene.ambient_occlusion(denoise=), rt_render --denoise, the counting build) gives the
same bits.  Every comparison is on the bit patterns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import grid_caps as gc
import scenes_gen
import switch_table
import test_gpu_lens as gl
import test_gpu_passes as gp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")
WORK_LIB = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")
F = np.float32
INF = float("inf")
YAW = 0.4
SIZES = ((1, 1), (3, 2), (37, 21), (48, 32), (70, 5))     # one pixel; smaller than every halo; not a multiple / a multiple of the 64 x 4 tile; wider than a wave's run
GUARD = 64                                   # floats in front of and behind the output and the scratch, holding PATTERN
PATTERN = 0xA5A5A5A5
FINITE = (0.6, 0.6, 0.3, 0.4)                # sigma colour, normal, depth, albedo: each stops some taps of the synthetic input and passes others
LENS = (0.08, 1.8)


def sigma_sets():
    """each sigma +inf in turn, all finite, and 1e-30f (its square underflows to 0: 0/0 and x/0 on the device) for depth and for colour"""
    sets = [tuple(INF if k == j else FINITE[k] for k in range(4)) for j in range(4)]
    sets += [FINITE, (FINITE[0], FINITE[1], 1e-30, FINITE[3]), (1e-30, INF, INF, INF)]
    return sets


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def differing(a, b):
    return int((bits(a) != bits(b)).sum())


def ref_params(p):
    return dr.Params(p.iterations, p.sigma_color, p.sigma_normal, p.sigma_depth, p.sigma_albedo)


def synthetic(rows, w, ch, seed=11):
    """a seeded random image and a hand-made gbuffer: holes, fractional alpha, -0.0f normal components, a depth step, two albedos, an
    isolated covered pixel between holes (centre tap only) -- so that every guide stops some taps and passes others"""
    rng = np.random.default_rng(seed + 1000 * rows + w)
    img = rng.random((rows, w, ch)).astype(F)
    alpha = np.ones((rows, w), F)
    alpha[rng.random((rows, w)) < 0.2] = 0.5
    alpha[rng.random((rows, w)) < 0.1] = 0.25
    z = np.where(np.arange(w)[None, :] * 2 < w, F(1.5), F(2.25)) + (np.arange(rows, dtype=F)[:, None] * F(0.03125))    # a depth step and a slope
    N = np.zeros((rows, w, 3), F)
    N[..., 2] = 1.0
    N[..., 0] = -0.0
    N[rows // 2:, :, :] = (0.6, -0.0, 0.8)                                         # a second normal below the middle row
    A = np.zeros((rows, w, 3), F)
    A[...] = (0.75, 0.5, 0.25)
    A[:, w // 3:2 * w // 3 + 1] = (0.5, 0.5, 0.625)                                # a second albedo in the middle third
    g = np.empty((rows, w, 8), F)
    g[..., 0] = alpha
    g[..., 1] = (z.astype(F) * alpha).astype(F)
    g[..., 2:5] = (N * alpha[..., None]).astype(F)
    g[..., 5:8] = (A * alpha[..., None]).astype(F)
    holes = rng.random((rows, w)) < 0.12
    if rows >= 5 and w >= 9:
        holes[0:5, 2:7] = True
        holes[2, 4] = False                                                           # alone: its 24 neighbours at step 1 are holes
        holes[rows - 1, w - 1] = False
    g[holes] = 0.0
    if rows * w == 1:
        g[0, 0, 0] = 1.0
    return img if ch == 3 else img[..., 0].copy(), g


class Guarded:
    """`nbytes` of device memory (rounded up to floats) with GUARD floats of PATTERN on both sides; the body starts 16-byte aligned"""

    def __init__(self, rt, nbytes, fill=None):
        self.floats = (int(nbytes) + 3) // 4
        self.init = np.full(self.floats + 2 * GUARD, PATTERN, np.uint32)
        if fill is not None:
            self.init[GUARD:GUARD + fill.size] = np.ascontiguousarray(fill, F).view(np.uint32).ravel()
        self.buf = rt.hipmem.DeviceBuffer(self.init.nbytes).from_numpy(self.init)
        self.address = self.buf.address + GUARD * 4
        self.ptr = C.c_void_p(self.address)

    def raw(self):
        return self.buf.to_numpy(np.uint32, self.init.shape)

    def guards_hold(self):
        raw = self.raw()
        return bool((raw[:GUARD] == PATTERN).all() and (raw[GUARD + self.floats:] == PATTERN).all())

    def body(self):
        return self.raw()[GUARD:GUARD + self.floats]

    def untouched(self):
        return bool((self.raw() == self.init).all())

    def free(self):
        self.buf.free()


def device_call(rt, lib, handle, img, g, p, stream=None, sync=None):
    """rt_denoise_device on guarded buffers -> the output in img's shape; checks the guards, that every output float was written and that the
    inputs are unchanged.  sync: a callable that waits for the call (default: hipDeviceSynchronize)"""
    rows, w = g.shape[:2]
    ch = 3 if img.ndim == 3 else 1
    d_in, d_g = Guarded(rt, img.nbytes, img), Guarded(rt, g.nbytes, g)
    need = lib.rt_denoise_scratch_bytes(w, rows, ch)
    d_scr, d_out = Guarded(rt, need), Guarded(rt, img.nbytes)
    try:
        st = lib.rt_denoise_device(handle, d_in.ptr, ch, d_g.ptr, w, rows, C.byref(p), d_scr.ptr, d_out.ptr, stream)
        rt.capi.check(lib, handle, st, "rt_denoise_device")
        (sync or rt.hipmem.synchronize)()
        assert d_out.guards_hold() and d_scr.guards_hold(), "bytes outside the output or the scratch were written"
        assert d_in.untouched() and d_g.untouched(), "an input was written"
        out = d_out.body()
        assert (out != PATTERN).all(), "floats of the output were left unwritten"
        return out.view(F).reshape(img.shape)
    finally:
        for b in (d_in, d_g, d_scr, d_out):
            b.free()


@pytest.fixture(scope="module")
def bare(rt):
    """a context WITHOUT a scene: the filter needs none"""
    ctx = rt.Context(0)
    yield ctx
    ctx.close()


_REFS = {}


def reference(key, img, g, p):
    """the restatement's answer, computed once per case and kept read-only"""
    if key not in _REFS:
        out = dr.denoise(img, g, ref_params(p))
        out.setflags(write=False)
        _REFS[key] = out
    return _REFS[key]


# ------------------------------------------------------------------------------------------ 1. synthetic images: every branch, every size
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_images_equal_the_restatement(rt, bare, size, ch):
    w, rows = size
    img, g = synthetic(rows, w, ch)
    lib = bare.lib
    outs = {}
    for it in (1, 2, 5):
        for k, sig in enumerate(sigma_sets()):
            p = rt.denoise_params(it, *sig)
            got = device_call(rt, lib, bare.handle, img, g, p)
            want = reference(("syn", size, ch, it, k), img, g, p)
            assert same(got, want), (it, sig, differing(got, want))
            outs[(it, k)] = got
    gd = dr.guide(g)
    assert same(outs[(5, 4)][~gd.covered], img[~gd.covered])
    if rows >= 5 and w >= 9:
        assert gd.covered[2, 4] and not gd.covered[0:5, 2:7].sum() > 1
        # the input takes the branches: with one guide finite and the others +inf the result differs from no guide at all
        free = dr.denoise(img, g, dr.Params(2))
        for j in range(4):
            only = [INF] * 4
            only[j] = FINITE[j]
            assert not same(dr.denoise(img, g, dr.Params(2, *only)), free), f"guide {j} stops no tap of the synthetic input"
        assert not same(free, img) and not same(outs[(5, 4)], outs[(2, 4)])


def test_eight_iterations_once(rt, bare):
    for ch in (1, 3):
        img, g = synthetic(21, 37, ch)
        p = rt.denoise_params(8, 2.0, 0.9, 0.3, 0.4)
        assert same(device_call(rt, bare.lib, bare.handle, img, g, p), reference(("eight", ch), img, g, p))


def test_the_pin_on_the_device(rt, bare):
    g = np.zeros((1, 2, 8), F)
    g[..., 0] = 1.0
    out = device_call(rt, bare.lib, bare.handle, np.array([[1.0, 0.0]], F), g, rt.denoise_params(1, INF, INF, INF, INF))
    assert bits(out).tolist() == [[0x3F19999A, 0x3ECCCCCD]]


# ------------------------------------------------------------------------------------------ 2. refusals on the device, no scene
def test_refusals_write_nothing_and_name_the_call(rt, bare):
    lib, h_ = bare.lib, bare.handle
    inv = rt.capi.RT_ERR_INVALID
    w, rows, ch = 37, 21, 3
    img, g = synthetic(rows, w, ch)
    p = rt.denoise_params()
    d_in, d_g = Guarded(rt, img.nbytes, img), Guarded(rt, g.nbytes, g)
    need = lib.rt_denoise_scratch_bytes(w, rows, ch)
    d_scr, d_out = Guarded(rt, need), Guarded(rt, img.nbytes)
    host_out = np.full(img.shape, 7.0, F)
    vp = lambda a: C.c_void_p(a.ctypes.data)

    def dev(in_=d_in.ptr, ch_=ch, g_=d_g.ptr, w_=w, r_=rows, p_=p, scr=d_scr.ptr, out=d_out.ptr):
        return lib.rt_denoise_device(h_, in_, ch_, g_, w_, r_, C.byref(p_) if p_ is not None else None, scr, out, None)

    def host(in_=vp(img), ch_=ch, g_=vp(g), w_=w, r_=rows, p_=p, out=vp(host_out)):
        return lib.rt_denoise(h_, in_, ch_, g_, w_, r_, C.byref(p_) if p_ is not None else None, out)

    def named(what=b"rt_denoise"):
        return what in lib.rt_last_error(h_)

    # NULL pointers, channels, width, rows
    for kw in (dict(in_=None), dict(g_=None), dict(p_=None), dict(out=None), dict(ch_=2), dict(ch_=0), dict(ch_=4), dict(w_=0), dict(w_=-3), dict(r_=-1)):
        assert dev(**kw) == inv and named(b"rt_denoise_device"), kw
        assert host(**kw) == inv and named(), kw
    assert dev(scr=None) == inv and named(b"rt_denoise_device")
    # iterations and sigmas out of range
    for bad in (rt.denoise_params(0), rt.denoise_params(9), rt.denoise_params(-1), rt.denoise_params(5, 0.0), rt.denoise_params(5, 1.0, -1.0),
                rt.denoise_params(5, 1.0, 1.0, float("nan")), rt.denoise_params(5, 1.0, 1.0, 1.0, -INF)):
        assert dev(p_=bad) == inv and named(b"rt_denoise_device") and host(p_=bad) == inv and named()
    # too many pixels
    assert dev(w_=2 ** 31 - 1, r_=2) == rt.capi.RT_ERR_UNSUPPORTED and named(b"rt_denoise_device")
    assert host(w_=46341, r_=46341) == rt.capi.RT_ERR_UNSUPPORTED and named()
    # an output or a scratch that is not 16-byte aligned (the device call only)
    for off in (4, 8, 12):
        assert dev(out=C.c_void_p(d_out.address + off)) == inv and named(b"aligned")
        assert dev(scr=C.c_void_p(d_scr.address + off)) == inv and named(b"aligned")
    # each overlap pair: out / scratch, out / image, out / gbuffer, scratch / image, scratch / gbuffer
    assert dev(out=d_scr.ptr) == inv and named(b"overlaps")
    assert dev(out=C.c_void_p(d_scr.address + need - 16)) == inv and named(b"overlaps")
    assert dev(out=d_in.ptr) == inv and named(b"overlaps")
    assert dev(out=C.c_void_p(d_in.address + (img.nbytes - 1) // 16 * 16)) == inv and named(b"overlaps")
    assert dev(out=d_g.ptr) == inv and named(b"overlaps")
    assert dev(in_=C.c_void_p(d_out.address + 16)) == inv and named(b"overlaps")
    assert dev(scr=d_in.ptr) == inv and named(b"overlaps")
    assert dev(scr=d_g.ptr) == inv and named(b"overlaps")
    assert dev(g_=C.c_void_p(d_scr.address + need - 4)) == inv and named(b"overlaps")
    # rows == 0: RT_OK, nothing enqueued
    assert dev(r_=0) == rt.capi.RT_OK and host(r_=0) == rt.capi.RT_OK
    rt.hipmem.synchronize()
    for b in (d_in, d_g, d_scr, d_out):
        assert b.untouched()
    assert (host_out == 7.0).all()
    # and the valid calls between the same guards, on a context that never saw a scene
    want = reference(("refusals",), img, g, p)
    assert dev() == rt.capi.RT_OK
    rt.hipmem.synchronize()
    assert d_out.guards_hold() and d_scr.guards_hold() and d_in.untouched() and d_g.untouched()
    assert same(d_out.body().view(F).reshape(img.shape), want)
    assert host() == rt.capi.RT_OK
    assert same(host_out, want)
    for b in (d_in, d_g, d_scr, d_out):
        b.free()


# ------------------------------------------------------------------------------------------ 3. real frames, buffers and occlusion
class Scene:
    def __init__(self, rt, path):
        self.rt, self.path = rt, path
        self.hs, self.ctx = gl.open_ctx(rt, path)
        self.lib = self.ctx.lib

    def settings(self, n=1, passes=(0, 1), lens=None, close=None, tau=-1.0):
        gp.set_frame(self.ctx, n, lens, close, passes, tau)
        self.ctx.set_pass_tolerance(-1.0, 8)

    def close(self):
        self.ctx.close()
        self.hs.close()


@pytest.fixture(scope="module")
def world(rt, scenes, tmp_path_factory):
    paths = {"cube": os.path.join(scenes, "cube.obj"), "dodge": os.path.join(scenes, "dodgeColorTest.obj"),
             "mixed": scenes_gen.mixed_materials(str(tmp_path_factory.mktemp("mixed")))}
    w = {k: Scene(rt, p) for k, p in paths.items()}
    yield w
    for s in w.values():
        s.close()


def frame_and_buffers(sc, w, h, depth=2):
    """rt_render_device colour and rt_gbuffer_device buffers of the context's settings at yaw 0.4, downloaded"""
    rt = sc.rt
    cam, L = rt.default_camera(w, h, YAW), gl.area_lights(rt, 5)
    rgb, _ = gl.render_device(rt, sc.ctx, cam, L, w, h, depth)
    buf = rt.hipmem.DeviceBuffer(w * h * 8 * 4)
    sc.ctx.gbuffer(cam, w, h, out=buf)
    sc.ctx.synchronize()
    g = buf.to_numpy(F, (h, w, 8))
    buf.free()
    return rgb, g


@pytest.mark.parametrize("name", ["cube", "mixed"])
def test_real_frames_equal_the_restatement(world, name):
    sc = world[name]
    w, h = 37, 21
    sc.settings(2, (1, 3), LENS)
    rgb, g = frame_and_buffers(sc, w, h)
    a = g[..., 0]
    assert ((a > 0) & (a < 1)).any() and (a == 0).any(), "the buffers hold partly covered and empty pixels"
    for it, sig in ((5, (1.0, 0.5, 0.125, 0.25)), (2, (0.25, INF, 0.05, 0.1)), (1, (INF, 0.3, INF, INF))):
        p = sc.rt.denoise_params(it, *sig)
        got = device_call(sc.rt, sc.lib, sc.ctx.handle, rgb, g, p)
        want = reference(("real", name, it, sig), rgb, g, p)
        print(f"{name} iterations {it} sigmas {sig}: {differing(got, want)} floats differ; {differing(got, rgb)} changed by the filter")
        assert same(got, want), (it, sig, differing(got, want))
        assert not same(got, rgb)
    sc.settings()


def test_flyscene_occlusion_with_and_without_the_filter(rt, world):
    w, h = 48, 32
    fs = rt.Flyscene(scene_path=world["mixed"].path)
    fs.initialize(w, h, True, False)
    try:
        fs.camera = rt.default_camera(w, h, YAW)
        raw = fs.ambient_occlusion(w, h, 2, 0.5, seed=3)
        fs.supersample, fs.passes = 1, 1
        g = fs.gbuffer(w, h)
        assert (g[..., 0] == 1.0).any() and len(np.unique(raw)) > 2
        p = rt.denoise_params()
        fs.ctx.set_supersampling(3)                                  # the call sets the one-ray pinhole frame itself
        got = fs.ambient_occlusion(w, h, 2, 0.5, seed=3, denoise=p)
        assert got.shape == raw.shape and same(got, dr.denoise(raw, g, ref_params(p)))
        assert not same(got, raw)
        assert same(fs.ambient_occlusion(w, h, 2, 0.5, seed=3), raw), "denoise=None is today's image"
    finally:
        fs.ctx.close()
        fs.scene.close()


# ------------------------------------------------------------------------------------------ 4. the context afterwards, a second stream
def frame(sc, w, h, n=1, tau=-1.0, depth=3):
    sc.settings(n, tau=tau)
    cam, L = sc.rt.default_camera(w, h, YAW), gl.area_lights(sc.rt, 5)
    rgb, _, st = gl.render(sc.rt, sc.ctx, cam, L, w, h, depth)
    return rgb, gl.counters(st), int(st.launches_total)


def test_refined_count_pass_map_and_later_frames_survive_a_call(world):
    sc = world["cube"]
    rt = sc.rt
    w, h = 64, 40
    img, g = synthetic(h, w, 3)
    p = rt.denoise_params()
    want_out = reference(("ctx",), img, g, p)
    before = frame(sc, w, h)
    adaptive = frame(sc, w, h, 2, 0.05)
    refined = sc.ctx.supersampling_refined()
    assert 0 < refined < w * h
    frame(sc, w, h, 2, 0.05)
    assert same(device_call(rt, sc.lib, sc.ctx.handle, img, g, p, sync=sc.ctx.synchronize), want_out)
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
    assert same(device_call(rt, sc.lib, sc.ctx.handle, img, g, p), want_out)
    assert np.array_equal(sc.ctx.pass_map(w, h), pm)
    rgb2, _, _ = gl.render(rt, sc.ctx, cam, L, w, h, 2)
    assert same(rgb2, rgb)
    sc.settings()


def test_a_call_on_a_second_stream_beside_a_frame(rt, world):
    sc = world["dodge"]
    hip = rt.hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    w, h = 96, 64
    try:
        sc.settings(2, (1, 2), LENS)
        cam, L = rt.default_camera(w, h, YAW), gl.area_lights(rt, 5)
        p = rt.make_params(w, h, 3)
        solo_rgb, g = frame_and_buffers(sc, w, h, 3)
        dp = rt.denoise_params()
        solo = device_call(rt, sc.lib, sc.ctx.handle, solo_rgb, g, dp)
        assert same(solo, reference(("stream",), solo_rgb, g, dp))
        rgb = Guarded(rt, w * h * 12)
        rt.capi.check(sc.lib, sc.ctx.handle, sc.lib.rt_render_device(sc.ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.ptr, None, None, None, None),
                      "rt_render_device")

        def wait():
            assert hip.hipStreamSynchronize(stream) == 0

        beside = device_call(rt, sc.lib, sc.ctx.handle, solo_rgb, g, dp, stream=stream, sync=wait)
        sc.ctx.synchronize()
        assert same(beside, solo)
        assert rgb.guards_hold() and same(rgb.body().view(F).reshape(h, w, 3), solo_rgb)
        rgb.free()
    finally:
        hip.hipStreamDestroy(stream)
        sc.settings()


# ------------------------------------------------------------------------------------------ 5. front ends
def test_context_denoise_on_tensors_and_device_buffers(rt, bare):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no device"
    w, rows = 37, 21
    dev = f"cuda:{bare.device}"
    for ch in (1, 3):
        img, g = synthetic(rows, w, ch)
        p = rt.denoise_params(3, *FINITE)
        want = reference(("front", ch), img, g, p)
        t_img, t_g = torch.from_numpy(img).to(dev), torch.from_numpy(g).to(dev)
        out = bare.denoise(t_img, t_g, w, rows, p)                            # torch's current (default) stream, scratch allocated
        assert out.dtype == torch.float32 and tuple(out.shape) == img.shape and str(out.device) == dev
        assert same(out.cpu().numpy(), want)
        s = torch.cuda.Stream(device=dev)
        canary = torch.full((img.size + 2 * GUARD,), 3.0, dtype=torch.float32, device=dev)
        scratch = torch.empty((bare.lib.rt_denoise_scratch_bytes(w, rows, ch),), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            view = canary[GUARD:GUARD + img.size]
            back = bare.denoise(t_img, t_g, w, rows, p, out=view, scratch=scratch)
        s.synchronize()
        assert back is view and same(view.cpu().numpy().reshape(img.shape), want)
        assert (canary[:GUARD] == 3.0).all() and (canary[-GUARD:] == 3.0).all()
        assert same(t_img.cpu().numpy(), img) and same(t_g.cpu().numpy(), g)
        b_img, b_g = rt.hipmem.DeviceBuffer(img.nbytes).from_numpy(img), rt.hipmem.DeviceBuffer(g.nbytes).from_numpy(g)
        b_out = rt.hipmem.DeviceBuffer(img.nbytes)
        assert bare.denoise(b_img, b_g, w, rows, p, out=b_out) is b_out     # channels from the buffer's size
        bare.synchronize()
        assert same(b_out.to_numpy(F, img.shape), want)
        fresh = bare.denoise(b_img, b_g, w, rows, p, channels=ch)
        bare.synchronize()
        assert same(fresh.to_numpy(F, img.shape), want)
        with pytest.raises(ValueError):
            bare.denoise(t_img, t_g[:-1], w, rows, p)
        with pytest.raises(ValueError):
            bare.denoise(t_img.double(), t_g, w, rows, p)
        with pytest.raises(ValueError):
            bare.denoise(b_img, b_g, w, rows, p, out=rt.hipmem.DeviceBuffer(16))
        with pytest.raises(ValueError):
            bare.denoise(t_img, t_g, w, rows, p, scratch=torch.empty((16,), dtype=torch.uint8, device=dev))
        for b in (b_img, b_g, b_out, fresh):
            b.free()
    p = rt.denoise_params()
    img, g = synthetic(rows, w, 3)
    assert same(bare.denoise(torch.from_numpy(img).to(dev), torch.from_numpy(g).to(dev), w, rows).cpu().numpy(), reference(("front", "default"), img, g, p))


def test_flyscene_member_and_the_cli(rt, scenes, tmp_path):
    w, h = 37, 21
    path = os.path.join(scenes, "dodgeColorTest.obj")
    args = (2, 0.5, 0.5, 0.125, 0.25)
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(w, h, True, False)
    try:
        fs.usteps = fs.vsteps = 2
        fs.max_depth, fs.supersample, fs.passes = 1, 2, 2
        fs.output_path = str(tmp_path / "python.ppm")
        assert fs.denoise is None
        plain = fs.raytraceScene(w, h, write_ppm=False).copy()
        g = fs.gbuffer(w, h)
        fs.denoise = rt.denoise_params(*args)
        got = fs.raytraceScene(w, h, write_ppm=True)
        assert same(got, dr.denoise(plain, g, ref_params(fs.denoise))) and not same(got, plain)
        fs.denoise = None
        assert same(fs.raytraceScene(w, h, write_ppm=False), plain), "unset is today's frame"
        fs.pass_tolerance, fs.passes, fs.denoise = 0.01, 12, rt.denoise_params(*args)
        with pytest.raises(rt.capi.RtError):
            fs.raytraceScene(w, h, write_ppm=False)                  # an adaptive-pass frame has no geometry buffers
    finally:
        fs.ctx.close()
        fs.scene.close()
    cli = ["--scene", path, "--size", str(w), str(h), "--samples", "2", "2", "--depth", "1", "--aa", "2", "--passes", "2"]
    r = subprocess.run([RT_RENDER] + cli + ["--denoise"] + [str(a) for a in args] + ["--out", "result.ppm"], input=b"1\n0\n", capture_output=True,
                       cwd=str(tmp_path), timeout=240)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(str(tmp_path / "result.ppm"), "rb").read() == open(str(tmp_path / "python.ppm"), "rb").read()
    r = subprocess.run([RT_RENDER] + cli + ["--out", "plain.ppm"], input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=240)
    assert r.returncode == 0 and open(str(tmp_path / "plain.ppm"), "rb").read() != open(str(tmp_path / "result.ppm"), "rb").read()
    r = subprocess.run([RT_RENDER] + cli + ["--pass-tolerance", "0.01", "--denoise"] + [str(a) for a in args], input=b"1\n0\n", capture_output=True,
                       cwd=str(tmp_path), timeout=240)
    assert r.returncode == 2 and b"--pass-tolerance" in r.stderr


# ------------------------------------------------------------------------------------------ 6. strided rounds and far taps
# The helpers below are pure numpy: tests/test_grid_stride_shapes.py asserts the same conditions on the restatement without a device.
FAR = (INF, 0.6, 0.3, 0.4)                   # no colour stop: the far taps of a noise image are accepted, so every iteration moves the image
EIGHT = (2.0, 0.9, 0.3, 0.4)                 # the sigmas of test_eight_iterations_once: the colour scale halves per iteration
FAR_SHAPES = {"column": None, "row": (1100, 3), "both": (300, 261)}       # (width, rows); the column's rows come from the CU count


def far_shape(which, cus):
    return gc.atrous_column(cus) if which == "column" else FAR_SHAPES[which]


def stepwise(img, g, p):
    """the restatement iteration by iteration -> (the images I_1 .. I_iterations in img's shape, the fraction of the covered pixels that
    iteration k moved, for every k)"""
    flat = img.ndim == 2
    cur = np.asarray(img[..., None] if flat else img, F)
    gd = dr.guide(g)
    images, moved = [], []
    for k in range(p.iterations):
        nxt = dr.iteration(cur, gd, k, p)
        moved.append(float(((bits(nxt) != bits(cur)).any(axis=-1) & gd.covered).sum()) / float(gd.covered.sum()))
        cur = nxt
        images.append(cur[..., 0].copy() if flat else cur)
    return images, moved


_STEPWISE = {}


def stepwise_reference(key, img, g, p):
    if key not in _STEPWISE:
        images, moved = stepwise(img, g, ref_params(p))
        for a in images:
            a.setflags(write=False)
        _STEPWISE[key] = (images, moved)
    return _STEPWISE[key]


def every_iteration_moves_the_image(moved):
    """with sigma_color = +inf: iteration k moves more than half of the covered pixels, for every k"""
    return len(moved) == dr.MAX_ITERATIONS and all(m > 0.5 for m in moved)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("sig", [FAR, EIGHT], ids=["far", "eight"])
def test_strided_tiles_of_a_pixel_column(rt, bare, sig, ch):
    """k_atrous beyond its grid: a block strides over tiles of one tile column, and the taps reach 256 rows up and down inside the image"""
    cus = gc.cu_count(bare.device)
    w, rows = far_shape("column", cus)
    tiles = gc.dn_tiles(w, rows)[2]
    assert gc.strides(tiles, gc.dn_cap(cus)) and gc.dn_grid(tiles, cus) < tiles, (cus, w, rows)
    assert rows > 2 * 128 and rows % gc.DN_TILE_H != 0
    img, g = synthetic(rows, w, ch)
    p = rt.denoise_params(8, *sig)
    images, moved = stepwise_reference(("far", "column", sig, ch), img, g, p)
    print(f"{w}x{rows} channels {ch} sigmas {sig}: moved per iteration {[round(m, 4) for m in moved]}")
    if sig[0] == INF:
        assert every_iteration_moves_the_image(moved), moved
    got = device_call(rt, bare.lib, bare.handle, img, g, p)
    assert same(got, images[-1]), differing(got, images[-1])


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("which,sigs", [("row", (FAR, EIGHT)), ("both", (FAR,))], ids=["row", "both"])
def test_far_taps_inside_the_image(rt, bare, which, sigs, ch):
    """eight iterations on images wider (and higher) than the reach of the last one, 2 * 128 pixels: taps of every step are accepted"""
    w, rows = far_shape(which, gc.cu_count(bare.device))
    assert w > 2 * 128 and (which == "row" or rows > 2 * 128)
    img, g = synthetic(rows, w, ch)
    for sig in sigs:
        p = rt.denoise_params(8, *sig)
        images, moved = stepwise_reference(("far", which, sig, ch), img, g, p)
        print(f"{w}x{rows} channels {ch} sigmas {sig}: moved per iteration {[round(m, 4) for m in moved]}")
        if sig[0] == INF:
            assert every_iteration_moves_the_image(moved), moved
        got = device_call(rt, bare.lib, bare.handle, img, g, p)
        assert same(got, images[-1]), (sig, differing(got, images[-1]))


@pytest.mark.parametrize("ch", [1, 3])
def test_strided_guide_blocks_and_tiles_of_a_frame(rt, bare, ch):
    """k_denoise_guide and k_atrous both beyond their grids on an image of several tile columns: two iterations, so a working-image write
    and the write of the output are both strided, and round 2 starts in the middle of a tile row"""
    cus = gc.cu_count(bare.device)
    w, rows = gc.denoise_frame(cus)
    tx, _, tiles = gc.dn_tiles(w, rows)
    assert gc.strides(tiles, gc.dn_cap(cus)) and gc.dn_grid(tiles, cus) < tiles, (cus, w, rows)
    assert gc.strides(w * rows, gc.dn_guide_cap(cus)) and gc.dn_guide_grid(w * rows, cus) * gc.DN_GUIDE_BLOCK < w * rows, (cus, w, rows)
    assert tx > 1 and gc.dn_cap(cus) % tx != 0 and w % gc.DN_TILE_W != 0
    img, g = synthetic(rows, w, ch)
    p = rt.denoise_params(2, *FINITE)
    images, _ = stepwise_reference(("frame", ch), img, g, p)
    assert not same(images[1], images[0]), "the second iteration must show"
    got = device_call(rt, bare.lib, bare.handle, img, g, p)
    assert same(got, images[1]), differing(got, images[1])


# ------------------------------------------------------------------------------------------ 7. non-finite inputs
POISON_SIZES = ((37, 21), (70, 5))
POISON_SIGMAS = (FINITE, (INF, INF, INF, INF), FAR)


def poisoned(rows, w, ch, seed=5):
    """synthetic() with a seeded ~6 % of the image pixels NaN / +inf / -inf (one channel of the pixel for three channels), ~5 % of the alphas
    NaN / -1 / +inf / -0.0 and one of g[1..7] NaN at a further ~4 % of the pixels -> (image, gbuffer, the pixels whose image value is not
    finite).  The same pixels for one and for three channels."""
    img, g = synthetic(rows, w, ch)
    img, g = img.copy(), g.copy()
    rng = np.random.default_rng(seed + 1000 * rows + w)
    draws = [rng.random((rows, w)) for _ in range(3)]
    bad_img = draws[0] < 0.06
    bad_alpha = draws[1] < 0.05
    bad_g = (draws[2] < 0.04) & ~bad_alpha
    channel = rng.integers(0, 3, (rows, w))
    which = rng.integers(1, 8, (rows, w))
    ys, xs = np.nonzero(bad_img)
    value = np.array([np.nan, np.inf, -np.inf], F)[np.arange(len(ys)) % 3]             # the kinds in turn: a small image holds each of them
    if ch == 3:
        img[ys, xs, channel[ys, xs]] = value
    else:
        img[ys, xs] = value
    ys, xs = np.nonzero(bad_alpha)
    g[ys, xs, 0] = np.array([np.nan, -1.0, np.inf, -0.0], F)[np.arange(len(ys)) % 4]
    ys, xs = np.nonzero(bad_g)
    g[ys, xs, which[ys, xs]] = np.nan
    return img, g, bad_img


def pixel_not_finite(img):
    a = ~np.isfinite(np.asarray(img, F))
    return a.any(axis=-1) if a.ndim == 3 else a


def same_but_nan_payloads(got, want):
    """where `want` is not NaN the bit patterns are equal; where it is NaN, `got` is NaN (the default NaN of the CPU and the device's differ)"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.isnan(got[nan]).all()) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def poison_stays_where_it_was(out, clean_out, bad):
    """(the pixels with a non-finite output are the pixels with a non-finite input, how many finite pixels differ from the clean run)"""
    gone = pixel_not_finite(out)
    d = bits(out) != bits(clean_out)
    d = d.any(axis=-1) if d.ndim == 3 else d
    return bool(np.array_equal(gone, bad)), int((d & ~gone).sum())


def poison_shows(size):
    """the finite pixels that must differ from the run on the clean image with the same buffers: more than 100 of the 777 of 37 x 21, any of
    the 350 of 70 x 5"""
    return 100 if size == (37, 21) else 0


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("size", POISON_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_non_finite_inputs_follow_the_definition(rt, bare, size, ch):
    """NaN and infinities in the image, NaN / negative / infinite / -0.0f alphas and NaN guide values are inputs the definition covers: a tap
    whose u is not > 0.0f is stopped, a pixel is covered exactly when a > 0.0f"""
    w, rows = size
    img, g, bad = poisoned(rows, w, ch)
    clean, _ = synthetic(rows, w, ch)
    assert np.array_equal(pixel_not_finite(img), bad) and bad.sum() >= 5
    assert np.isnan(g[..., 0]).any() and (g[..., 0] < 0).any() and np.isinf(g[..., 0]).any() and np.isnan(g[..., 1:]).any()
    for it in (1, 5):
        for k, sig in enumerate(POISON_SIGMAS):
            p = rt.denoise_params(it, *sig)
            want = reference(("poison", size, ch, it, k), img, g, p)
            stays, differ = poison_stays_where_it_was(want, reference(("poison clean", size, ch, it, k), clean, g, p), bad)
            print(f"{w}x{rows} channels {ch} iterations {it} sigmas {sig}: {int(bad.sum())} pixels not finite, {differ} finite pixels differ from the clean run")
            assert stays, "a non-finite value leaked to another pixel or vanished"
            assert differ > poison_shows(size), "the poisoned taps must be stopped, not merely absent"
            got = device_call(rt, bare.lib, bare.handle, img, g, p)
            assert same_but_nan_payloads(got, want), (it, sig)


def test_counting_build_gives_the_same_bits(rt):
    lib = rt.capi.load_library(WORK_LIB)
    ctx = C.c_void_p()
    assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
    try:
        for ch in (1, 3):
            img, g = synthetic(21, 37, ch)
            p = rt.denoise_params(3, *FINITE)
            want = reference(("front", ch), img, g, p)
            assert same(device_call(rt, lib, ctx, img, g, p), want)
            out = np.zeros(img.shape, F)
            vp = lambda a: C.c_void_p(a.ctypes.data)
            rt.capi.check(lib, ctx, lib.rt_denoise(ctx, vp(img), ch, vp(g), 37, 21, C.byref(p), vp(out)), "rt_denoise")
            assert same(out, want)
    finally:
        lib.rt_destroy(ctx)
