"""The temporal reprojection on a real MI355X: rt_reproject_device returns, bit for bit, what the "temporal reprojection" section of
include/rt_mi355x.h defines -- against tests/reproject_ref.py -- for synthetic images that take every branch at every size, channel count and
map, for images of more tiles than its grid holds (tests/grid_caps.py: blocks stride to a second round), for NaN, infinite and negative
values in every input, and for real one-ray frames of a camera path with their geometry buffers; it writes nothing outside its two outputs,
leaves its inputs and the context as they were, refuses what it must, needs no scene, and the host form, Context.reproject and the counting
build give the same bits.  Every comparison is on the bit patterns.  No graph is captured anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import grid_caps as gc
import scenes_gen
import switch_table
import test_gpu_denoise as gd
import test_gpu_lens as gl
import test_reproject_api as ra
import reproject_ref as rr
from test_gpu_denoise import Guarded, PATTERN, bits, differing, same, same_but_nan_payloads

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORK_LIB = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")
F = np.float32
INF = float("inf")
SIGMA_SETS = (ra.ALL_INF, ra.DEFAULTS, ra.TIGHT)
LEN_PATTERN = 0xA5


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def ref_params(p):
    return rr.Params(p.max_history, p.sigma_normal, p.sigma_depth, p.sigma_albedo)


def c_map(m):
    return (C.c_float * 12)(*[float(v) for v in np.asarray(m, F).reshape(12)])


def device_call(rt, lib, handle, cur, g_cur, hist, g_hist, lens, m, p, stream=None, sync=None):
    """rt_reproject_device on guarded buffers -> (out in cur's shape, len_out); checks the guards, that every output float and length byte
    was written and that the inputs are unchanged.  sync: a callable that waits for the call (default: hipDeviceSynchronize)"""
    rows, width = g_cur.shape[:2]
    ch = 3 if cur.ndim == 3 else 1
    ins = [Guarded(rt, a.nbytes, a) for a in (cur, g_cur, hist, g_hist)]
    packed = np.full((width * rows + 3) // 4 * 4, LEN_PATTERN, np.uint8)
    packed[:width * rows] = lens.reshape(-1)
    d_len = Guarded(rt, width * rows, packed.view(F))
    d_out, d_lo = Guarded(rt, width * rows * ch * 4), Guarded(rt, width * rows)
    try:
        st = lib.rt_reproject_device(handle, ins[0].ptr, ch, ins[1].ptr, ins[2].ptr, ins[3].ptr, d_len.ptr, width, rows, c_map(m), C.byref(p), d_out.ptr,
                                     d_lo.ptr, stream)
        rt.capi.check(lib, handle, st, "rt_reproject_device")
        (sync or rt.hipmem.synchronize)()
        assert d_out.guards_hold() and d_lo.guards_hold(), "bytes outside an output were written"
        assert all(b.untouched() for b in ins) and d_len.untouched(), "an input was written"
        out = d_out.body()
        assert (out != PATTERN).all(), "floats of the output were left unwritten"
        raw = d_lo.body().view(np.uint8)
        lo = raw[:width * rows].reshape(rows, width).copy()
        assert (raw[width * rows:] == LEN_PATTERN).all(), "bytes behind the lengths were written"
        assert (lo != LEN_PATTERN).all(), "length bytes were left unwritten"
        return out.view(F).reshape(cur.shape), lo
    finally:
        for b in ins + [d_len, d_out, d_lo]:
            b.free()


@pytest.fixture(scope="module")
def bare(rt):
    """a context WITHOUT a scene: the operator needs none"""
    ctx = rt.Context(0)
    yield ctx
    ctx.close()


_REFS = {}


def reference(key, cur, g_cur, hist, g_hist, lens, m, p):
    """the restatement's (out, len_out), computed once per case and kept read-only"""
    if key not in _REFS:
        out, lo = rr.reproject(cur, g_cur, hist, g_hist, lens, m, ref_params(p))
        out.setflags(write=False)
        lo.setflags(write=False)
        _REFS[key] = (out, lo)
    return _REFS[key]


def synthetic(rows, width, ch):
    """ra.synthetic; no length is LEN_PATTERN - 1, so no len_out is LEN_PATTERN (which would read as unwritten)"""
    cur, g, hist, gh, lens = ra.synthetic(rows, width, ch)
    assert LEN_PATTERN - 1 not in lens
    return cur, g, hist, gh, lens


# ------------------------------------------------------------------------------------------ 1. synthetic images: every size, map, sigma set
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("size", ra.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_images_equal_the_restatement(rt, bare, size, ch):
    width, rows = size
    cur, g, hist, gh, lens = synthetic(rows, width, ch)
    assert 0 in lens or width * rows < 16
    for name, m in ra.maps(rt, width, rows).items():
        for k, sig in enumerate(SIGMA_SETS):
            if name not in ("identity", "half+x", "yaw", "behind") and k != 1:
                continue                                     # the other shifts with the defaults only
            p = rt.reproject_params(255 if k == 0 else 32, *sig)
            want, want_len = reference(("syn", size, ch, name, k), cur, g, hist, gh, lens, m, p)
            got, lo = device_call(rt, bare.lib, bare.handle, cur, g, hist, gh, lens, m, p)
            assert same(got, want), (name, sig, differing(got, want))
            assert np.array_equal(lo, want_len), (name, sig, int((lo != want_len).sum()))


def test_the_pins_on_the_device(rt, bare):
    cg = ra.covered_gbuffer
    g2, one = cg(1, 2), np.ones((1, 2), np.uint8)
    P = rt.reproject_params
    call = lambda *a: device_call(rt, bare.lib, bare.handle, *a)
    out, lo = call(np.array([[0.0, 1.0]], F), g2, np.array([[1.0, 0.0]], F), g2, one, ra.identity(), P(255, INF, INF, INF))
    assert bits(out).tolist() == [[0x3F000000, 0x3F000000]] and lo.tolist() == [[2, 2]]
    out, lo = call(np.zeros((1, 2), F), g2, np.array([[1.0, 0.0]], F), g2, one, ra.identity(x_W=0.5), P(255, INF, INF, INF))
    assert bits(out).tolist() == [[0x3E800000, 0]] and lo.tolist() == [[2, 2]]
    out, lo = call(np.array([[0.0, 1.0]], F), g2, np.array([[1.0, 0.0]], F), cg(1, 2, [1.0, 3.0]), one, ra.identity(), P(255, INF, 0.25, INF))
    assert bits(out).tolist() == [[0x3F000000, 0x3F800000]] and lo.tolist() == [[2, 1]]
    out, lo = call(np.array([[0.0, 1.0]], F), g2, np.array([[1.0, 0.0]], F), g2, np.array([[255, 0]], np.uint8), ra.identity(), P(4, INF, INF, INF))
    assert bits(out).tolist() == [[0x3F400000, 0x3F800000]] and lo.tolist() == [[4, 1]]
    g3 = cg(3, 1)
    out, lo = call(np.zeros((3, 1), F), g3, np.array([[1.0], [2.0], [3.0]], F), g3, np.ones((3, 1), np.uint8), ra.identity(y_W=-1.0), P(255, INF, INF, INF))
    assert bits(out).tolist() == [[0], [0x3F000000], [0x3F800000]] and lo.tolist() == [[1], [2], [2]]


# ------------------------------------------------------------------------------------------ 2. refusals on the device, no scene
def test_refusals_write_nothing_and_name_the_call(rt, bare):
    lib, h_ = bare.lib, bare.handle
    inv = rt.capi.RT_ERR_INVALID
    width, rows, ch = 37, 21, 3
    cur, g, hist, gh, lens = synthetic(rows, width, ch)
    p = rt.reproject_params()
    ident = ra.identity()
    d_cur, d_gc, d_hist, d_gh = (Guarded(rt, a.nbytes, a) for a in (cur, g, hist, gh))
    packed = np.zeros((width * rows + 3) // 4 * 4, np.uint8)
    packed[:width * rows] = lens.reshape(-1)
    d_lh = Guarded(rt, width * rows, packed.view(F))
    d_out, d_lo = Guarded(rt, width * rows * ch * 4), Guarded(rt, width * rows)
    host_out, host_lo = np.full((rows, width, ch), 7.0, F), np.full((rows, width), 9, np.uint8)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    at = lambda b, off=0: C.c_void_p(b.address + off)

    def dev(cur_=d_cur.ptr, ch_=ch, gc_=d_gc.ptr, hist_=d_hist.ptr, gh_=d_gh.ptr, lh_=d_lh.ptr, w_=width, r_=rows, m_=ident, p_=p, out=d_out.ptr, lo=d_lo.ptr):
        return lib.rt_reproject_device(h_, cur_, ch_, gc_, hist_, gh_, lh_, w_, r_, c_map(m_) if m_ is not None else None,
                                       C.byref(p_) if p_ is not None else None, out, lo, None)

    def host(cur_=vp(cur), ch_=ch, gc_=vp(g), hist_=vp(hist), gh_=vp(gh), lh_=vp(lens), w_=width, r_=rows, m_=ident, p_=p, out=vp(host_out), lo=vp(host_lo)):
        return lib.rt_reproject(h_, cur_, ch_, gc_, hist_, gh_, lh_, w_, r_, c_map(m_) if m_ is not None else None, C.byref(p_) if p_ is not None else None,
                                out, lo)

    def named(what=b"rt_reproject"):
        return what in lib.rt_last_error(h_)

    for kw in (dict(cur_=None), dict(gc_=None), dict(hist_=None), dict(gh_=None), dict(lh_=None), dict(m_=None), dict(p_=None), dict(out=None), dict(lo=None),
               dict(ch_=2), dict(ch_=0), dict(ch_=4), dict(w_=0), dict(w_=-3), dict(r_=-1)):
        assert dev(**kw) == inv and named(b"rt_reproject_device"), kw
        assert host(**kw) == inv and named(), kw
    P = rt.reproject_params
    for bad in (P(0), P(256), P(-1), P(4, 0.0), P(4, 1.0, -1.0), P(4, 1.0, float("nan")), P(4, 1.0, 1.0, -INF)):
        assert dev(p_=bad) == inv and named(b"rt_reproject_device") and host(p_=bad) == inv and named()
    for k, v in ((0, float("nan")), (5, INF), (11, -INF)):
        m = ident.copy()
        m.reshape(-1)[k] = v
        assert dev(m_=m) == inv and named(b"not finite") and host(m_=m) == inv and named(b"not finite")
    assert dev(w_=2 ** 31 - 1, r_=2) == rt.capi.RT_ERR_UNSUPPORTED and named(b"rt_reproject_device")
    assert host(w_=46341, r_=46341) == rt.capi.RT_ERR_UNSUPPORTED and named()
    for off in (4, 8, 12):
        assert dev(out=at(d_out, off)) == inv and named(b"aligned")
        assert dev(gc_=at(d_gc, off)) == inv and named(b"aligned")
        assert dev(gh_=at(d_gh, off)) == inv and named(b"aligned")
    img = width * rows * ch * 4
    assert dev(lo=at(d_out, img - 1)) == inv and named(b"overlaps")
    for inp, nbytes in ((d_cur, img), (d_gc, g.nbytes), (d_hist, img), (d_gh, gh.nbytes), (d_lh, width * rows)):
        assert dev(out=at(inp, 0)) == inv and named(b"overlap"), "the output on an input"
        assert dev(lo=at(inp, nbytes - 1)) == inv and named(b"overlap"), "the output lengths on an input's last byte"
    assert dev(hist_=at(d_out, 16)) == inv and named(b"overlaps") and dev(lh_=at(d_lo, 3)) == inv and named(b"overlap")
    assert dev(r_=0) == rt.capi.RT_OK and host(r_=0) == rt.capi.RT_OK
    rt.hipmem.synchronize()
    for b in (d_cur, d_gc, d_hist, d_gh, d_lh, d_out, d_lo):
        assert b.untouched()
    assert (host_out == 7.0).all() and (host_lo == 9).all()
    # and the valid calls between the same guards, on a context that never saw a scene
    want, want_len = reference(("refusals",), cur, g, hist, gh, lens, ident, p)
    assert dev() == rt.capi.RT_OK
    rt.hipmem.synchronize()
    assert d_out.guards_hold() and d_lo.guards_hold() and all(b.untouched() for b in (d_cur, d_gc, d_hist, d_gh, d_lh))
    assert same(d_out.body().view(F).reshape(want.shape), want)
    assert np.array_equal(d_lo.body().view(np.uint8)[:width * rows].reshape(rows, width), want_len)
    assert host() == rt.capi.RT_OK
    assert same(host_out, want) and np.array_equal(host_lo, want_len)
    assert host(hist_=vp(cur), gh_=vp(g)) == rt.capi.RT_OK, "inputs may share bytes"
    for b in (d_cur, d_gc, d_hist, d_gh, d_lh, d_out, d_lo):
        b.free()


# ------------------------------------------------------------------------------------------ 3. non-finite inputs
def poisoned(rows, width, ch, seed=5):
    """synthetic() with a seeded ~8 % of the pixels of both images NaN / +inf / -inf / negative, ~5 % of the alphas of both buffers NaN / -1 /
    +inf / -0.0, one of g[1..7] NaN at a further ~4 % of their pixels and a zero or negative depth at ~3 %"""
    cur, g, hist, gh, lens = (a.copy() for a in synthetic(rows, width, ch))
    rng = np.random.default_rng(seed + rows + width)
    for img in (cur, hist):
        ys, xs = np.nonzero(rng.random(img.shape[:2]) < 0.08)
        value = np.array([np.nan, np.inf, -np.inf, -2.5], F)[np.arange(len(ys)) % 4]
        if ch == 3:
            img[ys, xs, rng.integers(0, 3, len(ys))] = value
        else:
            img[ys, xs] = value
    for b in (g, gh):
        bad_alpha = rng.random(b.shape[:2]) < 0.05
        bad_g = (rng.random(b.shape[:2]) < 0.04) & ~bad_alpha
        bad_z = (rng.random(b.shape[:2]) < 0.03) & ~bad_alpha & ~bad_g
        ys, xs = np.nonzero(bad_alpha)
        b[ys, xs, 0] = np.array([np.nan, -1.0, np.inf, -0.0], F)[np.arange(len(ys)) % 4]
        ys, xs = np.nonzero(bad_g)
        b[ys, xs, rng.integers(1, 8, len(ys))] = np.nan
        ys, xs = np.nonzero(bad_z)
        b[ys, xs, 1] = np.array([0.0, -1.5, np.inf, -0.0], F)[np.arange(len(ys)) % 4]
    return cur, g, hist, gh, lens


@pytest.mark.parametrize("ch", [1, 3])
def test_non_finite_inputs_follow_the_definition(rt, bare, ch):
    """NaN and infinities in both images, NaN / negative / infinite / -0.0f alphas, NaN guide values and zero, negative and infinite depths
    are inputs the definition covers: every test on them is a float test that a NaN fails, made before any conversion to an integer"""
    width, rows = 67, 21
    cur, g, hist, gh, lens = poisoned(rows, width, ch)
    assert np.isnan(cur).any() and np.isinf(hist).any()
    for b in (g, gh):
        assert np.isnan(b[..., 0]).any() and (b[..., 0] < 0).any() and np.isinf(b[..., 0]).any() and np.isnan(b[..., 1:]).any() and (b[..., 1] == 0).any()
    for name in ("identity", "half-y", "yaw", "behind"):
        m = ra.maps(rt, width, rows)[name]
        for k, sig in enumerate(SIGMA_SETS):
            p = rt.reproject_params(32, *sig)
            want, want_len = reference(("poison", ch, name, k), cur, g, hist, gh, lens, m, p)
            got, lo = device_call(rt, bare.lib, bare.handle, cur, g, hist, gh, lens, m, p)
            assert same_but_nan_payloads(got, want), (name, sig)
            assert np.array_equal(lo, want_len), (name, sig)


# ------------------------------------------------------------------------------------------ 4. strided rounds
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("which", ["column", "frame"])
def test_strided_tiles(rt, bare, which, ch):
    """k_reproject beyond its grid: a pixel column of more tiles than one round holds, and a frame of several tile columns whose second round
    starts in the middle of a tile row (the shapes of the denoiser's strided tests)"""
    cus = gc.cu_count(bare.device)
    width, rows = gc.atrous_column(cus) if which == "column" else gc.denoise_frame(cus)
    tiles = gc.dn_tiles(width, rows)[2]
    assert gc.strides(tiles, gc.dn_cap(cus)) and gc.dn_grid(tiles, cus) < tiles, (cus, width, rows)
    cur, g, hist, gh, lens = synthetic(rows, width, ch)
    m = ra.identity(y_W=0.5) if which == "column" else ra.maps(rt, width, rows)["yaw"]
    p = rt.reproject_params(32, *ra.DEFAULTS)
    want, want_len = reference(("strided", which, ch), cur, g, hist, gh, lens, m, p)
    got, lo = device_call(rt, bare.lib, bare.handle, cur, g, hist, gh, lens, m, p)
    assert same(got, want), differing(got, want)
    assert np.array_equal(lo, want_len)
    assert (want_len > 1).any() and (want_len[-4:] > 1).any(), "the last rows, written in the second round, carry history"


# ------------------------------------------------------------------------------------------ 5. real frames of a camera path
@pytest.fixture(scope="module")
def world(rt, scenes, tmp_path_factory):
    paths = {"cube": os.path.join(scenes, "cube.obj"), "mixed": scenes_gen.mixed_materials(str(tmp_path_factory.mktemp("mixed")))}
    w = {k: gd.Scene(rt, p) for k, p in paths.items()}
    yield w
    for s in w.values():
        s.close()


def frame_and_buffers(sc, w, h, yaw):
    rt = sc.rt
    cam, L = rt.default_camera(w, h, yaw), gl.area_lights(rt, 5)
    rgb, _ = gl.render_device(rt, sc.ctx, cam, L, w, h, 2)
    buf = rt.hipmem.DeviceBuffer(w * h * 8 * 4)
    try:
        sc.ctx.gbuffer(cam, w, h, out=buf)
        sc.ctx.synchronize()
        return cam, rgb, buf.to_numpy(F, (h, w, 8))
    finally:
        buf.free()


@pytest.mark.parametrize("name", ["cube", "mixed"])
def test_real_frames_of_a_camera_path(world, name):
    """96 x 64 one-ray pinhole frames at yaw 0.40 and 0.42 with their rt_gbuffer_device buffers and the map of the two cameras: the
    restatement's bits; most covered pixels find their history; then a 4-frame chain through ping-pong buffers"""
    sc = world[name]
    rt = sc.rt
    W, H = 96, 64
    sc.settings()
    prev, rgb0, g0 = frame_and_buffers(sc, W, H, 0.40)
    cam, rgb1, g1 = frame_and_buffers(sc, W, H, 0.42)
    m = rt.reproject_map(cam, prev)
    ones = np.ones((H, W), np.uint8)
    assert (g1[..., 0] == 1.0).any() and (g1[..., 0] == 0.0).any() and not same(g0, g1)
    for k, sig in enumerate((ra.DEFAULTS, ra.ALL_INF, ra.TIGHT)):
        p = rt.reproject_params(32, *sig)
        want, want_len = reference(("real", name, k), rgb1, g1, rgb0, g0, ones, m, p)
        got, lo = device_call(rt, sc.lib, sc.ctx.handle, rgb1, g1, rgb0, g0, ones, m, p)
        cov = g1[..., 0] > 0
        print(f"{name} sigmas {sig}: {differing(got, want)} floats differ, {int((want_len[cov] == 1).sum())} of {int(cov.sum())} covered pixels lost their history")
        assert same(got, want) and np.array_equal(lo, want_len), sig
        if sig == ra.DEFAULTS:
            assert (want_len[cov] == 2).mean() > 0.5 and (want_len[~cov] == 1).all()
    p = rt.reproject_params()
    acc, ln, g_prev, c_prev = rgb0, ones, g0, prev
    for step, yaw in enumerate((0.42, 0.44, 0.46)):
        c, rgb, g = frame_and_buffers(sc, W, H, yaw)
        mm = rt.reproject_map(c, c_prev)
        want, want_len = rr.reproject(rgb, g, acc, g_prev, ln, mm, ref_params(p))
        got, lo = device_call(rt, sc.lib, sc.ctx.handle, rgb, g, acc, g_prev, ln, mm, p)
        assert same(got, want) and np.array_equal(lo, want_len), step
        acc, ln, g_prev, c_prev = got, lo, g, c
    assert ln.max() == 4


def test_refined_count_pass_map_and_later_frames_survive_a_call(world):
    sc = world["cube"]
    rt = sc.rt
    w, h = 64, 40
    cur, g, hist, gh, lens = synthetic(h, w, 3)
    p, m = rt.reproject_params(), ra.identity(x_W=0.5)
    want, want_len = reference(("ctx",), cur, g, hist, gh, lens, m, p)
    before = gd.frame(sc, w, h)
    adaptive = gd.frame(sc, w, h, 2, 0.05)
    refined = sc.ctx.supersampling_refined()
    assert 0 < refined < w * h
    got, lo = device_call(rt, sc.lib, sc.ctx.handle, cur, g, hist, gh, lens, m, p, sync=sc.ctx.synchronize)
    assert same(got, want) and np.array_equal(lo, want_len)
    assert sc.ctx.supersampling_refined() == refined
    again = gd.frame(sc, w, h, 2, 0.05)
    assert same(again[0], adaptive[0]) and again[1:] == adaptive[1:]
    after = gd.frame(sc, w, h)
    assert same(after[0], before[0]) and after[1:] == before[1:]
    sc.settings(1, (0, 12))
    sc.ctx.set_pass_tolerance(0.01, 4)
    cam, L = rt.default_camera(w, h, gd.YAW), gl.area_lights(rt, 5)
    rgb, _, _ = gl.render(rt, sc.ctx, cam, L, w, h, 2)
    pm = sc.ctx.pass_map(w, h)
    assert same(device_call(rt, sc.lib, sc.ctx.handle, cur, g, hist, gh, lens, m, p)[0], want)
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
        cam, L = rt.default_camera(w, h, gd.YAW), gl.area_lights(rt, 5)
        prm = rt.make_params(w, h, 3)
        solo_rgb, _ = gl.render_device(rt, sc.ctx, cam, L, w, h, 3)
        cur, g, hist, gh, lens = synthetic(h, w, 3)
        p, m = rt.reproject_params(), ra.maps(rt, w, h)["yaw"]
        want, want_len = reference(("stream",), cur, g, hist, gh, lens, m, p)
        rgb = Guarded(rt, w * h * 12)
        rt.capi.check(sc.lib, sc.ctx.handle, sc.lib.rt_render_device(sc.ctx.handle, C.byref(cam), C.byref(L), C.byref(prm), rgb.ptr, None, None, None, None),
                      "rt_render_device")

        def wait():
            assert hip.hipStreamSynchronize(stream) == 0

        beside, lo = device_call(rt, sc.lib, sc.ctx.handle, cur, g, hist, gh, lens, m, p, stream=stream, sync=wait)
        sc.ctx.synchronize()
        assert same(beside, want) and np.array_equal(lo, want_len)
        assert rgb.guards_hold() and same(rgb.body().view(F).reshape(h, w, 3), solo_rgb)
        rgb.free()
    finally:
        hip.hipStreamDestroy(stream)
        sc.settings()


# ------------------------------------------------------------------------------------------ 6. front ends
def test_context_reproject_on_tensors_and_device_buffers(rt, bare):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no device"
    width, rows = 37, 21
    dev = f"cuda:{bare.device}"
    for ch in (1, 3):
        arrays = synthetic(rows, width, ch)
        cur, g, hist, gh, lens = arrays
        m = ra.maps(rt, width, rows)["half+x"]
        p = rt.reproject_params(32, *ra.DEFAULTS)
        want, want_len = reference(("front", ch), cur, g, hist, gh, lens, m, p)
        tens = [torch.from_numpy(a).to(dev) for a in arrays]
        out, lo = bare.reproject(*tens, width, rows, m, p)                            # torch's current (default) stream
        assert out.dtype == torch.float32 and tuple(out.shape) == want.shape and lo.dtype == torch.uint8 and tuple(lo.shape) == (rows, width)
        assert same(out.cpu().numpy(), want) and np.array_equal(lo.cpu().numpy(), want_len)
        st = torch.cuda.Stream(device=dev)
        guard = gd.GUARD
        canary = torch.full((want.size + 2 * guard,), 3.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            view = canary[guard:guard + want.size]
            back, _ = bare.reproject(*tens, width, rows, m, p, out=view)
        st.synchronize()
        assert back is view and same(view.cpu().numpy().reshape(want.shape), want)
        assert (canary[:guard] == 3.0).all() and (canary[-guard:] == 3.0).all()
        for t, a in zip(tens, arrays):
            assert np.array_equal(t.cpu().numpy(), a, equal_nan=True)
        bufs = [rt.hipmem.DeviceBuffer(max(16, a.nbytes)).from_numpy(a) for a in arrays]
        b_out, b_lo = rt.hipmem.DeviceBuffer(want.nbytes), rt.hipmem.DeviceBuffer(max(16, width * rows))
        res = bare.reproject(*bufs, width, rows, m, p, out=b_out, len_out=b_lo)       # channels from the buffer's size
        assert res[0] is b_out and res[1] is b_lo
        bare.synchronize()
        assert same(b_out.to_numpy(F, want.shape), want) and np.array_equal(b_lo.to_numpy(np.uint8, (rows, width)), want_len)
        fresh, fresh_len = bare.reproject(*bufs, width, rows, m, p, channels=ch)
        bare.synchronize()
        assert same(fresh.to_numpy(F, want.shape), want) and np.array_equal(fresh_len.to_numpy(np.uint8, (rows, width)), want_len)
        with pytest.raises(ValueError):
            bare.reproject(tens[0], tens[1][:-1], *tens[2:], width, rows, m, p)
        with pytest.raises(ValueError):
            bare.reproject(tens[0].double(), *tens[1:], width, rows, m, p)
        with pytest.raises(ValueError):
            bare.reproject(*bufs, width, rows, m, p, out=rt.hipmem.DeviceBuffer(16))
        with pytest.raises(ValueError):
            bare.reproject(*tens, width, rows, m, p, len_out=b_lo)
        with pytest.raises(rt.capi.RtError, match="max_history"):
            bare.reproject(*tens, width, rows, m, rt.reproject_params(0))
        with pytest.raises(rt.capi.RtError, match="overlaps"):
            bare.reproject(*tens, width, rows, m, p, out=tens[2])                     # the output on the history: ping-pong instead
        for b in bufs + [b_out, b_lo, fresh, fresh_len]:
            b.free()


def by_hand(rt, fs, W, H, first, count):
    """the frame and the buffers of fs.camera under fs's settings with the passes (first, count), downloaded"""
    cam = fs._frame_settings(W, H)
    fs.ctx.set_passes(first, count)
    p, L = rt.make_params(W, H, fs.max_depth), fs._lights()
    rgb = np.empty((H, W, 3), F)
    rt.capi.check(fs.ctx.lib, fs.ctx.handle, fs.ctx.lib.rt_render(fs.ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(rgb.ctypes.data), None,
                                                                   C.byref(fs.stats)), "rt_render")
    buf = rt.hipmem.DeviceBuffer(W * H * 8 * 4)
    try:
        fs.ctx.gbuffer(cam, W, H, out=buf)
        fs.ctx.synchronize()
        return rgb, buf.to_numpy(F, (H, W, 8))
    finally:
        buf.free()
        fs.ctx.set_passes(0, count)


def test_flyscene_temporal_over_a_path_equals_the_chain_by_hand(rt, scenes):
    import denoise_ref as dr
    W, H = 72, 40
    yaws = (0.40, 0.42, 0.44, 0.46)
    fs = rt.Flyscene(scene_path=os.path.join(scenes, "dodgeColorTest.obj"))
    fs.initialize(W, H, True, False)
    try:
        fs.usteps = fs.vsteps = 2
        fs.max_depth, fs.supersample, fs.passes = 1, 2, 2
        assert fs.temporal is None and fs.history_lengths() is None
        p = rt.reproject_params()
        acc = ln = g_prev = None
        for k, yaw in enumerate(yaws):
            fs.camera = rt.default_camera(W, H, yaw)
            rgb, g = by_hand(rt, fs, W, H, 2 * k, 2)
            if k == 0:
                acc, ln = rgb, np.ones((H, W), np.uint8)
                plain = fs.raytraceScene(W, H, write_ppm=False).copy()
                assert same(plain, rgb), "the first frame is itself: passes (0, 2)"
            else:
                m = rt.reproject_map(fs.camera, rt.default_camera(W, H, yaws[k - 1]))
                acc, ln = rr.reproject(rgb, g, acc, g_prev, ln, m, ref_params(p))
            g_prev = g
            fs.temporal = p
            if k == 3:
                fs.denoise = rt.denoise_params(2)
            got = fs.raytraceScene(W, H, write_ppm=False)
            want = acc if k < 3 else dr.denoise(acc, g, gd.ref_params(fs.denoise))
            assert same(got, want), (k, differing(got, want))
            assert np.array_equal(fs.history_lengths(), ln), k
            fs.temporal = None
        assert ln.max() == 4 and not same(acc, rgb)
        fs.denoise = None
        fs.temporal = p
        with pytest.raises(ValueError):
            fs.raytraceScene(W, H, write_ppm=False, want_hits=True)
        fs.upsample = rt.upsample_params(2)
        with pytest.raises(ValueError):
            fs.raytraceScene(W, H, write_ppm=False)
        fs.upsample = None
        fs.reset_history()
        assert fs.history_lengths() is None
        first, _ = by_hand(rt, fs, W, H, 0, 2)
        assert same(fs.raytraceScene(W, H, write_ppm=False), first) and (fs.history_lengths() == 1).all(), "after a reset the frame is itself"
        small = fs.raytraceScene(36, 20, write_ppm=False)                      # another size drops the history
        assert small.shape == (20, 36, 3) and (fs.history_lengths() == 1).all() and fs.history_lengths().shape == (20, 36)
        fs.temporal = None
        fs.reset_history()
        fs.camera = rt.default_camera(W, H, yaws[0])
        assert same(fs.raytraceScene(W, H, write_ppm=False), plain), "unset is today's frame"
    finally:
        fs.reset_history()
        fs.ctx.close()
        fs.scene.close()


def test_flyscene_occlusion_accumulates_over_a_path(rt, world):
    W, H = 64, 40
    yaws = (0.40, 0.42, 0.44)
    fs = rt.Flyscene(scene_path=world["mixed"].path)
    fs.initialize(W, H, True, False)
    try:
        p = rt.reproject_params()
        acc = ln = g_prev = None
        for k, yaw in enumerate(yaws):
            fs.camera = rt.default_camera(W, H, yaw)
            ao = fs.ambient_occlusion(W, H, 2, 0.5, seed=3 + k)
            fs.supersample, fs.passes = 1, 1
            g = fs.gbuffer(W, H)
            if k == 0:
                acc, ln = ao, np.ones((H, W), np.uint8)
            else:
                acc, ln = rr.reproject(ao, g, acc, g_prev, ln, rt.reproject_map(fs.camera, rt.default_camera(W, H, yaws[k - 1])), ref_params(p))
            g_prev = g
            got = fs.ambient_occlusion(W, H, 2, 0.5, seed=3, temporal=p)
            assert same(got, acc), (k, differing(got, acc))
            assert np.array_equal(fs.history_lengths(), ln)
        assert ln.max() == 3 and not same(acc, ao)
        with pytest.raises(ValueError):
            fs.ambient_occlusion(W, H, 2, 0.5, temporal=p, upsample=rt.upsample_params(2))
        fs.reset_history()
        assert same(fs.ambient_occlusion(W, H, 2, 0.5, seed=5, temporal=p), fs.ambient_occlusion(W, H, 2, 0.5, seed=5)), "the first frame is itself"
    finally:
        fs.reset_history()
        fs.ctx.close()
        fs.scene.close()


def test_the_cli_against_the_python_chain(rt, scenes, tmp_path):
    """rt_render --temporal K DYAW: K frames, the last at the default camera and frame j at yaw -(float)(K - 1 - j) * DYAW, through the C++
    Flyscene::setTemporal -- the same image file as Flyscene.temporal over the same path, with and without --denoise and explicit parameters"""
    import subprocess
    RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")
    W, H, K, DYAW = 72, 40, 3, 0.02
    path = os.path.join(scenes, "dodgeColorTest.obj")
    yaws = [float(F(-(K - 1 - j)) * F(DYAW)) for j in range(K)]
    assert yaws[-1] == 0.0 and yaws[0] < yaws[1] < 0.0
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(W, H, True, False)
    try:
        fs.usteps = fs.vsteps = 2
        fs.max_depth, fs.supersample, fs.passes = 1, 2, 2
        fs.camera = rt.default_camera(W, H)
        fs.output_path = str(tmp_path / "plain_python.ppm")
        fs.raytraceScene(W, H, write_ppm=True)
        for name, dn in (("python.ppm", None), ("python_dn.ppm", rt.denoise_params(2, 1.0, 0.5, 0.125, 0.25))):
            fs.reset_history()
            fs.temporal, fs.denoise = rt.reproject_params(), dn
            fs.output_path = str(tmp_path / name)
            for j, yaw in enumerate(yaws):
                fs.camera = rt.default_camera(W, H, yaw)
                fs.raytraceScene(W, H, write_ppm=j == K - 1)
            assert fs.history_lengths().max() == K
    finally:
        fs.reset_history()
        fs.ctx.close()
        fs.scene.close()
    cli = ["--scene", path, "--size", str(W), str(H), "--samples", "2", "2", "--depth", "1", "--aa", "2", "--passes", "2"]

    def run(extra, out):
        return subprocess.run([RT_RENDER] + cli + extra + (["--out", out] if out else []), input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=240)

    data = lambda name: open(str(tmp_path / name), "rb").read()
    r = run(["--temporal", str(K), str(DYAW)], "cli.ppm")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert data("cli.ppm") == data("python.ppm") and data("cli.ppm") != data("plain_python.ppm")
    r = run(["--temporal", str(K), str(DYAW), "32", "2.0", "0.015625", "0.25"], "cli_params.ppm")
    assert r.returncode == 0 and data("cli_params.ppm") == data("python.ppm")
    r = run(["--temporal", str(K), str(DYAW), "--denoise", "2", "1.0", "0.5", "0.125", "0.25"], "cli_dn.ppm")
    assert r.returncode == 0 and data("cli_dn.ppm") == data("python_dn.ppm") and data("cli_dn.ppm") != data("cli.ppm")
    r = run(["--temporal", "1", str(DYAW)], "cli_one.ppm")
    assert r.returncode == 0 and data("cli_one.ppm") == data("plain_python.ppm"), "one frame is itself"
    for bad in (["--temporal", "0", "0.02"], ["--temporal", "3", "nan"], ["--temporal", "3", "0.02", "32"], ["--temporal", "3", "0.02", "0", "2", "1", "1"],
                ["--temporal", "3", "0.02", "256", "2", "1", "1"], ["--temporal", "3", "0.02", "32", "2", "-1", "1"],
                ["--pass-tolerance", "0.01", "--temporal", "3", "0.02"], ["--upsample", "2", "--temporal", "3", "0.02"]):
        r = run(bad, None)
        assert r.returncode == 2 and b"--temporal" in r.stderr, bad


def test_counting_build_gives_the_same_bits(rt):
    lib = rt.capi.load_library(WORK_LIB)
    ctx = C.c_void_p()
    assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
    try:
        for ch in (1, 3):
            cur, g, hist, gh, lens = synthetic(21, 37, ch)
            m = ra.maps(rt, 37, 21)["half+x"]
            p = rt.reproject_params(32, *ra.DEFAULTS)
            want, want_len = reference(("front", ch), cur, g, hist, gh, lens, m, p)
            got, lo = device_call(rt, lib, ctx, cur, g, hist, gh, lens, m, p)
            assert same(got, want) and np.array_equal(lo, want_len)
            out, l2 = np.zeros(want.shape, F), np.zeros((21, 37), np.uint8)
            vp = lambda a: C.c_void_p(a.ctypes.data)
            rt.capi.check(lib, ctx, lib.rt_reproject(ctx, vp(cur), ch, vp(g), vp(hist), vp(gh), vp(lens), 37, 21, c_map(m), C.byref(p), vp(out), vp(l2)),
                          "rt_reproject")
            assert same(out, want) and np.array_equal(l2, want_len)
    finally:
        lib.rt_destroy(ctx)
