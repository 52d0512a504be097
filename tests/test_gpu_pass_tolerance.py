"""Adaptive pass counts (rt_set_pass_tolerance, rt_pass_map) through every frame entry point.  Tolerance 0 wherever frames are compared.

The expectation of an adaptive-pass frame never comes from the adaptive code: the passes first .. first + count - 1 are rendered one by one
with rt_set_passes(p, 1) -- frames that tests/test_gpu_passes.py pins to the CPU oracle -- and folded by the numpy restatement of the rule
(tests/pass_tolerance_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pass_tolerance_ref as ptr
import switch_table
import test_gpu_lens as gl
import test_gpu_shutter as gs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCENES = os.path.join(HERE, "golden", "scenes")
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")
WORK_LIB = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")
F = np.float32
AP = 0.08
bits_equal, diff, quantise_u8, counters = gl.bits_equal, gl.diff, gl.quantise_u8, gl.counters
open_ctx, render, render_device, area_lights = gl.open_ctx, gl.render, gl.render_device, gl.area_lights
shutter_pair = gs.shutter_pair
SUMMED = gl.COUNTERS + ("pixels", "launches_total", "launches_trace", "launches_shadow", "launches_shade")


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def summed(st):
    return {k: int(getattr(st, k)) for k in SUMMED}


def lights5(rt):
    return rt.make_lights(points=gl.THREE[:1], area=True, usteps=5, vsteps=5)


def set_frame(ctx, n=1, lens=None, close=None, passes=(0, 1), tol=(-1.0, 8), tau=-1.0):
    ctx.set_supersampling(n)
    ctx.set_supersampling_threshold(tau)
    ctx.set_lens(*(lens or (0.0, 2.0)))
    ctx.set_shutter(close)
    ctx.set_passes(*passes)
    ctx.set_pass_tolerance(*tol)


def single_passes(rt, ctx, cam, L, w, h, n, lens, close, passes, depth=4):
    """{p: F_p}: every pass rendered on its own, as the one-pass frame rt_set_passes(p, 1)"""
    out = {}
    for p in passes:
        set_frame(ctx, n, lens, close, (p, 1))
        out[p], _ = render_device(rt, ctx, cam, L, w, h, depth)
    return out


# ------------------------------------------------------------------------------------------ 1. off is off
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_off_is_the_passes_frame_launch_for_launch(rt, name):
    w, h = 128, 80
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "yaw", 0.3)
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))

    def frames():
        out = []
        for n, lens, close, passes in ((1, None, None, (0, 8)), (2, (AP, 1.8), b, (3, 5)), (3, None, None, (0, 1)), (1, None, b, (2, 4))):
            ctx.set_supersampling(n); ctx.set_lens(*(lens or (0.0, 2.0))); ctx.set_shutter(close); ctx.set_passes(*passes)
            rgb, _, st = render(rt, ctx, a, L, w, h, 4)
            st2 = rt.capi.rt_stats()
            rgb2, u8 = render_device(rt, ctx, a, L, w, h, 4, stats=st2)
            assert bits_equal(rgb, rgb2)
            out.append((rgb, u8, summed(st), int(st2.launches_total)))
        return out

    never = frames()                             # the default: tol = -1, min_passes = 8
    ctx.set_pass_tolerance(-1.0, 2)
    negative = frames()
    ctx.set_pass_tolerance(0.01, 8)              # count <= min_passes in every frame above
    short = frames()
    set_frame(ctx, 1, passes=(0, 8), tol=(0.01, 4))
    _, _, st_on = render(rt, ctx, a, L, w, h, 4)
    assert (ctx.pass_map(w, h) < 8).any()
    ctx.set_pass_tolerance(-0.5, 4)
    back = frames()
    ctx.close(); hs.close()
    assert int(st_on.pixels) < never[0][2]["pixels"], "the feature must have been on in between"
    for other in (negative, short, back):
        for x, y in zip(never, other):
            assert bits_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] and x[3] == y[3]


# ------------------------------------------------------------------------------------------ 2. the definition
CASES = {
    "cube-n1-pinhole": ("cube.obj", 1, False, False),
    "cube-n2-lens-shutter": ("cube.obj", 2, True, True),
    "dodge-n1-shutter": ("dodgeColorTest.obj", 1, False, True),
    "dodge-n3-pinhole": ("dodgeColorTest.obj", 3, False, False),          # 8 x 8 tiles of sub-samples straddle the pixels
}
# the two frames whose passes the CPU oracle also renders and folds (tests/test_pass_tolerance_api.py): pixels that stopped at min_passes, in
# between, and that ran every pass.  64 x 40, yaw 0.2, 5 x 5 area light, depth 4, passes 0 .. 15, min 4.
CUBE_PINHOLE = ("cube-n1-pinhole", 64, 0, 16, 0.004, 4)
CUBE_PINHOLE_CLASSES = (2478, 16, 66)
DODGE_PINHOLE_CLASSES = (2449, 34, 77)                                      # dodge n = 1 pinhole, tol 0.02


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(64, 40), (61, 37)])
@pytest.mark.parametrize("case", list(CASES))
def test_frame_is_the_rule_folded_over_its_single_passes(rt, case, size):
    name, n, lens_on, shutter_on = CASES[case]
    w, h = size
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = lights5(rt)
    a, b = shutter_pair(rt, w, h, "yaw", 0.2)
    lens, close = ((AP, 1.8) if lens_on else None), (b if shutter_on else None)
    oracle_checked = False
    try:
        single = single_passes(rt, ctx, a, L, w, h, n, lens, close, range(16))
        for first, count in ((0, 16), (3, 12)):
            frames = [single[p] for p in range(first, first + count)]
            for tol, m in ((0.004, 4), (0.02, 4), (0.02, 2)):
                want, taken = ptr.fold_adaptive(frames, tol, m)
                cls = ptr.classes(taken, m, count)
                print(f"{case} {w}x{h} ({first}, {count}) tol {tol} min {m}: stopped at min / in between / ran all = {cls}, mean {taken.mean():.2f}")
                assert (taken < count).any(), "a case in which no pixel stops early checks nothing"
                set_frame(ctx, n, lens, close, (first, count), (tol, m))
                st = rt.capi.rt_stats()
                rgb, u8 = render_device(rt, ctx, a, L, w, h, 4, stats=st)
                got_map = ctx.pass_map(w, h)
                key = (first, count, tol, m)
                assert np.array_equal(got_map, taken), (key, int((got_map != taken).sum()))
                assert bits_equal(rgb, want), (key, diff(rgb, want), float(np.abs(rgb - want).max()))
                assert np.array_equal(u8, quantise_u8(want)), key
                assert int(st.pixels) == n * n * int(taken.astype(np.int64).sum()), key
                host, _, st_h = render(rt, ctx, a, L, w, h, 4)
                assert bits_equal(host, rgb), (key, "rt_render")
                assert np.array_equal(ctx.pass_map(w, h), taken) and int(st_h.pixels) == int(st.pixels)
                if (case, w, first, count, tol, m) == CUBE_PINHOLE:
                    assert min(cls) > 0 and cls == CUBE_PINHOLE_CLASSES, (key, cls, "all three classes, in the oracle's counts")
                    oracle_checked = True
    finally:
        ctx.close(); hs.close()
    assert oracle_checked == ((case, w) == CUBE_PINHOLE[:2]), "the loops above must contain the frame the oracle counted"


@pytest.mark.gpu
def test_dodge_pinhole_shows_the_oracle_classes(rt):
    w, h, m, count, tol = 64, 40, 4, 16, 0.02
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "dodgeColorTest.obj"))
    L, cam = lights5(rt), rt.default_camera(w, h, 0.2)
    single = single_passes(rt, ctx, cam, L, w, h, 1, None, None, range(count))
    want, taken = ptr.fold_adaptive([single[p] for p in range(count)], tol, m)
    set_frame(ctx, 1, passes=(0, count), tol=(tol, m))
    rgb, u8 = render_device(rt, ctx, cam, L, w, h, 4)
    got = ctx.pass_map(w, h)
    ctx.close(); hs.close()
    assert ptr.classes(taken, m, count) == DODGE_PINHOLE_CLASSES
    assert np.array_equal(got, taken) and bits_equal(rgb, want) and np.array_equal(u8, quantise_u8(want))


# ------------------------------------------------------------------------------------------ 3. tol = +inf
@pytest.mark.gpu
@pytest.mark.parametrize("name,n", [("cube.obj", 2), ("dodgeColorTest.obj", 1)])
def test_infinite_tolerance_is_the_min_passes_frame(rt, name, n):
    w, h, first, count, m = 96, 61, 2, 9, 3
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "both", 0.2)
    set_frame(ctx, n, (AP, 1.8), b, (first, m))
    want, _, st0 = render(rt, ctx, a, L, w, h, 4)
    _, want8 = render_device(rt, ctx, a, L, w, h, 4)
    set_frame(ctx, n, (AP, 1.8), b, (first, count), (float("inf"), m))
    rgb, _, st1 = render(rt, ctx, a, L, w, h, 4)
    got_map = ctx.pass_map(w, h)
    _, u8 = render_device(rt, ctx, a, L, w, h, 4)
    ctx.close(); hs.close()
    assert bits_equal(rgb, want) and np.array_equal(u8, want8)
    assert (got_map == m).all()
    assert counters(st1) == counters(st0) and int(st1.pixels) == int(st0.pixels) == m * n * n * w * h
    assert int(st1.launches_total) > int(st0.launches_total), "the later passes still launch, over empty lists"


# ------------------------------------------------------------------------------------------ 4. shards, row ranges, the gather
@pytest.mark.gpu
def test_shards_row_ranges_and_the_gather_equal_the_full_frame(rt):
    import torch
    w, h, n = 256, 157, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "both", 0.3)
    set_frame(ctx, n, (AP, 1.8), b, (2, 6), (0.01, 3))
    full, full8 = render_device(rt, ctx, a, L, w, h, 4)
    full_map = ctx.pass_map(w, h)
    assert 3 <= int(full_map.min()) and (full_map == 3).any() and (full_map > 3).any()
    for stripe in (8, 1, 5):
        for nranks in (2, 3):
            for rank in range(nranks):
                ys = [y for y in range(h) if (y // stripe) % nranks == rank]
                rgb, u8 = render_device(rt, ctx, a, L, w, h, 4, stripe=stripe, rank=rank, nranks=nranks)
                assert bits_equal(rgb, full[ys]), (stripe, nranks, rank, diff(rgb, full[ys]))
                assert np.array_equal(u8, full8[ys])
                assert np.array_equal(ctx.pass_map(w, len(ys)), full_map[ys]), (stripe, nranks, rank)
    rgb, u8 = render_device(rt, ctx, a, L, w, h, 4, row0=5, row1=h - 3)
    assert bits_equal(rgb, full[5:h - 3]) and np.array_equal(u8, full8[5:h - 3])
    assert np.array_equal(ctx.pass_map(w, h - 8), full_map[5:h - 3])
    stripe = 8
    p = rt.make_params(w, h, 4, 0, h, stripe, 0, 1)
    comm = rt.shard.Comm(0, rt.shard.Comm.unique_id(), 1, 0)
    local = torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda")
    gathered = torch.zeros_like(local)
    torch.cuda.synchronize()
    st = ctx.lib.rt_render_gather(ctx.handle, comm.handle, C.byref(a), C.byref(L), C.byref(p), C.c_void_p(local.data_ptr()), local.numel(),
                                  C.c_void_p(gathered.data_ptr()), 0, None)
    rt.capi.check(ctx.lib, ctx.handle, st, "rt_render_gather")
    torch.cuda.synchronize()
    frame = np.zeros(w * h * 3, np.uint8)
    g = gathered.cpu().numpy()
    assert ctx.lib.rt_stitch_rows(g.ctypes.data_as(C.c_void_p), local.numel(), w, h, stripe, 1, frame.ctypes.data_as(C.c_void_p)) == 0
    gather_map = ctx.pass_map(w, h)
    comm.close(); ctx.close(); hs.close()
    assert np.array_equal(frame, full8.reshape(-1)) and np.array_equal(gather_map, full_map)


# ------------------------------------------------------------------------------------------ 5. graphs
@pytest.mark.gpu
@pytest.mark.parametrize("name,shutter", [("cube.obj", True), ("dodgeColorTest.obj", False)])
def test_graph_replays_the_adaptive_frame_and_keeps_its_setting(rt, name, shutter):
    w, h, n, passes, tol = 160, 100, 2, (1, 10), (0.01, 3)
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    pairs = [shutter_pair(rt, w, h, "yaw", 0.0), shutter_pair(rt, w, h, "both", 0.3), shutter_pair(rt, w, h, "move", -0.5)]
    order = [0, 1, 1, 2]                       # the same camera twice in a row: a replay must not see the state of the one before
    set_frame(ctx, n, None, pairs[0][1] if shutter else None, passes, tol)
    out, out8 = rt.hipmem.DeviceBuffer(h * w * 3 * 4), rt.hipmem.DeviceBuffer(h * w * 3)
    g = rt.FrameGraph(ctx, L, rt.make_params(w, h, 4), out.address, out8.address)
    got = []
    for k, i in enumerate(order):
        if k == 1:
            ctx.set_pass_tolerance(-1.0, 8)                   # the graph keeps the setting it was captured with
        a, b = pairs[i]
        g.launch(a, close=b if shutter else None)
        pixels = int(g.stats().pixels)                        # (synchronises)
        got.append((out.to_numpy(F, (h, w, 3)), out8.to_numpy(np.uint8, (h, w, 3)), pixels))
    g.close()
    set_frame(ctx, n, None, pairs[1][1] if shutter else None, passes)
    st_off = rt.capi.rt_stats()
    render_device(rt, ctx, pairs[1][0], L, w, h, 4, stats=st_off)         # the context itself is back at "off"
    assert int(st_off.pixels) == passes[1] * n * n * w * h
    for i, (rgb, u8, pixels) in zip(order, got):
        a, b = pairs[i]
        set_frame(ctx, n, None, b if shutter else None, passes, tol)
        want, want8 = render_device(rt, ctx, a, L, w, h, 4)
        taken = ctx.pass_map(w, h)
        assert (taken < passes[1]).any() and (taken > tol[1]).any()
        assert bits_equal(rgb, want), (i, diff(rgb, want))
        assert np.array_equal(u8, want8)
        assert pixels == n * n * int(taken.astype(np.int64).sum()), i
    assert not bits_equal(got[0][0], got[1][0]) and bits_equal(got[1][0], got[2][0])
    ctx.close(); hs.close(); out.free(); out8.free()


# ------------------------------------------------------------------------------------------ 6. interleaving on one context
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_interleaved_frames_equal_those_of_a_fresh_context(rt, name):
    """the adaptive-pass frame, the plain passes frame and the adaptive supersampling frame share the tile list, its counters and the refine bytes"""
    w, h, n = 128, 80, 2
    L = area_lights(rt)
    cam = rt.default_camera(w, h, 0.2)
    kinds = {
        "passes-adaptive": dict(passes=(0, 10), tol=(0.01, 3)),
        "plain": dict(passes=(0, 4)),
        "aa-adaptive": dict(passes=(0, 1), tau=0.05),
    }

    def one(ctx, kind):
        set_frame(ctx, n, **kinds[kind])
        rgb, _, st = render(rt, ctx, cam, L, w, h, 4)
        return rgb, summed(st), (ctx.pass_map(w, h) if kind == "passes-adaptive" else ctx.supersampling_refined())

    fresh = {}
    for kind in kinds:
        hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
        fresh[kind] = one(ctx, kind)
        ctx.close(); hs.close()
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    try:
        for kind in ("passes-adaptive", "plain", "aa-adaptive", "passes-adaptive", "aa-adaptive", "plain"):
            rgb, st, extra = one(ctx, kind)
            want, want_st, want_extra = fresh[kind]
            assert bits_equal(rgb, want), (kind, diff(rgb, want))
            assert st == want_st, kind
            assert np.array_equal(extra, want_extra), kind
    finally:
        ctx.close(); hs.close()
    assert 0 < fresh["aa-adaptive"][2] < w * h and (fresh["passes-adaptive"][2] < 10).any()


# ------------------------------------------------------------------------------------------ 7. statistics
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_stats_lie_between_the_short_and_the_full_frame(rt, name):
    w, h, n, first, count, m, tol = 128, 80, 2, 1, 10, 3, 0.01
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "yaw")
    set_frame(ctx, n, None, b, (first, m))
    _, _, lo = render(rt, ctx, a, L, w, h, 4)
    set_frame(ctx, n, None, b, (first, count))
    _, _, hi = render(rt, ctx, a, L, w, h, 4)
    set_frame(ctx, n, None, b, (first, count), (tol, m))
    base, _, st = render(rt, ctx, a, L, w, h, 4)
    taken = ctx.pass_map(w, h)
    assert (taken == m).any() and (taken == count).any()
    for k in gl.COUNTERS + ("pixels",):
        print(f"{name} {k}: {int(getattr(lo, k))} <= {int(getattr(st, k))} <= {int(getattr(hi, k))}")
        assert int(getattr(lo, k)) <= int(getattr(st, k)) <= int(getattr(hi, k)), k
    assert int(lo.rays_primary) < int(st.rays_primary) < int(hi.rays_primary)
    assert int(st.pixels) == n * n * int(taken.astype(np.int64).sum()) and st.ms_total > 0 and st.ms_resolve > 0
    assert int(st.launches_trace) == int(hi.launches_trace), "every pass launches"
    p = rt.make_params(w, h, 4, collect_stats=True)
    counted, _, st1 = render(rt, ctx, a, L, w, h, 4, p=p)
    assert bits_equal(counted, base) and summed(st1) == summed(st) and int(st1.box_tests) > 0
    assert np.array_equal(ctx.pass_map(w, h), taken)
    lib = ctx.lib
    lib.rt_timing_collect(ctx.handle, C.byref(rt.capi.rt_stats()))
    p.collect_stats = 2
    for _ in range(3):
        last, _, _ = render(rt, ctx, a, L, w, h, 4, p=p)
    assert bits_equal(last, base)
    tim = rt.capi.rt_stats()
    rt.capi.check(lib, ctx.handle, lib.rt_timing_collect(ctx.handle, C.byref(tim)), "rt_timing_collect")
    assert tim.ms_total > 0 and int(tim.pixels) == int(st.pixels) and int(tim.launches_total) == int(st.launches_total)
    assert int(tim.launches_trace) == 3 * int(st.launches_trace), "one pending event set per pass and frame"
    for k in gl.COUNTERS:
        assert int(getattr(tim, k)) == int(getattr(st, k)), k
    ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 8. it saves rays and keeps the error
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_adaptive_frame_saves_rays_within_its_tolerance(rt, name):
    """E_x: whole-frame RMS error against R = passes (128, 128), in float64.  The rule stops a pixel when its estimated standard error is at most
    tol, so E_ad <= sqrt(E_full^2 + tol^2) is the bound it promises.  The CPU oracle gives for these inputs: cube 9.2 passes per pixel, E_ad
    0.00090, E_full 0.00054, E_min 0.00129; dodgeColorTest 10.5 passes, 0.0050, 0.0032, 0.0116."""
    w, h, count, m, tol = 64, 40, 64, 8, 0.01
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L, cam = lights5(rt), rt.default_camera(w, h, 0.2)
    frames = {}
    for key, passes, t in (("R", (128, 128), (-1.0, 8)), ("full", (0, count), (-1.0, 8)), ("min", (0, m), (-1.0, 8)), ("ad", (0, count), (tol, m))):
        set_frame(ctx, 1, passes=passes, tol=t)
        frames[key], _ = render_device(rt, ctx, cam, L, w, h, 4)
    taken = ctx.pass_map(w, h)
    ctx.close(); hs.close()
    R = frames["R"].astype(np.float64)
    e = {k: float(np.sqrt(((frames[k].astype(np.float64) - R) ** 2).mean())) for k in ("full", "min", "ad")}
    mean = float(taken.mean())
    print(f"{name}: mean passes {mean:.2f} of {count}; E_ad {e['ad']:.6f}, E_full {e['full']:.6f}, E_min {e['min']:.6f}, bound {np.hypot(e['full'], tol):.6f}")
    assert e["ad"] <= float(np.hypot(e["full"], tol))
    assert e["ad"] < e["min"]
    assert mean <= 0.25 * count


# ------------------------------------------------------------------------------------------ 9. the counting build
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_counting_build_renders_the_adaptive_frame(rt, name):
    assert os.path.exists(WORK_LIB), "the counting build is part of `make all`"
    hs = rt.HostScene(os.path.join(SCENES, name), 1000, 15)
    w, h, n = 96, 64, 2
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "both")
    frames = []
    for lib in (rt.load_library(), rt.capi.load_library(WORK_LIB)):
        ctx = C.c_void_p()
        assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
        try:
            rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(hs.view)), "rt_upload_scene")
            rt.capi.check(lib, ctx, lib.rt_set_supersampling(ctx, n), "rt_set_supersampling")
            rt.capi.check(lib, ctx, lib.rt_set_shutter(ctx, C.byref(b)), "rt_set_shutter")
            rt.capi.check(lib, ctx, lib.rt_set_passes(ctx, 0, 8), "rt_set_passes")
            rt.capi.check(lib, ctx, lib.rt_set_pass_tolerance(ctx, 0.01, 3), "rt_set_pass_tolerance")
            p = rt.make_params(w, h, 4)
            rgb = np.full((h, w, 3), np.nan, F)
            st = rt.capi.rt_stats()
            rt.capi.check(lib, ctx, lib.rt_render(ctx, C.byref(a), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), None, C.byref(st)), "rt_render")
            taken = np.zeros((h, w), np.uint16)
            rt.capi.check(lib, ctx, lib.rt_pass_map(ctx, taken.ctypes.data_as(C.c_void_p), taken.size), "rt_pass_map")
            frames.append((rgb, summed(st), taken))
        finally:
            lib.rt_destroy(ctx)
    hs.close()
    assert bits_equal(frames[1][0], frames[0][0])
    assert frames[1][1] == frames[0][1] and np.array_equal(frames[1][2], frames[0][2])
    assert (frames[0][2] < 8).any() and (frames[0][2] > 3).any()


# ------------------------------------------------------------------------------------------ 10. the front ends
@pytest.mark.gpu
def test_python_flyscene_and_cli_write_the_adaptive_frame(rt, tmp_path):
    path, w, h, n = os.path.join(SCENES, "cube.obj"), 64, 64, 2
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(w, h, True, False)
    fs.supersample = n
    fs.passes = 16
    fs.pass_tolerance, fs.pass_min = 0.01, 4
    fs.output_path = str(tmp_path / "py.ppm")
    rgb = fs.raytraceScene()
    taken = fs.ctx.pass_map(w, h)
    pixels = int(fs.stats.pixels)
    with pytest.raises(ValueError):
        fs.raytraceScene(write_ppm=False, want_hits=True)
    fs.pass_tolerance = -1.0
    fs.raytraceScene(write_ppm=False)
    full_pixels = int(fs.stats.pixels)
    fs.ctx.close(); fs.scene.close()
    assert (taken == 4).any() and (taken > 4).any() and pixels == n * n * int(taken.astype(np.int64).sum())
    assert full_pixels == 16 * n * n * w * h and rgb.shape == (h, w, 3)
    r = subprocess.run([RT_RENDER, "--scene", path, "--aa", str(n), "--passes", "16", "--pass-tolerance", "0.01", "4", "--size", str(w), str(h),
                        "--out", str(tmp_path / "cli.ppm")], input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert (tmp_path / "cli.ppm").read_bytes() == (tmp_path / "py.ppm").read_bytes()
    assert f"mean passes per pixel {taken.mean():.2f}".encode() in r.stdout, r.stdout


# ------------------------------------------------------------------------------------------ 11. rejections
@pytest.mark.gpu
def test_rejections_keep_the_setting_and_the_frame(rt):
    import torch
    w, h = 96, 64
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    lib, c = ctx.lib, rt.capi
    L = area_lights(rt)
    cam = rt.default_camera(w, h, 0.2)
    vptr = lambda x: x.ctypes.data_as(C.c_void_p)
    out = np.full((h, w), 9, np.uint16)
    # the default needs no frame: nothing to map yet
    assert lib.rt_pass_map(ctx.handle, vptr(out), out.size) == c.RT_ERR_INVALID and b"rt_pass_map" in lib.rt_last_error(ctx.handle)
    set_frame(ctx, 1, passes=(0, 8), tol=(0.01, 3))
    want, _, _ = render(rt, ctx, cam, L, w, h, 4)
    want_map = ctx.pass_map(w, h)
    assert (want_map < 8).any()
    for tol, m in ((float("nan"), 3), (0.5, 1), (0.5, 0), (0.5, -3), (0.5, 257), (float("nan"), 300)):
        assert lib.rt_set_pass_tolerance(ctx.handle, tol, m) == c.RT_ERR_INVALID, (tol, m)
        assert b"rt_set_pass_tolerance" in lib.rt_last_error(ctx.handle)
        got, _, _ = render(rt, ctx, cam, L, w, h, 4)
        assert bits_equal(got, want) and np.array_equal(ctx.pass_map(w, h), want_map), (tol, m)
    assert lib.rt_set_pass_tolerance(None, 0.5, 4) == c.RT_ERR_INVALID
    got, _, _ = render(rt, ctx, cam, L, w, h, 4)
    assert bits_equal(got, want)
    # a wrong size
    for npx in (0, w * h - 1, w * h + 1, w):
        assert lib.rt_pass_map(ctx.handle, vptr(out), npx) == c.RT_ERR_INVALID, npx
    assert (out == 9).all()
    assert lib.rt_pass_map(ctx.handle, vptr(out), out.size) == c.RT_OK and np.array_equal(out, want_map)
    # hit ids
    p = rt.make_params(w, h, 4)
    rgb, hit = np.full((h, w, 3), 3.0, F), np.full((h, w), -7, np.int32)
    assert lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), vptr(rgb), vptr(hit), None) == c.RT_ERR_INVALID
    d_rgb = torch.full((h, w, 3), 3.0, dtype=torch.float32, device="cuda")
    d_hit = torch.full((h, w), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(d_rgb.data_ptr()), None, C.c_void_p(d_hit.data_ptr()),
                                None, None) == c.RT_ERR_INVALID
    rt.capi.check(lib, ctx.handle, lib.rt_synchronize(ctx.handle), "rt_synchronize")
    torch.cuda.synchronize()
    assert (rgb == 3.0).all() and (hit == -7).all() and bool((d_rgb == 3.0).all()) and bool((d_hit == -7).all())
    # the adaptive supersampling threshold is ignored
    set_frame(ctx, 2, passes=(0, 8), tol=(0.01, 3))
    regular, _, st0 = render(rt, ctx, cam, L, w, h, 4)
    set_frame(ctx, 2, passes=(0, 8), tol=(0.01, 3), tau=0.05)
    ad, _, st1 = render(rt, ctx, cam, L, w, h, 4)
    assert bits_equal(ad, regular) and summed(st1) == summed(st0)
    # after a plain frame there is no map
    set_frame(ctx, 1, passes=(0, 8))
    render(rt, ctx, cam, L, w, h, 4)
    assert lib.rt_pass_map(ctx.handle, vptr(out), out.size) == c.RT_ERR_INVALID and b"rt_pass_map" in lib.rt_last_error(ctx.handle)
    # +inf and the limits are accepted
    for tol, m in ((float("inf"), 2), (0.0, 256), (-7.0, 2)):
        assert lib.rt_set_pass_tolerance(ctx.handle, tol, m) == c.RT_OK, (tol, m)
    ctx.close(); hs.close()
