"""Multi-pass accumulation (rt_set_passes) through every frame entry point.  Tolerance 0 wherever frames are compared.

A single pass is checked against frames that never come from the pass code: the CPU oracle's one-ray frames with the viewport shifted by the
offsets of rt_pass_offsets (lens and shutter off), or the rays of lens_ref / shutter_ref with the scrambles of tests/passes_ref.py, traced by
rt_trace_rays / rt_box_intersect (which ignore every frame setting).  The fold of several passes is checked against the float32 fold of the
individually rendered single-pass frames."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lens_ref
import passes_ref
import shutter_ref
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
bits_equal, diff, fold, quantise_u8, counters = gl.bits_equal, gl.diff, gl.fold, gl.quantise_u8, gl.counters
open_ctx, render, render_device, area_lights, lights_pair = gl.open_ctx, gl.render, gl.render_device, gl.area_lights, gl.lights_pair
copy_cam, shutter_pair = gs.copy_cam, gs.shutter_pair
# rt_stats fields that must sum exactly.  rays_sample_walked sums on the device like the others, but on the flat scene it is not a function of
# the frame alone: it counts the sample segments left over by k_beam's tile tests, and which 64 hits share a tile follows the order in which
# the trace kernel's waves appended them to the hit list.  Measured (256 x 160, n = 2, shutter on): dodge, the four passes sum to 4784256 and
# the (0, 4) frame has 4784256; cube, the same four single passes summed to 112768 in one session and to 113472 in another, the (0, 4) frame
# had 112640 both times.  No existing test compares the counter for equality either, so it is bounded instead.
SUMMED = gl.COUNTERS + ("pixels", "launches_total", "launches_trace", "launches_shadow", "launches_shade")


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def summed(st):
    return {k: int(getattr(st, k)) for k in SUMMED}


def set_frame(ctx, n=1, lens=None, close=None, passes=(0, 1), tau=-1.0):
    ctx.set_supersampling(n)
    ctx.set_supersampling_threshold(tau)
    ctx.set_lens(*(lens or (0.0, 2.0)))
    ctx.set_shutter(close)
    ctx.set_passes(*passes)


# ------------------------------------------------------------------------------------------ 1. off is off
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_default_passes_are_the_frame_it_was_launch_for_launch(rt, name):
    w, h = 200, 136
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "yaw", 0.3)
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))

    def frames():
        out = []
        for n in (1, 3):
            for lens in (None, (AP, 2.0)):
                for close in (None, b):
                    ctx.set_supersampling(n); ctx.set_lens(*(lens or (0.0, 2.0))); ctx.set_shutter(close)
                    rgb, hit, st = render(rt, ctx, a, L, w, h, 4, hits=(n == 1))
                    st2 = rt.capi.rt_stats()
                    rgb2, u8 = render_device(rt, ctx, a, L, w, h, 4, stats=st2)
                    assert bits_equal(rgb, rgb2)
                    out.append((rgb, u8, hit, dict(counters(st), pixels=int(st.pixels), launches=int(st.launches_total)), int(st2.launches_total)))
        return out

    never = frames()
    ctx.set_passes(0, 1)
    explicit = frames()
    ctx.set_passes(3, 5)
    ctx.set_supersampling(3); ctx.set_lens(0.0, 2.0); ctx.set_shutter(None)
    on, _ = render_device(rt, ctx, a, L, w, h, 4)
    ctx.set_passes(0, 1)
    back = frames()
    ctx.close(); hs.close()
    assert not bits_equal(on, never[4][0]), "passes (3, 5) must change the n = 3 frame"
    for other in (explicit, back):
        for x, y in zip(never, other):
            assert bits_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[3] == y[3] and x[4] == y[4]
            assert (x[2] is None and y[2] is None) or np.array_equal(x[2], y[2])


# ------------------------------------------------------------------------------------------ 2. a single pass against the oracle
def oracle_pass_frame(oracle, osc, oL, w, h, n, p, depth, yaw, ox, oy):
    """the definition's fold of the oracle's one-ray frames with viewport[0] = -ox[sx], viewport[1] = -oy[sy]; also the hit ids of (0, 0)"""
    subs, hits = np.zeros((h, w, n, n, 3), F), None
    for sy in range(n):
        for sx in range(n):
            cam = oracle.camera(w, h, yaw)
            cam.viewport[0], cam.viewport[1] = float(-ox[sx]), float(-oy[sy])      # (float)i - (-o) == (float)i + o
            rgb, hit, _ = osc.render(cam, oL, w, h, max_depth=depth, threads=8, want_hits=True)
            subs[:, :, sy, sx] = rgb
            hits = hit if hits is None else hits
    return (fold(subs, n) if n > 1 else subs[:, :, 0, 0].copy()), hits


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cube.obj", "dodgeColorTest.obj"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_single_pass_equals_the_oracle_with_shifted_viewports(rt, oracle, which, n):
    path = os.path.join(SCENES, which)
    hs, ctx = open_ctx(rt, path)
    osc = oracle.load_scene(path)
    w, h, depth, yaw = 40, 24, 4, 0.2
    L, oL = lights_pair(rt, oracle, "area5")
    cam = rt.default_camera(w, h, yaw)
    try:
        ctx.set_supersampling(n)
        base, _ = render_device(rt, ctx, cam, L, w, h, depth)
        for p in (1, 2, 7, 255):
            ox, oy = passes_ref.library_offsets(ctx.lib, n, p)
            want, want_hit = oracle_pass_frame(oracle, osc, oL, w, h, n, p, depth, yaw, ox, oy)
            ctx.set_passes(p, 1)
            st = rt.capi.rt_stats()
            rgb, u8 = render_device(rt, ctx, cam, L, w, h, depth, stats=st)
            print(f"{which} n={n} p={p}: differs from the oracle in {diff(rgb, want)} pixels, from pass 0 in {diff(rgb, base)}")
            assert bits_equal(rgb, want), (p, diff(rgb, want), float(np.abs(rgb - want).max()))
            assert np.array_equal(u8, quantise_u8(want)), p
            assert int(st.pixels) == n * n * w * h
            assert not bits_equal(rgb, base), "the shifted grid must change the frame"
            if n == 1:
                got, hit, _ = render(rt, ctx, cam, L, w, h, depth, hits=True)
                assert bits_equal(got, want) and np.array_equal(hit, want_hit), p
    finally:
        osc.close(); ctx.close(); hs.close()


@pytest.mark.gpu
def test_full_size_pass_equals_the_shifted_gpu_frames(rt):
    w, h, n, p = 1920, 1080, 2, 7
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    L = area_lights(rt)
    ox, oy = passes_ref.library_offsets(ctx.lib, n, p)
    subs = np.zeros((h, w, n, n, 3), F)
    for sy in range(n):
        for sx in range(n):
            cam = rt.default_camera(w, h)
            cam.viewport[0], cam.viewport[1] = float(-ox[sx]), float(-oy[sy])
            subs[:, :, sy, sx], _, _ = render(rt, ctx, cam, L, w, h, 4)
    want = fold(subs, n)
    set_frame(ctx, n, passes=(p, 1))
    rgb, u8 = render_device(rt, ctx, rt.default_camera(w, h), L, w, h, 4)
    ctx.close(); hs.close()
    assert bits_equal(rgb, want), (diff(rgb, want), float(np.abs(rgb - want).max()))
    assert np.array_equal(u8, quantise_u8(want))


# ------------------------------------------------------------------------------------------ 3. a single pass with the lens / the shutter
def raster_terms(rt, ctx, cam, w, h, n, ox, oy):
    """gs.raster_terms with the pass's own column and row offsets"""
    ident = copy_cam(cam)
    for k in range(12):
        ident.inv_view[k] = 1.0 if k in (0, 5, 10) else 0.0
    n0, n1 = np.zeros((h, w, n, n), F), np.zeros((h, w, n, n), F)
    for sy in range(n):
        for sx in range(n):
            ident.viewport[0], ident.viewport[1] = float(-ox[sx]), float(-oy[sy])
            pts = np.zeros((h, w, 3), F)
            rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_primary_points(ctx.handle, C.byref(ident), w, h, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
            n0[:, :, sy, sx], n1[:, :, sy, sx] = pts[..., 0], pts[..., 1]
    return n0, n1


def ref_pass_frame(rt, ctx, hs, a, b, L, w, h, n, p, depth, lens):
    """pass p by the definitions: raster offsets from rt_pass_offsets, h / g from passes_ref, rays from shutter_ref (close == open where the
    shutter is off: K(t) is then the open camera bit for bit), traced by rt_trace_rays behind rt_box_intersect on the root box.  The entry
    points used here ignore the context's frame settings."""
    lib = ctx.lib
    ox, oy = passes_ref.library_offsets(lib, n, p)
    n0, n1 = raster_terms(rt, ctx, a, w, h, n, ox, oy)
    full = None if lens is None else (lens[0], lens[1], lens_ref.library_table(lib, n))
    with passes_ref.pass_scrambles(p):
        O, P, D = shutter_ref.shutter_rays(n0, n1, shutter_ref.pose(a), shutter_ref.pose(b if b is not None else a), n, np.arange(h), lens=full)
    N = O.size // 3
    O, P, D = (np.ascontiguousarray(x.reshape(N, 3)) for x in (O, P, D))
    node0 = hs.view.nodes[0]
    boxes = np.ascontiguousarray(np.broadcast_to(np.array(list(node0.bmin) + list(node0.bmax), F), (N, 6)))
    pre = np.zeros(N, np.uint8)
    vptr = lambda x: x.ctypes.data_as(C.c_void_p)
    rt.capi.check(lib, ctx.handle, lib.rt_box_intersect(ctx.handle, N, vptr(boxes), vptr(O), vptr(P), vptr(pre)), "rt_box_intersect")
    col, face = np.zeros((N, 3), F), np.zeros(N, np.int32)
    rt.capi.check(lib, ctx.handle, lib.rt_trace_rays(ctx.handle, C.byref(L), depth, N, vptr(O), vptr(D), vptr(col), vptr(face), None), "rt_trace_rays")
    col[pre == 0] = 1.0
    face[pre == 0] = -1
    col = col.reshape(h, w, n, n, 3)
    return (fold(col, n) if n > 1 else col[:, :, 0, 0].copy()), int((pre == 0).sum()), face.reshape(h, w, n, n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
@pytest.mark.parametrize("mode", ["lens", "shutter", "both"])
def test_single_pass_with_lens_and_shutter_equals_the_reference_rays(rt, name, mode):
    w, h, depth = 96, 64, 4
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "both", 0.2)
    lens = (AP, 1.8) if mode in ("lens", "both") else None
    close = b if mode in ("shutter", "both") else None
    try:
        for n in (1, 2, 4):
            set_frame(ctx, n, lens, close)
            base, _ = render_device(rt, ctx, a, L, w, h, depth)
            for p in (1, 9):
                want, culled, face = ref_pass_frame(rt, ctx, hs, a, close, L, w, h, n, p, depth, lens)
                set_frame(ctx, n, lens, close, (p, 1))
                st = rt.capi.rt_stats()
                rgb, u8 = render_device(rt, ctx, a, L, w, h, depth, stats=st)
                print(f"{name} {mode} n={n} p={p}: differs from the reference rays in {diff(rgb, want)} pixels, from pass 0 in {diff(rgb, base)}")
                assert bits_equal(rgb, want), (n, p, diff(rgb, want), float(np.abs(rgb - want).max()))
                assert np.array_equal(u8, quantise_u8(want))
                assert int(st.pixels_culled) == culled and int(st.pixels) == n * n * w * h
                assert not bits_equal(rgb, base)
                if n == 1:
                    _, hit, _ = render(rt, ctx, a, L, w, h, depth, hits=True)
                    assert np.array_equal(hit, face[:, :, 0, 0]), (p, "the level-0 hit of that pass's ray")
    finally:
        ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 4. the fold
FOLD_CASES = [(0, 2), (0, 5), (3, 4), (0, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,blur", [("cube.obj", 1, False), ("cube.obj", 2, True), ("dodgeColorTest.obj", 1, True), ("dodgeColorTest.obj", 2, False)])
def test_accumulated_frame_is_the_float32_fold_of_its_passes(rt, name, n, blur):
    w, h = 160, 100
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "yaw", 0.3)
    lens, close = ((AP, 1.8), b) if blur else (None, None)
    single = {}
    try:
        for first, count in FOLD_CASES:
            for p in range(first, first + count):
                if p not in single:
                    set_frame(ctx, n, lens, close, (p, 1))
                    single[p], _ = render_device(rt, ctx, a, L, w, h, 4)
            want = passes_ref.fold_passes([single[p] for p in range(first, first + count)])
            set_frame(ctx, n, lens, close, (first, count))
            rgb, u8 = render_device(rt, ctx, a, L, w, h, 4)
            host, _, _ = render(rt, ctx, a, L, w, h, 4)
            assert bits_equal(rgb, want), (first, count, diff(rgb, want), float(np.abs(rgb - want).max()))
            assert np.array_equal(u8, quantise_u8(want)), (first, count)
            assert bits_equal(host, want), "rt_render"
        assert len({single[p].tobytes() for p in single}) == len(single), "every pass is a different frame"
    finally:
        ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 5. shards, row ranges, the gather, graphs
@pytest.mark.gpu
def test_shards_row_ranges_and_the_gather_equal_the_full_frame(rt):
    import torch
    w, h, n = 256, 157, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "both", 0.3)
    set_frame(ctx, n, (AP, 1.8), b, (2, 3))
    full, full8 = render_device(rt, ctx, a, L, w, h, 4)
    for stripe in (8, 1, 5):
        for nranks in (2, 3):
            for rank in range(nranks):
                ys = [y for y in range(h) if (y // stripe) % nranks == rank]
                rgb, u8 = render_device(rt, ctx, a, L, w, h, 4, stripe=stripe, rank=rank, nranks=nranks)
                assert bits_equal(rgb, full[ys]), (stripe, nranks, rank, diff(rgb, full[ys]))
                assert np.array_equal(u8, full8[ys])
    rgb, u8 = render_device(rt, ctx, a, L, w, h, 4, row0=5, row1=h - 3)
    assert bits_equal(rgb, full[5:h - 3]) and np.array_equal(u8, full8[5:h - 3])
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
    comm.close(); ctx.close(); hs.close()
    assert np.array_equal(frame, full8.reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("name,shutter", [("cube.obj", False), ("dodgeColorTest.obj", False), ("cube.obj", True), ("dodgeColorTest.obj", True)])
def test_graph_replays_its_passes_and_keeps_them(rt, name, shutter):
    w, h, n = 320, 200, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    pairs = [shutter_pair(rt, w, h, "yaw", 0.0), shutter_pair(rt, w, h, "both", 0.3), shutter_pair(rt, w, h, "move", -0.5)]
    set_frame(ctx, n, None, pairs[0][1] if shutter else None, (0, 4))
    out, out8 = rt.hipmem.DeviceBuffer(h * w * 3 * 4), rt.hipmem.DeviceBuffer(h * w * 3)
    g = rt.FrameGraph(ctx, L, rt.make_params(w, h, 4), out.address, out8.address)
    got = []
    for k, (a, b) in enumerate(pairs):
        if k == 1:
            ctx.set_passes(0, 1)                              # the graph keeps the passes it was captured with
        g.launch(a, close=b if shutter else None)
        assert int(g.stats().pixels) == 4 * n * n * w * h
        got.append((out.to_numpy(F, (h, w, 3)), out8.to_numpy(np.uint8, (h, w, 3))))
    g.close()
    one, _ = render_device(rt, ctx, pairs[1][0], L, w, h, 4)  # the context itself is back at (0, 1)
    for (a, b), (rgb, u8) in zip(pairs, got):
        set_frame(ctx, n, None, b if shutter else None, (0, 4))
        want, want8 = render_device(rt, ctx, a, L, w, h, 4)
        assert bits_equal(rgb, want), diff(rgb, want)
        assert np.array_equal(u8, want8)
    assert not bits_equal(got[1][0], one) and not bits_equal(got[0][0], got[1][0])
    ctx.close(); hs.close(); out.free(); out8.free()


# ------------------------------------------------------------------------------------------ 6. statistics
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_stats_sum_over_the_passes(rt, name):
    w, h, n = 256, 160, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, name))
    L = area_lights(rt)
    a, b = shutter_pair(rt, w, h, "yaw")
    total = dict.fromkeys(SUMMED, 0)
    walked = []
    for p in range(4):
        set_frame(ctx, n, None, b, (p, 1))
        _, _, st = render(rt, ctx, a, L, w, h, 4)
        for k, v in summed(st).items():
            total[k] += v
        walked.append(int(st.rays_sample_walked))
    set_frame(ctx, n, None, b, (0, 4))
    base, _, st0 = render(rt, ctx, a, L, w, h, 4)
    print(f"{name}: rays_sample_walked of the four passes {walked} (sum {sum(walked)}), of the (0, 4) frame {int(st0.rays_sample_walked)}")
    assert summed(st0) == total
    # a sum of four positive terms: more than any one pass walked, no more than the sample rays of all four
    assert max(walked) < int(st0.rays_sample_walked) <= total["rays_sample"]
    assert int(st0.pixels) == 4 * n * n * w * h and st0.ms_total > 0 and st0.ms_resolve > 0
    p = rt.make_params(w, h, 4, collect_stats=True)
    counted, _, st1 = render(rt, ctx, a, L, w, h, 4, p=p)
    assert bits_equal(counted, base) and summed(st1) == total
    set_frame(ctx, n, None, b, (0, 1))
    _, _, one = render(rt, ctx, a, L, w, h, 4, p=p)
    assert int(st1.box_tests) > 3 * int(one.box_tests) > 0, "the counting pass counts every pass"
    set_frame(ctx, n, None, b, (0, 4))
    lib = ctx.lib
    lib.rt_timing_collect(ctx.handle, C.byref(rt.capi.rt_stats()))
    p.collect_stats = 2
    for _ in range(3):
        last, _, _ = render(rt, ctx, a, L, w, h, 4, p=p)
    assert bits_equal(last, base)
    tim = rt.capi.rt_stats()
    rt.capi.check(lib, ctx.handle, lib.rt_timing_collect(ctx.handle, C.byref(tim)), "rt_timing_collect")
    assert tim.ms_total > 0 and int(tim.pixels) == total["pixels"] and int(tim.launches_total) == total["launches_total"]
    assert int(tim.launches_trace) == 3 * total["launches_trace"], "one pending event set per pass and frame"
    for k in gl.COUNTERS:
        assert int(getattr(tim, k)) == total[k], k
    ctx.close(); hs.close()


# ------------------------------------------------------------------------------------------ 7. rejections and overrides
@pytest.mark.gpu
def test_rejections_and_the_adaptive_override(rt):
    import torch
    w, h, n = 96, 64, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    lib, c = ctx.lib, rt.capi
    L = area_lights(rt)
    cam = rt.default_camera(w, h, 0.2)
    vptr = lambda x: x.ctypes.data_as(C.c_void_p)
    # a rejected rt_set_passes keeps the previous setting
    set_frame(ctx, n, passes=(3, 5))
    want, _, _ = render(rt, ctx, cam, L, w, h, 4)
    for first, count in ((-1, 1), (0, 0), (0, -3), (250, 7), (256, 1), (0, 257), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.rt_set_passes(ctx.handle, first, count) == c.RT_ERR_INVALID, (first, count)
        assert b"rt_set_passes" in lib.rt_last_error(ctx.handle)
        got, _, _ = render(rt, ctx, cam, L, w, h, 4)
        assert bits_equal(got, want), (first, count)
    assert lib.rt_set_passes(ctx.handle, 255, 1) == c.RT_OK and lib.rt_set_passes(ctx.handle, 0, 256) == c.RT_OK
    # hit ids: NULL when count > 1, also with n = 1
    set_frame(ctx, 1, passes=(0, 2))
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
    # the adaptive threshold is ignored with passes on
    for passes in ((0, 3), (2, 1)):
        set_frame(ctx, n, passes=passes)
        regular, _, st0 = render(rt, ctx, cam, L, w, h, 4)
        assert ctx.supersampling_refined() == w * h
        set_frame(ctx, n, passes=passes, tau=0.05)
        ad, _, st1 = render(rt, ctx, cam, L, w, h, 4)
        assert ctx.supersampling_refined() == w * h
        assert bits_equal(ad, regular) and summed(st1) == summed(st0)
    set_frame(ctx, n, tau=0.05)                               # ... and the adaptive frame is back with (0, 1)
    render(rt, ctx, cam, L, w, h, 4)
    assert 0 < ctx.supersampling_refined() < w * h
    # 25 lights x 1024 samples at 4K with n = 4 is refused before anything is freed, passes or not
    big = rt.make_lights(points=[(-1.0 + 0.05 * i, 1.0, 1.0) for i in range(25)], area=True, usteps=32, vsteps=32)
    W, H = 3840, 2160
    set_frame(ctx, 4, passes=(0, 4))
    d_u8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    pb = rt.make_params(W, H, 4)
    assert lib.rt_render_device(ctx.handle, C.byref(rt.default_camera(W, H)), C.byref(big), C.byref(pb), None, C.c_void_p(d_u8.data_ptr()), None,
                                None, None) == c.RT_ERR_UNSUPPORTED
    assert b"GB" in lib.rt_last_error(ctx.handle)
    del d_u8
    set_frame(ctx, n, passes=(3, 5))
    got, _, _ = render(rt, ctx, cam, L, w, h, 4)              # the context still renders
    ctx.close(); hs.close()
    assert bits_equal(got, want)


# ------------------------------------------------------------------------------------------ 8. it converges
@pytest.mark.gpu
def test_sixteen_passes_converge_on_the_out_of_focus_cube(rt):
    """E1 = RMSE(F(0,1) - R), E16 = RMSE(F(0,16) - R) against R = passes (128, 128), over the pixels where F(0,1) != R.  Independent samples
    give E16 / E1 = sqrt(1/16 + 1/128) / sqrt(1 + 1/128) = 0.26; the bound 0.5 is that with a factor 2, not a measurement."""
    w, h, n = 256, 192, 2
    hs, ctx = open_ctx(rt, os.path.join(SCENES, "cube.obj"))
    L = area_lights(rt)
    cam = rt.default_camera(w, h)
    frames = {}
    for passes in ((128, 128), (0, 1), (0, 16)):
        set_frame(ctx, n, (0.08, 1.6), None, passes)
        frames[passes], _ = render_device(rt, ctx, cam, L, w, h, 4)
    ctx.close(); hs.close()
    R, F1, F16 = (frames[k].astype(np.float64) for k in ((128, 128), (0, 1), (0, 16)))
    mask = (F1 != R).any(axis=-1)
    share = float(mask.mean())
    e1 = float(np.sqrt(((F1 - R)[mask] ** 2).mean()))
    e16 = float(np.sqrt(((F16 - R)[mask] ** 2).mean()))
    print(f"pixels where F(0,1) != R: {share:.4f}; E1 = {e1:.6f}, E16 = {e16:.6f}, ratio {e16 / e1:.4f}")
    assert share >= 0.01, "the frame must be blurred somewhere"
    assert e16 / e1 < 0.5


# ------------------------------------------------------------------------------------------ 9. the counting build and the front ends
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_counting_build_renders_the_accumulated_frame(rt, name):
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
            rt.capi.check(lib, ctx, lib.rt_set_passes(ctx, 0, 3), "rt_set_passes")
            p = rt.make_params(w, h, 4)
            rgb = np.full((h, w, 3), np.nan, F)
            st = rt.capi.rt_stats()
            rt.capi.check(lib, ctx, lib.rt_render(ctx, C.byref(a), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), None, C.byref(st)), "rt_render")
            frames.append((rgb, summed(st)))
        finally:
            lib.rt_destroy(ctx)
    hs.close()
    assert bits_equal(frames[1][0], frames[0][0])
    assert frames[1][1] == frames[0][1]


@pytest.mark.gpu
def test_python_flyscene_and_cli_write_the_accumulated_frame(rt, tmp_path):
    path, w, h, n = os.path.join(SCENES, "cube.obj"), 64, 64, 2
    fs = rt.Flyscene(scene_path=path)
    fs.initialize(w, h, True, False)
    fs.supersample = n
    fs.passes = 4
    fs.output_path = str(tmp_path / "py.ppm")
    rgb = fs.raytraceScene()
    with pytest.raises(ValueError):
        fs.raytraceScene(write_ppm=False, want_hits=True)
    L = fs._lights()
    p = rt.make_params(w, h, -1)
    abi = np.zeros((h, w, 3), F)
    fs.ctx.set_passes(0, 4)
    rt.capi.check(fs.ctx.lib, fs.ctx.handle, fs.ctx.lib.rt_render(fs.ctx.handle, C.byref(rt.default_camera(w, h)), C.byref(L), C.byref(p),
                                                                   abi.ctypes.data_as(C.c_void_p), None, None), "rt_render")
    fs.passes = 1
    one = fs.raytraceScene(write_ppm=False)
    fs.ctx.close(); fs.scene.close()
    assert bits_equal(rgb, abi) and not bits_equal(one, rgb)
    r = subprocess.run([RT_RENDER, "--scene", path, "--aa", str(n), "--passes", "4", "--size", str(w), str(h), "--out", str(tmp_path / "cli.ppm")],
                       input=b"1\n0\n", capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert (tmp_path / "cli.ppm").read_bytes() == (tmp_path / "py.ppm").read_bytes()


# ------------------------------------------------------------------------------------------ 10. every primary instantiation the launchers reach
def debug_tasks(capfd):
    """the leaf tasks of the one frame rendered since the last call (RT_DEBUG level-0 line, as tests/test_gpu_switches.py reads it)"""
    import test_gpu_switches
    lines = test_gpu_switches.DEBUG_LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1, "one RT_DEBUG level-0 line per rendered frame"
    return {"closest": int(lines[0][1]), "centre": int(lines[0][2])}


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [(0, 1), (3, 1)])
@pytest.mark.parametrize("kind", ["pinhole", "lens", "shutter"])
@pytest.mark.parametrize("name", ["cube.obj", "dodgeColorTest.obj"])
def test_kind_and_pass_under_the_trace_paths_and_the_counting_variants(rt, monkeypatch, capfd, name, kind, passes):
    """launch_trace / launch_stage pick one kernel per (primary, counting, flat | stage, continuation, kind, pass).  The pass p > 0 of every
    kind through the leaf-task continuations (RT_TRACE_BUDGET=1) and, with the lens or the shutter, through the counting variants
    (collect_stats=1) is rendered by no other test; the fused tree kernel (RT_STAGED_TRACE=0) exists for the pinhole's first pass alone and
    is rendered there.  Every such frame must equal the frame of the
    default environment bit for bit (that one is tied to the numpy restatements and the oracle by the tests above).  The library hands out hit
    ids with n = 1 only, so each path also renders the n = 1 frame of the case, whose RGB and hit ids are compared as well."""
    w, h, depth, n = 64, 48, 2, 2
    tree = name != "cube.obj"
    L = area_lights(rt, 3)
    a, b = shutter_pair(rt, w, h, "both", 0.3)
    lens, close = ((AP, 1.8) if kind == "lens" else None), (b if kind == "shutter" else None)
    hs = rt.HostScene(os.path.join(SCENES, name), 1000, 15)
    monkeypatch.setenv("RT_DEBUG", "1")
    frames = {}
    try:
        fused = tree and kind == "pinhole" and passes[0] == 0
        for env in ("",) + (("RT_STAGED_TRACE=0",) if fused else ()) + (("RT_TRACE_BUDGET=1",) if tree else ()):
            if env:
                monkeypatch.setenv(*env.split("="))              # read by rt_create / rt_upload_scene
            ctx = rt.Context(0)
            ctx.upload(hs)
            try:
                capfd.readouterr()
                set_frame(ctx, n, lens, close, passes)
                rgb, _, st = render(rt, ctx, a, L, w, h, depth)
                tasks = debug_tasks(capfd)
                set_frame(ctx, 1, lens, close, passes)
                rgb1, hit1, _ = render(rt, ctx, a, L, w, h, depth, hits=True)
                frames[env] = (rgb, rgb1, hit1, tasks, int(st.launches_total))
                if not env:
                    set_frame(ctx, n, lens, close, passes)
                    counted, _, stc = render(rt, ctx, a, L, w, h, depth, p=rt.make_params(w, h, depth, collect_stats=True))
            finally:
                ctx.close()
            if env:
                monkeypatch.delenv(env.split("=")[0])
    finally:
        hs.close()
    base = frames[""]
    print(f"{name} {kind} {passes}: counted frame differs in {diff(counted, base[0])} pixels, rays_primary {int(stc.rays_primary)}, box_tests {int(stc.box_tests)}")
    assert bits_equal(counted, base[0]), diff(counted, base[0])
    assert int(stc.rays_primary) > 0 and int(stc.box_tests) > 0
    assert (base[2] >= 0).any(), "the frame must show the object"
    for env, f in frames.items():
        print(f"{name} {kind} {passes} [{env or 'default'}]: differs from the default frame in {diff(f[0], base[0])} pixels (n = 2), {diff(f[1], base[1])} pixels and "
              f"{int((f[2] != base[2]).sum())} hit ids (n = 1); level-0 tasks {f[3]}, launches {f[4]}")
        assert bits_equal(f[0], base[0]) and bits_equal(f[1], base[1]) and np.array_equal(f[2], base[2]), env
    if fused:
        assert frames["RT_STAGED_TRACE=0"][4] != base[4], "the fused kernel replaces the staged launches"
    if tree:
        assert frames["RT_TRACE_BUDGET=1"][3]["closest"] > base[3]["closest"], "tasks:closest"
