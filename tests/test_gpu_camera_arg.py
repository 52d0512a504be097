"""The camera block as a kernel argument: an eager launch sequence passes its frame's camera to the kernels by value and uploads nothing; a
captured graph reads the block a replay uploaded.  All frames against the CPU oracle, bit for bit.
  (i)   forty eager frames with forty yaws queued on one stream without a synchronisation in between -- more frames than the pinned upload
        ring has slots -- each into its own device buffers;
  (ii)  the frames made of several launch sequences, whose later sequences used to read the camera the first one had uploaded: adaptive
        supersampling, three passes, and an open shutter;
  (iii) an eager frame, a graph replay with another camera, an eager frame with a third."""
import ctypes as C
import os

import numpy as np
import pytest

import passes_ref
import switch_table
import test_gpu_adaptive_aa as ga
import test_gpu_lens as gl
import test_gpu_passes as gp
import test_gpu_shutter as gs
from adaptive_ref import adaptive_frame, refine

SCENES = gl.SCENES
F = np.float32
W, H, DEPTH = 96, 64, 4
bits_equal, diff, quantise_u8, open_ctx, render_device, lights_pair = gl.bits_equal, gl.diff, gl.quantise_u8, gl.open_ctx, gl.render_device, gl.lights_pair


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def cube(rt, oracle):
    path = os.path.join(SCENES, "cube.obj")
    hs, ctx = open_ctx(rt, path)
    osc = oracle.load_scene(path)
    yield ctx, osc
    osc.close(); ctx.close(); hs.close()


@pytest.mark.gpu
def test_forty_queued_eager_frames_each_keep_their_camera(rt, oracle, cube):
    import torch
    ctx, osc = cube
    L, oL = lights_pair(rt, oracle, "area5")
    yaws = [0.02 * k * (-1) ** k for k in range(40)]
    p = rt.make_params(W, H, DEPTH)
    outs = [(torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda"), torch.full((H, W, 3), 77, dtype=torch.uint8, device="cuda")) for _ in yaws]
    torch.cuda.synchronize()
    for yaw, (d_rgb, d_u8) in zip(yaws, outs):
        cam = rt.default_camera(W, H, yaw)
        st = ctx.lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(d_rgb.data_ptr()), C.c_void_p(d_u8.data_ptr()), None, None, None)
        rt.capi.check(ctx.lib, ctx.handle, st, "rt_render_device")
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_synchronize(ctx.handle), "rt_synchronize")
    frames = set()
    for yaw, (d_rgb, d_u8) in zip(yaws, outs):
        want = osc.render(oracle.camera(W, H, yaw), oL, W, H, max_depth=DEPTH, threads=8)[0]
        rgb = d_rgb.cpu().numpy()
        assert bits_equal(rgb, want), (yaw, diff(rgb, want))
        assert np.array_equal(d_u8.cpu().numpy(), quantise_u8(want)), yaw
        frames.add(want.tobytes())
    assert len(frames) == len(yaws), "every yaw is a different frame"


@pytest.mark.gpu
def test_adaptive_frame_reads_its_camera_in_both_sequences(rt, oracle, cube):
    ctx, osc = cube
    L, oL = lights_pair(rt, oracle, "area5")
    n, tau, yaw = 2, 0.05, 0.3
    try:
        one = osc.render(oracle.camera(W, H, yaw), oL, W, H, max_depth=DEPTH, threads=8)[0]
        reg = ga.box([osc.render(ga.shifted(oracle.camera(W, H, yaw), n, sx, sy), oL, W, H, max_depth=DEPTH, threads=8)[0] for sy in range(n) for sx in range(n)], n)
        mask = refine(one, tau)
        assert 0 < mask.sum() < mask.size, "the threshold must refine some pixels but not all"
        want = adaptive_frame(one, reg, tau)
        render_device(rt, ctx, rt.default_camera(W, H, 1.1), L, W, H, DEPTH)          # another camera in front: nothing of it may be read
        ga.setting(ctx, n, tau)
        rgb, u8 = render_device(rt, ctx, rt.default_camera(W, H, yaw), L, W, H, DEPTH)
        assert bits_equal(rgb, want), diff(rgb, want)
        assert np.array_equal(u8, quantise_u8(want))
        assert ctx.supersampling_refined() == int(mask.sum())
    finally:
        ga.setting(ctx, 1, -1.0)


@pytest.mark.gpu
def test_three_passes_read_their_camera_in_every_pass(rt, oracle, cube):
    ctx, osc = cube
    L, oL = lights_pair(rt, oracle, "area5")
    yaw = 0.25
    try:
        singles = []
        for p in range(3):
            ox, oy = passes_ref.library_offsets(ctx.lib, 1, p)
            singles.append(gp.oracle_pass_frame(oracle, osc, oL, W, H, 1, p, DEPTH, yaw, ox, oy)[0])
        want = passes_ref.fold_passes(singles)
        render_device(rt, ctx, rt.default_camera(W, H, 1.1), L, W, H, DEPTH)
        ctx.set_passes(0, 3)
        rgb, u8 = render_device(rt, ctx, rt.default_camera(W, H, yaw), L, W, H, DEPTH)
        assert bits_equal(rgb, want), diff(rgb, want)
        assert np.array_equal(u8, quantise_u8(want))
    finally:
        ctx.set_passes(0, 1)


@pytest.mark.gpu
def test_open_shutter_reads_both_poses(rt, oracle, cube):
    ctx, osc = cube
    L, oL = lights_pair(rt, oracle, "area5")
    a, b = gs.shutter_pair(rt, W, H, "both", 0.2)
    try:
        want, _ = gs.oracle_shutter_frame(oracle, osc, a, b, oL, W, H, 1, DEPTH, None)
        render_device(rt, ctx, rt.default_camera(W, H, 1.1), L, W, H, DEPTH)
        still, _ = render_device(rt, ctx, a, L, W, H, DEPTH)
        ctx.set_shutter(b)
        rgb, u8 = render_device(rt, ctx, a, L, W, H, DEPTH)
        assert bits_equal(rgb, want), diff(rgb, want)
        assert np.array_equal(u8, quantise_u8(want))
        assert not bits_equal(want, still), "the shutter must change the frame"
    finally:
        ctx.set_shutter(None)


@pytest.mark.gpu
def test_eager_frame_graph_replay_eager_frame(rt, oracle, cube):
    ctx, osc = cube
    L, oL = lights_pair(rt, oracle, "area5")
    y0, y1, y2 = 0.0, 0.6, -0.4
    want = [osc.render(oracle.camera(W, H, y), oL, W, H, max_depth=DEPTH, threads=8)[0] for y in (y0, y1, y2)]
    assert len({w_.tobytes() for w_ in want}) == 3
    out, out8 = rt.hipmem.DeviceBuffer(H * W * 3 * 4), rt.hipmem.DeviceBuffer(H * W * 3)
    g = rt.FrameGraph(ctx, L, rt.make_params(W, H, DEPTH), out.address, out8.address)
    try:
        first, first8 = render_device(rt, ctx, rt.default_camera(W, H, y0), L, W, H, DEPTH)
        g.launch(rt.default_camera(W, H, y1))
        g.stats()                                                   # (waits for the replay)
        replay, replay8 = out.to_numpy(F, (H, W, 3)), out8.to_numpy(np.uint8, (H, W, 3))
        last, last8 = render_device(rt, ctx, rt.default_camera(W, H, y2), L, W, H, DEPTH)
    finally:
        g.close(); out.free(); out8.free()
    for got, got8, ref, what in ((first, first8, want[0], "eager"), (replay, replay8, want[1], "replay"), (last, last8, want[2], "eager behind the replay")):
        assert bits_equal(got, ref), (what, diff(got, ref))
        assert np.array_equal(got8, quantise_u8(ref)), what
