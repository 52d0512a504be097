"""Frame overlap (rt_set_frame_overlap; DESIGN.md §5, Frames in flight): plain rt_render_device frames run their launches up to the resolve
on an internal stream and on two working sets in turn, k_resolve on the caller's stream.  Every output against the CPU oracle bit for bit
(rgb as uint32, the 8-bit image exact), and every sequence of calls again with the overlap off: the same bits.
Which route a frame took is counted (rt_debug_overlapped_frames), and with the default switch it depends on whether the frame found
something in flight to run beside -- on timing, at these sizes.  So every sequence runs three times on fresh contexts: with
rt_set_frame_overlap(ctx, 2), where every qualifying frame overlaps and the count is asserted exactly, with the default, where it may not
exceed that, and with 0, where it is 0; the three give the same bits.
  1. seven frames back to back without a synchronise, each into its own buffers: cube, the mixed-material flat scene, dodge (tree kernels);
  2. one output buffer for all frames, a device-to-device copy behind each call on the caller's stream: every snapshot is its frame;
  3. mixed traffic without a synchronise: overlapped, stats frame, overlapped, graph replay, closest hits, overlapped, rt_render;
  4. sizes 64x48 -> 160x120 -> 64x48 -> 160x120: the sets regrow with frames in flight;
  5. rt_upload_scene between overlapped frames, no synchronise by the caller;
  6. two caller streams alternating, each output checked after synchronising only its own stream;
  7. frames enqueued, then close() at once: the buffers, read afterwards, are the frames."""
import ctypes as C
import os

import numpy as np
import pytest

import scenes_gen
import switch_table
import test_gpu_lens as gl

F = np.float32
bits_equal, diff, quantise_u8 = gl.bits_equal, gl.diff, gl.quantise_u8
LIGHT_A, LIGHT_B = gl.THREE[0], (0.6, 0.9, 1.3)


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def lights(rt, oracle, pos, grid):
    return rt.make_lights(points=(pos,), area=True, usteps=grid, vsteps=grid), oracle.lights(area=True, usteps=grid, vsteps=grid, points=(pos,))


def buffers(w, h):
    import torch
    return (torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda"), torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda"))


def enqueue(rt, ctx, cam, L, p, out, stream=None, stats=None):
    st = ctx.lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()), None,
                                  C.c_void_p(stream.cuda_stream) if stream is not None else None, C.byref(stats) if stats is not None else None)
    rt.capi.check(ctx.lib, ctx.handle, st, "rt_render_device")


def synchronize(rt, ctx):
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_synchronize(ctx.handle), "rt_synchronize")


def check(out, want, what):
    rgb, u8 = (out[0].cpu().numpy(), out[1].cpu().numpy()) if not isinstance(out[0], np.ndarray) else out
    assert bits_equal(rgb, want), (what, diff(rgb, want))
    assert np.array_equal(u8, quantise_u8(want)), what


def same(a, b, what):
    for x, y in zip(a, b):
        assert bits_equal(x[0].cpu().numpy(), y[0].cpu().numpy()) and np.array_equal(x[1].cpu().numpy(), y[1].cpu().numpy()), what


def scene_path(which, tmp):
    return scenes_gen.mixed_materials(str(tmp)) if which == "mixed" else os.path.join(gl.SCENES, which)


class World:
    """the scenes, their contexts and oracle scenes, and the oracle's frames, made once and shared by the cases"""

    def __init__(self, rt, oracle, tmp):
        self.rt, self.oracle = rt, oracle
        self.paths = {k: scene_path(k, tmp) for k in ("cube.obj", "mixed", "dodgeColorTest.obj")}
        self.osc, self.frames = {}, {}

    def want(self, which, w, h, grid, depth, yaw, pos):
        key = (which, w, h, grid, depth, round(yaw, 6), pos)
        if key not in self.frames:
            if which not in self.osc:
                self.osc[which] = self.oracle.load_scene(self.paths[which])
            oL = self.oracle.lights(area=True, usteps=grid, vsteps=grid, points=(pos,))
            self.frames[key] = self.osc[which].render(self.oracle.camera(w, h, yaw), oL, w, h, max_depth=depth, threads=8, want_hits=True)[:2]
        return self.frames[key][0]

    def hits(self, which, w, h, grid, depth, yaw, pos):
        self.want(which, w, h, grid, depth, yaw, pos)
        return self.frames[(which, w, h, grid, depth, round(yaw, 6), pos)][1]

    def close(self):
        for o in self.osc.values():
            o.close()


@pytest.fixture(scope="module")
def world(rt, oracle, tmp_path_factory):
    w = World(rt, oracle, tmp_path_factory.mktemp("overlap"))
    yield w
    w.close()


def both_ways(rt, world, which, sequence, overlapped, outputs=lambda r: r):
    """sequence(ctx) on three fresh contexts: every qualifying frame overlapped (2), the default (1), the overlap off (0) -> the results of 2
    and 0.  `overlapped`: how many frames of the sequence qualify; outputs(result): its (rgb, u8) pairs, equal between 2 and 1."""
    results = {}
    for mode in (2, 1, 0):
        hs, ctx = gl.open_ctx(rt, world.paths[which])
        ctx.overlap_mode = mode
        try:
            if mode != 1:
                ctx.set_frame_overlap(mode)
            results[mode] = sequence(ctx)
            took = ctx.overlapped_frames()
        finally:
            ctx.close(); hs.close()
        print(f"overlap mode {mode}: {took} of {overlapped} qualifying frames took the overlapped route")
        assert took == overlapped if mode == 2 else (took == 0 if mode == 0 else took <= overlapped), (mode, took, overlapped)
    same(outputs(results[2]), outputs(results[1]), "the default against every frame overlapped")
    return results[2], results[0]


# ------------------------------------------------------------------------------------------ 1. seven frames back to back
@pytest.mark.gpu
@pytest.mark.parametrize("which,w,h,grid,depth", [("cube.obj", 96, 64, 8, 4), ("mixed", 96, 64, 8, 4), ("dodgeColorTest.obj", 96, 72, 5, 2)])
def test_seven_frames_back_to_back(rt, oracle, world, which, w, h, grid, depth):
    import torch
    p = rt.make_params(w, h, depth)
    plan = [(0.07 * f, LIGHT_A if f < 3 else LIGHT_B) for f in range(7)]

    def sequence(ctx):
        outs = [buffers(w, h) for _ in plan]
        torch.cuda.synchronize()
        for (yaw, pos), out in zip(plan, outs):
            enqueue(rt, ctx, rt.default_camera(w, h, yaw), lights(rt, oracle, pos, grid)[0], p, out)
        synchronize(rt, ctx)
        return outs

    on, off = both_ways(rt, world, which, sequence, len(plan))
    wants = [world.want(which, w, h, grid, depth, yaw, pos) for yaw, pos in plan]
    assert len({x.tobytes() for x in wants}) == len(plan), "every frame is a different frame"
    for k, (out, want) in enumerate(zip(on, wants)):
        check(out, want, (which, k))
    same(on, off, which)


# ------------------------------------------------------------------------------------------ 2. one output buffer, snapshots on the caller's stream
@pytest.mark.gpu
def test_one_output_buffer_snapshots_on_the_callers_stream(rt, oracle, world):
    import torch
    w, h, grid, depth = 96, 64, 8, 4
    p = rt.make_params(w, h, depth)
    yaws = [0.07 * f for f in range(7)]
    L = lights(rt, oracle, LIGHT_A, grid)[0]

    def sequence(ctx):
        stream = torch.cuda.Stream()
        out = buffers(w, h)
        snaps = [buffers(w, h) for _ in yaws]
        torch.cuda.synchronize()
        for yaw, snap in zip(yaws, snaps):
            enqueue(rt, ctx, rt.default_camera(w, h, yaw), L, p, out, stream)
            with torch.cuda.stream(stream):
                snap[0].copy_(out[0], non_blocking=True)
                snap[1].copy_(out[1], non_blocking=True)
        stream.synchronize()
        return snaps

    on, off = both_ways(rt, world, "cube.obj", sequence, len(yaws))
    for k, (snap, yaw) in enumerate(zip(on, yaws)):
        check(snap, world.want("cube.obj", w, h, grid, depth, yaw, LIGHT_A), k)
    same(on, off, "snapshots")


# ------------------------------------------------------------------------------------------ 3. mixed traffic
@pytest.mark.gpu
def test_mixed_traffic_without_a_synchronise(rt, oracle, world):
    import torch
    w, h, grid, depth = 96, 64, 8, 4
    p = rt.make_params(w, h, depth)
    L = lights(rt, oracle, LIGHT_A, grid)[0]
    yaws = {"a": 0.0, "stats": 0.07, "b": 0.14, "graph": 0.21, "hits": 0.28, "c": 0.35, "host": 0.42}
    cam = {k: rt.default_camera(w, h, y) for k, y in yaws.items()}

    def primary_rays(ctx, c):
        pts = np.empty((w * h, 3), F)
        rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_primary_points(ctx.handle, C.byref(c), w, h, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
        centre = torch.tensor(list(c.center), dtype=torch.float32, device="cuda")
        return centre.expand(w * h, 3).contiguous(), (torch.from_numpy(pts).cuda() - centre).contiguous()

    def sequence(ctx):
        outs = {k: buffers(w, h) for k in ("a", "stats", "b", "graph", "c")}
        g = rt.FrameGraph(ctx, L, p, outs["graph"][0].data_ptr(), outs["graph"][1].data_ptr())
        origins, dirs = primary_rays(ctx, cam["hits"])
        host = np.full((h, w, 3), np.nan, F)
        st = rt.capi.rt_stats()
        query_stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        try:
            enqueue(rt, ctx, cam["a"], L, p, outs["a"])
            enqueue(rt, ctx, cam["stats"], L, p, outs["stats"], stats=st)
            enqueue(rt, ctx, cam["b"], L, p, outs["b"])
            g.launch(cam["graph"])
            faces, _ = ctx.closest_hits(origins, dirs, stream=query_stream.cuda_stream)
            enqueue(rt, ctx, cam["c"], L, p, outs["c"])
            s = ctx.lib.rt_render(ctx.handle, C.byref(cam["host"]), C.byref(L), C.byref(p), host.ctypes.data_as(C.c_void_p), None, None)
            rt.capi.check(ctx.lib, ctx.handle, s, "rt_render")
            synchronize(rt, ctx)
            query_stream.synchronize()
        finally:
            g.close()
        outs["host"] = (torch.from_numpy(host).cuda(), torch.from_numpy(quantise_u8(host)).cuda())
        return outs, faces.cpu().numpy(), {k: int(getattr(st, k)) for k in gl.COUNTERS + ("launches_total",)}

    # (a, b, c and the frame of rt_render qualify; the stats frame, the replay and the query do not)
    (on, faces_on, st_on), (off, faces_off, st_off) = both_ways(rt, world, "cube.obj", sequence, 4, lambda r: [r[0][k] for k in sorted(r[0])])
    for k in ("a", "stats", "b", "graph", "c", "host"):
        check(on[k], world.want("cube.obj", w, h, grid, depth, yaws[k], LIGHT_A), k)
    same([on[k] for k in sorted(on)], [off[k] for k in sorted(off)], "mixed traffic")
    hits = world.hits("cube.obj", w, h, grid, depth, yaws["hits"], LIGHT_A)
    assert np.array_equal(faces_on.reshape(h, w), hits) and np.array_equal(faces_off, faces_on)
    # the stats frame alone on a fresh context
    hs, ctx = gl.open_ctx(rt, world.paths["cube.obj"])
    try:
        alone = rt.capi.rt_stats()
        gl.render_device(rt, ctx, cam["stats"], L, w, h, depth, stats=alone)
    finally:
        ctx.close(); hs.close()
    alone = {k: int(getattr(alone, k)) for k in gl.COUNTERS + ("launches_total",)}
    assert st_on == alone and st_off == alone and alone["launches_total"] == 9 and alone["rays_primary"] > 0


# ------------------------------------------------------------------------------------------ 4. the sets regrow with frames in flight
@pytest.mark.gpu
def test_sizes_grow_and_shrink_in_a_row(rt, oracle, world):
    import torch
    grid, depth = 5, 4
    sizes = [(64, 48), (160, 120), (64, 48), (160, 120)]
    yaws = [0.0, 0.1, 0.2, 0.3]
    L = lights(rt, oracle, LIGHT_A, grid)[0]

    def sequence(ctx):
        outs = [buffers(w, h) for w, h in sizes]
        torch.cuda.synchronize()
        for (w, h), yaw, out in zip(sizes, yaws, outs):
            enqueue(rt, ctx, rt.default_camera(w, h, yaw), L, rt.make_params(w, h, depth), out)
        synchronize(rt, ctx)
        return outs

    on, off = both_ways(rt, world, "cube.obj", sequence, len(sizes))
    for (w, h), yaw, out in zip(sizes, yaws, on):
        check(out, world.want("cube.obj", w, h, grid, depth, yaw, LIGHT_A), (w, h))
    same(on, off, "sizes")


# ------------------------------------------------------------------------------------------ 5. a scene upload between overlapped frames
@pytest.mark.gpu
def test_upload_between_overlapped_frames(rt, oracle, world):
    import torch
    w, h, grid, depth = 96, 64, 5, 4
    p = rt.make_params(w, h, depth)
    L = lights(rt, oracle, LIGHT_A, grid)[0]
    order = ["cube.obj", "mixed", "cube.obj"]
    yaws = [0.0, 0.4, 0.2]
    scenes = {k: rt.HostScene(world.paths[k], 1000, 15) for k in set(order)}

    def sequence(ctx):
        outs = [(buffers(w, h), buffers(w, h)) for _ in order]
        torch.cuda.synchronize()
        for which, yaw, (first, second) in zip(order, yaws, outs):
            ctx.upload(scenes[which])
            enqueue(rt, ctx, rt.default_camera(w, h, yaw), L, p, first)
            enqueue(rt, ctx, rt.default_camera(w, h, yaw + 0.05), L, p, second)
        synchronize(rt, ctx)
        return [o for pair in outs for o in pair]

    try:
        on, off = both_ways(rt, world, "cube.obj", sequence, 2 * len(order))
    finally:
        for s in scenes.values():
            s.close()
    k = 0
    for which, yaw in zip(order, yaws):
        for y in (yaw, yaw + 0.05):
            check(on[k], world.want(which, w, h, grid, depth, y, LIGHT_A), (which, y))
            k += 1
    same(on, off, "uploads")


# ------------------------------------------------------------------------------------------ 6. two caller streams
@pytest.mark.gpu
def test_two_caller_streams_alternating(rt, oracle, world):
    import torch
    w, h, grid, depth = 96, 64, 5, 4
    p = rt.make_params(w, h, depth)
    L = lights(rt, oracle, LIGHT_A, grid)[0]
    yaws = [0.05 * f for f in range(6)]

    def sequence(ctx):
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = [buffers(w, h) for _ in yaws]
        torch.cuda.synchronize()
        for k, (yaw, out) in enumerate(zip(yaws, outs)):
            enqueue(rt, ctx, rt.default_camera(w, h, yaw), L, p, out, streams[k & 1])
            if ctx.overlap_mode == 0:
                # (the one-set route: frames of one context on two streams share the working set and are the caller's to order, as they
                #  always were; the overlapped route orders them itself through its sets)
                streams[(k + 1) & 1].wait_event(streams[k & 1].record_event())
        got = [None] * len(yaws)
        for s in (1, 0):                                     # each stream's outputs after synchronising only that stream
            streams[s].synchronize()
            for k in range(s, len(yaws), 2):
                got[k] = (outs[k][0].cpu(), outs[k][1].cpu())
        synchronize(rt, ctx)
        return got

    on, off = both_ways(rt, world, "cube.obj", sequence, len(yaws))
    for k, (yaw, a, b) in enumerate(zip(yaws, on, off)):
        want = world.want("cube.obj", w, h, grid, depth, yaw, LIGHT_A)
        check(a, want, ("on", k))
        check(b, want, ("off", k))
    same(on, off, "two streams")


# ------------------------------------------------------------------------------------------ 7. close() with frames in flight
@pytest.mark.gpu
def test_close_at_once_with_frames_enqueued(rt, oracle, world):
    import torch
    w, h, grid, depth = 96, 64, 8, 4
    p = rt.make_params(w, h, depth)
    L = lights(rt, oracle, LIGHT_A, grid)[0]
    yaws = [0.07 * f for f in range(5)]
    stream = torch.cuda.Stream()
    outs = [buffers(w, h) for _ in yaws]
    torch.cuda.synchronize()
    hs, ctx = gl.open_ctx(rt, world.paths["cube.obj"])
    ctx.set_frame_overlap(2)
    for yaw, out in zip(yaws, outs):
        enqueue(rt, ctx, rt.default_camera(w, h, yaw), L, p, out, stream)
    took = ctx.overlapped_frames()
    ctx.close(); hs.close()
    assert took == len(yaws)
    for k, (out, yaw) in enumerate(zip(outs, yaws)):
        check(out, world.want("cube.obj", w, h, grid, depth, yaw, LIGHT_A), k)
