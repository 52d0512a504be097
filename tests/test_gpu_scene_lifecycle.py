"""Scene changes on a live context, on a real MI355X: the second and every later rt_upload_scene.

rt_upload_scene recomputes the facts every frame, query and graph branches on (the device pointers and counts of the scene image, flat,
reflective, the root box of the primary cull, the occupancies, the scene generation) beside state that must survive it (the sample settings,
the cached row tables, the frame buffers).  Everything here is compared bit for bit with a TWIN: the same calls on a fresh context that only
ever saw that one scene, its two frames anchored to the CPU oracle at tolerance 0.  (tests/scene_cases.py has the scenes, their classes, the
order of the walk and the corrupted views; tests/test_scene_cases.py their CPU side.)"""
import ctypes as C

import numpy as np
import pytest

import scene_cases as sc
from test_gpu_parity import assert_frame_parity
from test_gpu_ray_queries import awkward_rays

pytestmark = pytest.mark.gpu

F = np.float32
YAW = 0.5                                            # every scene's projected root box leaves part of the 96 x 64 frame outside (pixels_culled > 0)
W1, H1, W2, H2, DEPTH = 96, 64, 61, 37, 3
LIGHTS3 = ((-1.0, 1.0, 1.0), (0.8, 0.4, 1.5), (0.0, 0.0, 2.0))
COUNTERS = ("rays_primary", "rays_bounce", "rays_centre", "rays_sample", "shaded_hits", "pixels_culled", "box_tests", "leaf_tri_refs")
PATTERN = 0xA5
AO_GRID, AO_RADIUS, AO_SEED = 3, 0.5, 5


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def first_difference(got, want):
    """the first item of a probe (in the order it was taken) that differs bitwise, or None"""
    assert list(got) == list(want)
    for k in want:
        if not same(got[k], want[k]):
            return k
    return None


def lights1(rt):
    return rt.make_lights(area=True, usteps=5, vsteps=5)


def lights2(rt):
    return rt.make_lights(points=LIGHTS3, area=True, usteps=9, vsteps=9)


def render(rt, ctx, cam, L, w, h, hits=True, stats=True):
    """rt_render -> (rgb, hit ids or None, rt_stats)"""
    rgb = np.empty((h, w, 3), F)
    hid = np.empty((h, w), np.int32) if hits else None
    st = rt.capi.rt_stats()
    p = rt.make_params(w, h, DEPTH, collect_stats=stats)
    rt.capi.check(ctx.lib, ctx.handle, ctx.lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), vp(rgb), vp(hid) if hits else None,
                                                         C.byref(st)), "rt_render")
    return rgb, hid, st


def closest(rt, ctx, rays):
    """rt_closest_hits_device of the awkward rays -> (faces, t), and the device buffers: rays, results, and room for their hit points and
    normals (the caller frees them).  The outputs are allocated FIRST: a DeviceBuffer is zeroed by a hipMemset on the null stream, which
    the context's non-blocking stream does not wait for, and the copies of the rays behind them do."""
    o, d = rays
    n = o.shape[0]
    outs = [rt.hipmem.DeviceBuffer(n * 4), rt.hipmem.DeviceBuffer(n * 4), rt.hipmem.DeviceBuffer(n * 12), rt.hipmem.DeviceBuffer(n * 12)]
    bufs = [rt.hipmem.DeviceBuffer(o.nbytes).from_numpy(o), rt.hipmem.DeviceBuffer(d.nbytes).from_numpy(d)] + outs
    ctx.closest_hits(bufs[0], bufs[1], n=n, faces=bufs[2], ts=bufs[3])
    ctx.synchronize()
    return bufs[2].to_numpy(np.int32, (n,)), bufs[3].to_numpy(F, (n,)), bufs


class Mode:
    """the sampling state of a walk, set once on a context before its first upload, and what its frames can report"""

    def __init__(self, name, setup=None, hits=False, launches=False, refined=False, pass_map=False):
        self.name, self.setup, self.hits, self.launches, self.refined, self.pass_map = name, setup, hits, launches, refined, pass_map

    def context(self, rt):
        ctx = rt.Context(0)
        if self.setup:
            self.setup(ctx)
        return ctx


# (launches_total: the one-ray frames enqueue the same sequence whatever came before them; it is what shows a stale `reflective` on a scene
# without a reflective face -- levels launched over empty lists change no pixel)
PLAIN = Mode("plain", hits=True, launches=True)


def _mode_a(ctx):
    ctx.set_supersampling(2); ctx.set_passes(0, 3); ctx.set_lens(0.02, 2.0)


def _mode_b(ctx):
    ctx.set_supersampling(2); ctx.set_supersampling_threshold(0.1)


def _mode_c(ctx):
    ctx.set_passes(0, 12); ctx.set_pass_tolerance(0.01, 8)


MODES = {"a": Mode("supersampling 2, passes (0, 3), lens", _mode_a), "b": Mode("supersampling 2, threshold 0.1", _mode_b, refined=True),
         "c": Mode("passes (0, 12), pass tolerance 0.01", _mode_c, pass_map=True)}


def probe(rt, ctx, rays, mode=PLAIN):
    """everything a test looks at after an upload, in a fixed order -> {item: array}: two frames with their counters, the closest hits of the
    1,500 awkward rays, the ambient occlusion of the first 256 of their hit points, the geometry buffers"""
    out = {}
    lib = ctx.lib
    for tag, (w, h, L) in (("frame1", (W1, H1, lights1(rt))), ("frame2", (W2, H2, lights2(rt)))):
        rgb, hid, st = render(rt, ctx, rt.default_camera(w, h, YAW), L, w, h, hits=mode.hits)
        out[tag + ".rgb"] = rgb
        if mode.hits:
            out[tag + ".hits"] = hid
        for k in COUNTERS + (("launches_total",) if mode.launches else ()):
            out[f"{tag}.{k}"] = np.array([getattr(st, k)], np.uint64)
        if mode.refined:
            out[tag + ".refined"] = np.array([ctx.supersampling_refined()], np.uint64)
        if mode.pass_map:
            out[tag + ".pass_map"] = ctx.pass_map(w, h)
    faces, ts, bufs = closest(rt, ctx, rays)
    out["closest.faces"], out["closest.t"] = faces, ts
    n = rays[0].shape[0]
    pts, nrm = ctx.hit_points(bufs[0], bufs[1], bufs[2], bufs[3], n=n, points=bufs[4], normals=bufs[5])
    ctx.synchronize()
    hit = np.nonzero(faces >= 0)[0][:256]
    P = np.ascontiguousarray(pts.to_numpy(F, (n, 3))[hit])
    N = np.ascontiguousarray(nrm.to_numpy(F, (n, 3))[hit])
    for b in bufs:
        b.free()
    out["hit.points"], out["hit.normals"] = P, N
    opened, ao = np.zeros(len(hit), np.uint16), np.zeros(len(hit), F)
    rt.capi.check(lib, ctx.handle, lib.rt_ambient_occlusion(ctx.handle, len(hit), vp(P), vp(N), AO_GRID, AO_RADIUS, AO_SEED, vp(opened), vp(ao)),
                  "rt_ambient_occlusion")
    out["ao.open"], out["ao.ao"] = opened, ao
    gb = np.zeros((H2, W2, rt.capi.RT_GBUFFER_CHANNELS), F)
    p = rt.make_params(W2, H2)
    cam = rt.default_camera(W2, H2, YAW)
    out["gbuffer.status"] = np.array([lib.rt_gbuffer(ctx.handle, C.byref(cam), C.byref(p), vp(gb))], np.int64)     # (refused with adaptive passes on)
    out["gbuffer"] = gb
    return out


def twin_of(rt, hs, rays, mode=PLAIN):
    ctx = mode.context(rt)
    ctx.upload(hs)
    t = probe(rt, ctx, rays, mode)
    ctx.close()
    return t


@pytest.fixture(scope="module")
def rays():
    o, d, _, _ = awkward_rays()
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


@pytest.fixture(scope="module")
def hosts(rt, scenes, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lifecycle")
    hs = sc.load_scenes(rt, scenes, tmp)
    hs["_files"] = sc.scene_files(scenes, tmp)
    yield hs
    for k, h in hs.items():
        if k != "_files":
            h.close()


@pytest.fixture(scope="module")
def twins(rt, oracle, hosts, rays):
    """name -> the probe of a fresh context that saw only that scene; its two frames are the oracle's bit for bit, hit ids included, and a
    part of frame 1 lies outside the projected root box"""
    out = {}
    for name in sc.NAMES:
        t = twin_of(rt, hosts[name], rays)
        path, cap = hosts["_files"][name]
        osc = oracle.load_scene(path, capacity=cap)
        for tag, (w, h, L) in (("frame1", (W1, H1, oracle.lights(area=True, usteps=5, vsteps=5))),
                               ("frame2", (W2, H2, oracle.lights(area=True, usteps=9, vsteps=9, points=LIGHTS3)))):
            ref, rhits, ost = osc.render(oracle.camera(w, h, YAW), L, w, h, max_depth=DEPTH, threads=8, want_hits=True)
            assert_frame_parity(oracle, t[tag + ".rgb"], t[tag + ".hits"], ref, rhits)
            assert same(t[tag + ".rgb"], ref), (name, tag)
            for k in COUNTERS:
                want = ost.precull_tests - ost.rays_primary if k == "pixels_culled" else getattr(ost, k)
                assert int(t[f"{tag}.{k}"][0]) == want, (name, tag, k)
        osc.close()
        assert int(t["frame1.pixels_culled"][0]) > 0 and int(t["frame1.shaded_hits"][0]) > 0, name
        assert (t["closest.faces"] >= 0).any() and t["ao.open"].size > 0 and int(t["gbuffer.status"][0]) == 0, name
        out[name] = t
    return out


def walk(rt, hosts, rays, order, twin, mode=PLAIN):
    """uploads order[0], order[1], ... on ONE context and probes after each; every probe must be the twin's"""
    ctx = mode.context(rt)
    prev = None
    for name in order:
        ctx.upload(hosts[name])
        k = first_difference(probe(rt, ctx, rays, mode), twin[name])
        assert k is None, f"{mode.name}: after the upload {prev} -> {name}, {k} differs from the context that saw only {name}"
        prev = name
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ 1. scene walks
def test_every_scene_after_every_other_on_one_context(rt, hosts, twins, rays):
    """The 21 uploads of scene_cases.WALK -- every ordered pair (previous, next) of the five scenes once: flat <-> tree, reflective <-> not,
    chunks that may never be culled <-> none, larger <-> smaller -- on one context.  After each, the two frames (float RGB as bits, hit ids,
    eight counters and the launch count), the closest hits (faces, t bits), the hit points, the AO counts and the eight geometry-buffer floats
    per pixel equal those of a fresh context that was only ever given that scene."""
    walk(rt, hosts, rays, sc.WALK, twins)


@pytest.mark.parametrize("which", sorted(MODES))
def test_sampling_state_survives_uploads(rt, hosts, rays, which):
    """cube -> dodge -> mixed -> cube with the sampling state set once, before the first upload: (a) supersampling, passes and the lens;
    (b) adaptive supersampling, whose row tables stay cached across the uploads because the rows do not change, with rt_supersampling_refined;
    (c) adaptive pass counts with rt_pass_map.  The settings are the context's, not the scene's: every probe equals the twin given the
    same calls."""
    mode = MODES[which]
    twin = {name: twin_of(rt, hosts[name], rays, mode) for name in ("cube", "dodge", "mixed")}
    for name, t in twin.items():
        for tag, px in (("frame1", W1 * H1), ("frame2", W2 * H2)):
            if mode.refined:                  # tau refines some pixels, not all
                assert 0 < int(t[tag + ".refined"][0]) < px, (name, tag, int(t[tag + ".refined"][0]))
            if mode.pass_map:                 # some pixels stop early, some take every pass
                assert t[tag + ".pass_map"].min() < 12 and t[tag + ".pass_map"].max() == 12, (name, tag)
        assert int(t["gbuffer.status"][0]) == (rt.capi.RT_ERR_INVALID if mode.pass_map else 0)
    walk(rt, hosts, rays, ("cube", "dodge", "mixed", "cube"), twin, mode)


# ------------------------------------------------------------------------------------------------------------ 2. refused uploads
@pytest.mark.parametrize("name", ["dodge", "cube"])
def test_refused_uploads_leave_everything_as_it_was(rt, hosts, twins, rays, name):
    """Every corrupted view of scene_cases.corrupted_views is refused by rt_upload_scene with its status and text -- the same verdicts
    validate_scene gives on the CPU (tests/test_scene_cases.py) -- and after all 18 refusals the graph captured before them replays to the same
    frame, rt_graph_stats answers, and an eager frame and the closest hits are what they were."""
    lib, c = rt.load_library(), rt.capi
    hs = hosts[name]
    ctx = rt.Context(0)
    ctx.upload(hs)
    cam, L, p = rt.default_camera(W1, H1, YAW), lights1(rt), rt.make_params(W1, H1, DEPTH)
    eager_before, hits_before, _ = render(rt, ctx, cam, L, W1, H1, stats=False)
    out = rt.hipmem.DeviceBuffer(H1 * W1 * 12)
    g = rt.FrameGraph(ctx, L, p, out.address, None)
    g.launch(cam)
    st_before = g.stats()
    before = out.to_numpy(F, (H1, W1, 3))
    assert same(before, twins[name]["frame1.rgb"]) and same(eager_before, before)
    faces_before, ts_before, bufs = closest(rt, ctx, rays)
    for b in bufs:
        b.free()
    for b in sc.corrupted_views(rt, hs.view):
        assert lib.rt_upload_scene(ctx.handle, C.byref(b.view)) == b.status, b.name
        assert b.text in lib.rt_last_error(ctx.handle), (b.name, lib.rt_last_error(ctx.handle))
    out.from_numpy(np.full(H1 * W1 * 12, PATTERN, np.uint8))
    assert lib.rt_graph_launch(g.handle, C.byref(cam), None) == c.RT_OK, lib.rt_last_error(ctx.handle)
    st = c.rt_stats()
    assert lib.rt_graph_stats(g.handle, C.byref(st)) == c.RT_OK, lib.rt_last_error(ctx.handle)
    assert same(out.to_numpy(F, (H1, W1, 3)), before), "the replayed frame changed"
    assert [getattr(st, k) for k in COUNTERS[:5]] == [getattr(st_before, k) for k in COUNTERS[:5]]
    eager, hits, _ = render(rt, ctx, cam, L, W1, H1, stats=False)
    assert same(eager, before) and same(hits, hits_before), "the eager frame changed"
    faces, ts, bufs = closest(rt, ctx, rays)
    for b in bufs:
        b.free()
    assert same(faces, faces_before) and same(ts, ts_before) and same(faces, twins[name]["closest.faces"]), "the closest hits changed"
    g.close(); out.free(); ctx.close()
