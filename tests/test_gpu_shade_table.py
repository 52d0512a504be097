"""k_shade's light-sample table.

On flat scenes with a SIMPLE light k_beam writes the sample positions of the scene's lights into a small table (one wave, lane = sample) and
k_shade<.., FOLD> reads them with scalar loads, one sample ahead, for every tile none of whose hits carries a light of its own; tiles behind
a mirror bounce keep the per-hit arithmetic.  RT_SHADOW_UNITS=1 runs no fold and therefore no table.  Every frame here is compared bit for
bit with the oracle and with RT_SHADOW_UNITS=1: RGB, hit ids and the ray counters.

The cases: 64, 25 and 1 table entries per light (lights that fill a slot, part of one, and a single entry); up to three light slots, with level-1 tiles whose lanes carry their own light and tiles that
mix both kinds; nearly every tile through the per-hit cull and the pending walks in front of the table loop; one context rendering with one
light, another, the first again and another grid (a table left over from an earlier frame would show); two graphs captured with different
lights on one context, replayed in turn.

What these frames cannot show: every assertion is on outputs, and the table holds the very floats the per-hit arithmetic produces, so a
build in which no tile took the table loop would pass as well (that the loop runs is read off the listing and the profile, DESIGN.md §5 /
§6).  Nor can a frame tell whether the prefetch index is clamped: the pair loaded in a light's last iteration is never consumed, and an
index one past a slot's used entries still lies inside the table's allocation.  A wrong table, a stale one, or a wrong slot does show.
"""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")
CUBE = os.path.join(SCENES, "cube.obj")
POINTS = [(-1.0, 1.0, 1.0), (0.8, 0.4, 1.5), (0.0, 0.0, 2.0)]
ENV = ("RT_SHADOW_UNITS", "RT_NO_CULL", "RT_BEAM_BUDGET")


def _render(rt, ctx, cam, L, w, h, depth):
    p = rt.make_params(w, h, depth)
    rgb, hits, st = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.int32), rt.capi.rt_stats()
    rc = ctx.lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), C.byref(st))
    rt.capi.check(ctx.lib, ctx.handle, rc, "rt_render")
    return rgb, hits, st


def _fresh(rt, hs, cam, L, w, h, depth, env, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = rt.Context(0)             # (the switches are read when the context is made)
    ctx.upload(hs)
    out = _render(rt, ctx, cam, L, w, h, depth)
    ctx.close()
    return out


def _counters(st):
    return (st.rays_primary, st.rays_bounce, st.rays_centre, st.rays_sample, st.shaded_hits)


def _same(a, b, what):
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (what, float(np.abs(a[0] - b[0]).max()))


def _oracle(oracle, path, yaw, w, h, depth, area, u, pts):
    osc = oracle.load_scene(path)
    ref, rhits, ost = osc.render(oracle.camera(w, h, yaw), oracle.lights(area=area, usteps=u, vsteps=u, points=pts), w, h, max_depth=depth, threads=8,
                                 want_hits=True)
    osc.close()
    assert (rhits >= 0).sum() > 0.02 * rhits.size
    return ref, rhits, ost


def _check(rt, oracle, monkeypatch, path, yaw, w, h, depth, area, u, pts, extra_env=None):
    extra = extra_env or {}
    hs = rt.HostScene(path, 1000, 15)
    cam, L = rt.default_camera(w, h, yaw), rt.make_lights(points=pts, area=area, usteps=u, vsteps=u)
    table = _fresh(rt, hs, cam, L, w, h, depth, dict(extra), monkeypatch)
    units = _fresh(rt, hs, cam, L, w, h, depth, dict(extra, RT_SHADOW_UNITS="1"), monkeypatch)
    hs.close()
    ref = _oracle(oracle, path, yaw, w, h, depth, area, u, pts)
    _same(table, units, "RT_SHADOW_UNITS=1")
    assert _counters(table[2]) == _counters(units[2])
    _same(table, ref, "oracle")
    st, ost = table[2], ref[2]
    assert (st.rays_bounce, st.rays_centre, st.rays_sample, st.shaded_hits) == (ost.rays_bounce, ost.rays_centre, ost.rays_sample, ost.shaded_hits)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("area,u", [(True, 8), (True, 5), (False, 1)])
def test_cube_table_entries_64_25_1(rt, oracle, monkeypatch, area, u):
    """cube.obj, 320 x 200, depth 4: a full slot, a 25-entry light and a single entry"""
    _check(rt, oracle, monkeypatch, CUBE, 0.0, 320, 200, 4, area, u, POINTS[:1])


@pytest.mark.gpu
@pytest.mark.parametrize("lights,u", [(1, 8), (2, 5), (3, 8)])
def test_mixed_materials_own_light_tiles_and_several_slots(rt, oracle, monkeypatch, tmp_path, lights, u):
    """level-1 tiles whose lanes carry their own light (no table), tiles that mix both kinds, more than one light slot in the table"""
    import scenes_gen
    st = _check(rt, oracle, monkeypatch, scenes_gen.mixed_materials(str(tmp_path)), 0.4, 224, 152, 4, True, u, POINTS[:lights])
    assert st.rays_bounce > 0


@pytest.mark.gpu
def test_beam_budget_one_pending_walks_in_front_of_the_table_loop(rt, oracle, monkeypatch):
    """RT_BEAM_BUDGET=1: nearly every tile goes through the per-hit cull and the pending walks before it is shaded"""
    st = _check(rt, oracle, monkeypatch, CUBE, 0.0, 320, 200, 4, True, 8, POINTS[:1], extra_env={"RT_BEAM_BUDGET": "1"})
    assert 0 < st.rays_sample_walked < st.rays_sample


@pytest.mark.gpu
def test_no_stale_table_on_one_context(rt, oracle, monkeypatch):
    """light A, light B, A again, then the 5 x 5 grid, all on one context: each frame equals its own oracle frame"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    w, h, depth = 320, 200, 4
    A, B = (-1.0, 1.0, 1.0), (0.8, 0.4, 1.5)
    frames = [(A, 8), (B, 8), (A, 8), (A, 5)]
    refs = {f: _oracle(oracle, CUBE, 0.0, w, h, depth, True, f[1], [f[0]]) for f in set(frames)}      # one oracle frame per distinct light
    assert not np.array_equal(refs[(A, 8)][0], refs[(B, 8)][0]) and not np.array_equal(refs[(A, 8)][0], refs[(A, 5)][0])
    hs = rt.HostScene(CUBE, 1000, 15)
    ctx = rt.Context(0)
    ctx.upload(hs)
    cam = rt.default_camera(w, h, 0.0)
    for k, f in enumerate(frames):
        got = _render(rt, ctx, cam, rt.make_lights(points=[f[0]], area=True, usteps=f[1], vsteps=f[1]), w, h, depth)
        _same(got, refs[f], (k, f))
        ost = refs[f][2]
        assert (got[2].rays_bounce, got[2].rays_centre, got[2].rays_sample, got[2].shaded_hits) == (ost.rays_bounce, ost.rays_centre, ost.rays_sample, ost.shaded_hits)
    ctx.close(); hs.close()


@pytest.mark.gpu
def test_graph_replays_rewrite_the_table(rt, monkeypatch):
    """a graph with a yawing camera for three frames, then a second graph captured with another light on the same context, then the first
    again: every replay equals the eager frame of its camera and light"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    w, h, depth = 240, 136, 4
    hs = rt.HostScene(CUBE, 1000, 15)
    ctx = rt.Context(0)
    ctx.upload(hs)
    p = rt.make_params(w, h, depth)
    L1 = rt.make_lights(points=POINTS[:1], area=True, usteps=8, vsteps=8)
    L2 = rt.make_lights(points=POINTS[1:2], area=True, usteps=5, vsteps=5)
    out1, out2 = rt.hipmem.DeviceBuffer(h * w * 3 * 4), rt.hipmem.DeviceBuffer(h * w * 3 * 4)

    def eager(L, yaw):
        return _render(rt, ctx, rt.default_camera(w, h, yaw), L, w, h, depth)[0]

    def replay(g, out, L, yaw):
        g.launch(rt.default_camera(w, h, yaw))
        g.stats()
        got = out.to_numpy(np.float32, (h, w, 3))
        want = eager(L, yaw)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (yaw, float(np.abs(got - want).max()))
        return got

    g1 = rt.FrameGraph(ctx, L1, p, out1.address, 0)
    first = [replay(g1, out1, L1, float(np.float32(0.07 * f))) for f in range(3)]
    g2 = rt.FrameGraph(ctx, L2, p, out2.address, 0)
    other = replay(g2, out2, L2, 0.0)
    assert not np.array_equal(other, first[0])
    again = replay(g1, out1, L1, 0.0)
    assert np.array_equal(again.view(np.uint32), first[0].view(np.uint32))
    g1.close(); g2.close(); out1.free(); out2.free(); ctx.close(); hs.close()
