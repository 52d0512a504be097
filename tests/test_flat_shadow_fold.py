"""Flat scenes without a k_shadow launch.

With a SIMPLE light (a point or a grid of at most 64 samples) k_beam settles the hits its tile test cannot clear with the shadow units' triangle
cull (lane = hit) and leaves the rest pending; k_shade walks the pending pairs' sample segments before it shades them.  RT_SHADOW_UNITS=1
restores the k_shadow launch.  Every check is bit for bit: default == RT_SHADOW_UNITS=1 == RT_NO_CULL=1 == the oracle, on the frame, the hit
ids and the ray counters.
"""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")
MODES = {"fold": {}, "units": {"RT_SHADOW_UNITS": "1"}, "no_cull": {"RT_NO_CULL": "1"}}


def _render(rt, hs, cam, L, w, h, depth, env, monkeypatch):
    for k in ("RT_SHADOW_UNITS", "RT_NO_CULL", "RT_BEAM_BUDGET"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = rt.Context(0)
    ctx.upload(hs)
    p = rt.make_params(w, h, depth)
    rgb = np.zeros((h, w, 3), np.float32)
    hits = np.zeros((h, w), np.int32)
    st = rt.capi.rt_stats()
    rc = ctx.lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), C.byref(st))
    rt.capi.check(ctx.lib, ctx.handle, rc, "rt_render")
    ctx.close()
    return rgb, hits, st


def _counters(st):
    return (st.rays_primary, st.rays_bounce, st.rays_centre, st.rays_sample, st.shaded_hits)


def _scene(which, tmp_path):
    if which == "cube":
        return os.path.join(SCENES, "cube.obj"), 0.0
    import scenes_gen
    return scenes_gen.mixed_materials(str(tmp_path)), 0.4


def _check_modes(rt, oracle, tmp_path, monkeypatch, which, area, u, lights, depth, w, h, extra_env=None):
    path, yaw = _scene(which, tmp_path)
    pts = [(-1.0, 1.0, 1.0), (0.8, 0.4, 1.5), (0.0, 0.0, 2.0)][:lights]
    hs = rt.HostScene(path, 1000, 15)
    cam, L = rt.default_camera(w, h, yaw), rt.make_lights(points=pts, area=area, usteps=u, vsteps=u)
    out = {m: _render(rt, hs, cam, L, w, h, depth, dict(env, **(extra_env or {})), monkeypatch) for m, env in MODES.items()}
    rgb0, hits0, st0 = out["fold"]
    for m in ("units", "no_cull"):
        rgb, hits, st = out[m]
        assert np.array_equal(hits, hits0), m
        assert np.array_equal(rgb.view(np.uint32), rgb0.view(np.uint32)), (m, float(np.abs(rgb - rgb0).max()))
        assert _counters(st) == _counters(st0), m
    osc = oracle.load_scene(path)
    ref, rhits, ost = osc.render(oracle.camera(w, h, yaw), oracle.lights(area=area, usteps=u, vsteps=u, points=pts), w, h, max_depth=depth, threads=8,
                                 want_hits=True)
    assert np.array_equal(hits0, rhits)
    assert np.array_equal(rgb0.view(np.uint32), ref.view(np.uint32)), float(np.abs(rgb0 - ref).max())
    assert (rhits >= 0).sum() > 0.02 * rhits.size
    assert (st0.rays_bounce, st0.rays_centre, st0.rays_sample) == (ost.rays_bounce, ost.rays_centre, ost.rays_sample)
    osc.close(); hs.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("area,u", [(True, 8), (True, 5), (False, 1)])
def test_cube_fold_equals_shadow_units_no_cull_and_oracle(rt, oracle, tmp_path, monkeypatch, area, u):
    """cube.obj under the 8 x 8 headline light, the reference's 5 x 5 and the point light."""
    _check_modes(rt, oracle, tmp_path, monkeypatch, "cube", area, u, 1, 4, 320, 200)


@pytest.mark.gpu
@pytest.mark.parametrize("lights,u", [(1, 8), (2, 5), (3, 8)])
def test_mixed_materials_fold_equals_shadow_units_no_cull_and_oracle(rt, oracle, tmp_path, monkeypatch, lights, u):
    """The mixed-material scene: populated bounce levels, hits that carry their own light after a mirror bounce, several lights."""
    out = _check_modes(rt, oracle, tmp_path, monkeypatch, "mixed", True, u, lights, 4, 224, 152)
    assert out["fold"][2].rays_bounce > 0


@pytest.mark.gpu
def test_beam_budget_one_sends_the_tiles_to_the_per_hit_cull(rt, oracle, tmp_path, monkeypatch):
    """RT_BEAM_BUDGET=1: the tile test gives up on nearly every tile, so k_beam's per-hit cull and k_shade's pending walks carry the frame."""
    out = _check_modes(rt, oracle, tmp_path, monkeypatch, "cube", True, 8, 1, 4, 320, 200, extra_env={"RT_BEAM_BUDGET": "1"})
    st = out["fold"][2]
    assert 0 < st.rays_sample_walked < st.rays_sample


@pytest.mark.gpu
def test_launches_per_frame(rt, monkeypatch):
    """A depth-4 cube frame: memset, (k_trace, k_beam, k_shade) x 2, k_deep, k_resolve = 9 launches; RT_SHADOW_UNITS=1 adds k_shadow per level."""
    hs = rt.HostScene(os.path.join(SCENES, "cube.obj"), 1000, 15)
    w, h = 192, 108
    cam, L = rt.default_camera(w, h), rt.make_lights(area=True, usteps=8, vsteps=8)
    n = {m: _render(rt, hs, cam, L, w, h, 4, env, monkeypatch)[2].launches_total for m, env in MODES.items() if m != "no_cull"}
    assert n == {"fold": 9, "units": 11}
    hs.close()


@pytest.mark.gpu
def test_graph_replay_equals_eager(rt, oracle, monkeypatch):
    """The folded launch sequence captured in a hipGraph: replays with a yawing camera equal the eager frame and the oracle."""
    monkeypatch.delenv("RT_SHADOW_UNITS", raising=False)
    w, h, depth = 240, 136, 4
    path = os.path.join(SCENES, "cube.obj")
    hs = rt.HostScene(path, 1000, 15)
    ctx = rt.Context(0)
    ctx.upload(hs)
    L = rt.make_lights(area=True, usteps=8, vsteps=8)
    p = rt.make_params(w, h, depth)
    out = rt.hipmem.DeviceBuffer(h * w * 3 * 4)
    g = rt.FrameGraph(ctx, L, p, out.address, 0)
    osc = oracle.load_scene(path)
    for f in range(6):
        yaw = float(np.float32(0.07 * f))
        g.launch(rt.default_camera(w, h, yaw))
        if f in (0, 5):
            g.stats()
            got = out.to_numpy(np.float32, (h, w, 3))
            ref, _, _ = osc.render(oracle.camera(w, h, yaw), oracle.lights(area=True, usteps=8, vsteps=8), w, h, max_depth=depth, threads=8)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (f, float(np.abs(got - ref).max()))
            p_ = rt.make_params(w, h, depth)
            eager = np.zeros((h, w, 3), np.float32)
            rc = ctx.lib.rt_render(ctx.handle, C.byref(rt.default_camera(w, h, yaw)), C.byref(L), C.byref(p_), eager.ctypes.data_as(C.c_void_p), None, None)
            rt.capi.check(ctx.lib, ctx.handle, rc, "rt_render")
            assert np.array_equal(got.view(np.uint32), eager.view(np.uint32))
    g.close(); out.free(); osc.close(); ctx.close(); hs.close()
