"""k_shade's all-visible sample loop beside the general one.

With a SIMPLE light (a point or a grid of at most 64 samples) a tile whose valid lanes all hold the light's full visibility mask runs the
sample loop without the visibility bit; any other tile runs the general loop.  The frames here have tiles of both kinds, under a full 64-bit
mask (8 x 8) and a 25-bit one (5 x 5), on the flat and the tree instantiations, and are compared with the oracle bit for bit: RGB, hit ids and
the ray counters, as tests/test_flat_shadow_fold.py does.

That both loops ran is read off the counters the frame reports where they can tell: on flat scenes a (hit, light) pair whose sample segments
were never walked was proven unblocked, so its word is the full mask (rays_sample_walked < rays_sample: such pairs exist, and every frame
here has far more of them than the other kind, so whole tiles of them), and the pairs that were walked are the ones that can come out partly
blocked (rays_sample_walked > 0).  A tree scene walks every sample segment, so there the oracle's per-pixel visibility decides: the frame
has no bounce level, every shaded hit is a level-0 hit, B of them have a blocked sample (each puts its tile on the general loop: B >= 1) and
the S shaded hits fill at least ceil(S / 64) tiles, of which at most B can hold such a hit (B < ceil(S / 64): an all-visible tile exists).
"""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")


def oracle_sample_visibility(oracle, path, yaw, w, h, u, point):
    """(hits lit with every sample visible, hits lit with a blocked sample, unlit hits) over the level-0 hits of the frame, by the oracle"""
    F = np.float32
    osc = oracle.load_scene(path)
    cam, L = oracle.camera(w, h, yaw), oracle.lights(area=True, usteps=u, vsteps=u, points=[point])
    org, lp = np.array(list(cam.center), F), np.array(point, F)
    samples = oracle.light_samples(L, lp)
    assert samples.shape[0] == u * u
    full = part = unlit = 0
    for j in range(h):
        for i in range(w):
            d = (oracle.screen_to_world(cam, i, j) - org).astype(F)                      # the primary ray as raytraceScene forms it
            face, t = osc.closest_hit(org, d)
            if face < 0:
                continue
            hit = (org + F(t) * d).astype(F)
            if not osc.light_strikes(hit, lp[None, :])[1][0]:
                unlit += 1
            elif osc.light_strikes(hit, samples)[1].all():
                full += 1
            else:
                part += 1
    osc.close()
    return full, part, unlit


def _frame(rt, oracle, path, yaw, w, h, depth, u, points, walked_tells=True):
    hs = rt.HostScene(path, 1000, 15)
    cam, L = rt.default_camera(w, h, yaw), rt.make_lights(points=points, area=True, usteps=u, vsteps=u)
    ctx = rt.Context(0)
    ctx.upload(hs)
    p = rt.make_params(w, h, depth)
    rgb, hits, st = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.int32), rt.capi.rt_stats()
    rc = ctx.lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), C.byref(st))
    rt.capi.check(ctx.lib, ctx.handle, rc, "rt_render")
    ctx.close(); hs.close()
    osc = oracle.load_scene(path)
    ref, rhits, ost = osc.render(oracle.camera(w, h, yaw), oracle.lights(area=True, usteps=u, vsteps=u, points=points), w, h, max_depth=depth, threads=8,
                                 want_hits=True)
    osc.close()
    print(f"{os.path.basename(path)} {w}x{h} u={u}: shaded {st.shaded_hits}, sample rays {st.rays_sample}, walked {st.rays_sample_walked}")
    assert np.array_equal(hits, rhits)
    assert np.array_equal(rgb.view(np.uint32), ref.view(np.uint32)), float(np.abs(rgb - ref).max())
    assert (st.rays_bounce, st.rays_centre, st.rays_sample, st.shaded_hits) == (ost.rays_bounce, ost.rays_centre, ost.rays_sample, ost.shaded_hits)
    assert (rhits >= 0).sum() > 0.02 * rhits.size
    if walked_tells:                 # tiles of both kinds (module docstring)
        assert 0 < st.rays_sample_walked < st.rays_sample
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("u", [8, 5])
def test_cube_all_visible_and_general_tiles(rt, oracle, u):
    """cube.obj at 200 x 120, depth 4: mostly all-visible tiles with partly filled last tiles of each shard; a 64-bit and a 25-bit full mask"""
    _frame(rt, oracle, os.path.join(SCENES, "cube.obj"), 0.0, 200, 120, 4, u, [(-1.0, 1.0, 1.0)])


@pytest.mark.gpu
def test_mixed_materials_two_lights(rt, oracle, tmp_path):
    """tiles that mix visible, shadowed and partly shadowed hits; hits that carry their own light after a bounce"""
    import scenes_gen
    st = _frame(rt, oracle, scenes_gen.mixed_materials(str(tmp_path)), 0.4, 160, 104, 4, 5, [(-1.0, 1.0, 1.0), (0.8, 0.4, 1.5)])
    assert st.rays_bounce > 0


DODGE = (os.path.join(SCENES, "dodgeColorTest.obj"), 0.0, 96, 64, 5, (1.0, 0.2, 0.5))      # a light to the side: the car shadows part of itself


def test_dodge_frame_has_hits_of_both_kinds(oracle):
    """no GPU: the oracle's per-pixel visibility of the frame below (module docstring)"""
    full, part, unlit = oracle_sample_visibility(oracle, *DODGE)
    print(f"dodge: {full} hits all visible, {part} with a blocked sample, {unlit} unlit")
    assert part >= 1 and part < -(-(full + part) // 64)


@pytest.mark.gpu
def test_dodge_tree_instantiation(rt, oracle):
    """dodgeColorTest.obj at 96 x 64, depth 2, 5 x 5 light: k_shade<SIMPLE, not FLAT>"""
    path, yaw, w, h, u, point = DODGE
    st = _frame(rt, oracle, path, yaw, w, h, 2, u, [point], walked_tells=False)
    full, part, _ = oracle_sample_visibility(oracle, *DODGE)
    assert st.rays_bounce == 0 and st.shaded_hits == full + part              # every shaded hit is one of the level-0 hits counted here
    assert part >= 1 and part < -(-st.shaded_hits // 64)
