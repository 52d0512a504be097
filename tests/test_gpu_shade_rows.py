"""k_shade's table loop by rows and columns of the light grid, and the light vectors' range test hoisted out of it.

Sample s = i * vsteps + j of a grid light lies at (x_i, y_j, z): on tiles lit by the scene's lights k_shade<.., FOLD> forms x_i - hx and its
square once per row, and evaluates the range test in front of normalize3_shared's fast body once per (tile, light) from the usteps + vsteps + 1
components; a tile in which the test fails for any lane keeps the loop by samples ("The sample loop: rows and columns").  Every
frame here is at most 96 x 64 pixels at depth <= 2 and is compared bit for bit with the oracle and with the same frame under
RT_SHADOW_UNITS=1 (no fold, no table, so neither the row loop nor the hoisted test): RGB, hit ids and the ray counters.

The cases: square, non-square and one-row / one-column grids (swapped row and column indices would show on 3 x 7 against 7 x 3) and a point
light; a light placed so that a whole pixel column (row) of hits has hx (hy) exactly equal to the x of a grid row (the y of a grid column),
and one whose z is the z of the cube's front vertices, so that ldx, ldy or ldz is 0 and the hoisted test fails there; a light scaled 2^41
away (the q clause fails in every lane); two and three light slots; a mirror floor whose level-1 hits carry their own light (the loops by
samples without the table); one context whose light changes between frames; a captured graph; a frame with pending shadow walks in front
of the row loop; a partly shadowed frame, so that the visibility-bit variant of the row loop runs beside the all-visible one.

What the equality cases can and cannot show.  The items of a level are appended through atomics, so which 64 hits share a tile is not known
on the host.  The CPU half (test_*_on_the_cpu, from the oracle's own hit points) asserts what holds for any order: F lit hits fail the
hoisted test, 0 < F < 64, and more than 64 lit hits pass it.  Then a tile with a failing lane exists (it falls back), no full tile holds
failing lanes only (every full tile with one of them is mixed; only a shard's partly filled last tile could hold nothing else), and the
passing hits fill at least one tile's worth.  Tiles of failing lanes ONLY are the front-vertex z case and the 2^41 case, where every lit
hit fails.
Frames cannot show that the row loop ran at all: it produces the floats of the loop by samples (that is read off the listing and the
profile).  The scene file planecube.obj was never part of this repository; the mirror case uses scenes_gen.mixed_materials, whose floor is
a mirror.  The light grid of frames has no jitter switch (rt_light_jitter_offsets is a definition only), so there is no jittered frame here.
"""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")
CUBE = os.path.join(SCENES, "cube.obj")
F = np.float32
W, H = 96, 64
POINTS = [(-1.0, 1.0, 1.0), (0.8, 0.4, 1.5), (0.0, 0.0, 2.0)]
ENV = ("RT_SHADOW_UNITS", "RT_NO_CULL", "RT_BEAM_BUDGET")


def _render(rt, ctx, cam, L, w, h, depth):
    p = rt.make_params(w, h, depth)
    rgb, hits, st = np.zeros((h, w, 3), F), np.zeros((h, w), np.int32), rt.capi.rt_stats()
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


def _oracle(oracle, path, yaw, w, h, depth, area, u, v, pts):
    osc = oracle.load_scene(path)
    ref, rhits, ost = osc.render(oracle.camera(w, h, yaw), oracle.lights(area=area, usteps=u, vsteps=v, points=pts), w, h, max_depth=depth, threads=8,
                                 want_hits=True)
    osc.close()
    assert (rhits >= 0).sum() > 0.02 * rhits.size
    return ref, rhits, ost


def _check(rt, oracle, monkeypatch, path, yaw, depth, area, u, v, pts, extra_env=None, w=W, h=H):
    extra = extra_env or {}
    hs = rt.HostScene(path, 1000, 15)
    cam, L = rt.default_camera(w, h, yaw), rt.make_lights(points=pts, area=area, usteps=u, vsteps=v)
    rows = _fresh(rt, hs, cam, L, w, h, depth, dict(extra), monkeypatch)
    units = _fresh(rt, hs, cam, L, w, h, depth, dict(extra, RT_SHADOW_UNITS="1"), monkeypatch)
    hs.close()
    ref = _oracle(oracle, path, yaw, w, h, depth, area, u, v, pts)
    _same(rows, units, "RT_SHADOW_UNITS=1")
    assert _counters(rows[2]) == _counters(units[2])
    _same(rows, ref, "oracle")
    st, ost = rows[2], ref[2]
    assert (st.rays_bounce, st.rays_centre, st.rays_sample, st.shaded_hits) == (ost.rays_bounce, ost.rays_centre, ost.rays_sample, ost.shaded_hits)
    assert st.shaded_hits > 0
    return st


# ---- the CPU half of the equality cases: the oracle's hit points and the table's floats ----------------------------------------------------

def _grid_axis(steps, length, corner):
    """the `steps` coordinates (((float)k + 0.5f) * c, c = (corner + length * 1.0f) / (float)steps) of light_grid / grid_sample along one axis"""
    c = F(F(F(corner) + F(F(length) * F(1.0))) / F(steps))
    return np.array([F(F(F(k) + F(0.5)) * c) for k in range(steps)], F)


def _cube_hits(oracle):
    """the level-0 hit points of the 96 x 64 cube frame at yaw 0, as raytraceScene forms them: [n, 3] float32"""
    osc = oracle.load_scene(CUBE)
    cam = oracle.camera(W, H, 0.0)
    org = np.array(list(cam.center), F)
    sp = oracle.screen_points(cam, W, H)
    pts = []
    for j in range(H):
        for i in range(W):
            d = (sp[j, i] - org).astype(F)
            face, t = osc.closest_hit(org, d)
            if face >= 0:
                pts.append((org + (F(t) * d).astype(F)).astype(F))
    return osc, np.array(pts, F)


def _corner_for(value, k, steps, length):
    """a light corner coordinate for which grid coordinate k of `steps` is exactly `value`, searched among the floats around the real solution"""
    fk = F(F(k) + F(0.5))
    c0 = F(F(value) / fk)
    for dc in range(-4, 5):
        c = (c0.view(np.uint32) + np.uint32(dc)).view(F) if dc >= 0 else (c0.view(np.uint32) - np.uint32(-dc)).view(F)
        if F(fk * c) != F(value):
            continue
        p0 = F(F(c * F(steps)) - F(length))
        for dp in range(-8, 9):
            p = (p0.view(np.uint32) + np.uint32(dp)).view(F) if dp >= 0 else (p0.view(np.uint32) - np.uint32(-dp)).view(F)
            if _grid_axis(steps, length, p)[k] == F(value):
                return float(p)
    return None


def _equality_light(oracle, axis):
    """(light point, failing lit hits, passing lit hits): an 8 x 8 light near the default one whose grid row 3 (axis 0) or column 3 (axis 1)
    has exactly the x (y) of the most common hit coordinate on that axis -- a pixel column (row) of the front face; z clear of every hit"""
    osc, hits = _cube_hits(oracle)
    L = oracle.lights(area=True, usteps=8, vsteps=8)
    length = (L.len_x, L.len_y)[axis]
    vals, cnt = np.unique(hits[:, axis], return_counts=True)
    point = None
    for value in vals[np.argsort(-cnt)]:
        if value >= 0:                                   # the default light stands at x < 0 < y; keep the corner on its side for x
            continue
        p = _corner_for(value, 3, 8, length)
        if p is not None:
            point = [-1.0, 1.0, 1.0]
            point[axis] = p
            break
    assert point is not None
    xs, ys = _grid_axis(8, L.len_x, point[0]), _grid_axis(8, L.len_y, point[1])
    lp = np.array(point, F)
    lit = np.array([osc.light_strikes(hp, lp[None, :])[1][0] for hp in hits])
    zero = (np.isin(hits[:, 0], xs) | np.isin(hits[:, 1], ys)) & lit                # ldx == 0 or ldy == 0 for some sample: the component clause fails
    osc.close()
    return tuple(point), int(zero.sum()), int((lit & ~zero).sum())


@pytest.mark.parametrize("axis", [0, 1])
def test_equality_light_has_failing_and_passing_hits_on_the_cpu(oracle, axis):
    """no GPU: the frame of test_hit_coordinate_equal_to_a_sample has 0 < F < 64 lit hits with a zero component and more than 64 without"""
    point, fail, ok = _equality_light(oracle, axis)
    print(f"axis {axis}: light {point}, {fail} lit hits with a zero component, {ok} without")
    assert 0 < fail < 64 and ok > 64


def test_front_vertex_z_fails_in_every_hit_on_the_cpu(oracle):
    """no GPU: with the light's z at the z of the cube's front vertices every hit of the yaw-0 frame has ldz == 0"""
    osc, hits = _cube_hits(oracle)
    z = osc.arrays()["wverts"][:, 2].max()
    osc.close()
    assert len(hits) > 64 and (hits[:, 2] == z).all()


def _front_z(oracle):
    osc = oracle.load_scene(CUBE)
    z = float(osc.arrays()["wverts"][:, 2].max())
    osc.close()
    return z


# ---- frames ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("area,u,v", [(True, 8, 8), (True, 5, 5), (True, 1, 64), (True, 64, 1), (True, 3, 7), (True, 7, 3), (False, 1, 1)])
def test_grids_and_a_point_light(rt, oracle, monkeypatch, area, u, v):
    """cube.obj, depth 2: square, one-row, one-column and non-square grids, and a point light"""
    _check(rt, oracle, monkeypatch, CUBE, 0.0, 2, area, u, v, POINTS[:1])


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 1])
def test_hit_coordinate_equal_to_a_sample(rt, oracle, monkeypatch, axis):
    """a pixel column (row) of hits with ldx (ldy) == 0 for grid row (column) 3: those lanes fail the hoisted test, their tiles fall back"""
    point, fail, ok = _equality_light(oracle, axis)
    assert 0 < fail < 64 and ok > 64
    _check(rt, oracle, monkeypatch, CUBE, 0.0, 2, True, 8, 8, [point])


@pytest.mark.gpu
def test_light_z_equal_to_the_front_vertices(rt, oracle, monkeypatch):
    """ldz == 0 in every hit of the front face: tiles of failing lanes only"""
    _check(rt, oracle, monkeypatch, CUBE, 0.0, 2, True, 8, 8, [(-1.0, 1.0, _front_z(oracle))])


@pytest.mark.gpu
@pytest.mark.parametrize("area,u,v", [(True, 8, 8), (True, 3, 7), (False, 1, 1)])
def test_light_scaled_far_away(rt, oracle, monkeypatch, area, u, v):
    """the light 2^41 away on every axis: q > 2^80 for every (hit, sample), the q clause fails in every lane"""
    s = float(2.0 ** 41)
    _check(rt, oracle, monkeypatch, CUBE, 0.0, 2, area, u, v, [(-s, s, s)])


@pytest.mark.gpu
@pytest.mark.parametrize("lights,u,v", [(2, 5, 5), (3, 8, 8), (2, 3, 7)])
def test_two_and_three_light_slots(rt, oracle, monkeypatch, lights, u, v):
    _check(rt, oracle, monkeypatch, CUBE, 0.0, 2, True, u, v, POINTS[:lights])


@pytest.mark.gpu
@pytest.mark.parametrize("lights,u,v", [(1, 8, 8), (2, 3, 7)])
def test_mirror_floor_own_light_tiles(rt, oracle, monkeypatch, tmp_path, lights, u, v):
    """level-1 hits behind the mirror floor carry their own light: the loops by samples without the table, beside level-0 tiles on the row loop"""
    import scenes_gen
    st = _check(rt, oracle, monkeypatch, scenes_gen.mixed_materials(str(tmp_path)), 0.4, 2, True, u, v, POINTS[:lights])
    assert st.rays_bounce > 0


@pytest.mark.gpu
def test_pending_walks_in_front_of_the_row_loop(rt, oracle, monkeypatch, tmp_path):
    """RT_BEAM_BUDGET=1 on mixed_materials: pairs go through the per-hit cull and the pending walks before their tiles are shaded"""
    import scenes_gen
    st = _check(rt, oracle, monkeypatch, scenes_gen.mixed_materials(str(tmp_path)), 0.4, 1, True, 8, 8, POINTS[:1], extra_env={"RT_BEAM_BUDGET": "1"})
    assert 0 < st.rays_sample_walked <= st.rays_sample


def test_partly_shadowed_frame_has_hits_of_both_kinds_on_the_cpu(oracle, tmp_path):
    """no GPU: in the frame below the oracle sees lit hits with a blocked sample (their tiles take the visibility-bit variant) and enough lit
    hits without one that some tile holds none of the others (test_gpu_shade_visible.py's argument)"""
    import scenes_gen
    import test_gpu_shade_visible as sv
    full, part, _ = sv.oracle_sample_visibility(oracle, scenes_gen.mixed_materials(str(tmp_path)), 0.4, W, H, 5, POINTS[0])
    print(f"mixed_materials: {full} hits all visible, {part} with a blocked sample")
    assert part >= 1 and part < -(-(full + part) // 64)


@pytest.mark.gpu
def test_partly_shadowed_frame(rt, oracle, monkeypatch, tmp_path):
    """mixed_materials under one 5 x 5 light: boxes shadow the floor, so tiles with blocked samples stand beside all-visible ones"""
    import scenes_gen
    st = _check(rt, oracle, monkeypatch, scenes_gen.mixed_materials(str(tmp_path)), 0.4, 1, True, 5, 5, POINTS[:1])
    assert 0 < st.rays_sample_walked


@pytest.mark.gpu
def test_light_changes_between_frames_on_one_context(rt, oracle, monkeypatch):
    """an 8 x 8 light, a 3 x 7 one elsewhere, the equality light, the first again: each frame equals its own oracle frame"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    A, B = POINTS[0], POINTS[1]
    E = _equality_light(oracle, 0)[0]
    frames = [(A, 8, 8), (B, 3, 7), (E, 8, 8), (A, 8, 8)]
    refs = {f: _oracle(oracle, CUBE, 0.0, W, H, 2, True, f[1], f[2], [f[0]]) for f in set(frames)}
    assert not np.array_equal(refs[frames[0]][0], refs[frames[1]][0]) and not np.array_equal(refs[frames[0]][0], refs[frames[2]][0])
    hs = rt.HostScene(CUBE, 1000, 15)
    ctx = rt.Context(0)
    ctx.upload(hs)
    cam = rt.default_camera(W, H, 0.0)
    for k, f in enumerate(frames):
        got = _render(rt, ctx, cam, rt.make_lights(points=[f[0]], area=True, usteps=f[1], vsteps=f[2]), W, H, 2)
        _same(got, refs[f], (k, f))
    ctx.close(); hs.close()


@pytest.mark.gpu
def test_graph_replays_the_row_loop(rt, oracle, monkeypatch):
    """a graph captured with a 7 x 3 light, replayed for three cameras: every replay equals the eager frame, the first the oracle's"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    hs = rt.HostScene(CUBE, 1000, 15)
    ctx = rt.Context(0)
    ctx.upload(hs)
    p = rt.make_params(W, H, 2)
    L = rt.make_lights(points=POINTS[:1], area=True, usteps=7, vsteps=3)
    out = rt.hipmem.DeviceBuffer(H * W * 3 * 4)
    g = rt.FrameGraph(ctx, L, p, out.address, 0)
    for f in range(3):
        yaw = float(F(0.07 * f))
        g.launch(rt.default_camera(W, H, yaw))
        g.stats()
        got = out.to_numpy(F, (H, W, 3))
        want = _render(rt, ctx, rt.default_camera(W, H, yaw), L, W, H, 2)[0]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (yaw, float(np.abs(got - want).max()))
        if f == 0:
            ref = _oracle(oracle, CUBE, 0.0, W, H, 2, True, 7, 3, POINTS[:1])[0]
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    g.close(); out.free(); ctx.close(); hs.close()
