"""Primary culling (rt_set_primary_cull) on the host: the rectangle of rt_debug_primary_rect against the CPU oracle.  No GPU.

The rectangle must contain every pixel the oracle reports a hit for, must leave outside no more pixels than the oracle culls with its
root-box test (so every pixel outside it is a culled pixel), and must be the whole frame in every case the header lists as a fallback.
tests/test_gpu_primary_cull.py renders the same cameras and shapes with culling on and off.  The soundness checks also run over the general
cameras of tests/camera_cases.py, which tests/test_gpu_cameras.py renders.
"""
import math
import os

import numpy as np
import pytest

import camera_cases as cc

HERE =os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")
NAMES = ("cube.obj", "dodgeColorTest.obj")
# the default camera; a yaw sweep that leaves the object partly off-screen (0.55 .. 0.9), wholly off-screen with a corner of its box still
# beside the camera (1.2: cube) and behind the camera (2.0, pi); and (None) a camera at the centre of the root box
YAWS = (0.0, 0.2, 0.55, 0.9, 1.2, 2.0, math.pi, None)
SHAPES = ((96, 64), (101, 67), (64, 45))
SPLITS = ((8, 2), (5, 3))          # (stripe, nranks)
GENERAL_SHAPES = ((96, 64), (101, 67))


def whole(w, h):
    return (0, 0, (w + 7) // 8, (h + 7) // 8)


def root_box(rt, name):
    hs = rt.HostScene(os.path.join(SCENES, name), 1000, 15)
    box = hs.info()["root_box"]
    hs.close()
    return box


def camera(rt, w, h, yaw, box):
    """the yaw camera, or (yaw None) the default camera moved to the centre of `box`"""
    if yaw is not None:
        return rt.default_camera(w, h, yaw)
    cam = rt.default_camera(w, h)
    for k in range(3):
        c = 0.5 * (box[k] + box[3 + k])
        cam.center[k] = c
        cam.inv_view[4 * k + 3] = c
    return cam


def oracle_camera(oracle, w, h, yaw, box):
    if yaw is not None:
        return oracle.camera(w, h, yaw)
    cam = oracle.camera(w, h)
    for k in range(3):
        c = 0.5 * (box[k] + box[3 + k])
        cam.center[k] = c
        cam.inv_view[4 * k + 3] = c
    return cam


def outside_mask(rect, w, h):
    m = np.ones((h, w), bool)
    m[rect[1] * 8:rect[3] * 8, rect[0] * 8:rect[2] * 8] = False
    return m


def shard_rows(h, stripe, nranks, rank, row0=0, row1=None):
    row1 = h if row1 is None else row1
    return [y for y in range(row0, row1) if ((y - row0) // stripe) % nranks == rank]


@pytest.fixture(scope="module")
def views(rt, oracle):
    """(name, shape, yaw) -> (rect, oracle hit ids, oracle culled pixels)"""
    out = {}
    for name in NAMES:
        box = root_box(rt, name)
        osc = oracle.load_scene(os.path.join(SCENES, name))
        for (w, h) in SHAPES:
            for yaw in YAWS:
                rect = rt.primary_rect(camera(rt, w, h, yaw, box), box, w, h)
                _, hits, st = osc.render(oracle_camera(oracle, w, h, yaw, box), oracle.lights(area=False), w, h, max_depth=0, threads=8, want_hits=True)
                out[(name, (w, h), yaw)] = (rect, hits, int(st.precull_tests - st.rays_primary))
        # the general cameras of tests/camera_cases.py: pitched, translated, sheared, mirrored, other fields of view, a shifted viewport
        for (w, h) in GENERAL_SHAPES:
            for cname in cc.NAMES:
                if cname == "corner" and not (w % 8 > 2 and h % 8 > 2):
                    continue
                cam, ocam = cc.pair(rt, oracle, cname, w, h, box, osc)
                rect = rt.primary_rect(cam, box, w, h)
                _, hits, st = osc.render(ocam, oracle.lights(area=False), w, h, max_depth=0, threads=8, want_hits=True)
                out[(name, (w, h), cname)] = (rect, hits, int(st.precull_tests - st.rays_primary))
        osc.close()
    return out


def test_rectangle_is_well_formed_and_contains_every_hit(views):
    for (name, (w, h), yaw), (rect, hits, _) in views.items():
        tx0, ty0, tx1, ty1 = rect
        assert 0 <= tx0 <= tx1 <= (w + 7) // 8 and 0 <= ty0 <= ty1 <= (h + 7) // 8, (name, w, h, yaw, rect)
        assert not (hits[outside_mask(rect, w, h)] >= 0).any(), (name, w, h, yaw, rect)


def test_pixels_outside_never_exceed_the_oracles_culled_pixels(views):
    for (name, (w, h), yaw), (rect, hits, culled) in views.items():
        outside = int(outside_mask(rect, w, h).sum())
        print(f"{name} {w}x{h} yaw {yaw}: rect {rect}, {outside} of {w * h} pixels outside, the oracle culls {culled}, {int((hits >= 0).sum())} hits")
        assert outside <= culled, (name, w, h, yaw, rect, outside, culled)


def test_the_camera_set_is_not_vacuous(views):
    for name in NAMES:
        for (w, h) in SHAPES:
            fr = [outside_mask(views[(name, (w, h), yaw)][0], w, h).mean() for yaw in YAWS]
            assert max(fr) > 0.5, (name, w, h, fr)            # some camera leaves more than half the frame outside
            assert min(fr) == 0.0, (name, w, h, fr)           # ... and some camera nothing
            hit_views = [yaw for yaw in YAWS if (views[(name, (w, h), yaw)][1] >= 0).any()]
            assert any(outside_mask(views[(name, (w, h), yaw)][0], w, h).mean() > 0.2 for yaw in hit_views), "a view WITH hits must cull too"


def test_general_cameras_reach_the_window_and_the_fallbacks(views):
    """the two soundness tests above run over the general cameras too (they are entries of `views`); this one shows that those entries
    reach a proper window, the empty rectangle and the whole-frame fallback"""
    for name in NAMES:
        for (w, h) in GENERAL_SHAPES:
            rects = {c: views[(name, (w, h), c)][0] for c in cc.NAMES if (name, (w, h), c) in views}
            for c, r in rects.items():
                print(f"{name} {w}x{h} {c}: rect {r}")
            assert rects["inside"] == whole(w, h)
            assert rects["away"] == (0, 0, 0, 0)
            proper = [c for c in rects if rects[c] != whole(w, h) and rects[c][2] > rects[c][0] and rects[c][3] > rects[c][1]]
            assert proper, (name, w, h, rects)
            if "corner" in rects:
                tx, ty = (w + 7) // 8, (h + 7) // 8
                assert rects["corner"][0] > tx // 2 and rects["corner"][1] > ty // 2 and rects["corner"][2:] == (tx, ty)      # the far corner only
    assert any(k[2] == "corner" for k in views)


def test_shards_and_row_ranges_see_the_same_rectangle(rt, oracle, views):
    """the rectangle is a property of the frame: a rank's rows hold their share of the outside pixels and none of its hits lies outside;
    a row range is bounded by the oracle's count for that range"""
    for name in NAMES:
        box = root_box(rt, name)
        osc = oracle.load_scene(os.path.join(SCENES, name))
        for (w, h) in SHAPES:
            for yaw in (0.0, 0.55, 0.9):
                rect, hits, culled = views[(name, (w, h), yaw)]
                out = outside_mask(rect, w, h)
                for stripe, nranks in SPLITS:
                    total = 0
                    for rank in range(nranks):
                        ys = shard_rows(h, stripe, nranks, rank)
                        assert not (hits[ys][out[ys]] >= 0).any()
                        total += int(out[ys].sum())
                    assert total == int(out.sum())
                r0, r1 = 5, h - 3
                _, _, st = osc.render(oracle_camera(oracle, w, h, yaw, box), oracle.lights(area=False), w, h, max_depth=0, threads=8, row0=r0, row1=r1)
                assert int(out[r0:r1].sum()) <= int(st.precull_tests - st.rays_primary), (name, w, h, yaw)
        osc.close()


def test_sample_settings_that_cannot_cull_keep_the_whole_frame(rt):
    w, h = 96, 64
    for name in NAMES:
        box = root_box(rt, name)
        cam = rt.default_camera(w, h)
        assert rt.primary_rect(cam, box, w, h) != whole(w, h)
        assert rt.primary_rect(cam, box, w, h, supersampling=2) == whole(w, h)
        assert rt.primary_rect(cam, box, w, h, aperture=0.05) == whole(w, h)
        assert rt.primary_rect(cam, box, w, h, shutter=True) == whole(w, h)
        assert rt.primary_rect(cam, box, w, h, passes=(0, 2)) == whole(w, h)
        assert rt.primary_rect(cam, box, w, h, passes=(1, 1)) == whole(w, h)
        assert rt.primary_rect(cam, box, w, h, passes=(0, 1)) == rt.primary_rect(cam, box, w, h)


def test_cameras_the_argument_does_not_cover_keep_the_whole_frame(rt):
    w, h = 96, 64
    box = root_box(rt, "cube.obj")
    W = whole(w, h)
    # the camera centre inside the box, just outside it (inside the inflated box) and exactly on a face plane
    assert rt.primary_rect(camera(rt, w, h, None, box), box, w, h) == W
    near = rt.default_camera(w, h)
    near.center[2] = near.inv_view[11] = box[5] * 1.0005
    assert rt.primary_rect(near, box, w, h) == W
    plane = rt.default_camera(w, h)
    plane.center[0] = plane.inv_view[3] = box[3]
    assert rt.primary_rect(plane, box, w, h) == W
    # a corner behind the camera while another lies in front of it; a corner at a depth small against the box's
    assert rt.primary_rect(rt.default_camera(w, h, 1.2), box, w, h) == W
    close = rt.default_camera(w, h)
    close.center[2] = close.inv_view[11] = box[5] + 0.002
    long_box = list(box)
    long_box[2] = -50.0
    assert rt.primary_rect(close, long_box, w, h) == W
    # non-finite inputs, a singular view matrix, a degenerate viewport
    for bad in (float("nan"), float("inf")):
        cam = rt.default_camera(w, h)
        cam.center[1] = bad
        assert rt.primary_rect(cam, box, w, h) == W
        cam = rt.default_camera(w, h)
        cam.inv_view[5] = bad
        assert rt.primary_rect(cam, box, w, h) == W
        b = list(box)
        b[4] = bad
        assert rt.primary_rect(rt.default_camera(w, h), b, w, h) == W
    cam = rt.default_camera(w, h)
    for k in (0, 1, 2):
        cam.inv_view[4 + k] = 0.0
    assert rt.primary_rect(cam, box, w, h) == W
    cam = rt.default_camera(w, h)
    cam.viewport[2] = 0.0
    assert rt.primary_rect(cam, box, w, h) == W
    # the whole box behind the camera: nothing to trace
    assert rt.primary_rect(rt.default_camera(w, h, math.pi), box, w, h) == (0, 0, 0, 0)


def test_margin_is_at_least_one_tile(rt):
    """the tiles of the projected corners themselves lie strictly inside the rectangle wherever the frame allows"""
    w, h = 640, 360
    for name in NAMES:
        box = root_box(rt, name)
        cam = rt.default_camera(w, h, 0.1)
        lib = rt.load_library()
        import ctypes as C
        xs, ys = [], []
        # raster position of a corner: march the pixel grid for the ray that passes closest -- rt_screen_to_world gives the screen points
        for k in range(8):
            P = np.array([box[3 if k & 1 else 0], box[4 if k & 2 else 1], box[5 if k & 4 else 2]], np.float64)
            c = np.array(list(cam.center), np.float64)
            o = (C.c_float * 3)()
            pts = {}
            for (i, j) in ((0, 0), (w, 0), (0, h)):
                lib.rt_screen_to_world(C.byref(cam), float(i), float(j), o)
                pts[(i, j)] = np.array(list(o), np.float64)
            ex, ey = (pts[(w, 0)] - pts[(0, 0)]) / w, (pts[(0, h)] - pts[(0, 0)]) / h       # the screen plane is affine in (i, j)
            # c + t (P - c) = s00 + i ex + j ey
            sol = np.linalg.solve(np.stack([ex, ey, -(P - c)], axis=1), c - pts[(0, 0)])
            assert sol[2] > 0
            xs.append(sol[0]); ys.append(sol[1])
        rect = rt.primary_rect(cam, box, w, h)
        assert rect[0] * 8 <= max(0, min(xs) - 8) and rect[2] * 8 >= min(w, max(xs) + 8), (rect, xs)
        assert rect[1] * 8 <= max(0, min(ys) - 8) and rect[3] * 8 >= min(h, max(ys) + 8), (rect, ys)
        assert rect != whole(w, h)
