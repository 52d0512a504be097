"""The camera set of tests/camera_cases.py, checked without a device so that tests/test_gpu_cameras.py cannot pass vacuously:

* the oracle, an independent numpy restatement of Camera::screenToWorld and the library's host rt_screen_to_world agree bit for bit on
  every pixel of every camera, the ones the reference cannot produce included;
* every camera that is meant to be general has nine non-zero linear entries, none of them +-1;
* two deliberately wrong restatements of the sum -- the other association, and a fused multiply-add -- change the world point on at
  least 1 % of the pixels of each such camera and on NO pixel of the four yaw cameras all earlier pins use: the gap, stated as a test;
* the cameras see what their names say, by the oracle: 10 % .. 90 % of the pixels hit for the in-view cameras on each scene, none for
  `away`, every pixel and one face for `closeup`, hits in the last partial tile only for `corner`.

Measured (the tests print every figure): percent of the pixels with a hit at 96 x 72 (`corner`: 61 x 45), by the oracle

    camera     cube  mixed  dodge      camera     cube  mixed  dodge
    fly0       63.8   17.6   31.9      corner      0.5    0.1    0.1
    fly1       52.0   20.9   31.4      closeup   100.0  100.0  100.0
    fly2       55.4   23.3   19.5      sheared    88.8   62.4   36.6
    fly3       51.6   36.9   33.6      mirrored   63.3   36.8   13.6
    fly4       63.5   36.8   13.6      fovy20     63.8   19.5   46.2
    fly5       46.7   31.5   28.2      fovy120    75.2   25.9   53.0
    fly6       75.7   19.5   22.6      aspect1    72.6   31.0   26.0
    inside    100.0   53.7  100.0      vporigin   63.6   36.6   13.7
    away        0.0    0.0    0.0

and the share of pixels whose world point changes under the wrong restatements: the other association 13 % (`fovy20`) to 56 %
(`fovy120`), typically 40-55 %; the fused multiply-add 1.2 % (`fovy20`) to 37 % (`fovy120`), typically 12-26 %; both 0 on the four yaw
cameras and on the pitch-only fly camera.
"""
import ctypes as C

import numpy as np
import pytest

import camera_cases as cc
import ref_inputs as RI

F = np.float32


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def sizes_of(name):
    return ((61, 45),) if name == "corner" else cc.SIZES


@pytest.fixture(scope="module")
def world(rt, oracle, tmp_path_factory):
    """scene -> (root box, oracle scene)"""
    tmp = tmp_path_factory.mktemp("cameras")
    out = {}
    for name in cc.SCENE_NAMES:
        path = cc.scene_path(name, tmp)
        hs = rt.HostScene(path, 1000, 15)
        box = list(hs.info()["root_box"])
        hs.close()
        out[name] = (box, oracle.load_scene(path))
    yield out
    for _, osc in out.values():
        osc.close()


@pytest.fixture(scope="module")
def hits(rt, oracle, world):
    """(scene, camera, size) -> (oracle hit ids, oracle stats) of the primary rays"""
    out = {}
    for scene, (box, osc) in world.items():
        for name in cc.NAMES:
            for (w, h) in sizes_of(name):
                cam = cc.oracle_camera(rt, oracle, name, w, h, box, osc)
                _, ids, st = osc.render(cam, oracle.lights(area=False), w, h, max_depth=0, threads=8, want_hits=True)
                out[(scene, name, (w, h))] = (ids, st)
    return out


def host_points(rt, cam, w, h):
    f = rt.load_library().rt_screen_to_world
    out = np.empty((h * w, 3), F)
    buf = (C.c_float * 3)()
    ref = C.byref(cam)
    for j in range(h):
        for i in range(w):
            f(ref, float(i), float(j), buf)
            out[j * w + i] = buf
    return out.reshape(h, w, 3)


def test_oracle_numpy_and_host_agree_on_every_camera(rt, oracle, world):
    seen = set()
    for scene, (box, osc) in world.items():
        for name in cc.NAMES:
            for (w, h) in sizes_of(name):
                cam, ocam = cc.pair(rt, oracle, name, w, h, box, osc)
                key = (bytes(ocam), w, h)
                if key in seen:                       # the cameras that do not depend on the scene
                    continue
                seen.add(key)
                want = cc.numpy_points(ocam, w, h)
                assert np.isfinite(want).all()
                got = oracle.screen_points(ocam, w, h)
                assert np.array_equal(u32(got), u32(want)), (scene, name, w, h, "oracle", cc.differing_share(got, want))
                got = host_points(rt, cam, w, h)
                assert np.array_equal(u32(got), u32(want)), (scene, name, w, h, "rt_screen_to_world", cc.differing_share(got, want))
    assert len(seen) > len(cc.NAMES)


def test_the_abi_only_cameras_are_what_their_names_say(rt, oracle, world):
    box, osc = world["cube.obj"]
    w, h = 61, 45
    lin = {n: cc.linear_part(cc.oracle_camera(rt, oracle, n, w, h, box, osc)).astype(np.float64).reshape(3, 3) for n in cc.NAMES}
    for n in cc.FLY:
        assert np.abs(lin[n] @ lin[n].T - np.eye(3)).max() < 1e-6 and np.linalg.det(lin[n]) > 0.999, n
    assert np.abs(lin["sheared"] @ lin["sheared"].T - np.eye(3)).max() > 0.05, "a blend of two rotations is not orthonormal"
    assert np.linalg.det(lin["mirrored"]) < -0.999
    cams = {n: cc.oracle_camera(rt, oracle, n, w, h, box, osc) for n in cc.ABI_ONLY}
    assert cams["fovy20"].fovy == 20.0 and cams["fovy120"].fovy == 120.0
    assert cams["aspect1"].aspect == 1.0 != F(w) / F(h)
    assert (cams["vporigin"].viewport[0], cams["vporigin"].viewport[1]) == (-0.25, 0.5)
    # the two fly cameras behind `sheared` differ in pitch and translation
    a, b = RI.FLY_CAMERAS[1], RI.FLY_CAMERAS[4]
    assert a[3] != b[3] and a[4] != b[4]


def test_general_cameras_have_no_structural_zero_or_one(rt, oracle, world):
    for scene, (box, osc) in world.items():
        for name in cc.GENERAL:
            for (w, h) in sizes_of(name):
                lin = cc.linear_part(cc.oracle_camera(rt, oracle, name, w, h, box, osc))
                assert (lin != 0).all() and (np.abs(lin) != 1).all(), (scene, name, lin)
    # ... which the yaw cameras are not, and neither is a pitch without yaw
    for (w, h, yaw) in RI.CAMERAS:
        assert (cc.linear_part(oracle.camera(w, h, yaw)) == 0).sum() >= 4
    assert set(cc.NAMES) - set(cc.GENERAL) == {"inside", "away", "closeup", "fly0"} and RI.FLY_CAMERAS[0][2] == 0.0
    assert (cc.linear_part(cc.fly(oracle, 0, 96, 72)) == 0).sum() == 4


def test_wrong_restatements_show_on_general_cameras_and_never_on_yaw_cameras(rt, oracle, world):
    """the other association of the sum and a contracted multiply-add: at least 1 % of the pixels of every general camera, none of the
    four yaw cameras of ref_inputs.CAMERAS (and none of the pitch-only camera): what the earlier pins could not see"""
    seen = set()
    for scene, (box, osc) in world.items():
        for name in cc.GENERAL:
            for (w, h) in sizes_of(name):
                cam = cc.oracle_camera(rt, oracle, name, w, h, box, osc)
                if (bytes(cam), w, h) in seen:                    # the cameras that do not depend on the scene
                    continue
                seen.add((bytes(cam), w, h))
                ref = cc.numpy_points(cam, w, h)
                shares = {v: cc.differing_share(ref, cc.numpy_points(cam, w, h, v)) for v in ("association", "fused")}
                print(f"{scene} {name} {w}x{h}: association {shares['association']:.3f}, fused {shares['fused']:.3f}")
                assert shares["association"] >= 0.01 and shares["fused"] >= 0.01, (scene, name, w, h, shares)
    for (w, h, yaw) in RI.CAMERAS:
        cam = oracle.camera(w, h, yaw)
        ref = cc.numpy_points(cam, w, h)
        assert np.array_equal(u32(ref), u32(oracle.screen_points(cam, w, h)))
        for v in ("association", "fused"):
            assert cc.differing_share(ref, cc.numpy_points(cam, w, h, v)) == 0.0, (w, h, yaw, v)
    cam = cc.fly(oracle, 0, 96, 72)
    for v in ("association", "fused"):
        assert cc.differing_share(cc.numpy_points(cam, 96, 72), cc.numpy_points(cam, 96, 72, v)) == 0.0


def test_reproject_map_of_general_cameras_equals_its_restatement(rt, oracle, world):
    """rt_reproject_map (rt_reproject_layout.hpp: the ray matrix B of a camera and its inverse, in double) had yaw cameras only, like the
    frames: here every pair has two general matrices, against the numpy restatement tests/reproject_ref.py, bit for bit"""
    import reproject_ref as rr
    box, osc = world["cube.obj"]
    pairs = []
    for (w, h) in cc.SIZES:
        for k in (1, 2, 3, 4, 5, 6):
            _, _, yaw, pitch, t = RI.FLY_CAMERAS[k]
            prev = oracle.fly_camera(w, h, yaw - 0.03, pitch + 0.02, (t[0] + 0.02, t[1] - 0.01, t[2] + 0.03))
            pairs.append((cc.rt_camera(rt, cc.fly(oracle, k, w, h)), cc.rt_camera(rt, prev)))
        for name, k in (("sheared", 1), ("mirrored", 4), ("vporigin", 4), ("aspect1", 2)):
            pairs.append((cc.pair(rt, oracle, name, w, h, box, osc)[0], cc.rt_camera(rt, cc.fly(oracle, k, w, h))))
            pairs.append((pairs[-1][1], pairs[-1][0]))
    for cur, prev in pairs:
        got, want = rt.reproject_map(cur, prev), rr.reproject_map(cur, prev)
        assert want is not None and np.array_equal(u32(got), u32(want)), (list(cur.inv_view), list(prev.inv_view), got, want)
        assert not np.array_equal(u32(got), u32(rr.IDENTITY))


def test_cameras_see_what_their_names_say(rt, oracle, world, hits):
    for (scene, name, (w, h)), (ids, st) in sorted(hits.items()):
        share = float((ids >= 0).mean())
        print(f"{scene} {name} {w}x{h}: {share:.3f} of the pixels hit, {int(st.precull_tests - st.rays_primary)} culled")
        if name in cc.IN_VIEW:
            assert 0.10 <= share <= 0.90, (scene, name, w, h, share)
        elif name == "away":
            assert share == 0.0 and st.rays_primary == 0 and st.precull_tests == w * h, (scene, w, h, share, st.rays_primary)
        elif name == "inside":
            box, _ = world[scene]
            c = cc.oracle_camera(rt, oracle, name, w, h, box).center
            assert all(box[k] < c[k] < box[3 + k] for k in range(3))
            assert share > 0.0 and st.rays_primary == w * h, (scene, w, h, share)
        elif name == "closeup":
            assert share == 1.0 and np.unique(ids).size == 1, (scene, w, h, share, np.unique(ids))
        elif name == "corner":
            box, osc = world[scene]
            ys, xs = np.nonzero(ids >= 0)
            assert ys.size > 0 and xs.min() >= (w // 8) * 8 and ys.min() >= (h // 8) * 8, (scene, w, h, ys.size)
            rect = rt.primary_rect(cc.pair(rt, oracle, name, w, h, box, osc)[0], box, w, h)
            tx, ty = (w + 7) // 8, (h + 7) // 8
            assert rect[2] == tx and rect[3] == ty and rect[0] >= tx - 2 and rect[1] >= ty - 2, (scene, rect)
