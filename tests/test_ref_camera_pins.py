"""Reference pins of pitched and translated cameras: tests/golden/ref_camera_pins.npz holds OUTPUTS of the reference's own Camera
(tucano/camera.hpp compiled in place, oracle/ref_probe2.cpp `fly`, recorded by oracle/make_ref_camera_fixtures.py) under the view matrix
Flycamera::updateViewMatrix composes from yaw, pitch and translation_vector -- ref_inputs.FLY_CAMERAS.

tests/golden/ref_pins.npz pins yaw cameras only, whose inv_view has m[1] = m[4] = m[6] = m[9] = 0 and m[5] = 1: neither the association
of the sums of screenToWorld nor that of the 3x3 inverse and of the inverse's translation can show there.  Here they do.
CPU tests pin the ORACLE (camera and screen_to_world) and the library's host rt_screen_to_world on every pixel; the `-m gpu` test pins
the device's primary-ray generator (rt_primary_points) to the same numbers."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import camera_cases as cc
import ref_inputs as RI

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = np.load(os.path.join(HERE, "golden", "ref_camera_pins.npz"))
K = range(len(RI.FLY_CAMERAS))


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fly(oracle, k):
    W, H, yaw, pitch, t = RI.FLY_CAMERAS[k]
    return W, H, oracle.fly_camera(W, H, yaw, pitch, t)


def pinned_rt_camera(rt, k):
    """the rt_camera of FLY_CAMERAS[k] from the RECORDED centre and inverse view matrix: no oracle in between"""
    W, H = RI.FLY_CAMERAS[k][:2]
    cam = rt.default_camera(W, H)
    for i in range(3):
        cam.center[i] = PINS[f"fly{k}_center"][i]
    for i in range(12):
        cam.inv_view[i] = PINS[f"fly{k}_inv_view"][i]
    return W, H, cam


def assert_points_equal_pins(out, k):
    assert np.array_equal(u32(out.reshape(-1)[::1009]), u32(PINS[f"fly{k}_every1009"])), k
    assert hashlib.sha256(np.ascontiguousarray(out, np.float32).tobytes()).hexdigest() == str(PINS[f"fly{k}_sha"]), k


def test_inputs_are_the_recorded_ones_and_cover_what_they_must():
    assert RI.sha(RI.fly_camera_inputs()) == str(PINS["fly_in_sha"]), "tests/ref_inputs.py drifted from the inputs the fixture was generated from"
    zero = (0.0, 0.0, 0.0)
    assert len(RI.FLY_CAMERAS) >= 6
    assert any(yaw == 0.0 and pitch != 0.0 for (_, _, yaw, pitch, _) in RI.FLY_CAMERAS)                         # pitch alone
    assert any(yaw != 0.0 and pitch > 0.0 for (_, _, yaw, pitch, _) in RI.FLY_CAMERAS)
    assert any(yaw != 0.0 and pitch < 0.0 for (_, _, yaw, pitch, _) in RI.FLY_CAMERAS)
    assert any(abs(pitch) > 1.0 for (_, _, _, pitch, _) in RI.FLY_CAMERAS)
    assert any(pitch != 0.0 and t != zero for (_, _, _, pitch, t) in RI.FLY_CAMERAS)
    assert any(yaw != 0.0 and pitch != 0.0 and t == zero for (_, _, yaw, pitch, t) in RI.FLY_CAMERAS)            # rotation alone
    assert sum((W, H) == (1920, 1080) for (W, H, _, _, _) in RI.FLY_CAMERAS) == 1
    assert all(W <= 160 and H <= 90 for (W, H, _, _, _) in RI.FLY_CAMERAS if (W, H) != (1920, 1080))
    assert any(W % 8 and H % 8 for (W, H, _, _, _) in RI.FLY_CAMERAS)


def test_yaw_pins_are_untouched():
    """this fixture is an addition: the yaw pins every earlier claim rests on are the bytes they were"""
    data = open(os.path.join(HERE, "golden", "ref_pins.npz"), "rb").read()
    assert hashlib.sha256(data).hexdigest() == REF_PINS_SHA256


REF_PINS_SHA256 = "acb9ebcaacb2e6972124fba76f63de01200e08f15b42aa00e642e1ca9dd93776"


@pytest.mark.parametrize("yaw", [c[2] for c in RI.CAMERAS] + [-0.7, 0.05, 2.9, -3.1])
def test_yaw_camera_is_the_fly_camera_without_pitch_and_translation(oracle, yaw):
    for (w, h) in ((256, 256), (61, 45)):
        assert bytes(oracle.camera(w, h, yaw)) == bytes(oracle.fly_camera(w, h, yaw, 0.0, (0.0, 0.0, 0.0))), (w, h, yaw)


@pytest.mark.parametrize("k", K)
def test_oracle_camera_equals_reference(oracle, k):
    """getCenter (camera.hpp:115-118) and getViewMatrix().inverse() (camera.hpp:170): Eigen's 3x3 inverse by cofactors and
    translation = -linear_inv * translation, on a rotation matrix without structural zeros"""
    _, _, cam = fly(oracle, k)
    assert np.array_equal(u32(list(cam.center)), u32(PINS[f"fly{k}_center"])), (list(cam.center), PINS[f"fly{k}_center"])
    assert np.array_equal(u32(list(cam.inv_view)), u32(PINS[f"fly{k}_inv_view"])), (list(cam.inv_view), PINS[f"fly{k}_inv_view"])


@pytest.mark.parametrize("k", K)
def test_oracle_screen_to_world_equals_reference(oracle, k):
    """Camera::screenToWorld (camera.hpp:155-173) on EVERY pixel: Eigen's Affine3f * Vector3f"""
    W, H, cam = fly(oracle, k)
    out = oracle.screen_points(cam, W, H)
    assert_points_equal_pins(out, k)
    # the bulk entry point is the per-pixel one
    buf = (C.c_float * 3)()
    for (i, j) in ((0, 0), (W - 1, H - 1), (W // 3, H // 2)):
        oracle.lib.orc_screen_to_world(C.byref(cam), float(i), float(j), buf)
        assert np.array_equal(u32(list(buf)), u32(out[j, i]))


@pytest.mark.parametrize("k", K)
def test_numpy_restatement_equals_reference(oracle, k):
    """the restatement the camera set's ABI-only cameras are checked with (camera_cases.numpy_points) is itself pinned"""
    W, H, cam = fly(oracle, k)
    assert_points_equal_pins(cc.numpy_points(cam, W, H), k)


@pytest.mark.parametrize("k", K)
def test_host_screen_to_world_equals_reference(rt, oracle, k):
    """the library's host function rt_screen_to_world (host_scene.cpp: screen_to_world) on every pixel"""
    W, H, cam = pinned_rt_camera(rt, k)
    assert bytes(cam) == bytes(fly(oracle, k)[2])
    f = rt.load_library().rt_screen_to_world
    out = np.empty((H, W, 3), np.float32)
    flat = out.reshape(-1, 3)
    buf = (C.c_float * 3)()
    ref = C.byref(cam)
    n = 0
    for j in range(H):
        fj = float(j)
        for i in range(W):
            f(ref, float(i), fj, buf)
            flat[n] = buf
            n += 1
    assert_points_equal_pins(out, k)


# ---------------------------------------------------------------------------------------------------------------- GPU: the HIP path
@pytest.fixture(scope="module")
def gpu_ctx(rt):
    hs = rt.HostScene(os.path.join(HERE, "golden", "scenes", "cube.obj"), 1000, 15)
    ctx = rt.Context(0)
    ctx.upload(hs)
    yield ctx
    ctx.close()
    hs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_gpu_primary_points_equal_reference(rt, gpu_ctx, k):
    """rt_primary_points = the device's primary-ray generator (screen_point) on every pixel, against Camera::screenToWorld"""
    ctx = gpu_ctx
    W, H, cam = pinned_rt_camera(rt, k)
    out = np.zeros((H, W, 3), np.float32)
    st = ctx.lib.rt_primary_points(ctx.handle, C.byref(cam), W, H, out.ctypes.data_as(C.c_void_p))
    rt.capi.check(ctx.lib, ctx.handle, st, "rt_primary_points")
    assert_points_equal_pins(out, k)
