"""General cameras for the frame tests (test infrastructure): every named camera as the oracle's struct and an rt_camera of the same bits.

The yaw cameras every other frame test uses have a degenerate inv_view (m[1] = m[4] = m[6] = m[9] = 0, m[5] = 1): the sums that turn a
raster point into a world point never run as written.  The cameras here have no structural zero: the fly cameras of
ref_inputs.FLY_CAMERAS (Flycamera::updateViewMatrix with yaw, pitch and translation_vector, pinned against the reference by
tests/golden/ref_camera_pins.npz), cameras placed where the frame path changes its route (inside the root box, facing away, the model in
the last partial tile, one face over the whole frame) and cameras the reference cannot produce but the ABI accepts.

numpy_points() restates Camera::screenToWorld (camera.hpp:155-173) in numpy float32, one rounded operation per line, with two
deliberately wrong variants; tests/test_camera_cases.py holds the oracle, the library's host function and that restatement against each
other and checks that the set is not vacuous.
"""
import ctypes as C
import math
import os

import numpy as np

import ref_inputs as RI

F = np.float32
D = np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")
SCENE_NAMES = ("cube.obj", "mixed", "dodgeColorTest.obj")
SIZES = ((96, 72), (61, 45))
# the fly cameras of the reference pins that are placed so that the model is in view (a translation_vector other than 0), by their index
FLY = tuple(f"fly{k}" for k, c in enumerate(RI.FLY_CAMERAS) if c[4] != (0.0, 0.0, 0.0))
ABI_ONLY = ("sheared", "mirrored", "fovy20", "fovy120", "aspect1", "vporigin")
PLACED = ("inside", "away", "corner", "closeup")
NAMES = FLY + PLACED + ABI_ONLY
# the cameras whose frames show the model among background (10 % .. 90 % of the pixels hit)
IN_VIEW = FLY + ABI_ONLY
# the cameras whose matrix must be general: no zero and no +-1 among the nine linear entries, and both wrong restatements of the sum show.
# Beside the three the placement exempts, a fly camera with yaw 0 cannot be: pitch alone is a rotation about X, whose matrix keeps
# m[1] = m[2] = m[4] = m[8] = 0 and m[0] = 1 -- every sum has at most two terms that are not exact, as on a yaw camera.  It is pinned and
# rendered all the same.
GENERAL = tuple(n for n in NAMES if n not in ("inside", "away", "closeup") and not (n in FLY and RI.FLY_CAMERAS[int(n[3:])][2] == 0.0))


def scene_path(name, tmpdir):
    if name == "mixed":
        import scenes_gen
        return scenes_gen.mixed_materials(str(tmpdir))
    return os.path.join(SCENES, name)


# ------------------------------------------------------------------------------------------ construction
def aim(oracle, w, h, yaw, pitch, target, dist):
    """the fly camera of (yaw, pitch) whose translation_vector puts `target` on the optical axis at distance `dist`.  The centre of a fly
    camera is (0, 0, 2) - translation_vector whatever its rotation (flycamera.hpp:186-190), the axis is -(third column of inv_view)."""
    m = np.array(list(oracle.fly_camera(w, h, yaw, pitch).inv_view), F)
    axis = -np.array([m[2], m[6], m[10]], D)
    centre = np.asarray(target, D) - dist * axis
    return oracle.fly_camera(w, h, yaw, pitch, tuple(F(x) for x in (np.array([0.0, 0.0, 2.0]) - centre)))


def box_centre(box):
    return np.array([0.5 * (box[k] + box[3 + k]) for k in range(3)], D)


def fly(oracle, k, w, h):
    _, _, yaw, pitch, t = RI.FLY_CAMERAS[k]
    return oracle.fly_camera(w, h, yaw, pitch, t)


def oracle_camera(rt, oracle, name, w, h, box, osc=None):
    """the oracle's struct of camera `name` for a w x h frame of a scene whose root box is `box` (min3, max3); `closeup` needs the oracle's
    scene `osc` for the triangles"""
    mid = box_centre(box)
    size = max(box[3 + k] - box[k] for k in range(3))
    if name in FLY:
        return fly(oracle, int(name[3:]), w, h)
    if name == "inside":
        return aim(oracle, w, h, 0.4, -0.3, mid + 0.1 * size, 0.0)
    if name == "away":
        return aim(oracle, w, h, 0.5, 0.35, mid, -2.0)
    if name == "corner":
        return corner_camera(oracle, w, h, box)
    if name == "closeup":
        return closeup_camera(oracle, w, h, osc)
    if name == "sheared":
        a, b = rt_camera(rt, fly(oracle, 1, w, h)), rt_camera(rt, fly(oracle, 4, w, h))
        out = rt.capi.rt_camera()
        assert rt.load_library().rt_shutter_camera(C.byref(a), C.byref(b), 0.37, C.byref(out)) == 0
        return ocamera_of(out)
    # a narrow and a wide field of view, at the distances that keep the model a part of the frame
    if name == "fovy20":
        cam = aim(oracle, w, h, -0.8, -0.5, mid, 4.0 * size)
        cam.fovy = 20.0
        return cam
    if name == "fovy120":
        cam = aim(oracle, w, h, 0.6, 0.35, mid, 0.7 * size)
        cam.fovy = 120.0
        return cam
    cam = fly(oracle, 2 if name == "aspect1" else 4, w, h)
    if name == "mirrored":
        for r in range(3):
            cam.inv_view[4 * r] = -cam.inv_view[4 * r]
    elif name == "aspect1":
        cam.aspect = 1.0
    elif name == "vporigin":
        cam.viewport[0], cam.viewport[1] = -0.25, 0.5
    else:
        raise KeyError(name)
    return cam


def corner_camera(oracle, w, h, box, dist=16.0, yaw=0.6, pitch=0.35):
    """looks past the model so that it shows within the last tile column and the last tile row, both partial (w and h are no multiples
    of 8): the middle of the box is put on the ray of the raster point (w - 2.5, h - 2.5), far enough away to span a pixel or two"""
    assert w % 8 > 2 and h % 8 > 2
    m = np.array(list(oracle.fly_camera(w, h, yaw, pitch).inv_view), D).reshape(3, 4)[:, :3]
    t30 = math.tan(math.radians(30.0))
    x = ((w - 2.5) - 0.5 * w) / (0.5 * h) * t30
    y = -((h - 2.5) - 0.5 * h) / (0.5 * h) * t30
    centre = box_centre(box) - m @ (dist * np.array([x, y, -1.0]))
    return oracle.fly_camera(w, h, yaw, pitch, tuple(F(v) for v in (np.array([0.0, 0.0, 2.0]) - centre)))


def closeup_camera(oracle, w, h, osc):
    """a few hundredths of an edge above the centroid of the scene's largest triangle, looking at it 0.2 rad off its normal both ways:
    that one face covers the whole frame"""
    a = osc.arrays()
    tri = a["wverts"][a["face_vid"].astype(np.int64)].astype(D)                  # [faces, 3, 3]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    f = int(np.argmax(np.linalg.norm(nrm, axis=1)))
    g = tri[f].mean(axis=0)
    edge = min(np.linalg.norm(tri[f, k] - tri[f, (k + 1) % 3]) for k in range(3))
    n = nrm[f] / np.linalg.norm(nrm[f])
    for side in (1.0, -1.0):
        # the camera's backward axis is (sin yaw cos pitch, -sin pitch, cos yaw cos pitch)
        yaw, pitch = math.atan2(side * n[0], side * n[2]) + 0.2, -math.asin(side * n[1]) - 0.2
        cam = aim(oracle, w, h, yaw, pitch, g, 0.04 * edge)
        hit, _ = osc.closest_hit(np.array(list(cam.center), F), (g - np.array(list(cam.center), D)).astype(F))
        if hit == f:
            return cam
    raise AssertionError("the largest triangle is hidden from both sides")


def rt_camera(rt, ocam):
    """an rt_camera with the oracle struct's bits, field by field"""
    cam = rt.capi.rt_camera()
    for k in range(3):
        cam.center[k] = ocam.center[k]
    for k in range(12):
        cam.inv_view[k] = ocam.inv_view[k]
    cam.fovy, cam.aspect = ocam.fovy, ocam.aspect
    for k in range(4):
        cam.viewport[k] = ocam.viewport[k]
    assert bytes(cam) == bytes(ocam)
    return cam


def ocamera_of(cam):
    import oracle_lib
    o = oracle_lib.ocamera()
    for k in range(3):
        o.center[k] = cam.center[k]
    for k in range(12):
        o.inv_view[k] = cam.inv_view[k]
    o.fovy, o.aspect = cam.fovy, cam.aspect
    for k in range(4):
        o.viewport[k] = cam.viewport[k]
    assert bytes(cam) == bytes(o)
    return o


def pair(rt, oracle, name, w, h, box, osc=None):
    o = oracle_camera(rt, oracle, name, w, h, box, osc)
    return rt_camera(rt, o), o


# ------------------------------------------------------------------------------------------ the restatement
def numpy_points(cam, w, h, variant="reference"):
    """Camera::screenToWorld (camera.hpp:155-173, getPerspectiveScale :263-266) of every pixel, [h, w, 3] float32.  Every line is one
    rounded operation: float32 where the reference computes in float, float64 where it computes in double.
    variant "association": the sum as (a + (b + c)) + d; "fused": the two inner additions as single-rounding multiply-adds (the exact
    product of two float32 is a float64; the sum is rounded once to float64 and once more to float32).  Both are WRONG on purpose."""
    vp = [F(cam.viewport[k]) for k in range(4)]
    m = [F(cam.inv_view[k]) for k in range(12)]
    i = np.arange(w, dtype=F)[None, :]
    j = np.arange(h, dtype=F)[:, None]
    di = i - vp[0]                                   # float
    dj = j - vp[1]                                   # float
    x = 2.0 * di.astype(D)                           # double from here
    x = x / D(vp[2])
    x = x - 1.0
    y = 2.0 * dj.astype(D)
    y = y / D(vp[3])
    y = 1.0 - y
    n0 = x.astype(F)                                 # Vector3f(...)
    n1 = y.astype(F)
    n2 = F(-1.0)
    half = F(cam.fovy) / F(2.0)                      # float
    rad = D(half) * (math.pi / D(F(180.0)))          # double
    persp = F(1.0 / math.tan(rad))                   # float getPerspectiveScale()
    scale = F(1.0 / D(persp))                        # float scale = 1.0 / ...
    ks = F(cam.aspect) * scale
    n0 = n0 * ks
    n1 = n1 * scale
    n0, n1 = np.broadcast_to(n0, (h, w)), np.broadcast_to(n1, (h, w))
    out = np.empty((h, w, 3), F)
    for r in range(3):
        a = m[4 * r] * n0
        b = m[4 * r + 1] * n1
        c = m[4 * r + 2] * n2
        d = m[4 * r + 3] * F(1.0)
        if variant == "reference":
            s = a + b
            s = s + c
            s = s + d
        elif variant == "association":
            s = b + c
            s = a + s
            s = s + d
        elif variant == "fused":
            s = (D(m[4 * r + 1]) * n1.astype(D) + a.astype(D)).astype(F)
            s = (D(m[4 * r + 2]) * D(n2) + s.astype(D)).astype(F)
            s = s + d
        else:
            raise KeyError(variant)
        assert s.dtype == F
        out[:, :, r] = s
    return out


def differing_share(a, b):
    """share of pixels on which at least one bit of the world point differs"""
    return float((a.view(np.uint32) != b.view(np.uint32)).any(axis=2).mean())


def linear_part(cam):
    return np.array([cam.inv_view[4 * r + k] for r in range(3) for k in range(3)], F)
