"""Ambient occlusion as include/rt_mi355x.h defines it ("ambient occlusion"), restated in numpy float32 -- test infrastructure only.

Every float32 step is one numpy float32 operation (numpy rounds each on its own, there is no FMA), in the order the header writes; the
directions and rotations are computed in double and rounded once, as rt_ao_directions / rt_ao_rotation do.  Visibility is the CPU
checker's lightStrikes (OracleScene.light_strikes)."""
import math

import numpy as np

F = np.float32
MAX_GRID, ROTATIONS = 16, 64
M32 = 0xFFFFFFFF


def concentric_disc(u, v):
    """Shirley-Chiu, [-1, 1]^2 -> unit disc, the rule of rt_lens_table (double)"""
    if u == 0.0 and v == 0.0:
        return 0.0, 0.0
    if abs(u) > abs(v):
        r, t = u, (math.pi / 4.0) * (v / u)
    else:
        r, t = v, (math.pi / 2.0) - (math.pi / 4.0) * (u / v)
    return r * math.cos(t), r * math.sin(t)


def directions(m):
    """-> float32 (m * m, 3)"""
    out = np.empty((m * m, 3), F)
    for k in range(m * m):
        a, b = concentric_disc(2.0 * ((k % m + 0.5) / m) - 1.0, 2.0 * ((k // m + 0.5) / m) - 1.0)
        out[k] = (a, b, math.sqrt(max(0.0, 1.0 - a * a - b * b)))
    return out


def hash32(seed, i):
    h = (((i & M32) * 0x9E3779B1) & M32) ^ (((seed & M32) * 0x85EBCA6B) & M32)
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & M32
    h ^= h >> 12
    h = (h * 0x297A2D39) & M32
    h ^= h >> 15
    return h


def rotation_cs(r):
    a = (math.pi / 2.0) * r / ROTATIONS
    return F(math.cos(a)), F(math.sin(a))


def rotation(seed, i):
    """-> (r, c, s)"""
    r = hash32(seed, i) >> 26
    return (r,) + rotation_cs(r)


def rotation_steps(seed, i):
    """r of rotation(seed, i) for an array of indices (uint32 arithmetic carried in uint64)"""
    m = np.uint64(M32)
    i = np.asarray(i).reshape(-1).astype(np.uint64) & m
    h = ((i * np.uint64(0x9E3779B1)) & m) ^ np.uint64(((seed & M32) * 0x85EBCA6B) & M32)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m
    h ^= h >> np.uint64(15)
    return (h >> np.uint64(26)).astype(np.int64)


def frame(N):
    """N float32 (..., 3) -> (T, B), the branchless basis of Duff et al."""
    N = np.asarray(N, F)
    nx, ny, nz = N[..., 0], N[..., 1], N[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        sg = np.copysign(F(1.0), nz)
        a = F(-1.0) / (sg + nz)
        b = (nx * ny) * a
        T = np.stack([F(1.0) + (sg * (nx * nx)) * a, sg * b, -(sg * nx)], axis=-1)
        B = np.stack([b, sg + (ny * ny) * a, -ny], axis=-1)
    return T.astype(F), B.astype(F)


def is_point(N):
    """a normal whose three components are +-0 marks "no point" """
    return ~(np.asarray(N, F) == 0).all(axis=-1)


def segments(P, N, i, seed, m, radius):
    """far ends Q, float32 (n, K, 3), of the segments Q -> P of points P (n, 3) with normals N (n, 3) and call indices i (n,); rows of
    "no point" inputs hold what the arithmetic gives and are not to be used (is_point)"""
    P, N = np.asarray(P, F).reshape(-1, 3), np.asarray(N, F).reshape(-1, 3)
    n = P.shape[0]
    D = directions(m)
    x, y, z = D[None, :, 0], D[None, :, 1], D[None, :, 2]
    cs = np.array([rotation_cs(r) for r in range(ROTATIONS)], F)[rotation_steps(seed, i)].reshape(n, 2)
    c, s = cs[:, 0:1], cs[:, 1:2]
    T, B = frame(N)
    with np.errstate(invalid="ignore", over="ignore"):
        xr = c * x - s * y
        yr = s * x + c * y
        Q = np.empty((n, m * m, 3), F)
        for q in range(3):
            d = ((xr * T[:, q:q + 1]) + (yr * B[:, q:q + 1])) + (z * N[:, q:q + 1])
            Q[:, :, q] = P[:, q:q + 1] + F(radius) * d
    return Q


def hit_points(origins, dirs, faces, ts, face_normal):
    """rt_hit_points_device: -> (P, N) float32 (n, 3)"""
    o, d = np.asarray(origins, F).reshape(-1, 3), np.asarray(dirs, F).reshape(-1, 3)
    f, t = np.asarray(faces, np.int32).reshape(-1), np.asarray(ts, F).reshape(-1)
    fn = np.asarray(face_normal, F).reshape(-1, 3)
    ok = (f >= 0) & (f < fn.shape[0])
    g = np.where(ok, f, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        P = o + t[:, None] * d
        N = fn[g].copy()
        flip = (N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2] > 0
    N[flip] = -N[flip]
    P[~ok] = 0
    N[~ok] = 0
    return P.astype(F), N.astype(F)


def counts(oracle_scene, P, N, seed, m, radius, i=None):
    """open, uint16 (n,): the visible segments per point by the CPU checker's lightStrikes"""
    P, N = np.asarray(P, F).reshape(-1, 3), np.asarray(N, F).reshape(-1, 3)
    n = P.shape[0]
    i = np.arange(n) if i is None else np.asarray(i)
    Q = segments(P, N, i, seed, m, radius)
    live = is_point(N)
    out = np.full(n, m * m, np.uint16)
    for k in range(n):
        if live[k]:
            out[k] = int(oracle_scene.light_strikes(P[k], Q[k])[1].sum())
    return out


def ao_of(open_, m):
    """ao = (float)open / (float)K"""
    return (np.asarray(open_).astype(F) / F(m * m)).astype(F)


def camera_points(orc, oracle_scene, width=48, height=32, yaw=0.4):
    """the fixed point sets of the tests: the closest hits of the width x height default camera at `yaw`, in raster order over the hits
    only -> (origins, dirs, faces, ts) of ALL rays and (P, N) of the hits"""
    cam = orc.camera(width, height, yaw)
    org = np.array(list(cam.center), F)
    o, d, f, t = [], [], [], []
    for j in range(height):
        for i in range(width):
            dd = (orc.screen_to_world(cam, i, j) - org).astype(F)
            ff, tt = oracle_scene.closest_hit(org, dd)
            o.append(org); d.append(dd); f.append(ff); t.append(tt if ff >= 0 else -1.0)
    o, d, f, t = np.array(o, F), np.array(d, F), np.array(f, np.int32), np.array(t, F)
    P, N = hit_points(o, d, f, t, oracle_scene.arrays()["face_normal"])
    hit = f >= 0
    return (o, d, f, t), (P[hit], N[hit])
