"""The thin-lens camera of rt_set_lens (include/rt_mi355x.h) restated in numpy: the per-pixel hash, the lens table in double precision and
the six steps that turn a sub-sample's screen point into its ray -- float32 with an explicit cast after every operation, no FMA.

Test infrastructure only: the frames the GPU tests expect are built from these rays by the CPU oracle or by rt_trace_rays."""
import math

import numpy as np

RT_LENS_ROTATIONS = 64
F = np.float32
_M = 0xFFFFFFFF


def lens_hash(i, j):
    """the per-pixel scramble of output pixel (column i, frame row j), uint32 arithmetic"""
    h = ((i * 0x9E3779B1) & _M) ^ ((j * 0x85EBCA6B) & _M)
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & _M
    h ^= h >> 12
    h = (h * 0x297A2D39) & _M
    h ^= h >> 15
    return h


def lens_hash_array(i, j):
    """lens_hash for integer arrays"""
    i, j = np.asarray(i, np.uint64), np.asarray(j, np.uint64)
    m = np.uint64(_M)
    h = ((i * np.uint64(0x9E3779B1)) & m) ^ ((j * np.uint64(0x85EBCA6B)) & m)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m
    h ^= h >> np.uint64(15)
    return h


def rotation_and_point(i, j, sx, sy, n):
    """(r, k): the rotation and the lens point of sub-sample (sx, sy) of output pixel (i, j)"""
    h = lens_hash(i, j)
    return h >> 26, (sy * n + sx + ((h >> 8) & 0xFFFF)) % (n * n)


def concentric(u, v):
    """Shirley-Chiu concentric map of (u, v) in [-1, 1]^2 onto the unit disc (double)"""
    if u == 0.0 and v == 0.0:
        return 0.0, 0.0
    if abs(u) > abs(v):
        r, t = u, (math.pi / 4.0) * (v / u)
    else:
        r, t = v, (math.pi / 2.0) - (math.pi / 4.0) * (u / v)
    return r * math.cos(t), r * math.sin(t)


def lens_table_double(n):
    """T[r][k] in double precision, shape [RT_LENS_ROTATIONS, n*n, 2]"""
    t = np.zeros((RT_LENS_ROTATIONS, n * n, 2), np.float64)
    for k in range(n * n):
        x, y = concentric(2.0 * ((k % n + 0.5) / n) - 1.0, 2.0 * ((k // n + 0.5) / n) - 1.0)
        for r in range(RT_LENS_ROTATIONS):
            a = (math.pi / 2.0) * r / RT_LENS_ROTATIONS
            t[r, k] = (x * math.cos(a) - y * math.sin(a), x * math.sin(a) + y * math.cos(a))
    return t


def library_table(lib, n):
    """rt_lens_table: the LIBRARY's float table [RT_LENS_ROTATIONS, n*n, 2] (frames take it as data: libm's sin / cos may differ in the last place)"""
    import ctypes as C
    out = np.full((RT_LENS_ROTATIONS, n * n, 2), np.nan, np.float32)
    assert lib.rt_lens_table(n, out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    return out


def lens_ray(S, center, inv_view, aperture, focus, t):
    """steps 1, 2, 4, 5 for one sub-sample: screen point S, camera centre, inv_view[12], lens point t = T[r][k] -> (O, P, D), float32"""
    S, c, m = np.asarray(S, F), np.asarray(center, F), np.asarray(inv_view, F)
    ap, fo = F(aperture), F(focus)
    v = (S - c).astype(F)
    P = (c + (fo * v).astype(F)).astype(F)
    a, b = F(ap * F(t[0])), F(ap * F(t[1]))
    U, V = m[[0, 4, 8]], m[[1, 5, 9]]
    O = ((c + (a * U).astype(F)).astype(F) + (b * V).astype(F)).astype(F)
    D = (P - O).astype(F)
    return O, P, D


def lens_rays(S, center, inv_view, aperture, focus, T, n, rows=None):
    """every sub-sample ray of a frame.  S[H, W, n, n, 3] (S[j, i, sy, sx] = screenToWorld at the sub-sample's raster point), T the library's
    table for n, rows the frame row of each row of S (default 0..H-1) -> O, P, D of the same shape, float32"""
    S = np.asarray(S, F)
    H, W = S.shape[:2]
    c, m = np.asarray(center, F), np.asarray(inv_view, F)
    ap, fo = F(aperture), F(focus)
    rows = np.arange(H) if rows is None else np.asarray(rows)
    jj, ii, sy, sx = np.meshgrid(rows, np.arange(W), np.arange(n), np.arange(n), indexing="ij")
    h = lens_hash_array(ii, jj)
    r = (h >> np.uint64(26)).astype(np.int64)
    k = ((sy * n + sx).astype(np.int64) + ((h >> np.uint64(8)) & np.uint64(0xFFFF)).astype(np.int64)) % (n * n)
    t = np.asarray(T, F)[r, k]                                        # [H, W, n, n, 2]
    v = (S - c).astype(F)
    P = (c + (fo * v).astype(F)).astype(F)
    a, b = (ap * t[..., 0:1]).astype(F), (ap * t[..., 1:2]).astype(F)
    U, V = m[[0, 4, 8]], m[[1, 5, 9]]
    O = ((c + (a * U).astype(F)).astype(F) + (b * V).astype(F)).astype(F)
    D = (P - O).astype(F)
    return O, P, D
