"""The camera motion blur of rt_set_shutter (include/rt_mi355x.h) restated in numpy: the time of a sub-sample, the camera at that time, the
screen point of a per-sample camera and the ray (pinhole, or the thin lens of rt_set_lens on that camera) -- float32 with an explicit cast
after every operation, no FMA.

Test infrastructure only: the frames the GPU tests expect are built from these rays by the CPU oracle or by rt_trace_rays."""
import numpy as np

import lens_ref

F = np.float32
_M = 0xFFFFFFFF
G_XOR = 0x68E31DA4
U_SCALE = F(1.0 / 65536.0)          # 2^-16


def _mix(v):
    v ^= v >> 15
    v = (v * 0x2C1B3C6D) & _M
    v ^= v >> 12
    v = (v * 0x297A2D39) & _M
    v ^= v >> 15
    return v


def shutter_g(i, j):
    """the time scramble of output pixel (column i, frame row j): the lens's h, mixed once more"""
    return _mix(lens_ref.lens_hash(i, j) ^ G_XOR)


def shutter_g_array(i, j):
    g = lens_ref.lens_hash_array(i, j) ^ np.uint64(G_XOR)
    m = np.uint64(_M)
    g ^= g >> np.uint64(15)
    g = (g * np.uint64(0x2C1B3C6D)) & m
    g ^= g >> np.uint64(12)
    g = (g * np.uint64(0x297A2D39)) & m
    g ^= g >> np.uint64(15)
    return g


def slot_u_t(i, j, sx, sy, n):
    """(slot, u, t) of sub-sample (sx, sy) of output pixel (i, j)"""
    g = shutter_g(i, j)
    nn = n * n
    slot = (sx * n + sy + (g & 0xFFFF)) % nn
    u = F(F(g >> 16) * U_SCALE)
    t = F(F(F(slot) + u) / F(nn))
    return slot, u, t


def shutter_time(i, j, sx, sy, n):
    return slot_u_t(i, j, sx, sy, n)[2]


def shutter_times(W, n, rows):
    """t[len(rows), W, n, n] (index [row, i, sy, sx]) for the frame rows `rows`"""
    jj, ii, sy, sx = np.meshgrid(np.asarray(rows), np.arange(W), np.arange(n), np.arange(n), indexing="ij")
    g = shutter_g_array(ii, jj)
    nn = n * n
    slot = ((sx * n + sy).astype(np.int64) + (g & np.uint64(0xFFFF)).astype(np.int64)) % nn
    u = ((g >> np.uint64(16)).astype(F) * U_SCALE).astype(F)
    return ((slot.astype(F) + u).astype(F) / F(nn)).astype(F)


def pose(cam):
    """the 15 pose values of a camera struct (center[3] then inv_view[12]) as float32"""
    return np.array(list(cam.center) + list(cam.inv_view), F)


def shutter_pose(open15, close15, t):
    """K(t): q_open where d == 0, else q_open + t*d (multiply, then add).  t a scalar or an array [...]; returns [..., 15]"""
    o, c = np.asarray(open15, F), np.asarray(close15, F)
    d = (c - o).astype(F)
    t = np.asarray(t, F)[..., None]
    with np.errstate(invalid="ignore", over="ignore"):
        moved = (o + (t * d).astype(F)).astype(F)
    return np.where(d == 0, o, moved).astype(F)


def shutter_camera(open_cam, close_cam, t):
    """K(t) as a camera struct of open's type: open's fovy / aspect / viewport"""
    k = type(open_cam)()
    q = shutter_pose(pose(open_cam), pose(close_cam), F(t))
    for a in range(3):
        k.center[a] = float(q[a])
    for a in range(12):
        k.inv_view[a] = float(q[3 + a])
    k.fovy, k.aspect = open_cam.fovy, open_cam.aspect
    for a in range(4):
        k.viewport[a] = open_cam.viewport[a]
    return k


def screen_points(m, n0, n1):
    """screenToWorld's last step with a matrix per sample: m[..., 12] (3 x 4 row-major), n0 / n1 [...] the raster point's camera-independent
    terms (normalised x times aspect*scale, normalised y times scale) -> [..., 3], in the order ((m0*n0 + m1*n1) + m2*(-1)) + m3*1"""
    m, n0, n1 = np.asarray(m, F), np.asarray(n0, F), np.asarray(n1, F)
    out = np.empty(m.shape[:-1] + (3,), F)
    for r in range(3):
        a = ((m[..., 4 * r] * n0).astype(F) + (m[..., 4 * r + 1] * n1).astype(F)).astype(F)
        a = (a + (m[..., 4 * r + 2] * F(-1.0)).astype(F)).astype(F)
        out[..., r] = (a + (m[..., 4 * r + 3] * F(1.0)).astype(F)).astype(F)
    return out


def lens_rays_per_sample(S, K, aperture, focus, tab):
    """steps 1, 2, 4, 5 of rt_set_lens with a camera per sample: S[..., 3], K[..., 15], tab[..., 2] the lens point of each sample -> O, P, D"""
    S, K, tab = np.asarray(S, F), np.asarray(K, F), np.asarray(tab, F)
    ap, fo = F(aperture), F(focus)
    c = K[..., 0:3]
    v = (S - c).astype(F)
    P = (c + (fo * v).astype(F)).astype(F)
    a, b = (ap * tab[..., 0:1]).astype(F), (ap * tab[..., 1:2]).astype(F)
    U, V = K[..., [3, 7, 11]], K[..., [4, 8, 12]]
    O = ((c + (a * U).astype(F)).astype(F) + (b * V).astype(F)).astype(F)
    return O, P, (P - O).astype(F)


def shutter_rays(n0, n1, open15, close15, n, rows, lens=None):
    """every sub-sample ray of a frame.  n0, n1 [H, W, n, n] (index [row, i, sy, sx]): the raster terms of screen_points; rows: the frame row of
    each row; lens: None or (aperture, focus, T) with T the library's table for n -> O, P, D [H, W, n, n, 3], float32.  P is the second point
    of the pre-cull segment: the screen point (pinhole) or the focus point (lens)."""
    H, W = n0.shape[:2]
    t = shutter_times(W, n, rows)
    K = shutter_pose(open15, close15, t)                                  # [H, W, n, n, 15]
    S = screen_points(K[..., 3:15], n0, n1)
    if lens is None:
        O = np.ascontiguousarray(K[..., 0:3])
        return O, S, (S - O).astype(F)
    aperture, focus, T = lens
    jj, ii, sy, sx = np.meshgrid(np.asarray(rows), np.arange(W), np.arange(n), np.arange(n), indexing="ij")
    h = lens_ref.lens_hash_array(ii, jj)
    r = (h >> np.uint64(26)).astype(np.int64)
    k = ((sy * n + sx).astype(np.int64) + ((h >> np.uint64(8)) & np.uint64(0xFFFF)).astype(np.int64)) % (n * n)
    return lens_rays_per_sample(S, K, aperture, focus, np.asarray(T, F)[r, k])


def shutter_ray(S, K15, lens=None, lens_point=None):
    """one sub-sample, scalar form: screen point S of K(t), K(t)'s 15 values -> (O, P, D); the lens steps are lens_ref.lens_ray's"""
    S, K15 = np.asarray(S, F), np.asarray(K15, F)
    if lens is None:
        O = K15[0:3].copy()
        return O, S, (S - O).astype(F)
    return lens_ref.lens_ray(S, K15[0:3], K15[3:15], lens[0], lens[1], lens_point)
