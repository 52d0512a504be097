"""The temporal reprojection defined in include/rt_mi355x.h (rt_reproject_device, rt_reproject_map) restated: the map in Python floats
(doubles), operation by operation in the header's order with math.tan, and the operator in numpy float32 -- every operation one np.float32
array operation, rounded on its own, in the header's order; a tap is evaluated for the whole image at once (the order of the four taps and of
the three guides is what the definition fixes, not the order of the pixels).  The guide of a pixel and the squared distances are the
denoiser's (tests/denoise_ref.py).

Test infrastructure only."""
import math

import numpy as np

import denoise_ref as dr

F = np.float32
MAX_HISTORY = 255
INF = float("inf")
IDENTITY = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F)


class Params:
    """rt_reproject_params"""

    def __init__(self, max_history=MAX_HISTORY, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF):
        self.max_history = int(max_history)
        self.sigma_normal, self.sigma_depth, self.sigma_albedo = (F(s) for s in (sigma_normal, sigma_depth, sigma_albedo))

    def sigmas(self):
        return self.sigma_normal, self.sigma_depth, self.sigma_albedo

    def valid(self):
        return 1 <= self.max_history <= MAX_HISTORY and all(s > 0 for s in self.sigmas())


def scales(p):
    """(sn2, sz2, sa2), each sigma squared once"""
    with np.errstate(all="ignore"):
        return F(p.sigma_normal * p.sigma_normal), F(p.sigma_depth * p.sigma_depth), F(p.sigma_albedo * p.sigma_albedo)


# ---------------------------------------------------------------------------------------------------------------- the map
class Cam:
    """the fields of an rt_camera as float32 values (from any object with center, inv_view, fovy, aspect, viewport)"""

    def __init__(self, cam):
        self.center = [F(v) for v in cam.center]
        self.inv_view = [F(v) for v in cam.inv_view]
        self.fovy, self.aspect = F(cam.fovy), F(cam.aspect)
        self.viewport = [F(v) for v in cam.viewport]

    def fields(self):
        return self.center + self.inv_view + [self.fovy, self.aspect] + self.viewport

    def raw(self):
        return np.array(self.fields(), F).tobytes()


def ray_matrix(c):
    """B [3][3] in Python floats: D(x, y) = screenToWorld(x, y) - center = B (x, y, 1)^T"""
    persp = F(1.0 / math.tan(float(F(c.fovy / F(2.0))) * (math.pi / 180.0)))
    scale = F(1.0 / float(persp))
    sc, as_ = float(scale), float(F(c.aspect * scale))
    v0, v1, v2, v3 = (float(v) for v in c.viewport)
    ax, bx = (2.0 / v2) * as_, ((-2.0 * v0) / v2 - 1.0) * as_
    ay, by = (-2.0 / v3) * sc, (1.0 + (2.0 * v1) / v3) * sc
    B = []
    for r in range(3):
        m0, m1, m2, t = (float(v) for v in c.inv_view[r * 4:r * 4 + 4])
        B.append([m0 * ax, m1 * ay, (((m0 * bx + m1 * by) - m2) + t) - float(c.center[r])])
    return B


def cofactor3(m, i, j):
    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
    return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1]


def mat3_inverse(m):
    """the inverse by cofactors in mat3_inverse's order; None for a determinant that is 0 or not finite"""
    c0, c1, c2 = cofactor3(m, 0, 0), cofactor3(m, 1, 0), cofactor3(m, 2, 0)
    det = c0 * m[0][0] + (c1 * m[1][0] + c2 * m[2][0])
    if det == 0.0 or not math.isfinite(det):
        return None
    invdet = 1.0 / det
    return [[c0 * invdet, c1 * invdet, c2 * invdet],
            [cofactor3(m, 0, 1) * invdet, cofactor3(m, 1, 1) * invdet, cofactor3(m, 2, 1) * invdet],
            [cofactor3(m, 0, 2) * invdet, cofactor3(m, 1, 2) * invdet, cofactor3(m, 2, 2) * invdet]]


def reproject_map(cur, prev, double=False):
    """rt_reproject_map -> float32 (3, 4), or None where the call returns RT_ERR_INVALID.  double: the entries before the cast, and no
    identity rule (what the tests compare positions against)"""
    a, b = Cam(cur), Cam(prev)
    if not all(math.isfinite(float(v)) for v in a.fields() + b.fields()):
        return None
    if 0.0 in (float(a.viewport[2]), float(a.viewport[3]), float(b.viewport[2]), float(b.viewport[3])):
        return None
    if mat3_inverse([[float(b.inv_view[r * 4 + k]) for k in range(3)] for r in range(3)]) is None:
        return None
    with np.errstate(all="ignore"):
        Bc, Bp = ray_matrix(a), ray_matrix(b)
    I = mat3_inverse(Bp)
    if I is None:
        return None
    if a.raw() == b.raw() and not double:
        return IDENTITY.copy()
    d = [float(a.center[k]) - float(b.center[k]) for k in range(3)]
    m = []
    for r in range(3):
        row = [I[r][0] * d[0] + (I[r][1] * d[1] + I[r][2] * d[2])]
        row += [I[r][0] * Bc[0][k] + (I[r][1] * Bc[1][k] + I[r][2] * Bc[2][k]) for k in range(3)]
        m.append(row)
    if double:
        return np.array(m, np.float64)
    with np.errstate(all="ignore"):
        out = np.array(m, np.float64).astype(F)
    return out if np.isfinite(out).all() else None


# ---------------------------------------------------------------------------------------------------------------- the operator
def project(m, width, rows, z):
    """step 2 for every pixel: (x', y', zr, den) float32 [rows, width] from the map m (3, 4) and the depths z [rows, width]"""
    m = np.asarray(m, F).reshape(3, 4)
    xf, yf = np.arange(width).astype(F)[None, :], np.arange(rows).astype(F)[:, None]
    with np.errstate(all="ignore"):
        rho = (F(1.0) / z).astype(F)
        num = []
        for r in range(3):
            lin = (((xf * m[r, 1]).astype(F) + (yf * m[r, 2]).astype(F)).astype(F) + m[r, 3]).astype(F)
            num.append(((m[r, 0] * rho).astype(F) + lin).astype(F))
        den = num[2]
        return (num[0] / den).astype(F), (num[1] / den).astype(F), (z * den).astype(F), den


def reproject(cur, g_cur, hist, g_hist, len_hist, m, p, want_taps=False):
    """the operator: cur, hist [rows, width, C] (or [rows, width] for one channel), g_cur, g_hist [rows, width, 8], len_hist uint8
    [rows, width], m (3, 4) -> (out in cur's shape, len_out uint8 [rows, width]); want_taps: also the number of live taps per pixel"""
    assert p.valid()
    a = np.asarray(cur, F)
    flat = a.ndim == 2
    Cu = a[..., None] if flat else a
    Hi = np.asarray(hist, F)
    Hi = Hi[..., None] if flat else Hi
    g_cur, g_hist = np.asarray(g_cur, F), np.asarray(g_hist, F)
    len_hist = np.asarray(len_hist, np.uint8)
    rows, width = g_cur.shape[:2]
    ch = Cu.shape[2]
    assert Cu.shape == Hi.shape == (rows, width, ch) and ch in (1, 3) and g_cur.shape == g_hist.shape == (rows, width, 8)
    assert len_hist.shape == (rows, width) and np.isfinite(np.asarray(m, F)).all()
    if rows == 0:
        out = np.zeros(a.shape, F)
        return (out, np.zeros((0, width), np.uint8)) + ((np.zeros((0, width), np.int32),) if want_taps else ())
    gp, gq = dr.guide(g_cur), dr.guide(g_hist)
    s2 = scales(p)
    with np.errstate(all="ignore"):
        look = gp.covered & (gp.z > F(0.0))
        xp, yp, zr, den = project(m, width, rows, gp.z)
        look = look & (den > F(0.0))
        look = look & (xp > F(-1.0)) & (xp < F(width)) & (yp > F(-1.0)) & (yp < F(rows))
        xs, ys = np.where(look, xp, F(0.0)).astype(F), np.where(look, yp, F(0.0)).astype(F)      # (any place where there is none: no tap is taken)
        i0, j0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
        fx, fy = (xs - i0.astype(F)).astype(F), (ys - j0.astype(F)).astype(F)
        bx, by = ((F(1.0) - fx).astype(F), fx), ((F(1.0) - fy).astype(F), fy)
        sumw = np.zeros((rows, width), F)
        acc = np.zeros((rows, width, ch), F)
        nmin = np.full((rows, width), 255, np.int32)
        taps = np.zeros((rows, width), np.int32)
        for ey in (0, 1):
            for ex in (0, 1):
                qx, qy = i0 + ex, j0 + ey
                inside = (qx >= 0) & (qx < width) & (qy >= 0) & (qy < rows)
                cx, cy = np.clip(qx, 0, width - 1), np.clip(qy, 0, rows - 1)
                take = lambda v: v[cy, cx]
                h = (bx[ex] * by[ey]).astype(F)
                lq = take(len_hist).astype(np.int32)
                ok = look & inside & (h != F(0.0)) & (lq != 0) & take(gq.covered)
                wt = h.copy()
                for (vp, vq), sig2 in zip(((gp.N, take(gq.N)), (zr[..., None], take(gq.z)[..., None]), (gp.A, take(gq.A))), s2):
                    u = (F(1.0) - (dr._d2(vp, vq) / sig2).astype(F)).astype(F)
                    ok = ok & (u > F(0.0))
                    wt = (wt * (u * u).astype(F)).astype(F)
                hq = take(Hi)
                sumw = np.where(ok, (sumw + wt).astype(F), sumw)
                acc = np.where(ok[..., None], (acc + (wt[..., None] * hq).astype(F)).astype(F), acc)
                nmin = np.where(ok, np.minimum(nmin, lq), nmin)
                taps += ok
        hit = sumw > F(0.0)
        n = np.minimum(nmin + 1, p.max_history)
        H = (acc / sumw[..., None]).astype(F)
        blend = (H + ((Cu - H).astype(F) / n.astype(F)[..., None]).astype(F)).astype(F)
    out = np.where(hit[..., None], blend, Cu).astype(F)
    len_out = np.where(hit, n, 1).astype(np.uint8)
    out = out[..., 0].copy() if flat else out
    return (out, len_out, taps) if want_taps else (out, len_out)
