"""The guided upsample defined in include/rt_mi355x.h (rt_upsample_device) restated in numpy float32: the low size, the low camera, the four
taps of a high pixel and the whole operator.  Every operation is one np.float32 array operation, rounded on its own, in the header's order;
a tap is evaluated for the whole image at once (the order of the four taps and of the three guides is what the definition fixes, not the
order of the pixels).  The guide of a pixel and the squared distances are the denoiser's (tests/denoise_ref.py).

Test infrastructure only."""
import numpy as np

import denoise_ref as dr

F = np.float32
MAX_FACTOR = 8
INF = float("inf")


class Params:
    """rt_upsample_params"""

    def __init__(self, factor=2, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF):
        self.factor = int(factor)
        self.sigma_normal, self.sigma_depth, self.sigma_albedo = (F(s) for s in (sigma_normal, sigma_depth, sigma_albedo))

    def sigmas(self):
        return self.sigma_normal, self.sigma_depth, self.sigma_albedo

    def valid(self):
        return 2 <= self.factor <= MAX_FACTOR and all(s > 0 for s in self.sigmas())


def low_size(width, rows, s):
    """(w, r) = (ceil(width / s), ceil(rows / s))"""
    return (width + s - 1) // s, (rows + s - 1) // s


def scales(p):
    """(sn2, sz2, sa2): sn = sigma_normal, sz = sigma_depth * (float)s, sa = sigma_albedo, each squared once"""
    with np.errstate(all="ignore"):
        sz = F(p.sigma_depth * F(p.factor))
        return F(p.sigma_normal * p.sigma_normal), F(sz * sz), F(p.sigma_albedo * p.sigma_albedo)


def low_viewport(viewport, s):
    """the viewport of the low camera: the high camera's with [2] and [3] each divided by (float)s, one float division each"""
    v = np.array(viewport, F)
    v[2] = F(v[2] / F(s))
    v[3] = F(v[3] / F(s))
    return v


def nearest(v, s, extent):
    """min((2v + s) / (2s), extent - 1) for an integer array v"""
    return np.minimum((2 * v.astype(np.int64) + s) // (2 * s), extent - 1)


def upsample(low, g_low, g_high, p, want_miss=False):
    """the operator: low [r, w, C] (or [r, w] for one channel), g_low [r, w, 8], g_high [rows, width, 8] -> out [rows, width, C] (or
    [rows, width]); want_miss: -> (out, miss uint8 [rows, width])"""
    assert p.valid()
    a = np.asarray(low, F)
    flat = a.ndim == 2
    L = a[..., None] if flat else a
    g_low, g_high = np.asarray(g_low, F), np.asarray(g_high, F)
    rows, width = g_high.shape[:2]
    s = p.factor
    w, r = low_size(width, rows, s)
    assert L.shape[:2] == (r, w) and L.shape[2] in (1, 3) and g_low.shape == (r, w, 8) and g_high.shape == (rows, width, 8)
    ch = L.shape[2]
    if rows == 0:
        out = np.zeros((0, width, ch), F)
        out = out[..., 0] if flat else out
        return (out, np.zeros((0, width), np.uint8)) if want_miss else out
    gp, gq = dr.guide(g_high), dr.guide(g_low)
    s2 = scales(p)
    x, y = np.arange(width), np.arange(rows)
    i0, j0 = x // s, y // s
    fx, fy = x - i0 * s, y - j0 * s
    with np.errstate(all="ignore"):
        bx = ((s - fx).astype(F) / F(s)).astype(F), (fx.astype(F) / F(s)).astype(F)
        by = ((s - fy).astype(F) / F(s)).astype(F), (fy.astype(F) / F(s)).astype(F)
        sumw = np.zeros((rows, width), F)
        acc = np.zeros((rows, width, ch), F)
        pz = gp.z[..., None]
        for ey in (0, 1):
            for ex in (0, 1):
                qx, qy = i0 + ex, j0 + ey
                inside = (qy < r)[:, None] & (qx < w)[None, :]
                cx, cy = np.minimum(qx, w - 1), np.minimum(qy, r - 1)          # (any pixel where the tap is outside: it is skipped)
                take = lambda v: v[cy[:, None], cx[None, :]]
                h = (by[ey][:, None] * bx[ex][None, :]).astype(F)               # (a product of two floats commutes)
                ok = inside & (h != F(0.0)) & (take(gq.covered) == gp.covered)
                wt = h.copy()
                live = ok & gp.covered                                          # the guides are evaluated for covered pixels only
                for (vp, vq), sig2 in zip(((gp.N, take(gq.N)), (pz, take(gq.z[..., None])), (gp.A, take(gq.A))), s2):
                    u = (F(1.0) - (dr._d2(vp, vq) / sig2).astype(F)).astype(F)
                    ok = ok & (~gp.covered | (u > F(0.0)))
                    wt = np.where(live, (wt * (u * u).astype(F)).astype(F), wt)
                lq = take(L)
                sumw = np.where(ok, (sumw + wt).astype(F), sumw)
                acc = np.where(ok[..., None], (acc + (wt[..., None] * lq).astype(F)).astype(F), acc)
        hit = sumw > F(0.0)
        out = (acc / sumw[..., None]).astype(F)
    near = L[nearest(y, s, r)[:, None], nearest(x, s, w)[None, :]]
    out = np.where(hit[..., None], out, near).astype(F)
    out = out[..., 0].copy() if flat else out
    return (out, (~hit).astype(np.uint8)) if want_miss else out


def bilinear(low, width, rows, s):
    """plain float bilinear with the operator's weights and tap order, written on its own: what every +inf sigma gives on an all-covered image"""
    a = np.asarray(low, F)
    flat = a.ndim == 2
    L = a[..., None] if flat else a
    r, w = L.shape[:2]
    out = np.zeros((rows, width, L.shape[2]), F)
    for yy in range(rows):
        j0 = yy // s
        fy = yy - j0 * s
        by = (F(s - fy) / F(s), F(fy) / F(s))
        for xx in range(width):
            i0 = xx // s
            fx = xx - i0 * s
            bx = (F(s - fx) / F(s), F(fx) / F(s))
            sw, sc = F(0.0), np.zeros(L.shape[2], F)
            for ey in (0, 1):
                for ex in (0, 1):
                    if i0 + ex >= w or j0 + ey >= r:
                        continue
                    h = F(bx[ex] * by[ey])
                    if h == 0:
                        continue
                    sw = F(sw + h)
                    sc = (sc + (h * L[j0 + ey, i0 + ex]).astype(F)).astype(F)
            out[yy, xx] = (sc / sw).astype(F)
    return out[..., 0].copy() if flat else out
