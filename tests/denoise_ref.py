"""The edge-avoiding denoiser defined in include/rt_mi355x.h (rt_denoise_device) restated in numpy float32: the guide of a pixel, one a-trous
iteration and the whole filter.  Every operation is one np.float32 array operation, rounded on its own, in the header's order; a tap is
evaluated for the whole image at once (the order of the 25 taps is what the definition fixes, not the order of the pixels).

Test infrastructure only."""
import numpy as np

F = np.float32
H = (F(0.375), F(0.25), F(0.0625))
MAX_ITERATIONS = 8
INF = float("inf")


class Params:
    """rt_denoise_params"""

    def __init__(self, iterations=5, sigma_color=INF, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF):
        self.iterations = int(iterations)
        self.sigma_color, self.sigma_normal, self.sigma_depth, self.sigma_albedo = (F(s) for s in (sigma_color, sigma_normal, sigma_depth, sigma_albedo))

    def sigmas(self):
        return self.sigma_color, self.sigma_normal, self.sigma_depth, self.sigma_albedo

    def valid(self):
        return 1 <= self.iterations <= MAX_ITERATIONS and all(s > 0 for s in self.sigmas())


class Guide:
    """covered [rows, W] bool; z [rows, W], N [rows, W, 3], A [rows, W, 3] float32 (0 where not covered)"""

    def __init__(self, covered, z, N, A):
        self.covered, self.z, self.N, self.A = covered, z, N, A


def guide(g):
    """g [rows, W, 8] -> Guide: a = G[0]; covered exactly when a > 0.0f; z = G[1] / a, N = G[2..4] / a, A = G[5..7] / a"""
    g = np.asarray(g, F)
    assert g.ndim == 3 and g.shape[2] == 8
    a = g[..., 0]
    with np.errstate(all="ignore"):
        covered = a > F(0.0)
        q = (g[..., 1:8] / a[..., None]).astype(F)
    q[~covered] = F(0.0)
    return Guide(covered, q[..., 0].copy(), q[..., 1:4].copy(), q[..., 4:7].copy())


def scales(k, p):
    """(sc2, sn2, sz2, sa2) of iteration k: sc = sigma_color * 2^-k, sn = sigma_normal, sz = sigma_depth * (float)step, sa = sigma_albedo, each squared once"""
    with np.errstate(all="ignore"):
        sc = F(p.sigma_color * F(2.0 ** -k))
        sz = F(p.sigma_depth * F(1 << k))
        return F(sc * sc), F(p.sigma_normal * p.sigma_normal), F(sz * sz), F(p.sigma_albedo * p.sigma_albedo)


def _shift(a, ox, oy):
    """b[y, x] = a[y + oy, x + ox] where that pixel exists (else 0) and the mask of where it does"""
    rows, w = a.shape[:2]
    b = np.zeros_like(a)
    inside = np.zeros((rows, w), bool)
    y0, y1, x0, x1 = max(0, -oy), min(rows, rows - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return b, inside


def _d2(p, q):
    """squared distance of [..., C] values: ((d0*d0) + (d1*d1)) + (d2*d2), or d*d for C == 1; each difference is value(p) - value(q)"""
    d = (p - q).astype(F)
    s = (d[..., 0] * d[..., 0]).astype(F)
    for c in range(1, d.shape[-1]):
        s = (s + (d[..., c] * d[..., c]).astype(F)).astype(F)
    return s


def iteration(img, gd, k, p):
    """I_k [rows, W, C] -> I_{k+1}"""
    img = np.asarray(img, F)
    assert img.ndim == 3 and img.shape[2] in (1, 3) and img.shape[:2] == gd.covered.shape
    step = 1 << k
    s2 = scales(k, p)
    sumw = np.zeros(img.shape[:2], F)
    acc = np.zeros(img.shape, F)
    z1 = gd.z[..., None]
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                iq, inside = _shift(img, step * dx, step * dy)
                cq, _ = _shift(gd.covered, step * dx, step * dy)
                ok = inside & cq & gd.covered
                w = np.full(img.shape[:2], F(H[abs(dx)] * H[abs(dy)]), F)
                if dx or dy:
                    pairs = ((img, iq), (gd.N, _shift(gd.N, step * dx, step * dy)[0]), (z1, _shift(z1, step * dx, step * dy)[0]),
                             (gd.A, _shift(gd.A, step * dx, step * dy)[0]))
                    for (vp, vq), sig2 in zip(pairs, s2):
                        u = (F(1.0) - (_d2(vp, vq) / sig2).astype(F)).astype(F)
                        ok = ok & (u > F(0.0))
                        w = (w * (u * u).astype(F)).astype(F)
                w = np.where(ok, w, F(0.0)).astype(F)
                sumw = np.where(ok, (sumw + w).astype(F), sumw)
                acc = np.where(ok[..., None], (acc + (w[..., None] * iq).astype(F)).astype(F), acc)
        out = (acc / sumw[..., None]).astype(F)
    return np.where(gd.covered[..., None], out, img).astype(F)


def denoise(img, g, p):
    """the filter: img [rows, W, C] (or [rows, W] for one channel), g [rows, W, 8] -> the output in img's shape"""
    assert p.valid()
    a = np.asarray(img, F)
    flat = a.ndim == 2
    cur = a[..., None] if flat else a
    gd = guide(g)
    for k in range(p.iterations):
        cur = iteration(cur, gd, k, p)
    return cur[..., 0].copy() if flat else cur
