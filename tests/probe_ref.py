"""The light probes as include/rt_mi355x.h defines them ("light probes"), restated in numpy -- test infrastructure only.

The tables are computed in Python floats (IEEE double, the C library's sqrt / cos / sin, one operation at a time in the order of
rt_capi.cpp) and stored as float32.  Every float32 step of the device half is one numpy float32 operation, in the order the header writes.
The closest hit of a probe ray and the visibility of a light come from a `tracer` of tests/indirect_ref.py (OracleTracer over the CPU
checker, LibraryTracer over rt_closest_hits / rt_light_strikes); the radiance of a hit is that module's, word for word."""
import math

import numpy as np

import indirect_ref as ir

F = np.float32
COEFFS = 27
A_BAND = (1.0, 2.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0, 0.25, 0.25, 0.25, 0.25, 0.25)
B_BAND = np.array([3.14159274] + [2.09439510] * 3 + [0.785398163] * 5, F)
C0, C1, C2, C3, C4 = F(0.282094792), F(0.488602512), F(1.092548431), F(0.315391565), F(0.546274215)


# ------------------------------------------------------------------------------------------ the tables
def directions(m):
    """rt_probe_directions -> float32 (K, 3)"""
    out = np.empty((m * m, 3), F)
    for k in range(m * m):
        x, y = (k % m + 0.5) / m, (k // m + 0.5) / m
        z = 1.0 - 2.0 * y
        rr = 1.0 - z * z
        r = math.sqrt(rr if rr > 0.0 else 0.0)
        phi = 2.0 * math.pi * x
        out[k] = (r * math.cos(phi), r * math.sin(phi), z)
    return out


def weights(m):
    """rt_probe_weights -> float32 (K, 9)"""
    K = m * m
    D = directions(m).astype(np.float64)
    s1, s2 = math.sqrt(3.0 / (4.0 * math.pi)), 0.5 * math.sqrt(15.0 / math.pi)
    s6, s8 = 0.25 * math.sqrt(5.0 / math.pi), 0.25 * math.sqrt(15.0 / math.pi)
    solid = 4.0 * math.pi / K
    out = np.empty((K, 9), F)
    for k in range(K):
        x, y, z = (float(v) for v in D[k])
        Y = (0.5 * math.sqrt(1.0 / math.pi), s1 * y, s1 * z, s1 * x, s2 * x * y, s2 * y * z, s6 * (3.0 * z * z - 1.0), s2 * x * z, s8 * (x * x - y * y))
        out[k] = [solid * A_BAND[j] * Y[j] for j in range(9)]
    return out


def sh9(n):
    """rt_sh9 on float32 (.., 3) -> float32 (.., 9)"""
    n = np.asarray(n, F)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        out = [np.broadcast_to(C0, x.shape), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), C3 * ((F(3.0) * (z * z)) - F(1.0)), C2 * (x * z), C4 * ((x * x) - (y * y))]
    return np.stack(out, axis=-1).astype(F)


# ------------------------------------------------------------------------------------------ the probes
class Traced:
    """the part of the definition that depends neither on the light colour nor on `direct`: per probe ray whether it hit, and per hit and
    light whether the light is visible and the clamped cosine ct; per probe and light whether the probe sees the light"""

    def __init__(self, P, m, pos, hit, kd, vis, ct, seen):
        self.P, self.m, self.pos, self.n, self.K = P, m, pos, len(P), m * m
        self.hit, self.kd, self.vis, self.ct, self.seen = hit, kd, vis, ct, seen


def trace(tracer, data, P, m, pos):
    P = np.asarray(P, F).reshape(-1, 3)
    pos = np.asarray(pos, F).reshape(-1, 3)
    n, K = len(P), m * m
    D = directions(m)
    o = np.ascontiguousarray(np.broadcast_to(P[:, None, :], (n, K, 3)), F)
    d = np.ascontiguousarray(np.broadcast_to(D[None, :, :], (n, K, 3)), F)
    f, t = (x.reshape(n, K) for x in tracer.closest(o.reshape(-1, 3), d.reshape(-1, 3)))
    hit = (f >= 0) & (f < data.face_normal.shape[0])
    fh, th, dh, oh = f[hit], t[hit], d[hit], o[hit]
    H = (oh + th[:, None] * dh).astype(F)                 # multiply, then add
    Nf = data.face_normal[fh].copy()
    flip = (Nf[:, 0] * dh[:, 0] + Nf[:, 1] * dh[:, 1]) + Nf[:, 2] * dh[:, 2] > 0
    Nf[flip] = -Nf[flip]
    kd = data.kd[data.face_mat[fh]]
    vis = tracer.strikes(H, pos)
    ct = np.zeros((len(H), len(pos)), F)
    for l in range(len(pos)):
        ld = ir.normalized(pos[l][None, :] - H)
        with np.errstate(invalid="ignore"):
            ldn = ir.dot3(ld, Nf)
            ct[:, l] = np.where(F(0.0) < ldn, ldn, F(0.0))
    seen = tracer.strikes(P, pos)                         # light = pos[l], hit = P
    return Traced(P, m, pos, hit, kd, vis, ct, seen)


def radiance(tr, color):
    """-> R float32 (n, K, 3), the radiance of every probe ray (misses +0)"""
    color = np.asarray(color, F).reshape(3)
    Rh = np.zeros((len(tr.kd), 3), F)
    ck = (color[None, :] * tr.kd).astype(F)
    for l in range(tr.vis.shape[1]):
        v = tr.vis[:, l]
        Rh[v] = Rh[v] + ck[v] * tr.ct[v, l:l + 1]
    R = np.zeros((tr.n, tr.K, 3), F)
    R[tr.hit] = Rh
    return R


def project(R, W, reverse=False):
    """step 4: C[j][c] = C[j][c] + R_c(k) * W[k][j] for k in order -> float32 (n, 9, 3).  reverse: k from K - 1 down to 0 -- NOT the
    definition, for the test of the order"""
    R, W = np.asarray(R, F), np.asarray(W, F)
    n, K = R.shape[0], R.shape[1]
    C = np.zeros((n, 9, 3), F)
    for k in (range(K - 1, -1, -1) if reverse else range(K)):
        C = C + R[:, k, None, :] * W[k][None, :, None]
    return C


def add_direct(C, P, pos, color, seen):
    """step 5, in place: for every light in order, where the probe sees it, C[j][c] = C[j][c] + color_c * (b_j * Yw_j)"""
    color = np.asarray(color, F).reshape(3)
    pos = np.asarray(pos, F).reshape(-1, 3)
    for l in range(len(pos)):
        Yw = sh9(ir.normalized(pos[l][None, :] - np.asarray(P, F)))
        term = (color[None, None, :] * (B_BAND[None, :] * Yw)[:, :, None]).astype(F)
        v = np.asarray(seen)[:, l]
        C[v] = C[v] + term[v]
    return C


def shade(tr, color, direct=False, reverse=False):
    """-> float32 (n, 27), coefficient j of channel c at j * 3 + c"""
    C = project(radiance(tr, color), weights(tr.m), reverse)
    if direct:
        add_direct(C, tr.P, tr.pos, color, tr.seen)
    return C.reshape(tr.n, COEFFS)


def probes(tracer, data, P, m, pos, color, direct=False, reverse=False):
    return shade(trace(tracer, data, P, m, pos), color, direct, reverse)


# ------------------------------------------------------------------------------------------ the grid and the lookup
class Grid:
    def __init__(self, origin, step, dims):
        self.origin, self.step = np.asarray(origin, F).reshape(3), np.asarray(step, F).reshape(3)
        self.dims = tuple(int(x) for x in dims)
        self.cells = self.dims[0] * self.dims[1] * self.dims[2]

    @classmethod
    def of(cls, g):
        """from an rt_probe_grid"""
        return cls(list(g.origin), list(g.step), list(g.dims))

    @classmethod
    def over(cls, box, dims, margin=0.0):
        """flyscene.probe_grid_over, restated"""
        b, mg = np.asarray(box, F).reshape(6), F(margin)
        origin, step = [], []
        for q in range(3):
            lo, hi = b[q] - mg, b[3 + q] + mg
            one = int(dims[q]) <= 1
            origin.append((lo + hi) * F(0.5) if one else lo)
            step.append(F(1.0) if one else (hi - lo) / F(int(dims[q]) - 1))
        return cls(origin, step, dims)

    def positions(self):
        """rt_probe_grid_positions -> float32 (cells, 3), probe (ix, iy, iz) at index (iz * dims[1] + iy) * dims[0] + ix"""
        dx, dy, dz = self.dims
        iz, iy, ix = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
        out = np.empty((self.cells, 3), F)
        for q, i in enumerate((ix, iy, iz)):
            out[:, q] = self.origin[q] + i.reshape(-1).astype(F) * self.step[q]
        return out


def axis(p, origin, step, dim):
    """step 2 of the lookup -> (i0 int64, w0, w1 float32)"""
    p = np.asarray(p, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = ((p - F(origin)) / F(step)).astype(F)
        g = np.where(F(0.0) < g, g, F(0.0)).astype(F)
        top = F(dim - 1)
        g = np.where(g > top, top, g).astype(F)
    i0 = np.minimum(g.astype(np.int64), max(dim - 2, 0))
    f = (g - i0.astype(F)).astype(F)
    return i0, (F(1.0) - f).astype(F), f


def lookup(grid, coeff, P, N):
    """rt_probe_irradiance -> float32 (n, 3)"""
    P, N = np.asarray(P, F).reshape(-1, 3), np.asarray(N, F).reshape(-1, 3)
    Cf = np.asarray(coeff, F).reshape(grid.cells, 9, 3)
    n = len(P)
    ax = [axis(P[:, q], grid.origin[q], grid.step[q], grid.dims[q]) for q in range(3)]
    B = np.zeros((n, 9, 3), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for dz in range(1 if grid.dims[2] == 1 else 2):
            for dy in range(1 if grid.dims[1] == 1 else 2):
                for dx in range(1 if grid.dims[0] == 1 else 2):
                    w = (ax[2][1 + dz] * ax[1][1 + dy]) * ax[0][1 + dx]
                    idx = ((ax[2][0] + dz) * grid.dims[1] + (ax[1][0] + dy)) * grid.dims[0] + (ax[0][0] + dx)
                    B = B + w[:, None, None] * Cf[idx]
        Y = sh9(N)
        out = np.zeros((n, 3), F)
        for j in range(9):
            out = out + B[:, j, :] * Y[:, j:j + 1]
    out[~(N != 0).any(axis=1)] = F(0.0)
    return out


def evaluate(C, n):
    """step 5 alone on coefficients (.., 27) at one direction n -> float32 (.., 3)"""
    C = np.asarray(C, F).reshape(-1, 9, 3)
    Y = sh9(np.asarray(n, F).reshape(3))
    out = np.zeros((len(C), 3), F)
    for j in range(9):
        out = out + C[:, j, :] * Y[j]
    return out


# ------------------------------------------------------------------------------------------ the measurement of DESIGN.md 6
def quality(orc, osc, width, height, yaw, pos, color, dims, m, truth_grid, margin=0.0, seed=0):
    """What a Lambert surface sends back, kd(P) * out, over the hit points of the width x height camera at `yaw`: the lookup of a dims volume
    of m x m probes over the scene's root box against rt_indirect_diffuse's definition with truth_grid x truth_grid rays, as an RMS distance
    over the pixels where the truth is not zero -> dict"""
    import ao_ref
    (o, d, f, t), _ = ao_ref.camera_points(orc, osc, width, height, yaw)
    P, N = ao_ref.hit_points(o, d, f, t, osc.arrays()["face_normal"])
    data, tracer = ir.SceneData(osc), ir.OracleTracer(osc)
    albedo = np.zeros((len(f), 3), F)
    albedo[f >= 0] = data.kd[data.face_mat[f[f >= 0]]]
    w = np.asarray(osc.arrays()["wverts"], F)
    grid = Grid.over(np.concatenate([w.min(axis=0), w.max(axis=0)]), dims, margin)
    coeff = probes(tracer, data, grid.positions(), m, pos, color)
    got = albedo * lookup(grid, coeff, P, N)
    truth = albedo * ir.gather(tracer, data, P, N, truth_grid, seed, pos, color)
    mask = (truth != 0).any(axis=-1)
    e = (np.asarray(got, np.float64) - np.asarray(truth, np.float64))[mask]
    return {"pixels": int(mask.sum()), "covered": int((f >= 0).sum()), "probes": grid.cells, "rms": float(np.sqrt((e * e).mean())),
            "truth_rms": float(np.sqrt((np.asarray(truth, np.float64)[mask] ** 2).mean()))}
