"""Bounced light as include/rt_mi355x.h defines it ("bounced light"), restated in numpy float32 -- test infrastructure only.

The radiance of a hit of tests/indirect_ref.py / tests/probe_ref.py with one more term behind the last light: the source volume looked up at
the hit H with the turned face normal Nf -- probe_ref.lookup (plain) or probe_visible_ref.lookup_visible over one lightStrikes judgement per
read corner (visible) --, clamped at zero, times kd.  Every float32 step is one numpy float32 operation in the order the header writes; the
directions, the tables, the projection, the direct term and the lookups are those modules' own code, imported and not edited.  Closest hits
and visibility come from a `tracer` of indirect_ref (OracleTracer over the CPU checker, LibraryTracer over rt_closest_hits /
rt_light_strikes)."""
import numpy as np

import ao_ref
import indirect_ref as ir
import probe_ref as pr
import probe_visible_ref as pv

F = np.float32


class Hits:
    """what the light loop and the bounce term need of the rays that hit, in raster order of `hit` (bool (n, K))"""

    def __init__(self, n, K, hit, H, Nf, kd, vis, ct):
        self.n, self.K, self.hit, self.H, self.Nf, self.kd, self.vis, self.ct = n, K, hit, H, Nf, kd, vis, ct


def trace_hits(tracer, data, o, d, live, pos):
    """o, d float32 (n, K, 3); live bool (n,): the element forms rays -> Hits (the indirect-diffuse section's hit, H, Nf, kd, vis, ct)"""
    n, K = o.shape[0], o.shape[1]
    pos = np.asarray(pos, F).reshape(-1, 3)
    f = np.full((n, K), -1, np.int32)
    t = np.full((n, K), -1.0, F)
    if live.any():
        f[live], t[live] = (x.reshape(-1, K) for x in tracer.closest(o[live].reshape(-1, 3), d[live].reshape(-1, 3)))
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
    return Hits(n, K, hit, H, Nf, kd, vis, ct)


def source_visibility(tracer, grid, hits):
    """the eight answers per hit of the visible mode (bool (hits, 8)): probe_visible_ref.visibility at (H, Nf)"""
    return pv.visibility(tracer, grid, hits.H, hits.Nf)


def source_lookup(grid, coeff, hits, vis=None):
    """I float32 (hits, 3).  vis None: the plain lookup; else the leak-free lookup given those answers"""
    if vis is None:
        return pr.lookup(grid, coeff, hits.H, hits.Nf)
    return pv.lookup_visible(grid, coeff, hits.H, hits.Nf, vis)[0]


def clamp(I):
    """b = smax(0.0f, I): NaN and -0 give +0"""
    I = np.asarray(I, F)
    with np.errstate(invalid="ignore"):
        return np.where(F(0.0) < I, I, F(0.0)).astype(F)


def radiance(hits, color, I=None, clamped=True):
    """-> R float32 (n, K, 3): the lights in order, then R_c = R_c + kd_c * b_c.  I None: no source (the parents' radiance).  clamped =
    False adds kd * I as it is -- NOT the definition, for the test of the clamp"""
    color = np.asarray(color, F).reshape(3)
    Rh = np.zeros((len(hits.kd), 3), F)
    ck = (color[None, :] * hits.kd).astype(F)
    for l in range(hits.vis.shape[1]):
        v = hits.vis[:, l]
        Rh[v] = Rh[v] + ck[v] * hits.ct[v, l:l + 1]
    if I is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            Rh = (Rh + hits.kd * (clamp(I) if clamped else np.asarray(I, F))).astype(F)
    R = np.zeros((hits.n, hits.K, 3), F)
    R[hits.hit] = Rh
    return R


# ------------------------------------------------------------------------------------------ the probes
class ProbeTrace:
    def __init__(self, P, m, pos, hits, seen):
        self.P, self.m, self.pos, self.hits, self.seen = P, m, pos, hits, seen


def trace_probes(tracer, data, P, m, pos):
    P = np.ascontiguousarray(np.asarray(P, F).reshape(-1, 3))
    pos = np.asarray(pos, F).reshape(-1, 3)
    n, K = len(P), m * m
    D = pr.directions(m)
    o = np.ascontiguousarray(np.broadcast_to(P[:, None, :], (n, K, 3)), F)
    d = np.ascontiguousarray(np.broadcast_to(D[None, :, :], (n, K, 3)), F)
    hits = trace_hits(tracer, data, o, d, np.ones(n, bool), pos)
    return ProbeTrace(P, m, pos, hits, tracer.strikes(P, pos))


def shade_probes(tr, color, direct, I=None, clamped=True):
    """-> float32 (n, 27)"""
    C = pr.project(radiance(tr.hits, color, I, clamped), pr.weights(tr.m))
    if direct:
        pr.add_direct(C, tr.P, tr.pos, color, tr.seen)
    return C.reshape(len(tr.P), pr.COEFFS)


def probes(tracer, data, P, m, pos, color, direct, grid, coeff, visible, tr=None):
    """rt_light_probes_bounce -> float32 (n, 27)"""
    tr = trace_probes(tracer, data, P, m, pos) if tr is None else tr
    vis = source_visibility(tracer, grid, tr.hits) if visible else None
    return shade_probes(tr, color, direct, source_lookup(grid, coeff, tr.hits, vis))


def feedback(tracer, data, grid, m, pos, color, direct, bounces, visible):
    """-> the list of the volumes of passes 0 .. bounces over the probes of `grid` (float32 (cells, 27) each): pass 0 without a source,
    pass b with pass b - 1 as its source, `direct` in the last pass alone -- what Flyscene.light_probes(bounces=) runs"""
    tr = trace_probes(tracer, data, grid.positions(), m, pos)
    vis = source_visibility(tracer, grid, tr.hits) if visible else None
    out = [shade_probes(tr, color, direct and bounces == 0)]
    for b in range(1, bounces + 1):
        out.append(shade_probes(tr, color, direct and b == bounces, source_lookup(grid, out[-1], tr.hits, vis)))
    return out


# ------------------------------------------------------------------------------------------ the gather
def trace_gather(tracer, data, P, N, m, seed, pos, i=None):
    P, N = np.asarray(P, F).reshape(-1, 3), np.asarray(N, F).reshape(-1, 3)
    n, K = len(P), m * m
    i = np.arange(n) if i is None else np.asarray(i)
    d = ir.directions(N, i, seed, m)
    live = ao_ref.is_point(N)
    o = np.ascontiguousarray(np.broadcast_to(P[:, None, :], (n, K, 3)), F)
    return trace_hits(tracer, data, o, d, live, pos), live


def shade_gather(hits, live, color, I=None, clamped=True):
    R = radiance(hits, color, I, clamped)
    E = np.zeros((hits.n, 3), F)
    for k in range(hits.K):
        E = E + R[:, k]
    out = (E / F(hits.K)).astype(F)
    out[~live] = F(0.0)
    return out


def gather(tracer, data, P, N, m, seed, pos, color, grid, coeff, visible, i=None):
    """rt_indirect_diffuse_bounce -> float32 (n, 3)"""
    hits, live = trace_gather(tracer, data, P, N, m, seed, pos, i)
    vis = source_visibility(tracer, grid, hits) if visible else None
    return shade_gather(hits, live, color, source_lookup(grid, coeff, hits, vis))
