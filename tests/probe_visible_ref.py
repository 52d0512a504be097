"""The leak-free probe lookup as include/rt_mi355x.h defines it ("leak-free probe lookup"), restated in numpy float32 -- test infrastructure
only.

Every float32 step is one numpy float32 operation in the order the header writes; the cell, the weights and the basis are those of
tests/probe_ref.py.  Whether a point sees a probe comes from a `tracer` of tests/indirect_ref.py: OracleTracer asks the CPU checker's
lightStrikes, LibraryTracer the host-pointer call rt_light_strikes, one batch for all segments.  The arithmetic around them is the same
code.  The module also generates the two-room scene on which the leak of the plain lookup, and its removal, show."""
import ctypes as C

import numpy as np

import indirect_ref as ir
import probe_ref as pr

F = np.float32


# ------------------------------------------------------------------------------------------ the definition
def is_point(N):
    return (np.asarray(N, F).reshape(-1, 3) != 0).any(axis=1)


def corners(grid, P):
    """steps 2 and 3 -> read bool (8,), weight float32 (n, 8), probe index int64 (n, 8; 0 where the corner is not read), probe position
    float32 (n, 8, 3); corner b = 4 dz + 2 dy + dx"""
    P = np.asarray(P, F).reshape(-1, 3)
    n = len(P)
    ax = [pr.axis(P[:, q], grid.origin[q], grid.step[q], grid.dims[q]) for q in range(3)]
    read = np.zeros(8, bool)
    w, idx, Pc = np.zeros((n, 8), F), np.zeros((n, 8), np.int64), np.zeros((n, 8, 3), F)
    for b in range(8):
        d = (b & 1, (b >> 1) & 1, b >> 2)
        read[b] = not any(d[q] and grid.dims[q] == 1 for q in range(3))
        w[:, b] = (ax[2][1 + d[2]] * ax[1][1 + d[1]]) * ax[0][1 + d[0]]
        i = [ax[q][0] + d[q] for q in range(3)]
        if read[b]:
            idx[:, b] = (i[2] * grid.dims[1] + i[1]) * grid.dims[0] + i[0]
        for q in range(3):
            Pc[:, b, q] = grid.origin[q] + i[q].astype(F) * grid.step[q]
    return read, w, idx, Pc


def pair_strikes(tracer, P, L):
    """-> bool (n, k): the segment light = L[i, j], hit = P[i] is visible, as lightStrikes judges it"""
    P, L = np.asarray(P, F).reshape(-1, 3), np.asarray(L, F)
    n, k = L.shape[0], L.shape[1]
    if n == 0:
        return np.zeros((0, k), bool)
    if isinstance(tracer, ir.LibraryTracer):
        hit = np.ascontiguousarray(np.broadcast_to(P[:, None, :], (n, k, 3)), F)
        light = np.ascontiguousarray(L, F)
        vis = np.full(n * k, 7, np.uint8)
        fp = lambda a: a.ctypes.data_as(C.c_void_p)
        tracer.rt.capi.check(tracer.lib, tracer.ctx.handle, tracer.lib.rt_light_strikes(tracer.ctx.handle, n * k, fp(hit), fp(light), fp(vis)), "rt_light_strikes")
        assert ((vis == 0) | (vis == 1)).all()
        return vis.reshape(n, k).astype(bool)
    out = np.empty((n, k), bool)
    for i in range(n):
        out[i] = tracer.strikes(P[i:i + 1], L[i])[0]
    return out


def visibility(tracer, grid, P, N):
    """step 4 -> bool (n, 8): corner b is read and the point sees its probe; no segment is formed for a point that is no point or for a
    corner that is not read"""
    P = np.asarray(P, F).reshape(-1, 3)
    read, _, _, Pc = corners(grid, P)
    live = is_point(N)
    vis = np.zeros((len(P), 8), bool)
    cols = np.flatnonzero(read)
    if live.any() and len(cols):
        vis[np.ix_(live, cols)] = pair_strikes(tracer, P[live], Pc[live][:, cols])
    return vis


def classes(grid, P, N, vis):
    """-> int (n,): 0 no point, 1 every read corner visible, 3 no corner USED, 2 some blocked and at least one USED"""
    read, w, _, _ = corners(grid, P)
    vis = np.asarray(vis, bool) & read[None, :]
    used = vis & (w > 0)
    out = np.full(len(vis), 2)
    out[~used.any(axis=1)] = 3
    out[(vis == read[None, :]).all(axis=1)] = 1
    out[~is_point(N)] = 0
    return out


def lookup_visible(grid, coeff, P, N, vis):
    """steps 1 to 6 given the visibility bits `vis` (bool (n, 8); bits of corners that are not read are ignored) -> (rgb float32 (n, 3),
    mask uint8 (n,))"""
    P, N = np.asarray(P, F).reshape(-1, 3), np.asarray(N, F).reshape(-1, 3)
    Cf = np.asarray(coeff, F).reshape(grid.cells, 9, 3)
    n = len(P)
    read, w, idx, _ = corners(grid, P)
    live = is_point(N)
    vis = np.asarray(vis, bool).reshape(n, 8) & read[None, :] & live[:, None]
    used = vis & (w > F(0.0))
    case_a = (vis == read[None, :]).all(axis=1) | ~used.any(axis=1)
    take = np.where(case_a[:, None], np.broadcast_to(read[None, :], (n, 8)), used)
    B, W = np.zeros((n, 9, 3), F), np.zeros(n, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for b in range(8):
            t = take[:, b] & live
            W[t] = W[t] + w[t, b]
            B[t] = B[t] + w[t, b][:, None, None] * Cf[idx[t, b]]
        Y = pr.sh9(N)
        out = np.zeros((n, 3), F)
        for j in range(9):
            out = out + B[:, j, :] * Y[:, j:j + 1]
        div = ~case_a & live
        out[div] = out[div] / W[div][:, None]
    out[~live] = F(0.0)
    mask = (vis.astype(np.uint8) << np.arange(8, dtype=np.uint8)[None, :]).sum(axis=1).astype(np.uint8)
    return out.astype(F), mask


def lookup(tracer, grid, coeff, P, N):
    """rt_probe_irradiance_visible -> (rgb, mask)"""
    return lookup_visible(grid, coeff, P, N, visibility(tracer, grid, P, N))


# ------------------------------------------------------------------------------------------ the two-room scene
# File coordinates (indirect_ref.to_world takes them to the tracer's): a closed box x in [-2, 2], y in [0, 1.5], z in [-1, 1], cut at x = 0 by
# a partition of thickness ROOM_W whose two faces span the whole cross-section.  Room A is x < 0 and holds the light; room B is x > 0.
ROOM_W = 0.2
ROOM_LIGHT = (-1.0, 0.75, 0.0)
ROOM_BOX = ((-2.0, 0.0, -1.0), (2.0, 1.5, 1.0))


def _room_mesh():
    verts, faces = [], []

    def quad(mat, p0, p1, p2, p3):
        base = len(verts)
        verts.extend([p0, p1, p2, p3])
        faces.extend([(mat, (base + 1, base + 2, base + 3)), (mat, (base + 1, base + 3, base + 4))])

    (x0, y0, z0), (x1, y1, z1) = ROOM_BOX
    h = ROOM_W / 2
    quad("floor", (x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1))
    quad("ceiling", (x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1))
    quad("wall", (x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0))
    quad("wall", (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1))
    quad("wall", (x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0))
    quad("wall", (x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0))
    quad("partition", (-h, y0, z0), (-h, y0, z1), (-h, y1, z1), (-h, y1, z0))
    quad("partition", (h, y0, z0), (h, y0, z1), (h, y1, z1), (h, y1, z0))
    return verts, faces


ROOM_VERTS = _room_mesh()[0]


def two_rooms(dirpath, name="rooms"):
    """-> path of the .obj: every material plain diffuse"""
    mtl = "".join(f"newmtl {m}\nNs 10.0\nKd {kd}\nKs 0.0 0.0 0.0\nillum 2\n"
                  for m, kd in (("floor", "0.6 0.6 0.6"), ("ceiling", "0.8 0.8 0.8"), ("wall", "0.7 0.5 0.3"), ("partition", "0.5 0.6 0.7")))
    verts, faces = _room_mesh()
    return ir._write(dirpath, name, mtl, verts, faces)


def room_grid(W):
    """-> probe_ref.Grid in world coordinates, W = to_world of the scene: 4 x 2 x 2 probes at file x = -1.5, -0.5, 0.5, 1.5, y = 0.4, 1.1,
    z = -0.5, 0.5 -- two layers in each room, step 1 (five partitions thick) across it"""
    lo, hi = W([-1.5, 0.4, -0.5]).astype(np.float64), W([1.5, 1.1, 0.5]).astype(np.float64)
    dims = (4, 2, 2)
    return pr.Grid(lo, [(hi[q] - lo[q]) / (dims[q] - 1) for q in range(3)], dims)


def room_b_points(W):
    """-> (P, N) in world coordinates: 72 points on room B's floor, ceiling and side walls, 0.05 to 0.35 file units (within half a grid
    step) behind the partition, normals into the room"""
    xs = [ROOM_W / 2 + d for d in (0.05, 0.15, 0.25, 0.35)]
    P, N = [], []
    for x in xs:
        for z in (-0.9, -0.5, -0.1, 0.3, 0.6, 0.9):
            P += [(x, 0.0, z), (x, 1.5, z)]
            N += [(0, 1, 0), (0, -1, 0)]
        for y in (0.2, 0.7, 1.3):
            P += [(x, y, -1.0), (x, y, 1.0)]
            N += [(0, 0, 1), (0, 0, -1)]
    return W(P), np.asarray(N, F)
