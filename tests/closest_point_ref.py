"""The closest-point query of include/rt_mi355x.h ("closest points") restated in numpy float32, operation by operation, and brute force over
the faces that the leaves of a tree reference -- the reference of tests/test_closest_points_api.py and tests/test_gpu_closest_points.py.

numpy rounds every float32 operation on its own and never contracts, so the lines below are the header's lines.  Everything broadcasts:
closest(P[:, None], A[None], B[None], C[None]) is all pairs."""
import numpy as np

F = np.float32
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "face")


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def closest(P, A, B, C):
    """-> (d2, Q, region) of float32 points P against float32 triangles (A, B, C); shapes broadcast, the last axis is xyz"""
    P, A, B, C = (np.asarray(x, F) for x in (P, A, B, C))
    with np.errstate(all="ignore"):
        ab, ac, ap = B - A, C - A, P - A
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = P - B
        d3, d4 = dot(ab, bp), dot(ac, bp)
        cp = P - C
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        d43, d56 = d4 - d3, d5 - d6
        tests = [(d1 <= 0) & (d2 <= 0),
                 (d3 >= 0) & (d4 <= d3),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                 (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & (d43 >= 0) & (d56 >= 0)]
        region = np.select(tests, list(range(6)), 6)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = d43 / (d43 + d56)
        den = F(1) / ((va + vb) + vc)
        v, w = vb * den, vc * den
        shape = np.broadcast(P, A).shape
        full = lambda x: np.broadcast_to(x, shape)                      # noqa: E731 -- a vertex region returns the vertex's own floats
        Q = np.select([(region == k)[..., None] for k in range(6)],
                      [full(A), full(B), A + ab * v_ab[..., None], full(C), A + ac * w_ac[..., None], B + (C - B) * w_bc[..., None]],
                      (A + ab * v[..., None]) + ac * w[..., None])
        e = P - Q
        return dot(e, e).astype(F), Q.astype(F), region


def referenced_faces(nodes, face_refs):
    """the query's scene: the sorted ids of the faces that some leaf references.  nodes: (first, count_flags) per node"""
    keep = []
    for first, cf in nodes:
        if cf & 0x80000000:
            keep.append(face_refs[first:first + (cf & 0x7fffffff)])
    return np.unique(np.concatenate(keep)) if keep else np.empty(0, np.int64)


def brute_force(points, tri_verts, faces, max_dist=np.inf, chunk=1 << 20):
    """-> (face int32, dist2 float32, closest float32 (n, 3)) over the face ids `faces` (ascending) of tri_verts (faces, 9): the candidate
    (d2 <= max_dist * max_dist, never a NaN) with the smallest d2, ties to the lowest id; -1, +inf and the point itself where there is none.
    Chunked, so that the (points x faces) arrays stay small."""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int64)
    T = np.asarray(tri_verts, F).reshape(-1, 3, 3)[faces]
    with np.errstate(all="ignore"):
        r2 = F(max_dist) * F(max_dist)
    n = len(points)
    out_f, out_d, out_q = np.full(n, -1, np.int32), np.full(n, np.inf, F), points.copy()
    if len(faces) == 0:
        return out_f, out_d, out_q
    step = max(1, chunk // max(1, len(faces)))                      # about `chunk` (point, face) pairs at a time
    for at in range(0, n, step):
        P = points[at:at + step]
        d2, Q, _ = closest(P[:, None], T[None, :, 0], T[None, :, 1], T[None, :, 2])
        with np.errstate(invalid="ignore"):
            cand = d2 <= r2
        key = np.where(cand, d2, F(np.inf))
        best = key.min(axis=1)
        first = np.argmax(cand & (key == best[:, None]), axis=1)          # faces ascend: the first minimum is the lowest id
        has = cand.any(axis=1)
        rows = np.arange(len(P))
        out_f[at:at + step] = np.where(has, faces[first], -1)
        out_d[at:at + step] = np.where(has, d2[rows, first], F(np.inf))
        out_q[at:at + step] = np.where(has[:, None], Q[rows, first], P)
    return out_f, out_d, out_q
