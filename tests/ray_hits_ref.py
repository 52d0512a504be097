"""The ordered multi-hit ray query (include/rt_mi355x.h, "ordered ray hits") restated over the CPU checker alone: per ray the root test on
(o, o + d), the checker's BoxTree::intersect (osc.tree_intersect: the distinct faces of the leaves reached), orc_ray_triangle per face,
the filter x != -72, x > 0.00001f, x <= t_max, and the sort by (x, face id).  numpy + ctypes only; slow (a Python loop per ray), so the
tests call it on at most some 1,500 rays per case."""
import ctypes as C

import numpy as np

import query_walk_cases as qc

F = np.float32
MAX_HITS = 8
SUBSET = 1536          # rays per case that the tests hold to this restatement
_FP = C.POINTER(C.c_float)


def _f(a):
    return a.ctypes.data_as(_FP)


def subset(n):
    """-> the indices (into the sorted rays of query_walk_cases) of the first SUBSET rays of the interleaved order: every family in every wave"""
    return qc.interleave(n)[:SUBSET]


def all_hits(osc, o, d, t_max=np.inf):
    """-> per ray the full sorted list [(t float32, face int)] of its distinct hits"""
    o, d = np.ascontiguousarray(o, F).reshape(-1, 3), np.ascontiguousarray(d, F).reshape(-1, 3)
    lib = osc.lib
    box = osc.node(0)["box"].astype(F)
    lo, hi = np.ascontiguousarray(box[:3]), np.ascontiguousarray(box[3:])
    t_max, eps = F(t_max), F(0.00001)
    out = []
    for i in range(len(o)):
        oi, di = np.ascontiguousarray(o[i]), np.ascontiguousarray(d[i])
        with np.errstate(all="ignore"):
            dest = (oi + di).astype(F)
        hits = []
        if lib.orc_box_intersect(_f(lo), _f(hi), _f(oi), _f(dest)):
            for f in osc.tree_intersect(oi, dest).tolist():          # (a std::set: distinct already)
                x = F(lib.orc_ray_triangle(osc.h, _f(oi), _f(di), int(f)))
                if x != F(-72) and x > eps and x <= t_max:             # (NaN fails both comparisons)
                    hits.append((x, int(f)))
        hits.sort()
        out.append(hits)
    return out


def outputs(lists, k):
    """the output rule on full lists -> (face int32 (n, k), t float32 (n, k), count int32 (n,))"""
    n = len(lists)
    face, t, count = np.full((n, k), -1, np.int32), np.full((n, k), -1.0, F), np.empty(n, np.int32)
    for i, h in enumerate(lists):
        count[i] = min(len(h), k + 1)
        for j, (x, f) in enumerate(h[:k]):
            face[i, j], t[i, j] = f, x
    return face, t, count


def ray_hits(osc, o, d, k=MAX_HITS, t_max=np.inf):
    return outputs(all_hits(osc, o, d, t_max), k)


def leaf_references(osc, o, d):
    """-> per ray {face: number of the leaves reached by BoxTree::intersect(o, o + d) that reference it} (no root pre-test, as tree_leaves)"""
    o, d = np.ascontiguousarray(o, F).reshape(-1, 3), np.ascontiguousarray(d, F).reshape(-1, 3)
    faces_of, out = {}, []
    for i in range(len(o)):
        refs = {}
        with np.errstate(all="ignore"):
            dest = (o[i] + d[i]).astype(F)
        for leaf in osc.tree_leaves(o[i], dest).tolist():
            if leaf not in faces_of:
                faces_of[leaf] = osc.node(leaf)["faces"].tolist()
            for f in faces_of[leaf]:
                refs[f] = refs.get(f, 0) + 1
        out.append(refs)
    return out


def has_tie(hits, first=MAX_HITS):
    """two different faces with bit-equal t among the first `first` hits of a sorted list"""
    h = hits[:first]
    return any(h[j][0] == h[j + 1][0] for j in range(len(h) - 1))
