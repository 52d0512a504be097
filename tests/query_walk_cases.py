"""Scenes, rays and segments that hold the query kernels' tree walk (packet_walk / leaf_visit of rt_kernels.hip, as k_closest, k_segments
and the compound queries instantiate it) to the CPU checker -- plain data and seeded generators, numpy only.

Shared by tests/test_query_walk_cases.py (the conditions, on the checker alone) and tests/test_gpu_query_walk.py (the kernels).

SCENES are seeded soups (scenes_gen.random_soup) at a (capacity, max_depth): single-leaf scenes of 12, 64 and 65 faces, trees whose
leaves hold several 64-triangle chunks, and depth-capped trees with thousands of over-full leaves and lost nodes (build_cases.py), plus
soup 8 under uniform scales.  These soups do NOT grow deep trees: a scene-sized triangle lands in every octant, so the deepest leaf of
any case here is at level 6 (the table below), whatever max_depth says.  Nothing here covers a walk fifteen levels deep.

Rays are generated from the checker's own arrays (world vertices, face_vid, face_normal), float32, from one seed per case; see rays().
"""
import collections

import numpy as np

import build_cases
import scenes_gen

F = np.float32
Case = collections.namedtuple("Case", "seed n cap depth scale_exp")

#                    seed     n   cap  depth  scale 2^e
CASES = {"flat12": Case(13,   12, 1000, 15, None),
         "flat64": Case(14,   64, 1000, 15, None),
         "flat65": Case(15,   65, 1000, 15, None),
         "soup8":  Case(8,   800,  250, 15, None),
         "soup10": Case(10, 1500,  250, 15, None),
         "soup9":  Case(9,  6000, 1000, 15, None),
         "cap38":  Case(38, 1000,    1,  3, None),
         "cap31":  Case(31, 2000,   64,  4, None),
         "cap34":  Case(34,  300,   16,  5, None),
         "soup8_2^-20": Case(8, 800, 250, 15, -20),
         "soup8_2^-10": Case(8, 800, 250, 15, -10),
         "soup8_2^10":  Case(8, 800, 250, 15, 10),
         "soup8_2^20":  Case(8, 800, 250, 15, 20)}
UNSCALED = [k for k, c in CASES.items() if c.scale_exp is None]
SCALED = [k for k, c in CASES.items() if c.scale_exp is not None]
NONFINITE_CASES = ("soup8", "flat12")
COMPOUND_CASES = ("soup8", "cap38")

# The CPU checker's trees, recorded once: non-empty leaves, level of the deepest one, leaves of <= 16 / 17 .. 64 / >= 65 faces, the
# largest leaf, lost nodes (a child with exactly `cap` faces: neither leaf nor split)
#                    leaves deepest  (<=16, 17..64, >=65) largest lost
TREES = {"flat12": (1,      0,       (1, 0, 0),            12,    0),
         "flat64": (1,      0,       (0, 1, 0),            64,    0),
         "flat65": (1,      0,       (0, 0, 1),            65,    0),
         "soup8":  (22,     2,       (0, 7, 15),           224,   0),
         "soup10": (112,    4,       (0, 21, 91),          249,   1),
         "soup9":  (106,    4,       (0, 0, 106),          950,   0),
         "cap38":  (4096,   4,       (697, 2759, 640),     174,   0),
         "cap31":  (18362,  5,       (0, 1498, 16864),     348,   42),
         "cap34":  (82958,  6,       (2099, 80859, 0),     63,    511)}
OVER_FULL = {"cap31": 16864, "cap34": 80859}          # leaves holding more than `cap` faces (build_cases.DEPTH_LIMITED)

FAMILY = 1024
FAMILIES = ("centroid", "vertex", "edge", "random", "axis", "long", "short", "onface")     # 1,024 rays each
AIMED = ("centroid", "vertex", "edge", "axis", "long", "short")
FAR, BUNDLES = 256, 16
ORDER = FAMILIES + ("far", "bundle", "ties")           # `ties` last: its length varies, everything before it is wave-aligned
STRIDE = 8191                                          # interleaved[i] = sorted[(i * 8191) % n]
S_EDGE = (0.97, 0.979, 0.9801, 0.99)
SEGMENT_FAMILIES = ("pairs", "onface", "mirrored", "edge")
SAME_POINT = 16
GRAZE, S_GRAZE, OUTSIDE = 1536, 0.9798, 4096
# Random pairs are drawn in the cube of side 1.25 ext: at 1.5 ext the twelve- and 65-face scenes block 17 to 19 % of them, short of the
# 20 % that tests/test_query_walk_cases.py asks of every case; at 1.25 ext every case has 23 % or more blocked and 28 % or more visible.
PAIR_SIDE = 1.25
EDGE_SIDE = 0.1
# Tie rays start at centroid + s * ext * unit normal: both sides at 0.02, and once more at 0.04 (the 64-face scene has one duplicated
# face; two rays per face would leave it short of the four tie rays that every case with duplicates must show)
TIE_OFFSETS = (0.02, -0.02, 0.04, -0.04)

# the leaf-mode rule of leaf_visit (rt_kernels.hip), restated; tests/test_query_walk_cases.py pins it to the source text
COST_RAY_MODE, COST_TRI_MODE, COST_CHUNK_TEST, SCALAR_LEAF_MAX, STAGE_TRIS = 45, 58, 30, 16, 64


def tri_mode(cnt, live):
    """lanes = triangles for a leaf of cnt faces that `live` rays of the wave need (kernels with the staging buffer)"""
    nchunk = (cnt + 63) // 64
    return nchunk * COST_CHUNK_TEST + live * ((nchunk + 2) // 3) * COST_TRI_MODE < cnt * COST_RAY_MODE


def leaf_class(cnt):
    """0: the scalar-load walk (lanes = rays), 1: one staged chunk at the most, 2: several chunks"""
    return 0 if cnt <= SCALAR_LEAF_MAX else (1 if cnt <= STAGE_TRIS else 2)


# ------------------------------------------------------------------------------------------ scenes
def scene_path(dirpath, name):
    c = CASES[name]
    return scenes_gen.random_soup(str(dirpath), c.seed, c.n)


def oracle_scene(oracle, dirpath, name):
    c = CASES[name]
    osc = oracle.load_scene(scene_path(dirpath, name), capacity=c.cap, maxdepth=c.depth)
    if c.scale_exp is not None:
        osc.set_model(build_cases.scale_model(c.scale_exp))
        osc.rebuild(c.cap, c.depth)
    return osc


def host_scene(rt, dirpath, name):
    c = CASES[name]
    hs = rt.HostScene(scene_path(dirpath, name), c.cap, c.depth)
    if c.scale_exp is not None:
        hs.set_model(build_cases.scale_model(c.scale_exp), True)
    return hs


def tree(osc):
    """-> (leaf node ids, their face counts, their levels, lost nodes) of an OracleScene, leaves holding at least one face"""
    ids, cnt, lvl, lost = [], [], [], 0
    for i in range(osc.nnodes):
        nd = osc.node(i)
        if nd["is_leaf"] and not nd["is_empty"] and nd["nfaces"] > 0:
            ids.append(i); cnt.append(nd["nfaces"]); lvl.append(nd["depth"])
        elif not nd["is_leaf"] and not nd["is_empty"] and nd["nchildren"] == 0:
            lost += 1
    return np.array(ids, np.int64), np.array(cnt, np.int64), np.array(lvl, np.int64), lost


# ------------------------------------------------------------------------------------------ rays
class Geometry:
    """what the generators read of a scene: float32 corners, centroids and unit normals per face, the box's centre and longest side"""

    def __init__(self, arrays):
        V, vid = arrays["wverts"].astype(F), arrays["face_vid"].astype(np.int64)
        self.A, self.B, self.C = V[vid[:, 0]], V[vid[:, 1]], V[vid[:, 2]]
        self.vid = vid
        self.centroid = ((self.A + self.B + self.C) / F(3)).astype(F)
        self.normal = arrays["face_normal"].astype(F)
        lo, hi = V.min(axis=0), V.max(axis=0)
        self.lo, self.hi = lo, hi
        self.ext = F((hi - lo).max())
        self.c = ((lo + hi) * F(0.5)).astype(F)
        self.nfaces = len(vid)
        e0, e1 = (self.B - self.A).astype(np.float64), (self.C - self.A).astype(np.float64)
        self.area = 0.5 * np.linalg.norm(np.cross(e0, e1), axis=1)

    def duplicates(self):
        """-> [(face, the earliest face with the same vertex triple)], for every face that repeats an earlier one"""
        first, out = {}, []
        for f, key in enumerate(map(tuple, self.vid)):
            if key in first:
                out.append((f, first[key]))
            else:
                first[key] = f
        return out


def _cube(rng, g, n, side):
    return (g.c + (rng.random((n, 3), dtype=F) - F(0.5)) * (F(side) * g.ext)).astype(F)


def _box(rng, n):
    return (rng.random((n, 3), dtype=F) * F(2) - F(1)).astype(F)


def _unit(rng, n):
    u = rng.standard_normal((n, 3))
    return (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(F)


def rays(arrays, seed):
    """-> {family: (origins, directions)} float32, in the families of ORDER"""
    g = Geometry(arrays)
    rng = np.random.default_rng(1000 + seed)
    n = FAMILY
    out = {}
    o = _cube(rng, g, n, 3)
    f = rng.integers(0, g.nfaces, n)
    out["centroid"] = (o, (g.centroid[f] - o).astype(F))
    o = _cube(rng, g, n, 3)
    f = rng.integers(0, g.nfaces, n)
    out["vertex"] = (o, (g.A[f] - o).astype(F))
    o = _cube(rng, g, n, 3)
    f = rng.integers(0, g.nfaces, n)
    out["edge"] = (o, (((g.A[f] + g.B[f]) * F(0.5)).astype(F) - o).astype(F))
    out["random"] = (_cube(rng, g, n, 3), _box(rng, n))
    # axis: +-3 ext along one axis, the other two components +0.0f or -0.0f
    axis, sign = rng.integers(0, 3, n), rng.integers(0, 2, (n, 3))
    d = np.where(sign == 1, F(-0.0), F(0.0)).astype(F)
    d[np.arange(n), axis] = np.where(sign[np.arange(n), axis] == 1, -F(3) * g.ext, F(3) * g.ext)
    f = rng.integers(0, g.nfaces, n)
    out["axis"] = ((g.centroid[f] - (F(2) / F(3)) * d).astype(F), d)
    co, cd = out["centroid"]
    out["long"] = (co.copy(), (cd * F(1e4)).astype(F))
    out["short"] = (co.copy(), (cd * F(1e-4)).astype(F))
    f = rng.integers(0, g.nfaces, n)
    out["onface"] = (g.centroid[f].copy(), _box(rng, n))
    # far: centroid rays from 1e4 extents away
    f = rng.integers(0, g.nfaces, FAR)
    o = (g.c + (F(1e4) * g.ext) * _unit(rng, FAR)).astype(F)
    out["far"] = (o, (g.centroid[f] - o).astype(F))
    # bundle: 16 groups of 64 rays from one origin at 64 barycentric grid points of one face (u + v < 1): the larger faces, so that the
    # 64 points are 64 different directions in float32; every other group starts close to its face, where little else can block
    k = 11
    uv = np.array([((i + 1.0 / 3.0) / k, (j + 1.0 / 3.0) / k) for i in range(k) for j in range(k - i)], F)[:64]
    assert len(uv) == 64 and (uv.sum(axis=1) < 1).all()
    big = np.argsort(-g.area, kind="stable")[:max(1, g.nfaces // 2)]
    bo, bd = [], []
    for b in range(BUNDLES):
        f = int(big[rng.integers(0, len(big))])
        pts = (g.A[f] + uv[:, 0:1] * (g.B[f] - g.A[f]) + uv[:, 1:2] * (g.C[f] - g.A[f])).astype(F)
        nrm = g.normal[f].astype(np.float64)
        ln = np.linalg.norm(nrm)
        if b % 2 == 0 and np.isfinite(ln) and ln > 0:
            org = (g.centroid[f] + (F(0.05) * g.ext * (1 if b % 4 == 0 else -1)) * (nrm / ln).astype(F)).astype(F)
        else:
            org = _cube(rng, g, 1, 3)[0]
        bo.append(np.broadcast_to(org, (64, 3)))
        bd.append((pts - org).astype(F))
    out["bundle"] = (np.concatenate(bo).astype(F), np.concatenate(bd).astype(F))
    # ties: both sides of every face that repeats an earlier face
    to, td = [], []
    for f, _ in g.duplicates():
        nrm = g.normal[f].astype(np.float64)
        ln = np.linalg.norm(nrm)
        if not np.isfinite(nrm).all() or not np.isfinite(ln) or ln == 0:
            continue
        for s in TIE_OFFSETS:
            org = (g.centroid[f] + (F(s) * g.ext) * (nrm / ln).astype(F)).astype(F)
            to.append(org); td.append((g.centroid[f] - org).astype(F))
    out["ties"] = (np.array(to, F).reshape(-1, 3), np.array(td, F).reshape(-1, 3))
    for k_, (a, b) in out.items():
        assert a.dtype == F and b.dtype == F and a.shape == b.shape and a.shape[1] == 3, k_
    return out


def sorted_rays(fam):
    """-> (origins, directions, {family: slice}) family after family"""
    o = np.ascontiguousarray(np.concatenate([fam[k][0] for k in ORDER]), F)
    d = np.ascontiguousarray(np.concatenate([fam[k][1] for k in ORDER]), F)
    where, at = {}, 0
    for k in ORDER:
        where[k] = slice(at, at + len(fam[k][0]))
        at += len(fam[k][0])
    return o, d, where


def interleave(n):
    """-> idx with interleaved[i] = sorted[idx[i]]: a permutation (8191 is prime) that puts every family into every wave"""
    assert n % STRIDE != 0
    idx = (np.arange(n, dtype=np.int64) * STRIDE) % n
    assert len(np.unique(idx)) == n
    return idx


# ------------------------------------------------------------------------------------------ segments
def segments(arrays, seed):
    """-> (hit, light, {family: slice}, info): float32 segments light[i] -> hit[i]; info holds s and the aimed-at face of the `edge` family
    and the aimed-at face of the `graze` family, per segment"""
    g = Geometry(arrays)
    rng = np.random.default_rng(2000 + seed)
    n = FAMILY
    hit, light = [], []
    light.append(_cube(rng, g, n, PAIR_SIDE)); hit.append(_cube(rng, g, n, PAIR_SIDE))
    f = rng.integers(0, g.nfaces, n)
    light.append(_cube(rng, g, n, 1.5)); hit.append(g.centroid[f].copy())
    f = rng.integers(0, g.nfaces, n)
    L = _cube(rng, g, n, 1.5)
    light.append(L); hit.append((F(2) * g.centroid[f] - L).astype(F))
    # the 0.98 edge: the blocker at X has t ~ s.  L lies within EDGE_SIDE ext of X: from further away the dense soups leave fewer than
    # eight segments per s whose only blocker is the face at X (soup 9: none or one with L anywhere in the 1.5 ext cube)
    f = rng.integers(0, g.nfaces, n)
    L = (g.centroid[f] + (rng.random((n, 3), dtype=F) - F(0.5)) * (F(EDGE_SIDE) * g.ext)).astype(F)
    s = np.array(S_EDGE, F)[np.arange(n) % len(S_EDGE)]
    light.append(L); hit.append((L + (g.centroid[f] - L) / s[:, None]).astype(F))
    p = _cube(rng, g, SAME_POINT, 1.5)
    light.append(p); hit.append(p.copy())
    # graze: axis-parallel segments 100 ext long whose blocker, a point X just inside a face next to one of its vertices, has t = S_GRAZE,
    # between the 0.98 of the rule and the 0.981 of the conservative culls.  Seen from the light, a vertex is often the nearest point of
    # its face and of the 64-triangle chunk that holds it, so the padded box of the chunk is entered only a little before X: a chunk test
    # whose margin were below the rule's 0.98 would skip the blocker.  Every (face, vertex, axis, sign), seeded order, GRAZE at the most.
    combos = rng.permutation(g.nfaces * 18)[:GRAZE]
    gf, q, k, sg = combos // 18, (combos % 18) // 6, (combos % 6) // 2, np.where(combos % 2 == 0, F(1), F(-1))
    V = np.stack([g.A, g.B, g.C], axis=1)[gf, q]
    X = (V + F(0.02) * (g.centroid[gf] - V)).astype(F)
    D = np.zeros((len(combos), 3), F)
    D[np.arange(len(combos)), k] = sg * (F(100) * g.ext)
    L = (X - F(S_GRAZE) * D).astype(F)
    light.append(L); hit.append((L + D).astype(F))
    # outside: short segments five extents away, which never meet the root box -- in the interleaved order they thin out the live rays of
    # every wave, so that also a single leaf of 65 faces is walked lanes = triangles (49 live rays at the most)
    L = (g.c + (F(5) * g.ext) * _unit(rng, OUTSIDE)).astype(F)
    light.append(L); hit.append((L + (rng.random((OUTSIDE, 3), dtype=F) - F(0.5)) * (F(0.1) * g.ext)).astype(F))
    where, at = {}, 0
    for name_, a in zip(SEGMENT_FAMILIES + ("same", "graze", "outside"), hit):
        where[name_] = slice(at, at + len(a))
        at += len(a)
    info = {"s": s, "edge_face": f, "graze_face": gf}
    return np.ascontiguousarray(np.concatenate(hit), F), np.ascontiguousarray(np.concatenate(light), F), where, info


# ------------------------------------------------------------------------------------------ non-finite rays
def nonfinite_rays(arrays, seed):
    """-> (origins, directions, finite mask) of 64 rays: 20 with NaN, +inf or -inf in one component of the origin or of the direction, the
    zero direction or three -0.0f, spread over the wave; the others are finite centroid rays"""
    g = Geometry(arrays)
    rng = np.random.default_rng(3000 + seed)
    o = _cube(rng, g, 64, 3)
    f = rng.integers(0, g.nfaces, 64)
    d = (g.centroid[f] - o).astype(F)
    bad = []
    for which in (o, d):
        for comp in range(3):
            for val in (np.nan, np.inf, -np.inf):
                bad.append((which, comp, val))
    finite = np.ones(64, bool)
    for k, (which, comp, val) in enumerate(bad):
        which[3 * k + 1, comp] = F(val)
        finite[3 * k + 1] = False
    d[3 * 18 + 1] = F(0.0)
    d[3 * 19 + 1] = F(-0.0)
    finite[[3 * 18 + 1, 3 * 19 + 1]] = False
    return o, d, finite


# ------------------------------------------------------------------------------------------ the checker's answers
def reference_hits(osc, o, d):
    """the checker's closest_hit per ray -> (face int32, t float32); -1 / -1.0f for a miss"""
    f, t = np.empty(len(o), np.int32), np.empty(len(o), F)
    for i in range(len(o)):
        ff, tt = osc.closest_hit(o[i], d[i])
        f[i], t[i] = (ff, tt) if ff >= 0 else (-1, -1.0)
    return f, t


def reference_strikes(osc, hit, light):
    """the checker's lightStrikes, called per segment -> visible, uint8"""
    return np.array([osc.light_strikes(hit[i], light[i:i + 1])[1][0] for i in range(len(hit))], np.uint8)
