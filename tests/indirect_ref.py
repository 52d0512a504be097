"""The one-bounce diffuse gather as include/rt_mi355x.h defines it ("indirect diffuse"), restated in numpy float32 -- test infrastructure only.

Every float32 step is one numpy float32 operation (numpy rounds each on its own, there is no FMA; its float32 division and square root are
correctly rounded), in the order the header writes.  Directions, rotation and frame are those of tests/ao_ref.py.  The closest hit of a
gather ray and the visibility of a light position come from a `tracer`, of which there are two: OracleTracer asks the CPU checker
(OracleScene.closest_hit / light_strikes), LibraryTracer the host-pointer calls rt_closest_hits / rt_light_strikes, batched.  The arithmetic
around them is the same code, so where the two tracers agree (tests/test_gpu_indirect.py shows it where both are affordable) either stands
for the definition."""
import ctypes as C
import os

import numpy as np

import ao_ref

F = np.float32


def dot3(a, b):
    """a0*b0 + (a1*b1 + a2*b2), the order of dot3 in rt_kernels.hip"""
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def normalized(v):
    """Eigen's normalized(): v / sqrt(squaredNorm) when that is > 0, else v"""
    v = np.asarray(v, F)
    q = dot3(v, v)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(q)
        out = (v / s[..., None]).astype(F)
    keep = ~(q > 0)
    out[keep] = v[keep]
    return out


def directions(N, i, seed, m):
    """the gather directions d, float32 (n, K, 3): d_q of the ambient-occlusion section, no radius"""
    N = np.asarray(N, F).reshape(-1, 3)
    n = N.shape[0]
    D = ao_ref.directions(m)
    x, y, z = D[None, :, 0], D[None, :, 1], D[None, :, 2]
    cs = np.array([ao_ref.rotation_cs(r) for r in range(ao_ref.ROTATIONS)], F)[ao_ref.rotation_steps(seed, i)].reshape(n, 2)
    c, s = cs[:, 0:1], cs[:, 1:2]
    T, B = ao_ref.frame(N)
    d = np.empty((n, m * m, 3), F)
    with np.errstate(invalid="ignore", over="ignore"):
        xr = c * x - s * y
        yr = s * x + c * y
        for q in range(3):
            d[:, :, q] = ((xr * T[:, q:q + 1]) + (yr * B[:, q:q + 1])) + (z * N[:, q:q + 1])
    return d


class SceneData:
    """what the definition reads of the scene besides the tracer: the face normals as uploaded, the material of a face, kd of a material"""

    def __init__(self, oracle_scene):
        a = oracle_scene.arrays()
        self.face_normal = np.ascontiguousarray(a["face_normal"], F)
        self.face_mat = np.ascontiguousarray(a["face_mat"], np.int64)
        self.kd = np.array([m[0][:3] for m in oracle_scene.materials()], F).reshape(-1, 3)


class OracleTracer:
    def __init__(self, oracle_scene):
        self.osc = oracle_scene

    def closest(self, o, d):
        f, t = np.empty(len(o), np.int32), np.empty(len(o), F)
        for k in range(len(o)):
            ff, tt = self.osc.closest_hit(o[k], d[k])
            f[k], t[k] = (ff, tt) if ff >= 0 else (-1, -1.0)
        return f, t

    def strikes(self, H, pos):
        """-> bool (len(H), len(pos)): light position l is visible from H[k]"""
        out = np.empty((len(H), len(pos)), bool)
        for k in range(len(H)):
            out[k] = self.osc.light_strikes(H[k], pos)[1]
        return out


class LibraryTracer:
    """rt_closest_hits / rt_light_strikes with host pointers on a context that holds the scene"""

    def __init__(self, rt, ctx):
        self.rt, self.ctx, self.lib = rt, ctx, ctx.lib

    def closest(self, o, d):
        n = len(o)
        o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
        f, t = np.full(n, -7, np.int32), np.full(n, 7, F)
        if n:
            fp = lambda a: a.ctypes.data_as(C.c_void_p)
            self.rt.capi.check(self.lib, self.ctx.handle, self.lib.rt_closest_hits(self.ctx.handle, n, fp(o), fp(d), fp(f), fp(t)), "rt_closest_hits")
        return f, t

    def strikes(self, H, pos):
        n, nl = len(H), len(pos)
        hit = np.ascontiguousarray(np.broadcast_to(np.asarray(H, F)[:, None, :], (n, nl, 3)), F)
        light = np.ascontiguousarray(np.broadcast_to(np.asarray(pos, F)[None, :, :], (n, nl, 3)), F)
        vis = np.full(n * nl, 7, np.uint8)
        if n * nl:
            fp = lambda a: a.ctypes.data_as(C.c_void_p)
            self.rt.capi.check(self.lib, self.ctx.handle, self.lib.rt_light_strikes(self.ctx.handle, n * nl, fp(hit), fp(light), fp(vis)), "rt_light_strikes")
            assert ((vis == 0) | (vis == 1)).all()
        return vis.reshape(n, nl).astype(bool)


class Traced:
    """the part of the definition that does not depend on the light colour: per gather ray whether it hit, and per hit and light whether the
    light is visible and the clamped cosine ct"""

    def __init__(self, n, K, live, hit, kd, vis, ct):
        self.n, self.K, self.live = n, K, live            # live (n,): the point is a point
        self.hit = hit                                    # bool (n, K)
        self.kd = kd                                      # float32 (hits, 3), in raster order of `hit`
        self.vis, self.ct = vis, ct                       # bool / float32 (hits, n_lights)


def trace(tracer, data, P, N, m, seed, pos, i=None):
    P, N = np.asarray(P, F).reshape(-1, 3), np.asarray(N, F).reshape(-1, 3)
    pos = np.asarray(pos, F).reshape(-1, 3)
    n, K = P.shape[0], m * m
    i = np.arange(n) if i is None else np.asarray(i)
    d = directions(N, i, seed, m)
    live = ao_ref.is_point(N)
    o = np.ascontiguousarray(np.broadcast_to(P[:, None, :], (n, K, 3)), F)
    f = np.full((n, K), -1, np.int32)
    t = np.full((n, K), -1.0, F)
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
        ld = normalized(pos[l][None, :] - H)
        with np.errstate(invalid="ignore"):
            ldn = dot3(ld, Nf)
            ct[:, l] = np.where(F(0.0) < ldn, ldn, F(0.0))
    return Traced(n, K, live, hit, kd, vis, ct)


def shade(tr, color, reverse=False):
    """-> out float32 (n, 3).  reverse: the sum over k taken from K - 1 down to 0 -- NOT the definition, for the test of the order"""
    color = np.asarray(color, F).reshape(3)
    Rh = np.zeros((len(tr.kd), 3), F)
    ck = (color[None, :] * tr.kd).astype(F)
    for l in range(tr.vis.shape[1]):
        v = tr.vis[:, l]
        Rh[v] = Rh[v] + ck[v] * tr.ct[v, l:l + 1]
    R = np.zeros((tr.n, tr.K, 3), F)
    R[tr.hit] = Rh
    E = np.zeros((tr.n, 3), F)
    for k in (range(tr.K - 1, -1, -1) if reverse else range(tr.K)):
        E = E + R[:, k]
    out = (E / F(tr.K)).astype(F)
    out[~tr.live] = F(0.0)
    return out


def gather(tracer, data, P, N, m, seed, pos, color, i=None):
    return shade(trace(tracer, data, P, N, m, seed, pos, i), color)


# ---- hand-built scenes ------------------------------------------------------------------------------------------------------------------
# The loader moves a mesh's centroid to the origin and scales its bounding sphere to radius 1 (a similarity, so angles and visibility stay);
# to_world() takes the coordinates the generators below are written in to the world coordinates the tracer works in.
def to_world(oracle_scene, verts):
    """-> f(points (.., 3) in file coordinates) = float32 world coordinates, from the first two vertices of the file and of the loaded mesh"""
    w = np.asarray(oracle_scene.arrays()["wverts"], np.float64)
    v = np.asarray(verts, np.float64)
    k = int(np.argmax(np.abs(v[1] - v[0])))
    s = (w[1, k] - w[0, k]) / (v[1, k] - v[0, k])
    c = v[0] - w[0] / s
    return lambda p: (s * (np.asarray(p, np.float64) - c)).astype(F)


def _write(dirpath, name, mtl, verts, faces):
    obj = [f"mtllib {name}.mtl"] + ["v %.6f %.6f %.6f" % p for p in verts]
    cur = None
    for mat, (a, b, c) in faces:
        if mat != cur:
            obj.append(f"usemtl {mat}")
            cur = mat
        obj.append(f"f {a} {b} {c}")
    os.makedirs(dirpath, exist_ok=True)
    with open(os.path.join(dirpath, name + ".mtl"), "w") as f:
        f.write(mtl)
    path = os.path.join(dirpath, name + ".obj")
    with open(path, "w") as f:
        f.write("\n".join(obj) + "\n")
    return path


TWO_VERTS = [(-5, 1, -5), (5, 1, -5), (0, 1, 5), (0.7, 0.7, -0.2), (0.3, 0.3, -0.2), (0.5, 0.5, 0.3)]


def two_triangles(dirpath, name="two"):
    """a ceiling triangle in the plane y = 1 above the origin, kd (0.5, 0.25, 0.125), and a small blocker in the plane x = y around
    (0.5, 0.5, 0), which hides the point (0, 1, 0) of the ceiling from a light at (1, 0, 0) and from nothing on the y axis"""
    mtl = "newmtl ceiling\nNs 10.0\nKd 0.5 0.25 0.125\nKs 0.5 0.5 0.5\nillum 2\nnewmtl blocker\nNs 10.0\nKd 0.9 0.9 0.9\nKs 0.5 0.5 0.5\nillum 2\n"
    return _write(dirpath, name, mtl, TWO_VERTS, [("ceiling", (1, 2, 3)), ("blocker", (4, 5, 6))])


STRIPS = 8
BINADE_VERTS = [(-4, 0, -4), (4, 0, -4)]          # the first two vertices of binade_ceiling's file (to_world)


def binade_ceiling(dirpath, name="binades"):
    """a floor at y = 0 and a ceiling at y = 1 of STRIPS strips along x, strip j of kd 2^(-6 j) in all three channels: the radiances that
    the gather rays of a point on the floor bring back differ by up to 42 binades, so the order of their float32 sum shows in its bits"""
    mtl, verts, faces = "newmtl floor\nNs 10.0\nKd 0.5 0.5 0.5\nKs 0.5 0.5 0.5\nillum 2\n", [], []

    def quad(mat, p0, p1, p2, p3):
        base = len(verts)
        verts.extend([p0, p1, p2, p3])
        faces.extend([(mat, (base + 1, base + 2, base + 3)), (mat, (base + 1, base + 3, base + 4))])

    quad("floor", (-4, 0, -4), (4, 0, -4), (4, 0, 4), (-4, 0, 4))
    for j in range(STRIPS):
        kd = repr(2.0 ** (-6 * j))
        mtl += f"newmtl strip{j}\nNs 10.0\nKd {kd} {kd} {kd}\nKs 0.5 0.5 0.5\nillum 2\n"
        x0, x1 = -4.0 + j, -3.0 + j
        quad(f"strip{j}", (x0, 1, -4), (x1, 1, -4), (x1, 1, 4), (x0, 1, 4))
    return _write(dirpath, name, mtl, verts, faces)


def binade_points(W):
    """14 points on the floor of binade_ceiling under the strips, normal up; W: to_world of that scene"""
    xs = np.linspace(-0.9, 0.9, 7)
    P = W([[x, 0.0, z] for x in xs for z in (-0.3, 0.4)])
    return P, np.tile(np.array([[0, 1, 0]], F), (len(P), 1))


def quality(orc, osc, width, height, yaw, pos, color, grid, truth_grid, params, seed=0):
    """The measurement of DESIGN.md 6, Indirect diffuse: what a Lambert surface sends back, kd(P) * out, over the hit points of the width x
    height camera at `yaw` (the frame is one call: point index = raster index, misses are "no point"), with grid x grid gather rays, raw and
    filtered with the denoise_ref.Params `params`, against truth_grid x truth_grid rays.  -> dict: pixels (those where the truth is not
    zero), raw / filtered (RMS distances over them) and ratio = filtered / raw."""
    import denoise_ref
    import gbuffer_ref
    (o, d, f, t), _ = ao_ref.camera_points(orc, osc, width, height, yaw)
    P, N = ao_ref.hit_points(o, d, f, t, osc.arrays()["face_normal"])
    kd_face = gbuffer_ref.face_kd(osc)
    g = gbuffer_ref.sample_values(f.reshape(height, width), t.reshape(height, width), osc.arrays()["face_normal"], kd_face)
    data, tracer = SceneData(osc), OracleTracer(osc)
    albedo = np.zeros((len(f), 3), F)
    albedo[f >= 0] = data.kd[data.face_mat[f[f >= 0]]]

    def image(m):
        return (albedo * gather(tracer, data, P, N, m, seed, pos, color)).reshape(height, width, 3)

    truth, raw = image(truth_grid), image(grid)
    mask = (truth != 0).any(axis=-1)
    filtered = denoise_ref.denoise(raw, g, params)

    def rms(a):
        e = (np.asarray(a, np.float64) - np.asarray(truth, np.float64))[mask]
        return float(np.sqrt((e * e).mean()))

    out = {"pixels": int(mask.sum()), "covered": int((f >= 0).sum()), "raw": rms(raw), "filtered": rms(filtered)}
    out["ratio"] = out["filtered"] / out["raw"]
    return out
