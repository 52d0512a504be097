"""The light jitter defined with rt_light_jitter_offsets (include/rt_mi355x.h) restated in Python: the offsets of a pass in host double, the sample positions
in float32 with an explicit cast after every operation, and a depth-0 pass frame composed from the CPU oracle's pieces.

Test infrastructure only.  The frame is NOT the oracle's renderer: orc_render knows the cell centres only.  It is put together from the parts
of traceRay that the oracle exports -- screen_to_world at the pass's raster point, closest_hit, light_strikes on the light positions (the
centre rays) and then on the samples, orc_interp_normal, the per-sample term phong_ref of tests/test_gpu_phong_samples.py and the in-order sum
colour * (sum / N) * (1.3f / N) -- so that the samples can be placed where the definition puts them.  With (fu, fv) = (0.5, 0.5) and no raster
shift it equals orc_render(max_depth = 0) bit for bit (tests/test_light_jitter_api.py)."""
import ctypes as C

import numpy as np

import passes_ref
import test_gpu_phong_samples as ps

F = np.float32
RT_MAX_PASSES = passes_ref.RT_MAX_PASSES
BACKGROUND = np.array([1.0, 1.0, 1.0], F)        # a primary ray that hits nothing
SHADOW = np.array([0.0, 0.0, 0.0], F)            # a hit none of whose light positions is visible
CENTRE = (F(0.5), F(0.5))
_fp = C.POINTER(C.c_float)


def jitter_offsets(p):
    """(fu, fv) of pass p: (float)(0.5 + e_5(p)), (float)(0.5 + e_7(p)), e_b the wrapped radical inverse of rt_set_passes"""
    return F(0.5 + passes_ref.wrapped(p, 5)), F(0.5 + passes_ref.wrapped(p, 7))


def library_offsets(lib, p):
    """rt_light_jitter_offsets as two float32"""
    fu, fv = C.c_float(float("nan")), C.c_float(float("nan"))
    assert lib.rt_light_jitter_offsets(p, C.byref(fu), C.byref(fv)) == 0
    return F(fu.value), F(fv.value)


def light_samples(usteps, vsteps, len_x, len_y, corner, fo):
    """[usteps * vsteps, 3]: sample (i, j) at index i * vsteps + j = (((float)i + fu) * cx, ((float)j + fv) * cy, z); cx, cy, z as light_grid"""
    c = np.asarray(corner, F)
    cx = F(F(c[0] + F(F(len_x) * F(1.0))) / F(usteps))
    cy = F(F(c[1] + F(F(len_y) * F(1.0))) / F(vsteps))
    z = F(c[2] + F(F(len_x) * F(0.0)))
    out = np.empty((usteps * vsteps, 3), F)
    for i in range(usteps):
        fi = F(F(i) + F(fo[0]))
        for j in range(vsteps):
            fj = F(F(j) + F(fo[1]))
            out[i * vsteps + j] = (F(fi * cx), F(fj * cy), z)
    return out


class PassShader:
    """traceRay at depth 0 for one scene, camera and set of area lights, the samples shifted by fo"""

    def __init__(self, orc, osc, cam, L, fo):
        ps.bind_powf(orc)
        self.orc, self.osc, self.cam = orc, osc, cam
        self.org = np.array(list(cam.center), F)
        self.color = np.array(list(L.color), F)
        self.points = np.array([[L.pos[l][k] for k in range(3)] for l in range(L.nlights)], F)
        self.N = L.usteps * L.vsteps
        self.samples = [light_samples(L.usteps, L.vsteps, L.len_x, L.len_y, lp, fo) for lp in self.points]
        self.mats = osc.materials()
        self.face_mat = osc.arrays()["face_mat"]

    def colour(self, x, y):
        """(rgb, the light of some scene light is partly visible) for the primary ray through raster point (x, y)"""
        orc, osc, org, N = self.orc, self.osc, self.org, self.N
        d = (orc.screen_to_world(self.cam, x, y) - org).astype(F)
        face, t = osc.closest_hit(org, d)
        if face < 0:
            return BACKGROUND, False
        hit = (org + (F(t) * d).astype(F)).astype(F)
        if not osc.light_strikes(hit, self.points)[0]:
            return SHADOW, False
        nrm = np.zeros(3, F)
        orc.lib.orc_interp_normal(osc.h, hit.ctypes.data_as(_fp), face, nrm.ctypes.data_as(_fp))
        nrm = np.array(ps.normalized(list(nrm)), F)
        eye = np.array(ps.normalized(list((F(-1.0) * (hit - org).astype(F)).astype(F))), F)
        mat = self.mats[int(self.face_mat[face])][0]
        lkd, lks = (self.color * mat[0:3]).astype(F), (self.color * mat[3:6]).astype(F)
        final = np.zeros(3, F)
        partial = False
        for smp in self.samples:
            vis = osc.light_strikes(hit, smp)[1]
            partial = partial or 0 < int(vis.sum()) < N
            rep = lambda v: np.ascontiguousarray(np.broadcast_to(v, (N, 3)), F)
            term = ps.phong_ref(orc, {"hit": rep(hit), "nrm": rep(nrm), "eye": rep(eye), "smp": smp, "lkd": rep(lkd), "lks": rep(lks),
                                      "shin": np.full(N, mat[6], F)})
            col, sm = np.zeros(3, F), F(0.0)
            for s in range(N):                                   # the visible samples in index order
                if vis[s]:
                    sm = F(sm + F(1.0))
                    col = (col + term[s, 3:6]).astype(F)
            final = (final + ((col * F(sm / F(N))).astype(F) * F(F(1.3) / F(N))).astype(F)).astype(F)
        return final, partial


def pass_frame(orc, osc, cam, L, w, h, fo=CENTRE, ox=(0.0,), oy=(0.0,)):
    """(frame [h, w, 3], partly-lit mask [h, w]) of one pass at depth 0: the area lights L (an oracle olights) sampled at fo, sub-sample
    (sx, sy) of pixel (i, j) through the raster point ((float)i + ox[sx], (float)j + oy[sy]), folded as rt_set_supersampling defines."""
    n = len(ox)
    assert len(oy) == n
    sh = PassShader(orc, osc, cam, L, fo)
    out = np.empty((h, w, 3), F)
    mask = np.zeros((h, w), bool)
    for j in range(h):
        for i in range(w):
            acc = np.zeros(3, F)
            for sy in range(n):
                for sx in range(n):
                    rgb, part = sh.colour(F(F(i) + F(ox[sx])), F(F(j) + F(oy[sy])))
                    mask[j, i] = mask[j, i] or part
                    acc = (acc + rgb).astype(F)
            out[j, i] = rgb if n == 1 else (acc / F(n * n)).astype(F)
    return out, mask


def jittered_pass(orc, osc, cam, L, w, h, p, n=1, jitter=True):
    """pass p of a frame with the jitter on (or off): its raster offsets are rt_set_passes', its light offsets jitter_offsets(p)"""
    ox, oy = passes_ref.pass_offsets(n, p)
    return pass_frame(orc, osc, cam, L, w, h, jitter_offsets(p) if jitter else CENTRE, ox, oy)
