"""The per-sample arithmetic of the shading kernels (phong_sample: normalize3_shared twice, pow_shininess) through rt_debug_phong_samples.

The device code chooses its paths by wave-uniform tests, so the cases are laid out in whole waves: every kind of case once as all 64 lanes of a
wave and once as a few lanes among ordinary ones, which runs both sides of every test and the mixing.  The expected values are a float32
restatement in numpy with the operation order of phong_sample (dot3 = ax*bx + (ay*by + az*bz), IEEE sqrt and /) and the oracle's orc_powf;
all six outputs of every case are compared as bit patterns.  The restatement itself is tied to the oracle's own phongShade on the CPU.

The cases keep invalid operations (0 * inf, inf / inf) out of the arithmetic: the NaN such an operation creates has no sign the two machines
agree on.  NaNs that are passed through (a NaN shininess) keep their bits on both.
"""
import ctypes as C
import os

import numpy as np
import pytest

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")
LANES = (0, 37, 63)                       # where the odd cases sit in a mixed wave
ONE_UP = np.nextafter(F(1.0), F(2.0))


def dot3(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def normalized(v):
    """Eigen's normalized(): v / sqrt(squaredNorm) where that is > 0 (what normalize3_shared computes on every one of its paths)"""
    q = dot3(v, v)
    s = np.sqrt(q)
    pos = q > 0
    safe = np.where(pos, s, F(1.0))
    return [np.where(pos, c / safe, c) for c in v]


def smax0(x):
    return np.where(F(0.0) < x, x, F(0.0)).astype(F)          # std::max(0.0f, x): NaN and -0 give +0


def reflection(hit, nrm, smp):
    """(ldn, unit reflection vector) of phong_sample"""
    ld = normalized([smp[k] - hit[k] for k in range(3)])
    ldn = dot3(ld, nrm)
    two = F(2.0) * ldn
    return ldn, normalized([ld[k] - two * nrm[k] for k in range(3)])


def phong_ref(orc, c):
    """the six outputs of rt_debug_phong_samples for the cases c (dict of float32 arrays: hit, nrm, eye, smp, lkd, lks [n, 3], shin [n])"""
    with np.errstate(all="ignore"):
        hit, nrm, eye, smp = ([c[k][:, j] for j in range(3)] for k in ("hit", "nrm", "eye", "smp"))
        ldn, r = reflection(hit, nrm, smp)
        costheta = smax0(ldn)
        cosphi = smax0(dot3(eye, [F(-1.0) * r[k] for k in range(3)]))
        pw = np.array([orc.lib.orc_powf(float(x), float(y)) for x, y in zip(cosphi, c["shin"])], F)
        out = np.empty((ldn.size, 6), F)
        out[:, 0], out[:, 1], out[:, 2] = ldn, cosphi, pw
        for k in range(3):
            out[:, 3 + k] = c["lkd"][:, k] * costheta + c["lks"][:, k] * pw
    return out


def bind_powf(orc):
    orc.lib.orc_powf.restype = C.c_float
    orc.lib.orc_powf.argtypes = [C.c_float, C.c_float]


# ---------------------------------------------------------------------------------------------------------------- the cases
def ordinary(rng, m):
    """m cases with every light-vector and reflection component well away from zero, cosphi in (0, 1), shininess 10"""
    n = 4 * m + 64
    sign = lambda shape: np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    hit = rng.uniform(-1, 1, (n, 3)).astype(F)
    smp = (hit + sign((n, 3)) * rng.uniform(0.3, 1.5, (n, 3))).astype(F)
    nrm = np.stack(normalized(list((sign((n, 3)) * rng.uniform(0.2, 1.0, (n, 3))).astype(F).T)), 1).astype(F)
    _, r = reflection(list(hit.T), list(nrm.T), list(smp.T))
    eye = np.stack(normalized([(-r[k] + rng.uniform(-0.4, 0.4, n)).astype(F) for k in range(3)]), 1).astype(F)
    c = {"hit": hit, "nrm": nrm, "eye": eye, "smp": smp, "lkd": rng.uniform(0.1, 1.0, (n, 3)).astype(F), "lks": rng.uniform(0.1, 1.0, (n, 3)).astype(F),
         "shin": np.full(n, 10.0, F)}
    cosphi = smax0(dot3(list(eye.T), [F(-1.0) * r[k] for k in range(3)]))
    rmin = np.min(np.abs(np.stack(r, 1)), 1)
    keep = np.flatnonzero((cosphi > 0.05) & (cosphi < 0.999) & (rmin > 1e-3))[:m]
    assert keep.size == m
    return {k: v[keep].copy() for k, v in c.items()}


def with_eye(c, f):
    """eye = f(unit reflection vector, per component)"""
    _, r = reflection(list(c["hit"].T), list(c["nrm"].T), list(c["smp"].T))
    c["eye"] = np.stack([f(r[k]) for k in range(3)], 1).astype(F)
    return c


def cosphi_of(c):
    _, r = reflection(list(c["hit"].T), list(c["nrm"].T), list(c["smp"].T))
    return smax0(dot3(list(c["eye"].T), [F(-1.0) * r[k] for k in range(3)]))


def pick(c, mask, m):
    idx = np.flatnonzero(mask)[:m]
    assert idx.size == m, (idx.size, m)
    return {k: v[idx].copy() for k, v in c.items()}


def kinds(rng):
    """name -> builder(m) of m cases of that kind"""
    def shin(value):
        def make(m):
            c = ordinary(rng, m)
            c["shin"][:] = value
            return c
        return make

    def base_half(value):                                   # cosphi = 0.5 up to rounding: y log2 x = -value up to 1e-5
        def make(m):
            c = with_eye(ordinary(rng, m), lambda r: F(-0.5) * r)
            c["shin"][:] = value
            return c
        return make

    def eye_search(want):                                   # eye = -r: cosphi is 1 up to an ulp; keep the cases where it is exactly `want`
        def make(m):
            c = with_eye(ordinary(rng, 4096), lambda r: F(-1.0) * r)
            return pick(c, cosphi_of(c) == want, m)
        return make

    def smp_offset(f):
        def make(m):
            c = ordinary(rng, m)
            c["smp"] = f(c).astype(F)
            return c
        return make

    def zero_x(c):                                          # light vector (0, a, b)
        s = c["smp"].copy(); s[:, 0] = c["hit"][:, 0]
        return s

    def refl_zero(m):                                       # light vector (0, a, b) and normal (0, c, d): reflection (0, ., .) exactly
        c = ordinary(rng, m)
        c["smp"][:, 0] = c["hit"][:, 0]
        c["nrm"][:, 0] = 0.0
        return c

    def tiny_x(m):                                          # light vector (1e-25, a, b): below the fast path's 2^-60
        c = ordinary(rng, m)
        c["hit"][:, 0] = 0.0
        c["smp"][:, 0] = 1e-25
        return c

    def combine(make, **fixed):
        def f(m):
            c = make(m)
            for k, v in fixed.items():
                c[k][:] = v
            return c
        return f

    zero = lambda m: with_eye(ordinary(rng, m), lambda r: r)                       # eye behind the reflected ray: cosphi = +0
    k = {
        "cosphi_zero": zero,
        "cosphi_one": eye_search(F(1.0)),
        "cosphi_one_up": eye_search(ONE_UP),
        "cosphi_subnormal": lambda m: with_eye(ordinary(rng, m), lambda r: F(-(2.0 ** -140)) * r),
        "shin_1e-3": shin(1e-3), "shin_1e4": shin(1e4),
        "ylogx_-140": base_half(140.0), "ylogx_-149.5": base_half(149.5), "ylogx_-200": base_half(200.0),
        "shin_zero": shin(0.0), "shin_negative": shin(-2.5), "shin_inf": shin(np.inf), "shin_nan": shin(np.nan),
        "zero_base_negative_shin": combine(zero, shin=-2.5), "zero_base_inf_shin": combine(zero, shin=np.inf), "zero_base_zero_shin": combine(zero, shin=0.0),
        "one_up_inf_shin": combine(eye_search(ONE_UP), shin=np.inf), "one_nan_shin": combine(eye_search(F(1.0)), shin=np.nan),
        "subnormal_negative_shin": combine(lambda m: with_eye(ordinary(rng, m), lambda r: F(-(2.0 ** -140)) * r), shin=-0.5),
        "light_zero_component": smp_offset(zero_x),
        "light_1e-25_component": tiny_x,
        "light_length_1e25": smp_offset(lambda c: np.sign(c["smp"] - c["hit"]) * np.array([1e25, 2e25, 1.5e25])),
        "light_length_zero": smp_offset(lambda c: c["hit"]),
        "reflection_zero_component": refl_zero,
    }
    return k


def build_cases():
    """(cases, names): names[w] = what wave w holds"""
    rng = np.random.default_rng(20261017)
    waves, names = [ordinary(rng, 64)], ["ordinary"]
    for name, make in kinds(rng).items():
        waves.append(make(64)); names.append(name + " x64")
        mixed, odd = ordinary(rng, 64), make(len(LANES))
        for j, lane in enumerate(LANES):
            for key in mixed:
                mixed[key][lane] = odd[key][j]
        waves.append(mixed); names.append(name + " in ordinary")
    # several kinds in one wave, one lane each, among ordinary lanes
    mixed = ordinary(rng, 64)
    for j, make in enumerate(kinds(rng).values()):
        odd = make(1)
        for key in mixed:
            mixed[key][2 * j + 1] = odd[key][0]
    waves.append(mixed); names.append("all kinds in ordinary")
    cases = {k: np.ascontiguousarray(np.concatenate([w[k] for w in waves]).astype(F)) for k in waves[0]}
    return cases, names


@pytest.fixture(scope="module")
def cases():
    c, names = build_cases()
    return c, names


def test_cases_cover_the_kinds_they_claim(oracle, cases):
    """the case builder on its own terms (no GPU): every named kind is what its name says, in both forms"""
    bind_powf(oracle)
    c, names = cases
    ref = phong_ref(oracle, c)
    n = ref.shape[0]
    assert n % 64 == 0 and 40 <= n // 64 <= 80
    cosphi, shin = ref[:, 1], c["shin"]
    wave = lambda name: slice(names.index(name) * 64, names.index(name) * 64 + 64)
    o = wave("ordinary")
    assert ((cosphi[o] > 0) & (cosphi[o] < 1)).all() and (shin[o] == 10).all()
    assert (cosphi[wave("cosphi_zero x64")].view(np.uint32) == 0).all()
    assert (cosphi[wave("cosphi_one x64")] == 1).all() and (cosphi[wave("cosphi_one_up x64")] == ONE_UP).all()
    sub = cosphi[wave("cosphi_subnormal x64")]
    assert ((sub > 0) & (sub < np.finfo(F).tiny)).all()
    with np.errstate(all="ignore"):
        ylogx = shin.astype(np.float64) * np.log2(cosphi.astype(np.float64))
    a, b, d = ylogx[wave("ylogx_-140 x64")], ylogx[wave("ylogx_-149.5 x64")], ylogx[wave("ylogx_-200 x64")]
    assert ((a > -149) & (a <= -126)).all() and ((b > -150) & (b < -149)).all() and (d < -150).all()
    assert (ref[wave("ylogx_-149.5 x64"), 2].view(np.uint32) == 1).all() and (ref[wave("ylogx_-200 x64"), 2] == 0).all()
    ld = c["smp"] - c["hit"]
    assert (ld[wave("light_zero_component x64"), 0] == 0).all() and (ld[wave("light_length_zero x64")] == 0).all()
    small = np.abs(ld[wave("light_1e-25_component x64"), 0])
    assert ((small > 0) & (small < 2.0 ** -60)).all()
    assert (np.abs(ld[wave("light_length_1e25 x64")]) > 1e24).all()
    m = wave("shin_nan in ordinary")
    assert np.isnan(shin[m]).sum() == len(LANES) and np.isnan(ref[m, 2]).sum() == len(LANES)
    # nothing in the expected values comes from an invalid operation: the only NaNs are the ones a NaN shininess passes on
    assert (np.isnan(shin) | ~np.isnan(ref).any(1)).all()


def test_restatement_equals_the_oracles_phong_term(oracle):
    """the numpy restatement against the oracle's own phongShade (orc_phong), bit for bit: cube.obj, the point light, primary rays of a 16 x 16
    frame.  One visible sample: phongShade returns ((0 + term) * (1 / 1)) * (1.3f / 1)."""
    bind_powf(oracle)
    pf = C.POINTER(C.c_float)
    oracle.lib.orc_phong.restype = None
    oracle.lib.orc_phong.argtypes = [C.c_void_p, C.c_void_p, pf, pf, C.c_int, pf, C.c_int, pf, C.c_void_p]
    osc = oracle.load_scene(os.path.join(SCENES, "cube.obj"))
    w = h = 16
    cam, L = oracle.camera(w, h), oracle.lights(area=False)
    org = np.array(list(cam.center), F)
    light = np.array([L.pos[0][k] for k in range(3)], F)
    kd_ks, _ = osc.materials()[0]
    color = np.array(list(L.color), F)
    rows, want = [], []
    for j in range(h):
        for i in range(w):
            d = (oracle.screen_to_world(cam, i, j) - org).astype(F)
            face, t = osc.closest_hit(org, d)
            if face < 0:
                continue
            hit = (org + F(t) * d).astype(F)
            if not osc.light_strikes(hit, light[None, :])[1][0]:
                continue
            nrm = np.zeros(3, F)
            oracle.lib.orc_interp_normal(osc.h, hit.ctypes.data_as(pf), face, nrm.ctypes.data_as(pf))     # (the cube's model matrix is the identity)
            out = np.zeros(3, F)
            oracle.lib.orc_phong(osc.h, C.byref(L), org.ctypes.data_as(pf), hit.ctypes.data_as(pf), face, light.ctypes.data_as(pf), 1, out.ctypes.data_as(pf), None)
            mat = osc.materials()[int(osc.arrays()["face_mat"][face])][0]
            rows.append((hit, nrm, F(-1.0) * (hit - org), mat))
            want.append(out)
    assert len(rows) >= 16
    stack = lambda k: np.stack([r[k] for r in rows]).astype(F)
    hit, nrm, eye = stack(0), np.stack(normalized(list(stack(1).T)), 1).astype(F), np.stack(normalized(list(stack(2).T)), 1).astype(F)
    mats = np.stack([r[3] for r in rows]).astype(F)
    c = {"hit": hit, "nrm": nrm, "eye": eye, "smp": np.broadcast_to(light, hit.shape).astype(F), "lkd": (color[None, :] * mats[:, 0:3]).astype(F),
         "lks": (color[None, :] * mats[:, 3:6]).astype(F), "shin": mats[:, 6].copy()}
    ref = phong_ref(oracle, c)
    assert ((ref[:, 1] > 0) & (ref[:, 1] < 1)).sum() >= 8                 # ordinary cases: cosphi in (0, 1)
    got = ((F(0.0) + ref[:, 3:6]) * F(1.0)) * (F(1.3) / F(1.0))
    assert np.array_equal(got.astype(F).view(np.uint32), np.stack(want).view(np.uint32))
    osc.close()


@pytest.mark.gpu
def test_gpu_phong_samples_equal_the_restatement(rt, oracle, cases):
    """all six outputs of every case, as bit patterns"""
    bind_powf(oracle)
    c, names = cases
    ref = phong_ref(oracle, c)
    n = ref.shape[0]
    got = np.zeros((n, 6), F)
    ctx = rt.Context(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ctx.lib.rt_debug_phong_samples(ctx.handle, n, vp(c["hit"]), vp(c["nrm"]), vp(c["eye"]), vp(c["smp"]), vp(c["lkd"]), vp(c["lks"]), vp(c["shin"]), vp(got))
    rt.capi.check(ctx.lib, ctx.handle, rc, "rt_debug_phong_samples")
    ctx.close()
    bad = np.flatnonzero((got.view(np.uint32) != ref.view(np.uint32)).any(1))
    print(f"{n} cases in {n // 64} waves, {bad.size} differ")
    for i in bad[:8]:
        print(names[i // 64], "lane", i % 64, "got", got[i], "want", ref[i])
    assert bad.size == 0, sorted({names[i // 64] for i in bad})


@pytest.mark.gpu
def test_gpu_phong_samples_rejects_partial_waves(rt):
    ctx = rt.Context(0)
    z = np.zeros((96, 3), F)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert ctx.lib.rt_debug_phong_samples(ctx.handle, 96, vp(z), vp(z), vp(z), vp(z), vp(z), vp(z), vp(z), vp(z)) != rt.capi.RT_OK
    ctx.close()
