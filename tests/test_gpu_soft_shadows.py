"""Soft shadows on a real MI355X: rt_soft_shadows_device returns, per point, bit for bit the count of the segments that rt_light_strikes
(and the CPU checker's lightStrikes) calls visible, the segments being built on the host from rt_light_samples and rt_shadow_jitter -- in
every wave layout, for every batch length around the unit boundaries, in the strided rounds, beside frames in flight; it writes nothing
behind element n, refuses what the header says it refuses and leaves the context as it was."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ao_ref
import grid_caps as gc
import scenes_gen
import shadow_ref
import switch_table
from test_gpu_ao import GUARD, In, Out, same  # noqa: F401 -- the guarded device arrays of the occlusion tests

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 48, 32
FILES = {"cube": "cube.obj", "dodge": "dodgeColorTest.obj"}
# three light positions; the first (with the default light lengths) puts penumbrae on every scene of this file at 48 x 32
THREE = ((0.6, 1.2, 0.2), (1.5, 1.5, 0.5), (0.8, 0.4, 1.5))
# 25 light positions on a 5 x 5 lattice above the scenes
MANY = tuple((-1.0 + 0.45 * (k % 5), 0.3 + 0.3 * (k // 5), 1.0 + 0.05 * k) for k in range(25))
# name -> (positions, area, usteps, vsteps): K = 1, 4, 25, 64, 21, 256, 50, 75 -- a wave unit of 64, 16, 64, 1, 64, 1, 32, 64 points in 1, 1,
# 25, 1, 21, 4, 25, 75 rounds: K dividing 64, 64 dividing K, and the K whose points straddle rounds, with one light and with several
LIGHTS = {"point": (THREE[:1], False, 1, 1), "2x2": (THREE[:1], True, 2, 2), "5x5": (THREE[:1], True, 5, 5), "8x8": (THREE[:1], True, 8, 8),
          "3x7": (THREE[:1], True, 3, 7), "16x16": (THREE[:1], True, 16, 16), "2 lights": (THREE[:2], True, 5, 5), "3 lights": (THREE, True, 5, 5)}
PARAMS = {"centre": dict(), "pass5": dict(pass_offsets=5), "seed0": dict(per_point=True, seed=0), "seed7": dict(per_point=True, seed=7)}


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def make_lights(rt, name):
    pos, area, u, v = LIGHTS[name] if name in LIGHTS else (MANY, True, 32, 32)
    return rt.make_lights(points=pos, area=area, usteps=u, vsteps=v)


def make_params(rt, lib, name):
    kw = dict(PARAMS[name])
    if "pass_offsets" in kw:
        fu, fv = C.c_float(), C.c_float()
        assert lib.rt_light_jitter_offsets(kw.pop("pass_offsets"), C.byref(fu), C.byref(fv)) == 0
        kw.update(fu=fu.value, fv=fv.value)
    return rt.shadow_params(**kw)


class Scene:
    """a scene on the GPU and in the CPU checker, and its fixed point set: the hit points of ALL rays of the 48 x 32 camera at yaw 0.4 through
    closest_hits / hit_points on the device, misses (six zeros) included"""

    def __init__(self, rt, oracle, path):
        self.rt, self.orc = rt, oracle
        self.fs = rt.Flyscene(scene_path=path)
        self.fs.initialize(64, 40, True, False)
        self.ctx, self.lib = self.fs.ctx, self.fs.ctx.lib
        self.osc = oracle.load_scene(path)
        self.rays, _ = ao_ref.camera_points(oracle, self.osc, W, H, 0.4)
        o, d, f, t = self.rays
        self.n = len(o)
        io, id_ = In(rt, o), In(rt, d)
        faces, ts = self.ctx.closest_hits(io.buf, id_.buf, n=self.n)
        points, normals = self.ctx.hit_points(io.buf, id_.buf, faces, ts, n=self.n)
        self.ctx.synchronize()
        self.P, self.N = points.to_numpy(F, (self.n, 3)), normals.to_numpy(F, (self.n, 3))
        wantP, wantN = ao_ref.hit_points(o, d, f, t, self.osc.arrays()["face_normal"])
        assert same(self.P, wantP) and same(self.N, wantN)
        self.hit = f >= 0
        assert 0 < int(self.hit.sum()) < self.n, "the frame must hold hits and misses"
        for a in (self.P, self.N, self.hit):
            a.setflags(write=False)
        self.ref = {}

    def samples(self, L, sp, n, first=0):
        """float32 (n, K, 3): the samples point first + k of a call sees, from rt_light_samples (and rt_shadow_jitter for a per-point call)"""
        lib = self.lib
        area = L.mode == self.rt.capi.RT_LIGHT_AREA
        N = L.usteps * L.vsteps if area else 1
        out = np.empty((n if sp.per_point else 1, L.n_lights, N, 3), F)
        fu, fv = C.c_float(sp.fu), C.c_float(sp.fv)
        for k in range(out.shape[0]):
            if sp.per_point:
                assert lib.rt_shadow_jitter(sp.seed, first + k, C.byref(fu), C.byref(fv)) == 0
            for l in range(L.n_lights):
                assert lib.rt_light_samples(C.byref(L), l, fu, fv, out[k, l].ctypes.data_as(C.c_void_p)) == 0
        return np.broadcast_to(out.reshape(out.shape[0], L.n_lights * N, 3), (n, L.n_lights * N, 3))

    def strikes(self, P, S):
        """rt_light_strikes on the segments S[i, e] -> P[i]: visible, bool (n, K)"""
        n, K = S.shape[0], S.shape[1]
        hit = np.ascontiguousarray(np.broadcast_to(P[:, None, :], S.shape), F)
        light = np.ascontiguousarray(S, F)
        vis = np.full(n * K, 7, np.uint8)
        fp = lambda a: a.ctypes.data_as(C.c_void_p)
        self.rt.capi.check(self.lib, self.ctx.handle, self.lib.rt_light_strikes(self.ctx.handle, n * K, fp(hit), fp(light), fp(vis)), "rt_light_strikes")
        assert ((vis == 0) | (vis == 1)).all()
        return vis.reshape(n, K).astype(bool)

    def counts_by_strikes(self, L, sp, P, N=None):
        """the expected `visible`: the segments from rt_light_samples, given to rt_light_strikes, counted; K for a "no point" """
        P = np.ascontiguousarray(P, F)
        n = len(P)
        S = self.samples(L, sp, n)
        live = shadow_ref.is_point(N, n)
        out = np.full(n, S.shape[1], np.uint16)
        if live.any():
            out[live] = self.strikes(P[live], S[live]).sum(axis=1).astype(np.uint16)
        return out

    def counts(self, lights, params):
        """... of the fixed point set, computed once per (lights, params)"""
        key = (lights, params)
        if key not in self.ref:
            self.ref[key] = self.counts_by_strikes(make_lights(self.rt, lights), make_params(self.rt, self.lib, params), self.P, self.N)
            self.ref[key].setflags(write=False)
        return self.ref[key]

    def close(self):
        self.ctx.close()
        self.fs.scene.close()
        self.osc.close()


@pytest.fixture(scope="module")
def world(rt, oracle, scenes, tmp_path_factory):
    paths = {k: os.path.join(scenes, v) for k, v in FILES.items()}
    paths["mixed"] = scenes_gen.mixed_materials(str(tmp_path_factory.mktemp("mixed")))
    w = {k: Scene(rt, oracle, p) for k, p in paths.items()}
    yield w
    for s in w.values():
        s.close()


def run(sc, L, sp, P, N, want_visible=True, want_share=True, stream=None, sync=True):
    """rt_soft_shadows_device on DeviceBuffers with guards -> (visible, share) as read back (None where left out); N None: no normal array"""
    n = len(P)
    p = In(sc.rt, P.reshape(-1, 3) if n else np.zeros((1, 3), F))
    nr = None if N is None else In(sc.rt, N.reshape(-1, 3) if n else np.zeros((1, 3), F))
    v = Out(sc.rt, n, 1, np.uint16) if want_visible else None
    s = Out(sc.rt, n, 1, np.float32) if want_share else None
    sc.ctx.soft_shadows(p.buf, nr.buf if nr else None, L, sp, n=n, visible=v.buf if v else None, share=s.buf if s else None,
                        want_visible=want_visible, want_share=want_share, stream=stream)
    if not sync:
        return v, s, (p, nr)
    sc.ctx.synchronize()
    p.check()
    if nr:
        nr.check()
    return (v.read() if v else None), (s.read() if s else None)


# ------------------------------------------------------------------------------------------ 1. exactness against rt_light_strikes
@pytest.mark.parametrize("params", list(PARAMS))
@pytest.mark.parametrize("name", ["cube", "dodge", "mixed"])
def test_counts_equal_light_strikes_in_every_layout(world, name, params):
    sc = world[name]
    sp = make_params(sc.rt, sc.lib, params)
    for lights in LIGHTS:
        L = make_lights(sc.rt, lights)
        K = L.n_lights * (L.usteps * L.vsteps if L.mode == sc.rt.capi.RT_LIGHT_AREA else 1)
        want = sc.counts(lights, params)
        vis, share = run(sc, L, sp, sc.P, sc.N)
        assert vis.dtype == np.uint16 and np.array_equal(vis, want), (name, lights, params, np.flatnonzero(vis != want)[:8])
        assert same(share, shadow_ref.share_of(want, K)), (name, lights, params)
        assert (want[~sc.hit] == K).all() and same(share[~sc.hit], np.full(int((~sc.hit).sum()), 1.0, F))
    # K = 25,600 on 8 points: 400 rounds of one point
    L = make_lights(sc.rt, "many")
    pick = np.flatnonzero(sc.hit)[np.linspace(0, int(sc.hit.sum()) - 1, 8).astype(int)]
    P, N = sc.P[pick], sc.N[pick]
    want = sc.counts_by_strikes(L, sp, P, N)
    vis, share = run(sc, L, sp, P, N)
    assert np.array_equal(vis, want) and same(share, shadow_ref.share_of(want, 25600)), (name, params, vis, want)
    if name != "cube":
        c = sc.counts("5x5", params)
        assert int(((c > 0) & (c < 25)).sum()) >= 10, "the fixture must hold partly lit points"


def test_jitter_moves_the_samples(world):
    """the four parameter sets are four different questions on a scene with penumbrae"""
    sc = world["mixed"]
    got = [sc.counts("5x5", p) for p in PARAMS]
    for a in range(len(got)):
        for b in range(a + 1, len(got)):
            assert not np.array_equal(got[a], got[b]), (a, b)


# ------------------------------------------------------------------------------------------ 2. against the oracle
@pytest.mark.parametrize("name", ["cube", "dodge", "mixed"])
def test_counts_equal_the_oracle(world, name):
    """independent of the library's walker: the CPU checker's lightStrikes on the restated samples (tests/shadow_ref.py), 200 points"""
    sc = world[name]
    pick = np.linspace(0, sc.n - 1, 200).astype(int)
    P, N = sc.P[pick], sc.N[pick]
    assert 0 < int(sc.hit[pick].sum()) < 200
    L = make_lights(sc.rt, "5x5")
    RL = shadow_ref.Lights(L)
    for params in PARAMS:
        sp = make_params(sc.rt, sc.lib, params)
        want = shadow_ref.oracle_counts(sc.osc, RL, P, N, bool(sp.per_point), sp.seed, (F(sp.fu), F(sp.fv)))
        vis, share = run(sc, L, sp, P, N)
        assert np.array_equal(vis, want), (name, params, np.flatnonzero(vis != want)[:8])
        assert same(share, shadow_ref.share_of(want, 25))
    if name != "cube":
        assert ((want > 0) & (want < 25)).any()


# ------------------------------------------------------------------------------------------ 3. batch lengths around the unit boundaries
@pytest.mark.parametrize("lights,lengths", [("5x5", (0, 1, 63, 64, 65)), ("2x2", (15, 16, 17))])
def test_batch_lengths(world, lights, lengths):
    sc = world["cube"]
    P, N = sc.P[sc.hit][:65], sc.N[sc.hit][:65]                  # (every one of them lies in the penumbra of this light)
    L = make_lights(sc.rt, lights)
    K = L.n_lights * L.usteps * L.vsteps
    assert 64 // math.gcd(K, 64) in (64, 16)
    for params in ("centre", "seed7"):
        sp = make_params(sc.rt, sc.lib, params)
        want = sc.counts_by_strikes(L, sp, P, N)                 # (point i of a call takes the jitter of its index i: a prefix of the batch is the batch of the prefix)
        assert len(set(want[:15].tolist())) > 1 and ((want > 0) & (want < K)).sum() > 32
        for n in lengths:
            vis, share = run(sc, L, sp, P[:n], N[:n])
            assert np.array_equal(vis, want[:n]), (lights, params, n)
            assert same(share, shadow_ref.share_of(want[:n], K)), (lights, params, n)


# ------------------------------------------------------------------------------------------ 4. more units than the grid holds
@pytest.mark.parametrize("lights", ["point", "16x16"])
def test_grid_stride(world, lights):
    """the grid is at most 8 blocks of 4 waves per CU times the rounds of a unit up to 4 (rt_shadow_layout.hpp: ao_grid's rule): these batches
    hold a quarter more units than that, in the one-round kernel and in the kernel of several rounds, so waves stride.  Against
    rt_light_strikes_device on the explicit segments."""
    import torch
    sc = world["mixed"]
    cus = gc.cu_count(sc.ctx.device)
    L = make_lights(sc.rt, lights)
    K = L.n_lights * L.usteps * L.vsteps
    group, rounds = 64 // math.gcd(K, 64), K // math.gcd(K, 64)
    n = 64 * gc.round_two(gc.ao_cap(cus, 1)) + 3 if lights == "point" else gc.round_two(gc.ao_cap(cus, 4)) + 1
    assert (group, rounds) == ((64, 1) if lights == "point" else (1, 4))
    units = -(-n // group)
    assert gc.strides(units, gc.ao_cap(cus, rounds)) and gc.ao_grid(units, cus, rounds) * gc.WAVES < units, (cus, units)
    dev = f"cuda:{sc.ctx.device}"
    hits = np.flatnonzero(sc.hit)
    P = torch.from_numpy(sc.P[hits[np.arange(n) % len(hits)]]).to(dev)
    sp = make_params(sc.rt, sc.lib, "pass5")
    S = torch.from_numpy(np.array(sc.samples(L, sp, 1)[0], F)).to(dev)                   # (K, 3)
    vis, share = sc.ctx.soft_shadows(P, None, L, sp)
    chunk = max(1, (1 << 22) // K)                                                                 # points per explicit call
    want = torch.empty(n, dtype=torch.int32, device=dev)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        hit = P[a:b, None, :].expand(b - a, K, 3).reshape(-1, 3).contiguous()
        light = S[None].expand(b - a, K, 3).reshape(-1, 3).contiguous()
        want[a:b] = sc.ctx.light_strikes_device(hit, light).reshape(b - a, K).sum(dim=1, dtype=torch.int32)
    sc.ctx.synchronize()
    torch.cuda.synchronize()
    got, want = vis.cpu().numpy(), want.cpu().numpy().astype(np.uint16)
    assert got.dtype == np.uint16 and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert same(share.cpu().numpy(), shadow_ref.share_of(want, K))
    assert 0 < int((want < K).sum()) < n and np.array_equal(want[:len(hits)], want[len(hits):2 * len(hits)])


# ------------------------------------------------------------------------------------------ 5. guards
def test_canaries_and_null_outputs(world):
    sc = world["mixed"]
    L, sp = make_lights(sc.rt, "3 lights"), make_params(sc.rt, sc.lib, "seed7")
    want = sc.counts("3 lights", "seed7")
    for n in (sc.n, 100, 1):                                     # (run() reads the GUARD elements behind n of both outputs)
        for want_v, want_s in ((True, True), (True, False), (False, True)):
            v, s = run(sc, L, sp, sc.P[:n], sc.N[:n], want_visible=want_v, want_share=want_s)
            assert (v is None) == (not want_v) and (s is None) == (not want_s)
            if want_v:
                assert np.array_equal(v, want[:n])
            if want_s:
                assert same(s, shadow_ref.share_of(want[:n], 75))


def test_no_point_rule_with_and_without_normals(world):
    sc = world["mixed"]
    L, sp = make_lights(sc.rt, "5x5"), make_params(sc.rt, sc.lib, "centre")
    # a normal array: three +-0 are "no point", whatever the position; any other normal is a point, whatever it is
    N = np.array(sc.N)
    hits = np.flatnonzero(sc.hit)
    N[hits[0::3]] = 0.0
    N[hits[3::6], 1] = -0.0                                       # (either sign of zero)
    N[hits[1::3]] = (1e-30, 0.0, 0.0)
    want = np.array(sc.counts("5x5", "centre"))
    assert (want[hits[0::3]] < 25).any()
    want[hits[0::3]] = 25
    v, s = run(sc, L, sp, sc.P, N)
    assert np.array_equal(v, want) and same(s, shadow_ref.share_of(want, 25))
    # all of them: no wave has an active lane
    v, s = run(sc, L, sp, sc.P, np.zeros_like(sc.N))
    assert (v == 25).all() and same(s, np.full(sc.n, 1.0, F))
    # no normal array: every point is a point, the zeros of the misses included
    want = sc.counts_by_strikes(L, sp, sc.P, None)
    v, s = run(sc, L, sp, sc.P, None)
    assert np.array_equal(v, want) and same(s, shadow_ref.share_of(want, 25))
    assert np.array_equal(want[sc.hit], sc.counts("5x5", "centre")[sc.hit]) and len(set(want[~sc.hit].tolist())) == 1


def test_no_scene_and_bad_arguments(rt, world):
    sc = world["mixed"]
    lib, inv = sc.lib, rt.capi.RT_ERR_INVALID
    p, nr = In(rt, sc.P), In(rt, sc.N)
    v, s = Out(rt, sc.n, 1, np.uint16), Out(rt, sc.n, 1, np.float32)
    fp = lambda x: x.ctypes.data_as(C.c_void_p)
    hv, hs = np.zeros(sc.n, np.uint16), np.zeros(sc.n, F)
    P, N = np.ascontiguousarray(sc.P), np.ascontiguousarray(sc.N)
    L, sp = make_lights(rt, "5x5"), rt.shadow_params()

    def calls(h, n, L=L, sp=sp):
        pl, ps = (C.byref(L) if L is not None else None), (C.byref(sp) if sp is not None else None)
        return [lib.rt_soft_shadows_device(h, pl, n, p.buf.ptr, nr.buf.ptr, ps, v.buf.ptr, s.buf.ptr, None),
                lib.rt_soft_shadows(h, pl, n, fp(P), fp(N), ps, fp(hv), fp(hs))]

    empty = rt.Context(0)
    try:
        for n in (sc.n, 0):
            assert calls(empty.handle, n) == [rt.capi.RT_ERR_NO_SCENE] * 2
    finally:
        empty.close()
    h = sc.ctx.handle
    assert calls(h, 0) == [0, 0]
    assert calls(h, -1) == [inv, inv]
    assert calls(h, sc.n, L=None) == [inv, inv] and calls(h, sc.n, sp=None) == [inv, inv] and calls(h, 0, sp=None) == [inv, inv]
    for fu in (1.0, -0.1, float("nan")):
        assert calls(h, sc.n, sp=rt.shadow_params(fu=fu)) == [inv, inv], fu
        assert calls(h, sc.n, sp=rt.shadow_params(fv=fu)) == [inv, inv], fu
        assert calls(h, 0, sp=rt.shadow_params(fu=fu)) == [inv, inv], fu
    # lights that a frame would refuse; sphere lights
    for bad in (rt.make_lights(points=THREE[:1], usteps=0), rt.make_lights(points=THREE[:1], usteps=33, vsteps=32), rt.make_lights(points=())):
        assert calls(h, sc.n, L=bad) == [inv, inv]
    sphere = rt.make_lights(points=THREE[:1])
    keep = rt.set_sphere(sphere, rt.sphere_offsets(3, 1.0, 25))                      # noqa: F841 -- keeps the offsets alive
    assert calls(h, sc.n, L=sphere) == [rt.capi.RT_ERR_UNSUPPORTED] * 2
    # NULL pointers, aliasing: an output that shares a byte with an input
    dev = lib.rt_soft_shadows_device
    assert dev(h, C.byref(L), sc.n, None, nr.buf.ptr, C.byref(sp), v.buf.ptr, s.buf.ptr, None) == inv
    assert dev(h, C.byref(L), sc.n, p.buf.ptr, nr.buf.ptr, C.byref(sp), None, None, None) == inv
    assert lib.rt_soft_shadows(h, C.byref(L), sc.n, fp(P), fp(N), C.byref(sp), None, None) == inv
    assert dev(h, C.byref(L), sc.n, p.buf.ptr, nr.buf.ptr, C.byref(sp), v.buf.ptr, nr.buf.ptr, None) == inv
    assert dev(h, C.byref(L), sc.n, p.buf.ptr, nr.buf.ptr, C.byref(sp), C.c_void_p(p.buf.address + sc.n * 12 - 2), s.buf.ptr, None) == inv
    assert dev(h, C.byref(L), sc.n, p.buf.ptr, None, C.byref(sp), p.buf.ptr, s.buf.ptr, None) == inv
    sc.ctx.synchronize()
    assert v.untouched() and s.untouched()
    p.check(); nr.check()
    assert not hv.any() and not hs.any()
    # ... and the host-pointer form answers as the device form does
    rt.capi.check(lib, h, lib.rt_soft_shadows(h, C.byref(L), sc.n, fp(P), fp(N), C.byref(sp), fp(hv), fp(hs)), "rt_soft_shadows")
    assert np.array_equal(hv, sc.counts("5x5", "centre")) and same(hs, shadow_ref.share_of(hv, 25))
    rt.capi.check(lib, h, lib.rt_soft_shadows(h, C.byref(L), sc.n, fp(P), None, C.byref(sp), fp(hv), None), "rt_soft_shadows")
    assert np.array_equal(hv[sc.hit], sc.counts("5x5", "centre")[sc.hit])


# ------------------------------------------------------------------------------------------ 6. streams
def test_side_stream_beside_overlapped_frames(rt, world):
    """the call on a torch side stream while overlapped frames of the same context are in flight: the frames are their earlier selves bit
    for bit, the counts are the reference's, and the refined count of an adaptive frame survives the call"""
    import torch
    sc = world["mixed"]
    ctx, lib = sc.ctx, sc.lib
    w, h = 96, 64
    p = rt.make_params(w, h, 4)
    Lf = rt.make_lights(points=THREE[:1], area=True, usteps=8, vsteps=8)
    cams = [rt.default_camera(w, h, 0.07 * k) for k in range(4)]

    def frames():
        outs = [torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda") for _ in cams]
        torch.cuda.synchronize()
        for cam, out in zip(cams, outs):
            rt.capi.check(lib, ctx.handle, lib.rt_render_device(ctx.handle, C.byref(cam), C.byref(Lf), C.byref(p), C.c_void_p(out.data_ptr()), None, None, None, None),
                          "rt_render_device")
        return outs

    ctx.set_frame_overlap(0)
    before = frames()
    ctx.synchronize()
    before = [b.cpu().numpy() for b in before]
    assert len({b.tobytes() for b in before}) == len(cams)
    L, sp = make_lights(rt, "3 lights"), make_params(rt, lib, "seed7")
    dev = f"cuda:{ctx.device}"
    tp, tn = torch.from_numpy(np.ascontiguousarray(sc.P)).to(dev), torch.from_numpy(np.ascontiguousarray(sc.N)).to(dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    try:
        ctx.set_frame_overlap(2)
        took = ctx.overlapped_frames()
        outs = frames()
        with torch.cuda.stream(side):
            vis, share = ctx.soft_shadows(tp, tn, L, sp)
        side.synchronize()
        ctx.synchronize()
        assert ctx.overlapped_frames() == took + len(cams)
    finally:
        ctx.set_frame_overlap(1)
    want = sc.counts("3 lights", "seed7")
    assert vis.dtype == torch.uint16 and share.dtype == torch.float32 and tuple(share.shape) == (sc.n,) and str(share.device) == dev
    assert np.array_equal(vis.cpu().numpy(), want) and same(share.cpu().numpy(), shadow_ref.share_of(want, 75))
    for k, (out, b) in enumerate(zip(outs, before)):
        assert same(out.cpu().numpy(), b), k
    # the refined count
    fs = sc.fs
    fs.areaLight, fs.pointLight, fs.usteps, fs.vsteps, fs.max_depth = True, False, 5, 5, 4
    fs.supersample, fs.supersample_threshold = 2, 0.05
    try:
        fs.raytraceScene(64, 40, write_ppm=False)
        refined = ctx.supersampling_refined()
        fs.raytraceScene(64, 40, write_ppm=False)
        v, _ = run(sc, L, sp, sc.P, sc.N)
        assert ctx.supersampling_refined() == refined and 0 < refined < 64 * 40
        assert np.array_equal(v, want)
    finally:
        fs.supersample, fs.supersample_threshold = 1, -1.0
        ctx.set_supersampling(1)
        ctx.set_supersampling_threshold(-1.0)


# ------------------------------------------------------------------------------------------ 7. RT_NO_CULL and the counting build
WORK_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")


@pytest.mark.parametrize("variant", ["no_cull", "counting"])
def test_switch_and_counting_build_give_the_same_counts(rt, world, monkeypatch, variant):
    if variant == "no_cull":
        monkeypatch.setenv("RT_NO_CULL", "1")
    lib = rt.capi.load_library(WORK_LIB) if variant == "counting" else rt.load_library()
    fp = lambda a: a.ctypes.data_as(C.c_void_p)
    L, sp = make_lights(rt, "3 lights"), make_params(rt, rt.load_library(), "seed7")
    for name in ("mixed", "dodge"):
        sc = world[name]
        ctx = C.c_void_p()
        assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK                 # (a fresh context: it reads RT_* when it is made and at upload)
        try:
            rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(sc.fs.scene.view)), "rt_upload_scene")
            v, s = np.full(sc.n, 0xA5A5, np.uint16), np.full(sc.n, 7, F)
            P, N = np.ascontiguousarray(sc.P), np.ascontiguousarray(sc.N)
            rt.capi.check(lib, ctx, lib.rt_soft_shadows(ctx, C.byref(L), sc.n, fp(P), fp(N), C.byref(sp), fp(v), fp(s)), "rt_soft_shadows")
        finally:
            lib.rt_destroy(ctx)
        want = sc.counts("3 lights", "seed7")
        assert np.array_equal(v, want) and same(s, shadow_ref.share_of(want, 75)), (variant, name)


# ------------------------------------------------------------------------------------------ 8. the Flyscene member
def test_flyscene_member_equals_the_composed_calls(rt, world):
    sc = world["mixed"]
    fs, ctx, lib = sc.fs, sc.ctx, sc.lib
    w, h = 37, 21
    keep, keep_lights = fs.camera, fs.lights
    fs.areaLight, fs.pointLight, fs.usteps, fs.vsteps = True, False, 5, 5
    fs.lights = [THREE[0]]
    sp = rt.shadow_params(per_point=True, seed=7)
    dn, up = rt.denoise_params(2, 0.5, 0.5, 0.125, 0.25), rt.upsample_params(factor=2)
    hipmem = rt.hipmem

    def composed(cam, cw, ch, L):
        """closest hits -> hit points -> soft shadows on the pinhole rays of cam, on the device -> the share buffer (cw * ch floats)"""
        n = cw * ch
        pts = np.empty((n, 3), F)
        rt.capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(cam), cw, ch, pts.ctypes.data_as(C.c_void_p)), "rt_primary_points")
        centre = np.asarray(list(cam.center), F)
        io, id_ = In(rt, np.broadcast_to(centre, (n, 3))), In(rt, pts - centre)
        faces, ts = ctx.closest_hits(io.buf, id_.buf, n=n)
        points, normals = ctx.hit_points(io.buf, id_.buf, faces, ts, n=n)
        _, share = ctx.soft_shadows(points, normals, L, sp, n=n, want_visible=False)
        ctx.synchronize()
        return share, faces.to_numpy(np.int32, (n,))

    try:
        fs.camera = rt.default_camera(fs.width, fs.height, 0.4)
        cam = rt.default_camera(w, h)
        cam.center, cam.inv_view = fs.camera.center, fs.camera.inv_view
        L = fs._lights()
        share, faces = composed(cam, w, h, L)
        plain = share.to_numpy(F, (h, w))
        got = fs.soft_shadows(w, h, sp)
        assert got.shape == (h, w) and got.dtype == np.float32 and same(got, plain)
        miss = (faces < 0).reshape(h, w)
        assert 0 < int(miss.sum()) < w * h and same(got[miss], np.full(int(miss.sum()), 1.0, F))
        assert ((got > 0) & (got < 1)).any()
        # explicit lights: another question
        L3 = make_lights(rt, "3 lights")
        assert same(fs.soft_shadows(w, h, sp, lights=L3), composed(cam, w, h, L3)[0].to_numpy(F, (h, w)))
        # denoise: the one-ray pinhole geometry buffers of the same camera
        for c in (lambda: ctx.set_supersampling(1), lambda: ctx.set_lens(0.0, fs.focus), lambda: ctx.set_shutter(None), lambda: ctx.set_passes(0, 1)):
            c()
        g = hipmem.DeviceBuffer(w * h * rt.capi.RT_GBUFFER_CHANNELS * 4)
        out = hipmem.DeviceBuffer(w * h * 4)
        ctx.synchronize(); hipmem.synchronize()
        ctx.gbuffer(cam, w, h, out=g)
        ctx.denoise(share, g, w, h, dn, out=out, channels=1)
        ctx.synchronize()
        want = out.to_numpy(F, (h, w))
        assert not same(want, plain)
        assert same(fs.soft_shadows(w, h, sp, denoise=dn), want)
        # upsample by 2: the call at 19 x 11 through the low camera, filtered there, then the guided upsample
        lcam, lw, lh = rt.low_camera(cam, 2)
        assert (lw, lh) == (19, 11)
        low, _ = composed(lcam, lw, lh, L)
        g_low, filt, big = hipmem.DeviceBuffer(lw * lh * rt.capi.RT_GBUFFER_CHANNELS * 4), hipmem.DeviceBuffer(lw * lh * 4), hipmem.DeviceBuffer(w * h * 4)
        ctx.synchronize(); hipmem.synchronize()
        ctx.gbuffer(lcam, lw, lh, out=g_low)
        ctx.upsample(low, g_low, g, w, h, up, out=big, channels=1)
        ctx.synchronize()
        assert same(fs.soft_shadows(w, h, sp, upsample=up), big.to_numpy(F, (h, w)))
        ctx.denoise(low, g_low, lw, lh, dn, out=filt, channels=1)
        ctx.upsample(filt, g_low, g, w, h, up, out=big, channels=1)
        ctx.synchronize()
        assert same(fs.soft_shadows(w, h, sp, denoise=dn, upsample=up), big.to_numpy(F, (h, w)))
    finally:
        fs.camera, fs.lights = keep, keep_lights
