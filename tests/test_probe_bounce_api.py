"""Bounced light, the parts that need no GPU: the four entry points are declared, bound and exported and refuse a NULL context; the numpy
restatement of tests/probe_bounce_ref.py equals the shared host code (the streamed blend of rt_probe_layout.hpp, run by
tools/probe_bounce_check.cpp under the sanitizers) bit for bit; a source of zeros gives the parents' definitions in every bit; the clamp;
and on the sealed two-room scene, over the CPU checker's closest hits and lightStrikes, the dark room stays exactly black under the visible
feedback and does not under the plain one."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import indirect_ref as ir
import probe_bounce_ref as pb
import probe_ref as pr
import probe_visible_ref as pv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer-in-cpp_amd", "csrc")
NAMES = ["rt_light_probes_bounce_device", "rt_light_probes_bounce", "rt_indirect_diffuse_bounce_device", "rt_indirect_diffuse_bounce"]
F = np.float32
WHITE = (1.0, 1.0, 1.0)


def bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


def same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.array_equal(bits(a), bits(b))


def test_header_declares_the_calls_and_the_definition():
    text = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    assert "bounced light" in text and "tests/probe_bounce_ref.py" in text
    for phrase in ("b_c = smax(0.0f, I_c)", "R_c = R_c + kd_c * b_c", "COMPUTED WITHOUT `direct`", "no segment is formed"):
        assert phrase in text, phrase
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\brt_status\s+" + name + r"\s*\(", code), name


def test_binding_and_library_hold_the_calls(rt):
    lib = rt.load_library()
    sigs = {s[0]: s for s in rt.capi._SIGNATURES}
    for name, nargs in zip(NAMES, (11, 10, 12, 11)):
        assert name in rt.capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(sigs[name][2]) == nargs
    for fn in (rt.Context.light_probes, rt.Context.indirect_diffuse):
        p = inspect.signature(fn).parameters
        assert p["source"].default is None and p["visible"].default is False
    p = inspect.signature(rt.Flyscene.light_probes).parameters
    assert p["bounces"].default == 0 and p["visible"].default is True
    p = inspect.signature(rt.Flyscene.indirect_diffuse).parameters
    assert p["probes"].default is None and p["visible"].default is True
    kernels = open(os.path.join(CSRC, "rt_kernels.hip")).read()
    assert "k_gather_bounce" in kernels and "k_probes_bounce" in kernels


def test_null_context_is_invalid(rt):
    lib = rt.load_library()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    g = rt.probe_grid((0, 0, 0), (1, 1, 1), (1, 1, 1))
    L = rt.make_lights()
    inv = rt.capi.RT_ERR_INVALID
    for n, q in ((1, p), (0, None)):
        assert lib.rt_light_probes_bounce_device(None, C.byref(L), n, q, 4, 0, C.byref(g), q, 0, q, None) == inv
        assert lib.rt_light_probes_bounce(None, C.byref(L), n, q, 4, 0, C.byref(g), q, 1, q) == inv
        assert lib.rt_indirect_diffuse_bounce_device(None, C.byref(L), n, q, q, 4, 0, C.byref(g), q, 0, q, None) == inv
        assert lib.rt_indirect_diffuse_bounce(None, C.byref(L), n, q, q, 4, 0, C.byref(g), q, 1, q) == inv
    assert not any(buf)


# ------------------------------------------------------------------------------------------ the restatement against the shared host code
def read_fixture(path):
    raw = open(path, "rb").read()
    out, at = [], 0
    while at < len(raw):
        head = np.frombuffer(raw, np.int32, 16, at)
        assert head[0] == 0x42504c42
        dims, points = tuple(int(x) for x in head[1:4]), int(head[4])
        origin, step = head[5:8].view(F), head[8:11].view(F)
        at += 64
        cells = dims[0] * dims[1] * dims[2]
        coeff = np.frombuffer(raw, F, cells * 27, at).reshape(cells, 27)
        at += cells * 108
        rec = np.frombuffer(raw, np.uint32, points * 17, at).reshape(points, 17)
        at += points * 68
        out.append((pr.Grid(origin, step, dims), coeff, rec))
    return out


def test_the_restatement_equals_the_shared_host_code(tmp_path):
    """tools/probe_bounce_check.cpp compares the streamed blend the kernels run with probe_lookup / probe_lookup_visible (all 256
    visibility bytes, every subset of single-layer axes, NaN / inf / negative coefficients) under ASan and UBSan, as the Makefile builds it,
    and writes records of probe_bounce_lookup + probe_bounce_add; the numpy restatement gives the same R in every bit"""
    fixture = tmp_path / "bounce.bin"
    r = subprocess.run(["make", "-C", CSRC, "probe_bounce_check", f"OUT={tmp_path}", f"FIXTURE={fixture}"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
    assert b"all checks held" in r.stdout
    assert b"-ffp-contract=off" in r.stdout and b"-fsanitize=address,undefined" in r.stdout
    cases = read_fixture(fixture)
    assert [g.dims.count(1) for g, _, _ in cases] == [0, 1, 2]
    for grid, coeff, rec in cases:
        fl = rec.view(F)
        P, N, vis_bits, mode = fl[:, 0:3], fl[:, 3:6], rec[:, 6], rec[:, 7]
        kd, R, want = fl[:, 8:11], fl[:, 11:14], fl[:, 14:17]
        vis = ((vis_bits[:, None] >> np.arange(8)[None, :]) & 1).astype(bool)
        I = np.where((mode != 0)[:, None], pv.lookup_visible(grid, coeff, P, N, vis)[0], pr.lookup(grid, coeff, P, N))
        with np.errstate(invalid="ignore", over="ignore"):
            got = (R + kd * pb.clamp(I)).astype(F)
        assert same(got, want), (grid.dims, np.flatnonzero((bits(got) != bits(want)).reshape(-1, 3).any(axis=1))[:8])
        assert np.isfinite(want).all() or grid.dims.count(1) == 2, "only the volume with the special values can give inf"
        assert (got != R).any() and (got == R).any(), "the fixture holds lookups above zero and clamped ones"


# ------------------------------------------------------------------------------------------ the two-room scene over the CPU checker
class Rooms:
    def __init__(self, oracle, tmp_path):
        self.osc = oracle.load_scene(pv.two_rooms(str(tmp_path)))
        self.data, self.tracer = ir.SceneData(self.osc), ir.OracleTracer(self.osc)
        self.W = ir.to_world(self.osc, pv.ROOM_VERTS)
        self.grid = pv.room_grid(self.W)
        self.light = [tuple(float(v) for v in self.W(pv.ROOM_LIGHT))]
        self.pos = self.grid.positions()
        self.wall = float(self.W([0, 0, 0])[0])
        self.room_b = self.pos[:, 0] > self.wall

    def points(self):
        """room_b_points and their mirror images in room A"""
        P, N = pv.room_b_points(self.W)
        PA = P.copy()
        PA[:, 0] = 2 * F(self.wall) - P[:, 0]
        NA = N.copy()
        return np.concatenate([P, PA]), np.concatenate([N, NA])


def test_a_source_of_zeros_gives_the_parents_in_every_bit(oracle, tmp_path):
    """R + kd * smax(0, 0) adds +0 to a sum that is never -0"""
    rm = Rooms(oracle, tmp_path)
    try:
        zero = np.zeros((rm.grid.cells, 27), F)
        for direct in (False, True):
            want = pr.probes(rm.tracer, rm.data, rm.pos, 3, rm.light, WHITE, direct)
            for visible in (False, True):
                got = pb.probes(rm.tracer, rm.data, rm.pos, 3, rm.light, WHITE, direct, rm.grid, zero, visible)
                assert same(got, want), (direct, visible)
        assert (want != 0).any()
        P, N = rm.points()
        N[3] = 0.0                                                 # no point
        want = ir.gather(rm.tracer, rm.data, P, N, 3, 5, rm.light, WHITE)
        for visible in (False, True):
            assert same(pb.gather(rm.tracer, rm.data, P, N, 3, 5, rm.light, WHITE, rm.grid, zero, visible), want), visible
        assert (want != 0).any() and not bits(want[3]).any()
    finally:
        rm.osc.close()


def test_the_clamp(oracle, tmp_path):
    """one strongly negative-lobed probe and one NaN coefficient in the source: the term is +0 where I_c <= 0 or NaN, and the result is
    not the unclamped sum"""
    rm = Rooms(oracle, tmp_path)
    try:
        rng = np.random.default_rng(3)
        src = (0.2 * rng.random((rm.grid.cells, 27))).astype(F)
        src[:, 3:] *= F(0.1)
        src[5, 0:3] = F(-40.0)                                     # a negative DC: every direction of that probe is negative
        src[10, 4] = np.nan
        tr = pb.trace_probes(rm.tracer, rm.data, rm.pos, 4, rm.light)
        I = pb.source_lookup(rm.grid, src, tr.hits)
        neg, nan, pos = (I <= 0), np.isnan(I), (I > 0)
        print("hits:", len(I), " channels <= 0 / NaN / > 0:", int(neg.sum()), int(nan.sum()), int(pos.sum()))
        assert neg.sum() >= 16 and nan.sum() >= 3 and pos.sum() >= 16
        b = pb.clamp(I)
        assert not bits(b[neg | nan]).any() and same(b[pos], I[pos])
        got = pb.shade_probes(tr, WHITE, False, I)
        raw = pb.shade_probes(tr, WHITE, False, I, clamped=False)
        assert np.isfinite(got).all() and not same(got, raw) and np.isnan(raw).any()
        # the term by hand on the radiances: only where I > 0 does a hit's radiance move
        R0, R1 = pb.radiance(tr.hits, WHITE)[tr.hits.hit], pb.radiance(tr.hits, WHITE, I)[tr.hits.hit]
        assert same(R1[~pos], R0[~pos]) and same(R1[pos], (R0 + tr.hits.kd * I)[pos].astype(F))
    finally:
        rm.osc.close()


def test_sealed_rooms(oracle, tmp_path):
    """the light is inside room A and the rooms are sealed.  Premises, on the checker alone: every room-B probe of pass 0 is exactly zero,
    and every hit of a room-B probe ray has at least one USED corner (case A's fallback to the plain blend never fires there).  Then:
    visible feedback keeps room B's 8 probes exactly zero for three passes, the plain feedback does not (the leak the flag exists for), and
    room A's DC coefficients grow from pass 0 to pass 1."""
    rm = Rooms(oracle, tmp_path)
    try:
        assert rm.room_b.sum() == 8 and (~rm.room_b).sum() == 8
        m = 4
        tr = pb.trace_probes(rm.tracer, rm.data, rm.pos, m, rm.light)
        ray_of_b = np.broadcast_to(rm.room_b[:, None], tr.hits.hit.shape)[tr.hits.hit]          # per hit: its ray belongs to a room-B probe
        assert tr.hits.hit.all(), "the box is closed: every probe ray hits"
        vis = pb.source_visibility(rm.tracer, rm.grid, tr.hits)
        read, w, _, _ = pv.corners(rm.grid, tr.hits.H)
        used = vis & read[None, :] & (w > 0)
        assert used[ray_of_b].any(axis=1).all(), "every hit of a room-B probe ray has a USED corner"
        assert (tr.hits.H[ray_of_b][:, 0] > rm.wall).all(), "room B's rays end in room B"
        seen = pb.feedback(rm.tracer, rm.data, rm.grid, m, rm.light, WHITE, False, 3, True)
        leaky = pb.feedback(rm.tracer, rm.data, rm.grid, m, rm.light, WHITE, False, 3, False)
        assert same(seen[0], leaky[0]) and same(seen[0], pr.probes(rm.tracer, rm.data, rm.pos, m, rm.light, WHITE))
        assert not bits(seen[0][rm.room_b]).any(), "pass 0: room B is exactly black"
        for b in (1, 2, 3):
            assert not bits(seen[b][rm.room_b]).any(), f"visible pass {b}: room B stays exactly +0.0f"
        assert (leaky[1][rm.room_b] != 0).any() and (leaky[3][rm.room_b] != 0).any(), "the plain lookup leaks room A's light into room B"
        dc0, dc1 = seen[0][~rm.room_b][:, 0:3], seen[1][~rm.room_b][:, 0:3]
        assert (dc1 > dc0).all(), "one more bounce: room A's DC grows"
        print("room A mean DC per pass:", [float(v[~rm.room_b][:, 0:3].mean()) for v in seen])
        print("largest room-B coefficient of the plain feedback per pass:", [float(np.abs(v[rm.room_b]).max()) for v in leaky])
    finally:
        rm.osc.close()


def test_convergence_is_recorded(oracle, tmp_path):
    """a measurement, not a claim: the largest coefficient change per pass on the two rooms and on the mixed-materials scene (DESIGN.md 6,
    Bounced light)"""
    import scenes_gen
    rm = Rooms(oracle, tmp_path)
    try:
        vol = pb.feedback(rm.tracer, rm.data, rm.grid, 4, rm.light, WHITE, False, 6, True)
        steps = [float(np.abs(vol[b] - vol[b - 1]).max()) for b in range(1, len(vol))]
        print("two_rooms, 4 x 2 x 2 probes, m = 4: largest coefficient change per pass:", steps, " largest coefficient:", float(np.abs(vol[-1]).max()))
        assert all(np.isfinite(steps))
    finally:
        rm.osc.close()
    osc = oracle.load_scene(scenes_gen.mixed_materials(str(tmp_path / "mixed")))
    try:
        w = np.asarray(osc.arrays()["wverts"], F)
        grid = pr.Grid.over(np.concatenate([w.min(axis=0), w.max(axis=0)]), (4, 3, 3), 0.0)
        vol = pb.feedback(ir.OracleTracer(osc), ir.SceneData(osc), grid, 4, [(-1.0, 1.0, 1.0)], WHITE, False, 6, True)
        steps = [float(np.abs(vol[b] - vol[b - 1]).max()) for b in range(1, len(vol))]
        print("mixed_materials, 4 x 3 x 3 probes, m = 4: largest coefficient change per pass:", steps, " largest coefficient:", float(np.abs(vol[-1]).max()))
        assert all(np.isfinite(steps))
    finally:
        osc.close()
