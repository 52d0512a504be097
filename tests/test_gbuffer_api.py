"""Geometry buffers: the definition in include/rt_mi355x.h and its numpy restatement (tests/gbuffer_ref.py), with the CPU frame it builds from
the oracle's pieces.  No device is needed: no frame fills the buffers yet (Geometry buffers)."""
import os
import re

import numpy as np
import pytest

import gbuffer_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
F = np.float32
NEG0 = np.array(-0.0, F).view(np.uint32)
POS0 = np.array(0.0, F).view(np.uint32)


def test_header_defines_the_channels_and_the_binding_repeats_them(rt):
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"^\s*#\s*define\s+RT_GBUFFER_CHANNELS\s+8\s*$", code, flags=re.M)
    assert "NO FRAME FILLS THEM" in text, "the section is a definition only (DESIGN.md 5, Geometry buffers)"
    assert rt.capi.RT_GBUFFER_CHANNELS == 8 == gr.CHANNELS


# ---------------------------------------------------------------------------------------------------- the restatement of the definition
def toy():
    """two faces (one with a -0.0f normal component), their kd, and a 1 x 2 frame of 2 x 2 sub-samples"""
    nrm = np.array([[-0.0, 1.0, 0.0], [0.6, -0.0, -0.8]], F)
    kd = np.array([[0.8, 0.1, 0.1], [0.2, 0.3, 0.9]], F)
    face = np.array([[[[0, 0], [0, -1]], [[-1, -1], [1, -1]]]], np.int32)          # pixel 0: 3 of 4 covered, pixel 1: 1 of 4
    t = np.array([[[[1.5, 1.25], [1.75, 9.0]], [[9.0, 9.0], [2.5, 9.0]]]], F)
    return nrm, kd, face, t


def test_sample_value_and_the_negative_zero_rule():
    nrm, kd, face, t = toy()
    v = gr.sample_values(face, t, nrm, kd)
    assert v.shape == (1, 2, 2, 2, 8) and v.dtype == F
    hit = v[0, 0, 0, 0]
    assert hit[0] == 1.0 and hit[1] == F(1.5) and np.array_equal(hit[5:8], kd[0])
    assert hit[2].view(np.uint32) == NEG0, "the normal is copied bit for bit"
    miss = v[0, 0, 1, 1]
    assert (miss.view(np.uint32) == POS0).all(), "a miss is eight +0.0f, whatever t says"
    # n = 1 keeps -0.0f ...
    one = gr.fold_subsamples(v[:, :, :1, :1], 1)
    assert one[0, 0, 2].view(np.uint32) == NEG0
    assert np.array_equal(one.view(np.uint32), v[:, :, 0, 0].view(np.uint32))
    # ... n > 1 starts from +0.0f: 0.0f + -0.0f = +0.0f
    same = np.repeat(np.repeat(v[:, :, :1, :1], 2, axis=2), 2, axis=3)
    two = gr.fold_subsamples(same, 2)
    assert two[0, 0, 2].view(np.uint32) == POS0
    # ... and so does a count > 1 fold of n = 1 passes, while count == 1 is the pass itself
    assert gr.fold_passes([one, one])[0, 0, 2].view(np.uint32) == POS0
    assert np.array_equal(gr.fold_passes([one]).view(np.uint32), one.view(np.uint32))


def test_fold_is_the_float32_sum_in_order_and_alpha_counts_quarters():
    nrm, kd, face, t = toy()
    g = gr.fold_subsamples(gr.sample_values(face, t, nrm, kd), 2)
    assert g[0, 0, 0] == F(0.75) and g[0, 1, 0] == F(0.25)
    want_depth = F(F(F(F(F(0.0) + F(1.5)) + F(1.25)) + F(1.75)) + F(0.0)) / F(4.0)
    assert g[0, 0, 1].view(np.uint32) == F(want_depth).view(np.uint32)
    want_kd = F(F(F(F(F(0.0) + kd[0, 0]) + kd[0, 0]) + kd[0, 0]) + F(0.0)) / F(4.0)
    assert g[0, 0, 5].view(np.uint32) == F(want_kd).view(np.uint32), "a coverage-weighted sum: divide by alpha for the mean"
    rng = np.random.default_rng(3)
    face = rng.integers(-1, 2, (9, 11, 2, 2)).astype(np.int32)
    a = gr.fold_subsamples(gr.sample_values(face, rng.random(face.shape, dtype=F), nrm, kd), 2)[..., 0]
    assert set(np.unique(a).tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    assert np.array_equal(a, (face >= 0).sum(axis=(2, 3)) / F(4.0))
    assert gr.coverage(a[..., None]) == (int((a == 1).sum()), int((a == 0).sum()), int(((a > 0) & (a < 1)).sum()))


def test_pass_fold_is_the_fold_of_rt_set_passes():
    rng = np.random.default_rng(8)
    gs = [rng.random((3, 4, 8), dtype=F) for _ in range(5)]
    acc = np.zeros((3, 4, 8), F)
    for g in gs:
        acc = (acc + g).astype(F)
    assert np.array_equal(gr.fold_passes(gs).view(np.uint32), (acc / F(5)).astype(F).view(np.uint32))


# ---------------------------------------------------------------------------------------------------- the CPU frame
# partly covered pixels of the CPU frame at yaw 0.4, (n, p) = (2, 0) and (3, 5): the counts the feature was specified with
SPECIFIED = {("cube.obj", 48, 32): (26, 35), ("dodgeColorTest.obj", 48, 32): (25, 39), ("cube.obj", 37, 21): (34, 40),
             ("dodgeColorTest.obj", 37, 21): (15, 27)}


@pytest.mark.parametrize("name,w,h", sorted(SPECIFIED))
def test_cpu_frame_shows_every_kind_of_pixel(oracle, name, w, h):
    osc = oracle.load_scene(os.path.join(SCENES, name))
    try:
        cam = oracle.camera(w, h, 0.4)
        one = gr.cpu_pass(oracle, osc, cam, w, h, 1, 0)
        parts = []
        for n, p in ((2, 0), (3, 5)):
            g = gr.cpu_pass(oracle, osc, cam, w, h, n, p)
            full, empty, part = gr.coverage(g)
            assert full > 0 and empty > 0
            assert set(np.unique(g[..., 0]).tolist()) <= {F(k) / F(n * n) for k in range(n * n + 1)}
            parts.append(part)
        neg0 = int((osc.arrays()["face_normal"].view(np.uint32) == 0x80000000).sum())
    finally:
        osc.close()
    assert tuple(parts) == SPECIFIED[(name, w, h)]
    assert gr.coverage(one)[2] == 0 and set(np.unique(one[..., 0]).tolist()) == {0.0, 1.0}
    if name == "dodgeColorTest.obj":
        assert neg0 == 616, "dodge's face normals hold negative zeros: the -0.0f rule has something to act on"
        hit = one[..., 0] == 1.0
        assert (one[hit][:, 2:5].view(np.uint32) == 0x80000000).any(), "and some of them are seen: n = 1 keeps them"


def test_cpu_frame_of_the_mixed_scene_shows_its_materials(oracle, tmp_path):
    import scenes_gen
    osc = oracle.load_scene(scenes_gen.mixed_materials(str(tmp_path)))
    try:
        face, t = gr.cpu_samples(oracle, osc, oracle.camera(48, 32, 0.4), 48, 32, 2, 0)
        kd = gr.face_kd(osc)
        g = gr.fold_subsamples(gr.sample_values(face, t, osc.arrays()["face_normal"], kd), 2)
    finally:
        osc.close()
    assert gr.coverage(g)[2] == 47 and len({tuple(x) for x in kd[face[face >= 0]].tolist()}) == 6
