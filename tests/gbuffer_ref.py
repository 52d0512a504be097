"""The geometry buffers defined in include/rt_mi355x.h (RT_GBUFFER_CHANNELS) restated in numpy: the value of a sub-sample, the n x n fold, the fold of the
passes -- float32 with an explicit cast after every operation -- and a CPU frame put together from the oracle's pieces.

Test infrastructure only.  The CPU frame is NOT the oracle's renderer (orc_render knows colours only): like tests/light_jitter_ref.py it forms
every sub-sample's primary ray with screen_to_world at the raster point ((float)i + ox[sx], (float)j + oy[sy]) of passes_ref.pass_offsets and asks
closest_hit for the face and the ray parameter."""
import numpy as np

import passes_ref

F = np.float32
CHANNELS = 8                    # alpha, depth, normal xyz, kd rgb


def sample_values(face, t, face_normal, kd):
    """v[..., 8] of the sub-samples with closest face `face` (-1: none) and ray parameter `t`: (1, t, face_normal[face], kd[face]) where
    face >= 0, eight +0.0f elsewhere.  face_normal [n_faces, 3], kd [n_faces, 3] (the kd of every face's material)."""
    face = np.asarray(face, np.int32)
    t = np.asarray(t, F)
    v = np.zeros(face.shape + (CHANNELS,), F)
    hit = face >= 0
    f = face[hit]
    v[hit, 0] = F(1.0)
    v[hit, 1] = t[hit]
    v[hit, 2:5] = np.asarray(face_normal, F)[f]
    v[hit, 5:8] = np.asarray(kd, F)[f]
    return v


def fold_subsamples(v, n):
    """v[H, W, n, n, 8] (sy, sx) -> G_p[H, W, 8].  n = 1: v itself, bit for bit; n > 1: a = 0.0f; a = a + v, sy outer and sx inner;
    a / (float)(n*n), every operation rounded to float32 on its own"""
    v = np.asarray(v, F)
    assert v.shape[2:] == (n, n, CHANNELS)
    if n == 1:
        return v[:, :, 0, 0].copy()
    acc = np.zeros(v.shape[:2] + (CHANNELS,), F)
    for sy in range(n):
        for sx in range(n):
            acc = (acc + v[:, :, sy, sx]).astype(F)
    return (acc / F(n * n)).astype(F)


def fold_passes(gs):
    """count == 1: G_first bit for bit; else A = 0.0f; A = A + G_p in order; A / (float)count (the fold of rt_set_passes)"""
    if len(gs) == 1:
        return np.asarray(gs[0], F).copy()
    return passes_ref.fold_passes(gs)


def face_kd(osc):
    """kd of every face's material, [n_faces, 3], from an oracle scene"""
    mats = np.array([m[0][0:3] for m in osc.materials()], F).reshape(-1, 3)
    return mats[osc.arrays()["face_mat"]]


def cpu_samples(orc, osc, cam, w, h, n=1, p=0, rows=None):
    """(face, t) [len(rows), w, n, n] (sy, sx) of the pinhole camera `cam` (an oracle ocamera) on the CPU: the closest hit of every sub-sample
    ray of pass p of an n x n frame, frame rows `rows` (default all)"""
    ox, oy = passes_ref.pass_offsets(n, p)
    rows = range(h) if rows is None else rows
    org = np.array(list(cam.center), F)
    face = np.full((len(rows), w, n, n), -1, np.int32)
    t = np.zeros((len(rows), w, n, n), F)
    for r, j in enumerate(rows):
        for i in range(w):
            for sy in range(n):
                for sx in range(n):
                    d = (orc.screen_to_world(cam, F(F(i) + F(ox[sx])), F(F(j) + F(oy[sy]))) - org).astype(F)
                    face[r, i, sy, sx], t[r, i, sy, sx] = osc.closest_hit(org, d)
    return face, t


def cpu_pass(orc, osc, cam, w, h, n=1, p=0, rows=None):
    """G_p[len(rows), w, 8]: cpu_samples folded as the definition says"""
    face, t = cpu_samples(orc, osc, cam, w, h, n, p, rows)
    return fold_subsamples(sample_values(face, t, osc.arrays()["face_normal"], face_kd(osc)), n)


def cpu_frame(orc, osc, cam, w, h, n=1, first=0, count=1):
    """the frame of passes first .. first + count - 1"""
    return fold_passes([cpu_pass(orc, osc, cam, w, h, n, p) for p in range(first, first + count)])


def coverage(g):
    """(fully covered, empty, partly covered) output pixels of a one-pass buffer"""
    a = np.asarray(g, F)[..., 0]
    return int((a == F(1.0)).sum()), int((a == F(0.0)).sum()), int(((a > F(0.0)) & (a < F(1.0))).sum())
