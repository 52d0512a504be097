"""Adaptive pass counts (rt_set_pass_tolerance) restated in numpy float32: the rule of include/rt_mi355x.h with an explicit cast after every
operation, so that nothing is evaluated in a wider type or fused.  The GPU tests fold individually rendered single-pass frames with it."""
import numpy as np

F = np.float32


def fold_adaptive(frames, tol, min_passes):
    """frames: the float32 [..., 3] frames F_first .. F_(first + count - 1), in order.  Returns (result [..., 3] float32, taken [...] uint16)."""
    frames = [np.asarray(f, F) for f in frames]
    count = len(frames)
    shape = frames[0].shape[:-1]
    s1, s2 = np.zeros(shape + (3,), F), np.zeros(shape + (3,), F)
    taken = np.zeros(shape, np.uint16)
    active = np.ones(shape, bool)
    tol = F(tol)
    with np.errstate(over="ignore", invalid="ignore"):
        tt = F(tol * tol)
        for k in range(1, count + 1):
            f = frames[k - 1]
            a = active[..., None]
            q = (f * f).astype(F)
            s1 = np.where(a, (s1 + f).astype(F), s1)
            s2 = np.where(a, (s2 + q).astype(F), s2)
            taken = np.where(active, np.uint16(k), taken).astype(np.uint16)
            if min_passes <= k < count:
                kf = F(k)
                d = ((kf * s2).astype(F) - (s1 * s1).astype(F)).astype(F)
                T = F(F(tt * F(kf * kf)) * F(kf - F(1.0)))
                conv = (d <= T).all(axis=-1)              # (a NaN compares false: it never converges)
                active = active & ~conv
        result = (s1 / taken.astype(F)[..., None]).astype(F)
    return result, taken


def classes(taken, min_passes, count):
    """(pixels stopped at min_passes, stopped in between, that ran every pass)"""
    t = np.asarray(taken)
    return int((t == min_passes).sum()), int(((t > min_passes) & (t < count)).sum()), int((t == count).sum())
