"""The adaptive supersampling rule of include/rt_mi355x.h (rt_set_supersampling_threshold), written in float32 numpy: the expected frames
of tests/test_gpu_adaptive_aa.py are built with it."""
import numpy as np


def refine(c, tau):
    """pixel p is refined when some 4-neighbour q inside the frame has a channel with fabsf(C(p) - C(q)) > tau (float32; NaN never refines)"""
    c = np.asarray(c, np.float32)
    tau = np.float32(tau)
    h, w = c.shape[:2]
    m = np.zeros((h, w), bool)
    with np.errstate(invalid="ignore"):
        d = (np.abs(c[:, 1:] - c[:, :-1]) > tau).any(axis=-1)     # horizontal pairs (the rule is symmetric)
        m[:, 1:] |= d
        m[:, :-1] |= d
        d = (np.abs(c[1:] - c[:-1]) > tau).any(axis=-1)           # vertical pairs
        m[1:] |= d
        m[:-1] |= d
    return m


def adaptive_frame(one_ray, regular, tau):
    """refined pixels from the regular n x n frame, the others from the one-ray frame"""
    return np.where(refine(one_ray, tau)[..., None], regular, one_ray).astype(np.float32)
