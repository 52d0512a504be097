"""The multi-pass accumulation of rt_set_passes (include/rt_mi355x.h) restated in Python: the raster offsets of a pass, the pass key of the lens /
time scrambles and the fold of the passes -- host double for the offsets, uint32 for the scrambles, float32 with an explicit cast after every
operation for the fold.

Test infrastructure only.  lens_ref / shutter_ref stay the definition of pass 0; `pass_scrambles(p)` makes their hashes those of pass p for the
duration of a `with` block, so that their ray builders serve every pass."""
import contextlib

import numpy as np

import lens_ref
import shutter_ref

F = np.float32
_M = 0xFFFFFFFF
RT_MAX_PASSES = 256
RT_MAX_SUPERSAMPLING = 4
PASS_MUL = 0xC2B2AE35


def radical_inverse(p, b):
    """phi_b(p), in double, in the order the header gives"""
    f, r = 1.0, 0.0
    while p > 0:
        f = f / b
        r = r + f * (p % b)
        p = p // b
    return r


def wrapped(p, b):
    """e_b(p): phi_b(p) wrapped to [-0.5, 0.5)"""
    r = radical_inverse(p, b)
    return r if r < 0.5 else r - 1.0


def pass_offsets(n, p):
    """(ox[n], oy[n]) of pass p as float32 arrays"""
    e2, e3 = wrapped(p, 2), wrapped(p, 3)
    ox = np.array([F((2 * s + 1 - n) / (2.0 * n) + e2 / n) for s in range(n)], F)
    oy = np.array([F((2 * s + 1 - n) / (2.0 * n) + e3 / n) for s in range(n)], F)
    return ox, oy


def library_offsets(lib, n, p):
    """rt_pass_offsets as float32 arrays"""
    import ctypes as C
    ox, oy = np.full(n, np.nan, F), np.full(n, np.nan, F)
    assert lib.rt_pass_offsets(n, p, ox.ctypes.data_as(C.POINTER(C.c_float)), oy.ctypes.data_as(C.POINTER(C.c_float))) == 0
    return ox, oy


def pass_key(p):
    return (p * PASS_MUL) & _M


def _mix(h):
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & _M
    h ^= h >> 12
    h = (h * 0x297A2D39) & _M
    h ^= h >> 15
    return h


def pass_hash(i, j, p):
    """h of output pixel (column i, frame row j) in pass p"""
    return _mix(((i * 0x9E3779B1) & _M) ^ ((j * 0x85EBCA6B) & _M) ^ pass_key(p))


def pass_g(i, j, p):
    """g of rt_set_shutter, derived from the h of pass p as before"""
    return _mix(pass_hash(i, j, p) ^ shutter_ref.G_XOR)


def pass_hash_array(i, j, p):
    i, j = np.asarray(i, np.uint64), np.asarray(j, np.uint64)
    m = np.uint64(_M)
    h = ((i * np.uint64(0x9E3779B1)) & m) ^ ((j * np.uint64(0x85EBCA6B)) & m) ^ np.uint64(pass_key(p))
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m
    h ^= h >> np.uint64(15)
    return h


@contextlib.contextmanager
def pass_scrambles(p):
    """inside the block lens_ref.lens_hash / lens_hash_array (which shutter_ref derives g from) are those of pass p"""
    saved = lens_ref.lens_hash, lens_ref.lens_hash_array
    lens_ref.lens_hash = lambda i, j: pass_hash(i, j, p)
    lens_ref.lens_hash_array = lambda i, j: pass_hash_array(i, j, p)
    try:
        yield
    finally:
        lens_ref.lens_hash, lens_ref.lens_hash_array = saved


def fold_passes(frames):
    """A = 0.0f; A = A + F_p in order; A / (float)count -- float32, no reassociation"""
    acc = np.zeros_like(np.asarray(frames[0], F))
    for f in frames:
        acc = (acc + np.asarray(f, F)).astype(F)
    return (acc / F(len(frames))).astype(F)
