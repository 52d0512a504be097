"""Soft shadows as include/rt_mi355x.h defines them ("soft shadows"), restated in numpy float32 -- test infrastructure only.

The samples are light_jitter_ref.light_samples (one float32 operation per step, in the header's order), the per-point jitter is the hash of
ao_ref mixed once more, and visibility is the CPU checker's lightStrikes (OracleScene.light_strikes) or whatever `strikes` the caller
hands in."""
import numpy as np

import ao_ref
import light_jitter_ref

F = np.float32
M32 = 0xFFFFFFFF
POINT, AREA, SPHERE = 0, 1, 2
MAX_K = 25 * 1024
CENTRE = (F(0.5), F(0.5))


def mix(g):
    g ^= g >> 15
    g = (g * 0x2C1B3C6D) & M32
    g ^= g >> 12
    g = (g * 0x297A2D39) & M32
    g ^= g >> 15
    return g


def hash32(seed, i):
    """g of rt_shadow_jitter(seed, i)"""
    return mix(ao_ref.hash32(seed, i) ^ 0xB5297A4D)


def jitter(seed, i):
    """-> (fu, fv), two float32 in [0, 1)"""
    g = hash32(seed, i)
    return F(F(g >> 16) * F(2.0 ** -16)), F(F(g & 0xFFFF) * F(2.0 ** -16))


def jitters(seed, i):
    """jitter for an array of indices -> float32 (n, 2) (uint32 arithmetic carried in uint64)"""
    m = np.uint64(M32)
    i = np.asarray(i).reshape(-1).astype(np.uint64) & m

    def mixed(g):
        g = g ^ (g >> np.uint64(15))
        g = (g * np.uint64(0x2C1B3C6D)) & m
        g = g ^ (g >> np.uint64(12))
        g = (g * np.uint64(0x297A2D39)) & m
        return g ^ (g >> np.uint64(15))

    h = mixed(((i * np.uint64(0x9E3779B1)) & m) ^ np.uint64(((seed & M32) * 0x85EBCA6B) & M32))
    h = mixed(h ^ np.uint64(0xB5297A4D))
    return np.stack([(h >> np.uint64(16)).astype(F) * F(2.0 ** -16), (h & np.uint64(0xFFFF)).astype(F) * F(2.0 ** -16)], axis=1).astype(F)


class Lights:
    """what the definition reads of an rt_lights / an oracle olights: positions, mode, grid, lengths"""

    def __init__(self, L):
        n = int(L.n_lights if hasattr(L, "n_lights") else L.nlights)
        self.pos = np.array([[L.pos[l][k] for k in range(3)] for l in range(n)], F).reshape(n, 3)
        self.mode = int(L.mode)
        self.usteps, self.vsteps = (int(L.usteps), int(L.vsteps)) if self.mode == AREA else (1, 1)
        self.len_x, self.len_y = F(L.len_x), F(L.len_y)
        self.N = self.usteps * self.vsteps
        self.K = n * self.N


def samples(L, fo=CENTRE):
    """the K samples of the lights L (a Lights) with the offsets fo, segment order e = l * N + s -> float32 (K, 3)"""
    if L.mode == POINT:
        return L.pos.copy()
    assert L.mode == AREA, "sphere lights are not part of the definition"
    return np.concatenate([light_jitter_ref.light_samples(L.usteps, L.vsteps, L.len_x, L.len_y, c, fo) for c in L.pos]).astype(F)


def is_point(N, n):
    """which of n points are points: all of them without normals, else those whose normal is not three +-0"""
    return np.ones(n, bool) if N is None else ao_ref.is_point(np.asarray(N, F).reshape(-1, 3))


def point_samples(L, n, per_point=False, seed=0, fo=CENTRE, i=None):
    """float32 (n, K, 3): the samples point i of the call sees (i: the call indices, default 0 .. n - 1)"""
    if not per_point or L.mode == POINT:
        return np.ascontiguousarray(np.broadcast_to(samples(L, fo)[None], (n, L.K, 3)), F)
    idx = np.arange(n) if i is None else np.asarray(i)
    jj = jitters(seed, idx)
    return np.stack([samples(L, (jj[k, 0], jj[k, 1])) for k in range(n)]).astype(F)


def counts(strikes, L, P, N=None, per_point=False, seed=0, fo=CENTRE, i=None):
    """visible, uint16 (n,): strikes(P[k], S) -> bool (K,) is lightStrikes on the segments S[e] -> P[k] (OracleScene.light_strikes' second
    value, or rt_light_strikes)"""
    P = np.asarray(P, F).reshape(-1, 3)
    n = P.shape[0]
    S = point_samples(L, n, per_point, seed, fo, i)
    live = is_point(N, n)
    out = np.full(n, L.K, np.uint16)
    for k in range(n):
        if live[k]:
            out[k] = int(np.asarray(strikes(P[k], S[k])).sum())
    return out


def oracle_counts(osc, L, P, N=None, per_point=False, seed=0, fo=CENTRE, i=None):
    return counts(lambda p, s: osc.light_strikes(p, s)[1], L, P, N, per_point, seed, fo, i)


def share_of(visible, K):
    """share = (float)visible / (float)K"""
    return (np.asarray(visible).astype(F) / F(K)).astype(F)


def rms(a, b, mask):
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64))[mask]
    return float(np.sqrt((d * d).mean()))


def direction(orc, osc, width, height, yaw, light, grid, truth_grid, params, seed=0):
    """The measurement behind the per-point jitter (Soft shadows): the lit share of one area light at `light` over the hit points
    of the width x height camera at `yaw`, the frame being one call (point index = raster index, misses are "no point"), with a grid x grid
    light three ways -- cell centres, cell centres filtered, per-point jitter filtered with the denoise_ref.Params `params` -- against the
    cell centres of a truth_grid x truth_grid light.  -> dict: covered / partly (pixel counts; partly lit by the truth) and, over each of the
    two sets, the RMS distances centres / centres_filtered / jitter / jitter_filtered."""
    import denoise_ref
    import gbuffer_ref
    (o, d, f, t), _ = ao_ref.camera_points(orc, osc, width, height, yaw)
    P, N = ao_ref.hit_points(o, d, f, t, osc.arrays()["face_normal"])
    g = gbuffer_ref.sample_values(f.reshape(height, width), t.reshape(height, width), osc.arrays()["face_normal"], gbuffer_ref.face_kd(osc))

    def image(n, per_point):
        L = Lights(orc.lights(area=True, usteps=n, vsteps=n, points=[light]))
        return share_of(oracle_counts(osc, L, P, N, per_point, seed), L.K).reshape(height, width)

    truth, centres, jit = image(truth_grid, False), image(grid, False), image(grid, True)
    covered = (f >= 0).reshape(height, width)
    partly = covered & (truth > 0) & (truth < 1)
    imgs = {"centres": centres, "centres_filtered": denoise_ref.denoise(centres, g, params), "jitter": jit,
            "jitter_filtered": denoise_ref.denoise(jit, g, params)}
    out = {"covered": int(covered.sum()), "partly": int(partly.sum())}
    for name, mask in (("all", covered), ("partly_lit", partly)):
        out[name] = {k: rms(v, truth, mask) for k, v in imgs.items()}
    return out
