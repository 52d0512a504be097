"""Child process of tests/test_gpu_gbuffer.py: the geometry buffers of a few fixed settings, computed in a fresh process (so that the RT_*
environment switches of the parent's command line are read by a fresh library and context) and saved to an .npz file.
usage: python gbuffer_child.py OUT.npz SCENE.obj [SCENE.obj ...]"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

W, H = 37, 21
# (key, n, (first, count), lens, shutter)
CASES = [("pinhole", 2, (1, 2), None, False), ("one", 1, (0, 1), None, False), ("both", 3, (2, 1), (0.08, 1.8), True)]


def buffers(rt, ctx, lib=None):
    """{key: float32 (H, W, 8)} of CASES on a context with a scene, through rt_gbuffer of `lib` (default: the context's)"""
    lib = lib or ctx.lib
    handle = ctx.handle if hasattr(ctx, "handle") else ctx
    cam, close, p = rt.default_camera(W, H, 0.4), rt.default_camera(W, H, 0.45), rt.make_params(W, H)
    out = {}
    for key, n, passes, lens, shutter in CASES:
        for st in (lib.rt_set_supersampling(handle, n), lib.rt_set_passes(handle, *passes), lib.rt_set_lens(handle, *(lens or (0.0, 2.0))),
                   lib.rt_set_shutter(handle, C.byref(close) if shutter else None)):
            assert st == 0
        g = np.full((H, W, 8), np.nan, np.float32)
        rt.capi.check(lib, handle, lib.rt_gbuffer(handle, C.byref(cam), C.byref(p), g.ctypes.data_as(C.c_void_p)), "rt_gbuffer")
        out[key] = g
    return out


def main(argv):
    import rtpkg
    rt = rtpkg.load()
    out = {}
    for path in argv[2:]:
        hs = rt.HostScene(path, 1000, 15)
        ctx = rt.Context(0)
        ctx.upload(hs)
        for key, g in buffers(rt, ctx).items():
            out[os.path.basename(path) + ":" + key] = g
        ctx.close()
        hs.close()
    np.savez(argv[1], **out)


if __name__ == "__main__":
    main(sys.argv)
