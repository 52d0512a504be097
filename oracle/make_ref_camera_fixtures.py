#!/usr/bin/env python3
"""Generates tests/golden/ref_camera_pins.npz: OUTPUTS of the reference's own Camera (tucano/camera.hpp) under the view matrix of
Flycamera::updateViewMatrix with yaw, pitch and translation_vector (oracle/_ref/ref_probe2 `fly`; the Eigen statements of
flycamera.hpp:166-191 issued on the base class, no stand-ins) for the cameras of tests/ref_inputs.py: FLY_CAMERAS.

Runs only where the reference tree exists: `make -C oracle ref && python oracle/make_ref_camera_fixtures.py`.
Per camera: getCenter(), the top three rows of getViewMatrix().inverse(), and of screenToWorld on EVERY pixel the sha256 and every
1009th float.  Numbers only.  tests/golden/ref_pins.npz (oracle/make_ref_fixtures.py) is not touched by this script.
"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_inputs as RI    # noqa: E402

PROBE = os.path.join(ROOT, "oracle", "_ref", "ref_probe2")


def bits(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", x))[0]


def main():
    if not os.path.exists(PROBE):
        raise SystemExit("oracle/_ref/ref_probe2 missing: run `make -C oracle ref` (needs the reference tree)")
    out = {"fly_in_sha": RI.sha(RI.fly_camera_inputs())}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "fly.out")
        for k, (W, H, yaw, pitch, t) in enumerate(RI.FLY_CAMERAS):
            subprocess.check_call([PROBE, "fly", str(W), str(H), bits(yaw), bits(pitch)] + [bits(x) for x in t] + [path])
            v = np.fromfile(path, np.float32)
            assert v.size == 15 + W * H * 3
            out[f"fly{k}_center"] = v[:3].copy()
            out[f"fly{k}_inv_view"] = v[3:15].copy()
            pts = v[15:]
            out[f"fly{k}_sha"] = hashlib.sha256(pts.tobytes()).hexdigest()
            out[f"fly{k}_every1009"] = pts[::1009].copy()
    dst = os.path.join(ROOT, "tests", "golden", "ref_camera_pins.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
