"""The ordered multi-hit ray query without a GPU: the two calls are declared, exported and bound; with a NULL context every call is refused
(rt_create needs a device, so the argument rule itself -- k, t_max, the outputs, the overlaps -- is checked by tools/hits_layout_check.cpp,
which this file builds and runs under the sanitizers as the Makefile does); the Python layers above are there; thickness_of and parity_of,
the host halves of Flyscene.thickness and Flyscene.inside, follow their definitions."""
import ctypes as C
import os
import subprocess

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer-in-cpp_amd", "csrc")


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    assert "#define RT_MAX_RAY_HITS 8" in text and "---- ordered ray hits" in text
    for name in ("rt_ray_hits_device", "rt_ray_hits"):
        assert f"rt_status {name}(" in text


def test_binding_and_library_hold_the_calls(rt):
    lib = rt.load_library()
    assert {"rt_ray_hits_device", "rt_ray_hits"} <= set(rt.capi.EXPORTED_SYMBOLS)
    assert rt.capi.RT_MAX_RAY_HITS == 8
    for name in ("rt_ray_hits_device", "rt_ray_hits"):
        assert getattr(lib, name) is not None


def test_refusals_without_a_device(rt):
    lib, inv = rt.load_library(), rt.capi.RT_ERR_INVALID
    o, d = np.zeros((4, 3), F), np.ones((4, 3), F)
    f, t, c = np.zeros((4, 8), np.int32), np.zeros((4, 8), F), np.zeros(4, np.int32)
    p = lambda a: a.ctypes.data
    inf = float("inf")
    # NULL context, valid arguments
    assert lib.rt_ray_hits_device(None, 4, p(o), p(d), 8, inf, p(f), p(t), p(c), None) == inv
    assert lib.rt_ray_hits(None, 4, p(o), p(d), 8, inf, p(f), p(t), p(c)) == inv
    # ... and with each refused argument
    for k in (0, 9, -1):
        assert lib.rt_ray_hits_device(None, 4, p(o), p(d), k, inf, p(f), p(t), p(c), None) == inv
        assert lib.rt_ray_hits(None, 4, p(o), p(d), k, inf, p(f), p(t), p(c)) == inv
    for t_max in (float("nan"), 0.0, -1.0):
        assert lib.rt_ray_hits_device(None, 4, p(o), p(d), 8, t_max, p(f), p(t), p(c), None) == inv
        assert lib.rt_ray_hits(None, 4, p(o), p(d), 8, t_max, p(f), p(t), p(c)) == inv
    assert lib.rt_ray_hits_device(None, 4, p(o), p(d), 8, inf, None, None, None, None) == inv
    assert lib.rt_ray_hits(None, 4, p(o), p(d), 8, inf, None, None, None) == inv
    assert lib.rt_ray_hits(None, -1, p(o), p(d), 8, inf, p(f), p(t), p(c)) == inv
    assert not f.any() and not t.any() and not c.any(), "a refused call writes nothing"


def test_the_hits_check_program_holds_under_the_sanitizers(tmp_path):
    """the insertion chain against a sort of the distinct set (seeded streams, every arrival order, every K and k <= K), the output rule
    behind guard words, the instantiation of a k and the argument rule: tools/hits_layout_check.cpp, built and run as the Makefile does"""
    r = subprocess.run(["make", "-C", CSRC, "hits_check", f"OUT={tmp_path}"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
    assert b"all checks held" in r.stdout
    assert b"-ffp-contract=off" in r.stdout and b"-fsanitize=address,undefined" in r.stdout


def test_the_layers_above_are_there(rt):
    assert callable(rt.Context.ray_hits) and callable(rt.Flyscene.thickness) and callable(rt.Flyscene.inside)
    import inspect
    assert inspect.signature(rt.Flyscene.distance_field).parameters["signed"].default is False
    sig = inspect.signature(rt.Context.ray_hits)
    assert list(sig.parameters)[1:7] == ["origins", "dirs", "k", "t_max", "n", "stream"] and sig.parameters["t_max"].default == float("inf")


def test_thickness_and_parity_rules(rt):
    t = np.full((5, 8), -1.0, F)
    t[1, :1] = [2.0]
    t[2, :2] = [1.0, 3.5]
    t[3, :5] = [1.0, 2.0, 4.0, 4.25, 9.0]
    t[4] = [1, 2, 3, 5, 8, 13, 21, 34]
    counts = np.array([0, 1, 2, 5, 9], np.int32)
    assert rt.thickness_of(t, counts).tolist() == [0.0, 0.0, 2.5, 1.25, 1.0 + 2.0 + 5.0 + 13.0]
    assert rt.thickness_of(t, counts).dtype == F
    assert rt.parity_of(np.array([0, 1, 2, 3, 8, 9], np.int32)).tolist() == [0, 1, 0, 1, 0, -1]
    assert rt.parity_of(counts).dtype == np.int8
    # float32, pair after pair: (a + b) + c in single precision
    t[4] = [0, 1e8, 0, 1, 0, 1, 0, 1]
    assert rt.thickness_of(t, counts)[4] == F(F(F(F(1e8) + F(1)) + F(1)) + F(1))
