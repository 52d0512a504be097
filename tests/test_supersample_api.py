"""Supersampling (rt_set_supersampling) at the C ABI, the binding and the front ends -- everything that needs no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
RT_RENDER = os.path.join(ROOT, "raytracer-in-cpp_amd", "lib", "rt_render")


def test_header_declares_supersampling():
    text = open(HEADER).read()
    assert re.search(r"^#define\s+RT_MAX_SUPERSAMPLING\s+4\b", text, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\brt_status\s+rt_set_supersampling\s*\(\s*rt_ctx\s*\*\s*ctx\s*,\s*int32_t\s+n\s*\)\s*;", code)


def test_binding_has_the_symbol_with_its_argtypes(rt):
    sig = {name: (res, args) for name, res, args in rt.capi._SIGNATURES}
    assert sig["rt_set_supersampling"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert rt.capi.RT_MAX_SUPERSAMPLING == 4
    lib = rt.load_library()
    assert lib.rt_set_supersampling.argtypes == [C.c_void_p, C.c_int32]
    assert lib.rt_set_supersampling.restype is C.c_int


@pytest.mark.parametrize("n", [-1, 0, 1, 2, 4, 5])
def test_null_context_is_invalid_without_a_device(rt, n):
    assert rt.load_library().rt_set_supersampling(None, n) == rt.capi.RT_ERR_INVALID


def test_flyscene_refuses_hit_ids_with_supersampling(rt):
    fs = rt.Flyscene()
    assert fs.supersample == 1
    fs.supersample = 2
    with pytest.raises(ValueError):                 # refused before any device call
        fs.raytraceScene(8, 8, write_ppm=False, want_hits=True)


def test_cli_usage_and_aa_range():
    assert os.path.exists(RT_RENDER), "rt_render is part of `make all`"
    bad = subprocess.run([RT_RENDER, "--bogus"], capture_output=True, timeout=60)
    assert bad.returncode == 2 and b"--aa N" in bad.stderr
    for n in ("0", "5"):
        r = subprocess.run([RT_RENDER, "--aa", n], capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--aa" in r.stderr, n
