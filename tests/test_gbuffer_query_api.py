"""The geometry-buffer query (rt_gbuffer_device, rt_gbuffer) without a device: header, binding and library agree on the two calls, the
argument rules that need no device hold, and the pass table the kernel reads is rt_pass_offsets, which equals its numpy restatement."""
import ctypes as C
import os
import re

import numpy as np

import passes_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
CSRC = os.path.join(ROOT, "raytracer-in-cpp_amd", "csrc")
F = np.float32
CALLS = {"rt_gbuffer_device": 5, "rt_gbuffer": 4}


def header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_binding_and_library_agree_on_the_two_calls(rt):
    code = header_code()
    sigs = dict((s[0], s) for s in rt.capi._SIGNATURES)
    lib = rt.load_library()
    for name, nargs in CALLS.items():
        m = re.search(r"\brt_status\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == nargs
        assert name in rt.capi.EXPORTED_SYMBOLS
        assert sigs[name][1] is C.c_int and len(sigs[name][2]) == nargs
        assert getattr(lib, name).argtypes == sigs[name][2]
    assert re.search(r"^\s*#\s*define\s+RT_GBUFFER_CHANNELS\s+8\s*$", code, flags=re.M) and rt.capi.RT_GBUFFER_CHANNELS == 8
    text = open(HEADER).read()
    section = text[text.index("---- geometry buffers"):text.index("---- light jitter offsets")]
    assert "NO FRAME FILLS THEM" in section and "rt_gbuffer_device" in section
    assert "no entry point takes them" not in section


def test_front_ends_exist(rt):
    assert callable(rt.Context.gbuffer) and callable(rt.Flyscene.gbuffer)
    assert "gbuffer(" in open(os.path.join(CSRC, "flyscene.hpp")).read()
    assert "--gbuffer" in open(os.path.join(CSRC, "rt_render_main.cpp")).read()
    assert re.search(r"^gbuffer_check:", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)


def test_the_kernel_is_appended_behind_k_hit_points():
    src = open(os.path.join(CSRC, "rt_kernels.hip")).read()
    table = src[src.index("kKernelOrder[] = {"):]
    table = re.sub(r"//[^\n]*", "", table[:table.index("};")])
    names = re.findall(r"\bK\((k_\w+)", table)
    assert "k_hit_points" in names
    tail = names[names.index("k_hit_points") + 1:]
    assert tail and set(tail) == {"k_gbuffer"} and len(tail) <= 4


def test_argument_rules_that_need_no_device(rt):
    lib = rt.load_library()
    cam, p = rt.default_camera(8, 8), rt.make_params(8, 8)
    out = np.full(8 * 8 * 8 + 16, 7.0, F)
    ptr = C.c_void_p(out.ctypes.data)
    assert lib.rt_gbuffer_device(None, C.byref(cam), C.byref(p), ptr, None) == rt.capi.RT_ERR_INVALID
    assert lib.rt_gbuffer(None, C.byref(cam), C.byref(p), ptr) == rt.capi.RT_ERR_INVALID
    assert lib.rt_gbuffer_device(None, None, None, None, None) == rt.capi.RT_ERR_INVALID
    assert lib.rt_gbuffer(None, None, None, None) == rt.capi.RT_ERR_INVALID
    assert (out == 7.0).all()
    # the rows of a call are rt_local_rows, as for a frame
    assert lib.rt_local_rows(C.byref(rt.make_params(37, 21, row0=5, row1=14))) == 9
    assert [lib.rt_local_rows(C.byref(rt.make_params(37, 21, stripe=2, rank=r, nranks=2))) for r in (0, 1)] == [11, 10]


def table_entry(n, p):
    """first float of (n, p) in the device table, as rt_gbuffer_layout.hpp lays it out: n = 1 .. 4, 256 passes each, ox[4] then oy[4]"""
    return ((n - 1) * 256 + p) * 8


def test_pass_table_is_rt_pass_offsets_and_equals_the_restatement(rt):
    lib = rt.load_library()
    layout = open(os.path.join(CSRC, "rt_gbuffer_layout.hpp")).read()
    assert "kGbMaxPasses) + static_cast<uint32_t>(p)) * 8u" in layout and "kGbMaxSupersampling = 4, kGbMaxPasses = 256" in layout
    assert "rt_pass_offsets(n, p, &h[gb_pass_entry(n, p)], &h[gb_pass_entry(n, p) + RT_MAX_SUPERSAMPLING])" in open(os.path.join(CSRC, "rt_capi.cpp")).read()
    table = np.zeros(4 * 256 * 8, F)
    seen = set()
    for n in range(1, 5):
        for p in (0, 1, 5, 255):
            ox, oy = passes_ref.library_offsets(lib, n, p)
            want_x, want_y = passes_ref.pass_offsets(n, p)
            assert np.array_equal(ox.view(np.uint32), want_x.view(np.uint32)) and np.array_equal(oy.view(np.uint32), want_y.view(np.uint32)), (n, p)
            e = table_entry(n, p)
            assert e % 8 == 0 and e + 8 <= table.size and e not in seen
            seen.add(e)
            table[e:e + n], table[e + 4:e + 4 + n] = ox, oy
            if p == 0:                                       # pass 0 is the frame of rt_set_supersampling: both halves hold its offsets
                o = np.array([F((2 * s + 1 - n) / (2.0 * n)) for s in range(n)], F)
                assert np.array_equal(ox, o) and np.array_equal(oy, o)
    assert table_entry(4, 255) + 8 == table.size == 32 * 1024 // 4
    # n = 1, pass 0: (float)v + 0.0f == (float)v for every v >= 0, so the PASS form of the raster coordinate is the pass-0 form
    assert table[0] == 0.0 and not np.signbit(table[0])
    v = np.arange(0, 4096, dtype=F)
    assert np.array_equal((v + table[0]).view(np.uint32), v.view(np.uint32))
