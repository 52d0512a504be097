"""rt_set_frame_overlap without a device: the declaration, the binding and the export agree, a null context is refused, the switch is a
call and not an environment variable, and the bookkeeping of the two working sets (rt_frame_sets.hpp) is a unit free of HIP whose check
program holds under the sanitizers.  (rt_create needs a device: what the switch does to frames is tests/test_gpu_frame_overlap.py.)"""
import os
import re
import subprocess

import switch_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
CSRC = os.path.join(ROOT, "raytracer-in-cpp_amd", "csrc")


def test_declaration_binding_and_export_agree(rt):
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\brt_status\s+rt_set_frame_overlap\s*\(([^)]*)\)\s*;", code)
    assert m, "rt_set_frame_overlap is not declared in the header"
    assert [a.strip() for a in m.group(1).split(",")] == ["rt_ctx *ctx", "int32_t on"]
    sigs = dict((s[0], s) for s in rt.capi._SIGNATURES)
    assert "rt_set_frame_overlap" in rt.capi.EXPORTED_SYMBOLS and len(sigs["rt_set_frame_overlap"][2]) == 2
    lib = rt.load_library()
    assert lib.rt_set_frame_overlap.argtypes == sigs["rt_set_frame_overlap"][2]
    assert callable(rt.Context.set_frame_overlap) and callable(rt.Context.overlapped_frames)
    m = re.search(r"\brt_status\s+rt_debug_overlapped_frames\s*\(([^)]*)\)\s*;", code)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["rt_ctx *ctx", "uint64_t *frames"]
    assert "rt_debug_overlapped_frames" in rt.capi.EXPORTED_SYMBOLS and lib.rt_debug_overlapped_frames(None, None) == rt.capi.RT_ERR_INVALID


def test_the_contract_stands_in_the_header():
    text = open(HEADER).read()
    for line in ("the internal work of such a frame may start before earlier work on the caller's stream has finished",
                 "that work reads and writes context memory only",
                 "the frame's outputs are written by work on the caller's stream, in call order"):
        assert line in text


def test_a_null_context_is_refused(rt):
    lib = rt.load_library()
    assert lib.rt_set_frame_overlap(None, 1) == rt.capi.RT_ERR_INVALID and lib.rt_set_frame_overlap(None, 0) == rt.capi.RT_ERR_INVALID


def test_the_switch_is_not_an_environment_variable():
    capi = open(os.path.join(CSRC, "rt_capi.cpp")).read()
    names = set(re.findall(r'getenv\("(RT_[A-Z0-9_]+)"\)', capi))
    assert names <= set(switch_table.SWITCHES), names - set(switch_table.SWITCHES)
    assert not [n for n in names if "OVERLAP" in n or "FRAME_SET" in n]


def test_the_bookkeeping_is_a_unit_without_hip():
    unit = open(os.path.join(CSRC, "rt_frame_sets.hpp")).read()
    assert re.findall(r"^\s*#\s*include\s+(\S+)", unit, flags=re.M) == ["<cstdint>"]
    code = re.sub(r"//[^\n]*", "", unit)
    assert "hipStream" not in code and "hipEvent" not in code and "hip_runtime" not in code and "__device__" not in code
    capi = open(os.path.join(CSRC, "rt_capi.cpp")).read()
    assert '#include "rt_frame_sets.hpp"' in capi
    # rt_capi.cpp executes what the unit returns: the internal streams and the four events are waited for and recorded in one place
    assert capi.count("hipStreamWaitEvent(") == 1 and "c->sets.overlapped_frame()" in capi
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^frame_sets_check:", mk, flags=re.M)
    for target in ("librt_mi355x.so", "librt_mi355x_work.so"):
        assert re.search(r"^\$\(OUT\)/%s:.*rt_frame_sets\.hpp" % re.escape(target), mk, flags=re.M), target


def test_the_check_program_holds_under_the_sanitizers(tmp_path):
    """long pseudo-random sequences of every call kind on up to three caller streams against a happens-before model of streams and
    events: tools/frame_sets_check.cpp, built and run as the Makefile does"""
    r = subprocess.run(["make", "-C", CSRC, "frame_sets_check", f"OUT={tmp_path}"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
    assert b"frame_sets_check: all checks held" in r.stdout
    src = open(os.path.join(ROOT, "tools", "frame_sets_check.cpp")).read()
    assert "-fsanitize=address,undefined" in open(os.path.join(CSRC, "Makefile")).read().split("frame_sets_check:")[1].split("\n\n")[0]
    for what in ("HOST_WAIT_FRAMES", "before_set0_use", "after_set0_use", "host_wait", "refuse", "set_on"):
        assert what in src
