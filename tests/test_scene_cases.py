"""CPU side of the scene-change tests: the classes of the five walk scenes, the walk itself, and the two copies of the validation rules held
together -- validate_scene (rt_scene_image.cpp, in front of rt_debug_chunk_stats / rt_debug_chunk_bounds) must refuse, with the same status,
every corrupted view that tests/test_gpu_scene_lifecycle.py hands to the copy inside rt_upload_scene."""
import ctypes as C

import numpy as np
import pytest

import scene_cases as sc


@pytest.fixture(scope="module")
def hosts(rt, scenes, tmp_path_factory):
    hs = sc.load_scenes(rt, scenes, tmp_path_factory.mktemp("scene_cases"))      # (asserts every scene's class)
    yield hs
    for h in hs.values():
        h.close()


def test_walk_scenes_are_of_their_classes(rt, hosts):
    """flat <-> tree, reflective <-> not, chunks that may never be culled <-> none, a bad-leaf list <-> too many bad leaves for one, pass-through
    faces <-> none, and node and face counts that grow and shrink: each side of every host decision of an upload is in the set."""
    assert set(hosts) == set(sc.NAMES)
    for key in ("flat", "reflective", "pass_through", "bad_chunks", "many_bad_leaves"):
        assert {sc.EXPECTED[n][key] for n in sc.NAMES} == {False, True}, key
    st, cs = sc.chunk_stats(rt, hosts["soup_tree"].view)
    assert st == 0 and cs[0] - cs[1] > 0 and hosts["soup_tree"].info()["flat_nodes"] > 1
    assert hosts["soup_flat"].view.n_faces <= 64


def test_walk_is_an_eulerian_circuit():
    pairs = list(zip(sc.WALK, sc.WALK[1:]))
    assert len(sc.WALK) == 21 and sc.WALK[0] == sc.WALK[-1]
    assert sorted(pairs) == sorted((a, b) for a in sc.NAMES for b in sc.NAMES if a != b)


@pytest.mark.parametrize("name", sc.NAMES)
def test_validate_scene_refuses_what_the_upload_refuses(rt, hosts, name):
    """every corrupted view: rt_debug_chunk_stats and rt_debug_chunk_bounds return the status the upload's own rules give it; the view they
    were made from, and the deepest chain the traversal stack allows, return RT_OK; and making them wrote nothing into the HostScene"""
    lib = rt.load_library()
    hs = hosts[name]
    before = {k: v.copy() for k, v in hs.arrays().items()}
    out, n = (C.c_int32 * 4)(), C.c_int32()
    bad = sc.corrupted_views(rt, hs.view)
    for b in bad:
        assert lib.rt_debug_chunk_stats(C.byref(b.view), out) == b.status, (name, b.name)
        assert lib.rt_debug_chunk_bounds(C.byref(b.view), None, 0, C.byref(n), None, None) == b.status, (name, b.name)
    assert sorted({b.status for b in bad}) == [rt.capi.RT_ERR_UNSUPPORTED, rt.capi.RT_ERR_INVALID]
    assert lib.rt_debug_chunk_stats(C.byref(hs.view), out) == 0 and lib.rt_debug_chunk_bounds(C.byref(hs.view), None, 0, C.byref(n), None, None) == 0
    ok, keep = sc.chain_view(rt, hs.view, 16)
    assert lib.rt_debug_chunk_stats(C.byref(ok), out) == 0 and out[2] == 1, name
    for k, v in hs.arrays().items():
        assert np.array_equal(v.view(np.uint8), before[k].view(np.uint8)), (name, k)
