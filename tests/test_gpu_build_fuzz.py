"""The device octree build (rt_build.hip: k_classify, k_scatter and the host loop of gpu_build_octree) on a real MI355X, held to the
host build (HostScene::build_octree) array for array on the input where such kernels go wrong: seeded soups with slivers, zero-area,
duplicated and scene-sized triangles; depth-limited trees with thousands of over-full leaves, lost "exactly capacity" nodes and child
lists of several 256-face chunks; parent lists of exactly 256 k and 256 k + 1 faces; uniform scales down to 2^-80, where the squares
inside normalized() are denormal and the reference builds another tree; repeated builds on one scene and context; and rays traced
through a tree that was built on the device.

The host build is the reference: tests/test_host_scene.py pins it bit for bit to the CPU oracle on these shapes (and the oracle is
pinned to the reference's boxTree.cpp), so a mismatch here points at the device.

Out of scope, on purpose: the refusal path (RT_ERR_UNSUPPORTED past 4 M nodes or 256 M face references).  Reaching it takes gigabytes
of host memory and minutes of classification; no test here goes there.
"""
import os
import types

import numpy as np
import pytest

import build_cases as bc
import scenes_gen
import test_gpu_parity
import test_gpu_ray_queries as queries

pytestmark = pytest.mark.gpu

LEAF = bc.RT_NODE_LEAF
TREE_KEYS = ("node_box", "node_first", "node_count_flags", "face_refs")
# the (seed, n_tri, cap) of the render fuzz test: until now these soups reached the device through the host build only
FUZZ_SOUPS = next(m for m in test_gpu_parity.test_random_soups_match_oracle.pytestmark if m.name == "parametrize").args[1]


def tree_arrays(hs):
    a = hs.arrays()
    return {k: a[k].copy() for k in TREE_KEYS}


def flat_levels(tree):
    """level of every node of a flattened tree (children of a node are contiguous from node_first)"""
    first, cf = tree["node_first"], tree["node_count_flags"]
    lvl = np.zeros(len(cf), np.int64)
    for i in range(len(cf)):
        if not int(cf[i]) & LEAF:
            lvl[int(first[i]):int(first[i]) + (int(cf[i]) & 0x7FFFFFFF)] = lvl[i] + 1
    return lvl


def first_difference(want, got):
    """-> None, or a sentence naming the first node (index and level, by the host tree) at which the two flattened trees differ"""
    nw, ng = len(want["node_count_flags"]), len(got["node_count_flags"])
    n = min(nw, ng)
    bad = np.zeros(n, bool)
    bad |= (want["node_box"][:n].view(np.uint32) != got["node_box"][:n].view(np.uint32)).any(axis=1)
    bad |= want["node_first"][:n] != got["node_first"][:n]
    bad |= want["node_count_flags"][:n] != got["node_count_flags"][:n]
    where = None
    if bad.any():
        node = int(np.argmax(bad))
        where = "box / first / count_flags"
    elif nw != ng:
        node, where = n - 1, f"node counts {nw} (host) and {ng} (device) differ after"
    else:
        rw, rg = want["face_refs"], got["face_refs"]
        m = min(len(rw), len(rg))
        d = np.nonzero(rw[:m] != rg[:m])[0]
        if len(d) == 0 and len(rw) == len(rg):
            return None
        r = int(d[0]) if len(d) else m
        leaves = np.nonzero((want["node_count_flags"] & LEAF) != 0)[0]
        node = int(leaves[np.searchsorted(want["node_first"][leaves], r, side="right") - 1])
        where = f"face_refs[{r}] (entry {r - int(want['node_first'][node])} of its list)"
    return (f"first difference at flat node {node} (level {int(flat_levels(want)[node])}): {where}; host "
            f"{want['node_box'][node].tolist()} first {int(want['node_first'][node])} count_flags {int(want['node_count_flags'][node]):#x}")


def assert_same_tree(cpu, gpu):
    """info() and the four tree arrays of two HostScenes, bit for bit; -> the host arrays"""
    a, b = tree_arrays(cpu), tree_arrays(gpu)
    diff = first_difference(a, b)
    assert diff is None, diff
    assert cpu.info() == gpu.info()
    assert np.array_equal(a["node_box"].view(np.uint32), b["node_box"].view(np.uint32))
    for k in ("node_first", "node_count_flags", "face_refs"):
        assert np.array_equal(a[k], b[k]), k
    return a


def build_both(rt, ctx, path, cap, depth, model=None, host_checks=None):
    """The same scene built twice: on the host (the reference) and, in a second HostScene, on the device of `ctx`.  `host_checks(cpu)` runs
    on the host tree before the device is called.  -> (cpu, gpu), equal array for array"""
    cpu = rt.HostScene(path, cap, depth)
    if model is not None:
        cpu.set_model(model, True)
    if host_checks:
        host_checks(cpu)
    gpu = rt.HostScene(path, cap, depth)
    if model is not None:
        gpu.set_model(model, False)                  # the moved vertices under the stale tree, as modifyTriangle leaves them
    gpu.build_gpu(ctx, cap, depth)
    assert_same_tree(cpu, gpu)
    return cpu, gpu


@pytest.fixture
def ctx(rt):
    c = rt.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("seed,n_tri,cap,max_depth,nodes,lost,overfull,largest", bc.DEPTH_LIMITED)
def test_depth_limited_soups(rt, ctx, tmp_path, seed, n_tri, cap, max_depth, nodes, lost, overfull, largest):
    """Trees of 3.6 k to 95 k nodes cut off by max_depth: the deepest level is thousands of over-full leaves whose lists k_scatter writes
    in one launch, children with exactly `cap` faces are lost nodes, and at seeds 31, 32, 37 and 40 a leaf holds more than 256 faces, so
    the running base of the compaction is carried over several chunks at the deepest level.  The conditions are asserted on the host
    tree alone, before the device builds."""
    def host_checks(cpu):
        got = bc.tree_figures(cpu, cap)
        assert got[0] == nodes, got
        assert got[1] >= 1 or seed == 38, got
        assert got[2] >= 1, got
        assert got[3] > 256 or seed not in (31, 32, 37, 40), got
        assert got == (nodes, lost, overfull, largest), got

    cpu, gpu = build_both(rt, ctx, scenes_gen.random_soup(str(tmp_path), seed, n_tri), cap, max_depth, host_checks=host_checks)
    cpu.close(); gpu.close()


@pytest.mark.parametrize("i,faces", list(enumerate((256, 257, 511, 512, 513, 1024, 1025))))
def test_block_edges_of_one_split(rt, ctx, tmp_path, i, faces):
    """A root list of exactly 256 k, 256 k + 1 or 256 k - 1 faces, split once (cap = F - 1, max_depth 0: eight leaf children, nine pool
    nodes): the tail block of k_classify has 256, 1 or 255 live lanes and the last chunk of k_scatter as many."""
    path = scenes_gen.random_soup(str(tmp_path), 50 + i, faces)

    def host_checks(cpu):
        assert cpu.view.n_faces == faces
        assert cpu.info()["nodes"] == 9 and cpu.info()["depth"] == 1

    cpu, gpu = build_both(rt, ctx, path, faces - 1, 0, host_checks=host_checks)
    cpu.close(); gpu.close()


@pytest.mark.parametrize("cap", [257, 1000])
def test_root_leaf_at_and_above_the_face_count(rt, ctx, tmp_path, cap):
    """257 faces at cap 257 (F == cap at the root: the root is a leaf, not a lost node) and at cap 1000: the early return before any launch"""
    path = scenes_gen.random_soup(str(tmp_path), 51, 257)

    def host_checks(cpu):
        assert cpu.view.n_faces == 257 and cpu.info()["nodes"] == 1 and cpu.info()["leaves"] == 1 and cpu.info()["lost_nodes"] == 0

    cpu, gpu = build_both(rt, ctx, path, cap, 0 if cap == 257 else 15, host_checks=host_checks)
    cpu.close(); gpu.close()


@pytest.mark.parametrize("seed,n_tri,cap", FUZZ_SOUPS)
def test_soups_of_the_render_fuzz_test(rt, ctx, tmp_path, seed, n_tri, cap):
    """the 16 soups of test_gpu_parity.test_random_soups_match_oracle at their capacities, depth 15: deep trees, single leaves, 5 to 6000 faces"""
    cpu, gpu = build_both(rt, ctx, scenes_gen.random_soup(str(tmp_path), seed, n_tri), cap, 15)
    cpu.close(); gpu.close()


@pytest.mark.parametrize("e", bc.SCALE_EXPONENTS)
@pytest.mark.parametrize("seed,n_tri,cap,max_depth", [bc.SCALE_SOUP_8, (37, 4000, 100, 3)])
def test_uniform_scales(rt, ctx, tmp_path, seed, n_tri, cap, max_depth, e):
    """Model matrices diag(2^e): at 2^-64 and below the squares inside normalized() are denormal or zero, at 2^60 they are near the top of
    the range.  For soup 8 the host tree at 2^-70 and 2^-80 is not the tree at scale 1 (asserted on the host alone), so a device that
    flushed or mis-rounded denormals in v * v, sqrtf or the divide would build a tree that differs from the host's."""
    path = scenes_gen.random_soup(str(tmp_path), seed, n_tri)

    def host_checks(cpu):
        if seed == 8 and e in bc.SOUP_8_DENORMAL_EXPONENTS:
            unit = rt.HostScene(path, cap, max_depth)
            assert len(cpu.arrays()["face_refs"]) != len(unit.arrays()["face_refs"])
            unit.close()

    cpu, gpu = build_both(rt, ctx, path, cap, max_depth, model=bc.scale_model(e), host_checks=host_checks)
    a, b = cpu.arrays(), gpu.arrays()
    assert np.array_equal(a["tri_verts"].view(np.uint32), b["tri_verts"].view(np.uint32))
    cpu.close(); gpu.close()


def test_sequence_of_builds_on_one_scene_and_context(rt, ctx, tmp_path):
    """large -> small -> root leaf -> large on ONE HostScene and ONE context: the node pool, the reference count and the flattened arrays
    are reset by every build, and the device buffers of a build do not leak into the next"""
    path = scenes_gen.random_soup(str(tmp_path), 40, 2500)
    gpu = rt.HostScene(path, 1000, 15)
    seen = []
    for cap, depth in [(50, 4), (1000, 15), (2500, 15), (50, 2), (50, 4)]:
        gpu.build_gpu(ctx, cap, depth)
        cpu = rt.HostScene(path, cap, depth)
        seen.append(assert_same_tree(cpu, gpu))
        if (cap, depth) == (2500, 15):
            assert cpu.info()["nodes"] == 1 and cpu.info()["leaves"] == 1                 # the root leaf
        cpu.close()
    assert len(seen[0]["node_count_flags"]) > len(seen[1]["node_count_flags"]) > len(seen[2]["node_count_flags"]) == 1
    for k in TREE_KEYS:
        assert np.array_equal(seen[0][k].view(np.uint32), seen[4][k].view(np.uint32)), k
    gpu.close()


@pytest.mark.parametrize("scene,cap,depth", [("soup31", 64, 4), ("dodgeColorTest.obj", 100, 15)])
def test_rays_through_a_device_built_tree(rt, scenes, tmp_path, scene, cap, depth):
    """The device-built scene uploaded to one context and the host-built scene to another: rt_closest_hits_device on the 1,500 awkward
    rays of test_gpu_ray_queries returns the same faces and, bit for bit, the same t"""
    path = scenes_gen.random_soup(str(tmp_path), 31, 2000) if scene == "soup31" else os.path.join(scenes, scene)
    o, d, _, _ = queries.awkward_rays()
    ctx_gpu, ctx_cpu = rt.Context(0), rt.Context(0)
    cpu, gpu = build_both(rt, ctx_gpu, path, cap, depth)
    ctx_gpu.upload(gpu)
    ctx_cpu.upload(cpu)
    got = queries.closest(types.SimpleNamespace(rt=rt, ctx=ctx_gpu, o=o, d=d), len(o))
    want = queries.closest(types.SimpleNamespace(rt=rt, ctx=ctx_cpu, o=o, d=d), len(o))
    assert (want[0] >= 0).sum() > 100                                  # the rays do reach the triangles
    assert np.array_equal(got[0], want[0])
    assert queries.same(got[1], want[1])
    ctx_gpu.close(); ctx_cpu.close(); cpu.close(); gpu.close()


def test_argument_rules(rt, ctx, scenes):
    """capacity 0, depth -1, depth 16, a NULL scene and a NULL context are RT_ERR_INVALID and leave the scene's arrays as they were"""
    lib = rt.load_library()
    hs = rt.HostScene(os.path.join(scenes, "dodgeColorTest.obj"), 100, 15)
    before, info = tree_arrays(hs), hs.info()
    inv = rt.capi.RT_ERR_INVALID
    assert lib.rt_host_scene_build_gpu(hs.handle, ctx.handle, 0, 15) == inv
    assert lib.rt_host_scene_build_gpu(hs.handle, ctx.handle, 100, -1) == inv
    assert lib.rt_host_scene_build_gpu(hs.handle, ctx.handle, 100, 16) == inv
    assert lib.rt_host_scene_build_gpu(None, ctx.handle, 100, 15) == inv
    assert lib.rt_host_scene_build_gpu(hs.handle, None, 100, 15) == inv
    hs._refresh()
    after = tree_arrays(hs)
    assert hs.info() == info
    for k in TREE_KEYS:
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
    hs.close()
