"""Shared pieces of the scene-change tests (tests/test_gpu_scene_lifecycle.py, tests/test_scene_cases.py): the five scenes a context is
walked through, each with the class of host decisions rt_upload_scene takes for it; the order of the walk; and the corrupted copies of a
valid rt_scene view, one per validation rule.  CPU only: nothing here needs a device."""
import ctypes as C
import os

import numpy as np

import scenes_gen

LEAF = 0x80000000
SOUP_TREE = (10, 1500, 400)          # scenes_gen.random_soup(seed, triangles), leaf capacity: a tree of 41 nodes, 103 of its 106 chunks never cullable
SOUP_FLAT = (12, 40, 1000)           # 40 triangles in the root leaf, its one chunk never cullable

# name -> what rt_upload_scene decides for the scene (rt_capi.cpp): flat = the root is a leaf of at most 64 references (k_trace and the
# flat shadow units instead of the tree walks); reflective = a material with illum 3, 4, 5, 6 or 9 (bounce levels exist); pass_through = a
# face of an illum-9 material (TriRec::flags & 1); bad_chunks = chunks that may never be culled (out[0] - out[1] of rt_debug_chunk_stats);
# many_bad_leaves = more than 32 leaves hold such a chunk (the bad-leaf list of k_beam is then given up: n_bad_leaves = 0xffffffff).
EXPECTED = {
    "cube":      dict(flat=True,  reflective=True,  pass_through=False, bad_chunks=False, many_bad_leaves=False, illums=(4,)),
    "dodge":     dict(flat=False, reflective=False, pass_through=False, bad_chunks=True,  many_bad_leaves=False, illums=(2,)),
    "mixed":     dict(flat=True,  reflective=True,  pass_through=True,  bad_chunks=False, many_bad_leaves=False, illums=(2, 3, 5, 6, 7, 9)),
    "soup_tree": dict(flat=False, reflective=True,  pass_through=True,  bad_chunks=True,  many_bad_leaves=True,  illums=(2, 3, 4, 5, 6, 9)),
    "soup_flat": dict(flat=True,  reflective=True,  pass_through=True,  bad_chunks=True,  many_bad_leaves=False, illums=(2, 3, 4, 5, 6, 9)),
}
NAMES = tuple(EXPECTED)


def scene_files(scenes_dir, tmp_dir):
    """name -> (path, leaf capacity) of the five scenes; the generated ones are written under tmp_dir"""
    tmp_dir = str(tmp_dir)
    return {
        "cube": (os.path.join(scenes_dir, "cube.obj"), 1000),
        "dodge": (os.path.join(scenes_dir, "dodgeColorTest.obj"), 1000),
        "mixed": (scenes_gen.mixed_materials(tmp_dir), 1000),
        "soup_tree": (scenes_gen.random_soup(tmp_dir, SOUP_TREE[0], SOUP_TREE[1]), SOUP_TREE[2]),
        "soup_flat": (scenes_gen.random_soup(tmp_dir, SOUP_FLAT[0], SOUP_FLAT[1]), SOUP_FLAT[2]),
    }


def chunk_stats(rt, view):
    """rt_debug_chunk_stats -> (status, [chunks, cullable chunks, leaves, max chunks per leaf])"""
    out = (C.c_int32 * 4)()
    st = rt.load_library().rt_debug_chunk_stats(C.byref(view), out)
    return st, [int(x) for x in out]


def chunk_bounds(rt, view):
    """rt_debug_chunk_bounds -> (status, bounds float32 [chunks, 16], leaf_chunk0 uint32 [n_nodes])"""
    lib = rt.load_library()
    n = C.c_int32()
    st = lib.rt_debug_chunk_bounds(C.byref(view), None, 0, C.byref(n), None, None)
    if st != 0:
        return st, None, None
    b = np.zeros((max(n.value, 1), 16), np.float32)
    chunk0 = np.zeros(view.n_nodes, np.uint32)
    st = lib.rt_debug_chunk_bounds(C.byref(view), b.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n),
                                   chunk0.ctypes.data_as(C.POINTER(C.c_uint32)), None)
    return st, b[:n.value], chunk0


def classify(rt, hs):
    """the class of a HostScene, from HostScene.info(), its materials and the chunk bounds (the rules of rt_upload_scene, restated)"""
    info, a = hs.info(), hs.arrays()
    st, cs = chunk_stats(rt, hs.view)
    assert st == 0
    st, bounds, chunk0 = chunk_bounds(rt, hs.view)
    assert st == 0 and len(bounds) == cs[0]
    bad_leaves = 0
    for i in np.nonzero(a["node_count_flags"] & LEAF)[0]:
        cnt = int(a["node_count_flags"][i] & 0x7fffffff)
        k0 = int(chunk0[i])
        bad_leaves += bool((bounds[k0:k0 + (cnt + 63) // 64, 6] >= 1.5).any())
    illums = a["mat_illum"]
    flat = info["flat_nodes"] == 1 and info["leaves"] == 1 and info["max_leaf"] <= 64
    assert flat or (info["flat_nodes"] > 1 and info["depth"] >= 1), info           # either the root leaf or a tree with inner nodes
    return dict(flat=bool(flat),
                reflective=bool(any(il == 9 or il == 6 or 2 < il < 6 for il in illums)),
                pass_through=bool((illums[a["mat_id"]] == 9).any()),
                bad_chunks=cs[0] - cs[1] > 0,
                many_bad_leaves=bad_leaves > 32,
                illums=tuple(sorted(set(int(x) for x in illums))))


def load_scenes(rt, scenes_dir, tmp_dir):
    """name -> HostScene of the five scenes, each asserted to be of its expected class (the caller closes them)"""
    out = {}
    for name, (path, cap) in scene_files(scenes_dir, tmp_dir).items():
        hs = rt.HostScene(path, cap, 15)
        got = classify(rt, hs)
        assert got == EXPECTED[name], (name, got)
        out[name] = hs
    sizes = {n: (h.view.n_nodes, h.view.n_faces) for n, h in out.items()}
    assert len(set(sizes.values())) >= 4 and sizes["dodge"] > sizes["soup_tree"] > sizes["mixed"], sizes     # larger <-> smaller both ways
    return out


def euler_circuit(n=len(NAMES), start=0):
    """a closed walk over 0 .. n-1 from `start` in which every ordered pair (previous, next), previous != next, occurs exactly once: an
    Eulerian circuit of the complete digraph (Hierholzer, smallest unused successor first) -> n * (n - 1) + 1 vertices"""
    unused = {v: [u for u in range(n) if u != v] for v in range(n)}
    stack, walk = [start], []
    while stack:
        v = stack[-1]
        if unused[v]:
            stack.append(unused[v].pop(0))
        else:
            walk.append(stack.pop())
    walk.reverse()
    pairs = list(zip(walk, walk[1:]))
    assert len(walk) == n * (n - 1) + 1 and walk[0] == walk[-1] and len(set(pairs)) == n * (n - 1) and all(a != b for a, b in pairs)
    return walk


# (from the one scene that is not reflective: a context that took `reflective` from its first upload alone would never trace a bounce)
WALK = tuple(NAMES[i] for i in euler_circuit(start=NAMES.index("dodge")))


# ------------------------------------------------------------------------------------------------------------ corrupted views
class BadView:
    """a corrupted copy of an rt_scene view: `view` (with `keep` holding the one array it owns), the status rt_upload_scene, rt_debug_chunk_stats
    and rt_debug_chunk_bounds return for it and the text rt_last_error holds after the refused upload"""

    def __init__(self, name, view, status, text, keep=None):
        self.name, self.view, self.status, self.text, self.keep = name, view, status, text, keep


def copy_view(rt, view):
    v = rt.capi.rt_scene()
    C.memmove(C.byref(v), C.byref(view), C.sizeof(v))
    return v


def _nodes(view):
    """a copy of the node array as uint32 [n_nodes, 8]: six box floats, first, count_flags"""
    return np.ctypeslib.as_array(C.cast(view.nodes, C.POINTER(C.c_uint32)), shape=(view.n_nodes, 8)).copy()


def _with_nodes(rt, view, nodes):
    v = copy_view(rt, view)
    nodes = np.ascontiguousarray(nodes, np.uint32)
    v.nodes = C.cast(nodes.ctypes.data_as(C.c_void_p), C.POINTER(rt.capi.rt_node))
    v.n_nodes = nodes.shape[0]
    return v, nodes


def chain_view(rt, view, inner):
    """`inner` single-child inner nodes 0 .. inner-1 (node k's child is k + 1, so node k is at depth k) above one leaf that holds every face
    reference; every node carries the root box.  Valid up to the leaf's depth 16 (inner = 16): the traversal stack bound."""
    root = _nodes(view)[0]
    nodes = np.tile(root, (inner + 1, 1))
    for k in range(inner):
        nodes[k, 6], nodes[k, 7] = k + 1, 1
    nodes[inner, 6], nodes[inner, 7] = 0, LEAF | view.n_face_refs
    return _with_nodes(rt, view, nodes)


def corrupted_views(rt, view):
    """-> [BadView]: one per rule of the validation in front of an upload (rt_upload_scene, validate_scene).  Each copies the struct and the
    one array it edits; the memory `view` points to is only read."""
    c = rt.capi
    INV, UNS = c.RT_ERR_INVALID, c.RT_ERR_UNSUPPORTED
    assert view.n_nodes > 0 and view.n_faces > 0 and view.n_face_refs > 0 and view.n_materials > 0
    out = []

    def field(name, attr, value, text, status=INV):
        v = copy_view(rt, view)
        setattr(v, attr, value)
        out.append(BadView(name, v, status, text))

    field("nodes NULL", "nodes", C.POINTER(c.rt_node)(), b"empty scene")
    field("n_nodes 0", "n_nodes", 0, b"empty scene")
    field("materials NULL", "materials", C.POINTER(c.rt_material)(), b"empty scene")
    field("n_materials 0", "n_materials", 0, b"empty scene")
    for attr, typ in (("tri_verts", C.c_float), ("face_normal", C.c_float), ("tri_vid", C.c_uint32), ("mat_id", C.c_int32), ("vert_normal", C.c_float)):
        field(f"{attr} NULL", attr, C.POINTER(typ)(), b"missing arrays")

    def nodes_case(name, edit, text, status=INV):
        nodes = _nodes(view)
        edit(nodes)
        v, keep = _with_nodes(rt, view, nodes)
        out.append(BadView(name, v, status, text, keep))

    base = _nodes(view)
    leaf = int(np.nonzero(base[:, 7] & LEAF)[0][-1])                  # the last leaf
    inner = np.nonzero((base[:, 7] & LEAF) == 0)[0]
    j = int(inner[-1]) if len(inner) else 0                           # the last inner node; a flat scene's root leaf is turned into one
    first_ok = j + 1 if j + 1 < view.n_nodes else view.n_nodes        # (a child range that starts behind j)

    def leaf_past(n):
        n[leaf, 7] = LEAF | (view.n_face_refs - int(n[leaf, 6]) + 1)
    nodes_case("leaf range past n_face_refs", leaf_past, b"leaf range outside face_refs")

    def nine(n):
        n[j, 6], n[j, 7] = first_ok, 9
    nodes_case("inner node with 9 children", nine, b"bad child range")

    def backward(n):
        n[j, 6], n[j, 7] = j, 1
    nodes_case("inner node with first <= i", backward, b"bad child range")

    def overrun(n):
        n[j, 6], n[j, 7] = view.n_nodes, 1
    nodes_case("inner node with first + count > n_nodes", overrun, b"bad child range")

    v, keep = chain_view(rt, view, 18)
    out.append(BadView("chain of 18 single-child inner nodes", v, UNS, b"deeper than 16 levels", keep))

    def array_case(name, attr, ctype, shape, edit, text):
        a = np.ctypeslib.as_array(getattr(view, attr), shape=shape).copy()
        edit(a)
        v = copy_view(rt, view)
        setattr(v, attr, a.ctypes.data_as(C.POINTER(ctype)))
        out.append(BadView(name, v, INV, text, a))

    def last_ref(a):
        a[-1] = view.n_faces
    array_case("last face ref == n_faces", "face_refs", C.c_uint32, (view.n_face_refs,), last_ref, b"face ref out of range")

    def mat_neg(a):
        a[view.n_faces // 2] = -1
    array_case("mat_id -1", "mat_id", C.c_int32, (view.n_faces,), mat_neg, b"material id out of range")

    def mat_high(a):
        a[-1] = view.n_materials
    array_case("mat_id == n_materials", "mat_id", C.c_int32, (view.n_faces,), mat_high, b"material id out of range")

    def vid_high(a):
        a[-1, 1] = view.n_vert_normals
    array_case("tri_vid entry == n_vert_normals", "tri_vid", C.c_uint32, (view.n_faces, 3), vid_high, b"vertex id outside vert_normal")
    assert len(out) == 18 and len({b.name for b in out}) == 18
    return out
