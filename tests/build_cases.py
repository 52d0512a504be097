"""Octree-build cases shared by tests/test_host_scene.py (host build against the CPU oracle) and tests/test_gpu_build_fuzz.py (device
build against the host build), and the figures of a flattened tree that both assert.

DEPTH_LIMITED: scenes_gen.random_soup(dir, seed, n) built at (capacity, max_depth).  Small capacities make the reference's construction
explode on these soups (the normalised-vector SAT accepts a scene-sized triangle in every octant), so every case bounds the tree with
max_depth; the depth limit then leaves thousands of over-full leaves, and the "exactly capacity" rule leaves lost nodes.  The figures are
the CPU oracle's (oracle/rt_oracle.c: orc_build_tree), recorded once: pool nodes, lost nodes (a child with exactly `capacity` faces:
neither leaf nor split), leaves holding more than `capacity` faces, and the largest leaf.
"""
import numpy as np

RT_NODE_LEAF = 0x80000000

#                seed     n  cap  max_depth   nodes  lost  over-full  largest leaf
DEPTH_LIMITED = [(31, 2000,  64, 4,           21033,   42,     16864,          348),
                 (32, 5000, 128, 4,           14601,   18,     11366,          750),
                 (33, 1000,  32, 4,           22065,   74,     18091,          190),
                 (34,  300,  16, 5,           95393,  511,     80859,           63),
                 (37, 4000, 100, 3,            3665,    2,      2585,          693),
                 (38, 1000,   1, 3,            4681,    0,      4096,          174),
                 (40, 2500,  50, 4,           33921,   16,     28800,          433)]

SCALE_EXPONENTS = (-20, -64, -70, -80, 40, 60)          # uniform scales 2^e; from 2^64 on the construction explodes on soup 8
SCALE_SOUP_8 = (8, 800, 250, 15)                        # 25 nodes at every scale above
SOUP_8_DENORMAL_EXPONENTS = (-70, -80)                  # the squares inside normalized() are denormal: the oracle builds ANOTHER tree there


def scale_model(e):
    s = 2.0 ** e
    return [s, 0.0, 0.0, 0.0, 0.0, s, 0.0, 0.0, 0.0, 0.0, s, 0.0]


def tree_figures(hs, cap):
    """(pool nodes, lost nodes, leaves over `cap`, largest leaf) of a HostScene, from info() and the flattened arrays"""
    info = hs.info()
    cf = hs.arrays()["node_count_flags"]
    leaf_sizes = (cf[(cf & RT_NODE_LEAF) != 0] & 0x7FFFFFFF).astype(np.int64)
    assert int(leaf_sizes.max(initial=0)) == info["max_leaf"] and int(leaf_sizes.sum()) == info["face_refs"]
    return info["nodes"], info["lost_nodes"], int((leaf_sizes > cap).sum()), info["max_leaf"]
