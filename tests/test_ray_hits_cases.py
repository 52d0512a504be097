"""The rays that tests/test_gpu_ray_hits.py holds to the restatement (tests/ray_hits_ref.py) prove their point on the CPU checker alone:
on the seeded soup and on the depth-capped tree the subset holds every list length 0 .. 8 and "more than 8", ties inside the first eight
hits (bit-equal t on different faces: the order is decided by the face id) and rays that meet one face in several leaves (the
de-duplication); the restatement's first entry is the checker's closest hit; the output rule and the prefix rule hold on its lists."""
import numpy as np
import pytest

import query_walk_cases as qc
import ray_hits_ref as rh

F = np.float32
CASES = ("soup8", "cap38")


@pytest.fixture(scope="module", params=CASES)
def lists(request, oracle, tmp_path_factory):
    name = request.param
    osc = qc.oracle_scene(oracle, tmp_path_factory.mktemp("hits"), name)
    o, d, _ = qc.sorted_rays(qc.rays(osc.arrays(), qc.CASES[name].seed))
    pick = rh.subset(len(o))
    o, d = o[pick], d[pick]
    yield name, osc, o, d, rh.all_hits(osc, o, d)
    osc.close()


def test_every_count_class_is_held(lists):
    name, _, _, _, hits = lists
    assert len(hits) == rh.SUBSET
    classes = np.bincount(np.minimum([len(h) for h in hits], rh.MAX_HITS + 1), minlength=rh.MAX_HITS + 2)
    print(name, "rays per count 0..8, >8:", classes.tolist())
    assert (classes >= 8).all(), (name, classes.tolist())


def test_ties_inside_the_first_eight_hits(lists):
    name, _, _, _, hits = lists
    ties = sum(rh.has_tie(h) for h in hits)
    print(name, "rays with a tie among their first 8 hits:", ties)
    assert ties >= 8, (name, ties)


def test_some_ray_meets_a_face_in_several_leaves(lists):
    name, osc, o, d, hits = lists
    step = 8                                        # (the leaf lists are slow: every 8th ray of the subset is enough)
    refs = rh.leaf_references(osc, o[::step], d[::step])
    shared = [i for i, r in enumerate(refs) if any(c >= 2 for c in r.values())]
    # ... and one of those faces is a HIT of its ray, so a walk without the de-duplication would report it twice
    twice = [i for i in shared if any(refs[i].get(f, 0) >= 2 for _, f in hits[i * step])]
    print(name, "rays with a face in two or more reached leaves:", len(shared), "of them with such a face among the hits:", len(twice))
    assert len(shared) >= 1, name
    assert len(twice) >= 1, name


def test_first_entry_is_the_closest_hit(lists):
    name, osc, o, d, hits = lists
    want_f, want_t = qc.reference_hits(osc, o, d)
    face, t, count = rh.outputs(hits, 1)
    assert np.array_equal(face[:, 0], want_f), name
    assert np.array_equal(t[:, 0].view(np.uint32), want_t.view(np.uint32)), name
    assert np.array_equal(count == 0, want_f < 0)


def test_output_and_prefix_rule_of_the_restatement(lists):
    _, _, _, _, hits = lists
    f8, t8, c8 = rh.outputs(hits, 8)
    for k in range(1, 8):
        f, t, c = rh.outputs(hits, k)
        assert np.array_equal(f, f8[:, :k]) and np.array_equal(t.view(np.uint32), t8[:, :k].view(np.uint32)) and np.array_equal(c, np.minimum(c8, k + 1))
    used = np.arange(8)[None, :] < np.minimum(c8, 8)[:, None]
    assert (f8[~used] == -1).all() and (t8[~used] == F(-1.0)).all() and (f8[used] >= 0).all()
    t = np.where(used, t8, np.inf)
    with np.errstate(invalid="ignore"):
        assert (np.diff(t, axis=1)[used[:, 1:]] >= 0).all(), "ascending t"
    same = used[:, 1:] & (t8[:, 1:] == t8[:, :-1])
    assert (f8[:, 1:][same] > f8[:, :-1][same]).all(), "ties by ascending face id"


def test_bounded_lists_are_prefixes_cut_at_t_max():
    hits = [[(F(1.0), 4), (F(2.0), 1), (F(2.0), 3), (F(5.0), 0)], [], [(F(2.0), 9)]]
    cut = [[h for h in r if h[0] <= F(2.0)] for r in hits]
    f, t, c = rh.outputs(cut, 2)
    assert f.tolist() == [[4, 1], [-1, -1], [9, -1]] and c.tolist() == [3, 0, 1] and t[1].tolist() == [-1.0, -1.0]
