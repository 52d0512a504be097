"""Every RT_* environment switch the library reads, and how the suite holds it to the default frame.

Plain data (no GPU, no torch).  tests/test_switch_coverage.py keeps the table equal to the set of getenv("RT_...") names in csrc/;
tests/test_gpu_switches.py renders every case below and asserts that it equals the default frame of its config bit for bit.

Each switch has exactly one of:
  cases   -- a list of {"env": {...}, "configs": [config keys], "proof": (evidence kinds)}; an empty proof tuple means a pure scheduling
             switch, where equality with the default frame is the whole assertion.  Evidence kinds (any one must hold):
               "launches"       rt_stats.launches_total differs from the default frame's
               "tasks:<queue>"  the RT_DEBUG level-0 line reports more tasks in <queue> (closest / centre / shadow) than the default frame's
               "tasks_changed"  the RT_DEBUG level-0 task counts differ from the default frame's
               "work:<k>"       the counting build's shadow step counter k (Control::prof[RT_WORK_SHADOW + k]) is higher under the case than
                                under the same environment without the switch (and the counting build renders the default frame too)
  covered -- "tests/<file>.py::<test name>" of an existing test that renders the switch against the default path or the oracle
  exempt  -- why the switch needs no frame test
"""

# Small frames that reach every shadow regime: the stack walk (k_shadow, up to 32 samples), the shaft walk (k_shadow_shaft, 33-64) and
# the per-hit beam test in front of it (k_pair_beam, more than 64), on tree and flat scenes.  scene: a file under tests/golden/scenes or
# a scenes_gen generator; cap: leaf capacity of the octree (1000 keeps the 52-triangle mixed scene flat, 16 makes it a tree of depth 3;
# at 8 and 12 the host octree build passes its bound of 4,194,304 nodes and the loader refuses the mesh; the seeded soup at 250 is a tree
# of depth 4 with full leaves).
THREE = ((-1.0, 1.0, 1.0), (0.8, 0.4, 1.5), (0.0, 0.0, 2.0))
CONFIGS = {
    "dodge_g5": dict(scene="dodgeColorTest.obj", cap=1000, area=True, grid=5, lights=THREE[:1], depth=2, size=(160, 120), yaw=0.0),
    "dodge_g8": dict(scene="dodgeColorTest.obj", cap=1000, area=True, grid=8, lights=THREE[:1], depth=2, size=(160, 120), yaw=0.0),
    "dodge_g16": dict(scene="dodgeColorTest.obj", cap=1000, area=True, grid=16, lights=THREE[:1], depth=2, size=(128, 96), yaw=0.0),
    "dodge_g16_l3": dict(scene="dodgeColorTest.obj", cap=1000, area=True, grid=16, lights=THREE, depth=2, size=(96, 72), yaw=0.0),
    "dodge_point": dict(scene="dodgeColorTest.obj", cap=1000, area=False, grid=1, lights=THREE[:1], depth=2, size=(160, 120), yaw=0.0),
    "soup_g3": dict(scene="soup", cap=250, area=True, grid=3, lights=THREE[:1], depth=3, size=(128, 96), yaw=0.0),
    "soup_g8": dict(scene="soup", cap=250, area=True, grid=8, lights=THREE[:1], depth=2, size=(96, 72), yaw=0.3),
    "mixed_tree": dict(scene="mixed", cap=16, area=True, grid=5, lights=THREE, depth=5, size=(160, 112), yaw=0.4),
    "cube": dict(scene="cube.obj", cap=1000, area=True, grid=8, lights=THREE[:1], depth=4, size=(160, 120), yaw=0.0),
    "mixed_flat1": dict(scene="mixed", cap=1000, area=True, grid=8, lights=THREE[:1], depth=4, size=(160, 112), yaw=0.4),
    "mixed_flat3": dict(scene="mixed", cap=1000, area=True, grid=5, lights=THREE, depth=4, size=(160, 112), yaw=0.4),
}
TREES = ["dodge_g5", "dodge_g8", "dodge_g16", "dodge_point", "soup_g3", "mixed_tree"]
FLATS = ["cube", "mixed_flat1", "mixed_flat3"]
# trees whose leaves span several 64-triangle chunks: a piece target changes how many tasks a leaf becomes (mixed_tree's hold 15 at most)
CHUNKY_TREES = ["dodge_g5", "dodge_g8", "dodge_point", "soup_g3"]

LAUNCHES, SCHEDULING = ("launches",), ()


def _case(env, configs, proof):
    return {"env": env, "configs": list(configs), "proof": tuple(proof)}


SWITCHES = {
    # ---- already rendered against the default path or the oracle elsewhere
    "RT_NO_CULL": {"covered": "tests/test_flat_shadow_fold.py::test_cube_fold_equals_shadow_units_no_cull_and_oracle"},
    "RT_NO_DEEP": {"covered": "tests/test_gpu_round3.py::test_deep_levels_in_one_launch_equal_the_wide_kernels_and_the_oracle"},
    "RT_SHADOW_UNITS": {"covered": "tests/test_flat_shadow_fold.py::test_cube_fold_equals_shadow_units_no_cull_and_oracle"},
    "RT_ITEM_BEAM": {"covered": "tests/test_gpu_round3.py::test_pair_beam_on_equals_off_equals_oracle"},
    "RT_BEAM_TREES": {"covered": "tests/test_gpu_paths.py::test_beam_test_of_whole_tiles_is_exact"},
    "RT_NO_BEAM": {"covered": "tests/test_gpu_paths.py::test_beam_test_of_whole_tiles_is_exact"},
    "RT_TASK_CAP": {"covered": "tests/test_gpu_parity.py::test_leaf_task_queue_overflow_is_exact"},
    # (flat scenes: tests/test_flat_shadow_fold.py::test_beam_budget_one_sends_the_tiles_to_the_per_hit_cull; here the beam test on a tree)
    "RT_BEAM_BUDGET": {"cases": [
        # beams over budget (counter 81): RT_BEAM_TREES=1 alone against RT_BEAM_TREES=1 with the budget of 1
        _case({"RT_BEAM_BUDGET": "1", "RT_BEAM_TREES": "1"}, ["dodge_g8"], ("work:81",)),
    ]},
    # ---- diagnostics
    "RT_DEBUG": {"exempt": "diagnostic output only: prints the level-0 task counts to stderr (the switch tests read that line as evidence)"},
    # ---- paths and budgets
    "RT_STAGED_TRACE": {"cases": [
        _case({"RT_STAGED_TRACE": "0"}, TREES, LAUNCHES),                                  # the fused k_trace<.., FLAT=false> on trees
    ]},
    "RT_TRACE_DYNAMIC": {"cases": [
        _case({"RT_TRACE_DYNAMIC": "1"}, FLATS, SCHEDULING),
        _case({"RT_TRACE_DYNAMIC": "1", "RT_STAGED_TRACE": "0"}, TREES, LAUNCHES),
    ]},
    "RT_NO_SHAFT": {"cases": [
        # dodge_g16: k_pair_beam + k_shadow_shaft become k_shadow + its leaf tasks, two launches either way; the tasks show the stack walk
        _case({"RT_NO_SHAFT": "1"}, ["dodge_g8", "dodge_g16", "soup_g8"], ("launches", "tasks:shadow")),
        _case({"RT_NO_SHAFT": "1", "RT_SHADOW_BUDGET": "1", "RT_TASK_CAP": "64"}, ["dodge_g8", "soup_g8"], ("tasks:shadow",)),
    ]},
    "RT_SHAFT_MIN_SAMPLES": {"cases": [
        _case({"RT_SHAFT_MIN_SAMPLES": "1"}, ["dodge_point", "dodge_g5", "mixed_tree"], LAUNCHES),     # mixed_tree: three lights, lslots 3
        _case({"RT_SHAFT_MIN_SAMPLES": "100000"}, ["dodge_g16"], ("launches", "tasks:shadow")),
    ]},
    "RT_SHAFT_BUDGET": {"cases": [
        _case({"RT_SHAFT_BUDGET": "1"}, ["dodge_g8", "dodge_g16", "soup_g8"], ("launches", "tasks:shadow")),
        # 0 differs from the default only on the bounce levels (3,000 there): soup_g8 reflects
        _case({"RT_SHAFT_BUDGET": "0"}, ["soup_g8"], LAUNCHES),
        _case({"RT_ITEM_BEAM": "2", "RT_SHAFT_BUDGET": "1"}, ["dodge_g8"], LAUNCHES),
    ]},
    "RT_SHADOW_BUDGET": {"cases": [
        _case({"RT_SHADOW_BUDGET": "1"}, ["dodge_g5", "soup_g3"], ("tasks:shadow",)),
        _case({"RT_SHADOW_BUDGET": "0"}, ["dodge_g5", "soup_g3"], LAUNCHES),
    ]},
    "RT_TRACE_BUDGET": {"cases": [
        _case({"RT_TRACE_BUDGET": "1"}, TREES, ("tasks:closest",)),
        _case({"RT_TRACE_BUDGET": "0"}, TREES, LAUNCHES),
    ]},
    "RT_TASK_TARGET": {"cases": [
        _case({"RT_TASK_TARGET": "1"}, CHUNKY_TREES, ("tasks_changed",)),
        _case({"RT_TASK_TARGET": "1048576"}, CHUNKY_TREES, ("tasks_changed",)),
        _case({"RT_TASK_TARGET": "1", "RT_TASK_CAP": "64"}, CHUNKY_TREES, ("tasks_changed",)),
    ]},
    "RT_NO_PLANE_CULL": {"cases": [
        _case({"RT_NO_PLANE_CULL": "1"}, FLATS, LAUNCHES),                                 # also turns the k_beam / k_shade fold off
    ]},
    # ---- pure scheduling: which wave does what
    "RT_QUEUE_LOCAL": {"cases": [_case({"RT_QUEUE_LOCAL": v}, ["dodge_g5", "dodge_g8"], SCHEDULING) for v in ("0", "1", "64")]},
    "RT_QUEUE_DIV": {"cases": [_case({"RT_QUEUE_DIV": v}, ["dodge_g5", "dodge_g8"], SCHEDULING) for v in ("1", "4096")]},
    "RT_GRID_MULT": {"cases": [_case({"RT_GRID_MULT": v, "RT_TRACE_OCC": "1"}, ["cube", "dodge_g8"], SCHEDULING) for v in ("1", "8")]},
    "RT_TRACE_OCC": {"cases": [_case({"RT_TRACE_OCC": "8"}, ["cube", "dodge_g8"], SCHEDULING)]},
    "RT_STAGE_MULT": {"cases": [_case({"RT_STAGE_MULT": v}, TREES, SCHEDULING) for v in ("1", "8")]},
    "RT_ITEM_BEAM_BLOCKS": {"cases": [_case({"RT_ITEM_BEAM_BLOCKS": "1"}, ["dodge_g16_l3"], SCHEDULING)]},
}
