"""Empty lists return first: k_shade and the bounce k_trace read their list counters ahead of every set-up and leave when the list is empty.
Both sides of that return against the CPU oracle, frame and counters: cube.obj, whose mirror children are all settled inside level 0 (the
level-1 launches find nothing), and the mixed-material scene, whose bounce levels are populated."""
import os

import numpy as np
import pytest

import scenes_gen
import switch_table
import test_gpu_lens as gl

F = np.float32
W, H, DEPTH = 96, 64, 4


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in switch_table.SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cube.obj", "mixed"])
def test_empty_and_populated_bounce_levels_equal_the_oracle(rt, oracle, tmp_path, which):
    path, yaw = (scenes_gen.mixed_materials(str(tmp_path)), 0.4) if which == "mixed" else (os.path.join(gl.SCENES, which), 0.0)
    hs, ctx = gl.open_ctx(rt, path)
    osc = oracle.load_scene(path)
    L, oL = gl.area_lights(rt), oracle.lights(area=True, usteps=8, vsteps=8, points=gl.THREE[:1])
    try:
        want, _, ost = osc.render(oracle.camera(W, H, yaw), oL, W, H, max_depth=DEPTH, threads=8)
        st = rt.capi.rt_stats()
        rgb, u8 = gl.render_device(rt, ctx, rt.default_camera(W, H, yaw), L, W, H, DEPTH, stats=st)
    finally:
        osc.close(); ctx.close(); hs.close()
    assert gl.bits_equal(rgb, want), gl.diff(rgb, want)
    assert np.array_equal(u8, gl.quantise_u8(want))
    got = (st.rays_primary, st.rays_bounce, st.rays_centre, st.rays_sample, st.pixels_culled)
    ref = (ost.rays_primary, ost.rays_bounce, ost.rays_centre, ost.rays_sample, ost.precull_tests - ost.rays_primary)
    print(f"{which}: (primary, bounce, centre, sample, culled) = {got}, launches {st.launches_total}")
    assert got == ref
    if which == "mixed":
        assert st.rays_bounce > 0, "the bounce levels of this scene must be populated"
    else:
        assert st.launches_total == 9
