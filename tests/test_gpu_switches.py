"""Every switch of tests/switch_table.py at the setting that forces its rare branch, held to the default frame bit for bit.

Each config's default frame is compared with the oracle once, at tolerance 0 (face ids, RGB bits, ray counters), and cached for the
module.  A case sets its environment, opens a fresh context and renders the same frame: the hit ids, the RGB bits and the five ray
counters must equal the default's (rays_sample_walked may differ).  A path or budget case must also show that its path ran: a different
launch count, more leaf tasks in the RT_DEBUG level-0 line than the default frame has, or a step counter of the counting build that the
same environment without the switch leaves lower (tests/switch_table.py says which).  Scheduling switches only change which wave does
what, so equality is the whole assertion there.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import switch_table

HERE = os.path.dirname(os.path.abspath(__file__))
WORK_LIB = os.path.join(os.path.dirname(HERE), "raytracer-in-cpp_amd", "lib", "librt_mi355x_work.so")
RT_WORK_SHADOW = 640          # rt_device.hpp: offset of the shadow kernels' step counters in Control::prof
SCENES = os.path.join(HERE, "golden", "scenes")
DEBUG_LINE = re.compile(r"RT_DEBUG level0: items (\d+) tasks closest (\d+) \d+ centre (\d+) \d+ shadow (\d+) \d+")


def counters(st):
    return (st.rays_primary, st.rays_bounce, st.rays_centre, st.rays_sample, st.shaded_hits)


def scene_path(scene, tmp_dir):
    import scenes_gen
    if scene == "soup":
        return scenes_gen.random_soup(tmp_dir, 10, 1500)
    if scene == "mixed":
        return scenes_gen.mixed_materials(tmp_dir)
    return os.path.join(SCENES, scene)


def set_env(monkeypatch, env):
    """only `env` (and RT_DEBUG=1, which prints the level-0 task counts) among the library's switches"""
    for name in switch_table.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("RT_DEBUG", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


class Frame:
    def __init__(self, rgb, hits, st, tasks, work=None):
        self.rgb, self.hits, self.st, self.tasks, self.work = rgb, hits, st, tasks, work


class Configs:
    """host scenes and default frames, built on first use"""

    def __init__(self, rt, oracle, tmp_dir):
        self.rt, self.oracle, self.tmp_dir = rt, oracle, tmp_dir
        self.scenes, self.defaults = {}, {}

    def host_scene(self, key):
        cfg = switch_table.CONFIGS[key]
        sk = (cfg["scene"], cfg["cap"])
        if sk not in self.scenes:
            path = scene_path(cfg["scene"], self.tmp_dir)
            self.scenes[sk] = (path, self.rt.HostScene(path, cfg["cap"], 15))
        return self.scenes[sk]

    def render(self, key, env, monkeypatch, capfd, counting=False):
        """one frame on a fresh context of the product library, or of the counting build (counting=True: its step counters come along)"""
        rt, cfg = self.rt, switch_table.CONFIGS[key]
        _, hs = self.host_scene(key)
        set_env(monkeypatch, env)
        w, h = cfg["size"]
        cam = rt.default_camera(w, h, cfg["yaw"])
        L = rt.make_lights(points=cfg["lights"], area=cfg["area"], usteps=cfg["grid"], vsteps=cfg["grid"])
        p = rt.make_params(w, h, cfg["depth"])
        rgb = np.zeros((h, w, 3), np.float32)
        hits = np.zeros((h, w), np.int32)
        st = rt.capi.rt_stats()
        lib = rt.capi.load_library(WORK_LIB) if counting else rt.load_library()
        work = (C.c_uint64 * 768)()
        capfd.readouterr()
        ctx = C.c_void_p()
        assert lib.rt_create(C.byref(ctx), 0) == rt.capi.RT_OK
        try:
            rt.capi.check(lib, ctx, lib.rt_upload_scene(ctx, C.byref(hs.view)), "rt_upload_scene")
            rc = lib.rt_render(ctx, C.byref(cam), C.byref(L), C.byref(p), rgb.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), C.byref(st))
            rt.capi.check(lib, ctx, rc, f"rt_render {key} {env}")
            if counting:
                rt.capi.check(lib, ctx, lib.rt_debug_work_counters(ctx, work, 768), "rt_debug_work_counters")
        finally:
            lib.rt_destroy(ctx)
        lines = DEBUG_LINE.findall(capfd.readouterr().err)
        assert len(lines) == 1, "one RT_DEBUG level-0 line per rendered frame"
        items, closest, centre, shadow = (int(x) for x in lines[0])
        return Frame(rgb, hits, st, {"items": items, "closest": closest, "centre": centre, "shadow": shadow},
                     np.array(work, np.uint64) if counting else None)

    def default(self, key, monkeypatch, capfd):
        if key not in self.defaults:
            cfg, orc = switch_table.CONFIGS[key], self.oracle
            f = self.render(key, {}, monkeypatch, capfd)
            path, _ = self.host_scene(key)
            w, h = cfg["size"]
            osc = orc.load_scene(path, capacity=cfg["cap"])
            try:
                ref, rhits, ost = osc.render(orc.camera(w, h, cfg["yaw"]), orc.lights(area=cfg["area"], usteps=cfg["grid"], vsteps=cfg["grid"],
                                             points=cfg["lights"]), w, h, max_depth=cfg["depth"], threads=8, want_hits=True)
            finally:
                osc.close()
            assert np.array_equal(f.hits, rhits), f"{key}: {int((f.hits != rhits).sum())} face ids differ from the oracle"
            assert np.array_equal(f.rgb.view(np.uint32), ref.view(np.uint32)), f"{key}: max |RGB - oracle| = {float(np.abs(f.rgb - ref).max())}"
            assert (f.st.rays_bounce, f.st.rays_centre, f.st.rays_sample) == (ost.rays_bounce, ost.rays_centre, ost.rays_sample), key
            assert (rhits >= 0).sum() > 0.02 * rhits.size, f"{key}: the frame must show the object"
            self.defaults[key] = f
        return self.defaults[key]

    def close(self):
        for _, hs in self.scenes.values():
            hs.close()


@pytest.fixture(scope="module")
def configs(rt, oracle, tmp_path_factory):
    c = Configs(rt, oracle, str(tmp_path_factory.mktemp("switch_scenes")))
    yield c
    c.close()


def assert_same_frame(f, d, what):
    assert np.array_equal(f.hits, d.hits), f"{what}: {int((f.hits != d.hits).sum())} face ids differ from the default frame"
    assert np.array_equal(f.rgb.view(np.uint32), d.rgb.view(np.uint32)), f"{what}: max |RGB - default| = {float(np.abs(f.rgb - d.rgb).max())}"
    assert counters(f.st) == counters(d.st), f"{what}: ray counters {counters(f.st)} != default {counters(d.st)}"


def evidence(configs, key, name, case, f, d, kind, monkeypatch, capfd):
    """(shown, what was compared)"""
    if kind == "launches":
        return f.st.launches_total != d.st.launches_total, f"launches {f.st.launches_total} vs default {d.st.launches_total}"
    if kind == "tasks_changed":
        return f.tasks != d.tasks, f"level-0 tasks {f.tasks} vs default {d.tasks}"
    if kind.startswith("tasks:"):
        q = kind.split(":")[1]
        return f.tasks[q] > d.tasks[q], f"level-0 {q} tasks {f.tasks[q]} vs default {d.tasks[q]}"
    # work:<k>: counting build, the case against the same environment without the switch itself
    k = RT_WORK_SHADOW + int(kind.split(":")[1])
    wf = configs.render(key, case["env"], monkeypatch, capfd, counting=True)
    wb = configs.render(key, {n: v for n, v in case["env"].items() if n != name}, monkeypatch, capfd, counting=True)
    assert_same_frame(wf, d, f"{key} {case['env']} (counting build)")
    return int(wf.work[k]) > int(wb.work[k]), f"counting build prof[{k}] {int(wf.work[k])} vs {int(wb.work[k])} without {name}"


CASES = [pytest.param(name, i, key, id=",".join(f"{k}={v}" for k, v in case["env"].items()) + "-" + key)
         for name, entry in switch_table.SWITCHES.items() for i, case in enumerate(entry.get("cases", ())) for key in case["configs"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name,index,key", CASES)
def test_switch_renders_the_default_frame(configs, monkeypatch, capfd, name, index, key):
    case = switch_table.SWITCHES[name]["cases"][index]
    d = configs.default(key, monkeypatch, capfd)
    f = configs.render(key, case["env"], monkeypatch, capfd)
    what = f"{key} {case['env']}"
    assert_same_frame(f, d, what)
    if case["proof"]:
        shown = [evidence(configs, key, name, case, f, d, k, monkeypatch, capfd) for k in case["proof"]]
        assert any(ok for ok, _ in shown), f"{what}: no sign that the forced path ran: " + "; ".join(msg for _, msg in shown)


@pytest.mark.gpu
def test_graph_replay_under_fused_trace_and_shaft_tasks_equals_eager(rt, configs, monkeypatch, capfd):
    """RT_STAGED_TRACE=0 + RT_SHAFT_BUDGET=1 (fused tree k_trace, shaft leaf tasks and their continuation launch) captured in a hipGraph:
    the replayed frame equals the eager frame of the same context and the default frame."""
    key = "dodge_g8"
    d = configs.default(key, monkeypatch, capfd)
    cfg = switch_table.CONFIGS[key]
    _, hs = configs.host_scene(key)
    set_env(monkeypatch, {"RT_STAGED_TRACE": "0", "RT_SHAFT_BUDGET": "1"})
    monkeypatch.delenv("RT_DEBUG")
    w, h = cfg["size"]
    ctx = rt.Context(0)
    ctx.upload(hs)
    L = rt.make_lights(points=cfg["lights"], area=cfg["area"], usteps=cfg["grid"], vsteps=cfg["grid"])
    p = rt.make_params(w, h, cfg["depth"])
    out = rt.hipmem.DeviceBuffer(h * w * 3 * 4)
    g = rt.FrameGraph(ctx, L, p, out.address, 0)
    try:
        for _ in range(3):
            g.launch(rt.default_camera(w, h, cfg["yaw"]))
        st = g.stats()
        got = out.to_numpy(np.float32, (h, w, 3))
        eager = np.zeros((h, w, 3), np.float32)
        est = rt.capi.rt_stats()
        rc = ctx.lib.rt_render(ctx.handle, C.byref(rt.default_camera(w, h, cfg["yaw"])), C.byref(L), C.byref(p), eager.ctypes.data_as(C.c_void_p), None,
                               C.byref(est))
        rt.capi.check(ctx.lib, ctx.handle, rc, "rt_render")
        assert np.array_equal(got.view(np.uint32), eager.view(np.uint32)), float(np.abs(got - eager).max())
        assert np.array_equal(got.view(np.uint32), d.rgb.view(np.uint32)), float(np.abs(got - d.rgb).max())
        assert est.launches_total != d.st.launches_total
        assert st.launches_total == est.launches_total and counters(st) == counters(d.st)
    finally:
        g.close(); out.free(); ctx.close()
