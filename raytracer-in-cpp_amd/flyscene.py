"""Python host mirror of the reference's scene controller (src/flyscene.hpp:28-200) for the ray-trace path.

``Flyscene`` keeps the reference's member names (initialize, raytraceScene, traceRay, lightStrikes,
createSpherePoint, addLight) over the C ABI; torch is plumbing only (device output buffers, torch.distributed).
"""
import ctypes as C
import sys
import time

import numpy as np

from . import capi, hipmem


def _fptr(a):
    return a.ctypes.data_as(C.c_void_p)


class HostScene:
    """rt_host_scene: OBJ/MTL import + normalisation + bug-compatible octree + flattening (host side, GL-free)."""

    def __init__(self, obj_path, leaf_capacity=1000, max_depth=15):
        self.lib = capi.load_library()
        self.handle = C.c_void_p()
        st = self.lib.rt_host_scene_load(str(obj_path).encode(), leaf_capacity, max_depth, C.byref(self.handle))
        if st != capi.RT_OK:
            raise capi.RtError(f"rt_host_scene_load({obj_path}) failed with status {st}")
        self.view = capi.rt_scene()
        self._refresh()

    def _refresh(self):
        capi.check(self.lib, None, self.lib.rt_host_scene_view(self.handle, C.byref(self.view)), "rt_host_scene_view")

    def set_model(self, model12, rebuild_tree=True):
        m = (C.c_float * 12)(*[float(x) for x in model12])
        capi.check(self.lib, None, self.lib.rt_host_scene_set_model(self.handle, m, 1 if rebuild_tree else 0), "set_model")
        self._refresh()

    def build_gpu(self, ctx, leaf_capacity=1000, max_depth=15):
        """rt_host_scene_build_gpu: the reference's octree construction on the device of `ctx` (same result as the host build)"""
        capi.check(self.lib, ctx.handle, self.lib.rt_host_scene_build_gpu(self.handle, ctx.handle, int(leaf_capacity), int(max_depth)), "rt_host_scene_build_gpu")
        self._refresh()

    def info(self):
        out = (C.c_int32 * 8)()
        box = (C.c_float * 6)()
        self.lib.rt_host_scene_info(self.handle, out, box)
        keys = ["nodes", "leaves", "face_refs", "max_leaf", "depth", "unreachable_faces", "flat_nodes", "lost_nodes"]
        d = dict(zip(keys, [int(x) for x in out]))
        d["root_box"] = [float(x) for x in box]
        return d

    # numpy copies of the flattened arrays (tests, debugging)
    def arrays(self):
        v = self.view
        nodes = np.ctypeslib.as_array(C.cast(v.nodes, C.POINTER(C.c_uint32)), shape=(v.n_nodes, 8)).copy()
        out = {
            "node_box": nodes[:, :6].copy().view(np.float32),
            "node_first": nodes[:, 6].copy(),
            "node_count_flags": nodes[:, 7].copy(),
            "face_refs": np.ctypeslib.as_array(v.face_refs, shape=(v.n_face_refs,)).copy() if v.n_face_refs else np.zeros(0, np.uint32),
            "tri_verts": np.ctypeslib.as_array(v.tri_verts, shape=(v.n_faces, 9)).copy(),
            "face_normal": np.ctypeslib.as_array(v.face_normal, shape=(v.n_faces, 3)).copy(),
            "tri_vid": np.ctypeslib.as_array(v.tri_vid, shape=(v.n_faces, 3)).copy(),
            "mat_id": np.ctypeslib.as_array(v.mat_id, shape=(v.n_faces,)).copy(),
            "vert_normal": np.ctypeslib.as_array(v.vert_normal, shape=(v.n_vert_normals, 3)).copy(),
        }
        mats = np.ctypeslib.as_array(C.cast(v.materials, C.POINTER(C.c_uint32)), shape=(v.n_materials, 9)).copy()
        out["mat_f"] = mats[:, :8].copy().view(np.float32)
        out["mat_illum"] = mats[:, 8].copy().view(np.int32)
        return out

    def close(self):
        if self.handle:
            self.lib.rt_host_scene_free(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """rt_ctx: one per HIP device."""

    def __init__(self, device=0):
        self.lib = capi.load_library()
        self.handle = C.c_void_p()
        st = self.lib.rt_create(C.byref(self.handle), int(device))
        if st != capi.RT_OK:
            raise capi.RtError(f"rt_create(device={device}) failed with status {st} "
                               "(no HIP device? this path has no CPU fallback)")
        self.device = int(device)

    def upload(self, host_scene):
        capi.check(self.lib, self.handle, self.lib.rt_upload_scene(self.handle, C.byref(host_scene.view)), "rt_upload_scene")

    def set_supersampling(self, n):
        """rt_set_supersampling: n x n sub-samples per pixel (box filter) for the frames rendered after this call; 1 = one ray per pixel"""
        capi.check(self.lib, self.handle, self.lib.rt_set_supersampling(self.handle, int(n)), "rt_set_supersampling")

    def set_supersampling_threshold(self, threshold):
        """rt_set_supersampling_threshold: with n > 1 refine only the pixels whose one-ray colour differs from a 4-neighbour's by more than
        `threshold` in some channel (< 0, the default: every pixel, the regular n x n frame)"""
        capi.check(self.lib, self.handle, self.lib.rt_set_supersampling_threshold(self.handle, float(threshold)), "rt_set_supersampling_threshold")

    def set_lens(self, aperture, focus):
        """rt_set_lens: thin-lens depth of field for the frames rendered after this call -- the n x n sub-sample rays of a pixel start at
        n x n points of a lens of radius `aperture` (world units) and meet on the plane at depth `focus` (screen-plane distances);
        aperture 0 = the pinhole camera"""
        capi.check(self.lib, self.handle, self.lib.rt_set_lens(self.handle, float(aperture), float(focus)), "rt_set_lens")

    def set_shutter(self, close):
        """rt_set_shutter: camera motion blur for the frames rendered after this call -- the camera given to a render call is the one at
        shutter open, `close` (an rt_camera, copied) the one at shutter close, and every sub-sample ray leaves the camera of its own
        time in between; None = the shutter is off"""
        capi.check(self.lib, self.handle, self.lib.rt_set_shutter(self.handle, C.byref(close) if close is not None else None), "rt_set_shutter")

    def set_passes(self, first, count):
        """rt_set_passes: the frames rendered after this call are the mean of the passes first .. first + count - 1, each with its own
        sub-sample shift and lens / time scrambles; (0, 1) = the single frame"""
        capi.check(self.lib, self.handle, self.lib.rt_set_passes(self.handle, int(first), int(count)), "rt_set_passes")

    def set_pass_tolerance(self, tol, min_passes=8):
        """rt_set_pass_tolerance: in the count-pass frames rendered after this call a pixel stops taking passes once it has taken
        `min_passes` and the standard error of its mean is at most `tol` in every channel; tol < 0 (the default) = every pixel takes
        every pass"""
        capi.check(self.lib, self.handle, self.lib.rt_set_pass_tolerance(self.handle, float(tol), int(min_passes)), "rt_set_pass_tolerance")

    def pass_map(self, width, rows):
        """rt_pass_map: the passes each output pixel of the latest eager adaptive-pass frame took, uint16 [rows, width] (synchronises)"""
        out = np.empty((int(rows), int(width)), np.uint16)
        capi.check(self.lib, self.handle, self.lib.rt_pass_map(self.handle, _fptr(out), out.size), "rt_pass_map")
        return out

    def set_primary_cull(self, on):
        """rt_set_primary_cull: the pinhole one-ray frames rendered after this call skip (True, the default) or trace (False) the primary
        tiles outside the projected bounding rectangle of the root box; the outputs and counters are the same either way"""
        capi.check(self.lib, self.handle, self.lib.rt_set_primary_cull(self.handle, 1 if on else 0), "rt_set_primary_cull")

    def set_frame_overlap(self, on):
        """rt_set_frame_overlap: the plain rt_render_device frames enqueued after this call run their launches up to the resolve on an
        internal stream and on two working sets in turn, beside the frame before them (True, the default), or on the caller's stream
        alone (False); the outputs are the same either way and are always written on the caller's stream"""
        capi.check(self.lib, self.handle, self.lib.rt_set_frame_overlap(self.handle, 2 if on == 2 else (1 if on else 0)), "rt_set_frame_overlap")

    def overlapped_frames(self):
        """rt_debug_overlapped_frames: frames of this context that took the overlapped route so far"""
        n = C.c_uint64(0)
        capi.check(self.lib, self.handle, self.lib.rt_debug_overlapped_frames(self.handle, C.byref(n)), "rt_debug_overlapped_frames")
        return int(n.value)

    def supersampling_refined(self):
        """rt_supersampling_refined: output pixels refined by the latest eager frame (synchronises)"""
        out = C.c_uint64()
        capi.check(self.lib, self.handle, self.lib.rt_supersampling_refined(self.handle, C.byref(out)), "rt_supersampling_refined")
        return int(out.value)

    # ---- device ray queries (include/rt_mi355x.h, "device ray queries").  Rays and results live in device memory: torch tensors, or
    # hipmem.DeviceBuffers with an explicit n.  Tensors must be float32, contiguous, of shape (n, 3), on this context's device; results
    # are new tensors there, and the calls run on torch's current stream.  (Torch's DEFAULT stream has no handle the C ABI could take --
    # its 0 is the ABI's "context stream" -- so there the call waits for torch's stream first, runs on the context's stream and returns
    # after rt_synchronize: correct, but not asynchronous.)  DeviceBuffers: results go to the buffers passed, or to new ones.

    def _device_array(self, what, a, count, dtype=None):
        """-> (address, whether `a` is a tensor) of a device array of `count` elements of the numpy `dtype`: a hipmem.DeviceBuffer of at least
        that many bytes, or a contiguous torch tensor of exactly that many elements of that dtype on this context's device.  dtype None: raw
        memory of at least `count` bytes, a tensor of any dtype.  ValueError otherwise.  (Every query call comes through here once per
        array, ahead of kernels of some ten microseconds: no import, and the dtype's name from its type -- numpy builds dtype.name anew.)"""
        if isinstance(a, hipmem.DeviceBuffer):
            if a.nbytes < count * (np.dtype(dtype).itemsize if dtype else 1):
                raise ValueError(f"{what}: the DeviceBuffer is shorter than {count} elements")
            return a.address, False
        torch = sys.modules.get("torch")            # (no tensor exists where nothing has imported torch)
        if torch is None or not isinstance(a, torch.Tensor) or not a.is_contiguous():
            raise ValueError(f"{what}: a contiguous torch tensor or a hipmem.DeviceBuffer, not {type(a).__name__}")
        if a.numel() * a.element_size() < count if dtype is None else (a.dtype != getattr(torch, np.dtype(dtype).type.__name__) or a.numel() != count):
            raise ValueError(f"{what}: the tensor must hold {count} " + ("bytes" if dtype is None else f"{np.dtype(dtype).name} elements"))
        if not a.is_cuda or a.device.index != self.device:
            raise ValueError(f"{what}: tensors must live on device {self.device}")
        return a.data_ptr(), True

    def _rays(self, what, arrays, n):
        """-> (addresses, n, torch or None) of ray arrays that are all tensors, of shape (n, 3), or all DeviceBuffers; ValueError before any
        call otherwise"""
        if all(isinstance(a, hipmem.DeviceBuffer) for a in arrays):
            if n is None or int(n) < 0:
                raise ValueError(f"{what}: DeviceBuffers need an explicit n >= 0")
        else:
            if any(getattr(a, "ndim", 0) != 2 or a.shape[1] != 3 for a in arrays):
                raise ValueError(f"{what}: rays are tensors of shape (n, 3), or all hipmem.DeviceBuffers")
            if n is not None and int(n) != arrays[0].shape[0]:
                raise ValueError(f"{what}: the ray arrays differ in length")
            n = arrays[0].shape[0]
        checked = [self._device_array(what, a, int(n) * 3, np.float32) for a in arrays]
        return [p for p, _ in checked], int(n), sys.modules["torch"] if checked[0][1] else None

    def _query(self, what, torch, stream, call):
        """runs call(stream pointer) on the caller's stream (tensors: torch's current stream, see above)"""
        bracket = False
        if stream is None and torch is not None:
            cur = torch.cuda.current_stream(self.device)
            stream = cur.cuda_stream
            if not stream:
                cur.synchronize()
                bracket = True
        capi.check(self.lib, self.handle, call(C.c_void_p(stream) if stream else None), what)
        if bracket:
            capi.check(self.lib, self.handle, self.lib.rt_synchronize(self.handle), "rt_synchronize")

    def _out(self, torch, buf, n, per, dtype):
        """an output of n * per elements: the caller's DeviceBuffer, else a new tensor / DeviceBuffer -> (object, address)"""
        if buf is not None:
            addr, is_tensor = self._device_array("an output", buf, n * per, dtype)
            if is_tensor:
                raise ValueError("an output that the caller passes is a hipmem.DeviceBuffer")
            return buf, addr
        if torch is not None:
            t = torch.empty((n, per) if per > 1 else (n,), dtype=getattr(torch, np.dtype(dtype).name), device=f"cuda:{self.device}")
            return t, t.data_ptr()
        b = hipmem.DeviceBuffer(max(1, n * per * np.dtype(dtype).itemsize))
        return b, b.address

    def closest_hits(self, origins, dirs, stream=None, n=None, faces=None, ts=None, want_faces=True, want_t=True):
        """rt_closest_hits_device: per ray the closest face id (int32, -1: none) and its ray parameter t (float32, -1.0: none) -> (faces, ts);
        want_faces / want_t = False leaves that output out (None)"""
        (po, pd), n, torch = self._rays("closest_hits", (origins, dirs), n)
        f, pf = self._out(torch, faces, n, 1, np.int32) if want_faces else (None, None)
        t, pt = self._out(torch, ts, n, 1, np.float32) if want_t else (None, None)
        self._query("rt_closest_hits_device", torch, stream,
                    lambda st: self.lib.rt_closest_hits_device(self.handle, n, po, pd, pf, pt, st))
        return f, t

    def closest_points(self, points, max_dist=float("inf"), stream=None, n=None, faces=None, dist2=None, closest=None, want_faces=True,
                       want_dist2=True, want_closest=True):
        """rt_closest_points_device: per point the nearest face of the scene within `max_dist` (int32, -1: none), the squared distance to it
        (float32, +inf: none) and the nearest point on it (float32 (n, 3); the point itself: none) -> (faces, dist2, closest); want_* = False
        leaves that output out (None).  The first call after an upload builds the query's bounds and synchronises the context's stream."""
        (pp,), n, torch = self._rays("closest_points", (points,), n)
        f, pf = self._out(torch, faces, n, 1, np.int32) if want_faces else (None, None)
        d, pd = self._out(torch, dist2, n, 1, np.float32) if want_dist2 else (None, None)
        q, pq = self._out(torch, closest, n, 3, np.float32) if want_closest else (None, None)
        self._query("rt_closest_points_device", torch, stream,
                    lambda st: self.lib.rt_closest_points_device(self.handle, n, pp, float(max_dist), pf, pd, pq, st))
        return f, d, q

    def ray_hits(self, origins, dirs, k, t_max=float("inf"), n=None, stream=None, faces=None, ts=None, counts=None, want_faces=True, want_t=True,
                 want_counts=True):
        """rt_ray_hits_device: per ray its first k hits in order of (t, face id) -- faces int32 (n, k) and ts float32 (n, k), -1 / -1.0 in the
        unused slots -- and counts int32 (n,) = min(hits, k + 1), so k + 1 says "more than k" -> (faces, ts, counts); 1 <= k <= 8, hits
        beyond t_max do not count; want_* = False leaves that output out (None)"""
        (po, pd), n, torch = self._rays("ray_hits", (origins, dirs), n)
        k = int(k)
        if not 1 <= k <= capi.RT_MAX_RAY_HITS:
            raise ValueError(f"ray_hits: k must be in 1 .. {capi.RT_MAX_RAY_HITS}")
        f, pf = self._out(torch, faces, n, k, np.int32) if want_faces else (None, None)
        t, pt = self._out(torch, ts, n, k, np.float32) if want_t else (None, None)
        c, pc = self._out(torch, counts, n, 1, np.int32) if want_counts else (None, None)
        if torch is not None and k == 1:          # (n, 1), like every other k
            f, t = (None if f is None else f.view(n, 1)), (None if t is None else t.view(n, 1))
        self._query("rt_ray_hits_device", torch, stream,
                    lambda st: self.lib.rt_ray_hits_device(self.handle, n, po, pd, k, float(t_max), pf, pt, pc, st))
        return f, t, c

    def light_strikes_device(self, hits, lights, stream=None, n=None, vis=None):
        """rt_light_strikes_device: vis[i] = 1 iff the segment lights[i] -> hits[i] is visible (uint8)"""
        (ph, pl), n, torch = self._rays("light_strikes_device", (hits, lights), n)
        v, pv = self._out(torch, vis, n, 1, np.uint8)
        self._query("rt_light_strikes_device", torch, stream,
                    lambda st: self.lib.rt_light_strikes_device(self.handle, n, ph, pl, pv, st))
        return v

    def trace_rays_device(self, lights, origins, dirs, max_depth=-1, want_hits=False, stream=None, n=None, rgb=None, faces=None, ts=None):
        """rt_trace_rays_device: the colour traceRay returns per ray (float32 (n, 3)) under the rt_lights `lights`; want_hits: -> (rgb, faces, ts)"""
        (po, pd), n, torch = self._rays("trace_rays_device", (origins, dirs), n)
        c, pc = self._out(torch, rgb, n, 3, np.float32)
        f, pf = self._out(torch, faces, n, 1, np.int32) if want_hits else (None, None)
        t, pt = self._out(torch, ts, n, 1, np.float32) if want_hits else (None, None)
        self._query("rt_trace_rays_device", torch, stream,
                    lambda st: self.lib.rt_trace_rays_device(self.handle, C.byref(lights), int(max_depth), n, po, pd, pc, pf, pt, st))
        return (c, f, t) if want_hits else c

    def _per_ray(self, what, a, n, torch, dtype):
        """-> the address of a per-ray input (n elements of `dtype`) of the kind the ray arrays of the call are (`torch`: tensors)"""
        addr, is_tensor = self._device_array(what, a, n, dtype)
        if is_tensor != (torch is not None) or (is_tensor and a.dim() != 1):
            raise ValueError(f"{what}: a per-ray input is a tensor of shape (n,) or a DeviceBuffer, like the ray arrays")
        return addr

    def hit_points(self, origins, dirs, faces, ts, stream=None, n=None, points=None, normals=None):
        """rt_hit_points_device: closest hits (faces, ts of closest_hits, with their rays) -> (points, normals), float32 (n, 3): the hit point
        and the face normal turned towards the ray; six zeros for a miss -- the inputs of ambient_occlusion"""
        (po, pd), n, torch = self._rays("hit_points", (origins, dirs), n)
        pf, pt = self._per_ray("hit_points", faces, n, torch, np.int32), self._per_ray("hit_points", ts, n, torch, np.float32)
        p, pp = self._out(torch, points, n, 3, np.float32)
        nr, pn = self._out(torch, normals, n, 3, np.float32)
        self._query("rt_hit_points_device", torch, stream,
                    lambda st: self.lib.rt_hit_points_device(self.handle, n, po, pd, pf, pt, pp, pn, st))
        return p, nr

    def ambient_occlusion(self, points, normals, grid, radius, seed=0, stream=None, n=None, open=None, ao=None, want_open=True, want_ao=True):
        """rt_ambient_occlusion_device: per point the number of its grid x grid cosine-weighted segments of length `radius` that nothing
        blocks (uint16) and that number over grid x grid (float32) -> (open, ao); want_open / want_ao = False leaves that output out (None).
        A point whose normal is all zeros is fully open."""
        (pp, pn), n, torch = self._rays("ambient_occlusion", (points, normals), n)
        o, po = self._out(torch, open, n, 1, np.uint16) if want_open else (None, None)
        a, pa = self._out(torch, ao, n, 1, np.float32) if want_ao else (None, None)
        self._query("rt_ambient_occlusion_device", torch, stream,
                    lambda st: self.lib.rt_ambient_occlusion_device(self.handle, n, pp, pn, int(grid), float(radius), int(seed) & 0xFFFFFFFF, po, pa, st))
        return o, a

    def soft_shadows(self, points, normals, lights, params=None, stream=None, n=None, visible=None, share=None, want_visible=True, want_share=True):
        """rt_soft_shadows_device: per point the number of the samples of the rt_lights `lights` (point or area) that it sees (uint16) and
        that number over n_lights * usteps * vsteps (float32) -> (visible, share); want_visible / want_share = False leaves that output out
        (None).  params: an rt_shadow_params (shadow_params()), None = the samples of every frame.  normals: None = every point is a point;
        else a point whose normal is all zeros (a miss of hit_points) sees every sample."""
        arrays = (points,) if normals is None else (points, normals)
        ptrs, n, torch = self._rays("soft_shadows", arrays, n)
        pp, pn = ptrs[0], (None if normals is None else ptrs[1])
        sp = shadow_params() if params is None else params
        v, pv = self._out(torch, visible, n, 1, np.uint16) if want_visible else (None, None)
        sh, ps = self._out(torch, share, n, 1, np.float32) if want_share else (None, None)
        self._query("rt_soft_shadows_device", torch, stream,
                    lambda st: self.lib.rt_soft_shadows_device(self.handle, C.byref(lights), n, pp, pn, C.byref(sp), pv, ps, st))
        return v, sh

    def _source(self, what, source, torch):
        """-> (rt_probe_grid, address of its coefficients) of a source=(pgrid, coeff) argument: coeff float32 (probes, 27), a tensor or a
        DeviceBuffer as the other arrays of the call are"""
        pgrid, coeff = source
        cells = int(pgrid.dims[0]) * int(pgrid.dims[1]) * int(pgrid.dims[2])
        pc, is_tensor = self._device_array(what, coeff, max(0, cells) * capi.RT_PROBE_COEFFS, np.float32)
        if is_tensor != (torch is not None):
            raise ValueError(f"{what}: the source's coefficients and the other arrays are all tensors or all hipmem.DeviceBuffers")
        return pgrid, pc

    def indirect_diffuse(self, points, normals, lights, grid, seed=0, stream=None, n=None, out=None, source=None, visible=False):
        """rt_indirect_diffuse_device: per point the mean radiance (float32 (n, 3)) that its grid x grid cosine-weighted gather rays bring
        back from their closest hits, each lit (diffuse term) by the positions of the rt_lights `lights` it sees; a Lambert surface at the
        point sends back its own kd times that.  A point whose normal is all zeros (a miss of hit_points) gives zeros.
        source=(pgrid, coeff): rt_indirect_diffuse_bounce_device -- every hit is lit, in addition, by the probe volume `coeff` of the
        rt_probe_grid `pgrid` looked up at the hit (a volume computed WITHOUT the direct term); visible: by the leak-free lookup."""
        (pp, pn), n, torch = self._rays("indirect_diffuse", (points, normals), n)
        o, po = self._out(torch, out, n, 3, np.float32)
        if source is None:
            self._query("rt_indirect_diffuse_device", torch, stream,
                        lambda st: self.lib.rt_indirect_diffuse_device(self.handle, C.byref(lights), n, pp, pn, int(grid), int(seed) & 0xFFFFFFFF, po, st))
            return o
        pgrid, pc = self._source("indirect_diffuse", source, torch)
        self._query("rt_indirect_diffuse_bounce_device", torch, stream,
                    lambda st: self.lib.rt_indirect_diffuse_bounce_device(self.handle, C.byref(lights), n, pp, pn, int(grid), int(seed) & 0xFFFFFFFF,
                                                                          C.byref(pgrid), pc, 1 if visible else 0, po, st))
        return o

    def light_probes(self, positions, lights, grid, direct=False, stream=None, n=None, out=None, source=None, visible=False):
        """rt_light_probes_device: per probe position the 9 spherical-harmonic coefficients per channel (float32 (n, 27), coefficient j of
        channel c at j * 3 + c) of the light that grid x grid rays over the whole sphere bring back from their closest hits, each lit (diffuse
        term) by the positions of the rt_lights `lights` it sees, already convolved with the clamped cosine and divided by pi; direct: the
        lights the probe itself sees are added as deltas.
        source=(pgrid, coeff): rt_light_probes_bounce_device -- every hit is lit, in addition, by the probe volume `coeff` of the
        rt_probe_grid `pgrid` looked up at the hit (a volume computed WITHOUT the direct term; not the output array); visible: by the
        leak-free lookup.  Feeding the previous volume of the same grid back adds one bounce per call."""
        (pp,), n, torch = self._rays("light_probes", (positions,), n)
        o, po = self._out(torch, out, n, capi.RT_PROBE_COEFFS, np.float32)
        if source is None:
            self._query("rt_light_probes_device", torch, stream,
                        lambda st: self.lib.rt_light_probes_device(self.handle, C.byref(lights), n, pp, int(grid), 1 if direct else 0, po, st))
            return o
        pgrid, pc = self._source("light_probes", source, torch)
        self._query("rt_light_probes_bounce_device", torch, stream,
                    lambda st: self.lib.rt_light_probes_bounce_device(self.handle, C.byref(lights), n, pp, int(grid), 1 if direct else 0, C.byref(pgrid), pc,
                                                                      1 if visible else 0, po, st))
        return o

    def probe_irradiance(self, pgrid, coeff, points, normals, stream=None, n=None, out=None):
        """rt_probe_irradiance_device: per point the trilinear blend of the probes of the rt_probe_grid `pgrid` round it (coeff: their
        coefficients, float32 (probes, 27), a tensor or a DeviceBuffer as the points are) evaluated at the point's normal -> float32 (n, 3);
        a Lambert surface sends back its own kd times that.  A normal of three zeros gives zeros."""
        (pp, pn), n, torch = self._rays("probe_irradiance", (points, normals), n)
        cells = int(pgrid.dims[0]) * int(pgrid.dims[1]) * int(pgrid.dims[2])
        pc, coeff_is_tensor = self._device_array("probe_irradiance", coeff, max(0, cells) * capi.RT_PROBE_COEFFS, np.float32)
        if coeff_is_tensor != (torch is not None):
            raise ValueError("probe_irradiance: coeff, points and normals are all tensors or all hipmem.DeviceBuffers")
        o, po = self._out(torch, out, n, 3, np.float32)
        self._query("rt_probe_irradiance_device", torch, stream,
                    lambda st: self.lib.rt_probe_irradiance_device(self.handle, C.byref(pgrid), pc, n, pp, pn, po, st))
        return o

    def probe_irradiance_visible(self, pgrid, coeff, points, normals, stream=None, n=None, out=None, mask=None, want_mask=True):
        """rt_probe_irradiance_visible_device: probe_irradiance over the probes each point can see -- every probe round a point is asked with
        one segment walk through the uploaded scene, the blend takes the visible ones and is renormalised; where all are visible (or none
        is) it is the plain blend bit for bit -> (float32 (n, 3), uint8 (n,): bit b = corner b = 4 dz + 2 dy + dx is visible); want_mask =
        False leaves the mask out (None)."""
        (pp, pn), n, torch = self._rays("probe_irradiance_visible", (points, normals), n)
        cells = int(pgrid.dims[0]) * int(pgrid.dims[1]) * int(pgrid.dims[2])
        pc, coeff_is_tensor = self._device_array("probe_irradiance_visible", coeff, max(0, cells) * capi.RT_PROBE_COEFFS, np.float32)
        if coeff_is_tensor != (torch is not None):
            raise ValueError("probe_irradiance_visible: coeff, points and normals are all tensors or all hipmem.DeviceBuffers")
        o, po = self._out(torch, out, n, 3, np.float32)
        k, pk = self._out(torch, mask, n, 1, np.uint8) if want_mask else (None, None)
        self._query("rt_probe_irradiance_visible_device", torch, stream,
                    lambda st: self.lib.rt_probe_irradiance_visible_device(self.handle, C.byref(pgrid), pc, n, pp, pn, po, pk, st))
        return o, k

    def gbuffer(self, cam, width, height, rows=None, out=None, stream=None):
        """rt_gbuffer_device: the geometry buffers (coverage, depth, face normal, diffuse colour: capi.RT_GBUFFER_CHANNELS floats per pixel) of
        the frame a render call on this context would render with the rt_camera `cam` at width x height, under the context's sample settings
        (supersampling, lens, shutter, passes).  rows: None = the whole frame, (row0, row1) = that row range, or an rt_params (its width,
        height and row shard are used).  out: None = a new float32 torch tensor of shape (local rows, width, 8) on this context's device;
        a contiguous float32 tensor of that many elements or a hipmem.DeviceBuffer of that many bytes is filled and returned.  Streams as
        for closest_hits: tensors run on torch's current stream, DeviceBuffers on `stream` (None = the context's)."""
        if isinstance(rows, capi.rt_params):
            p = rows
        else:
            r0, r1 = (0, int(height)) if rows is None else (int(rows[0]), int(rows[1]))
            p = make_params(width, height, row0=r0, row1=r1)
        n = int(self.lib.rt_local_rows(C.byref(p)))
        shape = (n, int(p.width), capi.RT_GBUFFER_CHANNELS)
        floats = n * max(int(p.width), 0) * capi.RT_GBUFFER_CHANNELS
        torch = None
        if not isinstance(out, hipmem.DeviceBuffer):
            import torch
            if out is None:
                out = torch.empty(shape, dtype=torch.float32, device=f"cuda:{self.device}")
        addr, _ = self._device_array("gbuffer: out", out, floats, np.float32)
        self._query("rt_gbuffer_device", torch, stream,
                    lambda st: self.lib.rt_gbuffer_device(self.handle, C.byref(cam), C.byref(p), C.c_void_p(addr), st))
        return out

    def denoise(self, image, gbuffer, width, rows, params=None, out=None, scratch=None, stream=None, channels=None):
        """rt_denoise_device: the edge-avoiding a-trous filter of a width x rows image of 1 or 3 floats per pixel, guided by the geometry
        buffers of the same frame (what gbuffer returns for the same rows).  image, gbuffer: float32 torch tensors on this context's device
        (contiguous, rows * width * channels and rows * width * 8 elements) or hipmem.DeviceBuffers (then `channels` says which, unless the
        buffer's size does).  params: an rt_denoise_params (denoise_params()), None = rt_default_denoise_params.  out: None = a new tensor
        shaped like `image` / a new DeviceBuffer; else filled and returned (16-byte aligned, apart from the inputs).  scratch: working
        memory of rt_denoise_scratch_bytes bytes, a uint8 tensor or a DeviceBuffer; None = allocated here (on DeviceBuffers the call then
        waits for the device before it frees it).  Streams as for closest_hits."""
        width, rows = int(width), int(rows)
        px = max(width, 0) * max(rows, 0)
        if params is None:
            params = denoise_params()
        own_scratch = None
        if channels is None:
            size = image.nbytes if isinstance(image, hipmem.DeviceBuffer) else 4 * image.numel() if hasattr(image, "numel") else -1
            channels = {px * 4: 1, px * 12: 3}.get(size) if px else 1
        if channels not in (1, 3):
            raise ValueError("denoise: image must hold rows * width * (1 or 3) floats (DeviceBuffers of another size need channels = 1 or 3)")
        p_in, tensors = self._device_array("denoise: image", image, px * channels, np.float32)
        p_gb, t_gb = self._device_array("denoise: gbuffer", gbuffer, px * capi.RT_GBUFFER_CHANNELS, np.float32)
        need = int(self.lib.rt_denoise_scratch_bytes(width, rows, channels))
        torch = None
        if tensors:
            import torch
        if out is None:
            out = torch.empty_like(image) if tensors else hipmem.DeviceBuffer(max(16, px * channels * 4))
        p_out, t_out = self._device_array("denoise: out", out, px * channels, np.float32)
        kinds = "denoise: image, gbuffer, out and scratch are all torch tensors or all hipmem.DeviceBuffers"
        if t_gb != tensors or t_out != tensors:
            raise ValueError(kinds)
        if scratch is None:
            scratch = torch.empty((max(16, need),), dtype=torch.uint8, device=f"cuda:{self.device}") if tensors else hipmem.DeviceBuffer(max(16, need))
            own_scratch = None if tensors else scratch
        p_scr, t_scr = self._device_array("denoise: scratch", scratch, need)
        if t_scr != tensors:
            raise ValueError(kinds)
        try:
            self._query("rt_denoise_device", torch, stream,
                        lambda st: self.lib.rt_denoise_device(self.handle, C.c_void_p(p_in), channels, C.c_void_p(p_gb), width, rows, C.byref(params),
                                                              C.c_void_p(p_scr), C.c_void_p(p_out), st))
        finally:
            if own_scratch is not None:
                hipmem.synchronize()
                own_scratch.free()
        return out

    def upsample(self, low, gb_low, gb_high, width, rows, params=None, out=None, miss=None, stream=None, channels=None):
        """rt_upsample_device: the guided upsample of a low image of ceil(width / s) x ceil(rows / s) pixels of 1 or 3 floats to width x
        rows, steered by the geometry buffers of the low and of the high frame (what gbuffer returns for them).  low, gb_low, gb_high:
        float32 torch tensors on this context's device (contiguous) or hipmem.DeviceBuffers (then `channels` says which, unless the
        buffer's size does).  params: an rt_upsample_params (upsample_params()), None = rt_default_upsample_params.  out: None = a new
        tensor of shape (rows, width[, 3]) / a new DeviceBuffer; else filled and returned (16-byte aligned, apart from the inputs).  miss:
        None = no mask; True = a new uint8 tensor of shape (rows, width) / DeviceBuffer; else filled; with a mask the call returns
        (out, miss).  Streams as for closest_hits."""
        width, rows = int(width), int(rows)
        if params is None:
            params = upsample_params()
        w, r = C.c_int32(0), C.c_int32(0)
        if self.lib.rt_upsample_low_size(width, rows, params.factor, C.byref(w), C.byref(r)) != capi.RT_OK:
            raise ValueError("upsample: width >= 1, rows >= 0 and a factor in 2 .. RT_UPSAMPLE_MAX_FACTOR")
        px, lpx = width * rows, w.value * r.value
        if channels is None:
            size = low.nbytes if isinstance(low, hipmem.DeviceBuffer) else 4 * low.numel() if hasattr(low, "numel") else -1
            channels = {lpx * 4: 1, lpx * 12: 3}.get(size) if lpx else 1
        if channels not in (1, 3):
            raise ValueError("upsample: low must hold r * w * (1 or 3) floats (DeviceBuffers of another size need channels = 1 or 3)")
        p_low, tensors = self._device_array("upsample: low", low, lpx * channels, np.float32)
        p_gl, t_gl = self._device_array("upsample: gb_low", gb_low, lpx * capi.RT_GBUFFER_CHANNELS, np.float32)
        p_gh, t_gh = self._device_array("upsample: gb_high", gb_high, px * capi.RT_GBUFFER_CHANNELS, np.float32)
        torch = None
        if tensors:
            import torch
        dev = f"cuda:{self.device}"
        if out is None:
            out = torch.empty((rows, width, 3) if channels == 3 else (rows, width), dtype=torch.float32, device=dev) if tensors \
                else hipmem.DeviceBuffer(max(16, px * channels * 4))
        if miss is True:
            miss = torch.empty((rows, width), dtype=torch.uint8, device=dev) if tensors else hipmem.DeviceBuffer(max(16, px))
        p_out, t_out = self._device_array("upsample: out", out, px * channels, np.float32)
        p_miss, t_miss = self._device_array("upsample: miss", miss, px, np.uint8) if miss is not None else (None, tensors)
        if not (t_gl == t_gh == t_out == t_miss == tensors):
            raise ValueError("upsample: low, gb_low, gb_high, out and miss are all torch tensors or all hipmem.DeviceBuffers")
        self._query("rt_upsample_device", torch, stream,
                    lambda st: self.lib.rt_upsample_device(self.handle, C.c_void_p(p_low), channels, C.c_void_p(p_gl), C.c_void_p(p_gh), width, rows,
                                                           C.byref(params), C.c_void_p(p_out), C.c_void_p(p_miss) if p_miss else None, st))
        return out if miss is None else (out, miss)

    def reproject(self, cur, gb_cur, hist, gb_hist, len_hist, width, rows, m, params=None, out=None, len_out=None, stream=None, channels=None):
        """rt_reproject_device: the accumulated image `hist` of the previous frame (with its lengths `len_hist`, uint8 per pixel, 0 = no
        history) carried into the current frame `cur` through the geometry buffers of both frames and the map `m` (reproject_map(cur camera,
        previous camera): 12 floats), blended as a running mean -> (out, len_out).  cur, gb_cur, hist, gb_hist: float32 torch tensors on
        this context's device (contiguous) or hipmem.DeviceBuffers (then `channels` says 1 or 3, unless the buffer's size does); len_hist
        a uint8 tensor / DeviceBuffer.  params: an rt_reproject_params (reproject_params()), None = rt_default_reproject_params.  out,
        len_out: None = new tensors shaped like cur and (rows, width) / new DeviceBuffers; else filled and returned (out 16-byte aligned,
        both apart from every input: ping-pong two sets).  Streams as for closest_hits."""
        width, rows = int(width), int(rows)
        if params is None:
            params = reproject_params()
        px = max(width, 0) * max(rows, 0)
        if channels is None:
            size = cur.nbytes if isinstance(cur, hipmem.DeviceBuffer) else 4 * cur.numel() if hasattr(cur, "numel") else -1
            channels = {px * 4: 1, px * 12: 3}.get(size) if px else 1
        if channels not in (1, 3):
            raise ValueError("reproject: cur must hold rows * width * (1 or 3) floats (DeviceBuffers of another size need channels = 1 or 3)")
        mm = (C.c_float * 12)(*[float(v) for v in np.asarray(m, np.float32).reshape(12)])
        p_cur, tensors = self._device_array("reproject: cur", cur, px * channels, np.float32)
        p_gc, t_gc = self._device_array("reproject: gb_cur", gb_cur, px * capi.RT_GBUFFER_CHANNELS, np.float32)
        p_hist, t_hist = self._device_array("reproject: hist", hist, px * channels, np.float32)
        p_gh, t_gh = self._device_array("reproject: gb_hist", gb_hist, px * capi.RT_GBUFFER_CHANNELS, np.float32)
        p_lh, t_lh = self._device_array("reproject: len_hist", len_hist, px, np.uint8)
        torch = None
        if tensors:
            import torch
        dev = f"cuda:{self.device}"
        if out is None:
            out = torch.empty((rows, width, 3) if channels == 3 else (rows, width), dtype=torch.float32, device=dev) if tensors \
                else hipmem.DeviceBuffer(max(16, px * channels * 4))
        if len_out is None:
            len_out = torch.empty((rows, width), dtype=torch.uint8, device=dev) if tensors else hipmem.DeviceBuffer(max(16, px))
        p_out, t_out = self._device_array("reproject: out", out, px * channels, np.float32)
        p_lo, t_lo = self._device_array("reproject: len_out", len_out, px, np.uint8)
        if not (t_gc == t_hist == t_gh == t_lh == t_out == t_lo == tensors):
            raise ValueError("reproject: the images, the buffers and the lengths are all torch tensors or all hipmem.DeviceBuffers")
        self._query("rt_reproject_device", torch, stream,
                    lambda st: self.lib.rt_reproject_device(self.handle, C.c_void_p(p_cur), channels, C.c_void_p(p_gc), C.c_void_p(p_hist), C.c_void_p(p_gh),
                                                            C.c_void_p(p_lh), width, rows, mm, C.byref(params), C.c_void_p(p_out), C.c_void_p(p_lo), st))
        return out, len_out

    def set_query_chunk(self, rays):
        """rt_set_query_chunk: rays per launch sequence of later trace_rays_device calls (64 .. 2^24, default 2^22)"""
        capi.check(self.lib, self.handle, self.lib.rt_set_query_chunk(self.handle, int(rays)), "rt_set_query_chunk")

    def synchronize(self):
        """rt_synchronize: waits for the frames and ray queries enqueued on the context's working set"""
        capi.check(self.lib, self.handle, self.lib.rt_synchronize(self.handle), "rt_synchronize")

    def close(self):
        if self.handle:
            self.lib.rt_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_params(width, height, max_depth=-1, row0=0, row1=None, stripe=1, rank=0, nranks=1, collect_stats=False):
    p = capi.rt_params()
    p.width, p.height, p.max_depth = int(width), int(height), int(max_depth)
    p.row0, p.row1 = int(row0), int(height if row1 is None else row1)
    p.stripe, p.rank, p.nranks = int(stripe), int(rank), int(nranks)
    p.collect_stats = 1 if collect_stats else 0
    return p


def denoise_params(iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None):
    """an rt_denoise_params: rt_default_denoise_params with the given fields replaced (float("inf") = that guide never stops a tap)"""
    lib = capi.load_library()
    p = capi.rt_denoise_params()
    lib.rt_default_denoise_params(C.byref(p))
    if iterations is not None:
        p.iterations = int(iterations)
    for name, v in (("sigma_color", sigma_color), ("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth), ("sigma_albedo", sigma_albedo)):
        if v is not None:
            setattr(p, name, float(v))
    return p


def upsample_params(factor=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None):
    """an rt_upsample_params: rt_default_upsample_params with the given fields replaced (float("inf") = that guide never stops a tap)"""
    lib = capi.load_library()
    p = capi.rt_upsample_params()
    lib.rt_default_upsample_params(C.byref(p))
    if factor is not None:
        p.factor = int(factor)
    for name, v in (("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth), ("sigma_albedo", sigma_albedo)):
        if v is not None:
            setattr(p, name, float(v))
    return p


def reproject_params(max_history=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None):
    """an rt_reproject_params: rt_default_reproject_params with the given fields replaced (float("inf") = that guide never stops a tap)"""
    lib = capi.load_library()
    p = capi.rt_reproject_params()
    lib.rt_default_reproject_params(C.byref(p))
    if max_history is not None:
        p.max_history = int(max_history)
    for name, v in (("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth), ("sigma_albedo", sigma_albedo)):
        if v is not None:
            setattr(p, name, float(v))
    return p


def shadow_params(per_point=None, seed=None, fu=None, fv=None):
    """an rt_shadow_params: rt_default_shadow_params (the samples of every frame) with the given fields replaced"""
    lib = capi.load_library()
    p = capi.rt_shadow_params()
    lib.rt_default_shadow_params(C.byref(p))
    if per_point is not None:
        p.per_point = 1 if per_point else 0
    if seed is not None:
        p.seed = int(seed) & 0xFFFFFFFF
    for name, v in (("fu", fu), ("fv", fv)):
        if v is not None:
            setattr(p, name, float(v))
    return p


def shadow_jitter(seed, i):
    """rt_shadow_jitter (host only): the offsets (fu, fv), two float32 in [0, 1), of point i of a per-point soft-shadow call with `seed`"""
    lib = capi.load_library()
    fu, fv = C.c_float(), C.c_float()
    capi.check(lib, None, lib.rt_shadow_jitter(int(seed) & 0xFFFFFFFF, int(i) & 0xFFFFFFFF, C.byref(fu), C.byref(fv)), "rt_shadow_jitter")
    return np.float32(fu.value), np.float32(fv.value)


def light_samples(lights, light, fu, fv):
    """rt_light_samples (host only): the samples of light `light` of the rt_lights `lights` with the offsets (fu, fv) -> float32 (N, 3),
    N = usteps * vsteps of an area light (sample (i, j) at i * vsteps + j), 1 of a point light.  ValueError where the call refuses the
    lights or the index; sphere lights are not supported."""
    lib = capi.load_library()
    n = int(lights.usteps) * int(lights.vsteps) if lights.mode == capi.RT_LIGHT_AREA else 1
    out = np.empty((max(n, 1), 3), np.float32)
    s = lib.rt_light_samples(C.byref(lights), int(light), float(fu), float(fv), _fptr(out)) if 1 <= n <= 1024 else capi.RT_ERR_INVALID
    if s != capi.RT_OK:
        raise ValueError(f"light_samples: rt_light_samples refused the lights or the light index (status {s})")
    return out


def reproject_map(cur, prev):
    """rt_reproject_map: the 12 floats (rows x, y, depth; columns E, U, V, W) of the map that sends a raster point and ray parameter of the
    rt_camera `cur` to the raster point and ray parameter of `prev` -> float32 (3, 4); equal cameras give the identity.  ValueError for
    cameras the call refuses (a non-finite field, a zero viewport size, a singular previous inv_view)."""
    lib = capi.load_library()
    m = (C.c_float * 12)()
    if lib.rt_reproject_map(C.byref(cur), C.byref(prev), m) != capi.RT_OK:
        raise ValueError("reproject_map: a camera field is not finite, a viewport size is zero or the previous inv_view is singular")
    return np.array(list(m), np.float32).reshape(3, 4)


def low_camera(cam, factor):
    """the camera of the low frame of an upsample by `factor`: `cam` with viewport[2] and viewport[3] each divided by (float)factor (one
    float32 division each) and cam's own aspect -> (camera, w, r).  Low pixel (I, J) is then pixel (factor * I, factor * J) of cam's frame,
    ray for ray; where factor divides both sizes the camera is default_camera(w, r) with cam's pose, in every bit."""
    lib = capi.load_library()
    width, rows = int(cam.viewport[2]), int(cam.viewport[3])
    w, r = C.c_int32(0), C.c_int32(0)
    capi.check(lib, None, lib.rt_upsample_low_size(width, rows, int(factor), C.byref(w), C.byref(r)), "rt_upsample_low_size")
    low = capi.rt_camera()
    C.memmove(C.byref(low), C.byref(cam), C.sizeof(low))
    low.viewport[2] = float(np.float32(cam.viewport[2]) / np.float32(factor))
    low.viewport[3] = float(np.float32(cam.viewport[3]) / np.float32(factor))
    return low, w.value, r.value


def probe_grid(origin, step, dims):
    """-> rt_probe_grid: dims[0] x dims[1] x dims[2] probes, probe (ix, iy, iz) at origin + (ix, iy, iz) * step"""
    g = capi.rt_probe_grid()
    for q in range(3):
        g.origin[q], g.step[q], g.dims[q] = float(origin[q]), float(step[q]), int(dims[q])
    return g


def probe_grid_over(box, dims, margin=0.0):
    """-> rt_probe_grid whose outermost probes lie on the box (min xyz, max xyz) grown by `margin` on every side, in float32: lo = min -
    margin, hi = max + margin, origin = lo, step = (hi - lo) / (float)(dims - 1); an axis of one probe has it at (lo + hi) * 0.5f with step
    1 (Flyscene::lightProbes of the C++ facade forms the same floats)"""
    F = np.float32
    b, mg = np.asarray(box, F).reshape(6), F(margin)
    origin, step = [], []
    for q in range(3):
        lo, hi = b[q] - mg, b[3 + q] + mg
        one = int(dims[q]) <= 1
        origin.append((lo + hi) * F(0.5) if one else lo)
        step.append(F(1.0) if one else (hi - lo) / F(int(dims[q]) - 1))
    return probe_grid(origin, step, dims)


def thickness_of(ts, counts):
    """the thickness rule of Flyscene.thickness on ray_hits results of k = RT_MAX_RAY_HITS: ts (n, 8), counts (n,) -> float32 (n,)"""
    ts, counts = np.asarray(ts, np.float32), np.asarray(counts)
    pairs = np.minimum(counts, capi.RT_MAX_RAY_HITS) // 2
    total = np.zeros(len(counts), np.float32)
    for j in range(capi.RT_MAX_RAY_HITS // 2):
        total = np.where(j < pairs, total + (ts[:, 2 * j + 1] - ts[:, 2 * j]), total).astype(np.float32)
    return total


def parity_of(counts):
    """the side rule of Flyscene.inside on ray_hits counts of k = RT_MAX_RAY_HITS -> int8: 1 odd, 0 even, -1 more than 8"""
    counts = np.asarray(counts)
    return np.where(counts > capi.RT_MAX_RAY_HITS, -1, counts & 1).astype(np.int8)


def probe_grid_positions(pgrid):
    """rt_probe_grid_positions -> float32 (probes, 3)"""
    lib = capi.load_library()
    out = np.empty((max(0, int(pgrid.dims[0]) * int(pgrid.dims[1]) * int(pgrid.dims[2])), 3), np.float32)
    capi.check(lib, None, lib.rt_probe_grid_positions(C.byref(pgrid), _fptr(out)), "rt_probe_grid_positions")
    return out


def make_lights(points=((-1.0, 1.0, 1.0),), area=True, usteps=5, vsteps=5):
    lib = capi.load_library()
    l = capi.rt_lights()
    lib.rt_default_lights(C.byref(l), 1 if area else 0)
    l.n_lights = len(points)
    for i, p in enumerate(points):
        for k in range(3):
            l.pos[i][k] = float(p[k])
    l.usteps, l.vsteps = int(usteps), int(vsteps)
    return l


def primary_rect(cam, box, width, height, supersampling=1, aperture=0.0, shutter=False, passes=(0, 1)):
    """rt_debug_primary_rect (host only): the tiles (tx0, ty0, tx1, ty1) a frame of `cam` over a scene with root box `box` (min, max) keeps"""
    lib = capi.load_library()
    b = (C.c_float * 6)(*[float(x) for x in box])
    out = (C.c_int32 * 4)()
    capi.check(lib, None, lib.rt_debug_primary_rect(C.byref(cam), b, int(width), int(height), int(supersampling), float(aperture),
                                                    1 if shutter else 0, int(passes[0]), int(passes[1]), out), "rt_debug_primary_rect")
    return tuple(int(x) for x in out)


def sphere_offsets(seed, radius=1.0, n=25):
    """rt_sphere_offsets: createSpherePoint's sphere loop (flyscene.cpp:976-993) with std::random_device replaced by mt19937(seed + i)"""
    lib = capi.load_library()
    out = np.zeros((int(n), 3), np.float32)
    lib.rt_sphere_offsets(int(seed) & 0xFFFFFFFF, float(radius), int(n), out.ctypes.data_as(C.c_void_p))
    return out


def set_sphere(lights, offsets):
    """switch an rt_lights to RT_LIGHT_SPHERE with the given [n, 3] float32 offsets (kept alive on the struct)"""
    off = np.ascontiguousarray(offsets, np.float32)
    lights._offsets_keepalive = off
    lights.mode = capi.RT_LIGHT_SPHERE
    lights.n_offsets = off.shape[0]
    lights.offsets = off.ctypes.data_as(C.POINTER(C.c_float))
    return lights


def default_camera(width, height, yaw=0.0):
    lib = capi.load_library()
    cam = capi.rt_camera()
    if yaw:
        lib.rt_yaw_camera(C.byref(cam), int(width), int(height), float(yaw))
    else:
        lib.rt_default_camera(C.byref(cam), int(width), int(height))
    return cam


class Flyscene:
    """Drop-in shaped like the reference's Flyscene for initialize() -> raytraceScene() -> result.ppm."""

    def __init__(self, scene_path="resources/models/cube.obj", device=0):
        self.scene_path = scene_path
        self.device = device
        self.areaLight, self.pointLight = True, False
        self.sphere_seed, self.sphere_offsets = 65, None
        self.usteps = self.vsteps = 5
        self.max_depth = -1
        self.supersample = 1          # n x n sub-samples per pixel in raytraceScene (rt_set_supersampling); 1 = the reference's one ray
        self.supersample_threshold = -1.0   # rt_set_supersampling_threshold: < 0 = every pixel refined (the regular n x n frame)
        self.aperture = 0.0           # rt_set_lens: lens radius in world units; 0 = the reference's pinhole camera
        self.focus = 2.0              # ... depth of the plane in focus (the default camera sits 2 in front of the normalised model's centre)
        self.shutter_close = None     # rt_set_shutter: the camera at shutter close (self.camera is the one at shutter open); None = off
        self.passes = 1               # rt_set_passes(0, passes): the frame is the mean of that many jittered, reseeded passes; 1 = the single frame
        self.pass_tolerance = -1.0    # rt_set_pass_tolerance: a pixel stops once its mean's standard error is within this; < 0 = off
        self.pass_min = 8             # ... and not before it has taken this many passes
        self.upsample = None          # an rt_upsample_params (upsample_params()): raytraceScene renders the frame at 1/factor of the size and brings it to
        #                               full size with rt_upsample_device, steered by the geometry buffers of both sizes; None = off
        self.denoise = None           # an rt_denoise_params (denoise_params()): raytraceScene filters its float frame with rt_denoise_device; None = off
        self.temporal = None          # an rt_reproject_params (reproject_params()): successive raytraceScene calls of one size keep history -- the previous
        #                               camera, buffers, accumulated image and lengths -- and blend it in with rt_reproject_device; None = off
        self._history = None          # that history: see _temporal_step / reset_history
        self.lights = [(-1.0, 1.0, 1.0)]
        self.output_path = "result.ppm"
        self.ctx = None
        self.scene = None
        self.stats = capi.rt_stats()
        self.image = None

    # reference: flyscene.cpp:29-126 (stdin switches become arguments)
    def initialize(self, width, height, areaLight=True, pointLight=False):
        self.reset_history()          # the history of `temporal` belongs to the scene that is replaced here
        self.areaLight, self.pointLight = bool(areaLight), bool(pointLight)
        if not self.areaLight and not self.pointLight:
            # spherical mode (flyscene.cpp:974-995): 25 offsets drawn once from the seeded restatement of the reference's loop
            self.sphere_offsets = sphere_offsets(self.sphere_seed, 1.0, 25)
        self.width, self.height = int(width), int(height)
        self.camera = default_camera(width, height)
        self.scene = HostScene(self.scene_path, 1000, 15)
        self.ctx = Context(self.device)
        self.ctx.upload(self.scene)

    def _lights(self, points=None):
        l = make_lights(points if points is not None else self.lights, area=(self.areaLight and not self.pointLight),
                        usteps=self.usteps, vsteps=self.vsteps)
        if not self.areaLight and not self.pointLight:
            set_sphere(l, self.sphere_offsets)
        return l

    # reference: flyscene.cpp:519-648
    def raytraceScene(self, width=0, height=0, write_ppm=True, want_hits=False, collect_stats=False):
        t0 = time.time()
        if width == 0 or height == 0:
            width, height = self.width, self.height
        if want_hits and self.supersample > 1:
            raise ValueError("raytraceScene: hit ids are per pixel; they do not exist with supersample > 1")
        if want_hits and self.passes > 1:
            raise ValueError("raytraceScene: hit ids are per ray; they do not exist with passes > 1")
        if want_hits and self.upsample is not None:
            raise ValueError("raytraceScene: hit ids are per traced pixel; they do not exist for an upsampled frame")
        if self.temporal is not None and self.upsample is not None:
            raise ValueError("raytraceScene: temporal together with upsample is not supported")
        if want_hits and self.temporal is not None:
            raise ValueError("raytraceScene: hit ids are per traced frame; they do not exist for an accumulated frame")
        cam = self._frame_settings(width, height)
        if self.temporal is not None:
            return self._raytrace_temporal(cam, width, height, write_ppm, collect_stats, t0)
        if self.upsample is not None:
            return self._raytrace_upsampled(cam, width, height, write_ppm, collect_stats, t0)
        p = make_params(width, height, self.max_depth, collect_stats=collect_stats)
        L = self._lights()
        rgb = np.empty((height, width, 3), np.float32)
        hits = np.empty((height, width), np.int32) if want_hits else None
        lib = self.ctx.lib
        capi.check(lib, self.ctx.handle,
                   lib.rt_render(self.ctx.handle, C.byref(cam), C.byref(L), C.byref(p), _fptr(rgb),
                                 _fptr(hits) if want_hits else None, C.byref(self.stats)), "rt_render")
        if self.denoise is not None:
            rgb = self._denoised(rgb, cam, width, height, self.denoise)
        self.image, self.hits = rgb, hits
        if write_ppm:
            capi.check(lib, None, lib.rt_write_ppm(self.output_path.encode(), _fptr(rgb), width, height), "rt_write_ppm")
        self.elapsed = time.time() - t0
        return rgb

    # no reference member: the frame at 1/factor of the size (the low camera), denoised there if asked, then rt_upsample_device
    def _raytrace_upsampled(self, cam, width, height, write_ppm, collect_stats, t0):
        from . import hipmem
        up, lib, ctx = self.upsample, self.ctx.lib, self.ctx
        lcam, w, r = low_camera(cam, up.factor)
        low = np.empty((r, w, 3), np.float32)
        p = make_params(w, r, self.max_depth, collect_stats=collect_stats)
        L = self._lights()
        capi.check(lib, ctx.handle, lib.rt_render(ctx.handle, C.byref(lcam), C.byref(L), C.byref(p), _fptr(low), None, C.byref(self.stats)), "rt_render")
        bufs = []
        try:
            # every buffer first, then one wait: a DeviceBuffer is zeroed on the null stream, which the context's stream does not wait for
            for nbytes in (low.nbytes, w * r * capi.RT_GBUFFER_CHANNELS * 4, width * height * capi.RT_GBUFFER_CHANNELS * 4, low.nbytes, width * height * 12):
                bufs.append(hipmem.DeviceBuffer(nbytes))
            src, g_low, g_high, filtered, out = bufs
            src.from_numpy(low)
            hipmem.synchronize()
            ctx.gbuffer(lcam, w, r, out=g_low)
            ctx.gbuffer(cam, width, height, out=g_high)
            if self.denoise is not None:
                ctx.denoise(src, g_low, w, r, self.denoise, out=filtered, channels=3)
                src = filtered
            ctx.upsample(src, g_low, g_high, width, height, up, out=out, channels=3)
            ctx.synchronize()
            rgb = out.to_numpy(np.float32, (height, width, 3))
        finally:
            for b in bufs:
                b.free()
        self.image, self.hits = rgb, None
        if write_ppm:
            capi.check(lib, None, lib.rt_write_ppm(self.output_path.encode(), _fptr(rgb), width, height), "rt_write_ppm")
        self.elapsed = time.time() - t0
        return rgb

    # no reference member: temporal reuse along a camera path (rt_reproject_device; DESIGN.md §5, Temporal reprojection)
    def reset_history(self):
        """drops the history of `temporal`: the next frame is itself, with every length 1"""
        h, self._history = self._history, None
        if h is not None:
            for s in h["sets"]:
                for b in s:
                    b.free()

    def _temporal_frame_index(self, kind, width, height):
        """the index of the coming frame in its history: 0 where there is none for this kind and size (another size or kind drops it)"""
        h = self._history
        if h is not None and h["key"] != (kind, width, height):
            self.reset_history()
            h = None
        return 0 if h is None else h["frames"]

    def _temporal_step(self, kind, cam, width, height, channels, cur, params):
        """cur: float32 (height, width[, 3]) or a DeviceBuffer holding it, the current frame of `cam`, whose geometry buffers are taken here under the context's sample
        settings -> (accumulated image as a DeviceBuffer that stays valid until the next step, the buffers of `cam`); stores both, the
        lengths and the camera as the history of the next step, in two ping-pong sets of (image, buffers, lengths)"""
        from . import hipmem
        ctx, px = self.ctx, width * height
        h = self._history
        if h is None:
            sizes = (max(16, px * channels * 4), max(16, px * capi.RT_GBUFFER_CHANNELS * 4), max(16, px))
            sets = [[hipmem.DeviceBuffer(n) for n in sizes] for _ in (0, 1)] + [[hipmem.DeviceBuffer(sizes[0])]]      # (the third: the upload of `cur`)
            h = self._history = dict(key=(kind, width, height), frames=0, at=0, cam=None, sets=sets)
            hipmem.synchronize()                                   # a DeviceBuffer is zeroed on the null stream, which the context's stream does not wait for
        prev, nxt = h["sets"][h["at"]], h["sets"][1 - h["at"]]
        if isinstance(cur, hipmem.DeviceBuffer):                    # already on the device (the occlusion): no host round trip
            d_cur = cur
        else:
            d_cur = h["sets"][2][0].from_numpy(np.ascontiguousarray(cur, np.float32))
        ctx.gbuffer(cam, width, height, out=nxt[1])
        # the first frame goes through the same call: the fresh set `prev` holds zeros, and a history length of 0 is "no history here", so the
        # output is the current frame bit for bit with every length 1
        m = reproject_map(cam, h["cam"] if h["frames"] else cam)
        ctx.reproject(d_cur, nxt[1], prev[0], prev[1], prev[2], width, height, m, params, out=nxt[0], len_out=nxt[2], channels=channels)
        keep = capi.rt_camera()
        C.memmove(C.byref(keep), C.byref(cam), C.sizeof(keep))
        h["cam"], h["at"], h["frames"] = keep, 1 - h["at"], h["frames"] + 1
        return nxt[0], nxt[1]

    def history_lengths(self):
        """uint8 (height, width): the number of frames each pixel of the latest accumulated frame stands for; None without history"""
        h = self._history
        if h is None:
            return None
        self.ctx.synchronize()
        _, w, r = h["key"]
        return h["sets"][h["at"]][2].to_numpy(np.uint8, (r, w))

    def _raytrace_temporal(self, cam, width, height, write_ppm, collect_stats, t0):
        from . import hipmem
        lib, ctx = self.ctx.lib, self.ctx
        k = self._temporal_frame_index("rgb", width, height)
        slots = max(1, capi.RT_MAX_PASSES // self.passes)            # frame k takes the passes (k mod slots) * count .., so that frames are decorrelated
        p = make_params(width, height, self.max_depth, collect_stats=collect_stats)
        L = self._lights()
        rgb = np.empty((height, width, 3), np.float32)
        filtered = None
        try:                                                         # (whatever fails, later frames start at pass 0 again)
            ctx.set_passes((k % slots) * self.passes, self.passes)
            capi.check(lib, ctx.handle, lib.rt_render(ctx.handle, C.byref(cam), C.byref(L), C.byref(p), _fptr(rgb), None, C.byref(self.stats)), "rt_render")
            acc, g = self._temporal_step("rgb", cam, width, height, 3, rgb, self.temporal)
            if self.denoise is not None:                            # the stored history is the image before the filter
                filtered = hipmem.DeviceBuffer(max(16, rgb.nbytes))
                hipmem.synchronize()
                ctx.denoise(acc, g, width, height, self.denoise, out=filtered, channels=3)
            ctx.synchronize()
            rgb = (acc if filtered is None else filtered).to_numpy(np.float32, (height, width, 3))
        finally:
            if filtered is not None:
                filtered.free()
            ctx.set_passes(0, self.passes)
        self.image, self.hits = rgb, None
        if write_ppm:
            capi.check(lib, None, lib.rt_write_ppm(self.output_path.encode(), _fptr(rgb), width, height), "rt_write_ppm")
        self.elapsed = time.time() - t0
        return rgb

    # reference: flyscene.cpp:651-771, batched (origins/directions [n,3])
    def traceRay(self, origin, direction, level=0, lights=None, countRay=False):
        o = np.ascontiguousarray(np.atleast_2d(np.asarray(origin, np.float32)))
        d = np.ascontiguousarray(np.atleast_2d(np.asarray(direction, np.float32)))
        n = o.shape[0]
        out = np.empty((n, 3), np.float32)
        face = np.empty(n, np.int32)
        t = np.empty(n, np.float32)
        L = self._lights(lights)
        budget = -1 if self.max_depth < 0 else max(0, self.max_depth - level)
        lib = self.ctx.lib
        capi.check(lib, self.ctx.handle,
                   lib.rt_trace_rays(self.ctx.handle, C.byref(L), budget, n, _fptr(o), _fptr(d), _fptr(out), _fptr(face), _fptr(t)),
                   "rt_trace_rays")
        self.last_face, self.last_t = face, t
        return out if np.ndim(origin) > 1 else out[0]

    # reference: flyscene.cpp:912-954
    def lightStrikes(self, hitPoint, lights):
        pts = np.ascontiguousarray(np.atleast_2d(np.asarray(lights, np.float32)))
        hit = np.ascontiguousarray(np.broadcast_to(np.asarray(hitPoint, np.float32), pts.shape).copy())
        vis = np.empty(pts.shape[0], np.uint8)
        lib = self.ctx.lib
        capi.check(lib, self.ctx.handle, lib.rt_light_strikes(self.ctx.handle, pts.shape[0], _fptr(hit), _fptr(pts), _fptr(vis)),
                   "rt_light_strikes")
        return bool(vis.any()), vis.astype(bool)

    # no reference member: the post-step of a float frame -- its geometry buffers under the context's current sample settings, then the filter
    def _denoised(self, image, cam, width, height, params):
        """image float32 (height, width, 3) or (height, width) of the frame of `cam` -> the same shape, filtered on the device"""
        from . import hipmem
        image = np.ascontiguousarray(image, np.float32)
        channels = 3 if image.ndim == 3 else 1
        bufs = []
        try:
            bufs.append(hipmem.DeviceBuffer(image.nbytes).from_numpy(image))
            bufs.append(hipmem.DeviceBuffer(width * height * capi.RT_GBUFFER_CHANNELS * 4))
            self.ctx.gbuffer(cam, width, height, out=bufs[1])
            bufs.append(hipmem.DeviceBuffer(image.nbytes))
            self.ctx.denoise(bufs[0], bufs[1], width, height, params, out=bufs[2], channels=channels)
            self.ctx.synchronize()
            return bufs[2].to_numpy(np.float32, image.shape)
        finally:
            for b in bufs:
                b.free()

    # no reference member: closest hits -> hit points -> rt_ambient_occlusion_device on the pinhole rays of the current camera
    def ambient_occlusion(self, width, height, grid, radius, seed=0, denoise=None, upsample=None, temporal=None):
        """-> float32 (height, width): per pixel the open share of the grid x grid cosine-weighted segments of length `radius` above the
        closest hit of the pixel's ray (origin = the camera centre, direction = screen point - centre, as raytraceScene forms it); 1.0
        where the ray hits nothing.  The point index of the rotation is the pixel's raster index j * width + i.  denoise: an
        rt_denoise_params = the image is filtered on the device before the download, guided by the one-ray pinhole geometry buffers of the
        same camera (this sets one sub-sample, no lens, no shutter, passes (0, 1) and no pass tolerance on the context).  upsample: an
        rt_upsample_params = the occlusion is computed at ceil(width / factor) x ceil(height / factor) through the low camera (the point
        index of the rotation is then the low pixel's raster index), filtered there if `denoise` is given, and brought to width x height
        with rt_upsample_device against the one-ray pinhole geometry buffers of both sizes (the same context settings).  temporal: an
        rt_reproject_params = successive calls of one size keep history as raytraceScene does with `Flyscene.temporal` (reset_history drops
        it): call k after the last reset takes the seed `seed + k`, its image is blended with the reprojected accumulated image of the
        call before, and `denoise` filters the result, the stored history being the image before the filter.  Not together with upsample."""
        from . import hipmem
        width, height = int(width), int(height)
        cam = self.camera
        if (width, height) != (self.width, self.height):
            cam = default_camera(width, height)
            cam.center, cam.inv_view = self.camera.center, self.camera.inv_view
        if upsample is not None:
            if temporal is not None:
                raise ValueError("ambient_occlusion: temporal together with upsample is not supported")
            return self._ambient_occlusion_upsampled(cam, width, height, grid, radius, seed, denoise, upsample)
        if temporal is not None:
            seed = int(seed) + self._temporal_frame_index("ao", width, height)
        n = width * height
        ctx, lib = self.ctx, self.ctx.lib
        pts = np.empty((n, 3), np.float32)
        capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(cam), width, height, _fptr(pts)), "rt_primary_points")
        centre = np.asarray(list(cam.center), np.float32)
        bufs = []
        try:
            for a in (np.broadcast_to(centre, (n, 3)), pts - centre):
                bufs.append(hipmem.DeviceBuffer(n * 12).from_numpy(np.ascontiguousarray(a, np.float32)))
            faces, ts = ctx.closest_hits(bufs[0], bufs[1], n=n)
            bufs += [faces, ts]
            points, normals = ctx.hit_points(bufs[0], bufs[1], faces, ts, n=n)
            bufs += [points, normals]
            _, ao = ctx.ambient_occlusion(points, normals, grid, radius, seed=seed, n=n, want_open=False)
            bufs.append(ao)
            if denoise is not None or temporal is not None:
                ctx.set_supersampling(1)
                ctx.set_lens(0.0, self.focus)
                ctx.set_shutter(None)
                ctx.set_passes(0, 1)
                ctx.set_pass_tolerance(-1.0, self.pass_min)
            g = None
            if temporal is not None:                                 # the history (image before the filter, buffers, lengths, camera) lives in self._history
                ao, g = self._temporal_step("ao", cam, width, height, 1, ao, temporal)
            if denoise is not None:
                if g is None:
                    g = hipmem.DeviceBuffer(n * capi.RT_GBUFFER_CHANNELS * 4)
                    bufs.append(g)
                    ctx.gbuffer(cam, width, height, out=g)
                bufs.append(hipmem.DeviceBuffer(n * 4))
                ctx.denoise(ao, g, width, height, denoise, out=bufs[-1], channels=1)
                ao = bufs[-1]
            ctx.synchronize()
            return ao.to_numpy(np.float32, (height, width))
        finally:
            for b in bufs:
                b.free()

    def _ambient_occlusion_upsampled(self, cam, width, height, grid, radius, seed, denoise, up):
        from . import hipmem
        ctx, lib = self.ctx, self.ctx.lib
        lcam, w, r = low_camera(cam, up.factor)
        n = w * r
        pts = np.empty((n, 3), np.float32)
        capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(lcam), w, r, _fptr(pts)), "rt_primary_points")
        centre = np.asarray(list(lcam.center), np.float32)
        bufs = []
        try:
            for a in (np.broadcast_to(centre, (n, 3)), pts - centre):
                bufs.append(hipmem.DeviceBuffer(n * 12).from_numpy(np.ascontiguousarray(a, np.float32)))
            faces, ts = ctx.closest_hits(bufs[0], bufs[1], n=n)
            bufs += [faces, ts]
            points, normals = ctx.hit_points(bufs[0], bufs[1], faces, ts, n=n)
            bufs += [points, normals]
            _, ao = ctx.ambient_occlusion(points, normals, grid, radius, seed=seed, n=n, want_open=False)
            bufs.append(ao)
            ctx.set_supersampling(1)
            ctx.set_lens(0.0, self.focus)
            ctx.set_shutter(None)
            ctx.set_passes(0, 1)
            ctx.set_pass_tolerance(-1.0, self.pass_min)
            # the remaining buffers first, then one wait: a DeviceBuffer is zeroed on the null stream, which the context's stream does not wait for
            g_low, filtered, g_high, out = (hipmem.DeviceBuffer(nbytes) for nbytes in (n * capi.RT_GBUFFER_CHANNELS * 4, max(16, n * 4),
                                                                                      width * height * capi.RT_GBUFFER_CHANNELS * 4, max(16, width * height * 4)))
            bufs += [g_low, filtered, g_high, out]
            ctx.synchronize()
            hipmem.synchronize()
            ctx.gbuffer(lcam, w, r, out=g_low)
            if denoise is not None:
                ctx.denoise(ao, g_low, w, r, denoise, out=filtered, channels=1)
                ao = filtered
            ctx.gbuffer(cam, width, height, out=g_high)
            ctx.upsample(ao, g_low, g_high, width, height, up, out=out, channels=1)
            ctx.synchronize()
            return out.to_numpy(np.float32, (height, width))
        finally:
            for b in bufs:
                b.free()

    # no reference member: closest hits -> hit points -> rt_soft_shadows_device on the pinhole rays of the current camera
    def soft_shadows(self, width, height, params=None, lights=None, denoise=None, upsample=None):
        """-> float32 (height, width): per pixel the share of the light samples that the closest hit of the pixel's ray sees (origin = the
        camera centre, direction = screen point - centre, as raytraceScene forms it); 1.0 where the ray hits nothing.  lights: an rt_lights,
        None = the lights of this object (point or area, not sphere).  params: an rt_shadow_params, None = the samples of every frame; the
        point index of a per-point jitter is the pixel's raster index j * width + i.  denoise / upsample: as in ambient_occlusion -- the
        image is filtered on the device, guided by the one-ray pinhole geometry buffers of the same camera (this sets one sub-sample, no
        lens, no shutter, passes (0, 1) and no pass tolerance on the context), or computed at ceil(width / factor) x ceil(height / factor)
        through the low camera (the point index is then the low pixel's raster index), filtered there if `denoise` is given, and brought to
        width x height with rt_upsample_device."""
        from . import hipmem
        width, height = int(width), int(height)
        cam = self.camera
        if (width, height) != (self.width, self.height):
            cam = default_camera(width, height)
            cam.center, cam.inv_view = self.camera.center, self.camera.inv_view
        L = self._lights() if lights is None else lights
        ctx, lib = self.ctx, self.ctx.lib
        qcam, w, r = (cam, width, height) if upsample is None else low_camera(cam, upsample.factor)
        n = w * r
        pts = np.empty((n, 3), np.float32)
        capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(qcam), w, r, _fptr(pts)), "rt_primary_points")
        centre = np.asarray(list(qcam.center), np.float32)
        bufs = []
        try:
            for a in (np.broadcast_to(centre, (n, 3)), pts - centre):
                bufs.append(hipmem.DeviceBuffer(n * 12).from_numpy(np.ascontiguousarray(a, np.float32)))
            faces, ts = ctx.closest_hits(bufs[0], bufs[1], n=n)
            bufs += [faces, ts]
            points, normals = ctx.hit_points(bufs[0], bufs[1], faces, ts, n=n)
            bufs += [points, normals]
            _, img = ctx.soft_shadows(points, normals, L, params, n=n, want_visible=False)
            bufs.append(img)
            if denoise is not None or upsample is not None:
                ctx.set_supersampling(1)
                ctx.set_lens(0.0, self.focus)
                ctx.set_shutter(None)
                ctx.set_passes(0, 1)
                ctx.set_pass_tolerance(-1.0, self.pass_min)
                # the remaining buffers first, then one wait: a DeviceBuffer is zeroed on the null stream, which the context's stream does not wait for
                g_low, filtered = hipmem.DeviceBuffer(n * capi.RT_GBUFFER_CHANNELS * 4), hipmem.DeviceBuffer(max(16, n * 4))
                bufs += [g_low, filtered]
                if upsample is not None:
                    g_high, out = hipmem.DeviceBuffer(width * height * capi.RT_GBUFFER_CHANNELS * 4), hipmem.DeviceBuffer(max(16, width * height * 4))
                    bufs += [g_high, out]
                ctx.synchronize()
                hipmem.synchronize()
                ctx.gbuffer(qcam, w, r, out=g_low)
                if denoise is not None:
                    ctx.denoise(img, g_low, w, r, denoise, out=filtered, channels=1)
                    img = filtered
                if upsample is not None:
                    ctx.gbuffer(cam, width, height, out=g_high)
                    ctx.upsample(img, g_low, g_high, width, height, upsample, out=out, channels=1)
                    img = out
            ctx.synchronize()
            return img.to_numpy(np.float32, (height, width))
        finally:
            for b in bufs:
                b.free()

    # no reference member: closest hits -> hit points -> rt_indirect_diffuse_device on the pinhole rays of the current camera
    def indirect_diffuse(self, width, height, grid, seed=0, lights=None, denoise=None, probes=None, visible=True):
        """-> float32 (height, width, 3): per pixel the mean radiance that grid x grid cosine-weighted gather rays bring back to the closest
        hit of the pixel's ray (origin = the camera centre, direction = screen point - centre, as raytraceScene forms it) after one diffuse
        bounce; zeros where the ray hits nothing.  The caller multiplies by the pixel's albedo.  The point index of the rotation is the
        pixel's raster index j * width + i.  lights: an rt_lights, None = the lights of this object (positions and colour are used; not
        sphere).  denoise: as in ambient_occlusion -- the three-channel image is filtered on the device, guided by the one-ray pinhole
        geometry buffers of the same camera (this sets one sub-sample, no lens, no shutter, passes (0, 1) and no pass tolerance on the
        context).  probes: (rt_probe_grid, coefficients) as light_probes(direct=False, bounces=...) returned them -- the hits of the gather
        rays are lit by that volume as well (rt_indirect_diffuse_bounce), the final gather over a bounced volume; visible: leak-free."""
        from . import hipmem
        width, height = int(width), int(height)
        cam = self.camera
        if (width, height) != (self.width, self.height):
            cam = default_camera(width, height)
            cam.center, cam.inv_view = self.camera.center, self.camera.inv_view
        L = self._lights() if lights is None else lights
        ctx, lib = self.ctx, self.ctx.lib
        n = width * height
        pts = np.empty((n, 3), np.float32)
        capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(cam), width, height, _fptr(pts)), "rt_primary_points")
        centre = np.asarray(list(cam.center), np.float32)
        bufs = []
        try:
            for a in (np.broadcast_to(centre, (n, 3)), pts - centre):
                bufs.append(hipmem.DeviceBuffer(n * 12).from_numpy(np.ascontiguousarray(a, np.float32)))
            faces, ts = ctx.closest_hits(bufs[0], bufs[1], n=n)
            bufs += [faces, ts]
            points, normals = ctx.hit_points(bufs[0], bufs[1], faces, ts, n=n)
            bufs += [points, normals]
            source = None
            if probes is not None:                         # the final gather over a bounced volume (what light_probes returned, direct off)
                pg, coeff = probes
                coeff = np.ascontiguousarray(coeff, np.float32)
                bufs.append(hipmem.DeviceBuffer(max(16, coeff.nbytes)).from_numpy(coeff))
                source = (pg, bufs[-1])
            img = ctx.indirect_diffuse(points, normals, L, grid, seed=seed, n=n, source=source, visible=visible)
            bufs.append(img)
            if denoise is not None:
                ctx.set_supersampling(1)
                ctx.set_lens(0.0, self.focus)
                ctx.set_shutter(None)
                ctx.set_passes(0, 1)
                ctx.set_pass_tolerance(-1.0, self.pass_min)
                # the remaining buffers first, then one wait: a DeviceBuffer is zeroed on the null stream, which the context's stream does not wait for
                g, filtered = hipmem.DeviceBuffer(n * capi.RT_GBUFFER_CHANNELS * 4), hipmem.DeviceBuffer(max(16, n * 12))
                bufs += [g, filtered]
                ctx.synchronize()
                hipmem.synchronize()
                ctx.gbuffer(cam, width, height, out=g)
                ctx.denoise(img, g, width, height, denoise, out=filtered, channels=3)
                img = filtered
            ctx.synchronize()
            return img.to_numpy(np.float32, (height, width, 3))
        finally:
            for b in bufs:
                b.free()

    # no reference member: an irradiance volume over the scene's root box (rt_light_probes)
    def light_probes(self, dims, grid, direct=False, margin=0.0, lights=None, bounces=0, visible=True):
        """-> (rt_probe_grid, float32 (probes, 27)): dims[0] x dims[1] x dims[2] probes over the scene's root box grown by `margin`
        (probe_grid_over), each traced with grid x grid rays and lit by `lights` (None = the lights of this object; not sphere).
        bounces: that many feedback passes (rt_light_probes_bounce) behind the first -- pass b lights every hit by pass b - 1 of this very
        volume as well, one more diffuse bounce each; the passes swap two buffers, run without the direct term, and `direct` goes into the
        last pass alone.  visible: the passes look the volume up leak-free.  bounces = 0 is the plain call."""
        pg = probe_grid_over(self.scene.info()["root_box"], dims, margin)
        pos = probe_grid_positions(pg)
        L = self._lights() if lights is None else lights
        bounces = int(bounces)
        if bounces < 0:
            raise ValueError("light_probes: bounces must be >= 0")
        coeff = np.empty((len(pos), capi.RT_PROBE_COEFFS), np.float32)
        lib, h = self.ctx.lib, self.ctx.handle
        capi.check(lib, h, lib.rt_light_probes(h, C.byref(L), len(pos), _fptr(pos), int(grid), 1 if direct and bounces == 0 else 0, _fptr(coeff)), "rt_light_probes")
        other = np.empty_like(coeff) if bounces else None
        for b in range(1, bounces + 1):
            capi.check(lib, h, lib.rt_light_probes_bounce(h, C.byref(L), len(pos), _fptr(pos), int(grid), 1 if direct and b == bounces else 0, C.byref(pg),
                                                          _fptr(coeff), 1 if visible else 0, _fptr(other)), "rt_light_probes_bounce")
            coeff, other = other, coeff
        return pg, coeff

    # no reference member: a distance volume over the scene's root box (rt_closest_points)
    def distance_field(self, dims, margin=0.0, max_dist=float("inf"), signed=False):
        """-> (rt_probe_grid, float32 (probes,) distances, int32 (probes,) faces): at each of the dims[0] x dims[1] x dims[2] points of
        probe_grid_over(root box, dims, margin) the distance to the nearest face within `max_dist` (the float32 square root of
        rt_closest_points' dist2; +inf: none) and that face's id (-1: none).  Both are flat, in the order of probe_grid_positions (x fastest):
        array.reshape(dims[2], dims[1], dims[0]) is the volume indexed [iz, iy, ix].
        signed: the distance is negated where inside() says 1, and a fourth result, bool (probes,), marks the points inside() left
        undecided (their distance stays positive)"""
        pg = probe_grid_over(self.scene.info()["root_box"], dims, margin)
        pos = probe_grid_positions(pg)
        dist, faces = self._distances(pos, max_dist)
        if not signed:
            return pg, dist, faces
        side = self.inside(pos)
        return pg, np.where(side == 1, -dist, dist).astype(np.float32), faces, side < 0

    def _ray_hits(self, origins, dirs, k=None, t_max=float("inf")):
        """rt_ray_hits on host arrays -> (faces (n, k), ts (n, k), counts (n,)); k None: RT_MAX_RAY_HITS"""
        k = capi.RT_MAX_RAY_HITS if k is None else int(k)
        o, d = np.ascontiguousarray(origins, np.float32).reshape(-1, 3), np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(o)
        faces, ts, counts = np.empty((n, k), np.int32), np.empty((n, k), np.float32), np.empty(n, np.int32)
        lib = self.ctx.lib
        capi.check(lib, self.ctx.handle, lib.rt_ray_hits(self.ctx.handle, n, _fptr(o), _fptr(d), k, float(t_max), _fptr(faces), _fptr(ts), _fptr(counts)),
                   "rt_ray_hits")
        return faces, ts, counts

    # no reference member: how much material the pinhole rays of the current camera pass through (rt_ray_hits)
    def thickness(self, width, height):
        """-> (float32 (height, width), bool (height, width)): per pixel the sum of t[2j+1] - t[2j] over the complete (entry, exit) pairs among
        the first RT_MAX_RAY_HITS hits of the pixel's primary ray (origin = the camera centre, direction = the pixel's screen point minus the
        centre, t in units of that direction; float32, pair after pair), and the mask of the pixels whose ray has more hits than that"""
        width, height = int(width), int(height)
        cam = self.camera
        if (width, height) != (self.width, self.height):
            cam = default_camera(width, height)
            cam.center, cam.inv_view = self.camera.center, self.camera.inv_view
        ctx, lib = self.ctx, self.ctx.lib
        pts = np.empty((width * height, 3), np.float32)
        capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(cam), width, height, _fptr(pts)), "rt_primary_points")
        centre = np.asarray(list(cam.center), np.float32)
        _, ts, counts = self._ray_hits(np.broadcast_to(centre, pts.shape), pts - centre)
        return thickness_of(ts, counts).reshape(height, width), (counts > capi.RT_MAX_RAY_HITS).reshape(height, width)

    # no reference member: which side of the surface a point is on, by the parity of the crossings of one ray (rt_ray_hits)
    def inside(self, points, direction=(1.0, 0.0, 0.0)):
        """-> int8 (points,): 1 = the ray from the point along `direction` crosses an odd number of faces, 0 = an even number, -1 = more
        than RT_MAX_RAY_HITS crossings (undecided).  Meaningful for closed surfaces; a ray through an edge or a doubled face counts both faces"""
        pos = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        _, _, counts = self._ray_hits(pos, np.broadcast_to(np.asarray(direction, np.float32), pos.shape))
        return parity_of(counts)

    def _distances(self, pos, max_dist=float("inf")):
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        d2, faces = np.empty(len(pos), np.float32), np.empty(len(pos), np.int32)
        lib = self.ctx.lib
        capi.check(lib, self.ctx.handle, lib.rt_closest_points(self.ctx.handle, len(pos), _fptr(pos), float(max_dist), _fptr(faces), _fptr(d2), None),
                   "rt_closest_points")
        return np.sqrt(d2), faces

    # no reference member: how much room the probes of light_probes have (a probe inside a wall gathers black; this tells)
    def probe_clearance(self, probes):
        """-> float32 (probes,): the distance of every probe of `probes` (what light_probes returned) to the nearest face of the scene"""
        return self._distances(probe_grid_positions(probes[0]))[0]

    # no reference member: closest hits -> hit points -> rt_probe_irradiance_device on the pinhole rays of the current camera
    def probe_irradiance(self, width, height, probes, visible=False):
        """-> float32 (height, width, 3): per pixel the lookup of `probes` (what light_probes returned) at the closest hit of the pixel's ray
        and its face normal; zeros where the ray hits nothing.  The caller multiplies by the pixel's albedo.  visible: the leak-free lookup
        (rt_probe_irradiance_visible_device), which blends the probes the hit point sees."""
        from . import hipmem
        pg, coeff = probes
        width, height = int(width), int(height)
        cam = self.camera
        if (width, height) != (self.width, self.height):
            cam = default_camera(width, height)
            cam.center, cam.inv_view = self.camera.center, self.camera.inv_view
        ctx, lib = self.ctx, self.ctx.lib
        n = width * height
        pts = np.empty((n, 3), np.float32)
        capi.check(lib, ctx.handle, lib.rt_primary_points(ctx.handle, C.byref(cam), width, height, _fptr(pts)), "rt_primary_points")
        centre = np.asarray(list(cam.center), np.float32)
        bufs = []
        try:
            for a in (np.broadcast_to(centre, (n, 3)), pts - centre, coeff):
                a = np.ascontiguousarray(a, np.float32)
                bufs.append(hipmem.DeviceBuffer(max(16, a.nbytes)).from_numpy(a))
            faces, ts = ctx.closest_hits(bufs[0], bufs[1], n=n)
            bufs += [faces, ts]
            points, normals = ctx.hit_points(bufs[0], bufs[1], faces, ts, n=n)
            bufs += [points, normals]
            if visible:
                img, _ = ctx.probe_irradiance_visible(pg, bufs[2], points, normals, n=n, want_mask=False)
            else:
                img = ctx.probe_irradiance(pg, bufs[2], points, normals, n=n)
            bufs.append(img)
            ctx.synchronize()
            return img.to_numpy(np.float32, (height, width, 3))
        finally:
            for b in bufs:
                b.free()

    def _frame_settings(self, width, height):
        """sets this object's sample settings (the shutter's close camera among them) on the context -> the camera of a width x height frame"""
        self.ctx.set_supersampling(self.supersample)
        self.ctx.set_supersampling_threshold(self.supersample_threshold)
        self.ctx.set_lens(self.aperture, self.focus)
        self.ctx.set_passes(0, self.passes)
        self.ctx.set_pass_tolerance(self.pass_tolerance, self.pass_min)
        cam = self.camera
        if (width, height) != (self.width, self.height):
            cam = default_camera(width, height)
            cam.center, cam.inv_view = self.camera.center, self.camera.inv_view
        close = self.shutter_close
        if close is not None and (width, height) != (self.width, self.height):
            close = default_camera(width, height)
            close.center, close.inv_view = self.shutter_close.center, self.shutter_close.inv_view
        self.ctx.set_shutter(close)
        return cam

    # no reference member: rt_gbuffer_device with the camera and the sample settings raytraceScene uses
    def gbuffer(self, width=0, height=0):
        """-> float32 (height, width, 8): coverage, depth, face normal and diffuse colour of every pixel of the frame raytraceScene(width,
        height) renders, averaged over its sub-samples and passes (include/rt_mi355x.h, RT_GBUFFER_CHANNELS)"""
        from . import hipmem
        if width == 0 or height == 0:
            width, height = self.width, self.height
        width, height = int(width), int(height)
        cam = self._frame_settings(width, height)
        buf = hipmem.DeviceBuffer(width * height * capi.RT_GBUFFER_CHANNELS * 4)
        try:
            self.ctx.gbuffer(cam, width, height, out=buf)
            capi.check(self.ctx.lib, self.ctx.handle, self.ctx.lib.rt_synchronize(self.ctx.handle), "rt_synchronize")
            return buf.to_numpy(np.float32, (height, width, capi.RT_GBUFFER_CHANNELS))
        finally:
            buf.free()

    # reference: flyscene.cpp:962-972, arealight.hpp:15-25 (float32 arithmetic in the reference's order)
    def createSpherePoint(self, lightPoint):
        p = np.asarray(lightPoint, np.float32)
        if self.pointLight:
            return p.reshape(1, 3).copy()
        if not self.areaLight:
            return (self.sphere_offsets + p).astype(np.float32)
        f = np.float32
        ux, uz, vy = f(p[0] + f(0.3) * f(1)), f(p[2] + f(0.3) * f(0)), f(p[1] + f(0.15) * f(1))
        out = np.empty((self.usteps * self.vsteps, 3), np.float32)
        k = 0
        for i in range(self.usteps):
            for j in range(self.vsteps):
                out[k] = (f(i + 0.5) * f(ux / f(self.usteps)), f(j + 0.5) * f(vy / f(self.vsteps)), uz)
                k += 1
        return out

    def addLight(self):
        if len(self.lights) < capi.RT_MAX_LIGHTS:
            self.lights.append(tuple(float(x) for x in self.camera.center))


class FrameGraph:
    """rt_graph: one frame's launch sequence captured into a hipGraph, replayed with a new camera per frame.
    Output buffers are caller-owned device memory (e.g. torch tensors); this class only keeps their addresses."""

    def __init__(self, ctx, lights, params, d_rgb_ptr=None, d_u8_ptr=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.handle = C.c_void_p()
        st = self.lib.rt_graph_create(ctx.handle, C.byref(lights), C.byref(params),
                                      C.c_void_p(d_rgb_ptr) if d_rgb_ptr else None,
                                      C.c_void_p(d_u8_ptr) if d_u8_ptr else None, C.byref(self.handle))
        capi.check(self.lib, ctx.handle, st, "rt_graph_create")

    def launch(self, camera, stream_ptr=None, close=None):
        """replay the frame with `camera`; a graph captured with the shutter on takes the camera at shutter close too (rt_graph_launch_shutter)"""
        stream = C.c_void_p(stream_ptr) if stream_ptr else None
        if close is not None:
            st = self.lib.rt_graph_launch_shutter(self.handle, C.byref(camera), C.byref(close), stream)
            capi.check(self.lib, self.ctx.handle, st, "rt_graph_launch_shutter")
            return
        st = self.lib.rt_graph_launch(self.handle, C.byref(camera), stream)
        capi.check(self.lib, self.ctx.handle, st, "rt_graph_launch")

    def stats(self):
        out = capi.rt_stats()
        capi.check(self.lib, self.ctx.handle, self.lib.rt_graph_stats(self.handle, C.byref(out)), "rt_graph_stats")
        return out

    def close(self):
        if self.handle:
            self.lib.rt_graph_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
