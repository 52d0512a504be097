"""MI355X-native primary/shadow ray-trace path: drop-in for Raytracer-in-CPP's CPU ThreadPool render.

Only what the path needs lives here: csrc/ (HIP kernels + C ABI + GL-free host scene code), the ctypes binding
(capi), the Python mirror of the reference's Flyscene interface (flyscene) and the row-shard helpers (shard).
"""
from . import capi, hipmem, rays, shard  # noqa: F401
from .capi import load_library  # noqa: F401
from .flyscene import (Context, Flyscene, FrameGraph, HostScene, default_camera, denoise_params, light_samples, low_camera, make_lights,  # noqa: F401
                       make_params, parity_of, primary_rect, probe_grid, probe_grid_over, probe_grid_positions, reproject_map, reproject_params, set_sphere, shadow_jitter, shadow_params, sphere_offsets, thickness_of,
                       upsample_params)
