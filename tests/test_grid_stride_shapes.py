"""Without a device: tests/grid_caps.py restates the grid rules of the C++ sources as they stand (pinned by text, so a changed cap fails here
instead of silently un-striding the GPU tests), the shapes of the strided GPU tests exceed their caps by the factor 1.25 and start round 2
where they claim to, and the conditions that those tests put on the restatement of the denoiser alone hold -- every iteration of the far-tap
cases moves the image, the second iteration of the strided frame shows, non-finite values stay in their pixels and their taps are stopped."""
import os

import numpy as np
import pytest

import denoise_ref as dr
import grid_caps as gc
import test_gpu_denoise as gd

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracer-in-cpp_amd", "csrc")
OTHER_CUS = (64, 72, 104, 145, 228, 304)            # (72 and 145: a cap is a multiple of the tile columns of the specified width)


def source(name):
    return open(os.path.join(CSRC, name)).read()


# ------------------------------------------------------------------------------------------ 1. the rules are the sources'
def test_grid_rules_are_the_ones_in_the_sources():
    dn, gb, ao, capi, kernels = (source(f) for f in ("rt_denoise_layout.hpp", "rt_gbuffer_layout.hpp", "rt_ao_layout.hpp", "rt_capi.cpp", "rt_kernels.hip"))
    chunks = source("rt_query_chunks.hpp")
    assert (gc.DN_TILE_W, gc.DN_TILE_H) == (64, 4) and "constexpr int32_t kDnTileW = 64, kDnTileH = 4;" in dn
    assert "constexpr int kDnThreads = kDnTileH * 64;" in source("rt_denoise.hip") and gc.DN_GUIDE_BLOCK == gc.DN_TILE_H * 64
    assert gc.BLOCKS_PER_CU == 8
    # the one rule (rt_query_chunks.hpp), and the five named grids as calls of it: per block 1, 256, 4, 256 and 4 with the multiplier min(rounds, 4)
    assert ("RT_QUERY_HD int32_t capped_grid(const uint64_t work, const uint32_t per_block, const int32_t cus, const int32_t cap_mult = 1) {\n"
            "    const uint64_t blocks = work / per_block + (work % per_block != 0u), cap = static_cast<uint64_t>(cus) * 8u * static_cast<uint64_t>(cap_mult);\n"
            "    return static_cast<int32_t>(blocks < cap ? blocks : cap);") in chunks
    assert "RT_QUERY_HD int32_t dn_grid(const uint32_t tiles, const int32_t cus) { return capped_grid(tiles, 1u, cus); }" in dn
    assert "RT_QUERY_HD int32_t dn_guide_grid(const uint64_t pixels, const int32_t cus) { return capped_grid(pixels, 256u, cus); }" in dn
    assert "tx = (static_cast<uint32_t>(width) + static_cast<uint32_t>(kDnTileW) - 1u) / static_cast<uint32_t>(kDnTileW);" in dn
    assert "ty = (static_cast<uint32_t>(rows) + static_cast<uint32_t>(kDnTileH) - 1u) / static_cast<uint32_t>(kDnTileH);" in dn
    assert gc.WAVES == 4 and "#define RT_WAVES 4 " in kernels and gc.GB_TILE == 8
    assert "const uint32_t tx = (static_cast<uint32_t>(width) + 7u) / 8u, ty = (static_cast<uint32_t>(rows) + 7u) / 8u;" in gb
    assert ("RT_QUERY_HD int32_t gb_grid(const uint32_t tiles, const int32_t cus) {\n"
            "    return capped_grid(tiles, 4u, cus);") in gb
    assert gc.QUERY_BLOCK == 256
    assert ("RT_QUERY_HD int32_t query_grid(const int32_t n, const int32_t cus) "
            "{ return capped_grid(n > 0 ? static_cast<uint64_t>(n) : 0u, 256u, cus); }") in chunks
    assert ("RT_QUERY_HD int32_t ao_grid(const uint64_t units, const int32_t cus, const int32_t rounds) {\n"
            "    return capped_grid(units, 4u, cus, rounds < 4 ? rounds : 4);") in ao
    # ... the launches take their grids from these rules, and the context its CU count from the device
    for call in ("launch_denoise_guide(dn_guide_grid(pixels, c->cus), ", "const int grid = dn_grid(dn_tiles(width, rows).tiles, c->cus);",
                 "launch_gbuffer(gb_grid(T.tiles, c->cus), ", "launch_closest(query_grid(n, c->cus), ", "launch_segments(query_grid(n, c->cus), stream_or_own(c, stream), ",
                 "launch_occlusion(ao_grid(ao_units(n, lay), c->cus, lay.rounds), ", "c->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;"):
        assert call in capi, call
    # ... and a block of the strided kernels holds what the rules count in
    for kernel in ("k_segments", "k_closest", "k_gbuffer", "k_occlusion"):
        assert f"__global__ __launch_bounds__(RT_WAVES * 64) void {kernel}(" in kernels, kernel


def test_grids_at_the_specified_cu_count():
    cus = gc.SPECIFIED_CUS
    assert (gc.dn_cap(cus), gc.dn_guide_cap(cus), gc.gb_cap(cus), gc.query_cap(cus)) == (2048, 524288, 8192, 524288)
    assert (gc.ao_cap(cus, 1), gc.ao_cap(cus, 9), gc.ao_cap(cus, 4)) == (8192, 32768, 32768)
    assert gc.dn_grid(24, cus) == 24 and gc.dn_grid(8100, cus) == 2048
    assert gc.dn_guide_grid(6144, cus) == 24 and gc.dn_guide_grid(1920 * 1080, cus) == 2048
    assert gc.gb_grid(24, cus) == 6 and gc.gb_grid(25, cus) == 7 and gc.gb_grid(32400, cus) == 2048
    assert gc.query_grid(1500, cus) == 6 and gc.query_grid(1920 * 1080, cus) == 2048
    assert gc.ao_grid(8193, cus, 1) == 2048 and gc.ao_grid(8193, cus, 25) == 2049
    assert gc.dn_tiles(1920, 1080) == (30, 270, 8100) and gc.gb_tiles(1920, 1080) == (240, 135, 32400)
    assert gc.strides(2560, 2048) and not gc.strides(2559, 2048) and gc.round_two(2048) == 2560


# ------------------------------------------------------------------------------------------ 2. the shapes stride
def check_shapes(cus):
    w, rows = gc.atrous_column(cus)
    tiles = gc.dn_tiles(w, rows)[2]
    assert w == 1 and gc.strides(tiles, gc.dn_cap(cus)) and gc.dn_grid(tiles, cus) < tiles and rows % gc.DN_TILE_H == 1
    w, rows = gc.denoise_frame(cus)
    tx, _, tiles = gc.dn_tiles(w, rows)
    assert gc.strides(tiles, gc.dn_cap(cus)) and gc.strides(w * rows, gc.dn_guide_cap(cus))
    assert gc.dn_grid(tiles, cus) < tiles and gc.dn_guide_grid(w * rows, cus) * gc.DN_GUIDE_BLOCK < w * rows
    assert tx > 1 and gc.dn_cap(cus) % tx != 0 and w % gc.DN_TILE_W != 0
    w, h = gc.gbuffer_frame(cus)
    tx, _, tiles = gc.gb_tiles(w, h)
    assert gc.strides(tiles, gc.gb_cap(cus)) and gc.gb_grid(tiles, cus) * gc.WAVES < tiles and gc.gb_cap(cus) % tx != 0
    row2 = gc.gbuffer_round_two_row(w, cus)
    assert (row2 // gc.GB_TILE) * tx >= gc.gb_cap(cus) > (row2 // gc.GB_TILE - 1) * tx and row2 + 8 <= h
    n = gc.query_rays(cus)
    assert gc.strides(n, gc.query_cap(cus)) and gc.query_grid(n, cus) * gc.QUERY_BLOCK < n and n % 64 == 3


def test_shapes_at_the_specified_cu_count():
    cus = gc.SPECIFIED_CUS
    check_shapes(cus)
    assert gc.atrous_column(cus) == (1, 10241) and gc.dn_tiles(1, 10241) == (1, 2561, 2561)
    assert gc.denoise_frame(cus) == (1100, 600) and gc.dn_tiles(1100, 600) == (18, 150, 2700) and 2048 % 18 != 0
    assert gc.dn_guide_grid(1100 * 600, 1 << 20) == 2579
    assert gc.gbuffer_frame(cus) == (1160, 580) and gc.gb_tiles(1160, 580) == (145, 73, 10585) and 8192 % 145 == 72
    assert gc.gbuffer_round_two_row(1160, cus) == 456 == 8 * (8192 // 145) + 8
    assert gc.query_rays(cus) == 655683 == 5 * 524288 // 4 + 64 * 5 + 3
    # the shapes of the far-tap cases that do not stride: wider, and higher, than the reach 2 * 128 of the eighth iteration on both sides
    assert gd.far_shape("row", cus) == (1100, 3) and gd.far_shape("both", cus) == (300, 261) and gd.far_shape("column", cus) == (1, 10241)
    assert gc.dn_tiles(300, 261) == (5, 66, 330) and 300 % 64 != 0 and 261 % 4 != 0 and min(1100, 300, 261, 10241) > 2 * 128


@pytest.mark.parametrize("cus", OTHER_CUS)
def test_shapes_scale_with_the_cu_count(cus):
    check_shapes(cus)


# ------------------------------------------------------------------------------------------ 3. the conditions on the restatement alone
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("which", ["column", "row", "both"])
def test_every_iteration_of_the_far_tap_cases_moves_the_image(which, ch):
    w, rows = gd.far_shape(which, gc.SPECIFIED_CUS)
    img, g = gd.synthetic(rows, w, ch)
    _, moved = gd.stepwise(img, g, dr.Params(8, *gd.FAR))
    assert gd.every_iteration_moves_the_image(moved), moved
    if which != "both":             # with the colour stop the far iterations fade: the reason for the case without it
        _, stopped = gd.stepwise(img, g, dr.Params(8, *gd.EIGHT))
        assert stopped[7] < 0.5 < moved[7]


@pytest.mark.parametrize("ch", [1, 3])
def test_the_second_iteration_of_the_strided_frame_shows(ch):
    w, rows = gc.denoise_frame(gc.SPECIFIED_CUS)
    img, g = gd.synthetic(rows, w, ch)
    images, moved = gd.stepwise(img, g, dr.Params(2, *gd.FINITE))
    assert not gd.same(images[1], images[0]) and moved[1] > 0.5


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("size", gd.POISON_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_non_finite_values_stay_in_their_pixels(size, ch):
    w, rows = size
    img, g, bad = gd.poisoned(rows, w, ch)
    clean, _ = gd.synthetic(rows, w, ch)
    assert np.array_equal(gd.pixel_not_finite(img), bad) and bad.sum() >= 5 and not gd.pixel_not_finite(clean).any()
    for kind in (np.isnan, np.isposinf, np.isneginf):
        assert kind(img).any()
    a = g[..., 0]
    assert np.isnan(a).any() and (a == -1.0).any() and np.isposinf(a).any() and (gd.bits(a) == 0x80000000).any() and np.isnan(g[..., 1:]).any()
    for it in (1, 5):
        for sig in gd.POISON_SIGMAS:
            p = dr.Params(it, *sig)
            stays, differ = gd.poison_stays_where_it_was(dr.denoise(img, g, p), dr.denoise(clean, g, p), bad)
            assert stays, (it, sig)
            assert differ > gd.poison_shows(size), (it, sig, differ)
