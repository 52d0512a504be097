"""The grid rules of the kernels that launch a capped grid and cover the rest of their work by grid stride, restated in Python -- dn_grid and
dn_guide_grid (rt_denoise_layout.hpp), gb_grid (rt_gbuffer_layout.hpp), query_grid (rt_capi.cpp), ao_grid (rt_ao_layout.hpp) -- and the
shapes of the tests that reach the strided rounds, derived from the device's CU count so that at least a quarter of a cap's worth of work
lies in the second round: work >= 1.25 x cap.  The shapes of 256 CUs are the ones the tests were specified with; for another CU count the
long dimension scales.  tests/test_grid_stride_shapes.py pins the constants here to the C++ sources.

Test infrastructure only."""

BLOCKS_PER_CU = 8                # every rule: at most 8 blocks per CU
DN_TILE_W, DN_TILE_H = 64, 4     # kDnTileW, kDnTileH: a block of k_atrous holds one tile
DN_GUIDE_BLOCK = 256             # pixels of a block of k_denoise_guide
GB_TILE = 8                      # a wave of k_gbuffer holds an 8 x 8 tile
WAVES = 4                        # RT_WAVES: tiles of a block of k_gbuffer, wave units of a block of k_occlusion
QUERY_BLOCK = 256                # rays of a block of k_closest / k_segments
SPECIFIED_CUS = 256


def cu_count(device=0):
    """the CU count the library's context of `device` reads (hipDeviceProp_t::multiProcessorCount), through torch"""
    import torch
    return int(torch.cuda.get_device_properties(device).multi_processor_count)


def _ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------ the rules
def dn_tiles(width, rows):
    """(tiles_x, tiles_y, tiles) of the 64 x 4 tiles of a denoiser image"""
    tx, ty = _ceil_div(width, DN_TILE_W), _ceil_div(rows, DN_TILE_H)
    return tx, ty, tx * ty


def dn_cap(cus):
    """tiles of one round of k_atrous"""
    return BLOCKS_PER_CU * cus


def dn_grid(tiles, cus):
    return min(tiles, dn_cap(cus))


def dn_guide_cap(cus):
    """pixels of one round of k_denoise_guide"""
    return BLOCKS_PER_CU * cus * DN_GUIDE_BLOCK


def dn_guide_grid(pixels, cus):
    return min(_ceil_div(pixels, DN_GUIDE_BLOCK), BLOCKS_PER_CU * cus)


def gb_tiles(width, rows):
    """(tiles_x, tiles_y, tiles) of the 8 x 8 tiles of a geometry-buffer frame"""
    tx, ty = _ceil_div(width, GB_TILE), _ceil_div(rows, GB_TILE)
    return tx, ty, tx * ty


def gb_cap(cus):
    """tiles of one round of k_gbuffer"""
    return BLOCKS_PER_CU * cus * WAVES


def gb_grid(tiles, cus):
    return min(_ceil_div(tiles, WAVES), BLOCKS_PER_CU * cus)


def query_cap(cus):
    """rays of one round of k_closest, segments of one round of k_segments"""
    return BLOCKS_PER_CU * cus * QUERY_BLOCK


def query_grid(n, cus):
    return min(_ceil_div(n, QUERY_BLOCK), BLOCKS_PER_CU * cus)


def ao_cap(cus, rounds):
    """wave units of one round of k_occlusion: the cap grows with the rounds of a unit, up to 4 times"""
    return BLOCKS_PER_CU * cus * min(rounds, 4) * WAVES


def ao_grid(units, cus, rounds):
    return min(_ceil_div(units, WAVES), BLOCKS_PER_CU * cus * min(rounds, 4))


def strides(work, cap):
    """at least a quarter of the cap's worth of work lies behind the first round: work >= 1.25 x cap"""
    return 4 * work >= 5 * cap


def round_two(cap):
    """the least work with strides(work, cap)"""
    return _ceil_div(5 * cap, 4)


# ------------------------------------------------------------------------------------------ the shapes (width, rows) of the strided tests
def atrous_column(cus=SPECIFIED_CUS):
    """one pixel column: every row of four is a tile, and one more row makes a partial last tile.  256 CUs: 1 x 10,241, 2,561 tiles"""
    return 1, DN_TILE_H * round_two(dn_cap(cus)) + 1


def _not_a_multiple(cap, width, tile):
    """`width`, or one tile column more where the cap is a multiple of the tile columns (then round 2 would start at tile column 0)"""
    return width + tile if cap % _ceil_div(width, tile) == 0 else width


def denoise_frame(cus=SPECIFIED_CUS):
    """several tile columns with a partial last one: k_denoise_guide and k_atrous both stride, and the first tile of round 2 is not in tile
    column 0.  256 CUs: 1,100 x 600 = 660,000 pixels in 2,579 guide blocks and 18 x 150 = 2,700 tiles"""
    width = _not_a_multiple(dn_cap(cus), 1100, DN_TILE_W)
    return width, _ceil_div(600 * cus, SPECIFIED_CUS)


def gbuffer_frame(cus=SPECIFIED_CUS):
    """256 CUs: 1,160 x 580, 145 x 73 = 10,585 tiles, the first tile of round 2 in tile column 8,192 % 145 = 72"""
    width = _not_a_multiple(gb_cap(cus), 1160, GB_TILE)
    return width, _ceil_div(580 * cus, SPECIFIED_CUS)


def gbuffer_round_two_row(width, cus=SPECIFIED_CUS):
    """the first frame row all of whose tiles belong to round 2 or later (the tile row before it is split between the rounds)"""
    tx = _ceil_div(width, GB_TILE)
    return GB_TILE * _ceil_div(gb_cap(cus), tx)


def query_rays(cus=SPECIFIED_CUS):
    """1.25 caps, five waves and three rays: the last wave of the batch is a partial one.  256 CUs: 655,683"""
    return round_two(query_cap(cus)) + 64 * 5 + 3
