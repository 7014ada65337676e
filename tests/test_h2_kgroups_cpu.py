"""``fgn_h2_k_groups`` (host logic, no GPU): which launches conv_pw_h2_kernel runs on two K-groups - its 64-row tile with
two sets of four waves per output tile, each on every other K-tile (csrc/conv_pw_h2.h).  Only an ungrouped
launch of at most 256 tiles (one per CU: the 96 KB of LDS cost no resident workgroup) with an even K-tile count at or
above the threshold; ``fgn_h2_row_tile`` itself is unchanged."""
import pytest

# the shapes tests/test_host_cpu.py::test_h2_routing_rule_is_host_logic pins, with the tile it pins for each
_ROW_TILES = [
    ((14700, 1024, 1024, 0, 0), 64), ((36 * 1280, 512, 512, 1280, 1236), 128), ((36 * 896, 1024, 1024, 896, 819), 128),
    ((36 * 512, 512, 512, 512, 400), 64), ((103664, 64, 256, 0, 0), 264), ((103664, 64, 576, 0, 0), 264),
    ((25916, 128, 1152, 0, 0), 64), ((12600, 76, 1024, 0, 0), 0), ((3000, 64, 256, 0, 0), 0), ((103664, 40, 256, 0, 0), 0),
    ((441, 512, 1024, 0, 0), 0),
]


@pytest.fixture(scope='module')
def L():
    from fgn_amd import lib
    return lib.load()


@pytest.mark.parametrize('shape', [(6504, 256, 1024, 0, 0),       # layer3.1-3.5 conv1: 204 tiles, 32 K-tiles
                                   (6504, 256, 2304, 0, 0)])      # layer3.0 conv2 as an implicit GEMM: 204 tiles, 72 K-tiles
def test_one_tile_per_cu_and_a_long_even_k_loop_run_on_two_groups(L, shape):
    assert L.fgn_h2_row_tile(*shape) == 64
    assert L.fgn_h2_k_groups(*shape) == 2


@pytest.mark.parametrize('shape', [
    (6504, 1024, 256, 0, 0),                     # 816 tiles
    (4200, 512, 1024, 0, 0),                     # 264 tiles: more than one per CU
    (14700, 1024, 1024, 0, 0),                   # relation Q
    (36 * 512, 512, 512, 512, 400),              # grouped (Winograd, mask head)
    (36 * 1280, 512, 512, 1280, 1236),           # grouped, 128-row tile
    (6504, 256, 1056, 0, 0),                     # 33 K-tiles: odd
    (6504, 256, 64, 0, 0),                       # 2 K-tiles: below any threshold the forced code accepts
    (6504, 256, 128, 0, 0),                      # 4 K-tiles: the least the forced code runs, below the routing threshold
    (6504, 256, 192, 0, 0),                      # 6 K-tiles: even, below the threshold of 8
])
def test_every_other_launch_stays_on_one_group(L, shape):
    assert L.fgn_h2_k_groups(*shape) == 1


def test_the_threshold_is_the_shallowest_k_loop_measured(L):
    assert L.fgn_h2_k_groups(6504, 256, 256, 0, 0) == 2              # 8 K-tiles: 11.4 -> 10.4 us (profiles/h2_kgroups_ab.json)
    assert L.fgn_h2_k_groups(6504, 256, 512, 0, 0) == 2


def test_256_tiles_is_the_last_grid_on_two_groups(L):
    assert L.fgn_h2_k_groups(128 * 64, 256, 1024, 0, 0) == 2         # 128 x 2 = 256 tiles
    assert L.fgn_h2_k_groups(128 * 64 + 1, 256, 1024, 0, 0) == 1     # 129 x 2 = 258


def test_only_the_64_row_tile_has_two_groups(L):
    """Every shape fgn_h2_row_tile does not put on the 64-row tile stays on one group, whatever its K."""
    for shape, tile in _ROW_TILES:
        assert L.fgn_h2_row_tile(*shape) == tile, shape       # unchanged by the K-groups
        if tile != 64:
            assert L.fgn_h2_k_groups(*shape) == 1, shape
    for cout in (40, 48, 64, 76, 128, 256):
        for rows in (441, 3000, 6504, 12300, 16000, 103664):
            for k in (256, 1024, 2304):
                if L.fgn_h2_row_tile(rows, cout, k, 0, 0) != 64:
                    assert L.fgn_h2_k_groups(rows, cout, k, 0, 0) == 1, (rows, cout, k)


def test_the_kernel_name_follows_the_groups(L):
    from fgn_amd import ops
    assert ops.h2_kernel(6504, 256, 1024) == 'conv_pw_h2_kernel<2, 2, 1, 2, false, 2>'
    assert ops.h2_kernel(6504, 256, 2304, im2col=True) == 'conv_pw_h2_kernel<2, 2, 1, 2, true, 2>'
    assert ops.h2_kernel(6504, 1024, 256) == 'conv_pw_h2_kernel<2, 2, 1, 2, false, 1>'
    assert ops.h2_kernel(36 * 1280, 512, 512, 1280, 1236) == 'conv_pw_h2_kernel<2, 2, 2, 2, false, 1>'
    assert all(n.startswith('conv_pw_h2_kernel') for n in ops.H2_KERNELS.values())
