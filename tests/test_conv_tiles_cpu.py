"""The block plans of the shapes tests/test_conv_tiles_gpu.py runs, from the restatement of conv_f16s_plan, conv_f16s_launch's planning loop in
tests/conv_plan_ref.py: the GPU tests are named for kernel bodies (k_conv3x3_f16s<NI, MODE, ...> run with ntile tiles), and these
assertions keep them on those bodies when a frame constant of csrc/conv_split.hip changes.

The rows for n = 41 were derived by hand from the loop and are confirmed by the restatement as they stand: none had to be moved
to a neighbouring shape."""
import pytest

import conv_plan_ref as cp

N = 41                                   # the smallest batch above the small-batch re-cut; 41 = 5 x 8 + 1: one image behind the XCD groups
SWEEP = {1: 1, 3: 2, 4: 3, 6: 4, 7: 5, 9: 6, 10: 7, 12: 8}      # H of an H x 21 image -> its NI (one block per image)
SHAPES = [(h, 21) for h in SWEEP] + [(21, 21), (37, 37)]


def test_the_constants_are_found_in_the_source():
    c = cp.constants()
    assert set(c) == {"HS_NPB", "HS_NST", "HS_NST16", "HS_BUF16", "HS_LDP", "HS_GAP16_FULL", "FINE_MAX"}
    assert all(v > 0 for v in c.values())
    assert N == c["FINE_MAX"] + 1, "n = 41 is meant to be the first batch size the re-cut leaves alone"


@pytest.mark.parametrize("a16", [False, True])
@pytest.mark.parametrize("H", sorted(SWEEP))
def test_the_sweep_shapes_run_one_block_of_each_tile_count(H, a16):
    p = cp.plan(N, H, 21, a16)
    assert p == cp.Plan(1, SWEEP[H], 0, SWEEP[H])
    assert cp.block_tiles(p) == [SWEEP[H]]
    assert (H * 21) % 32 != 0, "the last tile of every sweep shape is ragged"


@pytest.mark.parametrize("a16", [False, True])
def test_the_11x11_board_runs_two_even_blocks_of_seven_tiles(a16):
    assert cp.plan(N, 21, 21, a16) == cp.Plan(2, 7, 0, 7)


def test_the_19x19_board_runs_uneven_blocks_in_both_frames():
    f32, b16 = cp.plan(N, 37, 37, False), cp.plan(N, 37, 37, True)
    assert f32 == cp.Plan(9, 4, 7, 5) and cp.block_tiles(f32) == [5, 5, 5, 5, 5, 5, 5, 4, 4]
    assert b16 == cp.Plan(6, 7, 1, 8) and cp.block_tiles(b16) == [8, 7, 7, 7, 7, 7]
    assert 37 * 37 - 32 * 42 == 25, "the image's last tile has 25 of 32 rows"


@pytest.mark.parametrize("a16", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 9])
@pytest.mark.parametrize("H,W", SHAPES)
def test_small_batches_run_one_tile_blocks(H, W, n, a16):
    """the gap the batched tests close: every layer-level comparison with an independent reference elsewhere in the suite has
    n <= 9 (and the image launched on its own in the frame-independence test has n = 1), which the re-cut turns into NI = 1"""
    p = cp.plan(n, H, W, a16)
    assert p.NI == 1 and p.tiles_rem == 0 and p.n_blk == (H * W + 31) // 32


def test_the_re_cut_ends_at_its_threshold():
    c = cp.constants()
    assert cp.plan(c["FINE_MAX"], 21, 21, False).NI < 7 and cp.plan(c["FINE_MAX"] + 1, 21, 21, False).NI == 7
    assert cp.plan(37, 21, 21, False) == cp.Plan(14, 1, 0, 1)     # test_f16s_fused_head_equals_layer_plus_head's batch


def test_a_row_wider_than_the_frame_is_refused():
    with pytest.raises(ValueError):
        cp.plan(1, 4, 200, False)
    assert cp.plan(1, 4, 80, False).NI >= 1
