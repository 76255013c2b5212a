"""The shapes of tests/test_gpu_train_step_odd_sizes.py, pinned: what every (B, H, W) of `train_step_check.ODD_SHAPES` reaches is
arithmetic on `netspec.sizes_for` (every stage halves, rounding up), and a shape changed into one that crops nothing, or that leaves
the coarsest BatchNorm a handful of rows, would go on passing there while testing nothing.

level sizes: conv1, conv2 (= concat2), conv3_1 (= concat3), conv4_1, conv5_1, conv6_1.  crops: per decoder level, (rows, columns) --
True where the transposed convolution's 2x output has one row / column more than the skip it is concatenated with, so that the
forward crops it and the backward pass must leave that row / column without a gradient."""
import pytest

from coupe.optical_flow_based_deep_video_stabilization_amd import netspec
from tests.train_step_check import ODD_SHAPES

TABLE = {
    # a crop on both axes at every decoder level; odd tile grids in conv3_1 .. conv6_1; the head's H - 2 = 192 rows from 49
    (2, 194, 258): dict(levels=((97, 129), (49, 65), (25, 33), (13, 17), (7, 9), (4, 5)),
                        crops={"deconv5": (True, True), "deconv4": (True, True), "deconv3": (True, True), "deconv2": (True, True)}),
    # the mixed case: crops at deconv5, 4, 3 and none at deconv2; even conv1 and conv2
    (2, 200, 264): dict(levels=((100, 132), (50, 66), (25, 33), (13, 17), (7, 9), (4, 5)),
                        crops={"deconv5": (True, True), "deconv4": (True, True), "deconv3": (True, True), "deconv2": (False, False)}),
    # an odd frame, a batch of 3, deconv2 cropped on one axis only, 3x4 and 5x7 maps under Winograd.  (conv1: a row of 197 * 27
    # floats is no multiple of 4, which the row-window kernel declines, as it does 258 * 27; 264 * 27 it takes.)
    (3, 131, 197): dict(levels=((66, 99), (33, 50), (17, 25), (9, 13), (5, 7), (3, 4)),
                        crops={"deconv5": (True, True), "deconv4": (True, True), "deconv3": (True, True), "deconv2": (True, False)}),
}


def test_the_table_covers_the_shapes_of_the_gpu_test():
    assert set(TABLE) == set(ODD_SHAPES) and len(ODD_SHAPES) == 3


@pytest.mark.parametrize("shape", sorted(TABLE), ids=lambda s: "x".join(map(str, s)))
def test_level_sizes_crops_and_batchnorm_rows(shape):
    B, H, W = shape
    lv = netspec.sizes_for(H, W).level
    assert tuple(lv[k] for k in (1, 2, 3, 4, 5, 6)) == TABLE[shape]["levels"]
    crops = {f"deconv{k}": tuple(2 * lo != up for lo, up in zip(lv[k + 1], lv[k])) for k in (5, 4, 3, 2)}
    assert crops == TABLE[shape]["crops"]
    h6, w6 = lv[6]
    assert B * h6 * w6 >= 32
    # a crop is one row / column, never more (what the convolution entry points take), and some level is cropped
    assert all(2 * lo - up in (0, 1) for k in (5, 4, 3, 2) for lo, up in zip(lv[k + 1], lv[k]))
    assert any(any(c) for c in crops.values())
    assert H % 64 or W % 64
