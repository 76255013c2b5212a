"""Pins tests/data_loader_ref.py, the NumPy float64 restatement of the reference loader's `_read_frame` (cv2.resize on the float64
`/ 255.` image), which the HIP kernel is then held to bit for bit (tests/test_gpu_data_loader.py).  cv2 is not installed: the
restatement is unpinned against cv2 itself and pinned here by exact known answers, by the float32 restatement the project already
carries (oracle.vstab_oracle.cv_resize_f32) and by an independent half-pixel-centre bilinear (scipy.ndimage)."""
import numpy as np
import pytest

from oracle import vstab_oracle as vo
from tests import data_loader_ref as ref

SIZES = [((9, 13), (6, 10)), ((40, 31), (17, 23)), ((34, 46), (17, 23)), ((1, 7), (6, 10)), ((7, 1), (16, 32)), ((45, 60), (48, 64)),
         ((45, 60), (90, 120)), ((45, 60), (33, 47))]


def _img(sh, sw, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (sh, sw, 3), dtype=np.uint8)


def test_same_size_is_the_fp32_quotient():
    u = _img(11, 14)
    u[0, :3, 0] = (0, 255, 1)
    out = ref.read_frame(u, 11, 14)
    assert out.dtype == np.float64
    assert np.array_equal(out.astype(np.float32), (u / 255.).astype(np.float32))
    # the general formula gives the same bits: coefficient 1 on the pixel itself, 0 on its neighbour
    x0, x1, a0, a1 = ref._taps(14, 14)
    assert x0.tolist() == list(range(14)) and np.all(a0 == 1) and np.all(a1 == 0)


@pytest.mark.parametrize("src,dst", SIZES)
def test_constant_image_stays_constant(src, dst):
    for v in (0, 1, 77, 254, 255):
        u = np.full(src + (3,), v, np.uint8)
        out = ref.read_frame(u, *dst).astype(np.float32)
        # a0 = 1.f - a1 is rounded to float32, so a0 + a1 = 1 + e with |e| <= 2^-25 per axis; two axes and the final rounding to
        # float32 (2^-25 on values <= 1) stay within 3 * 2^-25 < 2^-23
        assert np.abs(out - np.float32(v / 255.)).max() <= 2.0 ** -23, v
    # ... and exactly constant where every tap is clamped (coefficients 1 and 0)
    out = ref.read_frame(np.full((1, 1, 3), 77, np.uint8), 6, 10)
    assert np.all(out == 77 / 255.)


def test_exact_x2_reduction_is_the_mean_of_four_in_double():
    u = _img(34, 46, 1)
    s = u / 255.
    # both coefficients are exactly 0.5 on both axes: (a*.5 + b*.5)*.5 + (c*.5 + d*.5)*.5, halving is exact
    want = ((s[0::2, 0::2] + s[0::2, 1::2]) * 0.5) * 0.5 + ((s[1::2, 0::2] + s[1::2, 1::2]) * 0.5) * 0.5
    got = ref.read_frame(u, 17, 23)
    assert np.array_equal(got, want)
    assert np.abs(got - (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]) / 4).max() <= 2.0 ** -52


@pytest.mark.parametrize("src,dst", SIZES)
def test_against_the_float32_restatement(src, dst):
    """cv_resize_f32 runs the same taps and coefficients in float32: rounding of the image to fp32, of the row value and of the result,
    three roundings of half an ulp (<= 2^-25 each on values <= 1) scaled by coefficients that sum to 1 -- within 2^-22."""
    u = _img(*src, seed=2)
    got = ref.read_frame(u, *dst)
    f32 = vo.cv_resize_f32((u / 255.).astype(np.float32), *dst)
    assert np.abs(got - f32.astype(np.float64)).max() <= 2.0 ** -22


@pytest.mark.parametrize("src,dst", SIZES)
def test_against_an_independent_bilinear(src, dst):
    """float64 bilinear at half-pixel centres, edge-replicated (scipy.ndimage.map_coordinates), as test_oracle_kat.py pins
    cv_resize_f32, with that file's tolerance (2e-6: the float32 coefficients)."""
    from scipy import ndimage
    u = _img(*src, seed=3)
    s = u / 255.
    (sh, sw), (dh, dw) = src, dst
    fy = np.clip((np.arange(dh) + 0.5) * (sh / dh) - 0.5, 0, sh - 1)
    fx = np.clip((np.arange(dw) + 0.5) * (sw / dw) - 0.5, 0, sw - 1)
    yy, xx = np.meshgrid(fy, fx, indexing="ij")
    want = np.stack([ndimage.map_coordinates(s[..., c], [yy, xx], order=1, mode="nearest") for c in range(3)], -1)
    assert np.abs(ref.read_frame(u, dh, dw) - want).max() <= 2e-6


def test_read_dataset_layout():
    rng = np.random.default_rng(4)
    stab, unstab = rng.integers(0, 256, (40, 9, 13, 3), dtype=np.uint8), rng.integers(0, 256, (40, 9, 13, 3), dtype=np.uint8)
    skip = [1, 9, 17, 25, 28, 29, 30, 31, 32]
    feats, gt, un = ref.read_dataset(stab, unstab, 5, skip, 6, 10)
    assert feats.shape == (6, 10, 27) and feats.dtype == np.float32 and gt.shape == un.shape == (6, 10, 3)
    for j in range(8):
        assert np.array_equal(feats[..., 3 * j:3 * j + 3], ref.read_frame(stab[5 + skip[j]], 6, 10).astype(np.float32))
    assert np.array_equal(feats[..., 24:], un) and np.array_equal(un, ref.read_frame(unstab[37], 6, 10).astype(np.float32))
    assert np.array_equal(gt, ref.read_frame(stab[37], 6, 10).astype(np.float32))
