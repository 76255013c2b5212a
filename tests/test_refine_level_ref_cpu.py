"""tests/refine_level_ref.py checked on the CPU: the Winograd F(2x2,2x2) algebra with wdec_geom's clipping rule against the plain
transposed convolution at every small size (which proves the rule nt[] without a GPU), and the flow head's reference against the oracle's
own layers (pad_conv, resize_bilinear_legacy, deconv4x4s2)."""
import numpy as np
import pytest
import torch

from oracle import vstab_oracle as vo
from tests import refine_level_ref as ref

AXIS = [(Hi, Ho) for Hi in range(1, 9) for Ho in (2 * Hi - 1, 2 * Hi)]


@pytest.mark.parametrize("Hi,Ho", AXIS, ids=lambda v: str(v))
def test_winograd_algebra_and_clipping_rule_vs_plain_deconv(Hi, Ho):
    """every (Hi, Ho) crossed with every (Wi, Wo): agreement to 1e-12 relative, every output pixel produced"""
    rng = np.random.default_rng(Hi * 17 + Ho)
    B, cin, cout = 2, 3, 2
    W = rng.standard_normal((4, 4, cout, cin))
    for Wi, Wo in AXIS:
        x = rng.standard_normal((B, Hi, Wi, cin))
        want = ref.deconv_ref(x, W, None, 0, (Ho, Wo)).numpy()
        got = ref.wdec_emulated(x, W, (Ho, Wo))
        assert not np.isnan(got).any(), (Hi, Ho, Wi, Wo)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (Hi, Ho, Wi, Wo)


def test_clipping_rule_is_tight_where_the_issue_says_the_grid_is_clipped():
    """the rule is not vacuous: one tile less in any position row breaks the result, and the named cases clip where they should"""
    assert ref.wdec_geom(4, 4, 7, 7)["nty"] == [2, 2, 2] and ref.wdec_geom(4, 4, 7, 7)["NTy"] == 2          # clipped by NT
    assert ref.wdec_geom(6, 6, 11, 11)["nty"] == [3, 3, 3]
    assert ref.wdec_geom(2, 2, 4, 4)["nty"] == [2, 1, 1] and ref.wdec_geom(2, 2, 4, 4)["NTy"] == 2          # clipped by the input
    rng = np.random.default_rng(1)
    for Hi, Ho in ((2, 4), (4, 7), (5, 10), (6, 11)):
        x = rng.standard_normal((1, Hi, Hi, 2))
        W = rng.standard_normal((4, 4, 2, 2))
        want = ref.deconv_ref(x, W, None, 0, (Ho, Ho)).numpy()
        g = ref.wdec_geom(Hi, Hi, Ho, Ho)
        for i in range(3):
            less = dict(g, nty=[n - (k == i) for k, n in enumerate(g["nty"])])
            assert np.abs(ref.wdec_emulated(x, W, (Ho, Ho), less) - want).max() > 1e-3, (Hi, Ho, i)


def test_deconv_ref_slice_bias_and_activation():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 3, 5, 8))
    W = rng.standard_normal((4, 4, 4, 6))                                  # cin = 6 of the pixel's 8 floats
    b = rng.standard_normal(4)
    out = torch.full((2, 5, 10, 12), 7.0, dtype=torch.float64)
    y = ref.deconv_ref(x, W, b, 1, (5, 10), out, 4)
    want = vo.deconv4x4s2(torch.from_numpy(x[..., :6].copy()), torch.from_numpy(W), torch.from_numpy(b), (5, 10))
    want = torch.maximum(want, 0.1 * want)
    assert float((y - want).abs().max()) <= 1e-12
    assert torch.equal(out[..., 4:8], y) and bool((out[..., :4] == 7.0).all()) and bool((out[..., 8:] == 7.0).all())


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (2, 3), (5, 9), (11, 13)])
@pytest.mark.parametrize("ks", [1, 3])
def test_predict_up_ref_vs_the_oracle_layers(h, w, ks):
    """the tap table is built from x [B,h,w,C] and the head's filter [3,3,C,2], split into ks slabs over channel groups; the reference
    must equal pad_conv(x) (+ 2 * the legacy resize of prev) and deconv4x4s2 of that"""
    rng = np.random.default_rng(h * 31 + w + ks)
    B, C = 2, 6
    x = rng.standard_normal((B, h, w, C))
    Wp = rng.standard_normal((3, 3, C, 2))
    b = rng.standard_normal(2)
    up_w = rng.standard_normal((4, 4, 2, 2))
    up_b = rng.standard_normal(2)
    groups = np.array_split(np.arange(C), ks)
    slabs = np.full((ks, B, h, w, 32), np.nan)
    for k, gch in enumerate(groups):
        slabs[k, ..., :18] = np.einsum("bhwc,tco->bhwto", x[..., gch], Wp.reshape(9, C, 2)[:, gch]).reshape(B, h, w, 18)
    conv = vo.pad_conv(torch.from_numpy(x), torch.from_numpy(Wp), torch.from_numpy(b), 1, 1)
    for prev in (None, rng.standard_normal((B, (h + 1) // 2, (w + 1) // 2, 2))):
        flow = conv if prev is None else conv + 2.0 * vo.resize_bilinear_legacy(torch.from_numpy(prev), h, w)
        for oh in (2 * h - 1, 2 * h):
            for ow in (2 * w - 1, 2 * w):
                r = ref.predict_up_ref(slabs, b, prev, up_w, up_b, (oh, ow))
                assert float((r["flow"] - flow).abs().max()) <= 1e-12 * max(1.0, float(flow.abs().max()))
                up = vo.deconv4x4s2(flow, torch.from_numpy(up_w), torch.from_numpy(up_b), (oh, ow))
                assert r["up"].shape == up.shape and float((r["up"] - up).abs().max()) <= 1e-12 * max(1.0, float(up.abs().max()))
                # the addend count: bias + ks per in-image tap (9 inside, 6 on an edge, 4 in a corner, fewer on a 1-wide axis) [+ 2]
                rows = np.array([sum(0 <= y + d < h for d in (-1, 0, 1)) for y in range(h)])
                cols = np.array([sum(0 <= xx + d < w for d in (-1, 0, 1)) for xx in range(w)])
                want_n = 1 + ks * np.outer(rows, cols) + (0 if prev is None else 2)
                assert np.array_equal(r["n"][0, ..., 0].numpy(), want_n) and np.array_equal(r["n"][1, ..., 1].numpy(), want_n)
                assert bool((r["S"] >= r["flow"].abs() - 1e-12).all())                        # a sum of magnitudes bounds the sum


def test_legacy_coordinates_are_the_oracle_s_and_inexact_where_expected():
    """h = 11 from ph = 6: the scale 6/11 is not a binary fraction, so the fp32 product decides the weights -- the reference takes
    them exactly as the oracle (and the kernel's legacy_coord) does"""
    lo, hi, t = ref.legacy_axis(6, 11)
    olo, ohi, ot = vo._legacy_axis(6, 11)
    assert np.array_equal(lo, olo) and np.array_equal(hi, ohi) and np.array_equal(t.astype(np.float32), ot)
    exact = np.arange(11) * 6.0 / 11.0
    assert np.any(t != exact - np.floor(exact))
    prev = np.random.default_rng(3).standard_normal((2, 6, 7, 2))
    u, mag = ref.legacy_sample(prev, 11, 13)
    assert float((u - vo.resize_bilinear_legacy(torch.from_numpy(prev), 11, 13)).abs().max()) <= 1e-14
    assert bool((mag >= u.abs() - 1e-14).all())
