"""The rest of spatial_transformer.py without a GPU: the drop-in's import surface (the reference's main:4 and cell.py:2 import
lines), the host inversion of the thin-plate spline's L, and known answers of the numpy restatement the GPU tests compare to."""
import ctypes as C

import numpy as np
import pytest

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib
from tests import st_extended_ref as ref


def test_reference_import_lines_resolve_against_the_drop_in():
    # main_flownetS_pyramid*.py:4 and flownet_trainer.py:4, then cell.py:2, with the module name pointed at the drop-in
    from coupe.optical_flow_based_deep_video_stabilization_amd.spatial_transformer import (  # noqa: F401
        ProjectiveSymmetryTransformer, ProjectiveTransformer, AffineSymmetryTransformer, SimilarityTransformer)
    from coupe.optical_flow_based_deep_video_stabilization_amd.spatial_transformer import ElasticTransformer  # noqa: F401
    from coupe.optical_flow_based_deep_video_stabilization_amd import spatial_transformer as st
    for name in ("bicubic_interp", "bilinear_interp", "_interpolate", "_meshgrid", "_repeat", "transformer", "AffineTransformer"):
        assert callable(getattr(st, name))
    assert SimilarityTransformer((8, 8)).param_dim == 4 and AffineSymmetryTransformer((8, 8)).param_dim == 6
    assert ProjectiveSymmetryTransformer((8, 8)).param_dim == 8


def _linv(g):
    K = g * g
    buf = (C.c_float * (K * (K + 3)))()
    code = _lib.lib().vstab_host_tps_linv(g, buf, K * (K + 3))
    return code, np.frombuffer(buf, dtype=np.float32).reshape(K, K + 3).copy()


@pytest.mark.parametrize("g", [2, 3, 4, 5, 6])
def test_host_tps_linv_matches_numpy_inverse(g):
    code, got = _linv(g)
    assert code == 0
    want = ref.tps_linv_t(g)
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()


def test_host_tps_linv_refuses_bad_arguments():
    L = _lib.lib()
    buf = (C.c_float * 64)()
    assert L.vstab_host_tps_linv(1, buf, 64) == -1               # g = 1: L is singular
    assert L.vstab_host_tps_linv(0, buf, 64) == -1
    assert L.vstab_host_tps_linv(17, buf, 64) == -1              # beyond VSTAB_TPS_GMAX
    assert L.vstab_host_tps_linv(3, buf, 10) == -4               # 9 x 12 floats do not fit
    assert L.vstab_host_tps_linv(2, None, 64) == -6
    assert b"host_tps_linv" in L.vstab_last_error(None)


def test_bicubic_restatement_returns_pixels_at_integer_coordinates():
    rng = np.random.default_rng(0)
    im = rng.random((2, 9, 5, 3), dtype=np.float32)
    ix, iy = np.meshgrid(np.arange(5), np.arange(9))
    x = (ix / 4.0 * 2 - 1).astype(np.float32)           # W-1, H-1 powers of two: (x+1)/2*(W-1) lands exactly on the integers
    y = (iy / 8.0 * 2 - 1).astype(np.float32)
    xs, ys = np.tile(x.reshape(-1), 2), np.tile(y.reshape(-1), 2)
    assert np.array_equal(((xs[:45] + 1) / 2 * 4), ix.reshape(-1).astype(np.float32))
    out = ref.bicubic_interp(im, xs, ys, (9, 5)).reshape(2, 9, 5, 3)
    assert np.array_equal(out, im)


def test_bicubic_weights_known_answers():
    w = [float(v) for v in ref.cubic_weights(np.float32(0.5))]
    assert w == [0.59375, -0.09375, 0.59375, -0.09375]
    assert [float(v) for v in ref.cubic_weights(np.float32(0.0))] == [1.0, 0.0, 0.0, 0.0]
    t = np.linspace(0, 1, 101, dtype=np.float32)
    assert np.abs(sum(ref.cubic_weights(t)) - 1).max() <= 1e-6          # a partition of unity
    taps, _ = ref.cubic_axis(np.array([-1, 1, np.nan, np.inf, -np.inf, 3.0], np.float32), 6)
    assert [list(map(int, t)) for t in zip(*taps)] == [[0, 0, 1, 2], [5, 4, 5, 5], [0, 0, 1, 2], [5, 4, 5, 5], [0, 0, 1, 2],
                                                       [5, 4, 5, 5]]


@pytest.mark.parametrize("n", [100, 137, 211])
def test_symmetric_pad_index_map_is_numpys(n):
    src = np.arange(n)
    want = np.pad(src, (100, 100), mode='symmetric')
    assert np.array_equal(src[ref.refl(np.arange(n + 200) - 100, n)], want)


def test_crop_or_pad_offsets():
    a = np.arange(2 * 7 * 5 * 1, dtype=np.float32).reshape(2, 7, 5, 1)
    out = ref.crop_or_pad(a, 3, 9)                 # crop 2 rows from the top (7-3)//2, pad 2 columns on the left (9-5)//2
    assert np.array_equal(out[:, :, 2:7], a[:, 2:5])
    assert not out[:, :, :2].any() and not out[:, :, 7:].any()


@pytest.mark.parametrize("g", [2, 3, 4, 5])
def test_tps_zero_theta_is_the_identity(g):
    theta = np.zeros((1, 2 * g * g), np.float32)
    xt, yt = ref.grid(9, 13)
    xs, ys, _, _ = ref.tps_coords(theta, g, (9, 13), ref.tps_linv_t(g))          # the exact (fp64) L_inv
    assert np.abs(xs[0] - xt).max() <= 1e-6 and np.abs(ys[0] - yt).max() <= 1e-6
    # the fp32 table the kernels use: each entry is within 2^-24 relative of the exact one, so the map moves by at most
    # 2^-24 * sum_j sum_k |P_k| |L_inv_kj| |R_j| (the third return of tps_coords) -- up to ~2e-6 at g = 4, 6
    _, linv = _linv(g)
    xs, ys, _, Tcoef = ref.tps_coords(theta, g, (9, 13), linv)
    bound = 2.0 ** -24 * Tcoef[0] * 1.01 + 1e-12
    assert (np.abs(xs[0] - xt) <= bound[0]).all() and (np.abs(ys[0] - yt) <= bound[1]).all()


def test_similarity_premap_interleaves_for_batches():
    th = np.array([[0.3, 0.2, 0.1, -0.1], [-0.5, 0.4, 0.3, 0.2]], np.float32)
    M = ref.sym_theta('similarity', th)
    a, s = th[:, 0] * np.float32(3.14 / 6), th[:, 1] * np.float32(0.1) + np.float32(1)
    # six [B] vectors on axis 0, reshaped [B, 6]: sample 0 takes s cos a and s sin a of both samples, then tx of both
    assert np.allclose(M[0], [s[0] * np.cos(a[0]), s[1] * np.cos(a[1]), s[0] * np.sin(a[0]), s[1] * np.sin(a[1]),
                              th[0, 2] * 0.2, th[1, 2] * 0.2], atol=1e-7)
