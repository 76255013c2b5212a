"""tests/st_tps_grad_ref.py checked on the CPU: its exact (plain fp64) mode against central differences, its coordinates against
tests/st_extended_ref.py's, and its chain (given coordinates) against autograd through the exact mode."""
import ctypes

import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib
from tests import st_extended_ref as xref
from tests import st_tps_grad_ref as ref

H, W, OUT, C = 9, 11, (7, 8), 2


def _linv(g):
    """The library's fp32 table (vstab_host_tps_linv runs on the host)."""
    K = g * g
    buf = np.empty((K, K + 3), dtype=np.float32)
    _lib.check(_lib.lib().vstab_host_tps_linv(g, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), buf.size))
    return buf


def _case(g, B=2):
    gen = torch.Generator().manual_seed(40 + g)
    im = torch.rand(B, H, W, C, generator=gen, dtype=torch.float64)
    theta = 0.08 * torch.randn(B, 2 * g * g, generator=gen, dtype=torch.float64)
    dout = torch.randn(B, OUT[0], OUT[1], C, generator=gen, dtype=torch.float64)
    return im, theta, dout


def _loss(im, theta, dout, g, linv):
    out, _ = ref.elastic_exact(im, theta, g, OUT, linv)
    return float((out.detach() * dout).sum())


@pytest.mark.parametrize("g", [2, 3])
def test_exact_mode_agrees_with_central_differences(g):
    linv = _linv(g)
    im, theta, dout = _case(g)
    xs, ys = ref.coords64(theta, g, OUT, linv, exact=True)
    # no pixel coordinate sits within 1e-4 of an integer: a step of 1e-6 in one offset moves a coordinate by less than 1e-5 pixel
    # (|d x_s / d theta| <= sum_j |linv_t R_j|, a few units, times (n - 1) / 2 <= 5), so a central difference crosses no floor
    for v, n in ((xs, W), (ys, H)):
        p = (v + 1.0) / 2.0 * (n - 1)
        assert float((p - p.round()).abs().min()) > 1e-4
        assert float(p.min()) > -1.0 and float(p.max()) < n          # inside the clip: every pixel passes a gradient
    out, leaves = ref.elastic_exact(im, theta, g, OUT, linv)
    d_im, d_th = torch.autograd.grad(out, leaves, dout)
    h = 1e-6
    for i in range(theta.numel()):
        e = torch.zeros_like(theta).reshape(-1)
        e[i] = h
        e = e.reshape(theta.shape)
        fd = (_loss(im, theta + e, dout, g, linv) - _loss(im, theta - e, dout, g, linv)) / (2 * h)
        assert abs(fd - float(d_th.reshape(-1)[i])) <= 1e-6 * max(1.0, abs(fd)), (i, fd, float(d_th.reshape(-1)[i]))
    idx = torch.randperm(im.numel(), generator=torch.Generator().manual_seed(1))[:40]
    for i in idx.tolist():
        e = torch.zeros_like(im).reshape(-1)
        e[i] = h
        e = e.reshape(im.shape)
        fd = (_loss(im + e, theta, dout, g, linv) - _loss(im - e, theta, dout, g, linv)) / (2 * h)
        assert abs(fd - float(d_im.reshape(-1)[i])) <= 1e-8 * max(1.0, abs(fd)), (i, fd)


@pytest.mark.parametrize("g", [2, 3, 5])
def test_chain_coordinates_equal_the_restatement(g):
    linv = _linv(g)
    theta = 0.15 * torch.randn(2, 2 * g * g, generator=torch.Generator().manual_seed(g))
    xs, ys = ref.coords64(theta, g, OUT, linv)
    wx, wy, _, _ = xref.tps_coords(theta.numpy(), g, OUT, linv)
    np.testing.assert_allclose(xs.numpy(), wx, rtol=0, atol=1e-13)
    np.testing.assert_allclose(ys.numpy(), wy, rtol=0, atol=1e-13)


@pytest.mark.parametrize("g", [2, 3])
def test_chain_on_given_coordinates_is_autograd_through_the_exact_mode(g):
    """Fed the exact mode's own coordinates rounded to fp32, the chain of `backward` reproduces autograd's d theta up to what
    that rounding moves (the coordinates by 2^-24, the weights with them), and the companion S_theta dominates |d theta|."""
    linv = _linv(g)
    im, theta, dout = _case(g)
    theta = theta.float().double()
    out, leaves = ref.elastic_exact(im, theta, g, OUT, linv)
    d_im, d_th = torch.autograd.grad(out, leaves, dout)
    xs, ys = ref.coords64(theta, g, OUT, linv, exact=True)
    s, lv = ref.elastic(im, xs.reshape(-1).float(), ys.reshape(-1).float(), g, OUT)
    r = ref.backward(s, lv, dout, g, linv)
    assert r["d_theta"].shape == (2, 2 * g * g) and r["d_cf"].shape == (2, 2, g * g + 3)
    assert float((r["d_theta"] - d_th).abs().max()) <= 1e-5 * float(d_th.abs().max())
    assert float((r["d_img"] - d_im).abs().max()) <= 1e-5 * float(dout.abs().max())
    assert bool((r["S_theta"] >= r["d_theta"].abs() * (1 - 1e-12)).all())
