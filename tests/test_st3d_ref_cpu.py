"""CPU checks of tests/st3d_ref.py, the reference the GPU tests of the 3-D volume transformer compare against: the restatement
against torch's own 5-D grid_sample, the _meshgrid3d layout, central differences against the autograd gradients, and the ABI's
declarations."""
import os
import re

import torch
import torch.nn.functional as F

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib
from tests import st3d_ref as ref

NEW_SYMBOLS = ("vstab_st3d_meshgrid", "vstab_st3d_bilinear_interp", "vstab_st3d_transform", "vstab_st3d_transform_backward_workspace_bytes",
               "vstab_st3d_transform_backward", "vstab_st3d_bilinear_interp_backward")


def test_restatement_equals_grid_sample_in_fp64():
    """vol 2x3x5x7x2, out (4, 6, 5), coordinates uniform in [-1.6, 1.6]^3: zero padding is edge_size 1 and 2 (a coordinate past the
    clip reads pad on both sides), border padding is edge_size 0."""
    g = torch.Generator().manual_seed(3)
    B, D, H, W, C = 2, 3, 5, 7, 2
    out_size = (4, 6, 5)
    n = B * out_size[0] * out_size[1] * out_size[2]
    vol = torch.rand(B, D, H, W, C, generator=g, dtype=torch.float64)
    x, y, z = (torch.rand(n, generator=g, dtype=torch.float64) * 3.2 - 1.6 for _ in range(3))
    grid = torch.stack([x, y, z], 1).reshape(B, *out_size, 3)
    for e, mode in ((1, "zeros"), (2, "zeros"), (0, "border")):
        got = ref.bilinear_interp3d(vol, x, y, z, out_size, e, torch.float64)
        want = F.grid_sample(vol.permute(0, 4, 1, 2, 3), grid, mode="bilinear", padding_mode=mode, align_corners=True)
        want = want.permute(0, 2, 3, 4, 1).reshape(n, C)
        err = float((got - want).abs().max())
        zero = float((want == 0).double().mean())
        print(f"edge_size {e} vs {mode}: max |diff| {err:.2e}, zero share {zero:.3f}")
        assert err <= 1e-12 * float(vol.abs().max())
        assert zero < 0.5


def test_meshgrid3d_layout():
    od, oh, ow = 3, 4, 5
    g = ref.meshgrid3d((od, oh, ow)).reshape(4, od, oh, ow)
    assert g.dtype == torch.float32
    assert torch.equal(g[0, 1, 2], ref.lin11(ow)) and torch.equal(g[1, 2, :, 3], ref.lin11(oh)) and torch.equal(g[2, :, 1, 1], ref.lin11(od))
    assert bool((g[3] == 1).all())
    assert float(g[0, 0, 0, 0]) == -1.0 and float(g[0, 0, 0, ow - 1]) == 1.0 and float(g[0, 0, 0, 1]) == -0.5
    flat = ref.meshgrid3d((od, oh, ow))
    assert flat.shape == (4 * od * oh * ow,) and torch.equal(flat[:ow], ref.lin11(ow))          # x fastest
    one = ref.meshgrid3d((1, 1, 2)).reshape(4, 2)
    assert one[:, 0].tolist() == [-1.0, -1.0, -1.0, 1.0] and one[:, 1].tolist() == [1.0, -1.0, -1.0, 1.0]      # n == 1: the single value is -1


def _away_from_boundaries(v, n, e, margin):
    """coordinates whose pixel position is `margin` away from every integer (floor boundaries; the clip bounds are integers)"""
    p = (v + 1.0) / 2.0 * (n - 1)
    return (p - p.round()).abs() > margin


def test_central_differences_agree_with_autograd():
    g = torch.Generator().manual_seed(11)
    B, D, H, W, C = 1, 4, 5, 6, 2
    out_size = (2, 3, 4)
    n = B * out_size[0] * out_size[1] * out_size[2]
    vol = torch.rand(B, D, H, W, C, generator=g, dtype=torch.float64)
    dout = torch.randn(n, C, generator=g, dtype=torch.float64)
    x, y, z = (torch.rand(n, generator=g, dtype=torch.float64) * 2.8 - 1.4 for _ in range(3))
    h = 1e-6
    for e in (0, 1, 2):
        keep = _away_from_boundaries(x, W, e, 1e-3) & _away_from_boundaries(y, H, e, 1e-3) & _away_from_boundaries(z, D, e, 1e-3)
        assert int(keep.sum()) > n // 2
        s, leaves = ref.grad_bilinear_interp3d(vol, x, y, z, out_size, e, exact=True)
        r = ref.backward(s, leaves, dout)
        f = lambda xx, yy, zz, vv=vol: float((ref.bilinear_interp3d(vv, xx, yy, zz, out_size, e, torch.float64) * dout).sum())  # noqa: E731
        for name, k in (("d_x", 0), ("d_y", 1), ("d_z", 2)):
            for i in torch.nonzero(keep).reshape(-1)[:12].tolist():
                c = [x.clone(), y.clone(), z.clone()]
                c[k][i] += h
                up = f(*c)
                c[k][i] -= 2 * h
                fd = (up - f(*c)) / (2 * h)
                assert abs(fd - float(r[name][i])) <= 1e-7 * max(1.0, abs(fd)), (e, name, i, fd, float(r[name][i]))
        for idx in ((0, 1, 2, 3, 0), (0, 3, 4, 5, 1), (0, 0, 0, 0, 0)):
            v2 = vol.clone()
            v2[idx] += h
            up = f(x, y, z, v2)
            v2[idx] -= 2 * h
            fd = (up - f(x, y, z, v2)) / (2 * h)
            assert abs(fd - float(r["d_vol"][idx])) <= 1e-7 * max(1.0, abs(fd))
    # theta: a near-identity 3x4 whose grid points stay off the boundaries
    theta = torch.tensor([[0.93, 0.07, -0.05, 0.013, -0.06, 0.91, 0.04, -0.021, 0.03, -0.045, 0.95, 0.017]], dtype=torch.float64)
    out_size = (3, 4, 5)
    dout = torch.randn(B, *out_size, C, generator=g, dtype=torch.float64)
    xs, ys, zs = ref.theta_coords(theta, out_size, B, torch.float64)
    assert bool((_away_from_boundaries(xs, W, 1, 1e-3) & _away_from_boundaries(ys, H, 1, 1e-3) & _away_from_boundaries(zs, D, 1, 1e-3)).all())
    s, leaves = ref.grad_transform(vol, theta, out_size, exact=True)
    r = ref.backward(s, leaves, dout)
    ft = lambda th: float((ref.transform(vol, th, out_size, torch.float64) * dout).sum())  # noqa: E731
    for k in range(12):
        t = theta.clone()
        t[0, k] += h
        up = ft(t)
        t[0, k] -= 2 * h
        fd = (up - ft(t)) / (2 * h)
        assert abs(fd - float(r["d_theta"][0, k])) <= 1e-7 * max(1.0, abs(fd)), (k, fd, float(r["d_theta"][0, k]))


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ref.ROOT, "include", "vstab.h")).read()
    declared = set(re.findall(r"VSTAB_API[^;(]*?\b(vstab_\w+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
    assert all(v >= 1 for v in ref.brick()) and ref.brick()[0] * ref.brick()[1] * ref.brick()[2] == 256
