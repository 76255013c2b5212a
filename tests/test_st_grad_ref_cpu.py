"""Pins tests/st_grad_ref.py, the reference of the spatial transformers' gradients, on the CPU: its forward is the oracle's, its
autograd gradients are the central differences of the function it states, and the clip's gradient rule gives the known answers."""
import numpy as np
import pytest
import torch

from oracle import vstab_oracle as vo
from tests import st_grad_ref as ref

AFFINE = [[0.9317, 0.2113, 0.0313, -0.1731, 1.0419, -0.0527], [1.1213, -0.3071, -0.2037, 0.2639, 0.8811, 0.1319]]
PROJECTIVE = [AFFINE[0] + [0.1103, -0.0709], AFFINE[1] + [-0.2011, 0.1607]]
# a third of the grid outside the image; z crossing zero inside the grid
WILD = {"outside": [[1.9, 0.0, 0.8, 0.0, 1.1, 0.0], [1.0, 0.5, 0.0, -0.4, 2.2, -0.9]],
        "z_cross": [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.5, 0.5], [0.9, 0.1, 0.0, 0.1, 1.1, 0.0, -0.8, 1.3]]}


def _img(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("theta", [AFFINE, PROJECTIVE, WILD["outside"], WILD["z_cross"]])
def test_forward_is_the_oracles(theta):
    im = _img((2, 9, 11, 3), 1)
    s, _ = ref.transform(im, torch.tensor(theta), (7, 8))
    want = vo.st_transform(im.double(), torch.tensor(theta), (7, 8), dtype=torch.float64, matmul="unfused")
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(s.out), fin)
    assert float((s.out.detach()[fin] - want[fin]).abs().max()) <= 1e-14


def test_interp_forward_is_the_oracles():
    im = _img((2, 6, 5, 4), 2)
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(2 * 4 * 7, generator=g) * 3 - 1.5, torch.rand(2 * 4 * 7, generator=g) * 3 - 1.5
    x[:5] = torch.tensor([float("nan"), -1.5, 1.5, float("inf"), -float("inf")])
    xo, yo = torch.where(torch.isnan(x), torch.tensor(-9.0), x), y          # the oracle's clamp keeps NaN; the kernels read it as -1
    s, _ = ref.bilinear_interp(im, x, y, (4, 7))
    want = vo.st_bilinear_interp(im.double(), xo, yo, (4, 7), dtype=torch.float64)
    assert float((s.out.detach() - want).abs().max()) <= 1e-14


def _margin(v, n):
    """distance of the padded pixel coordinates from the nearest integer (the clip bounds 0 and n + 1 are integers)"""
    p = (v.detach() + 1.0) / 2.0 * (n - 1) + 1.0
    return float((p - torch.round(p)).abs().min())


def _central(f, leaf, h):
    g = torch.zeros_like(leaf)
    flat = leaf.detach().clone().reshape(-1)
    for i in range(flat.numel()):
        a, b = flat.clone(), flat.clone()
        a[i] += h
        b[i] -= h
        g.reshape(-1)[i] = (f(a.reshape(leaf.shape)) - f(b.reshape(leaf.shape))) / (2 * h)
    return g


@pytest.mark.parametrize("theta", [AFFINE, PROJECTIVE])
def test_transform_gradients_are_central_differences(theta):
    """Hand-picked thetas (rotation, zoom, shift, perspective) on a 7 x 8 grid over a 9 x 11 image; the margin assertion states
    what makes central differences valid: no coordinate within 100 steps (times the pixels per unit) of an integer (the clip bounds are integers)."""
    H, W, out = 9, 11, (7, 8)
    im, th = _img((2, H, W, 3), 4).double(), torch.tensor(theta, dtype=torch.float64)
    dout = torch.randn(2, 7, 8, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    h = 1e-7
    s, (im64, th64) = ref.transform(im, th, out, exact=True)
    # the coordinates the sampler saw: recompute them from the graph's inputs
    grid = torch.from_numpy(vo.st_meshgrid(out)).reshape(3, -1).double()
    T = th.reshape(2, -1)
    xs = T[:, 0:1] * grid[0] + T[:, 1:2] * grid[1] + T[:, 2:3]
    ys = T[:, 3:4] * grid[0] + T[:, 4:5] * grid[1] + T[:, 5:6]
    if T.shape[1] == 8:
        z = T[:, 6:7] * grid[0] + T[:, 7:8] * grid[1] + 1.0
        xs, ys = xs / z, ys / z
    assert min(_margin(xs, W), _margin(ys, H)) > 100 * h * max(H, W)
    r = ref.backward(s, (im64, th64), dout)

    def f_theta(t):
        return float((ref.transform(im, t, out, exact=True)[0].out.detach() * dout).sum())

    def f_img(i):
        return float((ref.transform(i, th, out, exact=True)[0].out.detach() * dout).sum())

    assert float((r["d_theta"] - _central(f_theta, th, h)).abs().max()) <= 1e-6
    assert float((r["d_img"] - _central(f_img, im, h)).abs().max()) <= 1e-6
    assert (r["S_theta"] >= r["d_theta"].abs() - 1e-12).all() and (r["S_img"] >= r["d_img"].abs() - 1e-12).all()


def test_interp_gradients_are_central_differences():
    """Coordinates built as pixel k + a fraction in [0.2, 0.8], k from -2 (beyond the clip) to n (beyond it on the other side)."""
    B, H, W, C, out = 1, 5, 6, 2, (3, 8)
    n = out[0] * out[1]
    k = torch.arange(n, dtype=torch.float64)
    xp = (k % (W + 3)) - 2.0 + 0.2 + 0.6 * ((k * 7) % 5) / 4.0             # pixel coordinates, un-padded
    yp = ((k * 3) % (H + 3)) - 2.0 + 0.2 + 0.6 * ((k * 11) % 7) / 6.0
    x, y = xp * 2.0 / (W - 1) - 1.0, yp * 2.0 / (H - 1) - 1.0
    assert min(_margin(x, W), _margin(y, H)) > 0.19
    im = _img((B, H, W, C), 6).double()
    dout = torch.randn(n, C, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    s, leaves = ref.bilinear_interp(im, x, y, out, exact=True)
    r = ref.backward(s, leaves, dout)
    h = 1e-6
    fx = lambda t: float((ref.bilinear_interp(im, t, y, out, exact=True)[0].out.detach() * dout).sum())       # noqa: E731
    fy = lambda t: float((ref.bilinear_interp(im, x, t, out, exact=True)[0].out.detach() * dout).sum())       # noqa: E731
    fi = lambda t: float((ref.bilinear_interp(t, x, y, out, exact=True)[0].out.detach() * dout).sum())        # noqa: E731
    assert float((r["d_x"] - _central(fx, x, h)).abs().max()) <= 1e-6
    assert float((r["d_y"] - _central(fy, y, h)).abs().max()) <= 1e-6
    assert float((r["d_img"] - _central(fi, im, h)).abs().max()) <= 1e-6
    assert (r["d_x"][xp < -1] == 0).all() and (r["d_x"][xp > W] == 0).all() and int((r["d_x"] != 0).sum()) >= n // 3
    assert (r["S_x"] >= r["d_x"].abs() - 1e-12).all() and (r["S_y"] >= r["d_y"].abs() - 1e-12).all()
    rows, cols = [(i % ((W + 2) * (H + 2))) // (W + 2) for i in s.idx], [i % (W + 2) for i in s.idx]
    valid = sum(int(((rw >= 1) & (rw <= H) & (cl >= 1) & (cl <= W)).sum()) for rw, cl in zip(rows, cols))
    assert float(r["n_img"][..., 0].sum()) == valid               # every tap inside the image counts once, border taps never


def test_clip_bound_rule_known_answers():
    """W = 5: x = -1.5 is pixel -1 exactly, x = 1.5 pixel W exactly (both exact in fp32).  At exactly -1 the gradient passes:
    d out / d x = I[., 0] * (W - 1) / 2 for a pixel on row 0 (y = -1 -> pixel 0).  At exactly W the clip passes too, but both
    taps lie on the zero border, so the slope is 0 either way; `pass_x` shows the rule.  One step beyond either bound, and
    NaN: blocked, gradient 0."""
    W = H = 5
    im = torch.arange(1.0, 1.0 + H * W).reshape(1, H, W, 1)
    x = torch.tensor([-1.5, 1.5, -1.75, 1.75, float("nan"), float(np.nextafter(np.float32(-1.5), np.float32(-2))),
                      1.5000005])                                          # 1.5 + 1 ulp would round back to pixel 5.0 in the fp32 (x + 1)
    y = torch.full_like(x, -1.0)
    s, leaves = ref.bilinear_interp(im, x, y, (1, 7))
    assert s.pass_x.tolist() == [True, True, False, False, False, False, False]
    r = ref.backward(s, leaves, torch.ones(7, 1))
    assert r["d_x"].tolist() == [1.0 * (W - 1) / 2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert r["S_x"].tolist() == [1.0 * (W - 1) / 2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    # the same rule on the y axis, and an interior pixel for scale: x = 0 -> pixel 2, slope I[0,3] - I[0,2] = 1
    s, leaves = ref.bilinear_interp(im, torch.tensor([0.0, 0.0]), torch.tensor([-1.5, -1.75]), (1, 2))
    r = ref.backward(s, leaves, torch.ones(2, 1))
    assert s.pass_y.tolist() == [True, False]
    assert r["d_y"].tolist() == [3.0 * (H - 1) / 2, 0.0] and r["d_x"].tolist() == [0.0, 0.0]
