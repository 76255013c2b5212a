"""tests/st_bicubic_grad_ref.py checked on the CPU: its forward is st_extended_ref.bicubic_interp, its autograd agrees with central
differences of its `exact` form, and it reproduces hand-derived known answers."""
import numpy as np
import torch

from tests import st_bicubic_grad_ref as ref
from tests import st_extended_ref as xref


def _inputs(B=2, H=9, W=11, C=3, oh=7, ow=8, seed=3, span=1.15):
    g = torch.Generator().manual_seed(seed)
    im = torch.rand(B, H, W, C, generator=g)
    n = B * oh * ow
    x, y = (torch.rand(n, generator=g) * 2 - 1) * span, (torch.rand(n, generator=g) * 2 - 1) * span
    return im, x, y, torch.randn(n, C, generator=g), (oh, ow)


def test_forward_is_the_extended_reference():
    """fp64 blends on the fp32 coordinate sequence against the fp32 restatement: within 2^-20 of sum |w||w||I| <= 4.5 * 4.5."""
    im, x, y, _, out = _inputs()
    x[:4] = torch.tensor([-1.0, 1.0, float("nan"), 3.0])
    s, _ = ref.bicubic_interp(im, x, y, out)
    want = xref.bicubic_interp(im.numpy(), x.numpy(), y.numpy(), out)
    assert np.abs(s.out.detach().numpy() - want).max() <= 2.0 ** -20 * 4.5 * 4.5
    for kind_out, got in (("theta", ref.transform(im, torch.tensor([[1.0, 0.1, 0.0, -0.1, 0.9, 0.05]] * 2), out)[0].out),):
        want = xref.transform(im.numpy(), np.array([[1.0, 0.1, 0.0, -0.1, 0.9, 0.05]] * 2, np.float32), out, 'bicubic')
        assert np.abs(got.detach().numpy().reshape(want.shape) - want).max() <= 2.0 ** -20 * 4.5 * 4.5


def test_autograd_agrees_with_central_differences_of_the_exact_function():
    """d x, d y per point and d img on a few pixels.  The interpolant is C^1 across integer coordinates, so only the clip's kink is
    left out: the points within 1e-6 of +-1 (none of the 112 drawn here, asserted under 1 %); points outside [-1, 1] stay in and
    have zero gradient on both sides.  Step 1e-6 in fp64: truncation ~ h^2 |f'''| ~ 1e-10, rounding ~ 1e-16 / 1e-6 = 1e-10."""
    im, x, y, dout, out = _inputs()
    left_out = ((x.abs() - 1).abs() < 1e-6) | ((y.abs() - 1).abs() < 1e-6)
    assert left_out.double().mean() < 0.01
    keep = ~left_out
    s, leaves = ref.bicubic_interp(im, x.double(), y.double(), out, exact=True)
    r = ref.backward(s, leaves, dout)

    def f(im_, x_, y_):
        return (ref.bicubic_interp(im_, x_, y_, out, exact=True)[0].out.detach() * dout.double()).sum(1)

    h = 1e-6
    xd, yd = x.double(), y.double()
    nx = (f(im, xd + h, yd) - f(im, xd - h, yd)) / (2 * h)                      # each point's output depends on its own x only
    ny = (f(im, xd, yd + h) - f(im, xd, yd - h)) / (2 * h)
    assert (r["d_x"] - nx).abs()[keep].max() < 1e-6 and (r["d_y"] - ny).abs()[keep].max() < 1e-6
    assert bool((r["d_x"][x.abs() > 1] == 0).all()) and bool((r["d_y"][y.abs() > 1] == 0).all())
    for (b, i, j, c) in [(0, 0, 0, 0), (1, 4, 5, 2), (0, 8, 10, 1), (1, 0, 10, 0)]:
        e = torch.zeros_like(im.double())
        e[b, i, j, c] = 1.0
        num = float((f(im.double() + h * e, xd, yd) - f(im.double() - h * e, xd, yd)).sum() / (2 * h))
        assert abs(num - float(r["d_img"][b, i, j, c])) < 1e-8
    # the theta chain: autograd through the affine graph against differences in theta
    th = torch.tensor([[0.9, 0.1, 0.02, -0.1, 0.8, -0.03]] * 2, dtype=torch.float64)
    dd = torch.randn(2, out[0], out[1], 3, generator=torch.Generator().manual_seed(1)).double()
    s, leaves = ref.transform(im, th, out, exact=True)
    r = ref.backward(s, leaves, dd)
    for k in range(6):
        e = torch.zeros_like(th)
        e[1, k] = h
        num = float(((ref.transform(im, th + e, out, exact=True)[0].out - ref.transform(im, th - e, out, exact=True)[0].out).detach() * dd).sum() / (2 * h))
        assert abs(num - float(r["d_theta"][1, k])) < 1e-6 * max(1.0, abs(num))


def test_known_answers():
    w, dw, aw, adw = ref.weights(torch.tensor([0.0, 0.5, 0.3, 0.999], dtype=torch.float64))
    assert dw[:, 0].tolist() == [0.0, -0.75, 0.75, 0.0]                           # tap order [x0, x0-1, x0+1, x0+2]
    assert dw[:, 1].tolist() == [-1.3125, 0.1875, 1.3125, -0.1875]
    assert dw.sum(0).abs().max() < 1e-15 and (w.sum(0) - 1).abs().max() < 1e-15   # sum w = 1, so sum w' = 0 for every t
    assert bool((aw >= w.abs()).all()) and bool((adw >= dw.abs()).all())
    # one row, t = 0 at x0 = 2 of W = 5: d out / d v = 0.75 (I[x0+1] - I[x0-1]), times (W - 1) / 2
    im = torch.tensor([3.0, 1.0, 4.0, 1.5, 9.0]).reshape(1, 1, 5, 1)
    s, leaves = ref.bicubic_interp(im, torch.tensor([0.0]), torch.tensor([0.0]), (1, 1))
    r = ref.backward(s, leaves, torch.ones(1, 1))
    assert float(s.out) == 4.0 and float(r["d_x"]) == 0.75 * (1.5 - 1.0) * 2.0 and float(r["d_y"]) == 0.0
    # the clip: zero strictly outside and for NaN, the full gradient at exactly +-1 (x = 1: x0 = W-1, taps W-2, W-1, W-1, W-1)
    xs = torch.tensor([-1.0, 1.0, 1.0 + 2.0 ** -20, -1.5, float("nan")])
    s, leaves = ref.bicubic_interp(im.expand(5, 1, 5, 1), xs, torch.zeros(5), (1, 1))
    r = ref.backward(s, leaves, torch.ones(5, 1))
    assert r["d_x"].tolist() == [0.75 * (1.0 - 3.0) * 2.0, 0.75 * (9.0 - 1.5) * 2.0, 0.0, 0.0, 0.0]
    assert s.out.reshape(-1).tolist() == [3.0, 9.0, 9.0, 3.0, 3.0] and s.pass_x.tolist() == [True, True, False, False, False]
    # the replicated edge taps all add: at x = -1 taps are [0, 0, 1, 2] with weights (1, 0, 0, 0): times the four row taps of H = 1, and the sum is dout
    assert r["n_img"][0, 0, :, 0].tolist() == [8.0, 4.0, 4.0, 0.0, 0.0] and r["d_img"][0, 0, :, 0].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
