"""The reference of the tf_warp / get_pixel_value / flow-glue gradients (tests/warp_flow_grad_ref.py) checked on the CPU: its forward
is the oracle's tf_warp, hand-derived answers on a 2 x 3 image, and fp64 central differences of its plain fp64 form."""
import torch

from oracle import vstab_oracle as vo
from tests import warp_flow_grad_ref as ref


def _flows(B, H, W, seed, spread=2):
    """flows whose sample points have fractional parts in [0.1, 0.9]: whole-pixel offsets in [-spread, spread] (so the first and last
    rows / columns sample outside the image) plus a fraction; every sample point is at least 0.1 from a whole number, and so from
    the lines x in {-1, W-1}, y in {-1, H-1} where tf_warp is discontinuous"""
    g = torch.Generator().manual_seed(seed)
    whole = torch.randint(-spread, spread + 1, (B, H, W, 2), generator=g).double()
    return whole + 0.1 + 0.8 * torch.rand(B, H, W, 2, generator=g, dtype=torch.float64)


def test_forward_is_the_oracles_tf_warp():
    B, H, W, C = 2, 7, 9, 3
    g = torch.Generator().manual_seed(3)
    img = torch.rand(B, H, W, C, generator=g)
    for flow in (_flows(B, H, W, 4).float(), 3.0 * torch.randn(B, H, W, 2, generator=g), torch.zeros(B, H, W, 2)):
        s, _ = ref.warp(img, flow)
        want = vo.tf_warp(img, flow, H, W, torch.float64)
        assert s.out.shape == want.shape and torch.allclose(s.out.detach(), want, rtol=1e-14, atol=1e-15)


IMG = torch.tensor([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]]).view(1, 2, 3, 1)


def _one_pixel(yy, xx, fx, fy, g=3.0):
    """all flows zero but pixel (yy, xx)'s, dout = g there and 0 elsewhere -> (out at the pixel, d_img [2,3], d_flow at the pixel, Sampled)"""
    flow = torch.zeros(1, 2, 3, 2)
    flow[0, yy, xx] = torch.tensor([fx, fy])
    dout = torch.zeros(1, 2, 3, 1)
    dout[0, yy, xx, 0] = g
    s, leaves = ref.warp(IMG, flow)
    r = ref.backward(s, leaves, dout)
    assert bool((r["d_flow"][0][dout[0, ..., 0] == 0] == 0).all())                 # a pixel's flow moves that pixel alone
    return float(s.out.detach()[0, yy, xx, 0]), r["d_img"][0, ..., 0], r["d_flow"][0, yy, xx], s, r


def test_known_answer_inside():
    # pixel (0,0) sampling (x, y) = (0.25, 0.5): corners (0,1) x (0,1), weights .375 .375 .125 .125
    out, d_img, d_flow, _, r = _one_pixel(0, 0, 0.25, 0.5)
    assert out == 0.375 * 1 + 0.375 * 8 + 0.125 * 2 + 0.125 * 16
    assert torch.equal(d_img, 3.0 * torch.tensor([[0.375, 0.125, 0.0], [0.375, 0.125, 0.0]], dtype=torch.float64))
    # d_fx = (y1f-y)(Ic-Ia) + (y-y0f)(Id-Ib) = .5 (2-1) + .5 (16-8); d_fy = (x1f-x)(Ib-Ia) + (x-x0f)(Id-Ic) = .75 (8-1) + .25 (16-2)
    assert d_flow.tolist() == [3.0 * 4.5, 3.0 * 8.75]
    assert r["S_flow"][0, 0, 0].tolist() == [3.0 * (0.5 * 3 + 0.5 * 24), 3.0 * (0.75 * 9 + 0.25 * 18)]
    assert torch.equal(r["S_img"][0, ..., 0], 3.0 * torch.tensor([[0.375, 0.125, 0.0], [0.375, 0.125, 0.0]], dtype=torch.float64))
    assert float(r["n_img"][..., 0].sum()) == 4 * 6                                 # every pixel's four taps are counted, weight 0 or not


def test_known_answer_negative_fraction():
    # pixel (0,0) sampling x = -0.25, y = 0: truncation toward zero gives x0 = 0, x1 = 1 (not -1, 0): wa = 1.25 > 1, wc = -0.25 < 0
    out, d_img, d_flow, s, _ = _one_pixel(0, 0, -0.25, 0.0)
    assert [int(c[0, 0, 0]) for c in s.corners] == [0, 1, 0, 1]
    assert float(s.wts[0][0, 0, 0]) == 1.25 and float(s.wts[2][0, 0, 0]) == -0.25
    assert out == 1.25 * 1 - 0.25 * 2                                               # the linear extrapolation to the left
    assert torch.equal(d_img, 3.0 * torch.tensor([[1.25, -0.25, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64))
    # d_fx = 1 (2-1) + 0; d_fy = 1.25 (8-1) - 0.25 (16-2)
    assert d_flow.tolist() == [3.0 * 1.0, 3.0 * (1.25 * 7 - 0.25 * 14)]


def test_known_answer_beyond_the_last_column():
    # pixel (1,2) sampling x = 3.5, y = 0.5: both x corners clip to column 2, the weights are -.75 -.75 +.75 +.75 and cancel
    out, d_img, d_flow, s, r = _one_pixel(1, 2, 1.5, -0.5)
    assert [int(c[0, 1, 2]) for c in s.corners] == [2, 2, 0, 1]
    assert [float(w[0, 1, 2]) for w in s.wts] == [-0.75, -0.75, 0.75, 0.75]
    assert out == 0.0 and bool((d_img == 0).all()) and d_flow.tolist() == [0.0, 0.0]
    base = ref.backward(*ref.warp(IMG, torch.zeros(1, 2, 3, 2)), torch.zeros(1, 2, 3, 1))["n_img"][0, ..., 0]
    # pixel (1,2) at rest taps (1,2) four times (both axes clipped at the corner); displaced, each of (0,2) and (1,2) twice
    assert torch.equal(r["n_img"][0, ..., 0] - base, torch.tensor([[0.0, 0, 2], [0, 0, -2]], dtype=torch.float64))
    assert torch.equal(r["S_img"][0, ..., 0], torch.tensor([[0.0, 0, 4.5], [0, 0, 4.5]], dtype=torch.float64))


def test_central_differences():
    """fp64 central differences of the plain fp64 function against the reference's d_flow and d_img.  tf_warp is bilinear inside
    one set of corners, so the differences are exact up to rounding wherever no sample point crosses a whole number: the flows keep
    every fractional part in [0.1, 0.9], and warp_discontinuity_mask must exclude no pixel."""
    B, H, W, C = 2, 5, 6, 2
    g = torch.Generator().manual_seed(11)
    img = torch.rand(B, H, W, C, generator=g, dtype=torch.float64)
    dout = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    flow = _flows(B, H, W, 12)
    frac = (flow + torch.stack(torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")[::-1], -1).double()) % 1.0
    assert float(frac.min()) >= 0.1 - 1e-12 and float(frac.max()) <= 0.9 + 1e-12
    assert bool(vo.warp_discontinuity_mask(flow, H, W).all())                      # a condition of the test: zero pixels excluded
    s, leaves = ref.warp(img, flow, exact=True)
    xs, ys = s.x, s.y
    assert bool((xs < 0).any() and (xs > W - 1).any() and (ys < 0).any() and (ys > H - 1).any())    # both clipped branches are met
    r = ref.backward(s, leaves, dout)

    def f(i, fl):
        return ref.warp(i, fl, exact=True)[0].out.detach()

    h = 1e-6
    for k in range(2):
        e = torch.zeros(2, dtype=torch.float64)
        e[k] = h
        num = ((f(img, flow + e) - f(img, flow - e)) * dout).sum(-1) / (2 * h)     # a pixel's flow moves that pixel alone
        assert torch.allclose(num, r["d_flow"][..., k], rtol=1e-7, atol=1e-8), float((num - r["d_flow"][..., k]).abs().max())
    num = torch.zeros_like(img)
    flat = num.view(-1)
    for i in range(img.numel()):                                                    # linear in the image: any step is exact
        e = torch.zeros(img.numel(), dtype=torch.float64)
        e[i] = 0.5
        e = e.view(img.shape)
        flat[i] = ((f(img + e, flow) - f(img - e, flow)) * dout).sum()
    assert torch.allclose(num, r["d_img"], rtol=1e-12, atol=1e-13), float((num - r["d_img"]).abs().max())


def test_get_pixel_value_and_glue_adjoints_are_adjoints():
    """<J v, u> = <v, J^T u> in fp64 for the two linear maps"""
    g = torch.Generator().manual_seed(21)
    B, Hi, Wi, C, H, W = 2, 4, 5, 3, 3, 6
    img = torch.rand(B, Hi, Wi, C, generator=g, dtype=torch.float64)
    x, y = torch.randint(-2, Wi + 2, (B, H, W), generator=g), torch.randint(-2, Hi + 2, (B, H, W), generator=g)
    u = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    r = ref.get_pixel_value_backward(u, x, y, Hi, Wi)
    fwd = vo.get_pixel_value(img, x.clamp(0, Wi - 1), y.clamp(0, Hi - 1))
    assert torch.allclose((fwd * u).sum(), (img * r["d_img"]).sum(), rtol=1e-13)
    assert float(r["n_img"][..., 0].sum()) == B * H * W
    for (h, w), (oh, ow) in (((9, 13), (37, 45)), ((30, 41), (11, 17)), ((6, 7), (6, 7))):
        pf = torch.randn(B, h, w, 2, generator=g, dtype=torch.float64)
        u = torch.randn(B, oh, ow, 2, generator=g, dtype=torch.float64)
        r = ref.flow_resize_scale_backward(u, (h, w), 384, 512)
        assert torch.allclose((ref.glue(pf, 384, 512, oh, ow) * u).sum(), (pf * r["d_flow"]).sum(), rtol=1e-12)
        assert torch.allclose(ref.glue(pf, 384, 512, oh, ow), vo.flow_to_output_res(pf, 384, 512, oh, ow), rtol=1e-13, atol=1e-13)
        assert bool((r["n_flow"] >= 0).all()) and bool(((r["S_flow"] > 0) <= (r["n_flow"] > 0)).all())
