"""Reference for the gradients of the reference's tf_warp (main:70-130, "main" = main_flownetS_pyramid_noprevloss_dataloader.py),
get_pixel_value (main:44-68) and the flow glue (main:497-498), differentiated by torch.autograd in fp64 -- what TensorFlow's autodiff
gives for the same op sequence: the corner indices come from integer casts and carry no gradient, so the flow enters through the
four weights only, and the weights are those of the CLIPPED corners (outside the image they are negative or above 1).

The sample points, and so every truncation and clip decision, are the HIP kernels' fp32 values x = fl32(xx + fx), y = fl32(yy + fy),
brought into the fp64 graph by the straight-through substitution of tests/st_grad_ref.py (`_st`: the value of the fp32 sum, the
derivative of the fp64 one).  The corners are the kernels': the sample point clamped to [-2, W] (NaN reads as -2) before the
truncation toward zero, x1 = x0 + 1, both clipped into the image.  Everything downstream -- weights, blend, gradients -- is fp64.
`exact=True` drops the substitution: a plain fp64 function of the fp64 inputs, which is what central differences can be taken of.

Besides the gradients, `backward` returns what the tolerances of tests/test_gpu_warp_flow_backward.py are derived from, per gradient
element: the count `n` of contributions and the absolute companion `S`.  d img: n = the taps that address the element (two taps of
one clipped address count twice), S = sum |w| |dout| over them.  d flow: n = C, S_x = sum_c |dout_c| (|y1f - y| (|Ic| + |Ia|) +
|y - y0f| (|Id| + |Ib|)) and likewise S_y.  `get_pixel_value_backward` and `flow_resize_scale_backward` do the same for the other two
adjoints."""
import numpy as np
import torch

from oracle import vstab_oracle as vo
from tests.st_grad_ref import _st
from tests.warp_grad_ref import _leaf


class Sampled:
    """One forward through the graph: `out` (fp64, [B,H,W,C]) and what `backward` needs."""


def warp(img, flow, exact=False):
    """-> (Sampled with out [B,H,W,C], leaves (img64, flow64))"""
    img64, fl64 = _leaf(img, exact), _leaf(flow, exact)
    B, H, W, C = img64.shape
    gx = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    gy = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    x, y = gx + fl64[..., 0], gy + fl64[..., 1]
    if not exact:
        f32 = fl64.detach().float()
        x, y = _st(x, gx.float() + f32[..., 0]), _st(y, gy.float() + f32[..., 1])

    def corners(v, n):
        lo = torch.trunc(torch.nan_to_num(v.detach(), nan=-2.0).clamp(-2.0, float(n))).long()
        return lo.clamp(0, n - 1), (lo + 1).clamp(0, n - 1)

    x0, x1 = corners(x, W)
    y0, y1 = corners(y, H)
    x0f, x1f, y0f, y1f = (t.double() for t in (x0, x1, y0, y1))
    ax1, ax0, ay1, ay0 = (x1f - x).unsqueeze(-1), (x - x0f).unsqueeze(-1), (y1f - y).unsqueeze(-1), (y - y0f).unsqueeze(-1)
    wts = [ax1 * ay1, ax1 * ay0, ax0 * ay1, ax0 * ay0]                                     # a, b, c, d
    bidx = torch.arange(B).view(B, 1, 1)
    idx = [(bidx * H + yi) * W + xi for yi, xi in ((y0, x0), (y1, x0), (y0, x1), (y1, x1))]
    vec = img64.reshape(-1, C)
    taps = [vec[i] for i in idx]
    out = wts[0] * taps[0] + wts[1] * taps[1] + wts[2] * taps[2] + wts[3] * taps[3]
    s = Sampled()
    s.out, s.shape = out, (B, H, W, C)
    s.idx, s.wts, s.taps = idx, [w.detach() for w in wts], [t.detach() for t in taps]
    s.axes = tuple(a.detach() for a in (ax1, ax0, ay1, ay0))
    s.x, s.y, s.corners = x.detach(), y.detach(), (x0, x1, y0, y1)
    return s, (img64, fl64)


def backward(s, leaves, dout):
    """Gradients of sum(out * dout) by autograd, and the counts / absolute companions of the module docstring.
    Keys: d_img, n_img, S_img ([B,H,W,C]); d_flow, S_flow ([B,H,W,2]); n_flow (= C)."""
    B, H, W, C = s.shape
    dout = torch.as_tensor(dout).double().reshape(s.out.shape)
    d_img, d_flow = torch.autograd.grad(s.out, leaves, dout)
    ad = dout.abs()
    n_img = torch.zeros(B * H * W, dtype=torch.float64)
    S_img = torch.zeros(B * H * W, C, dtype=torch.float64)
    for w, i in zip(s.wts, s.idx):
        n_img.index_add_(0, i.reshape(-1), torch.ones(i.numel(), dtype=torch.float64))
        S_img.index_add_(0, i.reshape(-1), (w.abs() * ad).reshape(-1, C))
    aIa, aIb, aIc, aId = (t.abs() for t in s.taps)
    ax1, ax0, ay1, ay0 = (a.abs() for a in s.axes)
    Sx = (ad * (ay1 * (aIc + aIa) + ay0 * (aId + aIb))).sum(-1)
    Sy = (ad * (ax1 * (aIb + aIa) + ax0 * (aId + aIc))).sum(-1)
    return {"d_img": d_img, "n_img": n_img.reshape(B, H, W, 1).expand(B, H, W, C), "S_img": S_img.reshape(B, H, W, C),
            "d_flow": d_flow, "S_flow": torch.stack([Sx, Sy], -1), "n_flow": C}


def get_pixel_value_backward(dout, x, y, Hi, Wi):
    """Adjoint of get_pixel_value with the kernels' clipping of the indices.  Keys: d_img, n_img, S_img ([B,Hi,Wi,C])."""
    dout = torch.as_tensor(dout).double()
    B, H, W, C = dout.shape
    xi, yi = x.long().clamp(0, Wi - 1), y.long().clamp(0, Hi - 1)
    i = ((torch.arange(B).view(B, 1, 1) * Hi + yi) * Wi + xi).reshape(-1)
    d = torch.zeros(B * Hi * Wi, C, dtype=torch.float64).index_add_(0, i, dout.reshape(-1, C))
    S = torch.zeros(B * Hi * Wi, C, dtype=torch.float64).index_add_(0, i, dout.abs().reshape(-1, C))
    n = torch.zeros(B * Hi * Wi, dtype=torch.float64).index_add_(0, i, torch.ones(i.numel(), dtype=torch.float64))
    return {"d_img": d.reshape(B, Hi, Wi, C), "S_img": S.reshape(B, Hi, Wi, C), "n_img": n.reshape(B, Hi, Wi, 1).expand(B, Hi, Wi, C)}


def glue(pf, net_h, net_w, oh, ow):
    """main:497-498 on an fp64 graph tensor: vo.resize_bilinear_legacy (its fp32 interpolation weights) with the scalings"""
    h = pf.shape[1]
    f = vo.resize_bilinear_legacy(pf * net_h / h, oh, ow)
    return torch.stack([f[..., 0] * ow / net_w, f[..., 1] * oh / net_h], 3)


def flow_resize_scale_backward(dout, in_hw, net_h, net_w):
    """Adjoint of the glue by fp64 autograd.  Keys: d_flow, S_flow, n_flow ([B,h,w,2]); n counts the output pixels whose interpolation
    weight on the element is not zero, S is the adjoint applied to |dout| (the weights and scalings are non-negative)."""
    dout = torch.as_tensor(dout).double()
    B, oh, ow, _ = dout.shape
    h, w = in_hw
    pf = torch.zeros(B, h, w, 2, dtype=torch.float64, requires_grad=True)
    out = glue(pf, net_h, net_w, oh, ow)
    (d,) = torch.autograd.grad(out, pf, dout, retain_graph=True)
    (S,) = torch.autograd.grad(out, pf, dout.abs())

    def count(n_in, n_out):
        if n_in == n_out:
            return np.ones(n_in)
        lo, hi, t = vo._legacy_axis(n_in, n_out)
        c = np.zeros(n_in)
        np.add.at(c, lo[(1.0 - t != 0) | ((hi == lo) & (t != 0))], 1)
        np.add.at(c, hi[(t != 0) & (hi != lo)], 1)
        return c

    n = torch.from_numpy(np.outer(count(h, oh), count(w, ow))).view(1, h, w, 1).expand(B, h, w, 2)
    return {"d_flow": d, "S_flow": S, "n_flow": n}
