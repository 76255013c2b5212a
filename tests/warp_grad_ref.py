"""Reference for the gradients of the reference's warp.py: transformImage / transformCropImage (warp.py:46-86, 89-129) and vec2mtrx
(warp.py:25-43), differentiated by torch.autograd in fp64 -- what TensorFlow's autodiff gives for the same op sequence: floor, ceil and
to_int32 have zero derivative, there is no clip, a tap outside the image reads an appended zero row.  Where a source coordinate is an
exact integer floor == ceil, both taps are the same pixel and that axis' slope is 0.

The coordinate VALUES, and so every floor, ceil and inside decision, are those of the HIP kernels' fp32 sequence: `vo.warp_compose`
for refMtrx . pMtrx, the chain of `vo.warp_transform_image(..., matmul="unfused")` ((m0*X + m1*Y) + m2 with each product and sum
rounded, on the float64 np.linspace grid cast to fp32) and the fp32 division by zh + 1e-8f, brought into the fp64 graph by the
straight-through substitution of tests/st_grad_ref.py (`_st`): the value of the fp32 sequence, the derivative of the fp64 expression.
Everything downstream -- xr, yr, weights, blends, gradients -- is fp64.  `exact=True` drops the substitution: a plain fp64 function,
which is what central differences can be taken of.

Besides the gradients, `backward` returns what the tolerances of tests/test_gpu_warp_backward.py are derived from, per gradient
element: the count `n` of contributions (d img: every tap inside the image counts, two taps of one address twice) and the absolute
companion `S`: the same backward with |dout|, with (|UL| + |UR|) (1 - yr) + (|BL| + |BR|) yr in place of the x slope (likewise for y),
and with the absolute values of the chain factors (1 / |zs|, |xh| / zs^2, |X|, |Y|, |refMtrx|); for d img it is the adjoint applied to
|dout|, the weights being non-negative.  `vec2mtrx_backward` does the same for the Taylor matrix exponential: S is the backward of the
recurrence on |p| with the generator's minus signs made plus, applied to |d P|."""
import numpy as np
import torch

from oracle import vstab_oracle as vo
from tests.st_grad_ref import _st


class Sampled:
    """One forward through the graph: `out` (fp64, [B,oh,ow,C]) and what `backward` needs."""


def grid(oh, ow):
    """warp.py:50-52: np.linspace in float64, cast to fp32; flat [oh*ow] each, x fastest."""
    X, Y = np.meshgrid(np.linspace(-1, 1, ow), np.linspace(-1, 1, oh))
    return torch.from_numpy(X.flatten().astype(np.float32)), torch.from_numpy(Y.flatten().astype(np.float32))


def _leaf(t, exact):
    """data -> a new fp64 leaf (rounded to fp32 first unless `exact`); a tensor already in a graph is used as it is"""
    if torch.is_tensor(t) and t.dtype == torch.float64 and t.requires_grad:
        return t
    t = torch.as_tensor(t)
    return (t.double() if exact else t.float().double()).clone().requires_grad_(True)


def transform(im, mat, out_size, ref=None, exact=False):
    """ref None: mat [B,3,3] is M; else M = ref . mat (mat = pMtrx).  -> (Sampled with out [B,oh,ow,C], leaves (im64, mat64))."""
    im64 = _leaf(im, exact)
    B, Hi, Wi, C = im64.shape
    oh, ow = out_size
    mat64 = _leaf(mat, exact)
    m = mat64.reshape(B, 3, 3)
    ref64 = None
    if ref is not None:
        ref64 = torch.as_tensor(ref).reshape(3, 3)
        ref64 = ref64.double() if exact else ref64.float().double()
        M = torch.matmul(ref64.unsqueeze(0), m)
        if not exact:
            M = _st(M, vo.warp_compose(ref64.float(), m.detach().float()))
    else:
        M = m
    M = M.reshape(B, 9)
    X32, Y32 = grid(oh, ow)
    X, Y = X32.double(), Y32.double()
    M32 = M.detach().float()

    def row(k):
        v = (M[:, k:k + 1] * X + M[:, k + 1:k + 2] * Y) + M[:, k + 2:k + 3]
        if exact:
            return v
        return _st(v, (M32[:, k:k + 1] * X32 + M32[:, k + 1:k + 2] * Y32) + M32[:, k + 2:k + 3])

    xh, yh, zh = row(0), row(3), row(6)
    zs = zh + 1e-8
    if not exact:
        zs = _st(zs, zh.detach().float() + np.float32(1e-8))
    xw, yw = xh / zs, yh / zs
    if not exact:
        xw, yw = _st(xw, xh.detach().float() / zs.detach().float()), _st(yw, yh.detach().float() / zs.detach().float())
    xf, xc, yf, yc = torch.floor(xw.detach()), torch.ceil(xw.detach()), torch.floor(yw.detach()), torch.ceil(yw.detach())
    xr, yr = (xw - xf).unsqueeze(-1), (yw - yf).unsqueeze(-1)
    xfi, xci, yfi, yci = (torch.nan_to_num(t, nan=-1e9).clamp(-1e9, 1e9).long() for t in (xf, xc, yf, yc))
    vec = torch.cat([im64.reshape(-1, C), torch.zeros(1, C, dtype=torch.float64)], 0)
    bidx = torch.arange(B).view(B, 1)
    outside = B * Hi * Wi

    def tap(xi, yi):
        inside = (xi >= 0) & (xi < Wi) & (yi >= 0) & (yi < Hi)
        return torch.where(inside, (bidx * Hi + yi) * Wi + xi, torch.full_like(xi, outside)), inside

    taps = [tap(xfi, yfi), tap(xci, yfi), tap(xfi, yci), tap(xci, yci)]                    # UL, UR, BL, BR
    wts = [(1 - xr) * (1 - yr), xr * (1 - yr), (1 - xr) * yr, xr * yr]
    vals = [vec[i] for i, _ in taps]
    out = vals[0] * (1 - xr) * (1 - yr) + vals[1] * xr * (1 - yr) + vals[2] * (1 - xr) * yr + vals[3] * xr * yr
    s = Sampled()
    s.out = out.reshape(B, oh, ow, C)
    s.idx, s.inside = [i for i, _ in taps], [v for _, v in taps]
    s.wts, s.taps = [w.detach() for w in wts], [v.detach() for v in vals]
    s.xr, s.yr = xr.detach(), yr.detach()
    s.X, s.Y, s.xh, s.yh, s.zs = X, Y, xh.detach(), yh.detach(), zs.detach()
    s.floors = (xf, yf, xc, yc)
    s.ref, s.shape = ref64, (B, Hi, Wi, C)
    return s, (im64, mat64)


def backward(s, leaves, dout):
    """Gradients of sum(out * dout) by autograd, and the count / absolute companions described in the module docstring.
    Keys: d_img, n_img, S_img, d_M, S_M ([B,3,3]; with ref they are d pMtrx and its companion)."""
    B, Hi, Wi, C = s.shape
    dout = torch.as_tensor(dout).double().reshape(s.out.shape)
    grads = torch.autograd.grad(s.out, leaves, dout, allow_unused=True)
    r = {"d_img": grads[0] if grads[0] is not None else torch.zeros(s.shape, dtype=torch.float64)}
    ad = dout.abs().reshape(B, -1, C)
    n_img = torch.zeros(B * Hi * Wi + 1, dtype=torch.float64)
    S_img = torch.zeros(B * Hi * Wi + 1, C, dtype=torch.float64)
    for w, i in zip(s.wts, s.idx):
        n_img.index_add_(0, i.reshape(-1), torch.ones(i.numel(), dtype=torch.float64))
        S_img.index_add_(0, i.reshape(-1), (w * ad).reshape(-1, C))
    r["n_img"] = n_img[:-1].reshape(B, Hi, Wi, 1).expand(B, Hi, Wi, C)
    r["S_img"] = S_img[:-1].reshape(B, Hi, Wi, C)
    aUL, aUR, aBL, aBR = (t.abs() for t in s.taps)
    live = (s.inside[0] | s.inside[1] | s.inside[2] | s.inside[3])                         # a pixel with no tap inside contributes nothing
    zero = torch.zeros(live.shape, dtype=torch.float64)
    Sx = torch.where(live, (ad * ((aUL + aUR) * (1 - s.yr) + (aBL + aBR) * s.yr)).sum(-1), zero)
    Sy = torch.where(live, (ad * ((aUL + aBL) * (1 - s.xr) + (aUR + aBR) * s.xr)).sum(-1), zero)
    az = s.zs.abs()
    Sz = torch.where(live, (Sx * s.xh.abs() + Sy * s.yh.abs()) / (az * az), zero)
    Sx, Sy = torch.where(live, Sx / az, zero), torch.where(live, Sy / az, zero)
    aX, aY = s.X.abs(), s.Y.abs()
    S_M = torch.stack([(Sx * aX).sum(1), (Sx * aY).sum(1), Sx.sum(1), (Sy * aX).sum(1), (Sy * aY).sum(1), Sy.sum(1),
                       (Sz * aX).sum(1), (Sz * aY).sum(1), Sz.sum(1)], 1).reshape(B, 3, 3)
    if s.ref is not None:
        S_M = torch.matmul(s.ref.abs().t().unsqueeze(0), S_M)
    r["d_M"] = grads[1].reshape(B, 3, 3) if grads[1] is not None else torch.zeros(B, 3, 3, dtype=torch.float64)
    r["S_M"] = S_M
    return r


def _generator(p, warp_type, absolute=False):
    B = p.shape[0]
    if warp_type == "homography":
        p1, p2, p3, p4, p5, p6, p7, p8 = p.unbind(1)
        mid = p3 + p7 if absolute else -p3 - p7
        return torch.stack([torch.stack([p3, p2, p1], 1), torch.stack([p6, mid, p5], 1), torch.stack([p4, p8, p7], 1)], 1)
    O = torch.zeros(B, dtype=p.dtype)
    p1, p2, p3, p4, p5, p6 = p.unbind(1)
    return torch.stack([torch.stack([p1, p2, p3], 1), torch.stack([p4, p5, p6], 1), torch.stack([O, O, O], 1)], 1)


def _expm(A, warp_approx):
    """vo.warp_vec2mtrx's recurrence on an fp64 graph tensor"""
    B = A.shape[0]
    pM = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)
    numer = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)
    denom = 1.0
    for i in range(1, warp_approx):
        numer = torch.matmul(numer, A)
        denom *= i
        pM = pM + numer / denom
    return pM


def vec2mtrx(p, warp_type, warp_approx, exact=False):
    """-> (pMtrx [B,3,3] in the fp64 graph, the leaf p64): fp64 autograd of vo.warp_vec2mtrx's recurrence from the fp32 p"""
    p64 = _leaf(p, exact)
    return _expm(_generator(p64, warp_type), warp_approx), p64


def vec2mtrx_backward(p, d_out, warp_type, warp_approx, exact=False):
    """Keys: d_p, S_p ([B,8|6])."""
    P, p64 = vec2mtrx(p, warp_type, warp_approx, exact)
    d_out = torch.as_tensor(d_out).double().reshape(P.shape)
    pa = p64.detach().abs().clone().requires_grad_(True)
    Pa = _expm(_generator(pa, warp_type, absolute=True), warp_approx)
    if warp_approx < 2:                                                      # pMtrx = I whatever p is
        z = torch.zeros_like(p64)
        return {"d_p": z, "S_p": z.clone()}
    return {"d_p": torch.autograd.grad(P, p64, d_out)[0], "S_p": torch.autograd.grad(Pa, pa, d_out.abs())[0]}
