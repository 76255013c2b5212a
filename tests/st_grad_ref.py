"""Reference for the gradients of the bilinear spatial transformers ("ST" = the reference's spatial_transformer.py):
AffineTransformer / ProjectiveTransformer.transform (ST:400-452, 539-608) and bilinear_interp (ST:902-964), differentiated by
torch.autograd in fp64 -- what TensorFlow's autodiff gives for the same op sequence: floor and the casts have zero derivative,
clip_by_value passes the gradient where -1 <= x <= W inclusive (torch.clamp agrees) and not for NaN.

The coordinate VALUES, and so every floor and clip decision, are those of the HIP kernels' fp32 sequence (the chain of
`vo.st_transform(..., matmul="unfused")`: (t0*x + t1*y) + t2 with each product and sum rounded, the fp32 division by safe_z, the
fp32 pixel scaling, clip and +1), brought into the fp64 graph by the straight-through substitution v = v64 + (v32 - v64).detach():
the value of the fp32 sequence, the derivative of the fp64 expression, at every rounded step of the chain.  Everything downstream --
weights, blends, gradients -- is fp64.  `exact=True` drops the substitution: a plain fp64 function, which is what central
differences can be taken of.

Besides the gradients, `backward` returns what the tolerances of tests/test_gpu_st_backward.py are derived from, per gradient
element: the count `n` of contributions (d img) and the absolute companion `S`: the same backward with |dout|, with
(|I00| + |I01|) (y1f - y) + (|I10| + |I11|) (y - y0f) in place of the slope (likewise for y), and with the absolute values of the
chain factors; for d img it is the adjoint applied to |dout|, the weights being non-negative."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import vstab_oracle as vo


def _st(v64, v32):
    """Straight-through: the value of v32 (an fp32 tensor), the derivative of v64.  A value that is not finite is a constant
    (inf - inf would make it NaN): the clip blocks its gradient anyway."""
    fin = torch.isfinite(v64.detach()) & torch.isfinite(v32)
    v64 = torch.where(fin, v64, torch.zeros_like(v64))
    return torch.where(fin, v64 + (v32.double() - v64).detach(), v32.double())


def _axis(v, n, exact):
    """Normalised coordinate v (fp64, in the graph; its values are fp32 numbers unless `exact`) -> the coordinate in the image
    zero-padded by one pixel (ST:916-922), and whether the clip passes a gradient."""
    p = (v + 1.0) / 2.0 * float(n - 1)
    if not exact:
        p = _st(p, (v.detach().float() + 1.0) / 2.0 * (np.float32(n) - np.float32(1.0)))
    nan = torch.isnan(p.detach())
    p = torch.where(nan, torch.full_like(p, -1.0), p)                      # the kernels' rule: NaN reads as -1 (and gets no gradient)
    passed = (p.detach() >= -1.0) & (p.detach() <= float(n)) & ~nan
    q = torch.clamp(p, -1.0, float(n)) + 1.0
    if not exact:
        q = _st(q, torch.clamp(p.detach().float(), -1.0, float(n)) + 1.0)
    return q, passed


class Sampled:
    """One forward through the graph: `out` (fp64, [B,oh,ow,C] or [B*oh*ow,C]) and what `backward` needs."""


def _sample(im64, xn, yn, out_size, exact):
    """bilinear_interp (ST:902-964) on fp64 graph tensors.  xn, yn flat [B*oh*ow]."""
    B, H, W, C = im64.shape
    npix = out_size[0] * out_size[1]
    qx, px = _axis(xn, W, exact)
    qy, py = _axis(yn, H, exact)
    x0f, y0f = torch.floor(qx.detach()), torch.floor(qy.detach())
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = torch.clamp(x0 + 1, max=W + 1), torch.clamp(y0 + 1, max=H + 1)   # the index is clipped, the weight's x0 + 1 is not
    hx, lx, hy, ly = (x0f + 1.0) - qx, qx - x0f, (y0f + 1.0) - qy, qy - y0f
    imp = F.pad(im64, (0, 0, 1, 1, 1, 1)).reshape(-1, C)
    base = torch.arange(B).repeat_interleave(npix) * ((W + 2) * (H + 2))
    idx = [base + y0 * (W + 2) + x0, base + y0 * (W + 2) + x1, base + y1 * (W + 2) + x0, base + y1 * (W + 2) + x1]
    wts = [hx * hy, lx * hy, hx * ly, lx * ly]
    out = sum(w.unsqueeze(1) * imp[i] for w, i in zip(wts, idx))
    s = Sampled()
    s.out, s.idx, s.wts, s.pass_x, s.pass_y = out, idx, [w.detach() for w in wts], px, py
    s.taps = [imp[i].detach() for i in idx]
    s.hx, s.lx, s.hy, s.ly = hx.detach(), lx.detach(), hy.detach(), ly.detach()
    s.shape = (B, H, W, C)
    return s


def bilinear_interp(im, x, y, out_size, exact=False):
    """-> (Sampled, leaves (im64, x64, y64)).  x, y are rounded to fp32 first unless `exact` (vo.st_bilinear_interp does the same)."""
    im64 = torch.as_tensor(im).double().clone().requires_grad_(True)
    cast = (lambda t: torch.as_tensor(t).double()) if exact else (lambda t: torch.as_tensor(t).float().double())
    x64, y64 = cast(x).reshape(-1).clone().requires_grad_(True), cast(y).reshape(-1).clone().requires_grad_(True)
    s = _sample(im64, x64, y64, out_size, exact)
    s.kind = "coords"
    return s, (im64, x64, y64)


def transform(im, theta, out_size, exact=False):
    """Affine (theta [B,6]) / ProjectiveTransformer (theta [B,8]) .transform -> (Sampled with out [B,oh,ow,C], leaves (im64, theta64))."""
    im64 = torch.as_tensor(im).double().clone().requires_grad_(True)
    B, H, W, C = im64.shape
    th32 = torch.as_tensor(theta).float().reshape(B, -1)
    th = (torch.as_tensor(theta).double().reshape(B, -1) if exact else th32.double()).clone().requires_grad_(True)
    tdim = th.shape[1]
    grid = torch.from_numpy(vo.st_meshgrid(out_size)).reshape(3, -1)          # fp32 linspace values
    xt, yt = grid[0], grid[1]

    def row(k, last=None):                                                    # (t_k x + t_k+1 y) + t_k+2, fp64 graph + fp32 values
        c64 = th[:, k + 2:k + 3] if last is None else last
        v = (th[:, k:k + 1] * xt.double() + th[:, k + 1:k + 2] * yt.double()) + c64
        if exact:
            return v
        c32 = th32[:, k + 2:k + 3] if last is None else np.float32(last)
        return _st(v, (th32[:, k:k + 1] * xt + th32[:, k + 1:k + 2] * yt) + c32)

    xh, yh = row(0), row(3)
    z = None
    if tdim == 8:
        z = row(6, 1.0)
        if exact:
            z = torch.where(z.detach() == 0, z + 1e-8, z)
        else:
            z32 = z.detach().float()
            z = _st(z, torch.where(z32 == 0, z32 + np.float32(1e-8), z32))  # safe_z (ST:598): the gradient passes on both branches
        xs, ys = xh / z, yh / z
        if not exact:
            xs, ys = _st(xs, xh.detach().float() / z.detach().float()), _st(ys, yh.detach().float() / z.detach().float())
    else:
        xs, ys = xh, yh
    s = _sample(im64, xs.reshape(-1), ys.reshape(-1), out_size, exact)
    s.out = s.out.reshape(B, out_size[0], out_size[1], C)
    s.kind, s.tdim = "theta", tdim
    s.xt, s.yt = xt.double(), yt.double()
    s.xh, s.yh = xh.detach(), yh.detach()
    s.z = z.detach() if z is not None else None
    return s, (im64, th)


def backward(s, leaves, dout):
    """Gradients of sum(out * dout) by autograd, and the count / absolute companions described in the module docstring.
    Keys: d_img, n_img, S_img; coords: d_x, d_y, S_x, S_y; theta: d_theta, S_theta."""
    B, H, W, C = s.shape
    dout = torch.as_tensor(dout).double().reshape(s.out.shape)
    grads = torch.autograd.grad(s.out, leaves, dout, allow_unused=True)
    r = {"d_img": grads[0]}
    ad = dout.abs().reshape(-1, C)
    n_img = torch.zeros((B * (H + 2) * (W + 2),), dtype=torch.float64)
    S_img = torch.zeros((B * (H + 2) * (W + 2), C), dtype=torch.float64)
    for w, i in zip(s.wts, s.idx):
        n_img.index_add_(0, i, torch.ones_like(w))
        S_img.index_add_(0, i, w.unsqueeze(1) * ad)
    r["n_img"] = n_img.reshape(B, H + 2, W + 2)[:, 1:-1, 1:-1].unsqueeze(-1).expand(B, H, W, C)
    r["S_img"] = S_img.reshape(B, H + 2, W + 2, C)[:, 1:-1, 1:-1]
    a00, a01, a10, a11 = (t.abs() for t in s.taps)
    S_x = (ad * ((a00 + a01) * s.hy.unsqueeze(1) + (a10 + a11) * s.ly.unsqueeze(1))).sum(1) * (0.5 * (W - 1)) * s.pass_x
    S_y = (ad * ((a00 + a10) * s.hx.unsqueeze(1) + (a01 + a11) * s.lx.unsqueeze(1))).sum(1) * (0.5 * (H - 1)) * s.pass_y
    if s.kind == "coords":
        r["d_x"], r["d_y"], r["S_x"], r["S_y"] = grads[1], grads[2], S_x, S_y
        return r
    S_x, S_y = S_x.reshape(B, -1), S_y.reshape(B, -1)
    ax, ay = s.xt.abs(), s.yt.abs()
    if s.tdim == 8:
        S_z = (S_x * s.xh.abs() + S_y * s.yh.abs()) / (s.z * s.z)
        S_x, S_y = S_x / s.z.abs(), S_y / s.z.abs()
    cols = [S_x * ax, S_x * ay, S_x, S_y * ax, S_y * ay, S_y]
    if s.tdim == 8:
        cols += [S_z * ax, S_z * ay]
    r["d_theta"] = grads[1]
    r["S_theta"] = torch.stack([c.sum(1) for c in cols], 1)
    return r
