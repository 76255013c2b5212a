"""Reference for the gradients of the BICUBIC sampler ("ST" = the reference's spatial_transformer.py): bicubic_interp (ST:966-1072)
under explicit coordinates, the affine / projective transformers, the symmetric-pad transformers and the thin-plate spline,
differentiated by torch.autograd in fp64 -- what TensorFlow's autodiff gives for the same op sequence: floor and the casts have zero
derivative, clip_by_value to [-1, 1] passes the gradient where -1 <= x <= 1 inclusive (torch.clamp agrees) and not for NaN, which the
kernels read as -1.

In the manner of tests/st_grad_ref.py.  The coordinate VALUES, and so every floor, clip and clamp decision, are the kernels' fp32
sequence -- clip, (v + 1) / 2 * (n - 1) with each step rounded -- brought into the fp64 graph by the straight-through substitution
`_st`; t = v - floor(v), the weights, their derivatives and the blends are fp64.  The sources of coordinates are not restated: the
graphs theta -> (x_s, y_s) are those of st_grad_ref.transform and st_sym_grad_ref.transform, run with this module's sampler in
place of their bilinear `_sample`, and the spline's chain is st_tps_grad_ref's.  `exact=True` drops every substitution: a plain fp64
function, which is what central differences can be taken of.

`backward` returns, per gradient element, the count `n` of contributions (d img: the taps that land on the pixel, the replicated
edge taps and, for the symmetric pad, the folded ones included) and the absolute companion `S`.  The weights can be negative and
cancel (w_3 = -0.75 t^2 (1 - t) is the difference of two terms of size 0.75 near t = 1), and an fp32 evaluation errs in proportion
to the terms, not to their sum; so S is built from each weight's absolute companion |w|_i = sum_k |c_ik| t^k >= |w_i| (likewise
|w'|_i = sum_k k |c_ik| t^(k-1)), with |I| and |dout|:
    S_img = adjoint of the gather applied to |w|y_i |w|x_j |dout|,
    S_x   = pass (W - 1) / 2 sum_c |dout_c| sum_i |w|y_i sum_j |w'|x_j |I_ij|    (S_y likewise),
    S_theta from S_x, S_y through the absolute values of each source's chain factors, as in the bilinear references."""
from contextlib import contextmanager

import numpy as np
import torch

from tests import st_grad_ref as gref
from tests import st_sym_grad_ref as sref
from tests import st_tps_grad_ref as tref
from tests.st_grad_ref import Sampled, _st

# get_weights' table (ST:1038-1050), tap order [x0, x0-1, x0+1, x0+2]: w_i = c_i0 + c_i1 t + c_i2 t^2 + c_i3 t^3
COEFFS = torch.tensor([[1.0, 0.0, -2.25, 1.25], [0.0, -0.75, 1.5, -0.75], [0.0, 0.75, 1.5, -1.25], [0.0, 0.0, -0.75, 0.75]], dtype=torch.float64)


def weights(t):
    """t [N] fp64 -> (w, dw, |w|, |w'|), each [4, N]; w stays in t's graph."""
    c, a = COEFFS, COEFFS.abs()
    t = t.unsqueeze(0)
    td = t.detach()
    w = c[:, 0:1] + c[:, 1:2] * t + c[:, 2:3] * t * t + c[:, 3:4] * t * t * t
    dw = c[:, 1:2] + 2.0 * c[:, 2:3] * td + 3.0 * c[:, 3:4] * td * td
    aw = a[:, 0:1] + a[:, 1:2] * td + a[:, 2:3] * td * td + a[:, 3:4] * td * td * td
    adw = a[:, 1:2] + 2.0 * a[:, 2:3] * td + 3.0 * a[:, 3:4] * td * td
    return w, dw, aw, adw


def _axis(v, n, exact):
    """Normalised coordinate v (fp64, in the graph) -> (t in the graph, the four tap indices, whether the clip passes a gradient)."""
    nan = torch.isnan(v.detach())
    v = torch.where(nan, torch.full_like(v, -1.0), v)                     # the kernels' rule: NaN reads as -1 (and gets no gradient)
    passed = (v.detach() >= -1.0) & (v.detach() <= 1.0) & ~nan
    c = torch.clamp(v, -1.0, 1.0)
    p = (c + 1.0) / 2.0 * float(n - 1)
    if not exact:
        p = _st(p, (c.detach().float() + 1.0) / 2.0 * (np.float32(n) - np.float32(1.0)))
    p0 = torch.floor(p.detach())
    i0 = p0.long()
    idx = [i0, torch.clamp(i0 - 1, min=0), torch.clamp(i0 + 1, max=n - 1), torch.clamp(i0 + 2, max=n - 1)]
    return p - p0, idx, passed


def _sample(im64, xn, yn, out_size, exact):
    """bicubic_interp (ST:966-1072) on fp64 graph tensors.  xn, yn flat [B*oh*ow].  Edges replicate: no padding anywhere."""
    B, H, W, C = im64.shape
    npix = out_size[0] * out_size[1]
    tx, ix, px = _axis(xn, W, exact)
    ty, iy, py = _axis(yn, H, exact)
    wx, dwx, awx, adwx = weights(tx)
    wy, dwy, awy, adwy = weights(ty)
    flat = im64.reshape(-1, C)
    base = torch.arange(B).repeat_interleave(npix) * (H * W)
    s = Sampled()
    s.idx, s.aw, s.sxw, s.syw, s.ataps = [], [], [], [], []
    out = 0.0
    for i in range(4):
        rowsum = 0.0
        for j in range(4):
            k = base + iy[i] * W + ix[j]
            tap = flat[k]
            rowsum = rowsum + wx[j].unsqueeze(1) * tap
            s.idx.append(k)
            s.aw.append(awy[i] * awx[j])
            s.sxw.append(awy[i] * adwx[j])
            s.syw.append(adwy[i] * awx[j])
            s.ataps.append(tap.detach().abs())
        out = out + wy[i].unsqueeze(1) * rowsum
    s.out, s.pass_x, s.pass_y, s.shape = out, px, py, (B, H, W, C)
    s.wx, s.wy, s.dwx, s.dwy = wx.detach(), wy.detach(), dwx, dwy
    return s


def bicubic_interp(im, x, y, out_size, exact=False):
    """-> (Sampled with out [B*oh*ow, C], leaves (im64, x64, y64)).  x, y are rounded to fp32 first unless `exact`."""
    im64 = torch.as_tensor(im).double().clone().requires_grad_(True)
    cast = (lambda t: torch.as_tensor(t).double()) if exact else (lambda t: torch.as_tensor(t).float().double())
    x64, y64 = cast(x).reshape(-1).clone().requires_grad_(True), cast(y).reshape(-1).clone().requires_grad_(True)
    s = _sample(im64, x64, y64, out_size, exact)
    s.kind = "coords"
    return s, (im64, x64, y64)


@contextmanager
def _bicubic_sampler():
    """The bilinear references' coordinate graphs with this module's sampler at their end."""
    saved = gref._sample, sref._sample
    gref._sample = sref._sample = _sample
    try:
        yield
    finally:
        gref._sample, sref._sample = saved


def transform(im, theta, out_size, exact=False):
    """Affine (theta [B,6]) / ProjectiveTransformer (theta [B,8]) .transform with the bicubic sampler."""
    with _bicubic_sampler():
        return gref.transform(im, theta, out_size, exact)


def symmetry_transform(kind, im, theta, out_size, M32=None, xs32=None, ys32=None, exact=False):
    """The symmetric-pad transformers with the bicubic sampler (arguments of st_sym_grad_ref.transform)."""
    with _bicubic_sampler():
        s, leaves = sref.transform(kind, im, theta, out_size, M32, xs32, ys32, exact)
    s.sym = True
    return s, leaves


def elastic(im, x_s, y_s, g, out_size):
    """The sampler on the spline's given fp32 coordinates; the grid's R and A attached (st_tps_grad_ref.elastic)."""
    s, leaves = bicubic_interp(im, x_s, y_s, out_size)
    s.tps_R = tref.tps_R(g, out_size)
    return s, leaves


def elastic_backward(s, leaves, dout, g, linv_t):
    """st_tps_grad_ref.backward's chain on this module's per-pixel d x, d y."""
    saved = gref.backward
    gref.backward = backward
    try:
        return tref.backward(s, leaves, dout, g, linv_t)
    finally:
        gref.backward = saved


def _per_pixel(s, ad, Wn, Hn):
    """S_x, S_y per sampled point from |dout| `ad` [N, C]; Wn, Hn the extents the coordinates are scaled by."""
    S_x = sum((ad * t).sum(1) * w for t, w in zip(s.ataps, s.sxw)) * (0.5 * (Wn - 1)) * s.pass_x
    S_y = sum((ad * t).sum(1) * w for t, w in zip(s.ataps, s.syw)) * (0.5 * (Hn - 1)) * s.pass_y
    return S_x, S_y


def _theta_cols(s, S_x, S_y, proj):
    ax, ay = s.xt.abs(), s.yt.abs()
    cols = []
    if proj:
        S_z = (S_x * s.xh.abs() + S_y * s.yh.abs()) / (s.z * s.z)
        S_x, S_y = S_x / s.z.abs(), S_y / s.z.abs()
        cols = [S_z * ax, S_z * ay]
    return torch.stack([c.sum(1) for c in [S_x * ax, S_x * ay, S_x, S_y * ax, S_y * ay, S_y] + cols], 1)


def backward(s, leaves, dout):
    """Gradients of sum(out * dout) by autograd, and the counts / absolute companions of the module docstring.
    Keys: d_img, n_img, S_img; coords: d_x, d_y, S_x, S_y; theta and the symmetric pad: d_theta, S_theta."""
    B, H, W, C = s.shape                                                  # the SAMPLED extent: the padded image for the symmetric pad
    dout = torch.as_tensor(dout).double().reshape(s.out.shape)
    grads = torch.autograd.grad(s.out, leaves, dout, allow_unused=True)
    r = {"d_img": grads[0]}
    sym = getattr(s, "sym", False)
    if sym:
        oh, ow = s.out_size
        ad = sref.to_grid(dout.abs(), oh, ow).reshape(-1, C)
        kept = sref.to_grid(torch.ones(dout.shape[:3], dtype=torch.float64), oh, ow).reshape(-1)
    else:
        ad = dout.abs().reshape(-1, C)
        kept = torch.ones(ad.shape[0], dtype=torch.float64)
    n_img = torch.zeros((B * H * W,), dtype=torch.float64)
    S_img = torch.zeros((B * H * W, C), dtype=torch.float64)
    for w, i in zip(s.aw, s.idx):
        n_img.index_add_(0, i, kept)
        S_img.index_add_(0, i, w.unsqueeze(1) * ad)
    n_img, S_img = n_img.reshape(B, H, W, 1).expand(B, H, W, C), S_img.reshape(B, H, W, C)
    if sym:
        Hi, Wi = s.img_shape[1], s.img_shape[2]
        n_img, S_img = sref.fold(n_img.contiguous(), Hi, Wi), sref.fold(S_img.contiguous(), Hi, Wi)
    r["n_img"], r["S_img"] = n_img, S_img
    S_x, S_y = _per_pixel(s, ad, W, H)
    if s.kind == "coords":
        r["d_x"], r["d_y"], r["S_x"], r["S_y"] = grads[1], grads[2], S_x, S_y
        return r
    r["d_theta"] = grads[1] if grads[1] is not None else torch.zeros_like(leaves[1])
    S_x, S_y = S_x.reshape(B, -1), S_y.reshape(B, -1)
    if s.kind == "theta":
        r["S_theta"] = _theta_cols(s, S_x, S_y, s.tdim == 8)
        return r
    S_M = _theta_cols(s, S_x, S_y, s.kind == 'projective')                 # st_sym_grad_ref.backward's pre-map companions
    if s.kind == 'affine':
        r["S_theta"] = S_M * 0.0
    elif s.kind == 'projective':
        r["S_theta"] = S_M * sref._d(sref._P[:8])
    else:
        a, sc = s.aux
        SE = S_M.reshape(-1).reshape(6, B)
        sum_c, sum_s = SE[0] + SE[4], SE[1] + SE[3]
        S_a = sc.abs() * a.sin().abs() * sum_c + sc.abs() * a.cos().abs() * sum_s
        S_s = a.cos().abs() * sum_c + a.sin().abs() * sum_s
        k = sref._d(sref._SIM_SCALE)
        r["S_theta"] = torch.stack([S_a * k[0], S_s * k[1], SE[2] * k[2], SE[5] * k[3]], 1)
    return r
