"""Reference for the gradients of ElasticTransformer.transform with the bilinear sampler ("ST" = the reference's
spatial_transformer.py, ST:40-224): the thin-plate spline's chain on top of tests/st_grad_ref.py, which is used as it is.

x_s = cf_x . R, y_s = cf_y . R per output pixel, with R = [x_t, y_t, 1, U_1..U_K] (U_k = r^2 ln r^2 against control point k: it
depends on the output grid alone, nothing flows through it) and cf = (source points + theta) . linv_t.  So

    d cf[r]    = sum over the pixels of (d x_s | d y_s) R          [2, K+3]
    d theta[r] = d cf[r] . linv_t^T                                [2, K], flattened to [2K]: x offsets, then y offsets

Two modes.

`elastic(im, x_s, y_s, ...)`: the coordinates are GIVEN, as fp32 values -- the tests pass what ElasticTransformer.transform_coords
returns, so every floor and clip decision is the kernels' (their logf cannot be reproduced bit for bit on a CPU).
st_grad_ref.bilinear_interp / backward give d img, n_img, S_img and, per pixel, d x, d y, S_x, S_y in fp64; the chain above is then
applied in fp64, R from the fp64 U of the fp32 linspace values (st_extended_ref.tps_U) and linv_t the device's fp32 table read as
double.  The absolute companion of d theta is

    S_theta[r, k] = sum_j |linv_t[k, j]| sum_p S_r[p] A_j[p]

with A_j = |R_j| for the three affine columns and A = r^2 (|ln r^2| + 1) for a U column, not |U|: an fp32 r^2 carries its relative
error into ln r^2 as an absolute one, so near r^2 = 1, where U vanishes, |U| alone would understate the error.

`elastic_exact(im, theta, ...)`: the coordinates are computed in fp64 inside the torch graph from a theta leaf, with no
straight-through substitution anywhere: a plain fp64 function, which is what central differences can be taken of."""
import numpy as np
import torch

from tests import st_extended_ref as xref
from tests import st_grad_ref as gref


def tps_R(g, out_size):
    """R [K+3, oh*ow] in fp64 from the fp32 linspace values, and A (the companion's columns, same shape)."""
    xt, yt = xref.grid(*out_size)
    xt, yt = xt.astype(np.float64), yt.astype(np.float64)
    src = xref.tps_source_points(g).astype(np.float64)
    r2 = (xt[None] - src[0][:, None]) ** 2 + (yt[None] - src[1][:, None]) ** 2             # [K, N]
    U = xref.tps_U(r2)
    with np.errstate(divide='ignore', invalid='ignore'):
        ln = np.where(r2 == 0, 0.0, np.abs(np.log(np.where(r2 == 0, 1.0, r2))))
    head = np.stack([xt, yt, np.ones_like(xt)])
    R = np.concatenate([head, U], 0)
    A = np.concatenate([np.abs(head), r2 * (ln + 1.0)], 0)
    return torch.from_numpy(R), torch.from_numpy(A)


def coords64(theta, g, out_size, linv_t, exact=False):
    """(x_s, y_s) [B, oh*ow] in fp64 on torch tensors: (source + theta) . linv_t . R.  Unless `exact`, source + theta is the
    kernels' fp32 sum (ST:108 adds in fp32); `exact` keeps theta (an fp64 tensor, possibly a graph leaf) in fp64 throughout."""
    K = g * g
    src = torch.from_numpy(xref.tps_source_points(g))                                       # [2, K] fp32
    if exact:
        P = src.double()[None] + theta.reshape(-1, 2, K)
    else:
        P = (src[None] + torch.as_tensor(theta).float().reshape(-1, 2, K)).double()
    Lt = torch.as_tensor(linv_t).double()
    R, _ = tps_R(g, out_size)
    T = (P @ Lt) @ R                                                                        # [B, 2, N]
    return T[:, 0], T[:, 1]


def elastic(im, x_s, y_s, g, out_size):
    """The sampler on given fp32 coordinates (flat [B*oh*ow]) -> st_grad_ref's (Sampled, leaves), the grid's R and A attached."""
    s, leaves = gref.bilinear_interp(im, x_s, y_s, out_size)
    s.tps_R = tps_R(g, out_size)
    return s, leaves


def backward(s, leaves, dout, g, linv_t):
    """st_grad_ref.backward's d_img, n_img, S_img, d_x, d_y, S_x, S_y plus the chain: d_cf [B,2,K+3], d_theta and S_theta [B,2K]."""
    B = s.shape[0]
    K = g * g
    r = gref.backward(s, leaves, dout)
    npix = r["d_x"].numel() // B
    dxy = torch.stack([r["d_x"].reshape(B, npix), r["d_y"].reshape(B, npix)], 1)            # [B, 2, N]
    Sxy = torch.stack([r["S_x"].reshape(B, npix), r["S_y"].reshape(B, npix)], 1)
    R, A = s.tps_R
    Lt = torch.as_tensor(linv_t).double()                                                   # [K, K+3]
    r["d_cf"] = dxy @ R.T                                                                   # [B, 2, K+3]
    r["d_theta"] = (r["d_cf"] @ Lt.T).reshape(B, 2 * K)
    r["S_theta"] = ((Sxy @ A.T) @ Lt.abs().T).reshape(B, 2 * K)
    return r


def elastic_exact(im, theta, g, out_size, linv_t):
    """Plain fp64: -> (out [B,oh,ow,C] in the graph, leaves (im64, theta64 [B,2K]))."""
    im64 = torch.as_tensor(im).double().clone().requires_grad_(True)
    B, H, W, C = im64.shape
    th = torch.as_tensor(theta).double().reshape(B, -1).clone().requires_grad_(True)
    xs, ys = coords64(th, g, out_size, linv_t, exact=True)
    s = gref._sample(im64, xs.reshape(-1), ys.reshape(-1), out_size, True)
    return s.out.reshape(B, out_size[0], out_size[1], C), (im64, th)
