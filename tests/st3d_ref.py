"""Reference for the 3-D volume transformer ("ST" = the reference's spatial_transformer.py): _meshgrid3d (ST:725-753),
AffineVolumeTransformer._transform (ST:291-308) and bilinear_interp3d (ST:797-899), restated in torch on the CPU in the
reference's op order:
  grid     -1 + i * (2 / (n - 1)) (a single point is -1); rows x_t, y_t, z_t, ones; x fastest, z slowest
  theta    x_s = ((t0 x_t + t1 y_t) + t2 z_t) + t3, rows 1 and 2 likewise for y_s, z_s
  axis     v = (v + 1) / 2 * (n - 1), clip to [-e, n - 1 + e] (NaN reads as -e), + e; v0 = floor(v); index v1 = min(v0 + 1, n - 1 + 2e);
           weights hi = (v0 + 1) - v, lo = v - v0
  blend    weights (wz * wy) * wx, the eight products summed left to right in the order 000, 001, ..., 111 (last digit x, 1 = v1 tap)
`dtype` picks the arithmetic: torch.float32 gives the HIP kernels' sequence bit for bit, torch.float64 a clean function.

The gradient reference follows tests/st_grad_ref.py: an fp64 autograd graph (floor and the casts have zero derivative, the clip
passes the gradient where -e <= v <= n - 1 + e inclusive and not for NaN) into which the fp32 coordinate VALUES are substituted
straight-through, v = v64 + (v32 - v64).detach(), so every floor and clip decision is the kernels'; `exact=True` drops the
substitution.  `backward` returns, per gradient element, the contribution count `n` (d vol) and the absolute companion `S`: the same
backward with |dout|, with the sum of |tap| pairs times their pair weights in place of the slope, and with the absolute values of
the chain factors; for d vol the adjoint applied to |dout| (the weights are non-negative)."""
import os
import re

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brick():
    """(brick_z, brick_y, brick_x) of the shipped kernels, from include/vstab.h."""
    hdr = open(os.path.join(ROOT, "include", "vstab.h")).read()
    return tuple(int(re.search(rf"#define\s+VSTAB_ST3D_BRICK_{a}\s+(\d+)", hdr).group(1)) for a in "ZYX")


def lin11(n, dtype=torch.float32):
    if n == 1:
        return torch.full((1,), -1.0, dtype=dtype)
    step = torch.tensor(2.0, dtype=dtype) / torch.tensor(float(n - 1), dtype=dtype)
    return -1.0 + torch.arange(n, dtype=dtype) * step


def meshgrid3d(out_size, dtype=torch.float32):
    """Flat [4 * od * oh * ow]."""
    od, oh, ow = out_size
    z, y, x = torch.meshgrid(lin11(od, dtype), lin11(oh, dtype), lin11(ow, dtype), indexing='ij')
    x, y, z = x.reshape(1, -1), y.reshape(1, -1), z.reshape(1, -1)
    return torch.cat([x, y, z, torch.ones_like(x)], 0).reshape(-1)


def _axis(v, n, e):
    """-> padded coordinate (in v's dtype), v0f, padded indices i0, i1"""
    v = (v + 1.0) / 2.0 * float(n - 1)
    v = torch.where(torch.isnan(v), torch.full_like(v, -float(e)), v)
    v = torch.clamp(v, -float(e), float(n - 1 + e)) + float(e)
    v0f = torch.floor(v)
    i1 = torch.minimum(v0f + 1.0, torch.full_like(v, float(n - 1 + 2 * e))).long()
    return v, v0f, v0f.long(), i1


def _blend(volp, B, nvox, dims, ax):
    """volp: padded volume flat [-1, C]; dims (Dp, Hp, Wp); ax = per axis (v, v0f, i0, i1) in the order x, y, z."""
    Dp, Hp, Wp = dims
    (x, x0f, x0, x1), (y, y0f, y0, y1), (z, z0f, z0, z1) = ax
    base = torch.arange(B).repeat_interleave(nvox) * (Dp * Hp * Wp)
    wx, wy, wz = (x0f + 1.0 - x, x - x0f), (y0f + 1.0 - y, y - y0f), (z0f + 1.0 - z, z - z0f)
    ix, iy, iz = (x0, x1), (y0, y1), (z0, z1)
    out, idx, wts = None, [], []
    for k in range(8):
        bz, by, bx = (k >> 2) & 1, (k >> 1) & 1, k & 1
        i = base + iz[bz] * (Hp * Wp) + iy[by] * Wp + ix[bx]
        w = (wz[bz] * wy[by]) * wx[bx]
        term = w.unsqueeze(1) * volp[i]
        out = term if out is None else out + term
        idx.append(i)
        wts.append(w)
    return out, idx, wts, (wx, wy, wz)


def bilinear_interp3d(vol, x, y, z, out_size, edge_size=1, dtype=torch.float32):
    """vol [B,D,H,W,C]; x, y, z flat [B*od*oh*ow] -> [B*od*oh*ow, C], every operation in `dtype`."""
    vol = torch.as_tensor(vol).to(dtype)
    B, D, H, W, C = vol.shape
    e = int(edge_size)
    nvox = out_size[0] * out_size[1] * out_size[2]
    x, y, z = (torch.as_tensor(t).to(dtype).reshape(-1) for t in (x, y, z))          # fp32: the reference's tf.cast
    volp = F.pad(vol, (0, 0, e, e, e, e, e, e)).reshape(-1, C)
    out, _, _, _ = _blend(volp, B, nvox, (D + 2 * e, H + 2 * e, W + 2 * e), (_axis(x, W, e), _axis(y, H, e), _axis(z, D, e)))
    return out


def theta_coords(theta, out_size, B, dtype=torch.float32):
    """-> x_s, y_s, z_s flat [B * nvox]"""
    th = torch.as_tensor(theta).to(dtype).reshape(B, 12)
    g = meshgrid3d(out_size).to(dtype).reshape(4, -1)                         # the grid's values are the fp32 linspace in every dtype
    xt, yt, zt = g[0], g[1], g[2]
    rows = [((th[:, 4 * r:4 * r + 1] * xt + th[:, 4 * r + 1:4 * r + 2] * yt) + th[:, 4 * r + 2:4 * r + 3] * zt) + th[:, 4 * r + 3:4 * r + 4]
            for r in range(3)]
    return tuple(r.reshape(-1) for r in rows)


def transform(vol, theta, out_size, dtype=torch.float32):
    """AffineVolumeTransformer.transform -> [B,od,oh,ow,C] (edge_size = 1)."""
    vol = torch.as_tensor(vol)
    B, C = vol.shape[0], vol.shape[4]
    xs, ys, zs = theta_coords(theta, out_size, B, dtype)
    return bilinear_interp3d(vol, xs, ys, zs, out_size, 1, dtype).reshape(B, *out_size, C)


# ------------------------------------------------------------------------------------------------------------ gradients
def _st(v64, v32):
    """Straight-through: the value of v32 (an fp32 tensor), the derivative of v64.  A value that is not finite is a constant."""
    fin = torch.isfinite(v64.detach()) & torch.isfinite(v32)
    v64 = torch.where(fin, v64, torch.zeros_like(v64))
    return torch.where(fin, v64 + (v32.double() - v64).detach(), v32.double())


def _axis_graph(v, n, e, exact):
    """Normalised coordinate v (fp64, in the graph; fp32 values unless `exact`) -> (padded coordinate in the graph, v0f, i0, i1, pass)."""
    p = (v + 1.0) / 2.0 * float(n - 1)
    if not exact:
        p = _st(p, (v.detach().float() + 1.0) / 2.0 * float(n - 1))
    nan = torch.isnan(p.detach())
    p = torch.where(nan, torch.full_like(p, -float(e)), p)
    passed = (p.detach() >= -float(e)) & (p.detach() <= float(n - 1 + e)) & ~nan
    q = torch.clamp(p, -float(e), float(n - 1 + e)) + float(e)
    if not exact:
        q = _st(q, torch.clamp(p.detach().float(), -float(e), float(n - 1 + e)) + float(e))
    q0f = torch.floor(q.detach())
    i1 = torch.minimum(q0f + 1.0, torch.full_like(q0f, float(n - 1 + 2 * e))).long()
    return (q, q0f, q0f.long(), i1), passed


class Sampled:
    """One forward through the graph: `out` (fp64) and what `backward` needs."""


def _sample(vol64, xn, yn, zn, out_size, e, exact):
    B, D, H, W, C = vol64.shape
    nvox = out_size[0] * out_size[1] * out_size[2]
    ax, px = _axis_graph(xn, W, e, exact)
    ay, py = _axis_graph(yn, H, e, exact)
    az, pz = _axis_graph(zn, D, e, exact)
    volp = F.pad(vol64, (0, 0, e, e, e, e, e, e)).reshape(-1, C)
    out, idx, wts, (wx, wy, wz) = _blend(volp, B, nvox, (D + 2 * e, H + 2 * e, W + 2 * e), (ax, ay, az))
    s = Sampled()
    s.out, s.idx, s.wts = out, idx, [w.detach() for w in wts]
    s.taps = [volp[i].detach() for i in idx]
    s.wx, s.wy, s.wz = [w.detach() for w in wx], [w.detach() for w in wy], [w.detach() for w in wz]
    s.passed = (px, py, pz)
    s.shape, s.e = (B, D, H, W, C), e
    return s


def grad_bilinear_interp3d(vol, x, y, z, out_size, edge_size=1, exact=False):
    """-> (Sampled, leaves (vol64, x64, y64, z64)).  x, y, z are rounded to fp32 first unless `exact`."""
    vol64 = torch.as_tensor(vol).double().clone().requires_grad_(True)
    cast = (lambda t: torch.as_tensor(t).double()) if exact else (lambda t: torch.as_tensor(t).float().double())
    c = [cast(t).reshape(-1).clone().requires_grad_(True) for t in (x, y, z)]
    s = _sample(vol64, c[0], c[1], c[2], out_size, int(edge_size), exact)
    s.kind = "coords"
    return s, (vol64, c[0], c[1], c[2])


def grad_transform(vol, theta, out_size, exact=False):
    """AffineVolumeTransformer.transform -> (Sampled with out [B,od,oh,ow,C], leaves (vol64, theta64 [B,12]))."""
    vol64 = torch.as_tensor(vol).double().clone().requires_grad_(True)
    B, C = vol64.shape[0], vol64.shape[4]
    th32 = torch.as_tensor(theta).float().reshape(B, 12)
    th = (torch.as_tensor(theta).double().reshape(B, 12) if exact else th32.double()).clone().requires_grad_(True)
    g = meshgrid3d(out_size).reshape(4, -1)                                   # fp32 linspace values
    xt, yt, zt = g[0], g[1], g[2]
    rows = []
    for r in range(3):
        k = 4 * r
        v = ((th[:, k:k + 1] * xt.double() + th[:, k + 1:k + 2] * yt.double()) + th[:, k + 2:k + 3] * zt.double()) + th[:, k + 3:k + 4]
        if not exact:
            v = _st(v, ((th32[:, k:k + 1] * xt + th32[:, k + 1:k + 2] * yt) + th32[:, k + 2:k + 3] * zt) + th32[:, k + 3:k + 4])
        rows.append(v.reshape(-1))
    s = _sample(vol64, rows[0], rows[1], rows[2], out_size, 1, exact)
    s.out = s.out.reshape(B, *out_size, C)
    s.kind = "theta"
    s.grid = (xt.double(), yt.double(), zt.double())
    return s, (vol64, th)


def backward(s, leaves, dout):
    """Gradients of sum(out * dout) by autograd, and the counts / absolute companions of the module docstring.
    Keys: d_vol, n_vol, S_vol; coords: d_x, d_y, d_z, S_x, S_y, S_z; theta: d_theta, S_theta."""
    B, D, H, W, C = s.shape
    e = s.e
    dout = torch.as_tensor(dout).double().reshape(s.out.shape)
    grads = torch.autograd.grad(s.out, leaves, dout, allow_unused=True)
    r = {"d_vol": grads[0]}
    ad = dout.abs().reshape(-1, C)
    Dp, Hp, Wp = D + 2 * e, H + 2 * e, W + 2 * e
    n_vol = torch.zeros((B * Dp * Hp * Wp,), dtype=torch.float64)
    S_vol = torch.zeros((B * Dp * Hp * Wp, C), dtype=torch.float64)
    for w, i in zip(s.wts, s.idx):
        n_vol.index_add_(0, i, torch.ones_like(w))
        S_vol.index_add_(0, i, w.unsqueeze(1) * ad)
    core = (slice(None), slice(e, e + D), slice(e, e + H), slice(e, e + W))
    r["n_vol"] = n_vol.reshape(B, Dp, Hp, Wp)[core].unsqueeze(-1).expand(B, D, H, W, C)
    r["S_vol"] = S_vol.reshape(B, Dp, Hp, Wp, C)[core]
    a = [t.abs() for t in s.taps]

    def companion(bit, wa, wb):
        """axis with tap-index bit `bit`: sum over the other two axes' pairs of (|I0| + |I1|) * pair weight"""
        other = [b for b in (4, 2, 1) if b != bit]
        tot = 0.0
        for ka in (0, 1):
            for kb in (0, 1):
                k0 = ka * other[0] + kb * other[1]
                tot = tot + (a[k0] + a[k0 + bit]) * (wa[ka] * wb[kb]).unsqueeze(1)
        return (ad * tot).sum(1)

    S_x = companion(1, s.wz, s.wy) * (0.5 * (W - 1)) * s.passed[0]
    S_y = companion(2, s.wz, s.wx) * (0.5 * (H - 1)) * s.passed[1]
    S_z = companion(4, s.wy, s.wx) * (0.5 * (D - 1)) * s.passed[2]
    if s.kind == "coords":
        r["d_x"], r["d_y"], r["d_z"], r["S_x"], r["S_y"], r["S_z"] = grads[1], grads[2], grads[3], S_x, S_y, S_z
        return r
    xt, yt, zt = (t.abs() for t in s.grid)
    cols = []
    for S in (S_x, S_y, S_z):
        S = S.reshape(B, -1)
        cols += [S * xt, S * yt, S * zt, S]
    r["d_theta"] = grads[1]
    r["S_theta"] = torch.stack([c.sum(1) for c in cols], 1)
    return r
