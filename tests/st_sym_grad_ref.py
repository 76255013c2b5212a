"""Reference for the gradients of the symmetric-pad spatial transformers ("ST" = the reference's spatial_transformer.py):
SimilarityTransformer (ST:311-371), AffineSymmetryTransformer (ST:454-517) and ProjectiveSymmetryTransformer (ST:611-716) with the
bilinear sampler, differentiated by torch.autograd in fp64 -- what TensorFlow's autodiff gives for the same op sequence, in the
style of tests/st_grad_ref.py (whose `_st`, `_axis` and `_sample` it uses).

The exact fp64 expression: pre-map of theta -> M . (x_t, y_t, 1) on the linspace grid of (oh+200) x (ow+200) points (/ z for the
projective kind, no safe_z) -> bilinear sample of F.pad-by-one of the explicitly symmetric-padded image (an index gather, so autograd
folds the pad's adjoint) -> crop-or-pad to [B, ow, oh, C].  The VALUES at every rounded step are the device's: the pre-mapped
matrices (`matrix()`) and the source coordinates per final pixel (`transform_coords()`) are given as fp32 tensors and brought into
the graph by the straight-through substitution `_st` (the value of the fp32 number, the derivative of the fp64 expression); the rows
x_h, y_h, z in between are the fp32 sequence (m0 x + m1 y) + m2 of those matrices; the similarity angle and scale are the fp32
a = theta0 * (float)(3.14/6) + 0, s = theta1 * 0.1f + 1, with cos / sin taken in fp64 OF that fp32 angle.  Without device values the
matrices come from st_extended_ref.sym_theta (fp32 numpy) and the coordinates from the fp32 division on the CPU.  `exact=True`
drops every substitution: a plain fp64 function, which is what central differences can be taken of.

`backward` returns, besides the gradients, per gradient element the count `n` of contributions and the absolute companion `S`
(st_grad_ref's docstring).  For d img, n counts the FOLDED taps: every padded tap of a kept pixel that lands on the image pixel
through the symmetric pad (n_pad, S_pad are the same per padded pixel, before the fold).  For d theta, S is carried through the
pre-map with absolute factors: S_M per matrix entry, then |P|, or |s sin a|, |s cos a|, |cos a|, |sin a| and the interleave."""
import numpy as np
import torch

from oracle import vstab_oracle as vo
from tests import st_extended_ref as xref
from tests.st_grad_ref import Sampled, _sample, _st          # noqa: F401

f32 = np.float32
PDIM = {'affine': 6, 'projective': 8, 'similarity': 4}
KIND = {'affine': 0, 'projective': 1, 'similarity': 2}          # VSTAB_SYM_*
_C_AFF = np.array([.1, 0, .2, .1, 0, .2], f32)
_I_AFF = np.array([1, 0, 0, 0, 1, 0], f32)
_P = np.array([0.01, 0.005, 0.01, 0.01, 0.005, 0.01, 0.01, 0.01, 1], f32)
_A = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], f32)
_SIM_SCALE = np.array([3.14 / 6, 0.1, 0.2, 0.2], f32)
_SIM_SHIFT = np.array([0, 1, 0, 0], f32)


def _d(a):
    return torch.from_numpy(np.asarray(a, f32).astype(np.float64))


def crop_geometry(oh, ow):
    """resize_image_with_crop_or_pad of the (oh+200) x (ow+200) grid to height ow, width oh: (gh, gw, FH, FW, cy, py, ly, cx, px, lx)."""
    gh, gw, FH, FW = oh + 200, ow + 200, ow, oh
    return (gh, gw, FH, FW, max((gh - FH) // 2, 0), max((FH - gh) // 2, 0), min(gh, FH), max((gw - FW) // 2, 0), max((FW - gw) // 2, 0),
            min(gw, FW))


def to_grid(final, oh, ow, fill=0.0):
    """[B, FH, FW, ...] -> [B, gh, gw, ...]: the crop-or-pad's adjoint (kept window copied, `fill` elsewhere)."""
    gh, gw, FH, FW, cy, py, ly, cx, px, lx = crop_geometry(oh, ow)
    full = torch.full((final.shape[0], gh, gw) + tuple(final.shape[3:]), fill, dtype=final.dtype)
    full[:, cy:cy + ly, cx:cx + lx] = final[:, py:py + ly, px:px + lx]
    return full


def to_final(full, oh, ow):
    """[B, gh, gw, ...] -> [B, FH, FW, ...]: the crop-or-pad itself (zeros where it pads)."""
    gh, gw, FH, FW, cy, py, ly, cx, px, lx = crop_geometry(oh, ow)
    out = torch.zeros((full.shape[0], FH, FW) + tuple(full.shape[3:]), dtype=full.dtype)
    out[:, py:py + ly, px:px + lx] = full[:, cy:cy + ly, cx:cx + lx]
    return out


def fold(t, H, W):
    """The symmetric pad's adjoint: [B, H+200, W+200, ...] -> [B, H, W, ...], padded pixel p added to image pixel refl(p - 100)."""
    ridx = torch.from_numpy(xref.refl(np.arange(H + 200) - 100, H).astype(np.int64))
    cidx = torch.from_numpy(xref.refl(np.arange(W + 200) - 100, W).astype(np.int64))
    rows = torch.zeros((t.shape[0], H) + tuple(t.shape[2:]), dtype=t.dtype).index_add_(1, ridx, t)
    return torch.zeros((t.shape[0], H, W) + tuple(t.shape[3:]), dtype=t.dtype).index_add_(2, cidx, rows)


def _premap(kind, th, th32, exact):
    """theta [B, pdim] (fp64 graph) -> (M [B, 6|9] fp64 graph, aux for the companions)."""
    B = th.shape[0]
    if kind == 'affine':
        return (th * _d(_C_AFF)) * 0.0 + _d(_I_AFF), None
    if kind == 'projective':
        return torch.cat([th, torch.ones((B, 1), dtype=torch.float64)], 1) * _d(_P) + _d(_A), None
    t = th * _d(_SIM_SCALE) + _d(_SIM_SHIFT)
    a, s = t[:, 0], t[:, 1]
    if not exact:
        sc = torch.from_numpy(_SIM_SCALE)
        a = _st(a, th32[:, 0] * sc[0] + np.float32(0.0))
        s = _st(s, th32[:, 1] * sc[1] + np.float32(1.0))
    ca, sa = torch.cos(a), torch.sin(a)
    flat = torch.cat([s * ca, s * sa, t[:, 2], (-s) * sa, s * ca, t[:, 3]], 0)          # ST:358: six [B] vectors on axis 0
    return flat.reshape(B, 6), (a.detach(), s.detach())                                   # ST:360: interleaved for B > 1


def transform(kind, im, theta, out_size, M32=None, xs32=None, ys32=None, exact=False):
    """-> (Sampled with out [B, ow, oh, C] (the affine kind's relabelling reshape is left to the caller), leaves (im64, theta64)).
    M32 [B,3,3] / xs32, ys32 [B*ow*oh]: the device's matrices and per-final-pixel coordinates (fp32), or None."""
    oh, ow = int(out_size[0]), int(out_size[1])
    gh, gw, FH, FW, cy, py, ly, cx, px, lx = crop_geometry(oh, ow)
    im64 = torch.as_tensor(im).double().clone().requires_grad_(True)
    B, H, W, C = im64.shape
    th32 = torch.as_tensor(theta).float().reshape(B, PDIM[kind])
    th = (torch.as_tensor(theta).double().reshape(B, PDIM[kind]) if exact else th32.double()).clone().requires_grad_(True)
    M, aux = _premap(kind, th, th32, exact)
    nc = M.shape[1]
    if not exact:
        m32 = (torch.as_tensor(M32).float().reshape(B, 9)[:, :nc] if M32 is not None
               else torch.from_numpy(xref.sym_theta(kind, th32.numpy()).astype(f32)).reshape(B, nc))
        M = _st(M, m32)
    grid = torch.from_numpy(vo.st_meshgrid((gh, gw))).reshape(3, -1)          # fp32 linspace values
    xt, yt = grid[0], grid[1]

    def row(k):                                                                # (m_k x + m_k+1 y) + m_k+2, fp64 graph + fp32 values
        v = (M[:, k:k + 1] * xt.double() + M[:, k + 1:k + 2] * yt.double()) + M[:, k + 2:k + 3]
        return v if exact else _st(v, (m32[:, k:k + 1] * xt + m32[:, k + 1:k + 2] * yt) + m32[:, k + 2:k + 3])

    xh, yh = row(0), row(3)
    z = row(6) if kind == 'projective' else None
    xs, ys = (xh / z, yh / z) if z is not None else (xh, yh)
    if not exact:
        x32 = xh.detach().float() / z.detach().float() if z is not None else xh.detach().float()
        y32 = yh.detach().float() / z.detach().float() if z is not None else yh.detach().float()
        if xs32 is not None:                                                   # the device's values on the kept window
            x32 = x32.reshape(B, gh, gw).clone()
            y32 = y32.reshape(B, gh, gw).clone()
            x32[:, cy:cy + ly, cx:cx + lx] = torch.as_tensor(xs32).float().reshape(B, FH, FW)[:, py:py + ly, px:px + lx]
            y32[:, cy:cy + ly, cx:cx + lx] = torch.as_tensor(ys32).float().reshape(B, FH, FW)[:, py:py + ly, px:px + lx]
        xs, ys = _st(xs, x32.reshape(B, -1)), _st(ys, y32.reshape(B, -1))
    ridx = torch.from_numpy(xref.refl(np.arange(H + 200) - 100, H).astype(np.int64))
    cidx = torch.from_numpy(xref.refl(np.arange(W + 200) - 100, W).astype(np.int64))
    padded = im64[:, ridx][:, :, cidx]                                         # np.pad(mode='symmetric') by 100, as a gather
    s = _sample(padded, xs.reshape(-1), ys.reshape(-1), (gh, gw), exact)
    s.out = to_final(s.out.reshape(B, gh, gw, C), oh, ow)
    s.kind, s.out_size, s.img_shape = kind, (oh, ow), (B, H, W, C)
    s.xt, s.yt = xt.double(), yt.double()
    s.xh, s.yh, s.z = xh.detach(), yh.detach(), (z.detach() if z is not None else None)
    s.aux = aux
    return s, (im64, th)


def backward(s, leaves, dout):
    """Gradients of sum(out * dout) by autograd, and the counts / absolute companions of the module docstring.
    Keys: d_img, n_img, S_img (image shape), n_pad, S_pad (padded-image shape), d_theta, S_theta, S_M."""
    B, H, W, C = s.img_shape
    Hp, Wp = H + 200, W + 200
    oh, ow = s.out_size
    dout = torch.as_tensor(dout).double().reshape(s.out.shape)
    grads = torch.autograd.grad(s.out, leaves, dout, allow_unused=True)
    r = {"d_img": grads[0], "d_theta": grads[1] if grads[1] is not None else torch.zeros_like(leaves[1])}
    ad = to_grid(dout.abs(), oh, ow).reshape(-1, C)                            # |dout| per grid point, 0 where the crop drops it
    kept = to_grid(torch.ones(dout.shape[:3], dtype=torch.float64), oh, ow).reshape(-1)
    n_p = torch.zeros((B * (Hp + 2) * (Wp + 2),), dtype=torch.float64)
    S_p = torch.zeros((B * (Hp + 2) * (Wp + 2), C), dtype=torch.float64)
    for w, i in zip(s.wts, s.idx):
        n_p.index_add_(0, i, kept)
        S_p.index_add_(0, i, w.unsqueeze(1) * ad)
    r["n_pad"] = n_p.reshape(B, Hp + 2, Wp + 2)[:, 1:-1, 1:-1].unsqueeze(-1).expand(B, Hp, Wp, C)
    r["S_pad"] = S_p.reshape(B, Hp + 2, Wp + 2, C)[:, 1:-1, 1:-1]
    r["n_img"] = fold(r["n_pad"].contiguous(), H, W)
    r["S_img"] = fold(r["S_pad"].contiguous(), H, W)
    a00, a01, a10, a11 = (t.abs() for t in s.taps)
    S_x = (ad * ((a00 + a01) * s.hy.unsqueeze(1) + (a10 + a11) * s.ly.unsqueeze(1))).sum(1) * (0.5 * (Wp - 1)) * s.pass_x
    S_y = (ad * ((a00 + a10) * s.hx.unsqueeze(1) + (a01 + a11) * s.lx.unsqueeze(1))).sum(1) * (0.5 * (Hp - 1)) * s.pass_y
    S_x, S_y = S_x.reshape(B, -1), S_y.reshape(B, -1)
    ax, ay = s.xt.abs(), s.yt.abs()
    cols = []
    if s.kind == 'projective':
        S_z = (S_x * s.xh.abs() + S_y * s.yh.abs()) / (s.z * s.z)
        S_x, S_y = S_x / s.z.abs(), S_y / s.z.abs()
        cols = [S_z * ax, S_z * ay]
    S_M = torch.stack([c.sum(1) for c in [S_x * ax, S_x * ay, S_x, S_y * ax, S_y * ay, S_y] + cols], 1)
    r["S_M"] = S_M
    if s.kind == 'affine':
        r["S_theta"] = S_M * 0.0                                              # the pre-map multiplies by 0
    elif s.kind == 'projective':
        r["S_theta"] = S_M * _d(_P[:8])
    else:
        a, sc = s.aux
        SE = S_M.reshape(-1).reshape(6, B)                                    # undo the interleave: SE[v][b] = S_M[n][k], 6n + k = vB + b
        sum_c, sum_s = SE[0] + SE[4], SE[1] + SE[3]
        S_a = sc.abs() * a.sin().abs() * sum_c + sc.abs() * a.cos().abs() * sum_s
        S_s = a.cos().abs() * sum_c + a.sin().abs() * sum_s
        k = _d(_SIM_SCALE)
        r["S_theta"] = torch.stack([S_a * k[0], S_s * k[1], SE[2] * k[2], SE[5] * k[3]], 1)
    return r
