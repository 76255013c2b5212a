"""Drop-ins for the 2-D samplers of the reference's `spatial_transformer.py`: `transformer` (:34-38),
`ElasticTransformer` (:40-224), `AffineVolumeTransformer` (:227-308), `SimilarityTransformer` (:311-371), `AffineTransformer` (:373-452),
`AffineSymmetryTransformer` (:454-517), `ProjectiveTransformer` (:519-608), `ProjectiveSymmetryTransformer`
(:611-716), `_meshgrid3d` (:725-753), `_meshgrid` (:755-779), `_repeat` (:782-785), `_interpolate` (:787-792), `_interpolate3d` (:794-795),
`bilinear_interp3d` (:797-899), `bilinear_interp` (:902-964) and `bicubic_interp` (:966-1072).  None of them is executed by the reference's runnable scripts (they are only
imported, main:4 and cell.py:2); the arithmetic runs in HIP kernels (csrc/sampler_ops.hip, csrc/sampler3d_ops.hip for the volume transformer).

Differentiable (torch.autograd, HIP backward kernels): `AffineTransformer.transform`, `ProjectiveTransformer.transform`,
`ElasticTransformer.transform`, `SimilarityTransformer.transform`, `AffineSymmetryTransformer.transform`,
`ProjectiveSymmetryTransformer.transform` and `transformer()` with the bilinear sampler, with respect to the image and `theta` (for the
elastic one: the control-point offsets; for the symmetric-pad ones: through each class's pre-map, which makes `AffineSymmetryTransformer`'s
theta gradient exactly zero and couples the samples of a `SimilarityTransformer` batch), and `bilinear_interp` with respect to the image, `x` and `y`; `AffineVolumeTransformer.transform` with respect to the volume and `theta`, `bilinear_interp3d` with respect to the
volume, `x`, `y` and `z`.  The gradient of the image or volume is summed by float atomics (last bits may differ between runs); those of `theta`, `x`, `y`,
`z` are bit-reproducible.  The BICUBIC sampler is differentiable on request: `bicubic_interp(..., differentiable=True)` and
`differentiable=True` on the constructor of `AffineTransformer`, `ProjectiveTransformer`, `SimilarityTransformer`,
`AffineSymmetryTransformer`, `ProjectiveSymmetryTransformer` or `ElasticTransformer` (passed through by `transformer()`) with
`interp_method='bicubic'` go through HIP backward kernels too -- the image's gradient by float atomics (all 16 taps add, the
replicated edge taps onto their one pixel), those of `theta`, `x`, `y` reproducible, zero where a coordinate lies outside [-1, 1] or is
NaN (the sampler's clip).  Without the keyword a bicubic result has no `grad_fn`, whatever requires grad; with the bilinear sampler
the keyword changes nothing.  NOT differentiable: `ElasticTransformer.transform_coords`, and the symmetric-pad transformers'
`matrix` and `transform_coords`.
The homography samplers of the reference's `warp.py` (`warp.transformImage` and its kin) are differentiable too: see `warp.py`."""
from __future__ import annotations

import numpy as np
import torch

from . import _autograd, _lib, runtime, training          # the backward wrappers under their public names (sampler_grad's, re-exported)
from .runtime import f32_cuda as _f32_cuda

_INTERP = _lib.INTERP


def _meshgrid(out_size, device=None):
    """Flat [3*H*W] sampling grid: linspace(-1,1,W) as x (fastest), linspace(-1,1,H) as y, ones."""
    runtime._require_gpu()
    oh, ow = int(out_size[0]), int(out_size[1])
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    out = torch.empty(3 * oh * ow, dtype=torch.float32, device=dev)
    runtime.call(dev, "vstab_st_meshgrid", out.data_ptr(), oh, ow)
    return out


def _repeat(x, n_repeats):
    """tile(expand_dims(x, 1), [1, n]) flattened: every element repeated n times in place."""
    return x.reshape(-1, 1).repeat(1, int(n_repeats)).reshape(-1)


def _flat(d_theta):
    return d_theta.reshape(-1) if d_theta is not None else None


def _bilinear_interp_call(im, x, y, oh, ow):
    B, H, W, Cc = im.shape
    out = torch.empty((B * oh * ow, Cc), dtype=torch.float32, device=im.device)
    runtime.call(im.device, "vstab_st_bilinear_interp", im.data_ptr(), B, H, W, Cc, x.data_ptr(), y.data_ptr(), oh, ow, out.data_ptr())
    return out


def _bilinear_interp_backward(saved, dout, needs, out_size):
    return training.st_bilinear_interp_backward(*saved, dout, out_size, need_img=needs[0], need_x=needs[1], need_y=needs[2])


def bilinear_interp(im, x, y, out_size):
    """im [B,H,W,C]; x, y flat [B*out_h*out_w] normalised to [-1,1] -> [B*out_h*out_w, C].
    The image is zero-padded by one pixel; coordinates are clipped to [-1, W] / [-1, H].
    Differentiable with respect to im, x and y (module docstring)."""
    im = _f32_cuda(im, "im")
    B, H, W, Cc = im.shape
    x = _f32_cuda(x.to(torch.float32), "x").reshape(-1)
    y = _f32_cuda(y.to(torch.float32), "y").reshape(-1)
    oh, ow = int(out_size[0]), int(out_size[1])
    npix = oh * ow
    if x.numel() != B * npix or y.numel() != B * npix:
        raise ValueError(f"x/y must have B*out_h*out_w = {B * npix} elements")
    return _autograd.apply(_bilinear_interp_call, _bilinear_interp_backward, (im, x, y), (oh, ow))


def _bicubic_interp_call(im, x, y, oh, ow):
    B, H, W, Cc = im.shape
    out = torch.empty((B * oh * ow, Cc), dtype=torch.float32, device=im.device)
    runtime.call(im.device, "vstab_st_bicubic_interp", im.data_ptr(), B, H, W, Cc, x.data_ptr(), y.data_ptr(), oh, ow, out.data_ptr())
    return out


def _bicubic_interp_backward(saved, dout, needs, out_size):
    return training.st_bicubic_interp_backward(*saved, dout, out_size, need_img=needs[0], need_x=needs[1], need_y=needs[2])


def bicubic_interp(im, x, y, out_size, differentiable=False):
    """im [B,H,W,C]; x, y flat [B*out_h*out_w] normalised to [-1,1] -> [B*out_h*out_w, C].
    Coordinates are clipped to [-1, 1] before the scaling (NaN reads as -1); 4 x 4 taps, edges replicate
    (no zero border), alpha = -0.75.  differentiable=True: with respect to im, x and y (module docstring); otherwise the result
    carries no graph."""
    im = _f32_cuda(im, "im")
    B, H, W, Cc = im.shape
    x = _f32_cuda(x.to(torch.float32), "x").reshape(-1)
    y = _f32_cuda(y.to(torch.float32), "y").reshape(-1)
    oh, ow = int(out_size[0]), int(out_size[1])
    npix = oh * ow
    if x.numel() != B * npix or y.numel() != B * npix:
        raise ValueError(f"x/y must have B*out_h*out_w = {B * npix} elements")
    return _autograd.apply(_bicubic_interp_call, _bicubic_interp_backward, (im, x, y), (oh, ow), differentiable)


def _interpolate(im, x, y, out_size, method):
    if method == 'bilinear':
        return bilinear_interp(im, x, y, out_size)
    if method == 'bicubic':
        return bicubic_interp(im, x, y, out_size)
    return None            # the reference falls through to None for unknown methods (:792)


def _interp_code(method):
    if method not in _INTERP:
        raise NotImplementedError(f"interp_method must be 'bilinear' or 'bicubic', not {method!r}")
    return _INTERP[method]


def _theta_transform_call(inp, theta, param_dim, oh, ow, interp):
    B, H, W, Cc = inp.shape
    out = torch.empty((B, oh, ow, Cc), dtype=torch.float32, device=inp.device)
    if interp == 0:
        runtime.call(inp.device, "vstab_st_transform", inp.data_ptr(), B, H, W, Cc, theta.data_ptr(), param_dim, out.data_ptr(), oh, ow)
    else:
        runtime.call(inp.device, "vstab_st_transform_interp", inp.data_ptr(), B, H, W, Cc, theta.data_ptr(), param_dim, interp, out.data_ptr(),
                     oh, ow)
    return out


def _theta_transform_backward(saved, dout, needs, statics):
    _, oh, ow, interp = statics
    d_inp, d_theta = training.st_transform_backward(*saved, dout, (oh, ow), need_img=needs[0], need_theta=needs[1],
                                                    interp=_lib.INTERP_NAMES[interp])
    return d_inp, _flat(d_theta)


class _ThetaTransformer(object):
    param_dim = 0

    def __init__(self, out_size, name, interp_method='bilinear', differentiable=False, **kwargs):
        self.name = name
        self.out_size = (int(out_size[0]), int(out_size[1]))
        self.interp_method = interp_method
        self.differentiable = bool(differentiable)          # the bicubic sampler's graph is opt-in; the bilinear one always has it
        self._grid = None

    @property
    def pixel_grid(self):
        if self._grid is None:
            self._grid = _meshgrid(self.out_size)
        return self._grid

    def transform(self, inp, theta):
        interp = _interp_code(self.interp_method)
        inp = _f32_cuda(inp, "inp")
        B, H, W, Cc = inp.shape
        theta = _f32_cuda(theta.to(torch.float32), "theta").reshape(-1)
        if theta.numel() != B * self.param_dim:
            raise ValueError(f"theta must have shape [{B}, {self.param_dim}]")
        return _autograd.apply(_theta_transform_call, _theta_transform_backward, (inp, theta), (self.param_dim, *self.out_size, interp),
                               interp == 0 or self.differentiable)


class AffineTransformer(_ThetaTransformer):
    """theta [B,6] = row-major 2x3 matrix acting on (x_t, y_t, 1), x_t, y_t in [-1,1].  With the bilinear sampler `transform` is
    differentiable with respect to the image and theta; with the bicubic one when constructed with differentiable=True."""
    param_dim = 6

    def __init__(self, out_size, name='SpatialAffineTransformer', interp_method='bilinear', differentiable=False, **kwargs):
        super().__init__(out_size, name, interp_method, differentiable, **kwargs)


class ProjectiveTransformer(_ThetaTransformer):
    """theta [B,8] = first 8 entries of a 3x3 homography (last entry 1); divides by z,
    z == 0 replaced by 1e-8 (:598).  With the bilinear sampler `transform` is differentiable with respect to the image and theta
    (8 entries per sample: the ninth is the constant 1); with the bicubic one when constructed with differentiable=True."""
    param_dim = 8

    def __init__(self, out_size, name='SpatialProjectiveTransformer', interp_method='bilinear', differentiable=False, **kwargs):
        super().__init__(out_size, name, interp_method, differentiable, **kwargs)


def _symmetry_transform_call(inp, theta, kind, oh, ow, interp):
    B, H, W, Cc = inp.shape
    out = torch.empty((B, ow, oh, Cc), dtype=torch.float32, device=inp.device)
    runtime.call(inp.device, "vstab_st_symmetry_transform", inp.data_ptr(), B, H, W, Cc, theta.data_ptr(), kind, interp, out.data_ptr(), oh, ow)
    return out


def _symmetry_transform_backward(saved, dout, needs, statics):
    kind, oh, ow, interp = statics
    d_inp, d_theta = training.st_symmetry_transform_backward(*saved, dout, (oh, ow), kind, need_img=needs[0], need_theta=needs[1],
                                                             interp=_lib.INTERP_NAMES[interp])
    return d_inp, _flat(d_theta)


class _SymmetryTransformer(object):
    """The symmetric-pad transformers (ST:311-371, 454-517, 611-716): the input padded by 100 px per side in SYMMETRIC mode
    (H, W >= 100, as tf.pad requires; never materialised), sampled on the linspace grid of (oh+200) x (ow+200) points, then
    tf.image.resize_image_with_crop_or_pad(out, out_size[1], out_size[0]) -- target height ow, width oh: the result is
    [B, ow, oh, C].  For square outputs the swap does not show.  With the bilinear sampler `transform` is differentiable with
    respect to the image and theta (through the pre-map of each class); with the bicubic one when constructed with
    differentiable=True (no `grad_fn` otherwise)."""
    param_dim = 0
    kind = -1

    def __init__(self, out_size, name, interp_method='bilinear', differentiable=False, **kwargs):
        self.name = name
        self.out_size = (int(out_size[0]), int(out_size[1]))
        self.interp_method = interp_method
        self.differentiable = bool(differentiable)

    def _theta(self, theta, B=None):
        theta = _f32_cuda(theta.to(torch.float32), "theta").reshape(-1)
        if theta.numel() == 0 or theta.numel() % self.param_dim or (B is not None and theta.numel() != B * self.param_dim):
            raise ValueError(f"theta must have shape [{'B' if B is None else B}, {self.param_dim}]")
        return theta

    def transform(self, inp, theta):
        interp = _interp_code(self.interp_method)
        inp = _f32_cuda(inp, "inp")
        B, H, W, Cc = inp.shape
        if H < 100 or W < 100:
            raise ValueError(f"{type(self).__name__}: the 100-pixel symmetric pad needs H, W >= 100, got {H}x{W}")
        theta = self._theta(theta, B)
        return _autograd.apply(_symmetry_transform_call, _symmetry_transform_backward, (inp, theta), (self.kind, *self.out_size, interp),
                               interp == 0 or self.differentiable)

    def matrix(self, theta):
        """theta [B, param_dim] -> [B,3,3]: the pre-mapped matrices `transform` multiplies the grid by (affine kinds: last row 0 0 1),
        bit for bit -- the same device code computes them, SimilarityTransformer's interleave across samples included.  Forward
        only: the result carries no graph."""
        theta = self._theta(theta.detach())
        B = theta.numel() // self.param_dim
        out = torch.empty((B, 3, 3), dtype=torch.float32, device=theta.device)
        runtime.call(theta.device, "vstab_st_symmetry_matrix", theta.data_ptr(), B, self.kind, out.data_ptr())
        return out

    def transform_coords(self, theta):
        """theta [B, param_dim] -> (x_s, y_s), each flat [B*ow*oh] in the output's layout: the normalised source coordinates, on the
        (H+200) x (W+200) padded extent, that `transform` samples every final pixel at, bit for bit; 0 where the crop-or-pad pads.
        Needs no image.  Forward only: the results carry no graph."""
        theta = self._theta(theta.detach())
        B = theta.numel() // self.param_dim
        oh, ow = self.out_size
        x_s = torch.empty(B * oh * ow, dtype=torch.float32, device=theta.device)
        y_s = torch.empty_like(x_s)
        runtime.call(theta.device, "vstab_st_symmetry_coords", theta.data_ptr(), B, self.kind, oh, ow, x_s.data_ptr(), y_s.data_ptr())
        return x_s, y_s


class SimilarityTransformer(_SymmetryTransformer):
    """theta [B,4] = (angle, scale, tx, ty) pre-mapped by * [3.14/6, .1, .2, .2] + [0, 1, 0, 0] (ST:356-357) into
    [s cos a, s sin a, tx; -s sin a, s cos a, ty].  The reference concatenates the six [B] vectors on axis 0 before the
    reshape to [B,2,3] (ST:358-360), so for B > 1 the matrices interleave across samples ("BatchSize Should be One",
    ST:355); that order is kept.  Output [B, ow, oh, C].  With the bilinear sampler `transform` is differentiable with respect to
    the image and theta; for B > 1 the interleave makes a sample's output depend on other samples' theta, and the gradient follows it."""
    param_dim = 4
    kind = 2

    def __init__(self, out_size, name='SpatialAffineTransformer', interp_method='bilinear', differentiable=False, **kwargs):
        super().__init__(out_size, name, interp_method, differentiable, **kwargs)


class AffineSymmetryTransformer(_SymmetryTransformer):
    """theta [B,6] pre-mapped by * [[.1,0,.2],[.1,0,.2]] * 0 + I (ST:503-505): the identity for any finite theta (NaN / inf
    still propagate).  The [B, ow, oh, C] crop is relabelled [B, oh, ow, C] by a reshape, as the reference does (ST:492).  With the
    bilinear sampler `transform` is differentiable: the image's gradient arrives through the reshape, theta's is exactly zero (the
    pre-map multiplies it by 0) unless a non-finite gradient propagates."""
    param_dim = 6
    kind = 0

    def __init__(self, out_size, name='SpatialAffineTransformer', interp_method='bilinear', differentiable=False, **kwargs):
        super().__init__(out_size, name, interp_method, differentiable, **kwargs)

    def transform(self, inp, theta):
        out = super().transform(inp, theta)
        return out.reshape(out.shape[0], self.out_size[0], self.out_size[1], out.shape[3])


class ProjectiveSymmetryTransformer(_SymmetryTransformer):
    """theta [B,8]: [theta, 1] * [[.01,.005,.01],[.01,.005,.01],[.01,.01,1]] + [[1,0,0],[0,1,0],[0,0,0]] (ST:692-699), divided
    by z with no safe_z (ST:710-711).  Output [B, ow, oh, C].  With the bilinear sampler `transform` is differentiable with respect to
    the image and theta (z == 0 propagates by IEEE rules, as in the reference)."""
    param_dim = 8
    kind = 1

    def __init__(self, out_size, name='SpatialProjectiveTransformer', interp_method='bilinear', differentiable=False, **kwargs):
        super().__init__(out_size, name, interp_method, differentiable, **kwargs)


def _tps_linv(g):
    """transpose(L_inv[:,3:]) [g*g, g*g+3] of ElasticTransformer._initialize_tps (ST:187-225), inverted in double on the host
    and rounded to fp32."""
    K = g * g
    buf = np.empty((K, K + 3), dtype=np.float32)
    _lib.check(_lib.lib().vstab_host_tps_linv(int(g), buf.ctypes.data, buf.size))
    return buf


def _elastic_transform_call(inp, theta, linv_t, g, oh, ow, interp):
    B, H, W, Cc = inp.shape
    out = torch.empty((B, oh, ow, Cc), dtype=torch.float32, device=inp.device)
    runtime.call(inp.device, "vstab_st_elastic_transform", inp.data_ptr(), B, H, W, Cc, theta.data_ptr(), g, linv_t.data_ptr(), interp,
                 out.data_ptr(), oh, ow)
    return out


def _elastic_transform_backward(saved, dout, needs, statics):
    inp, theta, linv_t = saved
    g, oh, ow, interp = statics
    d_inp, d_theta = training.st_elastic_transform_backward(inp, theta, dout, (oh, ow), g, linv_t, need_img=needs[0], need_theta=needs[1],
                                                            interp=_lib.INTERP_NAMES[interp])
    return d_inp, _flat(d_theta), None


class ElasticTransformer(object):
    """Thin-plate spline transformer (ST:40-224).  param_dim = g, the side of the g x g control grid (linspace(-1,1,g)
    meshgrid, x fastest); theta [B, 2*g*g] = x offsets then y offsets of the control points.  L_inv is computed once at
    construction, in double, and kept on the device as fp32 transpose(L_inv[:,3:]); the kernel computes each sample's
    coefficients once and U = r^2 ln r^2 per output pixel.  Output [B, oh, ow, C].  With the bilinear sampler `transform` is
    differentiable with respect to the image and theta; with the bicubic one when constructed with differentiable=True (no `grad_fn`
    otherwise)."""

    def __init__(self, out_size, param_dim, name='SpatialElasticTransformer', interp_method='bilinear', differentiable=False, **kwargs):
        g = int(param_dim)
        if g < 2:
            raise ValueError("ElasticTransformer: param_dim (control grid side) must be >= 2; g = 1 makes L singular")
        self.name = name
        self.grid_size = g
        self.num_control_points = g * g
        self.param_dim = 2 * g * g
        self.interp_method = interp_method
        self.differentiable = bool(differentiable)
        self.out_size = (int(out_size[0]), int(out_size[1]))
        self.num_pixels = self.out_size[0] * self.out_size[1]
        linv = _tps_linv(g)                       # ValueError for g > VSTAB_TPS_GMAX
        runtime._require_gpu()
        self.L_inv = torch.from_numpy(linv).to(torch.device("cuda", torch.cuda.current_device()))

    def _theta(self, theta, B=None):
        theta = _f32_cuda(theta.to(torch.float32), "theta").reshape(-1)
        if theta.numel() % self.param_dim or (B is not None and theta.numel() != B * self.param_dim) or theta.numel() == 0:
            raise ValueError(f"theta must have shape [{'B' if B is None else B}, {self.param_dim}]")
        if self.L_inv.device != theta.device:
            self.L_inv = self.L_inv.to(theta.device)
        return theta

    def transform(self, inp, theta, forward=True, **kwargs):
        """forward=False gives the same output: the reference computes the same coordinates twice (ST:122-132)."""
        interp = _interp_code(self.interp_method)
        inp = _f32_cuda(inp, "inp")
        B = inp.shape[0]
        theta = self._theta(theta, B)
        if theta.device != inp.device:
            raise ValueError("theta must be on inp's device")
        return _autograd.apply(_elastic_transform_call, _elastic_transform_backward, (inp, theta, self.L_inv),
                               (self.grid_size, *self.out_size, interp), interp == 0 or self.differentiable)

    def transform_coords(self, theta):
        """theta [B, 2*g*g] -> (x_s, y_s), each flat [B*oh*ow]: the normalised source coordinates `transform` samples at (the
        x_s_flat, y_s_flat of ST:140-158), bit for bit -- the same device code computes them; for example the deformation field
        to draw.  Needs no image.  Forward only: the results carry no graph."""
        theta = self._theta(theta.detach())
        B = theta.numel() // self.param_dim
        oh, ow = self.out_size
        x_s = torch.empty(B * oh * ow, dtype=torch.float32, device=theta.device)
        y_s = torch.empty_like(x_s)
        runtime.call(theta.device, "vstab_st_elastic_coords", theta.data_ptr(), B, self.grid_size, self.L_inv.data_ptr(), oh, ow,
                     x_s.data_ptr(), y_s.data_ptr())
        return x_s, y_s


# ---------------------------------------------------------------------------------------------------- the 3-D volume transformer
def _out_size3(out_size):
    if len(out_size) != 3:
        raise ValueError("out_size must be (depth, height, width)")
    return int(out_size[0]), int(out_size[1]), int(out_size[2])


def _vol5(vol, name):
    vol = _f32_cuda(vol, name)
    if vol.dim() != 5:
        raise ValueError(f"{name} must be [B,D,H,W,C]")
    return vol


def _meshgrid3d(out_size, device=None):
    """Flat [4*D*H*W] sampling grid: linspace(-1,1,W) as x (fastest), linspace(-1,1,H) as y, linspace(-1,1,D) as z (slowest), ones."""
    runtime._require_gpu()
    od, oh, ow = _out_size3(out_size)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    out = torch.empty(4 * od * oh * ow, dtype=torch.float32, device=dev)
    runtime.call(dev, "vstab_st3d_meshgrid", out.data_ptr(), od, oh, ow)
    return out


def _bilinear_interp3d_call(vol, x, y, z, out_size, edge_size):
    B, D, H, W, Cc = vol.shape
    od, oh, ow = out_size
    out = torch.empty((B * od * oh * ow, Cc), dtype=torch.float32, device=vol.device)
    runtime.call(vol.device, "vstab_st3d_bilinear_interp", vol.data_ptr(), B, D, H, W, Cc, x.data_ptr(), y.data_ptr(), z.data_ptr(), od, oh, ow,
                 edge_size, out.data_ptr())
    return out


def _bilinear_interp3d_backward(saved, dout, needs, statics):
    out_size, edge_size = statics
    return training.st3d_bilinear_interp_backward(*saved, dout, out_size, edge_size=edge_size, need_vol=needs[0], need_x=needs[1],
                                                  need_y=needs[2], need_z=needs[3])


def bilinear_interp3d(vol, x, y, z, out_size, edge_size=1):
    """vol [B,D,H,W,C]; x, y, z flat [B*od*oh*ow] normalised to [-1,1]; out_size = (od, oh, ow) -> [B*od*oh*ow, C].
    The volume is zero-padded by edge_size voxels (never materialised); coordinates are clipped to [-edge_size, n-1+edge_size].
    Differentiable with respect to vol, x, y and z (module docstring)."""
    vol = _vol5(vol, "vol")
    B = vol.shape[0]
    out_size = _out_size3(out_size)
    edge_size = int(edge_size)
    if edge_size < 0:
        raise ValueError("edge_size must be >= 0")
    nvox = B * out_size[0] * out_size[1] * out_size[2]
    x, y, z = (_f32_cuda(t.to(torch.float32), n).reshape(-1) for t, n in ((x, "x"), (y, "y"), (z, "z")))
    if x.numel() != nvox or y.numel() != nvox or z.numel() != nvox:
        raise ValueError(f"x/y/z must have B*out_d*out_h*out_w = {nvox} elements")
    return _autograd.apply(_bilinear_interp3d_call, _bilinear_interp3d_backward, (vol, x, y, z), (out_size, edge_size))


def _interpolate3d(vol, x, y, z, out_size, method='bilinear'):
    return bilinear_interp3d(vol, x, y, z, out_size)            # `method` is ignored, as in the reference (:795)


def _volume_transform_call(inp, theta, out_size):
    B, D, H, W, Cc = inp.shape
    od, oh, ow = out_size
    out = torch.empty((B, od, oh, ow, Cc), dtype=torch.float32, device=inp.device)
    runtime.call(inp.device, "vstab_st3d_transform", inp.data_ptr(), B, D, H, W, Cc, theta.data_ptr(), out.data_ptr(), od, oh, ow)
    return out


def _volume_transform_backward(saved, dout, needs, statics):
    (out_size,) = statics
    d_inp, d_theta = training.st3d_transform_backward(*saved, dout, out_size, need_vol=needs[0], need_theta=needs[1])
    return d_inp, _flat(d_theta)


class AffineVolumeTransformer(object):
    """theta [B,12] = row-major 3x4 matrix acting on (x_t, y_t, z_t, 1), each in [-1,1]; out_size = (depth, height, width).
    inp [B,D,H,W,C] -> [B,od,oh,ow,C], sampled by bilinear_interp3d with edge_size = 1 whatever `interp_method` says (the
    reference ignores it, :794-795).  `transform` is differentiable with respect to the volume and theta."""
    param_dim = 12

    def __init__(self, out_size, name='SpatialAffineVolumeTransformer', interp_method='bilinear', **kwargs):
        self.name = name
        self.out_size = _out_size3(out_size)
        self.interp_method = interp_method
        self._grid = None

    @property
    def voxel_grid(self):
        if self._grid is None:
            self._grid = _meshgrid3d(self.out_size)
        return self._grid

    def transform(self, inp, theta):
        inp = _vol5(inp, "inp")
        B = inp.shape[0]
        theta = _f32_cuda(theta.to(torch.float32), "theta").reshape(-1)
        if theta.numel() != B * self.param_dim:
            raise ValueError(f"theta must have shape [{B}, {self.param_dim}]")
        return _autograd.apply(_volume_transform_call, _volume_transform_backward, (inp, theta), (self.out_size,))


def transformer(inp, theta, out_size, name='SpatialTransformer', **kwargs):
    """Legacy wrapper (:34-38).  The reference passes `out_size` to `transform`, which does not take
    it (a TypeError there); here the call does what the wrapper evidently means.  `differentiable` (and `interp_method`) among the
    keywords go to AffineTransformer."""
    return AffineTransformer(out_size, **kwargs).transform(inp, theta)
